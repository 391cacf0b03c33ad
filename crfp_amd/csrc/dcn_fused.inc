// The 32 -> 216 offset / mask head (model/CRFP.py:337-340) and dcn_g8 in ONE kernel on gfx950: the heaviest kernel of a clip.
//
// The head used to write 199 MB of offsets and masks that dcn_g8 read straight back (28 % of the clip for the pair).  The conv's
// accumulator layout already is the sampler's: lane = pixel, lane half = 4 deformable groups.  With the cout rows packed in
// ST_DCNFUSE order (crfp_common.h) every lane half receives the (dy, dx, mask) of its 36 sampling positions as accumulator slot
// 3 p + c of 7 cout tiles x 16 registers, in the order the sampler consumes them; the values go from the conv's registers through
// tanh / sigmoid into the coordinate arithmetic and never touch memory.  Workgroup = NW rows x 32 pixels (one wave per row, as
// dcn_g8_pipe_kernel); the offset feature's halo tile ((NW + 2) x 34 pixels, all 32 channels) and the DCN weight image stay in LDS
// for the workgroup's life, the conv weights stream through LDS stages (registers -> LDS, next stage's loads in flight under the
// MFMAs).  After cout tile T the sampling pairs it completed run (2-3 of the 18); the last pair's gathers stay in flight under tile
// T+1's MFMAs.
//
// The kernel is written once.  What the two storage builds do differently -- the tile's element type and LDS layout, the stage
// structure, the operand loads and MFMAs, how a cout tile's raw sums leave the accumulators, the schedule table and the number of
// sampling pairs in flight -- is the `#ifndef CRFP_ACT_BF16 ... #else ... #endif` block of macros in front of it.
//  * fp32 storage (f16x3): the halo tile holds both fp16 parts of the SRC_S3 image, the weights stream through one 18 KB stage per
//    (cout tile, 16-channel chunk).  Same arithmetic in the same order as conv3x3_split_kernel<1,1,2> + dcn_g8_pipe_kernel: the
//    results are bit-identical to the two-kernel path.  LDS 81 408 B (NW = 4, two workgroups per CU) / 155 008 B (NW = 8, shipped).
//  * bf16 storage: the offset feature arrives as bf16 Q4 (8-byte quads): its halo tile is copied into LDS as 16-byte elements of
//    8 channels (13 KB), the head's bf16 weights stream one WHOLE cout tile per stage (both 16-channel chunks, 18 KB, one barrier
//    pair per 18 MFMAs), one v_mfma_f32_32x32x16_bf16 per (tap, chunk) into ONE accumulator that starts at the bias -- the
//    arithmetic of conv3x3_bf16_kernel in the same order, so the clip is bit-identical to the two-kernel path here too.  A corner
//    pair of the sampler is one dwordx4 (24 registers per sampling pair), so three pairs are in flight instead of two.
//
// The kernel's issue order is pinned by hand (sched_barrier / sched_group_barrier): csrc/Makefile compiles gather.hip without a
// scheduling strategy.  The lab library's extras (fp32 build only) are in dcn_fused_lab.inc.
//
// Included by gather.hip inside namespace CRFP_NS, behind dcn_g8_pipe_kernel, and not a translation unit of its own: on its own the
// fp32 kernels come out the same, but bf16 dcn_g8_pipe_kernel, left alone in its module with the sampler helpers, is scheduled differently.
#if defined(CRFP_LAB) && defined(CRFP_ACT_BF16)
#error "the lab library links the product's bf16 objects: there is no bf16 lab build of this file"
#endif

constexpr int DF_LW = 34;   // halo tile width: 32 pixels + one column either side

// Round 5, late prologue (the 8-wave form): only what the first MFMA needs -- the halo tile and weight stage 0 -- is
// fetched in front of the first barrier.  The DCN weight image (36 KB, first used by the sampler's MFMAs behind stage 1's barrier) and weight
// stage 1 used to be ingested there too: 153 KB per workgroup before any MFMA, four rounds per launch.  They are now requested BEHIND the
// first barrier and land during cout tile 0, which has no sampler work to hide anyway (fp32: DF_BEGIN(0, 1); bf16: DF_LATE_FILL).  Same
// values in the same places before their first use: bit-identical.
// (PS: the DCN weight image is fetched once per workgroup, in front of the tile loop.)

__device__ __forceinline__ void df_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ================================================================ what the two storage builds do differently
// All DF_* macros expand inside dcn_fused_kernel and name its locals.
#ifndef CRFP_ACT_BF16
constexpr int DF_WCH = 9 * 2 * 64;                   // one (cout tile, chunk) of the fp16 pair image, 16-byte elements
typedef f32x4 df_tile_t;                             // tile element as loaded: 8 channels of one fp16 part
// chunks per weight stage: NW = 8 stages a whole cout tile (7 barriers per workgroup)
#define DF_STAGE_CONSTS constexpr int CPS = DB ? 2 : 1, DF_WST = CPS * DF_WCH, NSTG = 14 / CPS;
#define DF_TILE_LDS __shared__ f32x4 tile[8][DF_NEL];   // [part * 4 + 8-channel group][halo pixel]: x0 planes, then x1s planes
// per tile: the low conv accumulator, two sampling pairs, the operands of the next tap (round 5), one blended pair
#define DF_TILE_STATE f32x16 cl; DcnPair Q0, Q1; dcn_f16x8 pw0, pw1, pb0, pb1; float xs[8];
// the offset feature's halo tile of tile (TX, TY, NN) into rt[] (clamped addresses; what lies outside the image is zeroed on the way to LDS)
#define DF_TLOAD(TX, TY, NN)                                                                              \
    {                                                                                                     \
        const f32x4* __restrict__ s3_ = reinterpret_cast<const f32x4*>(a.feat + (long long)(NN) * a.feat_b); \
        _Pragma("unroll") for (int t = 0; t < DF_NIN; ++t) {                                              \
            const int idc = min(ltid + NT * t, 8 * DF_NEL - 1);                                           \
            const int pl = idc / DF_NEL, pix = idc - pl * DF_NEL, r = pix / DF_LW, c = pix - r * DF_LW;   \
            const int gy = (TY) + r - 1, gx = (TX) + c - 1;                                               \
            rt[t] = s3_[((long long)pl * H + min(max(gy, 0), H - 1)) * W + min(max(gx, 0), W - 1)];       \
        }                                                                                                 \
    }
#define DF_TWRITE(TX, TY)                                                                                 \
    _Pragma("unroll") for (int t = 0; t < DF_NIN; ++t) {                                                  \
        const int idx = ltid + NT * t;                                                                    \
        const int pl = idx / DF_NEL, pix = idx - pl * DF_NEL, r = pix / DF_LW, c = pix - r * DF_LW;       \
        const int gy = (TY) + r - 1, gx = (TX) + c - 1;                                                   \
        const bool tv = gy >= 0 && gy < H && gx >= 0 && gx < W;                                           \
        if (idx < 8 * DF_NEL) (&tile[0][0])[idx] = tv ? rt[t] : f32x4{0.0f, 0.0f, 0.0f, 0.0f};            \
    }
// one (cout tile, chunk) stage = DF_BEGIN (weights registers -> LDS, next stage's loads) + 9 taps x 3 MFMAs (DF_TAPS)
// single buffer: barrier (everyone done with the previous stage), registers -> LDS, barrier, next stage's loads.
// double buffer: one barrier (stage s complete in buffer s & 1 and everyone done with stage s - 1), then the registers
// (stage s + 1) go to the other buffer and stage s + 2's loads leave.  LATE: stage 0 only requests stage 1 and the DCN weight image
// behind its barrier; they are written to LDS at the chunk boundary of cout tile 0 (DF_BEGIN(0, 1)), where stage 2's loads leave.
#define DF_BEGIN(T, CH)                                                                                   \
    if (CPS == 2 && (CH) == 1) {                                                                          \
        wcur = &wst[(T) & 1][DF_WCH];                                                                     \
        if (LATE && (T) == 0) {                                                                           \
            DF_WRITE(1)                                                                                   \
            if (LATE_WL) {                                                                                \
                _Pragma("unroll") for (int k = 0; k < DF_NWL; ++k)                                        \
                    if (tid + NT * k < 36 * 64) wl[tid + NT * k] = rwl[k];                                \
            }                                                                                             \
            DF_WLOAD(2)                                                                                   \
            __builtin_amdgcn_sched_barrier(0);                                                            \
        }                                                                                                 \
    } else {                                                                                              \
        constexpr int s_ = (2 * (T) + (CH)) / CPS;                                                        \
        const bool first_ = s_ == 0;                                                                      \
        if (first_ || !(DF_PROBE & 4)) df_lds_barrier();                                                  \
        if (DB && LATE && first_) {                                                                       \
            DF_WLOAD(1)                                                                                   \
            if (LATE_WL) {                                                                                \
                _Pragma("unroll") for (int k = 0; k < DF_NWL; ++k)                                        \
                    rwl[k] = reinterpret_cast<const f32x4*>(a.wdcn)[min(tid + NT * k, 36 * 64 - 1)];      \
            }                                                                                             \
        } else if (DB) {                                                                                  \
            if (s_ + 1 < NSTG) { DF_WRITE((s_ + 1) & 1) }                                                 \
            if (s_ + 2 < NSTG) { DF_WLOAD(s_ + 2) }                                                       \
        } else {                                                                                          \
            if (first_ || !(DF_PROBE & 12)) { DF_WRITE(0) }                                               \
            if (first_ || !(DF_PROBE & 4)) df_lds_barrier();                                              \
            if (s_ + 1 < NSTG && !(DF_PROBE & 12)) { DF_WLOAD(s_ + 1) }                                   \
        }                                                                                                 \
        __builtin_amdgcn_sched_barrier(0);   /* the next stage's loads leave before this stage's MFMAs */  \
        wcur = &wst[DB ? (s_ & 1) : 0][0];                                                                \
    }
// Round 5: the operands of the NEXT tap are read from LDS before the current tap's MFMAs (one register set ahead: +16 VGPRs, 234 -> 250).
// hipcc had placed every tap's four ds_read_b128 directly in front of its MFMAs behind s_waitcnt lgkmcnt(0 / 1): one exposed LDS round trip
// per tap on a kernel with two waves per SIMD (378 conv MFMAs per wave).  The whole-tile weight stage of the 8-wave form holds both chunks,
// so the prefetch runs across the chunk boundary; the first tap of a cout tile (behind the stage barrier) loads its own operands.  Same
// operations on the same values in the same order: bit-identical.
// Round 5: the scheduling region (sampler item + tap) is laid out as 4 DS reads, then 3 x (1 MFMA, DF_SGB vector instructions) with
// sched_group_barrier, so that the sampler's vector work sits INSIDE each MFMA's shadow instead of in front of a burst of three MFMAs
// (gaps of one instruction between MFMAs: 196 -> 60; same-box 131.2 -> 128.4 us, bit-identical; 10 per MFMA: the same; GAP 3 / 7 / 9 / 12
// of the generated schedule: 130.0 / 128.8 / 131.8 / 139.4, profiles/r05_dcn_fused_sgb_ab.txt).
// The lab build has no operand prefetch: it carries a run-time probe word in this kernel, and with the 16 prefetch registers on top it
// spills (96 B, 255 us).
#ifndef CRFP_LAB
#define DF_SGB 6   // vector instructions per MFMA shadow
#define DF_TAP_PIPELINE                                                                                   \
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);                                                \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, DF_SGB, 0); \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, DF_SGB, 0); \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, DF_SGB, 0);
#define DF_LDOPS(W0, W1, B0, B1, WB, CH_, TAP_)                                                           \
    {                                                                                                     \
        const int ky_ = (TAP_) / 3, kx_ = (TAP_) - 3 * ky_;                                               \
        const int pix_ = (wave + ky_) * DF_LW + j + kx_;                                                  \
        W0 = __builtin_bit_cast(dcn_f16x8, (WB)[((TAP_) * 2) * 64 + lane]);                               \
        W1 = __builtin_bit_cast(dcn_f16x8, (WB)[((TAP_) * 2 + 1) * 64 + lane]);                           \
        B0 = __builtin_bit_cast(dcn_f16x8, tile[2 * (CH_) + h][pix_]);                                    \
        B1 = __builtin_bit_cast(dcn_f16x8, tile[4 + 2 * (CH_) + h][pix_]);                                \
    }
#define DF_TAPS(CH, TA, TB)                                                                               \
    if (!(DF_PROBE & 2))                                                                                  \
    _Pragma("unroll") for (int tap = (TA); tap < (TB); ++tap) {                                           \
        dcn_f16x8 w0, w1, b0, b1;                                                                         \
        const bool have_ = CPS == 2 ? !((CH) == 0 && tap == 0) : tap != 0;   /* prefetched by the tap before */ \
        if (have_) { w0 = pw0; w1 = pw1; b0 = pb0; b1 = pb1; }                                            \
        else DF_LDOPS(w0, w1, b0, b1, wcur, CH, tap)                                                      \
        if (DF_PROBE & 32) { /* lab probe: no operand reads after a tile's first tap (results wrong) */ }  \
        else if ((DF_PROBE & 64) && tap < 8) { /* lab probe: weights only (no activation reads) */         \
            pw0 = __builtin_bit_cast(dcn_f16x8, wcur[((tap + 1) * 2) * 64 + lane]);                       \
            pw1 = __builtin_bit_cast(dcn_f16x8, wcur[((tap + 1) * 2 + 1) * 64 + lane]);                   \
        }                                                                                                 \
        else if (tap < 8) DF_LDOPS(pw0, pw1, pb0, pb1, wcur, CH, tap + 1)                                 \
        else if (CPS == 2 && (CH) == 0) DF_LDOPS(pw0, pw1, pb0, pb1, wcur + DF_WCH, 1, 0)                 \
        cl = __builtin_amdgcn_mfma_f32_32x32x16_f16(w0, b1, cl, 0, 0, 0);                                 \
        ca = __builtin_amdgcn_mfma_f32_32x32x16_f16(w0, b0, ca, 0, 0, 0);                                 \
        cl = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1, b0, cl, 0, 0, 0);                                 \
        DF_TAP_PIPELINE                                                                                   \
    }
#else
#define DF_TAPS(CH, TA, TB)                                                                               \
    if (!(DF_PROBE & 2))                                                                                  \
    _Pragma("unroll") for (int tap = (TA); tap < (TB); ++tap) {                                           \
        const int ky = tap / 3, kx = tap - 3 * ky;                                                        \
        const dcn_f16x8 w0 = __builtin_bit_cast(dcn_f16x8, wcur[(tap * 2) * 64 + lane]);                  \
        const dcn_f16x8 w1 = __builtin_bit_cast(dcn_f16x8, wcur[(tap * 2 + 1) * 64 + lane]);              \
        const int pix = (wave + ky) * DF_LW + j + kx;                                                     \
        const dcn_f16x8 b0 = __builtin_bit_cast(dcn_f16x8, tile[2 * (CH) + h][pix]);                      \
        const dcn_f16x8 b1 = __builtin_bit_cast(dcn_f16x8, tile[4 + 2 * (CH) + h][pix]);                  \
        cl = __builtin_amdgcn_mfma_f32_32x32x16_f16(w0, b1, cl, 0, 0, 0);                                 \
        ca = __builtin_amdgcn_mfma_f32_32x32x16_f16(w0, b0, ca, 0, 0, 0);                                 \
        cl = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1, b0, cl, 0, 0, 0);                                 \
    }
#endif
#define DF_CL_ZERO _Pragma("unroll") for (int e = 0; e < 16; ++e) cl[e] = 0.0f;   // DF_BIAS: the low accumulator starts at zero
// end of cout tile T: the raw sums go to ov[] (the accumulators are free for tile T + 1); 10 tanh + flow / sigmoid follow
// in place, inside the first taps of tile T + 1
#define DF_RAW(T)                                                                                         \
    {                                                                                                     \
        _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                  \
            const int sl = 16 * (T) + e;                                                                  \
            if (sl < 108) {                                                                               \
                /* = ca + cl * 2^-11 as the two-kernel path forms it (the product is exact), in one instruction */ \
                ov[sl] = __builtin_fmaf(cl[e], 1.0f / 2048.0f, ca[e]);                                    \
            }                                                                                             \
        }                                                                                                 \
    }
// micro-items of the round-3 schedule (dcn_fused_schedule.inc): a quarter of a tile's activations, one position's coordinates +
// gathers, one position's blend, one pair's split + DCN MFMAs
#define DF_TR(T, Q)                                                                                       \
    {                                                                                                     \
        _Pragma("unroll") for (int e = 4 * (Q); e < 4 * (Q) + 4; ++e) {                                   \
            const int sl = 16 * (T) + e;                                                                  \
            if (sl < 108)                                                                                 \
                ov[sl] = sl % 3 == 0 ? tanh10_plus(ov[sl], cfy) : (sl % 3 == 1 ? tanh10_plus(ov[sl], cfx) : fast_sigmoid(ov[sl])); \
        }                                                                                                 \
    }
#define DF_I1(U, PI, P)                                                                                   \
    if (!(DF_PROBE & 1)) {                                                                                \
        dcn_issue_one(P, PI, rx, ov[6 * (U) + 3 * (PI)] * pz, ov[6 * (U) + 3 * (PI) + 1] * pz, ov[6 * (U) + 3 * (PI) + 2], 2 * (U) + (PI), \
                      fy0, fx0, fH, fW, PW, pitch, plane_b, hbase);                                       \
    }
#define DF_L(U, PI, P) if (!(DF_PROBE & 1)) { dcn_lerp_one(P, PI, xs); }
#define DF_S(U) if (!(DF_PROBE & 1)) { dcn_split_mfma(xs, acc, acl, wl, U, lane); }
// HBM bytes per pixel given to ProfScope: SRC_S3 feature, flow, sampled planes, output
constexpr double kFusedBytesPerPixel = 32 * 4.0 + 8.0 + (32 + 32) * sizeof(act_t);

#else   // ---------------------------------------------------------------- bf16 storage
constexpr int DF_WST = 2 * 9 * 64;                   // one cout tile of the bf16 image, 16-byte elements
typedef __bf16 df_bf16x8 __attribute__((ext_vector_type(8)));
typedef cu32x2 df_tile_t;                            // tile element as loaded: one 8-byte quad
#define DF_STAGE_CONSTS
#define DF_TILE_LDS __shared__ cu32x2 tile[4][DF_NEL][2];   // [8-channel group][halo pixel][quad of the pair]
// per tile: three sampling pairs, the operands of the next MFMA (round 5)
#define DF_TILE_STATE DcnPair Q0, Q1, Q2; df_bf16x8 pw0, pb0;
#define DF_TLOAD(TX, TY, NN)                                                                              \
    {                                                                                                     \
        const cu32x2* __restrict__ fq_ = reinterpret_cast<const cu32x2*>(as_act(a.feat) + (long long)(NN) * a.feat_b); \
        _Pragma("unroll") for (int t = 0; t < DF_NIN; ++t) {                                              \
            const int idc = min(ltid + NT * t, 8 * DF_NEL - 1);                                           \
            const int q = idc / DF_NEL, pix = idc - q * DF_NEL, r = pix / DF_LW, c = pix - r * DF_LW;     \
            const int gy = (TY) + r - 1, gx = (TX) + c - 1;                                               \
            rt[t] = fq_[((long long)q * H + min(max(gy, 0), H - 1)) * W + min(max(gx, 0), W - 1)];        \
        }                                                                                                 \
    }
#define DF_TWRITE(TX, TY)                                                                                 \
    _Pragma("unroll") for (int t = 0; t < DF_NIN; ++t) {                                                  \
        const int idx = ltid + NT * t;                                                                    \
        const int q = idx / DF_NEL, pix = idx - q * DF_NEL, r = pix / DF_LW, c = pix - r * DF_LW;         \
        const int gy = (TY) + r - 1, gx = (TX) + c - 1;                                                   \
        const bool tv = gy >= 0 && gy < H && gx >= 0 && gx < W;                                           \
        if (idx < 8 * DF_NEL) tile[q >> 1][pix][q & 1] = tv ? rt[t] : cu32x2{0u, 0u};                     \
    }
// single buffer: barrier (everyone done with the previous stage), registers -> LDS, barrier, next stage's loads.
// double buffer: one barrier (stage T complete in buffer T & 1 and everyone done with stage T - 1), then the registers
// (stage T + 1) go to the other buffer and stage T + 2's loads leave.  LATE: stage 0 only requests stage 1 and the DCN weight image
// behind its barrier; DF_LATE_FILL writes them to LDS in the middle of cout tile 0, where stage 2's loads leave.
#define DF_LATE_FILL                                                                                      \
    if (LATE) {                                                                                           \
        DF_WRITE(1)                                                                                       \
        if (LATE_WL) {                                                                                    \
            _Pragma("unroll") for (int k = 0; k < DF_NWL; ++k)                                            \
                if (tid + NT * k < 36 * 64) wl[tid + NT * k] = rwl[k];                                    \
        }                                                                                                 \
        DF_WLOAD(2)                                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                \
    }
#define DF_BEGIN(T)                                                                                       \
    {                                                                                                     \
        df_lds_barrier();                                                                                 \
        if (DB && LATE && (T) == 0) {                                                                     \
            DF_WLOAD(1)                                                                                   \
            if (LATE_WL) {                                                                                \
                _Pragma("unroll") for (int k = 0; k < DF_NWL; ++k)                                        \
                    rwl[k] = reinterpret_cast<const f32x4*>(a.wdcn)[min(tid + NT * k, 36 * 64 - 1)];      \
            }                                                                                             \
        } else if (DB) {                                                                                  \
            if ((T) + 1 < 7) { DF_WRITE(((T) + 1) & 1) }                                                  \
            if ((T) + 2 < 7) { DF_WLOAD((T) + 2) }                                                        \
        } else {                                                                                          \
            DF_WRITE(0)                                                                                   \
            df_lds_barrier();                                                                             \
            if ((T) + 1 < 7) { DF_WLOAD((T) + 1) }                                                        \
        }                                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        wcur = &wst[DB ? ((T) & 1) : 0][0];                                                               \
    }
// MFMAs MA .. MB-1 of the cout tile's 18 (chunk-major, then taps: the K order of conv3x3_bf16_kernel)
// Round 5: MFMA m + 1's two operands are read from LDS before MFMA m issues (one register set ahead, +8 VGPRs; the fp32 build's DF_TAPS
// has the measurement).  The first MFMA of a cout tile (behind the stage barrier) loads its own.  Same operations, same order: bit-identical.
#define DF_LDOPS(W0, B0, M_)                                                                              \
    {                                                                                                     \
        const int ch_ = (M_) / 9, tap_ = (M_) - 9 * ch_, ky_ = tap_ / 3, kx_ = tap_ - 3 * ky_;            \
        const int pix_ = (wave + ky_) * DF_LW + j + kx_;                                                  \
        W0 = __builtin_bit_cast(df_bf16x8, wcur[(M_) * 64 + lane]);                                       \
        B0 = __builtin_bit_cast(df_bf16x8, *reinterpret_cast<const f32x4*>(&tile[2 * ch_ + h][pix_][0])); \
    }
#define DF_M(MA, MB)                                                                                      \
    _Pragma("unroll") for (int m = (MA); m < (MB); ++m) {                                                 \
        df_bf16x8 w0, b0;                                                                                 \
        if (m != 0) { w0 = pw0; b0 = pb0; }                                                               \
        else DF_LDOPS(w0, b0, m)                                                                          \
        if (m + 1 < 18) DF_LDOPS(pw0, pb0, m + 1)                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        ca = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, b0, ca, 0, 0, 0);                                \
    }
#define DF_CL_ZERO   // one accumulator
#define DF_RAW(T)                                                                                         \
    {                                                                                                     \
        _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                  \
            const int sl = 16 * (T) + e;                                                                  \
            if (sl < 108) ov[sl] = ca[e];                                                                 \
        }                                                                                                 \
    }
// HBM bytes per pixel given to ProfScope: flow, bf16 feature, sampled planes, output
constexpr double kFusedBytesPerPixel = 8.0 + (32 + 32 + 32) * sizeof(act_t);
#endif

// ================================================================ what they share
#define DF_DECODE(T_, TX, TY, NN)                                                                         \
    {                                                                                                     \
        const int per_ = tiles_x * tiles_y, n_ = (T_) / per_, r_ = (T_) - n_ * per_, y_ = r_ / tiles_x;   \
        NN = n_; TY = y_ * NW; TX = (r_ - y_ * tiles_x) * 32;                                             \
    }
// weight stage ST into rws[]; rws[] (a stage) into LDS buffer B
#define DF_WLOAD(ST)                                                                                      \
    _Pragma("unroll") for (int k = 0; k < DF_NWS; ++k) rws[k] = wc[(ST) * DF_WST + min(ltid + NT * k, DF_WST - 1)];
#define DF_WRITE(B)                                                                                       \
    _Pragma("unroll") for (int k = 0; k < DF_NWS; ++k) {                                                  \
        const int idx = ltid + NT * k;                                                                    \
        if (idx < DF_WST) wst[B][idx] = rws[k];                                                           \
    }
// prologue: the head's 224 packed biases into LDS (NW = 8) or 4 VGPRs (NW = 4); the sampled P4 planes' pitches and the image size
#define DF_BIAS_FILL                                                                                     \
    float bv[4];   /* NW = 4: no LDS left for the bias table */                                           \
    if (DB && tid0 < 56) bl[tid0] = reinterpret_cast<const f32x4*>(a.bconv)[tid0];                        \
    _Pragma("unroll") for (int k = 0; k < 4; ++k) bv[k] = DB ? 0.0f : a.bconv[min(64 * k + (tid0 & 63), 223)];
#define DF_GEOMETRY                                                                                       \
    const long long plane = (long long)H * W * 4;                                                         \
    const int PW = W + 1, pitch = PW * QB, plane_b = (H + 1) * pitch;                                     \
    const int guard = pitch + QB;                                                                         \
    const float fH = (float)H, fW = (float)W;
// the accumulators of cout tile T start at its bias, as in the two-kernel path: the 224 packed biases sit in 4 VGPRs
// (lane L holds rows L, 64 + L, ...) and each value arrives through v_readlane -- scalar loads here cost a cache-miss
// round trip per cout tile and quad (28 per wave, a third of the kernel's fixed cost when measured), per-lane vector
// loads would drain the gathers in flight
#define DF_BIAS(T)                                                                                        \
    if (DB) {   /* four ds_read_b128 of the lane half's quads (lgkmcnt: the gathers in flight are not waited for) */ \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                   \
            const f32x4 bq = bl[(T) * 8 + 2 * q + h];                                                     \
            ca[4 * q] = bq.x; ca[4 * q + 1] = bq.y; ca[4 * q + 2] = bq.z; ca[4 * q + 3] = bq.w;           \
        }                                                                                                 \
    } else {                                                                                              \
        _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                  \
            const int r0 = 32 * (T) + 8 * (e >> 2) + (e & 3), r1 = r0 + 4;                                \
            const float s0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bv[r0 >> 6]), r0 & 63)); \
            const float s1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bv[r1 >> 6]), r1 & 63)); \
            ca[e] = h ? s1 : s0;                                                                          \
        }                                                                                                 \
    }                                                                                                     \
    DF_CL_ZERO
// the activations of cout tile T's raw sums, in place: 10 tanh + flow for (dy, dx), sigmoid for the mask
#define DF_TRANS(T)                                                                                       \
    {                                                                                                     \
        _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                  \
            const int sl = 16 * (T) + e;                                                                  \
            if (sl < 108)                                                                                 \
                ov[sl] = sl % 3 == 0 ? tanh10_plus(ov[sl], cfy) : (sl % 3 == 1 ? tanh10_plus(ov[sl], cfx) : fast_sigmoid(ov[sl])); \
        }                                                                                                 \
    }
#define DF_SB __builtin_amdgcn_sched_barrier(0);
// sampling pair U: coordinates + gathers into P; blend, split and DCN MFMAs out of P
#define DF_I(U, P)                                                                                        \
    if (!(DF_PROBE & 1)) {                                                                                \
        dcn_issue_one(P, 0, rx, ov[6 * (U)] * pz, ov[6 * (U) + 1] * pz, ov[6 * (U) + 2], 2 * (U), fy0, fx0, fH, fW, PW, pitch, plane_b, hbase); \
        dcn_issue_one(P, 1, rx, ov[6 * (U) + 3] * pz, ov[6 * (U) + 4] * pz, ov[6 * (U) + 5], 2 * (U) + 1, fy0, fx0, fH, fW, PW, pitch, plane_b, hbase); \
    }
#define DF_C(U, P)                                                                                        \
    if (!(DF_PROBE & 1)) { dcn_consume_pair(P, acc, acl, wl, U, lane); }
// (PS) hooks in the schedule's tail (behind the last conv MFMA, where rt, rws, the conv accumulators and the operand prefetch registers are
// dead).  DF_TAIL_REQUEST, behind the last gather issue: the next tile's halo tile and weight stage 0 are requested (no gather queues behind
// them in the in-order vmcnt).  DF_TAIL_COMMIT, behind the last DCN MFMA: one barrier (every wave is past its last conv operand read), then
// they go to LDS -- the next tile's first barrier publishes them.  Their registers never live across the loop's back edge.
#define DF_TAIL_REQUEST                                                                                   \
    if (PS) {                                                                                             \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        DF_DECODE(has_next ? t_cur + t_step : t_cur, ntx0, nty0, nn)                                      \
        DF_TLOAD(ntx0, nty0, nn) DF_WLOAD(0)                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                \
    }
#define DF_TAIL_COMMIT                                                                                    \
    if (PS && has_next) {                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        df_lds_barrier();                                                                                 \
        DF_TWRITE(ntx0, nty0) DF_WRITE(0)                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                \
    }

// The warp plan (DcnWarpPlan) of a one-tile launch: workgroups [tiles, tiles + M) of its 1-D grid, M = the CUs its last round leaves without a
// tile (launch_dcn_fused).  Workgroups are handed out in index order, so these start only when every tile has a CU: they fill the hole and never
// displace a tile.  Warp workgroup g of M walks the band's 64-pixel row segments -- (batch item, row, segment), wave-uniform -- wave by wave in a
// grid-stride loop, DF_WARP_U segments per trip: such a CU holds these 8 waves and nothing else (the kernel's LDS and registers allow one
// workgroup), so the load latency is covered inside the thread, not by occupancy -- 4 flow reads, then 16 corner loads (fp32) per thread, 128 KB
// of gathers in flight per CU.  Per pixel it is flow_warp_p4_kernel's program (flow_warp_p4_pixels): the same bits.
constexpr int DF_WARP_U = 4;
__device__ __forceinline__ void df_warp_tail(const DcnWarpPlan& p, int N, int g, int M, int tid) {
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int segs_x = (p.W8 + 63) >> 6, per = segs_x * (p.y1 - p.y0), total = per * N, step = 8 * M;
    for (int s0 = 8 * g + wave; s0 < total; s0 += DF_WARP_U * step) {
        int n[DF_WARP_U], px[DF_WARP_U], py[DF_WARP_U];
        bool st[DF_WARP_U];
#pragma unroll
        for (int u = 0; u < DF_WARP_U; ++u) {
            const int s = s0 + u * step, sc = min(s, total - 1);   // past the end: the last segment again, nothing stored
            const int nn = sc / per, r = sc - nn * per, y = r / segs_x, x = (r - y * segs_x) * 64 + lane;
            n[u] = nn; py[u] = p.y0 + y; px[u] = min(x, p.W8 - 1);
            st[u] = s < total && x < p.W8;
        }
        flow_warp_p4_pixels<DF_WARP_U>(p.src, p.src_b, p.flow, p.flow_b, p.dst, p.dst_b, 1, p.H8, p.W8, n, px, py, st);
    }
}

// NW = 4: workgroup of 4 rows x 32 pixels, two per CU, one weight stage (two barriers per stage).  NW = 8: 8 rows, one workgroup
// per CU, the weight stage double-buffered (one barrier per stage, half the L2 -> LDS weight and DCN-image traffic per pixel).
// PS (round 6): the PERSISTENT form.  gridDim.x workgroups (one per CU) walk the tile list of the whole launch (all batch items), XCD x
// taking the contiguous band x of it (xcd_band_tile's split).  The DCN weight image, the bias table and the kernel's registers are set up
// once per workgroup instead of once per tile; the NEXT tile's halo tile and weight stage 0 are requested in the schedule's tail behind the
// last gather issue (their registers -- rt, rws -- are dead there; nothing queues behind them in the in-order vmcnt) and go to LDS behind one
// barrier behind the last DCN MFMA, so only the first tile of a workgroup pays the 116 KB prologue in front of its first MFMA.  Same per-pixel
// operations in the same order: bit-identical.  Used for launches of >= 6 rounds of the chip (launch_dcn_fused); below that the one-tile form
// (PS = false, the same XCD-banded tile order) is 1-1.5 % faster (profiles/r06_dcn_fused_persistent_ab.txt).
template <int NW, bool PS = false>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void dcn_fused_kernel(const DcnFuseArgs a) {
    constexpr int NT = 64 * NW, DF_NEL = (NW + 2) * DF_LW;   // halo tile of an NW x 32-pixel workgroup
    constexpr int DF_NIN = (8 * DF_NEL + NT - 1) / NT;       // tile elements per thread
    constexpr bool DB = NW == 8;
    static_assert(!PS || DB, "the persistent form is the 8-wave form");
    DF_STAGE_CONSTS
    constexpr int DF_NWS = (DF_WST + NT - 1) / NT;
    DF_TILE_LDS
    __shared__ f32x4 wst[DB ? 2 : 1][DF_WST];
    __shared__ f32x4 wl[36 * 64];
    __shared__ f32x4 bl[DB ? 56 : 1];   // the head's 224 packed biases (NW = 8: LDS has room; NW = 4 keeps them in 4 VGPRs)
    const int tid0 = threadIdx.x;
    const int H = a.H, W = a.W;
    // the tile list (PS): tile id = (n * tiles_y + ty) * tiles_x + tx; this workgroup takes t_cur, t_cur + t_step, ... below t_end
    const int tiles_x = (W + 31) >> 5, tiles_y = (H + NW - 1) / NW;
    int t_cur = 0, t_end = 0, t_step = 1;
    if (PS) {
        const int total = tiles_x * tiles_y * a.N, G = (int)gridDim.x;
        const int q = total >> 3, r = total & 7, x = (int)blockIdx.x & 7;
        const int band0 = x * q + min(x, r);
        t_cur = band0 + ((int)blockIdx.x >> 3); t_end = band0 + q + (x < r ? 1 : 0); t_step = G >> 3;
        if (t_cur >= t_end) return;
    }
    int tx0, ty0, n;
    if (PS) DF_DECODE(t_cur, tx0, ty0, n)
    else if (DB) {   // the one-tile form: a 1-D grid that walks the tile list in the XCD-banded order too; the workgroups behind the tiles carry the warp plan
        const int ntiles_ = tiles_x * tiles_y * a.N;
        if ((int)blockIdx.x >= ntiles_) {
            df_warp_tail(a.warp, a.N, (int)blockIdx.x - ntiles_, (int)gridDim.x - ntiles_, tid0);
            return;
        }
        const int tb_ = xcd_band_tile((int)blockIdx.x, ntiles_);
        DF_DECODE(tb_, tx0, ty0, n)
    }
    else { tx0 = blockIdx.x * 32; ty0 = blockIdx.y * NW; n = blockIdx.z; }

    int ltid = tid0;  // the thread id as the tile loop sees it: re-defined (opaquely) per tile in the persistent form, so that everything derived
                      // from it (lane / wave / LDS addresses / the loaders' index math) is recomputed where it is used instead of being hoisted
                      // out of the tile loop into long-lived registers -- the kernel has none to spare
    df_tile_t rt[DF_NIN];
    DF_TLOAD(tx0, ty0, n)
    const f32x4* __restrict__ wc = reinterpret_cast<const f32x4*>(a.wconv);
    f32x4 rws[DF_NWS];
    DF_WLOAD(0)
    constexpr bool LATE = DB;   // the late prologue
    static_assert(!PS || LATE, "the persistent form builds on the late prologue");
    constexpr bool LATE_WL = LATE && !PS;   // the DCN weight image rides in rwl through cout tile 0
    constexpr int DF_NWL = (36 * 64 + NT - 1) / NT;
    f32x4 rwl[LATE_WL ? DF_NWL : 1];
    if (!LATE_WL)
        for (int i = tid0; i < 36 * 64; i += NT) wl[i] = reinterpret_cast<const f32x4*>(a.wdcn)[i];
    // the bias table, the sampled planes' geometry, and the halo tile in rt[] (tile at (tx0, ty0)) and weight stage 0 in rws[] on their way to
    // LDS -- the first three in each build's own order: either order moves instructions of the other build's kernel
#ifndef CRFP_ACT_BF16
    DF_BIAS_FILL DF_GEOMETRY DF_TWRITE(tx0, ty0)
#else
    DF_TWRITE(tx0, ty0) DF_GEOMETRY DF_BIAS_FILL
#endif
    if (DB) { DF_WRITE(0) if (!LATE) { DF_WLOAD(1) } }   // stage 0 in LDS (LATE: stage 1 is requested behind the first barrier)

    for (;;) {   // one tile per trip (not PS: one trip)
    if (PS) asm volatile("" : "+v"(ltid));
    const int tid = ltid, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
#ifndef CRFP_ACT_BF16   // (the bf16 build has this line further down: its place moves instructions in either kernel)
    const int hbase = 4 * h * plane_b + guard;
#endif
    const int px = tx0 + j, py = ty0 + wave;
    const bool valid = px < W && py < H;
    const int cx = min(px, W - 1), cy = min(py, H - 1);
    const float2 fl = *reinterpret_cast<const float2*>(a.flow + (long long)n * a.flow_b + ((long long)cy * W + cx) * 2);
    const float cfy = 10.0f + fl.y, cfx = 10.0f + fl.x;
    int ntx0 = 0, nty0 = 0, nn = 0;   // (PS) the workgroup's next tile
    const bool has_next = PS && t_cur + t_step < t_end;

    // sampler set-up (dcn_g8_pipe_kernel)
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        (char*)const_cast<act_t*>(as_act(a.x) + (long long)n * a.xb) - guard, 0, 8 * plane_b + guard, 0x00020000);
    const float fy0 = (float)(cy - 1), fx0 = (float)(cx - 1);
#ifdef CRFP_ACT_BF16
    const int hbase = 4 * h * plane_b + guard;
#endif

    f32x16 acc, acl, ca;
#pragma unroll
    for (int e = 0; e < 16; ++e) { acc[e] = 0.0f; acl[e] = 0.0f; }
#ifdef CRFP_LAB
    const int DF_PROBE = a.probe;   // timing experiments (results wrong), bits: 1 = no sampling, 2 = no conv MFMAs, 4 = no barriers / weight streaming after stage 0, 8 = barriers but no weight streaming, 32 = conv MFMAs without operand reads, 64 = weight reads only
    const float pz = (DF_PROBE & 16) ? 0.0f : 1.0f;   // 16: zero offsets = regular, coalesced sampling positions
#else
    constexpr int DF_PROBE = 0;
    constexpr float pz = 1.0f;
#endif
    float ov[108];   // activated (dy, dx, mask) of position p at 3 p + c; every index below is a compile-time constant
    DF_TILE_STATE
    const f32x4* wcur = &wst[0][0];

#ifdef CRFP_ACT_BF16
    // cout tile T completes the sampling pairs up to (16 T + 10) / 6: 1, 4, 7, 9, 12, 15, 17; they are sampled inside tile T + 1.
    // Pair u lives in Q[u % 3]; I(u) follows C(u - 3).
    DF_BEGIN(0) DF_BIAS(0) DF_M(0, 9) DF_LATE_FILL DF_M(9, 18) DF_RAW(0)   // (the bias table in LDS is complete behind the first barrier)
    DF_BIAS(1)
    DF_BEGIN(1) DF_M(0, 6) DF_TRANS(0) DF_SB DF_M(6, 12) DF_I(0, Q0) DF_SB DF_M(12, 18) DF_I(1, Q1) DF_SB DF_RAW(1)
    DF_BIAS(2)
    DF_BEGIN(2) DF_M(0, 4) DF_TRANS(1) DF_SB DF_M(4, 8) DF_I(2, Q2) DF_SB DF_M(8, 12) DF_SB DF_C(0, Q0) DF_SB DF_M(12, 15) DF_I(3, Q0) DF_SB
                DF_M(15, 18) DF_SB DF_C(1, Q1) DF_SB DF_I(4, Q1) DF_SB DF_RAW(2)
    DF_BIAS(3)
    DF_BEGIN(3) DF_M(0, 3) DF_TRANS(2) DF_SB DF_M(3, 6) DF_SB DF_C(2, Q2) DF_SB DF_M(6, 9) DF_I(5, Q2) DF_SB DF_M(9, 12) DF_SB DF_C(3, Q0) DF_SB
                DF_M(12, 15) DF_I(6, Q0) DF_SB DF_M(15, 18) DF_SB DF_C(4, Q1) DF_SB DF_I(7, Q1) DF_SB DF_RAW(3)
    DF_BIAS(4)
    DF_BEGIN(4) DF_M(0, 4) DF_TRANS(3) DF_SB DF_M(4, 8) DF_SB DF_C(5, Q2) DF_SB DF_M(8, 12) DF_I(8, Q2) DF_SB DF_M(12, 15) DF_SB DF_C(6, Q0) DF_SB
                DF_M(15, 18) DF_I(9, Q0) DF_SB DF_C(7, Q1) DF_SB DF_RAW(4)
    DF_BIAS(5)
    DF_BEGIN(5) DF_M(0, 4) DF_TRANS(4) DF_SB DF_M(4, 8) DF_I(10, Q1) DF_SB DF_M(8, 12) DF_SB DF_C(8, Q2) DF_SB DF_M(12, 15) DF_I(11, Q2) DF_SB
                DF_M(15, 18) DF_SB DF_C(9, Q0) DF_SB DF_I(12, Q0) DF_SB DF_RAW(5)
    DF_BIAS(6)
    DF_BEGIN(6) DF_M(0, 3) DF_TRANS(5) DF_SB DF_M(3, 6) DF_SB DF_C(10, Q1) DF_SB DF_M(6, 9) DF_I(13, Q1) DF_SB DF_M(9, 12) DF_SB DF_C(11, Q2) DF_SB
                DF_M(12, 15) DF_I(14, Q2) DF_SB DF_M(15, 18) DF_SB DF_C(12, Q0) DF_SB DF_I(15, Q0) DF_SB DF_RAW(6)
    DF_TRANS(6) DF_SB DF_C(13, Q1) DF_SB DF_I(16, Q1) DF_SB DF_C(14, Q2) DF_SB DF_I(17, Q2) DF_SB DF_TAIL_REQUEST DF_C(15, Q0) DF_SB DF_C(16, Q1) DF_SB DF_C(17, Q2) DF_TAIL_COMMIT
#else
    // Round 3: ONE micro-item in front of EVERY tap instead of whole pairs between groups of 2-4 taps (tools/gen/dcn_fused_schedule.py
    // holds the dependency rules and writes the table): <= ~30 vector instructions per 3 MFMAs, the regime in which
    // tools/micro/mfma_valu_overlap2 shows the vector work disappearing in the MFMA gaps.  Same operations on the same values in
    // the same per-accumulator order: bit-identical to the round-2 table it replaced and to the two-kernel path.
#include "dcn_fused_schedule.inc"
#endif
    if (valid) {
        DCN_G8_EPILOGUE(a.out, a.ob, a.bdcn, a.ovf, a.ovf_div)
    }
    if (!has_next) break;
    t_cur += t_step;
    tx0 = ntx0; ty0 = nty0; n = nn;
    }   // tiles
}

#ifdef CRFP_LAB
#include "dcn_fused_lab.inc"
#endif

bool dcn_fused_enabled() {
    static const bool on = !(getenv("CRFP_DCN_FUSED") && atoi(getenv("CRFP_DCN_FUSED")) == 0);
    return on;
}

// The CUs of the current device, rounded down to a multiple of 8 (one 8-wave workgroup per CU: 155 KB of LDS, 250 VGPRs; the persistent form
// deals its workgroups to the 8 XCDs evenly): 256 on an MI355X.  Read once per device.  <= 0 with the error set when the device cannot be asked.
static int fused_cus() {
    constexpr int kDevs = 64;
    static std::atomic<int> cus[kDevs];
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kDevs) { set_error("dcn_fused: no current device (hipGetDevice)"); return 0; }
    int v = cus[dev].load(std::memory_order_relaxed);
    if (v == 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess || prop.multiProcessorCount < 8) { set_error("dcn_fused: cannot read the device's CU count"); return 0; }
        v = prop.multiProcessorCount & ~7;
        cus[dev].store(v, std::memory_order_relaxed);
    }
    return v;
}
// launches with at least this many tiles take the persistent form (six rounds of one workgroup per CU); the lab knob overrides (tests)
static int fused_persist_min_tiles(int cus) {
    const int k = CRFP_LAB_KNOB("CRFP_DF_PS_MIN_TILES", 0);
    const int v = k > 0 ? k : 6 * cus;
    return v > cus ? v : cus + 1;
}

DcnFusedGrid dcn_fused_grid(int N, int H, int W) {
    DcnFusedGrid g = {fused_cus(), ((W + 31) / 32) * ((H + 7) / 8) * N, 0, 0};
    if (g.cus <= 0) return g;
    g.persistent = g.tiles >= fused_persist_min_tiles(g.cus);
    const int rem = g.tiles % g.cus;   // tiles of the last round
    if (!g.persistent && rem) g.warp_wgs = g.cus - rem;
    return g;
}

int dcn_fused_tail_wgs(int N, int H, int W) {
#ifdef CRFP_LAB   // the lab-only kernel forms (launch_dcn_fused_lab) take no plan
    if (CRFP_LAB_KNOB("CRFP_DCN_FUSE_NW", 8) != 8 || CRFP_LAB_KNOB("CRFP_DCN_FUSE_V", 1) == 2) return 0;
#endif
    return dcn_fused_grid(N, H, W).warp_wgs;
}

int launch_dcn_fused(const DcnFuseArgs& args, hipStream_t s) {
    if ((long long)(args.H + 1) * (args.W + 1) >= (1ll << 24)) { set_error("dcn_g8: plane of %d x %d exceeds the sampler's 2^24-element index range", args.H, args.W); return CRFP_E_UNSUPPORTED; }
    const DcnWarpPlan& wp = args.warp;
    const int warp_wgs = wp.dst ? dcn_fused_tail_wgs(args.N, args.H, args.W) : 0;
    if (wp.dst) {   // a plan is taken whole or refused: the caller asks dcn_fused_tail_wgs first and keeps its stand-alone warp where that is 0
        if (!warp_wgs) { set_error("dcn_fused: this launch (%d x %d x %d) has no idle last-round CUs for a warp plan", args.N, args.H, args.W); return CRFP_E_UNSUPPORTED; }
        if (!wp.src || !wp.flow || wp.H8 < 1 || wp.W8 < 1 || wp.y0 < 0 || wp.y1 <= wp.y0 || wp.y1 > wp.H8 || (long long)(wp.H8 + 1) * (wp.W8 + 1) >= (1ll << 27)) {   // (32-bit byte offsets)
            set_error("dcn_fused: bad warp plan (rows [%d, %d) of %d x %d)", wp.y0, wp.y1, wp.H8, wp.W8);
            return CRFP_E_BADARG;
        }
    }
    const double px = (double)args.N * args.H * args.W;
    const double wpx = wp.dst ? (double)args.N * (wp.y1 - wp.y0) * wp.W8 : 0.0;   // the band it carries: flow_warp_q4_c4's bytes and flops per pixel
    ProfScope prof("offset_mask_conv+dcnv2_g8_fused", s, px * kFusedBytesPerPixel + wpx * (2.0 * 4 * sizeof(act_t) + 8),
                   2.0 * px * 32 * 216 * 9 + 2.0 * px * 32 * 32 * 9 + px * 288 * 7 + wpx * 4 * 7.0);
#ifdef CRFP_LAB
    DcnFuseArgs a = args;
    if (launch_dcn_fused_lab(a, s)) { CRFP_CHECK_LAUNCH(); return 0; }   // the environment asked for a lab-only form
#else
    const DcnFuseArgs& a = args;
#endif
    // 8-wave workgroups: per launch same-box against <4>, 151.6 vs 165.3 us (fp32) and 91.9 vs 97.0 us (bf16, one clip)
    // Round 6: both forms walk the tile list in the XCD-banded order (HBM traffic 170 -> 112-116 MB per launch @A).  Launches of six rounds of
    // the chip and more (a lock-step batch, the 4K map) take the persistent form (-1 % there, +1.5 % at 3.5 rounds: profiles/r06_dcn_fused_persistent_ab.txt)
    // The one-tile form is a 1-D grid: its tiles, then the workgroups of the warp plan (one per CU the last round leaves idle), if it carries one.
    const DcnFusedGrid g = dcn_fused_grid(a.N, a.H, a.W);
    if (g.cus <= 0) return CRFP_E_UNSUPPORTED;
    if (g.persistent) dcn_fused_kernel<8, true><<<dim3(g.cus, 1, 1), 512, 0, s>>>(a);
    else dcn_fused_kernel<8><<<dim3(g.tiles + warp_wgs, 1, 1), 512, 0, s>>>(a);
    CRFP_CHECK_LAUNCH();
    return 0;
}
