// Lab-only part of conv_mfma.hip (included there under CRFP_LAB, after the shipped main loops): the conv main loops that lost their A/B against
// the shipped ones -- software-pipelined persistent (pipe), input-stationary (is), warp-specialised (ws) -- the environment knobs that select them, and their dispatch (launch_conv_lab, called once by launch_conv_mfma).  Never in the product.

// ---------------------------------------------------------------- software-pipelined persistent variant (f16x3)
// One 512-thread workgroup per CU (two waves per SIMD) walks a strided list of 8x64 output tiles; wave = one output
// row (two 32-pixel MFMA column tiles).  The work is a stream of items (tile, K-chunk).  LDS holds TWO items (halo tile
// images 2 x 42 KB + weight fragments 2 x 18 KB); the registers hold two more in raw fp32 form.  While the MFMAs of
// item s run out of LDS buffer s&1 the same waves
//   * issue the global loads of item s+2 (a full item of latency budget; measured wait at use: 16 cycles),
//   * split item s+1 (loaded during item s-1) into its two fp16 images and write them + its weights to buffer (s+1)&1,
// slice by slice between the taps: the MFMA is asynchronous (32 cycles per 32x32x16), so VALU/LDS instructions
// issued between two of them ride in its shadow.  The code between two barriers is branch-free (every thread
// writes both of its halo slots; surplus threads hit a dummy slot), otherwise the scheduler cannot interleave.
// One barrier per item; accumulators start at the bias; the epilogue runs when a tile's last chunk is done.
// History: the first version (bf16x6, 4 waves) needed 6.9 k cycles per item against 3.5 k of MFMA -- LDS operand traffic
// (0.75 ds_read_b128 per MFMA = 93 % of the LDS pipe) and in-order issue behind a full LDS queue with one wave per
// SIMD; 8 waves fixed the issue stalls but bf16x6 stayed LDS-bound (7.9 k per item).  f16x3 moves 2/3 of the bytes.
// Barrier that orders LDS traffic only.  __syncthreads() is a workgroup-scope release fence + s_barrier, and the release
// makes hipcc wait for vmcnt(0): every wave then sits out the write-acknowledge latency of its epilogue stores (2.5-3.3 k
// cycles per item measured) although nobody in the workgroup reads them.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

constexpr int PIPE_NW = 8, PIPE_NT = 64 * PIPE_NW;
constexpr int PIPE_NEL = (PIPE_NW + 2) * LW;                   // 660 halo pixels
constexpr int PIPE_WPC = 9 * 2 * 64;                           // weight vectors per (cout tile, chunk), f16x3
constexpr int PIPE_NWS = (PIPE_WPC + PIPE_NT - 1) / PIPE_NT;   // 3 weight vectors per thread

struct PipeRegs {
    f32x4 q[4][2];        // [K-quad of the chunk][halo element of this thread]
    bf16x8 w[PIPE_NWS];   // this thread's share of the chunk's 18 KB weight fragment image
    int m[4];             // component masks of the 4 quads (wave-uniform)
    bool ok[2];           // halo element inside the image
};

__device__ __forceinline__ void pipe_issue(PipeRegs& R, const ConvArgs& a, const bf16x8* __restrict__ wp, int n, int T0,
                                           int nchunks, int ch, int tx0, int ty0, int tid) {
    const int H = a.H, W = a.W;
    const int ns = a.src_bgroup > 0 ? n + n / a.src_bgroup : n;   // source batch item (ConvArgs::src_bgroup)
    int cgy[2], cgx[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int idx = min(tid + PIPE_NT * t, PIPE_NEL - 1);
        const int r = idx / LW, c = idx - r * LW;
        const int gy = ty0 + r - 1, gx = tx0 + c - 1;
        R.ok[t] = tid + PIPE_NT * t < PIPE_NEL && gy >= 0 && gy < H && gx >= 0 && gx < W;
        cgy[t] = min(max(gy, 0), H - 1);
        cgx[t] = min(max(gx, 0), W - 1);
    }
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) {
        const QuadDesc d = a.qd[4 * ch + qi];
        const float* qb = d.base + (long long)ns * d.bstride;
        R.m[qi] = d.mask;
#pragma unroll
        for (int t = 0; t < 2; ++t) R.q[qi][t] = *reinterpret_cast<const f32x4*>(qb + cgy[t] * d.rs + cgx[t] * d.cs);
    }
#pragma unroll
    for (int k = 0; k < PIPE_NWS; ++k)
        R.w[k] = wp[(long long)(T0 * nchunks + ch) * PIPE_WPC + min(tid + PIPE_NT * k, PIPE_WPC - 1)];
}

// unit U in 0..3: halo element U>>1, quad pair U&1 -> two fp16x8 images.  Slot PIPE_NEL is a dummy.
template <int U>
__device__ __forceinline__ void pipe_split_unit(const PipeRegs& R, bf16x8 (*tl)[2][PIPE_NEL + 1], int tid) {
    constexpr int t = U >> 1, pr = U & 1;
    const int idx = min(tid + PIPE_NT * t, PIPE_NEL);
    bf16x8 p0, p1;
    split_f16x8(mask_quad(R.q[2 * pr][t], R.ok[t] ? R.m[2 * pr] : 0), mask_quad(R.q[2 * pr + 1][t], R.ok[t] ? R.m[2 * pr + 1] : 0),
                p0, p1);
    tl[0][pr][idx] = p0; tl[1][pr][idx] = p1;
}

template <int K>
__device__ __forceinline__ void pipe_put_weight(const PipeRegs& R, bf16x8* wl, int tid) {
    wl[min(tid + PIPE_NT * K, PIPE_WPC)] = R.w[K];   // slot PIPE_WPC is a dummy
}

__device__ __forceinline__ void pipe_tap(f32x16 (&acc)[1][2], f32x16 (&acl)[1][2], const bf16x8* wl,
                                         const bf16x8 (*tl)[2][PIPE_NEL + 1], int tap, int wave, int lane) {
    const int j = lane & 31, h = lane >> 5;
    const int ky = tap / 3, kx = tap - 3 * ky;
    bf16x8 wa[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) wa[p] = wl[(tap * 2 + p) * 64 + lane];
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
        const int pix = (wave + ky) * LW + pt * 32 + j + kx;
        bf16x8 bq[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) bq[p] = tl[p][h][pix];
        split_mfma<2>(acc[0][pt], acl[0][pt], wa, bq);
    }
}

__global__ __launch_bounds__(PIPE_NT, 1) void conv3x3_split_pipe_kernel(const ConvArgs a) {
    __shared__ bf16x8 tile[2][2][2][PIPE_NEL + 1];   // [buffer][split part][quad pair][halo pixel (+1 dummy)]  84.6 KB
    __shared__ bf16x8 wlds[2][PIPE_WPC + 1];         // [buffer][(tap, part)][lane] (+1 dummy)                   36.9 KB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int tiles_x = (a.W + TW - 1) / TW, ntiles = tiles_x * ((a.H + PIPE_NW - 1) / PIPE_NW);
    const int T0 = blockIdx.y, n = blockIdx.z;
    const int ns = a.src_bgroup > 0 ? n + n / a.src_bgroup : n;   // source batch item (ConvArgs::src_bgroup)
    const int nchunks = a.kq >> 2;
    const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    const int nitems = my_tiles * nchunks;
    const bf16x8* __restrict__ wp = reinterpret_cast<const bf16x8*>(a.wsplit16);
    const EpiCtx ec = epi_ctx(a, n);
    float4 bq4[4];   // this lane's bias quads: the accumulators of every tile start there
#pragma unroll
    for (int g = 0; g < 4; ++g) bq4[g] = reinterpret_cast<const float4*>(a.bpk)[T0 * 8 + 2 * g + h];

    // issue cursor (items are issued two ahead of the one being multiplied)
    int ik = 0, ich = 0;
    PipeRegs RA, RB;
#define CRFP_PIPE_ISSUE(R)                                                                                \
    {                                                                                                     \
        if (ik < my_tiles) {                                                                              \
            const int t_ = blockIdx.x + ik * gridDim.x, ty_ = t_ / tiles_x, tx_ = t_ - ty_ * tiles_x;     \
            pipe_issue(R, a, wp, n, T0, nchunks, ich, tx_ * TW, ty_ * PIPE_NW, tid);                      \
        }                                                                                                 \
        if (++ich == nchunks) { ich = 0; ++ik; }                                                          \
    }
#define CRFP_PIPE_ACC_INIT                                                                                \
    _Pragma("unroll") for (int pt = 0; pt < 2; ++pt)                                                      \
        _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                   \
            acc[0][pt][4 * g + 0] = bq4[g].x; acc[0][pt][4 * g + 1] = bq4[g].y;                           \
            acc[0][pt][4 * g + 2] = bq4[g].z; acc[0][pt][4 * g + 3] = bq4[g].w;                           \
            acl[0][pt][4 * g + 0] = 0.0f; acl[0][pt][4 * g + 1] = 0.0f;                                   \
            acl[0][pt][4 * g + 2] = 0.0f; acl[0][pt][4 * g + 3] = 0.0f;                                   \
        }
    CRFP_PIPE_ISSUE(RA)
    CRFP_PIPE_ISSUE(RB)
    // item 0 -> buffer 0
    pipe_split_unit<0>(RA, tile[0], tid); pipe_split_unit<1>(RA, tile[0], tid);
    pipe_split_unit<2>(RA, tile[0], tid); pipe_split_unit<3>(RA, tile[0], tid);
    pipe_put_weight<0>(RA, wlds[0], tid); pipe_put_weight<1>(RA, wlds[0], tid); pipe_put_weight<2>(RA, wlds[0], tid);
    __syncthreads();

    f32x16 acc[1][2], acl[1][2];
    CRFP_PIPE_ACC_INIT
    int mk = 0, mch = 0;   // item being multiplied

#ifdef CRFP_PIPE_STAMPS
    long long st_wait = 0, st_taps = 0, st_epi = 0, st_bar = 0, st_t = __builtin_amdgcn_s_memtime();
#define CRFP_PST(ACC) { const long long t_ = __builtin_amdgcn_s_memtime(); ACC += t_ - st_t; st_t = t_; }
#else
#define CRFP_PST(ACC)
#endif
    // one item: MFMAs out of LDS buffer BUF; RNEXT (item s+1, landed) is split / copied into buffer BUF^1 between the
    // taps; RFREE (consumed by the previous item) receives the loads of item s+2 first of all
#define CRFP_PIPE_ITEM(BUF, RNEXT, RFREE)                                                                 \
    {                                                                                                     \
        CRFP_PST(st_bar)                                                                                  \
        CRFP_PIPE_ISSUE(RFREE)                                                                            \
        pipe_tap(acc, acl, wlds[BUF], tile[BUF], 0, wave, lane);                                          \
        pipe_split_unit<0>(RNEXT, tile[(BUF) ^ 1], tid);                                                  \
        pipe_tap(acc, acl, wlds[BUF], tile[BUF], 1, wave, lane);                                          \
        pipe_put_weight<0>(RNEXT, wlds[(BUF) ^ 1], tid);                                                  \
        pipe_tap(acc, acl, wlds[BUF], tile[BUF], 2, wave, lane);                                          \
        pipe_split_unit<1>(RNEXT, tile[(BUF) ^ 1], tid);                                                  \
        pipe_tap(acc, acl, wlds[BUF], tile[BUF], 3, wave, lane);                                          \
        pipe_put_weight<1>(RNEXT, wlds[(BUF) ^ 1], tid);                                                  \
        pipe_tap(acc, acl, wlds[BUF], tile[BUF], 4, wave, lane);                                          \
        pipe_split_unit<2>(RNEXT, tile[(BUF) ^ 1], tid);                                                  \
        pipe_tap(acc, acl, wlds[BUF], tile[BUF], 5, wave, lane);                                          \
        pipe_put_weight<2>(RNEXT, wlds[(BUF) ^ 1], tid);                                                  \
        pipe_tap(acc, acl, wlds[BUF], tile[BUF], 6, wave, lane);                                          \
        pipe_split_unit<3>(RNEXT, tile[(BUF) ^ 1], tid);                                                  \
        pipe_tap(acc, acl, wlds[BUF], tile[BUF], 7, wave, lane);                                          \
        pipe_tap(acc, acl, wlds[BUF], tile[BUF], 8, wave, lane);                                          \
        CRFP_PST(st_taps)                                                                                 \
        if (++mch == nchunks) {                                                                           \
            const int t_ = blockIdx.x + mk * gridDim.x, ty_ = t_ / tiles_x, tx_ = t_ - ty_ * tiles_x;     \
            _Pragma("unroll") for (int pt = 0; pt < 2; ++pt)                                              \
                _Pragma("unroll") for (int e = 0; e < 16; ++e) acc[0][pt][e] += acl[0][pt][e] * (1.0f / F16_RES_SCALE); \
            conv_epilogue<1, 2, 1, 2>(ec, acc, T0, tx_ * TW, ty_ * PIPE_NW, wave, j, h);                  \
            CRFP_PIPE_ACC_INIT                                                                            \
            mch = 0; ++mk;                                                                                \
        }                                                                                                 \
        CRFP_PST(st_epi)                                                                                  \
        lds_barrier();     /* buffer BUF^1 complete, every wave done with buffer BUF */                  \
    }

    for (int s = 0; s < nitems; s += 2) {
        CRFP_PIPE_ITEM(0, RB, RA)
        if (s + 1 < nitems) CRFP_PIPE_ITEM(1, RA, RB)
    }
#undef CRFP_PIPE_ITEM
#undef CRFP_PIPE_ISSUE
#undef CRFP_PIPE_ACC_INIT
#ifdef CRFP_PIPE_STAMPS
    if (a.stamps && tid == 0) {
        long long* o = a.stamps + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 8;
        o[0] = st_wait; o[1] = st_taps; o[2] = st_epi; o[3] = st_bar; o[4] = nitems;
    }
    if (a.stamps && lane == 0 && blockIdx.x == 3) {   // per-wave view of one workgroup
        long long* o = a.stamps + (8192 + wave) * 8;
        o[0] = st_wait; o[1] = st_taps; o[2] = st_epi; o[3] = st_bar; o[4] = nitems;
    }
#endif
}

// ---------------------------------------------------------------- input-stationary variant (short K, many couts)
// For convolutions whose whole K fits in LDS (Cin <= 32: the 32->216 offset/mask conv, the pixel-shuffle
// expanders 32->96 / 24->64 / 32->64) the halo tile is staged and split ONCE per workgroup and the
// workgroup then walks all cout tiles, streaming only the packed weights (27 KB per (cout tile, chunk),
// prefetched into registers during the previous step's MFMAs).  The regular kernel re-stages the same
// input once per cout tile and pays its prologue/epilogue bubble 7x for the 216-channel conv.
template <int NCH, int NWAVES, int NP>
__global__ __launch_bounds__(64 * NWAVES, NWAVES == 4 ? 2 : 1) void conv3x3_split_is_kernel(const ConvArgs a) {
    constexpr int RPW = 1, TH = NWAVES, LH = TH + 2, PT = 2, NT = 64 * NWAVES;
    constexpr int NEL = LH * LW;
    constexpr int NIN = (NEL + NT - 1) / NT;
    constexpr int WPC = 9 * NP * 64;
    constexpr int NWS = (WPC + NT - 1) / NT;
    __shared__ bf16x8 tile[NCH][NP][2][NEL];
    __shared__ bf16x8 wlds[WPC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int tiles_x = (a.W + TW - 1) / TW;
    const int btile = xcd_band_tile(blockIdx.x, gridDim.x);   // XCD x works on a contiguous band of tiles
    const int tx0 = (btile % tiles_x) * TW, ty0 = (btile / tiles_x) * TH;
    const int n = blockIdx.z;
    const int ns = a.src_bgroup > 0 ? n + n / a.src_bgroup : n;   // source batch item (ConvArgs::src_bgroup)
    const int H = a.H, W = a.W;
    const bf16x8* __restrict__ wp = reinterpret_cast<const bf16x8*>(NP == 3 ? a.wsplit : a.wsplit16);
    const int nsteps = a.ctiles * NCH;

    bf16x8 rws[NWS];
#define CRFP_IS_WLOAD(STEP)                                                                               \
    _Pragma("unroll") for (int k = 0; k < NWS; ++k)                                                       \
        rws[k] = wp[(long long)(STEP) * WPC + min(tid + NT * k, WPC - 1)];
    CRFP_IS_WLOAD(0)   // (cout tile 0, chunk 0): packed index (T*nchunks + ch)*WPC == step*WPC

    // ---- stage + split the whole input tile once
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        f32x4 rq[4][NIN];
        int msk[4];
        bool ok[NIN];
#pragma unroll
        for (int qi = 0; qi < 4; ++qi) {
            const QuadDesc d = a.qd[4 * ch + qi];
            const float* qb = d.base + (long long)ns * d.bstride;
            msk[qi] = d.mask;
#pragma unroll
            for (int t = 0; t < NIN; ++t) {
                const int idx = min(tid + NT * t, NEL - 1);
                const int r = idx / LW, c = idx - r * LW;
                const int gy = ty0 + r - 1, gx = tx0 + c - 1;
                ok[t] = tid + NT * t < NEL && gy >= 0 && gy < H && gx >= 0 && gx < W;
                rq[qi][t] = *reinterpret_cast<const f32x4*>(qb + min(max(gy, 0), H - 1) * d.rs + min(max(gx, 0), W - 1) * d.cs);
            }
        }
#pragma unroll
        for (int t = 0; t < NIN; ++t) {
            const int idx = tid + NT * t;
            if (idx < NEL) {
                bf16x8 pp[NP];
                split_parts<NP>(mask_quad(rq[0][t], ok[t] ? msk[0] : 0), mask_quad(rq[1][t], ok[t] ? msk[1] : 0), pp);
#pragma unroll
                for (int p = 0; p < NP; ++p) tile[ch][p][0][idx] = pp[p];
                split_parts<NP>(mask_quad(rq[2][t], ok[t] ? msk[2] : 0), mask_quad(rq[3][t], ok[t] ? msk[3] : 0), pp);
#pragma unroll
                for (int p = 0; p < NP; ++p) tile[ch][p][1][idx] = pp[p];
            }
        }
    }

    long long tA = 0, tB = 0, tC = 0, tD = 0, t0 = __builtin_amdgcn_s_memtime();
    if (a.stamps) { const long long t = __builtin_amdgcn_s_memtime(); tA += t - t0; t0 = t; }
    f32x16 acc[1][PT], acl[1][PT];
    const EpiCtx ec = epi_ctx(a, n);
    float2 flpre[PT];   // flow of this lane's pixels (ST_OFFMASK): loaded here, not between two epilogues' stores
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
        const int y = min(ty0 + wave * RPW + (pt >> 1), H - 1), x = min(tx0 + (pt & 1) * 32 + j, W - 1);
        flpre[pt] = a.store == ST_OFFMASK ? *reinterpret_cast<const float2*>(ec.flp + ((long long)y * W + x) * 2)
                                          : make_float2(0.0f, 0.0f);
    }
    for (int step = 0; step < nsteps; ++step) {
        const int ch = step % NCH, ct = step / NCH;
        if (ch == 0) {
#pragma unroll
            for (int pt = 0; pt < PT; ++pt)
#pragma unroll
                for (int e = 0; e < 16; ++e) { acc[0][pt][e] = 0.0f; acl[0][pt][e] = 0.0f; }
        }
        __syncthreads();  // all waves done with the previous step's weights (and, first time, tile staged)
#pragma unroll
        for (int k = 0; k < NWS; ++k) {
            const int idx = tid + NT * k;
            if (idx < WPC) wlds[idx] = rws[k];
        }
        __syncthreads();
        if (a.stamps) { const long long t = __builtin_amdgcn_s_memtime(); tB += t - t0; t0 = t; }
        if (step + 1 < nsteps) { CRFP_IS_WLOAD(step + 1) }
#pragma unroll kTapUnroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - 3 * ky;
            bf16x8 wa[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) wa[p] = wlds[(tap * NP + p) * 64 + lane];
#pragma unroll
            for (int pt = 0; pt < PT; ++pt) {
                const int pix = (wave * RPW + (pt >> 1) + ky) * LW + (pt & 1) * 32 + j + kx;
                bf16x8 bq[NP];
#pragma unroll
                for (int p = 0; p < NP; ++p) bq[p] = tile[ch][p][h][pix];
                split_mfma<NP>(acc[0][pt], acl[0][pt], wa, bq);
            }
        }
        if (a.stamps) { const long long t = __builtin_amdgcn_s_memtime(); tD += t - t0; t0 = t; }
        if (ch == NCH - 1) {
            if (NP == 2) {
#pragma unroll
                for (int pt = 0; pt < PT; ++pt)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[0][pt][e] += acl[0][pt][e] * (1.0f / F16_RES_SCALE);
            }
            conv_epilogue<1, PT, RPW, 0>(ec, acc, ct, tx0, ty0, wave, j, h, flpre);
        }
        if (a.stamps) { const long long t = __builtin_amdgcn_s_memtime(); tC += t - t0; t0 = t; }
    }
    if (a.stamps && tid == 0) {
        long long* o = a.stamps + (long long)blockIdx.x * 4;
        o[0] = tA; o[1] = tB; o[2] = tC; o[3] = tD;
    }
#undef CRFP_IS_WLOAD
}

// ================================================================ warp-specialised split-bf16 convolution
// Measured on the single-role kernels above (s_memtime stamps): the MFMA phase is only 40-50 % of a
// block's life; the rest is (a) the fp32->3xbf16 split + LDS write of the next chunk, which cannot
// overlap the MFMAs of the same waves, and (b) vmcnt being in-order on CDNA: a wave that has epilogue
// stores in flight must drain them before it can consume a prefetched load (12k cycles per cout tile
// in the 216-channel conv).  Here the roles are split:
//   * 8 compute waves (one output row of 64 px each, 2 per SIMD) only ever read LDS, issue MFMAs and
//     fire their epilogue stores -- they never wait on vmcnt inside the main loop;
//   * 4 loader waves (one per SIMD) own every global load: they fetch the next chunk's halo tile (fp32)
//     and packed weights, split the activations into 3 bf16 images and write them into the OTHER half
//     of a double-buffered LDS tile while the compute waves run the current chunk.
// Two workgroup barriers per chunk: X = compute done with the weight image / loaders done with the next
// tile, Y = weight image of this chunk visible.  Weights (27 KB per chunk) are single-buffered: the
// loaders hold them in registers and copy them in between X and Y (~400 idle compute cycles).
// IS = input-stationary form for Cin <= 32 and many couts: both LDS tile halves hold the (at most two)
// K-chunks for the whole block and the loop runs over (cout tile, chunk) steps streaming only weights.
constexpr int WS_NC = 8, WS_NL = 8, WS_NT = 64 * (WS_NC + WS_NL), WS_TH = 8, WS_LH = WS_TH + 2, WS_NEL = WS_LH * LW;

template <bool IS>
__global__ __launch_bounds__(WS_NT, 1) void conv3x3_split_ws_kernel(const ConvArgs a) {
    constexpr int NLT = 64 * WS_NL;                       // loader threads
    constexpr int NIN = (WS_NEL + NLT - 1) / NLT;         // halo pixels per loader thread (3)
    constexpr int NWS = (27 * 64 + NLT - 1) / NLT;        // weight vectors per loader thread (7)
    __shared__ bf16x8 tile[2][3][2][WS_NEL];
    __shared__ bf16x8 wlds[27 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_x = (a.W + TW - 1) / TW;
    const int tx0 = (blockIdx.x % tiles_x) * TW, ty0 = (blockIdx.x / tiles_x) * WS_TH;
    const int n = blockIdx.z;
    const int ns = a.src_bgroup > 0 ? n + n / a.src_bgroup : n;   // source batch item (ConvArgs::src_bgroup)
    const int H = a.H, W = a.W;
    const int nchunks = a.kq >> 2;
    const int T0 = IS ? 0 : blockIdx.y;
    const int nsteps = IS ? a.ctiles * nchunks : nchunks;   // IS: step = ct*nchunks + ch

    if (wave >= WS_NC) {
        // ------------------------------------------------------------ loader role
        const int lt = tid - 64 * WS_NC;
        const bf16x8* __restrict__ wp = reinterpret_cast<const bf16x8*>(a.wsplit);
        int cgy[NIN], cgx[NIN];
        bool sval[NIN];
#pragma unroll
        for (int t = 0; t < NIN; ++t) {
            const int idx = min(lt + NLT * t, WS_NEL - 1);
            const int r = idx / LW, c = idx - r * LW;
            const int gy = ty0 + r - 1, gx = tx0 + c - 1;
            sval[t] = lt + NLT * t < WS_NEL && gy >= 0 && gy < H && gx >= 0 && gx < W;
            cgy[t] = min(max(gy, 0), H - 1);
            cgx[t] = min(max(gx, 0), W - 1);
        }
        // Loader schedule, two register sets (A, B): right after barrier Y(s) the loads of chunk s+2 are
        // issued into the set that was just consumed, THEN the other set (chunk s+1, issued a whole step
        // earlier) is split and written to the idle tile half.  Every load is unconditional (chunk index
        // clamped) so that the in-order vmcnt counts are compile-time constants and the compiler can wait
        // for "all but the loads just issued" instead of vmcnt(0).
        f32x4 qa0[NIN], qa1[NIN], qa2[NIN], qa3[NIN], qb0[NIN], qb1[NIN], qb2[NIN], qb3[NIN];
        bf16x8 wa_[NWS], wb_[NWS];
        int ma0 = 0, ma1 = 0, ma2 = 0, ma3 = 0, mb0 = 0, mb1 = 0, mb2 = 0, mb3 = 0;
#define CRFP_WS_LOAD_IN(R0, R1, R2, R3, M0, M1, M2, M3, CH)                                               \
        {                                                                                                 \
            const QuadDesc d0 = a.qd[4 * (CH)], d1 = a.qd[4 * (CH) + 1], d2 = a.qd[4 * (CH) + 2],         \
                           d3 = a.qd[4 * (CH) + 3];                                                       \
            const float* b0 = d0.base + (long long)ns * d0.bstride;                                        \
            const float* b1 = d1.base + (long long)ns * d1.bstride;                                        \
            const float* b2 = d2.base + (long long)ns * d2.bstride;                                        \
            const float* b3 = d3.base + (long long)ns * d3.bstride;                                        \
            M0 = d0.mask; M1 = d1.mask; M2 = d2.mask; M3 = d3.mask;                                       \
            _Pragma("unroll") for (int t = 0; t < NIN; ++t) {                                             \
                R0[t] = *reinterpret_cast<const f32x4*>(b0 + cgy[t] * d0.rs + cgx[t] * d0.cs);            \
                R1[t] = *reinterpret_cast<const f32x4*>(b1 + cgy[t] * d1.rs + cgx[t] * d1.cs);            \
                R2[t] = *reinterpret_cast<const f32x4*>(b2 + cgy[t] * d2.rs + cgx[t] * d2.cs);            \
                R3[t] = *reinterpret_cast<const f32x4*>(b3 + cgy[t] * d3.rs + cgx[t] * d3.cs);            \
            }                                                                                             \
        }
#define CRFP_WS_LOAD_W(RW, WSTEP)                                                                         \
        _Pragma("unroll") for (int k = 0; k < NWS; ++k)                                                   \
            RW[k] = wp[(long long)(WSTEP) * 1728 + min(lt + NLT * k, 1727)];
#define CRFP_WS_WRITE_IN(R0, R1, R2, R3, M0, M1, M2, M3, BUF)                                             \
        _Pragma("unroll") for (int t = 0; t < NIN; ++t) {                                                 \
            const int idx = lt + NLT * t;                                                                 \
            if (idx < WS_NEL) {                                                                           \
                bf16x8 p0, p1, p2;                                                                        \
                split_bf16x8(mask_quad(R0[t], sval[t] ? M0 : 0), mask_quad(R1[t], sval[t] ? M1 : 0), p0, p1, p2); \
                tile[BUF][0][0][idx] = p0; tile[BUF][1][0][idx] = p1; tile[BUF][2][0][idx] = p2;          \
                split_bf16x8(mask_quad(R2[t], sval[t] ? M2 : 0), mask_quad(R3[t], sval[t] ? M3 : 0), p0, p1, p2); \
                tile[BUF][0][1][idx] = p0; tile[BUF][1][1][idx] = p1; tile[BUF][2][1][idx] = p2;          \
            }                                                                                             \
        }
#define CRFP_WS_WRITE_W(RW)                                                                               \
        _Pragma("unroll") for (int k = 0; k < NWS; ++k) {                                                 \
            const int idx = lt + NLT * k;                                                                 \
            if (idx < 1728) wlds[idx] = RW[k];                                                            \
        }
        // packed weight image of (cout tile T, chunk ch) starts at ((T*nchunks + ch)*27)*64 vectors
        const long long wbase = (long long)T0 * nchunks;
        const int last = nsteps - 1, lastc = nchunks - 1;
        if (IS) {
            CRFP_WS_LOAD_IN(qa0, qa1, qa2, qa3, ma0, ma1, ma2, ma3, 0)
            CRFP_WS_LOAD_W(wa_, wbase)
            CRFP_WS_WRITE_IN(qa0, qa1, qa2, qa3, ma0, ma1, ma2, ma3, 0)
            if (nchunks > 1) {
                CRFP_WS_LOAD_IN(qa0, qa1, qa2, qa3, ma0, ma1, ma2, ma3, 1)
                CRFP_WS_WRITE_IN(qa0, qa1, qa2, qa3, ma0, ma1, ma2, ma3, 1)
            }
            for (int step = 0; step < nsteps; ++step) {
                __syncthreads();  // X
                CRFP_WS_WRITE_W(wa_)
                __syncthreads();  // Y
                CRFP_WS_LOAD_W(wa_, wbase + min(step + 1, last))
            }
        } else {
            CRFP_WS_LOAD_IN(qa0, qa1, qa2, qa3, ma0, ma1, ma2, ma3, 0)
            CRFP_WS_LOAD_W(wa_, wbase)
            CRFP_WS_LOAD_IN(qb0, qb1, qb2, qb3, mb0, mb1, mb2, mb3, min(1, lastc))
            CRFP_WS_LOAD_W(wb_, wbase + min(1, last))
            CRFP_WS_WRITE_IN(qa0, qa1, qa2, qa3, ma0, ma1, ma2, ma3, 0)
            // top of an even step s: tile[s&1] = chunk s, wa_ = weights(s), set B = chunk s+1 (in flight)
            long long sA = 0, sB = 0, sC = 0, sD = 0, t0 = __builtin_amdgcn_s_memtime();
#define CRFP_ST(ACC) if (a.stamps) { const long long t_ = __builtin_amdgcn_s_memtime(); ACC += t_ - t0; t0 = t_; }
            for (int step = 0; step < nsteps; step += 2) {
                __syncthreads();  // X: compute done with wlds and with tile[(step+1)&1]
                CRFP_ST(sD)
                CRFP_WS_WRITE_W(wa_)
                __syncthreads();  // Y
                CRFP_ST(sC)
                CRFP_WS_LOAD_IN(qa0, qa1, qa2, qa3, ma0, ma1, ma2, ma3, min(step + 2, lastc))
                CRFP_WS_LOAD_W(wa_, wbase + min(step + 2, last))
                CRFP_ST(sA)
                if (step + 1 >= nsteps) break;
                CRFP_WS_WRITE_IN(qb0, qb1, qb2, qb3, mb0, mb1, mb2, mb3, (step + 1) & 1)
                CRFP_ST(sB)
                __syncthreads();  // X
                CRFP_ST(sD)
                CRFP_WS_WRITE_W(wb_)
                __syncthreads();  // Y
                CRFP_ST(sC)
                CRFP_WS_LOAD_IN(qb0, qb1, qb2, qb3, mb0, mb1, mb2, mb3, min(step + 3, lastc))
                CRFP_WS_LOAD_W(wb_, wbase + min(step + 3, last))
                CRFP_ST(sA)
                if (step + 2 < nsteps) CRFP_WS_WRITE_IN(qa0, qa1, qa2, qa3, ma0, ma1, ma2, ma3, step & 1)
                CRFP_ST(sB)
            }
            if (a.stamps && lt == 0) {
                long long* o = a.stamps + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 4 + 4 * 8192;
                o[0] = sA; o[1] = sB; o[2] = sC; o[3] = sD;
            }
#undef CRFP_ST
        }
#undef CRFP_WS_LOAD_IN
#undef CRFP_WS_LOAD_W
#undef CRFP_WS_WRITE_IN
#undef CRFP_WS_WRITE_W
        return;
    }

    // ---------------------------------------------------------------- compute role: wave = output row
    const int j = lane & 31, h = lane >> 5;
    f32x16 acc[1][2];
    const EpiCtx ec = epi_ctx(a, n);
    float2 flpre[2] = {make_float2(0.0f, 0.0f), make_float2(0.0f, 0.0f)};
    if (a.store == ST_OFFMASK) {
        const int y = min(ty0 + wave, H - 1);
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
            flpre[pt] = *reinterpret_cast<const float2*>(a.flow + (long long)n * a.flow_bstride +
                                                         ((long long)y * W + min(tx0 + pt * 32 + j, W - 1)) * 2);
    }
    long long tA = 0, tB = 0, tC = 0, tD = 0, t0 = __builtin_amdgcn_s_memtime();
    for (int step = 0; step < nsteps; ++step) {
        const int ch = IS ? step % nchunks : step;
        const int buf = IS ? ch : (step & 1);
        if (!IS ? step == 0 : ch == 0) {
#pragma unroll
            for (int pt = 0; pt < 2; ++pt)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[0][pt][e] = 0.0f;
        }
        __syncthreads();  // X
        if (a.stamps) { const long long t = __builtin_amdgcn_s_memtime(); tA += t - t0; t0 = t; }
        __syncthreads();  // Y
        if (a.stamps) { const long long t = __builtin_amdgcn_s_memtime(); tB += t - t0; t0 = t; }
#pragma unroll kTapUnroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - 3 * ky;
            const bf16x8 w0 = wlds[(tap * 3 + 0) * 64 + lane], w1 = wlds[(tap * 3 + 1) * 64 + lane],
                         w2 = wlds[(tap * 3 + 2) * 64 + lane];
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) {
                const int pix = (wave + ky) * LW + pt * 32 + j + kx;
                const bf16x8 b0 = tile[buf][0][h][pix], b1 = tile[buf][1][h][pix], b2 = tile[buf][2][h][pix];
                f32x16 c = acc[0][pt];
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, b1, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, b2, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2, b0, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, b1, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, b0, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, b0, c, 0, 0, 0);
                acc[0][pt] = c;
            }
        }
        if (a.stamps) { const long long t = __builtin_amdgcn_s_memtime(); tD += t - t0; t0 = t; }
        if (IS && ch == nchunks - 1) conv_epilogue<1, 2, 1, 0>(ec, acc, step / nchunks, tx0, ty0, wave, j, h, flpre);
        if (a.stamps) { const long long t = __builtin_amdgcn_s_memtime(); tC += t - t0; t0 = t; }
    }
    if (a.stamps && tid == 0) {
        long long* o = a.stamps + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 4;
        o[0] = tA; o[1] = tB; o[2] = tC; o[3] = tD;
    }
    if (!IS) conv_epilogue<1, 2, 1, 0>(ec, acc, T0, tx0, ty0, wave, j, h, flpre);
}


// ---------------------------------------------------------------- knobs and dispatch
static const char* lab_conv_mode() { const char* m = CRFP_LAB_ENV("CRFP_CONV_MODE"); return m ? m : "f16x3"; }

// SRC_S3 sources / s3_dst need the default selection: conv3x3_split_kernel<1,1,2> / conv3x3_split8_kernel
static bool lab_conv_s3_supported() {
    if (strcmp(lab_conv_mode(), "f16x3")) return false;
    if (CRFP_LAB_KNOB("CRFP_SPLIT_WS", 0) || CRFP_LAB_KNOB("CRFP_SPLIT_IS", 0) || CRFP_LAB_KNOB("CRFP_SPLIT_PIPE", 0)) return false;
    return CRFP_LAB_KNOB("CRFP_SPLIT_RPW", 1) == 1 && CRFP_LAB_KNOB("CRFP_CONV_S3", 1);
}

// The lab library's part of launch_conv_mfma, on the prepared plan: sets the stamp pointer and launches whatever the knobs select instead
// of the shipped kernel.  *done: the conv has been launched.
static int launch_conv_lab(ConvArgs& am, const char* name, bool split, hipStream_t s, bool* done) {
    const ConvArgs& a = am;
    // diagnostic: CRFP_STAMP_PTR=<device address> CRFP_STAMP_NAME=<launch site> records phase cycles per block
    am.stamps = lab_stamps(name);
    const int split_rpw = CRFP_LAB_KNOB("CRFP_SPLIT_RPW", 1);
    if (!split) return 0;
    *done = true;
    const int TH = split_rpw == 1 ? 4 : 8;
    const int tiles = ((a.W + TW - 1) / TW) * ((a.H + TH - 1) / TH);
    const bool use_f16 = strcmp(lab_conv_mode(), "bf16x6") != 0;
    // warp-specialised variant: measured 346 vs 351.5 frames/s for the single-role kernels (loader issue is
    // throttled by the ~12 B/clk/CU the memory system delivers) -> kept as an opt-in experiment
    const bool use_ws = CRFP_LAB_KNOB("CRFP_SPLIT_WS", 0) == 1;
    // input-stationary variant: wins for bf16x6 (65 KB workgroups, 2 per CU); with f16x3 the plain kernel runs 3 workgroups
    // per CU and is faster even for the 216-channel conv (139.8 vs 147.6 us), so it is opt-in there
    const int is_knob = CRFP_LAB_KNOB("CRFP_SPLIT_IS", -1);
    const bool use_is = is_knob < 0 ? !use_f16 : is_knob != 0;
    const bool use_pipe = CRFP_LAB_KNOB("CRFP_SPLIT_PIPE", 0) == 1;
    constexpr int pipe_wgs = 256;   // one workgroup per CU
    if (use_ws) {
        const int wtiles = ((a.W + TW - 1) / TW) * ((a.H + WS_TH - 1) / WS_TH);
        if (use_is && a.kq <= 8 && a.ctiles >= 2) {
            conv3x3_split_ws_kernel<true><<<dim3(wtiles, 1, a.N), WS_NT, 0, s>>>(a);
        } else {
            conv3x3_split_ws_kernel<false><<<dim3(wtiles, a.ctiles, a.N), WS_NT, 0, s>>>(a);
        }
        CRFP_CHECK_LAUNCH();
        return 0;
    }
    if (use_is && a.kq <= 8 && a.ctiles >= 2) {
        // input-stationary: whole K in LDS, one workgroup per 4x64 tile walks every cout tile
        dim3 grid(((a.W + TW - 1) / TW) * ((a.H + 7) / 8), 1, a.N);
        if (use_f16) {
            if (a.kq == 4) conv3x3_split_is_kernel<1, 8, 2><<<grid, 512, 0, s>>>(am);
            else conv3x3_split_is_kernel<2, 8, 2><<<grid, 512, 0, s>>>(am);
        } else {
            if (a.kq == 4) conv3x3_split_is_kernel<1, 8, 3><<<grid, 512, 0, s>>>(am);
            else conv3x3_split_is_kernel<2, 8, 3><<<grid, 512, 0, s>>>(am);
        }
        CRFP_CHECK_LAUNCH();
        return 0;
    }
    if (use_pipe) {
        // persistent: one workgroup per CU walks tiles blockIdx.x, blockIdx.x + gridDim.x, ...
        const int ntl = ((a.W + TW - 1) / TW) * ((a.H + PIPE_NW - 1) / PIPE_NW);
        const int per = (ntl + pipe_wgs - 1) / pipe_wgs;           // tiles per workgroup
        dim3 grid((ntl + per - 1) / per, a.ctiles, a.N);           // balanced shares
        conv3x3_split_pipe_kernel<<<grid, PIPE_NT, 0, s>>>(a);
        CRFP_CHECK_LAUNCH();
        return 0;
    }
    if (split_rpw != 1 || !use_f16) {
        if (split_rpw == 1) {
            conv3x3_split_kernel<1, 1, 3><<<dim3(tiles * a.ctiles, 1, a.N), 256, 0, s>>>(am);
        } else {
            dim3 grid(tiles * a.ctiles, 1, a.N);
            if (use_f16) conv3x3_split_kernel<1, 2, 2><<<grid, 256, 0, s>>>(am);
            else conv3x3_split_kernel<1, 2, 3><<<grid, 256, 0, s>>>(am);
        }
        CRFP_CHECK_LAUNCH();
        return 0;
    }
    *done = false;   // the shipped kernel
    return 0;
}
