// 3x3 stride-1 pad-1 convolution as an implicit GEMM on the MFMA, gfx950.  Replaces every "wide" nn.Conv2d(k=3) of
// the reference path (model/CRFP.py:303-317, 449-450, 532, 172-176, 257-261, 747-795; model/LTE.py:40-42).
//
// File map: shared epilogue (conv_epilogue_t) | fp32-MFMA kernel conv3x3_mfma_kernel (v_mfma_f32_32x32x2_f32: the per-op
// C-ABI and the few convs with NCHW / ragged-K sources) | the split-operand kernels: the DEFAULT
// conv3x3_split_kernel<1,1,2> (f16x3; bf16x6 as <.,.,3>) and the 8-wave conv3x3_split8_kernel | the
// bf16-storage kernels and the chunk-staging helpers two of them share | conv_mfma_lab.inc (lab library only: the main
// loops that lost their A/B -- persistent, pipelined, input-stationary, warp-specialised -- their knobs and dispatch) |
// weight packers | conv_work / prepare_plan and the four launchers.
// The layout notes below are written for the fp32 kernel; the split kernels share orientation, lane map and epilogue.
//
// GEMM orientation:  D[cout][pixel] += A[cout][k] * B[k][pixel]
//   A = weights (rows = 32 output channels of a cout tile), pre-packed so that the 64 lanes of a
//       wave read one contiguous 1 KiB (float4 per lane) per (k-quad-pair, tap): lane (row, half)
//       holds W[row][4 K-channels of quad 2*pair+half][tap].
//   B = activations from an LDS halo tile in Q4 layout: lane (pixel, half) does ONE ds_read_b128
//       = the 4 K-channels of quad 2*pair+half at its (shifted) pixel -> feeds 4 MFMAs.
//   D: lane (pixel = lane&31, half) ends up with 16 rows = four 4-channel groups
//       {8g+4*half .. +3}, g=0..3, i.e. four aligned Q4 elements -> four 16-B stores per tile.
// All layout permutations (virtual concat of several sources, pixel-shuffle on the store side,
// pixel-unshuffle on the load side) are folded into the weight packing (rows / K order) plus
// address arithmetic; no permutation kernel ever runs.
//
// Work decomposition: 256-thread workgroup (4 waves) = 8 rows x 64 px output tile; each wave owns
// 2 rows x 2 half-rows = four 32-pixel MFMA column tiles, times CT cout tiles.  K loop walks the
// input in chunks of 2 quads (8 channels): stage (8+2)x(64+2) halo -> LDS, 9 taps x 4 MFMAs x CT x 4.
#include "crfp_common.h"

#include <cstdlib>
#include <cstring>

namespace CRFP_NS {

constexpr int TW = 64, LW = TW + 2;
// activation loads of the implicit-GEMM kernels: plain (the non-temporal form, meant to keep a layer's INPUT from displacing its OUTPUT
// in the XCD's 4 MB L2, made every conv 4-10 % slower: profiles/README.md, round 4)
#define CRFP_LDACT(T, p) (*reinterpret_cast<const T*>(p))
constexpr int kTapUnroll = 3;   // tap-loop unroll factor of the fp32-MFMA and lab main loops

// tanh / sigmoid on the hardware exp2 + rcp (v_exp_f32, v_rcp_f32: ~1 ulp each) instead of the libm
// versions (~30 VALU instructions each): the 216-channel offset/mask epilogue is transcendental-bound
// otherwise.  |error| < 3e-7 absolute on both, i.e. < 3e-6 px on the +-10 px DCN offsets.
__device__ __forceinline__ float fast_tanh(float v) {
    const float e = __expf(-2.0f * fabsf(v));          // in (0, 1]: no overflow
    const float t = (1.0f - e) * __builtin_amdgcn_rcpf(1.0f + e);
    return copysignf(t, v);
}

__device__ __forceinline__ float apply_act(float v, int act) {
    switch (act) {
        case CRFP_ACT_RELU: return fmaxf(v, 0.0f);
        case CRFP_ACT_LRELU01: return v > 0.0f ? v : 0.1f * v;
        case CRFP_ACT_TANH: return fast_tanh(v);
        case CRFP_ACT_SIGMOID: return fast_sigmoid(v);
        default: return v;
    }
}

// Stage NIN halo elements of one K-quad into registers; the switch on the source kind is hoisted out
// of the (fully unrolled) element loop so every case is straight-line code with static register indices.
template <int NIN>
__device__ __forceinline__ void load_quad_batch(float4 (&r)[NIN], const ConvSrc& s, int n, int kql,
                                                const int (&gy)[NIN], const int (&gx)[NIN], const bool (&ok)[NIN],
                                                int H, int W) {
    const float* base = s.p + (long long)n * s.bstride;
#pragma unroll
    for (int k = 0; k < NIN; ++k) r[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    switch (s.kind) {
        case SRC_Q4: {
            const int PW = W + s.pad;
            const act_t* b = as_act(s.p) + (long long)n * s.bstride + (long long)kql * (H + s.pad) * PW * 4;
#pragma unroll
            for (int k = 0; k < NIN; ++k)
                if (ok[k]) { const cf32x4 v = ldq(b + ((long long)gy[k] * PW + gx[k]) * 4); r[k] = make_float4(v.x, v.y, v.z, v.w); }
            break;
        }
        case SRC_NCHW: {
#pragma unroll
            for (int k = 0; k < NIN; ++k)
                if (ok[k]) {
                    const long long o = (long long)gy[k] * W + gx[k], pl = (long long)H * W;
                    const int c0 = 4 * kql;
                    r[k].x = c0 + 0 < s.nch ? base[(c0 + 0) * pl + o] : 0.0f;
                    r[k].y = c0 + 1 < s.nch ? base[(c0 + 1) * pl + o] : 0.0f;
                    r[k].z = c0 + 2 < s.nch ? base[(c0 + 2) * pl + o] : 0.0f;
                    r[k].w = c0 + 3 < s.nch ? base[(c0 + 3) * pl + o] : 0.0f;
                }
            break;
        }
        case SRC_UNSHUF4: {
            const int Qp = kql >> 4, ij = kql & 15, i = ij >> 2, jj = ij & 3;
            const int H4 = 4 * H + s.pad, W4 = 4 * W + s.pad;
            const act_t* b = as_act(s.p) + (long long)n * s.bstride + (long long)Qp * H4 * W4 * 4;
#pragma unroll
            for (int k = 0; k < NIN; ++k)
                if (ok[k]) { const cf32x4 v = ldq(b + ((long long)(4 * gy[k] + i) * W4 + 4 * gx[k] + jj) * 4); r[k] = make_float4(v.x, v.y, v.z, v.w); }
            break;
        }
        case SRC_FLOW2: {
#pragma unroll
            for (int k = 0; k < NIN; ++k)
                if (ok[k]) {
                    const float2 f = *reinterpret_cast<const float2*>(base + ((long long)gy[k] * W + gx[k]) * 2);
                    r[k] = make_float4(f.x, f.y, 0.0f, 0.0f);
                }
            break;
        }
        case SRC_NCHW_SHIFT: {   // the tensor shifted by (sy, sx): its own validity test (ok[] belongs to the unshifted tile)
            const int sy = (s.rsv & 15) - 8, sx = ((s.rsv >> 4) & 15) - 8;
            const float lo = (s.rsv & 256) ? 0.0f : -__builtin_inff();   // ReLU on the way in
            const long long pl = (long long)H * W;
            const int c0 = 4 * kql;
#pragma unroll
            for (int k = 0; k < NIN; ++k) {
                const int y = gy[k] + sy, x = gx[k] + sx;
                if (y >= 0 && y < H && x >= 0 && x < W) {
                    const long long o = (long long)y * W + x;
                    r[k].x = c0 + 0 < s.nch ? fmaxf(base[(c0 + 0) * pl + o], lo) : 0.0f;
                    r[k].y = c0 + 1 < s.nch ? fmaxf(base[(c0 + 1) * pl + o], lo) : 0.0f;
                    r[k].z = c0 + 2 < s.nch ? fmaxf(base[(c0 + 2) * pl + o], lo) : 0.0f;
                    r[k].w = c0 + 3 < s.nch ? fmaxf(base[(c0 + 3) * pl + o], lo) : 0.0f;
                }
            }
            break;
        }
        default: break;
    }
}

// The f16x3 split of 4 values (same arithmetic as split_f16x8_fast further down, which a consuming conv would apply):
// hi[] = fp16(x) pairs, lo[] = fp16((x - fp16(x)) * 2^11) pairs.
__device__ __forceinline__ void split_f16x4(const float (&x)[4], unsigned (&hi)[2], unsigned (&lo)[2]) {
    typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
    typedef float f2_t __attribute__((ext_vector_type(2)));
    float negone = -1.0f;
    asm("" : "+v"(negone));   // opaque: keeps fma(x0, -1, x) a v_fma_mix_f32
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const h2_t a = __builtin_convertvector(f2_t{x[2 * i], x[2 * i + 1]}, h2_t);
        const float r0 = __builtin_fmaf((float)a[0], negone, x[2 * i]);
        const float r1 = __builtin_fmaf((float)a[1], negone, x[2 * i + 1]);
        const h2_t b = __builtin_convertvector(f2_t{r0 * 2048.0f, r1 * 2048.0f}, h2_t);
        hi[i] = __builtin_bit_cast(unsigned, a);
        lo[i] = __builtin_bit_cast(unsigned, b);
    }
}

// Epilogue shared by the fp32-MFMA and the split-bf16-MFMA main loops (identical C/D lane map):
// bias, activation, scale, residual, layout-aware store.
//
// Everything that comes from the kernel arguments (destinations, strides, activation, store mode) is read
// ONCE into registers and the store mode is a template parameter: the first version re-read descriptors through
// scalar loads inside the (pt, g, dst) loops and carried every mode's code -- 7 300 ISA lines, 146 branches,
// 15 k cycles per workgroup (38 % of a 32->32 conv's workgroup lifetime, measured with s_memtime stamps).
// Bias quads and the residual are loaded up front so that the stores leave back to back.
//
// VBIAS = 2: the caller initialised the accumulators with the bias (loads issued at kernel start: no L2 round trip here);
// VBIAS = 1: bias through per-lane vector loads (single epilogue per workgroup).  Inside a loop over cout tiles a vector
// load would force s_waitcnt vmcnt(0), i.e. drain every store of the previous tile's epilogue (vmcnt is in-order and
// counts stores on CDNA4: 12k cycles per tile measured); those callers pass VBIAS=0 (wave-uniform scalar loads,
// selected per lane half) and preload the flow vectors of the lane's PT pixels (flpre, ST_OFFMASK).
struct EpiCtx {
    int H, W, cout, ncq, act, store, n_off_quads, dstH, dstW, lr;
    int xend;       // columns >= xend are not stored (W; the fused pair kernel's 62-column tiles end before their 64 computed columns)
    bool single;    // exactly one destination, starting at quad 0 and taking all of them
    long long* dbg; // diagnostic stamps (null in production)
    float slope, post;
    const float4* bp;
    const act_t* rp;
    const float* flp;
    bool f32dst;         // ST_Q4: the (single) destination is a float tensor also in the bf16 build (flow fields)
    unsigned* ovf;       // fp16-operand overflow word (null: not tracked)
    float* s3p;          // SRC_S3 image of the output (null: none)
    int s3_ngroups;      // cout / 8
    float* dp[CRFP_MAX_DST];
    long long dplane[CRFP_MAX_DST];
    int dpitch[CRFP_MAX_DST], dq0[CRFP_MAX_DST], dq1[CRFP_MAX_DST];
};

__device__ __forceinline__ EpiCtx epi_ctx(const ConvArgs& a, int n) {
    EpiCtx e;
    e.H = a.H; e.W = a.W; e.cout = a.cout; e.act = a.act; e.store = a.store;
    e.xend = a.W;
    e.ncq = (conv_packed_rows(a.cout, a.store, a.ps_r) + 3) >> 2;
    e.n_off_quads = a.n_off_quads; e.dstH = a.dstH; e.dstW = a.dstW;
    e.lr = a.ps_r == 4 ? 2 : 1;                           // ST_PS: r in {2, 4} (checked by the launcher)
    // NONE / RELU / LRELU(0.1) as max(v, slope*v) with slope 1 / 0 / 0.1: exact, branch-free, 2 VALU ops
    e.slope = a.act == CRFP_ACT_RELU ? 0.0f : (a.act == CRFP_ACT_LRELU01 ? 0.1f : 1.0f);
    e.post = a.post_scale;
    e.bp = reinterpret_cast<const float4*>(a.bpk);
    e.rp = a.resid ? as_act(a.resid) + (long long)n * a.resid_bstride : nullptr;
    e.f32dst = a.dst_f32 != 0;
    e.flp = a.flow + (long long)n * a.flow_bstride;
    e.s3p = a.s3_dst ? a.s3_dst + (long long)n * a.s3_bstride : nullptr;
    e.s3_ngroups = a.cout >> 3;
#pragma unroll
    for (int d = 0; d < CRFP_MAX_DST; ++d) {
        const bool on = d < a.ndst;
        // batch stride counts ELEMENTS of the destination's storage type (float for offsets / masks / flow / NCHW planes)
        const bool fdst = a.store == ST_OFFMASK || a.store == ST_NCHW || a.dst_f32;
        e.dp[d] = fdst ? a.dst[d].p + (long long)n * a.dst[d].bstride
                       : reinterpret_cast<float*>(as_act(a.dst[d].p) + (long long)n * a.dst[d].bstride);
        e.dpitch[d] = a.W + a.dst[d].pad;
        e.dplane[d] = (long long)(a.H + a.dst[d].pad) * e.dpitch[d] * 4;
        e.dq0[d] = on ? a.dst[d].q0 : 0;
        e.dq1[d] = on ? a.dst[d].q1 : 0;
    }
    e.single = a.ndst == 1 && a.dst[0].q0 == 0 && a.dst[0].q1 >= e.ncq;
    e.dbg = a.stamps;
    e.ovf = ovf_word(a.ovf, a.ovf_div, a.ovf_add, n, a.ovf_skip0);
    return e;
}

template <int CT, int PT, int RPW, int STORE, int VBIAS, bool SLOWACT>
__device__ __forceinline__ void conv_epilogue_t(const EpiCtx& e, f32x16 (&acc)[CT][PT], int T0, int tx0, int ty0,
                                                int wave, int j, int h, const float2* flpre) {
    const int H = e.H, W = e.W;
    float4 bb[CT][4];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int cq0 = (T0 + ct) * 8 + 2 * g;          // wave-uniform
            if (VBIAS == 2) {
                bb[ct][g] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            } else if (VBIAS == 1) {
                bb[ct][g] = e.bp[cq0 + h];
            } else {
                const float4 b0 = e.bp[cq0], b1 = e.bp[cq0 + 1];
                bb[ct][g] = h ? b1 : b0;
            }
        }

#ifdef CRFP_EPI_DBG
    long long d0 = __builtin_amdgcn_s_memtime(), d1 = 0;
#endif
    float vmax = 0.0f;   // largest |value| this lane stores (fp16-operand range guard, see ConvArgs::ovf)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
#ifdef CRFP_EPI_DBG
        if (pt == 1) d1 = __builtin_amdgcn_s_memtime();
#endif
        const int y = ty0 + wave * RPW + (pt >> 1), x = tx0 + (pt & 1) * 32 + j;
        if (y >= H || x >= e.xend) continue;
        float2 fl = make_float2(0.0f, 0.0f);
        if (STORE == ST_OFFMASK) fl = flpre ? flpre[pt] : *reinterpret_cast<const float2*>(e.flp + ((long long)y * W + x) * 2);
        float4 rr[CT][4];
        if (e.rp) {   // wave-uniform; all residual quads of this pixel in flight together, before the first store
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int cq = min((T0 + ct) * 8 + 2 * g + h, e.ncq - 1);
                    { const cf32x4 rv = ldq(e.rp + (((long long)cq * H + y) * W + x) * 4); rr[ct][g] = make_float4(rv.x, rv.y, rv.z, rv.w); }
                }
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int cq = (T0 + ct) * 8 + 2 * g + h;
                if (cq >= e.ncq) continue;
                const float4 b = bb[ct][g];
                float v[4] = {acc[ct][pt][4 * g + 0] + b.x, acc[ct][pt][4 * g + 1] + b.y,
                              acc[ct][pt][4 * g + 2] + b.z, acc[ct][pt][4 * g + 3] + b.w};
                if (STORE == ST_OFFMASK) {
                    if (cq < e.n_off_quads) {  // (dy,dx) pairs: 10*tanh(.) + flow flipped to (y,x)
                        v[0] = tanh10_plus(v[0], 10.0f + fl.y);
                        v[1] = tanh10_plus(v[1], 10.0f + fl.x);
                        v[2] = tanh10_plus(v[2], 10.0f + fl.y);
                        v[3] = tanh10_plus(v[3], 10.0f + fl.x);
                    } else {
#pragma unroll
                        for (int c = 0; c < 4; ++c) v[c] = fast_sigmoid(v[c]);
                    }
                } else if (SLOWACT) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[c] = apply_act(v[c], e.act) * e.post;
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[c] = fmaxf(v[c], e.slope * v[c]) * e.post;   // slope in {1, 0, 0.1}: none / relu / lrelu
                }
                if (STORE != ST_PS && (e.cout & 3)) {  // zero the padding components of a ragged last quad (wave-uniform test)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (4 * cq + c >= e.cout) v[c] = 0.0f;
                }
                if (e.rp) { v[0] += rr[ct][g].x; v[1] += rr[ct][g].y; v[2] += rr[ct][g].z; v[3] += rr[ct][g].w; }
                if (STORE != ST_OFFMASK && STORE != ST_NCHW)   // those outputs never feed an fp16 operand
                    vmax = fmaxf(fmaxf(vmax, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
                // store addresses = per-lane pixel offset (one 32-bit multiply per pixel tile) + wave-uniform 64-bit
                // part per quad: the per-lane 64-bit multiplies of the first version were most of the epilogue's 6 k cycles
#ifndef CRFP_ACT_BF16
                if (STORE == ST_Q4 && e.s3p) {   // SRC_S3 image: this lane's 4 channels are half h of the 8-channel element
                    unsigned hi2[2], lo2[2];
                    split_f16x4(v, hi2, lo2);
                    // v_permlane32_swap: lanes 32-63 of the first operand trade places with lanes 0-31 of the second.  After
                    // it the lower lane (h = 0) holds the x0 words of all 8 channels and the upper lane (same pixel, h = 1)
                    // the x1s words: one 16-byte store per lane instead of two 8-byte ones.
                    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                    const u32x2 r0 = __builtin_amdgcn_permlane32_swap(hi2[0], lo2[0], false, false);
                    const u32x2 r1 = __builtin_amdgcn_permlane32_swap(hi2[1], lo2[1], false, false);
                    const int plane = (T0 + ct) * 4 + g + h * e.s3_ngroups;
                    *reinterpret_cast<uint4*>(e.s3p + (((long long)plane * H + y) * W + x) * 4) = make_uint4(r0.x, r1.x, r0.y, r1.y);
                }
#endif
                if (STORE == ST_OFFMASK || (STORE == ST_Q4 && kActBf16 && e.f32dst)) {   // float destination (offsets / masks / flow), single
                    const int cq0u = (T0 + ct) * 8 + 2 * g;
                    *reinterpret_cast<float4*>(e.dp[0] + (long long)cq0u * e.dplane[0] + h * e.dplane[0] + (y * e.dpitch[0] + x) * 4) =
                        make_float4(v[0], v[1], v[2], v[3]);
                } else if (STORE == ST_Q4) {
                    if (e.single) {   // one destination that takes every quad (wave-uniform)
                        const int cq0u = (T0 + ct) * 8 + 2 * g;
                        stq(as_act(e.dp[0]) + (long long)cq0u * e.dplane[0] + h * e.dplane[0] + (y * e.dpitch[0] + x) * 4,
                            cf32x4{v[0], v[1], v[2], v[3]});
                    } else {
#pragma unroll
                        for (int d = 0; d < CRFP_MAX_DST; ++d)
                            if (cq >= e.dq0[d] && cq < e.dq1[d])
                                stq(as_act(e.dp[d]) + (cq - e.dq0[d]) * e.dplane[d] + (y * e.dpitch[d] + x) * 4,
                                    cf32x4{v[0], v[1], v[2], v[3]});
                    }
                } else if (STORE == ST_PS) {
                    // cq0 is even and r >= 2: both lane halves share (Q, i) and differ by jj = +h
                    const int lr = e.lr, cq0u = (T0 + ct) * 8 + 2 * g;
                    const int Q = cq0u >> (2 * lr), sidx = cq0u & ((1 << (2 * lr)) - 1), i = sidx >> lr, jj = sidx & ((1 << lr) - 1);
                    stq(as_act(e.dp[0]) + ((long long)Q * e.dstH + i) * e.dstW * 4 + jj * 4 + (((y << lr) * e.dstW + (x << lr)) + h) * 4,
                        cf32x4{v[0], v[1], v[2], v[3]});
                } else {  // ST_NCHW
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int ch = 4 * cq + c;
                        if (ch < e.cout) e.dp[0][((long long)ch * H + y) * W + x] = v[c];
                    }
                }
            }
    }
    // a stored value that the next split-fp16 conv could not represent (>= 65504, inf): raise the sticky word; the output
    // head then poisons the frame with NaN instead of returning plausible garbage
    if (e.ovf && !(vmax < 65504.0f)) atomicOr(e.ovf, 1u);
#ifdef CRFP_EPI_DBG
    if (e.dbg && threadIdx.x == 0) {
        long long* o = e.dbg + (16384 + (long long)blockIdx.x) * 8;
        o[0] = d0; o[1] = d1; o[2] = __builtin_amdgcn_s_memtime(); o[3] = 1;
    }
#endif
}

// e: epi_ctx() made once per workgroup (outside any loop over cout tiles)
template <int CT, int PT, int RPW, int VBIAS = 1>
__device__ __forceinline__ void conv_epilogue(const EpiCtx& e, f32x16 (&acc)[CT][PT], int T0, int tx0, int ty0,
                                              int wave, int j, int h, const float2* flpre = nullptr) {
    const bool slow = e.act == CRFP_ACT_TANH || e.act == CRFP_ACT_SIGMOID;   // API only; the engine never uses them here
    switch (e.store) {   // wave-uniform
        case ST_Q4:
            if (slow) conv_epilogue_t<CT, PT, RPW, ST_Q4, VBIAS, true>(e, acc, T0, tx0, ty0, wave, j, h, flpre);
            else conv_epilogue_t<CT, PT, RPW, ST_Q4, VBIAS, false>(e, acc, T0, tx0, ty0, wave, j, h, flpre);
            break;
        case ST_PS: conv_epilogue_t<CT, PT, RPW, ST_PS, VBIAS, false>(e, acc, T0, tx0, ty0, wave, j, h, flpre); break;
        case ST_OFFMASK: conv_epilogue_t<CT, PT, RPW, ST_OFFMASK, VBIAS, false>(e, acc, T0, tx0, ty0, wave, j, h, flpre); break;
        default:
            if (slow) conv_epilogue_t<CT, PT, RPW, ST_NCHW, VBIAS, true>(e, acc, T0, tx0, ty0, wave, j, h, flpre);
            else conv_epilogue_t<CT, PT, RPW, ST_NCHW, VBIAS, false>(e, acc, T0, tx0, ty0, wave, j, h, flpre);
            break;
    }
}

typedef float f32x4 __attribute__((ext_vector_type(4)));  // native vector: stays in VGPRs (HIP's float4 struct
                                                          // copies lowered to memcpy into a private alloca)
template <int CT, int NW>
__device__ __forceinline__ void load_weight_batch(f32x4 (&rw)[NW], const f32x4* __restrict__ wp, int T0, int npairs,
                                                  int pair, int tid) {
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const int idx = min(tid + 256 * k, CT * 576 - 1);  // clamp: always a valid load
        const int ct = idx / 576, rem = idx - ct * 576;
        rw[k] = wp[((long long)(T0 + ct) * npairs + pair) * 576 + rem];
    }
}

// CT = cout tiles (of 32) per workgroup, RPW = output rows per wave (tile = 4*RPW rows x 64 px).
// KP = K-chunks (of 8 channels) per staging phase: 1 everywhere except the long-K convolutions of SPyNet (9 x cin virtual channels,
// up to 72 chunks: on its coarse pyramid levels a conv is one or two workgroups walking that many barrier pairs, so two chunks per
// phase halve the fixed part; same chunk order, same accumulation order, same values).
template <int CT, int RPW, int KP = 1>
__global__ __launch_bounds__(256, 2) void conv3x3_mfma_kernel(const ConvArgs a) {
    constexpr int TH = 4 * RPW, LH = TH + 2, PT = 2 * RPW;
    // One K-chunk (2 quads = 8 input channels) lives in LDS at a time: the halo tile of both quads
    // and the packed weights of the chunk for the CT cout tiles.  The NEXT chunk's global loads are
    // issued into registers before the MFMAs of the current chunk start, so HBM/L2 latency hides
    // behind 144*CT MFMAs per wave; LDS is rewritten between two barriers.
    __shared__ float4 tile[2 * KP][LH][LW];
    __shared__ float4 wlds[KP][CT][9 * 64];
    constexpr int NIN = (LH * LW + 255) / 256;       // 3 halo elements per thread per quad
    constexpr int NW = (CT * 9 * 64 + 255) / 256;    // 3 (CT=1) or 5 (CT=2) weight float4 per thread
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int tiles_x = (a.W + TW - 1) / TW;
    // 1-D grid over (tile, cout-tile group) with the groups of a tile adjacent, dealt to the XCDs in contiguous bands:
    // neighbouring tiles share their halo lines and the cout-tile groups of one tile re-read the same input in one L2
    const int ngrp = a.ctiles / CT;
    const int bwork = xcd_band_tile(blockIdx.x, gridDim.x);
    const int btile = bwork / ngrp;
    const int tx0 = (btile % tiles_x) * TW, ty0 = (btile / tiles_x) * TH;
    const int T0 = (bwork - btile * ngrp) * CT;
    const int n = blockIdx.z;                                         // destination "batch item" (ksplit: one per K slice)
    const int n_src = a.ksplit > 0 ? n / a.ksplit : (a.src_bgroup > 0 ? n + n / a.src_bgroup : n);   // source batch item (ConvArgs::ksplit / src_bgroup)
    const int H = a.H, W = a.W;

    // per-thread staging coordinates (constant over the K loop)
    int sgy[NIN], sgx[NIN];
    bool sval[NIN];
#pragma unroll
    for (int k = 0; k < NIN; ++k) {
        const int idx = tid + 256 * k;
        const int r = idx / LW, c = idx - r * LW;
        sgy[k] = ty0 + r - 1;
        sgx[k] = tx0 + c - 1;
        sval[k] = idx < LH * LW && sgy[k] >= 0 && sgy[k] < H && sgx[k] >= 0 && sgx[k] < W;
    }

    f32x16 acc[CT][PT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int pt = 0; pt < PT; ++pt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ct][pt][e] = 0.0f;

    const int npairs = a.kq >> 1;
    const int npl = a.ksplit > 0 ? npairs / a.ksplit : npairs;        // K chunks this workgroup walks ...
    const int pair0 = a.ksplit > 0 ? (n % a.ksplit) * npl : 0;        // ... starting here
    const f32x4* __restrict__ wp = reinterpret_cast<const f32x4*>(a.wpk);
    float4 rin0[KP][NIN], rin1[KP][NIN];
    f32x4 rw[KP][NW];

    // loads of the KP chunks of staging phase ST (chunk index clamped past the end: an odd chunk count repeats the last one, unused)
#define CRFP_ISSUE_LOADS(ST)                                                                            \
    _Pragma("unroll") for (int kp = 0; kp < KP; ++kp) {                                                 \
        const int pair_ = pair0 + min(KP * (ST) + kp, npl - 1);                                         \
        {                                                                                               \
            int kql = 2 * pair_, s = 0;                                                                 \
            while (s < a.nsrc - 1 && kql >= a.src[s].nq) { kql -= a.src[s].nq; ++s; }                  \
            load_quad_batch<NIN>(rin0[kp], a.src[s], n_src, kql, sgy, sgx, sval, H, W);                 \
        }                                                                                               \
        {                                                                                               \
            int kql = 2 * pair_ + 1, s = 0;                                                             \
            while (s < a.nsrc - 1 && kql >= a.src[s].nq) { kql -= a.src[s].nq; ++s; }                  \
            load_quad_batch<NIN>(rin1[kp], a.src[s], n_src, kql, sgy, sgx, sval, H, W);                 \
        }                                                                                               \
        load_weight_batch<CT, NW>(rw[kp], wp, T0, npairs, pair_, tid);                                  \
    }

    const int nstages = (npl + KP - 1) / KP;
    CRFP_ISSUE_LOADS(0)
    for (int st = 0; st < nstages; ++st) {
        __syncthreads();  // every wave finished reading the previous chunk
#pragma unroll
        for (int kp = 0; kp < KP; ++kp) {
#pragma unroll
            for (int k = 0; k < NIN; ++k) {
                const int idx = tid + 256 * k;
                if (idx < LH * LW) {
                    (&tile[2 * kp][0][0])[idx] = rin0[kp][k];
                    (&tile[2 * kp + 1][0][0])[idx] = rin1[kp][k];
                }
            }
#pragma unroll
            for (int k = 0; k < NW; ++k) {
                const int idx = tid + 256 * k;
                if (idx < CT * 576) reinterpret_cast<f32x4*>(&wlds[kp][0][0])[idx] = rw[kp][k];
            }
        }
        __syncthreads();
        if (st + 1 < nstages) CRFP_ISSUE_LOADS(st + 1)
#pragma unroll
        for (int kp = 0; kp < KP; ++kp) {
        if (KP * st + kp >= npl) break;   // workgroup-uniform
#pragma unroll kTapUnroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - 3 * ky;
            float4 wa[CT];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) wa[ct] = wlds[kp][ct][tap * 64 + lane];
            float4 b[PT];
#pragma unroll
            for (int pt = 0; pt < PT; ++pt) b[pt] = tile[2 * kp + h][wave * RPW + (pt >> 1) + ky][(pt & 1) * 32 + j + kx];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int pt = 0; pt < PT; ++pt) {
                    if ((pt & 1) && tx0 + 32 >= W) continue;   // workgroup-uniform: the tile's right half lies outside a narrow map
                    acc[ct][pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[ct].x, b[pt].x, acc[ct][pt], 0, 0, 0);
                    acc[ct][pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[ct].y, b[pt].y, acc[ct][pt], 0, 0, 0);
                    acc[ct][pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[ct].z, b[pt].z, acc[ct][pt], 0, 0, 0);
                    acc[ct][pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[ct].w, b[pt].w, acc[ct][pt], 0, 0, 0);
                }
        }
        }
    }
#undef CRFP_ISSUE_LOADS

    const EpiCtx ec = epi_ctx(a, n);
    conv_epilogue<CT, PT, RPW>(ec, acc, T0, tx0, ty0, wave, j, h);
}

// ================================================================ split-bf16 ("bf16x6") main loop
// fp32-grade convolution on the bf16 MFMA (v_mfma_f32_32x32x16_bf16, 16x the fp32-MFMA rate):
// every fp32 operand x is split exactly into three bf16 terms x = x0 + x1 + x2 (x0 = bf16(x),
// x1 = bf16(x - x0), x2 = bf16(x - x0 - x1); the subtractions are exact in fp32) and the product is
// accumulated in fp32 as  x0w0 + x0w1 + x1w0 + x0w2 + x2w0 + x1w1 ; the dropped terms are <= 2^-24
// relative, i.e. below fp32 rounding (measured: max rel. error 1.9e-6 vs 3.1e-6 for a plain fp32
// matmul at K = 576).  6 bf16 MFMAs replace 8 fp32 MFMAs of 1/16 the rate: 2.67x the throughput of
// the fp32-MFMA path at the same accuracy.  Weights are split once at pack time; activations are
// split while the halo tile is staged (global fp32 -> registers -> 3 bf16 images in LDS).
// K-chunk = 16 channels = 4 quads (lane-half h supplies k = 8h..8h+7 = quads 2h, 2h+1 of the chunk).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#ifndef CRFP_ACT_BF16   // the split-operand schemes exist for fp32 activations only
constexpr int kSplitTapUnroll = 9;   // tap loop of the default split kernel: full unroll measured +1.4 % frames/s over 3 (168 VGPRs, still 3 waves/SIMD)
__device__ __forceinline__ void split_bf16x8(const f32x4& lo, const f32x4& hi, bf16x8& p0, bf16x8& p1, bf16x8& p2) {
    const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const __bf16 a = (__bf16)x[i];
        const float r = x[i] - (float)a;
        const __bf16 b = (__bf16)r;
        const float r2 = r - (float)b;
        p0[i] = a;
        p1[i] = b;
        p2[i] = (__bf16)r2;
    }
}

// ---- split-fp16 ("f16x3"): x = x0 + 2^-11 * x1s with x0 = fp16(x), x1s = fp16((x - x0) * 2^11) (the subtraction and the
// scaling are exact; the scale keeps the residual out of fp16's subnormal range, where the MFMA would flush it).
// Product = x0w0 + 2^-11 * (x0w1s + x1sw0): two fp32 accumulators (hi, lo), THREE MFMAs per 16-channel tap instead of
// six, two LDS images per operand instead of three, and the dropped term x1w1 is <= 2^-22 relative.  CPU emulation
// of the whole 7-frame clip: max |err| 2.2e-6 vs 2.5e-6 for bf16x6 (both at the fp32 summation-order noise floor);
// without the scaling 6.7e-6 if subnormals survive and 1.0e-3 if they are flushed.  Needs |x| < 65504.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
constexpr float F16_RES_SCALE = 2048.0f;

__device__ __forceinline__ void split_f16x8(const f32x4& lo, const f32x4& hi, bf16x8& p0, bf16x8& p1) {
    const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    f16x8 a, b;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const _Float16 h = (_Float16)x[i];
        a[i] = h;
        b[i] = (_Float16)((x[i] - (float)h) * F16_RES_SCALE);
    }
    p0 = __builtin_bit_cast(bf16x8, a);   // LDS / register containers are typed bf16x8 for both schemes
    p1 = __builtin_bit_cast(bf16x8, b);
}

// Same values as split_f16x8 for a halo pixel whose 8 channels all exist (component masks = 15): pixel validity is
// folded into the residual scale (sc = valid ? 2^11 : 0) and an AND on the packed hi words (km = valid ? ~0 : 0), the
// hi parts come out of one v_cvt_pk_f16_f32 per pair and x - x0 out of one v_fma_mix_f32: 3.5 VALU ops per value
// instead of 8.5 (the masked form spends 3 on and/cmp/cndmask per value and converts the hi part twice).
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void split_f16x8_fast(const f32x4& lo, const f32x4& hi, float sc, unsigned km, bf16x8& p0, bf16x8& p1) {
    const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    u32x4 a, b;
    float negone = -1.0f;
    asm("" : "+v"(negone));   // opaque, or the fma is canonicalised to fpext + fsub (two instructions)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f16x2 h2 = __builtin_convertvector(f32x2{x[2 * i], x[2 * i + 1]}, f16x2);
        const float r0 = __builtin_fmaf((float)h2[0], negone, x[2 * i]);       // = x - x0, exact (v_fma_mix_f32)
        const float r1 = __builtin_fmaf((float)h2[1], negone, x[2 * i + 1]);
        const f16x2 l2 = __builtin_convertvector(f32x2{r0 * sc, r1 * sc}, f16x2);
        a[i] = __builtin_bit_cast(unsigned, h2) & km;
        b[i] = __builtin_bit_cast(unsigned, l2);
    }
    p0 = __builtin_bit_cast(bf16x8, a);
    p1 = __builtin_bit_cast(bf16x8, b);
}

// NP = 3: bf16x6, NP = 2: f16x3.  p[] receives the NP images of 8 channels.
template <int NP>
__device__ __forceinline__ void split_parts(const f32x4& lo, const f32x4& hi, bf16x8 (&p)[NP]);
template <>
__device__ __forceinline__ void split_parts<3>(const f32x4& lo, const f32x4& hi, bf16x8 (&p)[3]) { split_bf16x8(lo, hi, p[0], p[1], p[2]); }
template <>
__device__ __forceinline__ void split_parts<2>(const f32x4& lo, const f32x4& hi, bf16x8 (&p)[2]) { split_f16x8(lo, hi, p[0], p[1]); }

// all products of one (tap, 32-pixel tile): w[] / b[] are the NP images of the A / B fragments
template <int NP>
__device__ __forceinline__ void split_mfma(f32x16& hi, f32x16& lo, const bf16x8 (&w)[NP], const bf16x8 (&b)[NP]) {
    if (NP == 3) {
        f32x16 c = hi;
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[1], b[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], b[NP - 1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[NP - 1], b[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], b[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[1], b[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0], b[0], c, 0, 0, 0);
        hi = c;
    } else {
        const f16x8 w0 = __builtin_bit_cast(f16x8, w[0]), w1 = __builtin_bit_cast(f16x8, w[1]);
        const f16x8 b0 = __builtin_bit_cast(f16x8, b[0]), b1 = __builtin_bit_cast(f16x8, b[1]);
        lo = __builtin_amdgcn_mfma_f32_32x32x16_f16(w0, b1, lo, 0, 0, 0);
        hi = __builtin_amdgcn_mfma_f32_32x32x16_f16(w0, b0, hi, 0, 0, 0);
        lo = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1, b0, lo, 0, 0, 0);
    }
}

__device__ __forceinline__ f32x4 mask_quad(const f32x4& v, int m) {
    return f32x4{(m & 1) ? v.x : 0.0f, (m & 2) ? v.y : 0.0f, (m & 4) ? v.z : 0.0f, (m & 8) ? v.w : 0.0f};
}

// one K-quad of NIN halo elements into registers (native vectors, switch hoisted out of the loop)
template <int NIN>
__device__ __forceinline__ void load_quad_batch_v(f32x4 (&r)[NIN], const ConvSrc& s, int n, int kql,
                                                  const int (&gy)[NIN], const int (&gx)[NIN], const bool (&ok)[NIN],
                                                  int H, int W) {
    const float* base = s.p + (long long)n * s.bstride;
#pragma unroll
    for (int k = 0; k < NIN; ++k) r[k] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    switch (s.kind) {
        case SRC_Q4: {
            const int PW = W + s.pad;
            const float* b = base + (long long)kql * (H + s.pad) * PW * 4;
#pragma unroll
            for (int k = 0; k < NIN; ++k)
                if (ok[k]) r[k] = *reinterpret_cast<const f32x4*>(b + ((long long)gy[k] * PW + gx[k]) * 4);
            break;
        }
        case SRC_NCHW: {
#pragma unroll
            for (int k = 0; k < NIN; ++k)
                if (ok[k]) {
                    const long long o = (long long)gy[k] * W + gx[k], pl = (long long)H * W;
                    const int c0 = 4 * kql;
                    r[k].x = c0 + 0 < s.nch ? base[(c0 + 0) * pl + o] : 0.0f;
                    r[k].y = c0 + 1 < s.nch ? base[(c0 + 1) * pl + o] : 0.0f;
                    r[k].z = c0 + 2 < s.nch ? base[(c0 + 2) * pl + o] : 0.0f;
                    r[k].w = c0 + 3 < s.nch ? base[(c0 + 3) * pl + o] : 0.0f;
                }
            break;
        }
        case SRC_UNSHUF4: {
            const int Qp = kql >> 4, ij = kql & 15, i = ij >> 2, jj = ij & 3;
            const int H4 = 4 * H + s.pad, W4 = 4 * W + s.pad;
            const float* b = base + (long long)Qp * H4 * W4 * 4;
#pragma unroll
            for (int k = 0; k < NIN; ++k)
                if (ok[k]) r[k] = *reinterpret_cast<const f32x4*>(b + ((long long)(4 * gy[k] + i) * W4 + 4 * gx[k] + jj) * 4);
            break;
        }
        case SRC_FLOW2: {
#pragma unroll
            for (int k = 0; k < NIN; ++k)
                if (ok[k]) {
                    const float2 f = *reinterpret_cast<const float2*>(base + ((long long)gy[k] * W + gx[k]) * 2);
                    r[k] = f32x4{f.x, f.y, 0.0f, 0.0f};
                }
            break;
        }
        default: break;
    }
}

// s_memtime phase stamps of conv3x3_split_body (CRFP_STAMP_PTR / CRFP_STAMP_NAME): lab library only, nothing in the product
#ifdef CRFP_LAB
#define SB_STAMP_ENTRY const long long t_entry = __builtin_amdgcn_s_memtime();
#define SB_STAMP_BEGIN long long tA = 0, tB = 0, tC = 0, tD = 0, t0 = __builtin_amdgcn_s_memtime();
#define SB_STAMP(ACC) if (a.stamps) { const long long t = __builtin_amdgcn_s_memtime(); ACC += t - t0; t0 = t; }
// diagnostic: the load-landing wait is booked under C
#define SB_STAMP_LANDED                                                                                   \
    if (a.stamps) {                                                                                       \
        long long t = __builtin_amdgcn_s_memtime(); tA += t - t0; t0 = t;                                 \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                  \
        t = __builtin_amdgcn_s_memtime(); tC += t - t0; t0 = t;                                           \
    }
#define SB_STAMP_LOOP_END                                                                                 \
    if (a.stamps) {                                                                                       \
        const long long t = __builtin_amdgcn_s_memtime(); tD += t - t0; t0 = t;                           \
        if (tid == 0) {                                                                                   \
            long long* o = a.stamps + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 8;               \
            o[0] = tA; o[1] = tB; o[2] = tC; o[3] = tD; o[4] = t_entry; o[5] = t;                         \
        }                                                                                                 \
    }
#define SB_STAMP_ACC_DONE                                                                                 \
    long long te1 = 0, te2 = 0;                                                                           \
    if (a.stamps) { asm volatile("s_nop 0" ::"v"(acc[0][0][0]), "v"(acc[0][PT - 1][15])); te1 = __builtin_amdgcn_s_memtime(); }
#define SB_STAMP_EPI_CTX                                                                                  \
    if (a.stamps) { asm volatile("s_waitcnt lgkmcnt(0)" ::"s"(ec.dpitch[0]), "s"(ec.ncq), "s"(ec.slope)); te2 = __builtin_amdgcn_s_memtime(); }
#define SB_STAMP_EPI_DONE                                                                                 \
    if (a.stamps) {                                                                                       \
        const long long ti = __builtin_amdgcn_s_memtime();      /* epilogue issued (stores in flight) */  \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                  \
        if (tid == 0) {                                                                                   \
            a.stamps[((long long)blockIdx.y * gridDim.x + blockIdx.x) * 8 + 2] = te1;   /* overwrites phase C (unused here) */ \
            a.stamps[((long long)blockIdx.y * gridDim.x + blockIdx.x) * 8 + 3] = te2;   /* overwrites phase D */ \
            a.stamps[((long long)blockIdx.y * gridDim.x + blockIdx.x) * 8 + 7] = ti;                      \
            a.stamps[((long long)blockIdx.y * gridDim.x + blockIdx.x) * 8 + 6] = __builtin_amdgcn_s_memtime(); \
        }                                                                                                 \
    }
#else
#define SB_STAMP_ENTRY
#define SB_STAMP_BEGIN
#define SB_STAMP(ACC)
#define SB_STAMP_LANDED
#define SB_STAMP_LOOP_END
#define SB_STAMP_ACC_DONE
#define SB_STAMP_EPI_CTX
#define SB_STAMP_EPI_DONE
#endif

// The kernel's body: workgroup wg_x of wg_nx (the launch's work items: (tile, cout-tile group)) of batch item n of plan a.  A function so that
// conv3x3_split_dual_kernel (below) can run TWO plans in one launch.
template <int CT, int RPW, int NP>
__device__ __forceinline__ void conv3x3_split_body(const ConvArgs& a, const int wg_x, const int wg_nx, const int n) {
    SB_STAMP_ENTRY
    constexpr int TH = 4 * RPW, LH = TH + 2, PT = 2 * RPW;
    constexpr int NEL = LH * LW;                 // halo pixels
    constexpr int NIN = (NEL + 255) / 256;       // halo pixels per thread; each carries the chunk's 4 quads
    constexpr int WPC = 9 * NP * 64;             // weight vectors per (cout tile, chunk)
    __shared__ bf16x8 tile[NP][2][NEL];          // [split part][quad pair][halo pixel], 16 B each
    __shared__ bf16x8 wlds[CT][WPC];             // [cout tile][(tap, part)][lane]: this chunk's A fragments
    constexpr int NWS = (CT * WPC + 255) / 256;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int tiles_x = (a.W + TW - 1) / TW;
    // 1-D grid over (tile, cout-tile group) with the groups of a tile adjacent, dealt to the XCDs in contiguous bands:
    // neighbouring tiles share their halo lines and the cout-tile groups of one tile re-read the same input in one L2
    const int ngrp = a.ctiles / CT;
    const int bwork = xcd_band_tile(wg_x, wg_nx);
    const int btile = bwork / ngrp;
    const int tx0 = (btile % tiles_x) * TW, ty0 = (btile / tiles_x) * TH;
    const int T0 = (bwork - btile * ngrp) * CT;
    const int ns = a.src_bgroup > 0 ? n + n / a.src_bgroup : n;   // source batch item (ConvArgs::src_bgroup)
    const int H = a.H, W = a.W;

    // halo pixels of this thread: clamped coordinates (every load is unconditional and in range; pixels
    // outside the image are zeroed when the registers are converted, not when they are loaded)
    int cgy[NIN], cgx[NIN];
    bool sval[NIN];
#pragma unroll
    for (int t = 0; t < NIN; ++t) {
        const int idx = min(tid + 256 * t, NEL - 1);
        const int r = idx / LW, c = idx - r * LW;
        const int gy = ty0 + r - 1, gx = tx0 + c - 1;
        sval[t] = tid + 256 * t < NEL && gy >= 0 && gy < H && gx >= 0 && gx < W;
        cgy[t] = min(max(gy, 0), H - 1);
        cgx[t] = min(max(gx, 0), W - 1);
    }

    f32x16 acc[CT][PT], acl[CT][PT];   // acl: the 2^-11-scaled partial sums of the f16x3 scheme (dead for bf16x6)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int pt = 0; pt < PT; ++pt)
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc[ct][pt][e] = 0.0f; acl[ct][pt][e] = 0.0f; }
    {   // accumulators start at the bias: its loads are the first of the kernel and long landed when the MFMAs begin
        const float4* __restrict__ bp = reinterpret_cast<const float4*>(a.bpk);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 bq = bp[(T0 + ct) * 8 + 2 * g + h];
#pragma unroll
                for (int pt = 0; pt < PT; ++pt) {
                    acc[ct][pt][4 * g + 0] = bq.x; acc[ct][pt][4 * g + 1] = bq.y;
                    acc[ct][pt][4 * g + 2] = bq.z; acc[ct][pt][4 * g + 3] = bq.w;
                }
            }
    }

    const int nchunks = a.kq >> 2;
    const bf16x8* __restrict__ wp = reinterpret_cast<const bf16x8*>(NP == 3 ? a.wsplit : a.wsplit16);
    f32x4 rq0[NIN], rq1[NIN], rq2[NIN], rq3[NIN];   // the chunk's 4 quads of each of this thread's halo pixels
    bf16x8 rws[NWS];   // weights ride in the same prefetch batch: no global load (vmcnt is in-order!) may sit
                       // inside the MFMA loop, or every tap would wait for the whole input prefetch to land

    // Branch-free issue: each K-quad of the chunk is described by wave-uniform (base, row stride, column
    // stride, component mask); all source kinds share one load form.  Nothing between issue and the LDS
    // write touches a loaded register (a use, a zero-init or a copy forces s_waitcnt and serialises the
    // prefetch behind memory latency -- measured: 5.7k cycles per issue with conditional loads).
    const float* qb0; const float* qb1; const float* qb2; const float* qb3;
    int qrs0, qrs1, qrs2, qrs3, qcs0, qcs1, qcs2, qcs3, qm0 = 0, qm1 = 0, qm2 = 0, qm3 = 0;
#define CRFP_QDESC(QB, QRS, QCS, QM, QI, CH)                                                              \
    {                                                                                                     \
        const QuadDesc d_ = a.qd[4 * (CH) + (QI)];                                                        \
        QB = d_.base + (long long)ns * d_.bstride; QRS = d_.rs; QCS = d_.cs; QM = d_.mask;                \
    }
#define CRFP_SPLIT_ISSUE(CH)                                                                              \
    {                                                                                                     \
        CRFP_QDESC(qb0, qrs0, qcs0, qm0, 0, CH) CRFP_QDESC(qb1, qrs1, qcs1, qm1, 1, CH)                   \
        CRFP_QDESC(qb2, qrs2, qcs2, qm2, 2, CH) CRFP_QDESC(qb3, qrs3, qcs3, qm3, 3, CH)                   \
        _Pragma("unroll") for (int t = 0; t < NIN; ++t) {                                                 \
            rq0[t] = CRFP_LDACT(f32x4, qb0 + cgy[t] * qrs0 + cgx[t] * qcs0);                \
            rq1[t] = CRFP_LDACT(f32x4, qb1 + cgy[t] * qrs1 + cgx[t] * qcs1);                \
            rq2[t] = CRFP_LDACT(f32x4, qb2 + cgy[t] * qrs2 + cgx[t] * qcs2);                \
            rq3[t] = CRFP_LDACT(f32x4, qb3 + cgy[t] * qrs3 + cgx[t] * qcs3);                \
        }                                                                                                 \
        _Pragma("unroll") for (int k = 0; k < NWS; ++k) {                                                 \
            const int idx = min(tid + 256 * k, CT * WPC - 1);                                             \
            const int ct = idx / WPC, rem = idx - ct * WPC;                                               \
            rws[k] = wp[((long long)(T0 + ct) * nchunks + (CH)) * WPC + rem];                             \
        }                                                                                                 \
    }

    SB_STAMP_BEGIN
    CRFP_SPLIT_ISSUE(0)
    for (int ch = 0; ch < nchunks; ++ch) {
        const int m0 = qm0, m1 = qm1, m2 = qm2, m3 = qm3;  // component masks of the chunk now in registers
        __syncthreads();  // every wave finished reading the previous chunk
        SB_STAMP_LANDED
        if (NP == 2 && (m0 & 16)) {   // SRC_S3 chunk (wave-uniform): the producer already split it -- copy, zero outside the image
#pragma unroll
            for (int t = 0; t < NIN; ++t) {
                const int idx = tid + 256 * t;
                if (idx < NEL) {
                    const f32x4 z = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    tile[0][0][idx] = __builtin_bit_cast(bf16x8, sval[t] ? rq0[t] : z);        // (x0,  channels 0..7 of the chunk)
                    tile[0][1][idx] = __builtin_bit_cast(bf16x8, sval[t] ? rq1[t] : z);        // (x0,  channels 8..15)
                    tile[NP - 1][0][idx] = __builtin_bit_cast(bf16x8, sval[t] ? rq2[t] : z);   // (x1s, channels 0..7)
                    tile[NP - 1][1][idx] = __builtin_bit_cast(bf16x8, sval[t] ? rq3[t] : z);   // (x1s, channels 8..15)
                }
            }
        } else if (NP == 2 && (m0 & m1 & m2 & m3) == 15) {   // wave-uniform: every chunk but a ragged last one
#pragma unroll
            for (int t = 0; t < NIN; ++t) {
                const int idx = tid + 256 * t;
                if (idx < NEL) {
                    const float sc = sval[t] ? F16_RES_SCALE : 0.0f;
                    const unsigned km = sval[t] ? 0xffffffffu : 0u;
                    bf16x8 pa, pb;
                    split_f16x8_fast(rq0[t], rq1[t], sc, km, pa, pb);
                    tile[0][0][idx] = pa; tile[NP - 1][0][idx] = pb;
                    split_f16x8_fast(rq2[t], rq3[t], sc, km, pa, pb);
                    tile[0][1][idx] = pa; tile[NP - 1][1][idx] = pb;
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < NIN; ++t) {
                const int idx = tid + 256 * t;
                if (idx < NEL) {
                    bf16x8 pp[NP];
                    split_parts<NP>(mask_quad(rq0[t], sval[t] ? m0 : 0), mask_quad(rq1[t], sval[t] ? m1 : 0), pp);
#pragma unroll
                    for (int p = 0; p < NP; ++p) tile[p][0][idx] = pp[p];
                    split_parts<NP>(mask_quad(rq2[t], sval[t] ? m2 : 0), mask_quad(rq3[t], sval[t] ? m3 : 0), pp);
#pragma unroll
                    for (int p = 0; p < NP; ++p) tile[p][1][idx] = pp[p];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NWS; ++k) {
            const int idx = tid + 256 * k;
            if (idx < CT * WPC) (&wlds[0][0])[idx] = rws[k];
        }
        __syncthreads();
        SB_STAMP(tB)
        if (ch + 1 < nchunks) CRFP_SPLIT_ISSUE(ch + 1)
        SB_STAMP(tD)   // diagnostic: issue booked under D
#pragma unroll kSplitTapUnroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - 3 * ky;
            bf16x8 wa[CT][NP];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int p = 0; p < NP; ++p) wa[ct][p] = wlds[ct][(tap * NP + p) * 64 + lane];
#pragma unroll
            for (int pt = 0; pt < PT; ++pt) {
                const int pix = (wave * RPW + (pt >> 1) + ky) * LW + (pt & 1) * 32 + j + kx;
                bf16x8 bq[NP];
#pragma unroll
                for (int p = 0; p < NP; ++p) bq[p] = tile[p][h][pix];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) split_mfma<NP>(acc[ct][pt], acl[ct][pt], wa[ct], bq);
            }
        }
        SB_STAMP(tD)
    }
#undef CRFP_SPLIT_ISSUE
#undef CRFP_QDESC
    SB_STAMP_LOOP_END
    if (NP == 2) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int pt = 0; pt < PT; ++pt)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[ct][pt][e] += acl[ct][pt][e] * (1.0f / F16_RES_SCALE);
    }
    SB_STAMP_ACC_DONE
    const EpiCtx ec = epi_ctx(a, n);
    SB_STAMP_EPI_CTX
    conv_epilogue<CT, PT, RPW, 2>(ec, acc, T0, tx0, ty0, wave, j, h);
    SB_STAMP_EPI_DONE
}

template <int CT, int RPW, int NP>
__global__ __launch_bounds__(256, NP == 2 && CT == 1 && RPW == 1 ? 3 : 2) void conv3x3_split_kernel(const ConvArgs a) {
    conv3x3_split_body<CT, RPW, NP>(a, (int)blockIdx.x, (int)gridDim.x, (int)blockIdx.z);
}

#ifndef CRFP_ACT_BF16
// Round 6: TWO independent convs of the same shape in ONE launch (workgroups [0, w0) run plan a0, the rest plan a1; w0 is a multiple of 8, so a
// workgroup keeps its XCD).  The engine's two 32 -> 64 pixel-shuffle convs behind level 2 (the x4 upsample of the propagated features, dcn_3's
// pre-offset conv) are 1 800 four-wave workgroups each on the chip's 768 slots: 2.34 rounds paid as 3, twice; together 4.69 paid as 5
// (a lock-step batch of 4 clips shows the same arithmetic: 41.0 -> 34.7 us per clip).  Two streams cost more in fork / join than they save
// (profiles/r06_aux_stream_ab.txt).  Each plan's arithmetic is untouched: bit-identical.
template <int CT, int RPW, int NP>
__global__ __launch_bounds__(256, NP == 2 && CT == 1 && RPW == 1 ? 3 : 2) void conv3x3_split_dual_kernel(const ConvArgs a0, const ConvArgs a1, const int w0) {
    const bool second = (int)blockIdx.x >= w0;   // workgroup-uniform
    if (second) conv3x3_split_body<CT, RPW, NP>(a1, (int)blockIdx.x - w0, (int)gridDim.x - w0, (int)blockIdx.z);
    else conv3x3_split_body<CT, RPW, NP>(a0, (int)blockIdx.x, w0, (int)blockIdx.z);
}
#endif

// ---------------------------------------------------------------- f16x3, 8 waves, ONE accumulator ("f16x3s")
// The 4-wave kernel above needs 164 VGPRs (two fp32 accumulators per pixel tile, hi and lo) = 3 waves per SIMD = 768 workgroup
// slots, and a 360 x 640 map is 900 tiles: every 32-cout conv ran a full round plus a 17 % one.  Here the
// whole sum is kept scaled by 2^11 in ONE accumulator:
//     2^11 * x*w  ~=  x0 * A  +  x0 * B  +  x1s * C,    A = fp16(2^11 w),  B = fp16(2^11 (w - A/2^11)),  C = fp16(w)
// (x0 = fp16(x), x1s = fp16(2^11 (x - x0)) as before: same three MFMAs per tap, same exact products, same dropped term;
// the bias enters as 2^11 b and the result leaves through one multiply by 2^-11).  Three weight images instead of two,
// 32 VGPRs less; with 8 waves per workgroup (8 rows x 64 pixels, one weight image per 8 rows instead of per 4) the kernel
// fits 128 VGPRs: 2 workgroups = 16 waves per CU, 450 tiles on 512 slots -- one round.  Needs |w| < 32 (A must stay finite).
constexpr int S8_TH = 8;
constexpr int S8_WPC = 9 * 3 * 64;

// diagnostic timeline of conv3x3_split8_kernel (CRFP_STAMP_PTR / CRFP_STAMP_NAME, tools/stamp_conv8.py): absolute s_memtime of wave 0 at kernel
// entry, first tile in LDS, end of chunk 0's MFMAs, end of the MFMA loop, epilogue stores issued, stores acknowledged.  Lab library only.
#ifdef CRFP_LAB
#define S8_STAMP_BEGIN long long ts[6] = {0, 0, 0, 0, 0, 0}; if (a.stamps) ts[0] = __builtin_amdgcn_s_memtime();
#define S8_STAMP(I) if (a.stamps) ts[I] = __builtin_amdgcn_s_memtime();
#define S8_STAMP_ACC(I) if (a.stamps) { asm volatile("s_nop 0" ::"v"(acc[0][0][0]), "v"(acc[0][1][15])); ts[I] = __builtin_amdgcn_s_memtime(); }
#define S8_STAMP_END                                                                                      \
    if (a.stamps) {                                                                                       \
        ts[4] = __builtin_amdgcn_s_memtime();                                                             \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                  \
        ts[5] = __builtin_amdgcn_s_memtime();                                                             \
        if (tid == 0) {                                                                                   \
            long long* o = a.stamps + (long long)blockIdx.x * 8;                                          \
            for (int q = 0; q < 6; ++q) o[q] = ts[q];                                                     \
            o[6] = __builtin_amdgcn_s_getreg(6 << 11 | 4 << 6 | 20);   /* HW_REG_HW_ID (id 4), offset 0? -> unused placeholder */ \
            o[7] = 1;                                                                                     \
        }                                                                                                 \
    }
#else
#define S8_STAMP_BEGIN
#define S8_STAMP(I)
#define S8_STAMP_ACC(I)
#define S8_STAMP_END
#endif

// NW = 8: two workgroups per CU (the only form launched).  NW = 16 was an A/B build: ONE 16-row workgroup per CU -- the 27.6 KB
// weight stage is loaded once per CU instead of twice and the halo is 18 / 16 instead of 10 / 8 rows: 104 instead of 139 KB of ingest
// per CU and chunk (profiles/r03_conv_split8_timeline.txt: the prologue is ingest-bound).
template <int NW>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(4, 4))) void conv3x3_split8_kernel(const ConvArgs a) {
    constexpr int S8_NT = 64 * NW, S8_LH = NW + 2, S8_NEL = S8_LH * LW, S8_NIN = (S8_NEL + S8_NT - 1) / S8_NT;
    constexpr int S8_NWS = (S8_WPC + S8_NT - 1) / S8_NT;
    __shared__ bf16x8 tile[2][2][S8_NEL];        // [split part][quad pair][halo pixel]   42.2 KB (NW = 8)
    __shared__ bf16x8 wlds[S8_WPC];              // [(tap, image A/B/C)][lane]            27.6 KB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int tiles_x = (a.W + TW - 1) / TW;
    const int ngrp = a.ctiles;
    const int bwork = xcd_band_tile(blockIdx.x, gridDim.x);
    const int btile = bwork / ngrp;
    const int tx0 = (btile % tiles_x) * TW, ty0 = (btile / tiles_x) * NW;
    const int T0 = bwork - btile * ngrp;
    const int n = blockIdx.z;
    const int ns = a.src_bgroup > 0 ? n + n / a.src_bgroup : n;   // source batch item (ConvArgs::src_bgroup)
    const int H = a.H, W = a.W;
    S8_STAMP_BEGIN

    int cgy[S8_NIN], cgx[S8_NIN];
    bool sval[S8_NIN];
#pragma unroll
    for (int t = 0; t < S8_NIN; ++t) {
        const int idx = min(tid + S8_NT * t, S8_NEL - 1);
        const int r = idx / LW, c = idx - r * LW;
        const int gy = ty0 + r - 1, gx = tx0 + c - 1;
        sval[t] = tid + S8_NT * t < S8_NEL && gy >= 0 && gy < H && gx >= 0 && gx < W;
        cgy[t] = min(max(gy, 0), H - 1);
        cgx[t] = min(max(gx, 0), W - 1);
    }

    f32x16 acc[1][2];
    {   // accumulators start at 2^11 * bias
        const float4* __restrict__ bp = reinterpret_cast<const float4*>(a.bpk);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 bq = bp[T0 * 8 + 2 * g + h];
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) {
                acc[0][pt][4 * g + 0] = bq.x * F16_RES_SCALE; acc[0][pt][4 * g + 1] = bq.y * F16_RES_SCALE;
                acc[0][pt][4 * g + 2] = bq.z * F16_RES_SCALE; acc[0][pt][4 * g + 3] = bq.w * F16_RES_SCALE;
            }
        }
    }

    const int nchunks = a.kq >> 2;
    const bf16x8* __restrict__ wp = reinterpret_cast<const bf16x8*>(a.wsplit_sa);
    f32x4 rq0[S8_NIN], rq1[S8_NIN], rq2[S8_NIN], rq3[S8_NIN];
    bf16x8 rws[S8_NWS];
    const float* qb0; const float* qb1; const float* qb2; const float* qb3;
    int qrs0, qrs1, qrs2, qrs3, qcs0, qcs1, qcs2, qcs3, qm0 = 0, qm1 = 0, qm2 = 0, qm3 = 0;
#define CRFP_QDESC(QB_, QRS, QCS, QM, QI, CH)                                                             \
    {                                                                                                     \
        const QuadDesc d_ = a.qd[4 * (CH) + (QI)];                                                        \
        QB_ = d_.base + (long long)ns * d_.bstride; QRS = d_.rs; QCS = d_.cs; QM = d_.mask;                \
    }
#define CRFP_S8_ISSUE(CH)                                                                                 \
    {                                                                                                     \
        CRFP_QDESC(qb0, qrs0, qcs0, qm0, 0, CH) CRFP_QDESC(qb1, qrs1, qcs1, qm1, 1, CH)                   \
        CRFP_QDESC(qb2, qrs2, qcs2, qm2, 2, CH) CRFP_QDESC(qb3, qrs3, qcs3, qm3, 3, CH)                   \
        _Pragma("unroll") for (int t = 0; t < S8_NIN; ++t) {                                              \
            rq0[t] = CRFP_LDACT(f32x4, qb0 + cgy[t] * qrs0 + cgx[t] * qcs0);                \
            rq1[t] = CRFP_LDACT(f32x4, qb1 + cgy[t] * qrs1 + cgx[t] * qcs1);                \
            rq2[t] = CRFP_LDACT(f32x4, qb2 + cgy[t] * qrs2 + cgx[t] * qcs2);                \
            rq3[t] = CRFP_LDACT(f32x4, qb3 + cgy[t] * qrs3 + cgx[t] * qcs3);                \
        }                                                                                                 \
        _Pragma("unroll") for (int k = 0; k < S8_NWS; ++k) {                                              \
            const int idx = min(tid + S8_NT * k, S8_WPC - 1);                                             \
            rws[k] = wp[((long long)T0 * nchunks + (CH)) * S8_WPC + idx];                                 \
        }                                                                                                 \
    }

    CRFP_S8_ISSUE(0)
    for (int ch = 0; ch < nchunks; ++ch) {
        const int m0 = qm0, m1 = qm1, m2 = qm2, m3 = qm3;
        __syncthreads();
        if (m0 & 16) {   // SRC_S3 chunk (wave-uniform): already split by its producer -- copy, zero outside the image
#pragma unroll
            for (int t = 0; t < S8_NIN; ++t) {
                const int idx = tid + S8_NT * t;
                if (idx < S8_NEL) {
                    const f32x4 z = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    tile[0][0][idx] = __builtin_bit_cast(bf16x8, sval[t] ? rq0[t] : z);
                    tile[0][1][idx] = __builtin_bit_cast(bf16x8, sval[t] ? rq1[t] : z);
                    tile[1][0][idx] = __builtin_bit_cast(bf16x8, sval[t] ? rq2[t] : z);
                    tile[1][1][idx] = __builtin_bit_cast(bf16x8, sval[t] ? rq3[t] : z);
                }
            }
        } else if ((m0 & m1 & m2 & m3) == 15) {
#pragma unroll
            for (int t = 0; t < S8_NIN; ++t) {
                const int idx = tid + S8_NT * t;
                if (idx < S8_NEL) {
                    const float sc = sval[t] ? F16_RES_SCALE : 0.0f;
                    const unsigned km = sval[t] ? 0xffffffffu : 0u;
                    bf16x8 pa, pb;
                    split_f16x8_fast(rq0[t], rq1[t], sc, km, pa, pb);
                    tile[0][0][idx] = pa; tile[1][0][idx] = pb;
                    split_f16x8_fast(rq2[t], rq3[t], sc, km, pa, pb);
                    tile[0][1][idx] = pa; tile[1][1][idx] = pb;
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < S8_NIN; ++t) {
                const int idx = tid + S8_NT * t;
                if (idx < S8_NEL) {
                    bf16x8 pp[2];
                    split_parts<2>(mask_quad(rq0[t], sval[t] ? m0 : 0), mask_quad(rq1[t], sval[t] ? m1 : 0), pp);
                    tile[0][0][idx] = pp[0]; tile[1][0][idx] = pp[1];
                    split_parts<2>(mask_quad(rq2[t], sval[t] ? m2 : 0), mask_quad(rq3[t], sval[t] ? m3 : 0), pp);
                    tile[0][1][idx] = pp[0]; tile[1][1][idx] = pp[1];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < S8_NWS; ++k) {
            const int idx = tid + S8_NT * k;
            if (idx < S8_WPC) wlds[idx] = rws[k];
        }
        __syncthreads();
        if (ch == 0) { S8_STAMP(1) }
        if (ch + 1 < nchunks) CRFP_S8_ISSUE(ch + 1)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - 3 * ky;
            const f16x8 wA = __builtin_bit_cast(f16x8, wlds[(tap * 3 + 0) * 64 + lane]);
            const f16x8 wB = __builtin_bit_cast(f16x8, wlds[(tap * 3 + 1) * 64 + lane]);
            const f16x8 wC = __builtin_bit_cast(f16x8, wlds[(tap * 3 + 2) * 64 + lane]);
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) {
                const int pix = (wave + ky) * LW + pt * 32 + j + kx;
                const f16x8 b0 = __builtin_bit_cast(f16x8, tile[0][h][pix]);
                const f16x8 b1 = __builtin_bit_cast(f16x8, tile[1][h][pix]);
                acc[0][pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wB, b0, acc[0][pt], 0, 0, 0);
                acc[0][pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wC, b1, acc[0][pt], 0, 0, 0);
                acc[0][pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wA, b0, acc[0][pt], 0, 0, 0);
            }
        }
        if (ch == 0) { S8_STAMP_ACC(2) }
    }
    S8_STAMP_ACC(3)
#undef CRFP_S8_ISSUE
#undef CRFP_QDESC
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[0][pt][e] *= (1.0f / F16_RES_SCALE);
    const EpiCtx ec = epi_ctx(a, n);
    conv_epilogue<1, 2, 1, 2>(ec, acc, T0, tx0, ty0, wave, j, h);
    S8_STAMP_END
}

// ---------------------------------------------------------------- f16x3s: TWO 3x3 convs in one launch, the tensor between them in LDS
// The fp32 form of conv3x3_bf16_pair_kernel (further down; same scheme: conv A on the 10 x 64 region conv B's 8-row output tile needs,
// waves 0-3 three 32-pixel tiles, waves 4-7 two) with the arithmetic of conv3x3_split8_kernel: every accumulator sees the MFMAs of the
// stand-alone kernel in the same order, conv A's result goes through the stand-alone epilogue's arithmetic (2^-11, activation, post_scale,
// range guard on conv A's own status word) and then through split_f16x4 -- the values conv B's loader would form from the stored fp32
// tensor -- so the pair is bit-identical to the two launches.
// LDS is time-shared, 76 928 B = two workgroups per CU:
//   conv A, per chunk:  input halo [4 planes][12 x 64 + 2] x 16 B = 49 280  |  weight stage 27 648
//   conv B, per chunk:  ONE 16-channel half of the intermediate [4 planes][10 x 66] x 16 B = 42 240 in the dead halo  |  conv B's weight stage
// Conv A's accumulators wait in registers: couts 0-15 (registers 0-7 of each pixel tile) are written before conv B's chunk 0, couts 16-31
// before its chunk 1, into the same 42 KB.  Conv B's first weight stage rides under conv A's last chunk, its second under its own chunk 0.
// Registers (128 at 4 waves per SIMD, no scratch): 48 conv A accumulators and split8's even prefetch (32 halo + 16 weight registers per
// thread) do not fit.  So the output tile is 60 columns wide -- the input halo is then 12 x 64 pixels, one wave-row per prefetch slot, and the
// 640-wide map still takes 11 column tiles -- and the prefetch is divided by what a wave has left: waves 0-3 (three tiles) hold quads 0-1
// of every halo pixel and one weight slot (24 + 4 registers), waves 4-7 (two tiles) quads 2-3 and six weight slots (24 + 24).  Conv A's
// columns 62-63 read two pixels of the next halo row; they and everything outside the image are stored as exact zeros.
constexpr int PF_NT = 512, PF_OW = 60, PF_IH = 10, PF_IW = 64, PF_LH = 12, PF_LW = 64;
constexpr int PF_NEL = PF_LH * PF_LW, PF_PL = PF_NEL + 2;   // 768 input halo pixels; a plane ends with the two pixels the last row's taps overrun into
constexpr int PF_MP = PF_IW + 2, PF_MEL = PF_IH * PF_MP;    // intermediate rows of 64 + 2 zero columns
constexpr int PF_NWS = (S8_WPC + PF_NT - 1) / PF_NT;        // conv B's second weight stage: even slots
constexpr int PF_NWL = 1, PF_NWH = (S8_WPC - 256 * PF_NWL + 255) / 256;   // weight slots of a thread of waves 0-3 / waves 4-7
static_assert(PF_MEL <= PF_PL, "the intermediate half lives in the input halo's LDS");
static_assert(PF_NEL == 3 * 256, "three wave-rows per thread of either wave group");

struct PairB {          // what conv B adds to conv A's plan: its weights, bias, activation, destinations, residual, status word
    const void* wsplit_sa;
    const float* bpk;
    const float* resid;
    long long resid_bstride;
    ConvDst dst[CRFP_MAX_DST];
    int ndst, cout, act;
    float post_scale;
    float* s3_dst;
    long long s3_bstride;
    unsigned* ovf;
    int ovf_div, ovf_add, ovf_skip0;
};

// conv A's chunk loop for one wave group.  NTA = 3: waves 0-3, quads 0-1 of the halo, weight vectors [0, 256); NTA = 2: waves 4-7, quads 2-3,
// weight vectors [256, 1728).  Ends with conv B's first weight stage in wlds (fetched under the last chunk, staged behind the barrier
// that retires conv A's reads).  Thread (wave & 3, lane) holds halo pixels (row (wave & 3) + 4 t, column lane), t = 0..2.
template <int NTA>
__device__ __forceinline__ void pair_conv_a(const ConvArgs& a, const bf16x8* __restrict__ wpb, int ns, int ty0, int tx0, int tid, int lane, int wave,
                                            bf16x8* tile, bf16x8* wlds, f32x16 (&accA)[3]) {
    constexpr int P = NTA == 3 ? 0 : 1, NW = NTA == 3 ? PF_NWL : PF_NWH;
    const int j = lane & 31, h = lane >> 5;
    const int H = a.H, W = a.W;
    const int gx = tx0 + lane - 2, cgx = min(max(gx, 0), W - 1);
    const int w3 = wave & 3;
    const int widx0 = tid;   // weight vector of slot k: tid + 256 k (waves 4-7: tid >= 256)
    const int nchunks = a.kq >> 2;
    const bf16x8* __restrict__ wp = reinterpret_cast<const bf16x8*>(a.wsplit_sa);
    {   // accumulators start at 2^11 * bias
        const float4* __restrict__ bp = reinterpret_cast<const float4*>(a.bpk);
        int hb = h;   // opaque copy: the two wave groups' loads stay inside their own paths
        asm volatile("" : "+v"(hb));
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 bq = bp[2 * g + hb];
#pragma unroll
            for (int k = 0; k < NTA; ++k) {
                accA[k][4 * g + 0] = bq.x * F16_RES_SCALE; accA[k][4 * g + 1] = bq.y * F16_RES_SCALE;
                accA[k][4 * g + 2] = bq.z * F16_RES_SCALE; accA[k][4 * g + 3] = bq.w * F16_RES_SCALE;
            }
        }
    }
    f32x4 rqa[3], rqb[3];
    bf16x8 rws[NW];
    int m0 = 0, m1 = 0, m2 = 0, m3 = 0;
#define CRFP_PA_WEIGHTS(WP, CH)                                                                           \
    _Pragma("unroll") for (int k = 0; k < NW; ++k)                                                        \
        rws[k] = (WP)[(long long)(CH) * S8_WPC + min(widx0 + 256 * k, S8_WPC - 1)];
#define CRFP_PA_ISSUE(CH)                                                                                 \
    {                                                                                                     \
        const QuadDesc da_ = a.qd[4 * (CH) + 2 * P], db_ = a.qd[4 * (CH) + 2 * P + 1];                    \
        const float* qa_ = da_.base + (long long)ns * da_.bstride;                                        \
        const float* qb_ = db_.base + (long long)ns * db_.bstride;                                        \
        m0 = a.qd[4 * (CH)].mask; m1 = a.qd[4 * (CH) + 1].mask; m2 = a.qd[4 * (CH) + 2].mask; m3 = a.qd[4 * (CH) + 3].mask; \
        _Pragma("unroll") for (int t = 0; t < 3; ++t) {                                                   \
            const int cgy = min(max(ty0 + w3 + 4 * t - 2, 0), H - 1);                                     \
            rqa[t] = CRFP_LDACT(f32x4, qa_ + cgy * da_.rs + cgx * da_.cs);                                \
            rqb[t] = CRFP_LDACT(f32x4, qb_ + cgy * db_.rs + cgx * db_.cs);                                \
        }                                                                                                 \
        CRFP_PA_WEIGHTS(wp, CH)                                                                           \
    }
#define CRFP_PA_STAGE_WEIGHTS                                                                             \
    _Pragma("unroll") for (int k = 0; k < NW; ++k) {                                                      \
        const int idx = widx0 + 256 * k;                                                                  \
        if (idx < S8_WPC) wlds[idx] = rws[k];                                                             \
    }

    CRFP_PA_ISSUE(0)
    int ch = 0;
    do {   // (at least one chunk: no zero-trip path for the compiler to carry registers through)
        const int c0 = m0, c1 = m1, c2 = m2, c3 = m3;
        const int ma = P ? c2 : c0, mb = P ? c3 : c1;
        __syncthreads();
        int ls = lane;   // opaque copy: the staging addresses are recomputed per chunk instead of living through the MFMA loop
        asm volatile("" : "+v"(ls));
        const int gxs = tx0 + ls - 2;
        const bool xin = gxs >= 0 && gxs < W;
        if (c0 & 16) {   // SRC_S3 chunk (wave-uniform): already split by its producer -- copy, zero outside the image.  Quads 0-1: the x0 image
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int r = w3 + 4 * t, gy = ty0 + r - 2, idx = r * PF_LW + ls;
                const bool v = xin && gy >= 0 && gy < H;
                const f32x4 z = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                tile[(2 * P + 0) * PF_PL + idx] = __builtin_bit_cast(bf16x8, v ? rqa[t] : z);
                tile[(2 * P + 1) * PF_PL + idx] = __builtin_bit_cast(bf16x8, v ? rqb[t] : z);
            }
        } else if ((c0 & c1 & c2 & c3) == 15) {
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int r = w3 + 4 * t, gy = ty0 + r - 2, idx = r * PF_LW + ls;
                const bool v = xin && gy >= 0 && gy < H;
                const float sc = v ? F16_RES_SCALE : 0.0f;
                const unsigned km = v ? 0xffffffffu : 0u;
                bf16x8 pa, pb;
                split_f16x8_fast(rqa[t], rqb[t], sc, km, pa, pb);
                tile[(0 + P) * PF_PL + idx] = pa; tile[(2 + P) * PF_PL + idx] = pb;
            }
        } else {
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int r = w3 + 4 * t, gy = ty0 + r - 2, idx = r * PF_LW + ls;
                const bool v = xin && gy >= 0 && gy < H;
                bf16x8 pp[2];
                split_parts<2>(mask_quad(rqa[t], v ? ma : 0), mask_quad(rqb[t], v ? mb : 0), pp);
                tile[(0 + P) * PF_PL + idx] = pp[0]; tile[(2 + P) * PF_PL + idx] = pp[1];
            }
        }
        CRFP_PA_STAGE_WEIGHTS
        __syncthreads();
        if (ch + 1 < nchunks) CRFP_PA_ISSUE(ch + 1)
        else CRFP_PA_WEIGHTS(wpb, 0)   // conv B's first weight stage rides under conv A's last chunk
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - 3 * ky;
            const f16x8 wA = __builtin_bit_cast(f16x8, wlds[(tap * 3 + 0) * 64 + lane]);
            const f16x8 wB = __builtin_bit_cast(f16x8, wlds[(tap * 3 + 1) * 64 + lane]);
            const f16x8 wC = __builtin_bit_cast(f16x8, wlds[(tap * 3 + 2) * 64 + lane]);
#pragma unroll
            for (int k = 0; k < NTA; ++k) {
                const int t = wave + 8 * k;   // tile t of the 10 x 64 region: row t >> 1, half t & 1
                const int pix = ((t >> 1) + ky) * PF_LW + (t & 1) * 32 + j + kx;
                const f16x8 b0 = __builtin_bit_cast(f16x8, tile[(0 + h) * PF_PL + pix]);
                const f16x8 b1 = __builtin_bit_cast(f16x8, tile[(2 + h) * PF_PL + pix]);
                accA[k] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wB, b0, accA[k], 0, 0, 0);
                accA[k] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wC, b1, accA[k], 0, 0, 0);
                accA[k] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wA, b0, accA[k], 0, 0, 0);
            }
        }
    } while (++ch < nchunks);
    __syncthreads();   // every wave finished conv A's last chunk: the halo and the weight stage are dead
    CRFP_PA_STAGE_WEIGHTS
    if (NTA == 2) {   // never read (the caller's loops stop at the wave's tile count): defined, and not live during the chunk loop
#pragma unroll
        for (int e = 0; e < 16; ++e) accA[2][e] = 0.0f;
    }
#undef CRFP_PA_ISSUE
#undef CRFP_PA_WEIGHTS
#undef CRFP_PA_STAGE_WEIGHTS
}

__global__ __launch_bounds__(PF_NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void conv3x3_pair_kernel(const ConvArgs a, const PairB b) {
    __shared__ bf16x8 tile[4 * PF_PL];           // conv A: planes [x0 | x1s][quad pair] of the input halo; conv B: the same planes of one intermediate half, PF_MEL each
    __shared__ bf16x8 wlds[S8_WPC];              // [(tap, image A/B/C)][lane] of the current chunk of conv A, then of conv B
    const int tid0 = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);   // wave-uniform to the compiler as well
    const int tiles_x = (a.W + PF_OW - 1) / PF_OW;
    const int btile = xcd_band_tile(blockIdx.x, gridDim.x);
    const int tx0 = (btile % tiles_x) * PF_OW, ty0 = (btile / tiles_x) * 8;
    const int n = blockIdx.z;
    const int ns = a.src_bgroup > 0 ? n + n / a.src_bgroup : n;   // source batch item (ConvArgs::src_bgroup)
    const int H = a.H, W = a.W;

    const int ntA = wave < 4 ? 3 : 2;
    f32x16 accA[3];   // (initialised per wave group: the third tile's registers carry the prefetch of waves 4-7 during conv A)
    const bf16x8* __restrict__ wpb = reinterpret_cast<const bf16x8*>(b.wsplit_sa);
    if (tid0 < 8) tile[(tid0 >> 1) * PF_PL + PF_NEL + (tid0 & 1)] = __builtin_bit_cast(bf16x8, f32x4{0.0f, 0.0f, 0.0f, 0.0f});   // the planes' overrun pixels
    if (wave < 4) pair_conv_a<3>(a, wpb, ns, ty0, tx0, tid0, tid0 & 63, wave, tile, wlds, accA);
    else pair_conv_a<2>(a, wpb, ns, ty0, tx0, tid0, tid0 & 63, wave, tile, wlds, accA);
    int tid = tid0;   // opaque copy: what the rest derives from it is computed here, not carried through conv A's loop
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, j = lane & 31, h = lane >> 5;

    // conv A's epilogue into LDS, one 16-channel half (cout quads 4 * half .. + 3 = accumulator registers 8 * half .. + 7) at a time: the
    // stand-alone epilogue's arithmetic (VBIAS = 2: the bias is in the accumulator, `+ 0` is its bias add), exact zero outside the image
    // (conv B's zero padding pads A's output) and in the two columns no stored output reads, the range guard over what the stand-alone
    // launch would store, then the split conv B's loader applies to an fp32 Q4 source.  Channel 8 g + 4 h + r is position 4 h + r of the
    // 8-channel element (quad pair g & 1) of its half.
    bf16x8* const mid = tile;   // [x0 | x1s][quad pair][PF_MEL]
    const float slopeA = a.act == CRFP_ACT_RELU ? 0.0f : (a.act == CRFP_ACT_LRELU01 ? 0.1f : 1.0f);
    const float postA = a.post_scale;
    float vmaxA = 0.0f;
#define CRFP_PF_MID(HALF)                                                                                 \
    _Pragma("unroll") for (int k = 0; k < 3; ++k) {                                                       \
        if (k == 2 && ntA == 2) break;                                                                    \
        const int t = wave + 8 * k, r = t >> 1, c = (t & 1) * 32 + j;                                     \
        const int gy = ty0 + r - 1, gx = tx0 + c - 1;                                                     \
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W && c < PF_OW + 2;                          \
        _Pragma("unroll") for (int gg = 0; gg < 2; ++gg) {                                                \
            const int g = 2 * (HALF) + gg;                                                                \
            float v[4];                                                                                   \
            _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                               \
                const float x = accA[k][4 * g + e] * (1.0f / F16_RES_SCALE) + 0.0f;                       \
                v[e] = in ? fmaxf(x, slopeA * x) * postA : 0.0f;                                          \
            }                                                                                             \
            vmaxA = fmaxf(fmaxf(vmaxA, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3]))); \
            unsigned hi2[2], lo2[2];                                                                      \
            split_f16x4(v, hi2, lo2);                                                                     \
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));                                   \
            *(reinterpret_cast<u32x2*>(&mid[(0 + gg) * PF_MEL + r * PF_MP + c]) + h) = u32x2{hi2[0], hi2[1]}; \
            *(reinterpret_cast<u32x2*>(&mid[(2 + gg) * PF_MEL + r * PF_MP + c]) + h) = u32x2{lo2[0], lo2[1]}; \
        }                                                                                                 \
    }
#define CRFP_PF_WEIGHTS(WP, CH)                                                                           \
    _Pragma("unroll") for (int k = 0; k < PF_NWS; ++k)                                                    \
        rws[k] = (WP)[(long long)(CH) * S8_WPC + min(tid + PF_NT * k, S8_WPC - 1)];
#define CRFP_PF_STAGE_WEIGHTS                                                                             \
    _Pragma("unroll") for (int k = 0; k < PF_NWS; ++k) {                                                  \
        const int idx = tid + PF_NT * k;                                                                  \
        if (idx < S8_WPC) wlds[idx] = rws[k];                                                             \
    }

    // (pair_conv_a ended behind the barrier that retires conv A's LDS reads, with conv B's chunk 0 weights staged)
    CRFP_PF_MID(0)
    if (tid < 4 * PF_IH * 2) {   // the two zero columns behind each intermediate row (read by conv B's taps of discarded output columns only)
        const int pl = tid / (PF_IH * 2), rc = tid - pl * (PF_IH * 2);
        mid[pl * PF_MEL + (rc >> 1) * PF_MP + PF_IW + (rc & 1)] = __builtin_bit_cast(bf16x8, f32x4{0.0f, 0.0f, 0.0f, 0.0f});
    }
    f32x16 acc[1][2];
    {   // conv B's accumulators start at 2^11 * bias
        const float4* __restrict__ bp = reinterpret_cast<const float4*>(b.bpk);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 bq = bp[2 * g + h];
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) {
                acc[0][pt][4 * g + 0] = bq.x * F16_RES_SCALE; acc[0][pt][4 * g + 1] = bq.y * F16_RES_SCALE;
                acc[0][pt][4 * g + 2] = bq.z * F16_RES_SCALE; acc[0][pt][4 * g + 3] = bq.w * F16_RES_SCALE;
            }
        }
    }
    __syncthreads();
    bf16x8 rws[PF_NWS];
    CRFP_PF_WEIGHTS(wpb, 1)
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
        if (c2 == 1) {
            __syncthreads();   // every wave finished conv B's chunk 0
            CRFP_PF_MID(1)
            CRFP_PF_STAGE_WEIGHTS
            __syncthreads();
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - 3 * ky;
            const f16x8 wA = __builtin_bit_cast(f16x8, wlds[(tap * 3 + 0) * 64 + lane]);
            const f16x8 wB = __builtin_bit_cast(f16x8, wlds[(tap * 3 + 1) * 64 + lane]);
            const f16x8 wC = __builtin_bit_cast(f16x8, wlds[(tap * 3 + 2) * 64 + lane]);
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) {
                const int pix = (wave + ky) * PF_MP + pt * 32 + j + kx;
                const f16x8 b0 = __builtin_bit_cast(f16x8, mid[(0 + h) * PF_MEL + pix]);
                const f16x8 b1 = __builtin_bit_cast(f16x8, mid[(2 + h) * PF_MEL + pix]);
                acc[0][pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wB, b0, acc[0][pt], 0, 0, 0);
                acc[0][pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wC, b1, acc[0][pt], 0, 0, 0);
                acc[0][pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wA, b0, acc[0][pt], 0, 0, 0);
            }
        }
    }
#undef CRFP_PF_MID
#undef CRFP_PF_STAGE_WEIGHTS
#undef CRFP_PF_WEIGHTS
    {   // conv A's range guard, on the word the stand-alone launch raises
        unsigned* const ovfA = ovf_word(a.ovf, a.ovf_div, a.ovf_add, n, a.ovf_skip0);
        if (ovfA && !(vmaxA < 65504.0f)) atomicOr(ovfA, 1u);
    }
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[0][pt][e] *= (1.0f / F16_RES_SCALE);
    // conv B's epilogue: the shared one, on conv B's destinations / residual / activation / status word, PF_OW columns per tile
    ConvArgs eb = a;
    eb.cout = b.cout; eb.act = b.act; eb.post_scale = b.post_scale; eb.store = ST_Q4; eb.ps_r = 0;
    eb.resid = b.resid; eb.resid_bstride = b.resid_bstride; eb.s3_dst = b.s3_dst; eb.s3_bstride = b.s3_bstride; eb.dst_f32 = 0; eb.ndst = b.ndst;
    eb.ovf = b.ovf; eb.ovf_div = b.ovf_div; eb.ovf_add = b.ovf_add; eb.ovf_skip0 = b.ovf_skip0;
#pragma unroll
    for (int d = 0; d < CRFP_MAX_DST; ++d) eb.dst[d] = b.dst[d];
    EpiCtx ec = epi_ctx(eb, n);
    ec.xend = min(W, tx0 + PF_OW);
    conv_epilogue<1, 2, 1, 2>(ec, acc, 0, tx0, ty0, wave, j, h);
}

#endif  // !CRFP_ACT_BF16

#ifdef CRFP_ACT_BF16
// ================================================================ bf16-storage main loop
// Activations arrive as bf16 pixel quads (8 bytes): the halo tile is COPIED into one bf16 LDS image (no conversion, no
// split), weights are bf16 (rounded once at pack time), one v_mfma_f32_32x32x16_bf16 per (tap, 16-channel chunk,
// 32-pixel tile) with fp32 accumulators that start at the fp32 bias.  Same tile shape, lane map, K order and epilogue as
// conv3x3_split_kernel<1,1,2> of the fp32 build.  The only fp32 operand left is the flow field of dcn_block.0
// (SRC_FLOW2, QuadDesc::mask bit 5): its (dx, dy) pair has the width of a bf16 quad and is rounded to bf16 on the way
// into LDS.  LDS 22 KB per workgroup.
__device__ __forceinline__ unsigned pack_bf16x2(float a, float b) {
    typedef __bf16 h2_t __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(unsigned, __builtin_convertvector(cf32x2{a, b}, h2_t));
}
// one raw 8-byte K-quad -> its two packed bf16 words; m = component mask (bit 5: fp32 (dx, dy) pair)
__device__ __forceinline__ cu32x2 quad_words(cu32x2 r, int m, bool valid) {
    if (!valid) return cu32x2{0u, 0u};
    if (m & 32) {   // (per-component bit casts of r.x / r.y were folded into pack(x, x) by hipcc 7.2: cast the whole pair)
        typedef __bf16 h2_t __attribute__((ext_vector_type(2)));
        return cu32x2{__builtin_bit_cast(unsigned, __builtin_convertvector(__builtin_bit_cast(cf32x2, r), h2_t)), 0u};
    }
    const unsigned k0 = ((m & 1) ? 0x0000ffffu : 0u) | ((m & 2) ? 0xffff0000u : 0u);
    const unsigned k1 = ((m & 4) ? 0x0000ffffu : 0u) | ((m & 8) ? 0xffff0000u : 0u);
    return cu32x2{r.x & k0, r.y & k1};
}

// ---------------------------------------------------------------- chunk staging shared by the 8-wave and the pair kernel
// Both are: their tile decode | halo_coords | acc_from_bias | per 16-channel chunk { ChunkQuads::fetch + the load batch + issue_weights into
// registers; stage_bf16 + stage_weights into LDS; their own MFMA tap loop } | conv_epilogue.  Templates on the kernel's thread count NT,
// halo size NEL and halo slots per thread NIN, so each kernel keeps its own constants.
// The other main loops (conv3x3_split_body, conv3x3_split8_kernel, conv3x3_bf16_kernel) carry the same pieces as their own text: written
// with these helpers they computed the same bits at the same registers, LDS and occupancy, but hipcc scheduled them differently and
// their launch sites came out 0.3 - 1.5 % slower (profiles/r13_conv_stage_ab.txt), so their instruction streams stay as they were.

// halo pixels of this thread (rows of LW pixels, origin (ty0 - 1, tx0 - 1)): clamped coordinates -- every load is unconditional and in
// range; pixels outside the image (sval false) are zeroed when the registers are converted, not when they are loaded
template <int NT, int NEL, int NIN>
__device__ __forceinline__ void halo_coords(int tid, int ty0, int tx0, int H, int W, int (&cgy)[NIN], int (&cgx)[NIN], bool (&sval)[NIN]) {
#pragma unroll
    for (int t = 0; t < NIN; ++t) {
        const int idx = min(tid + NT * t, NEL - 1);
        const int r = idx / LW, c = idx - r * LW;
        const int gy = ty0 + r - 1, gx = tx0 + c - 1;
        sval[t] = tid + NT * t < NEL && gy >= 0 && gy < H && gx >= 0 && gx < W;
        cgy[t] = min(max(gy, 0), H - 1);
        cgx[t] = min(max(gx, 0), W - 1);
    }
}

// Branch-free issue: each K-quad of the chunk is described by wave-uniform (base, row stride, column
// stride, component mask); all source kinds share one load form.  Nothing between issue and the LDS
// write touches a loaded register (a use, a zero-init or a copy forces s_waitcnt and serialises the
// prefetch behind memory latency -- measured: 5.7k cycles per issue with conditional loads).
// The chunk's weights ride in the same prefetch batch: no global load (vmcnt is in-order!) may sit
// inside the MFMA loop, or every tap would wait for the whole input prefetch to land.
struct ChunkQuads {
    const float* base[4];
    int rs[4], cs[4], mask[4];
    __device__ __forceinline__ void fetch(const ConvArgs& a, int ns, int ch) {   // the 4 quad descriptors of chunk ch, source item ns
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const QuadDesc d = a.qd[4 * ch + q];
            base[q] = d.base + (long long)ns * d.bstride; rs[q] = d.rs; cs[q] = d.cs; mask[q] = d.mask;
        }
    }
};
// the NV weight vectors at wp (one chunk of one cout tile, or consecutive ones), index clamped: always a valid load
template <int NT, int NV, int NWS>
__device__ __forceinline__ void issue_weights(bf16x8 (&rws)[NWS], const bf16x8* __restrict__ wp, int tid) {
#pragma unroll
    for (int k = 0; k < NWS; ++k) rws[k] = wp[min(tid + NT * k, NV - 1)];
}
template <int NT, int NV, int NWS>
__device__ __forceinline__ void stage_weights(bf16x8* wlds, const bf16x8 (&rws)[NWS], int tid) {
#pragma unroll
    for (int k = 0; k < NWS; ++k) {
        const int idx = tid + NT * k;
        if (idx < NV) wlds[idx] = rws[k];
    }
}

// the PT accumulators of cout tile T start at the bias: its loads are the first of the kernel and long landed when the MFMAs begin
template <int PT>
__device__ __forceinline__ void acc_from_bias(f32x16 (&acc)[PT], const float* bpk, int T, int h) {
    const float4* __restrict__ bp = reinterpret_cast<const float4*>(bpk);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 bq = bp[T * 8 + 2 * g + h];
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) {
            acc[pt][4 * g + 0] = bq.x; acc[pt][4 * g + 1] = bq.y;
            acc[pt][4 * g + 2] = bq.z; acc[pt][4 * g + 3] = bq.w;
        }
    }
}

// registers -> the bf16 halo image in LDS ([quad pair][halo pixel], 8 bf16 = 16 B each): a plain copy where the chunk holds 16 real bf16
// channels (wave-uniform), quad_words otherwise; zero outside the image
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
template <int NT, int NEL, int NIN>
__device__ __forceinline__ void stage_bf16(u32x4_t (&tile)[2][NEL], const cu32x2 (&rq)[4][NIN], const int (&m)[4], const bool (&sval)[NIN], int tid) {
    if ((m[0] & m[1] & m[2] & m[3]) == 15 && !((m[0] | m[1] | m[2] | m[3]) & 32)) {
#pragma unroll
        for (int t = 0; t < NIN; ++t) {
            const int idx = tid + NT * t;
            if (idx < NEL) {
                const unsigned km = sval[t] ? 0xffffffffu : 0u;
                tile[0][idx] = u32x4_t{rq[0][t].x & km, rq[0][t].y & km, rq[1][t].x & km, rq[1][t].y & km};
                tile[1][idx] = u32x4_t{rq[2][t].x & km, rq[2][t].y & km, rq[3][t].x & km, rq[3][t].y & km};
            }
        }
    } else {
#pragma unroll
        for (int t = 0; t < NIN; ++t) {
            const int idx = tid + NT * t;
            if (idx < NEL) {
                const cu32x2 w0 = quad_words(rq[0][t], m[0], sval[t]), w1 = quad_words(rq[1][t], m[1], sval[t]);
                const cu32x2 w2 = quad_words(rq[2][t], m[2], sval[t]), w3 = quad_words(rq[3][t], m[3], sval[t]);
                tile[0][idx] = u32x4_t{w0.x, w0.y, w1.x, w1.y};
                tile[1][idx] = u32x4_t{w2.x, w2.y, w3.x, w3.y};
            }
        }
    }
}

constexpr int kBf16Lb = 5;   // workgroups per CU the register allocation aims at.  Round 4, same box, 4-clip lock-step batch: 4 -> 5 takes the kernel
                             // sum per clip 5.67 -> 5.60 ms (32 -> 32 convs 9.4 -> 8.9 us), one-clip calls unchanged; 6 spills (40 B) and loses 6 %
template <int RPW>
__global__ __launch_bounds__(256, RPW == 1 ? kBf16Lb : 3) void conv3x3_bf16_kernel(const ConvArgs a) {
    constexpr int CT = 1, TH = 4 * RPW, LH = TH + 2, PT = 2 * RPW;
    constexpr int NEL = LH * LW;                 // halo pixels
    constexpr int NIN = (NEL + 255) / 256;       // halo pixels per thread; each carries the chunk's 4 quads
    constexpr int WPC = 9 * 64;                  // weight vectors per (cout tile, chunk)
    constexpr int NWS = (WPC + 255) / 256;
    __shared__ u32x4_t tile[2][NEL];             // [quad pair][halo pixel]: 8 bf16 = 16 B
    __shared__ bf16x8 wlds[WPC];                 // [tap][lane]: this chunk's A fragments
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int tiles_x = (a.W + TW - 1) / TW;
    const int ngrp = a.ctiles;
    const int bwork = xcd_band_tile(blockIdx.x, gridDim.x);
    const int btile = bwork / ngrp;
    const int tx0 = (btile % tiles_x) * TW, ty0 = (btile / tiles_x) * TH;
    const int T0 = bwork - btile * ngrp;
    const int n = blockIdx.z;
    const int ns = a.src_bgroup > 0 ? n + n / a.src_bgroup : n;   // source batch item (ConvArgs::src_bgroup)
    const int H = a.H, W = a.W;

    int cgy[NIN], cgx[NIN];
    bool sval[NIN];
#pragma unroll
    for (int t = 0; t < NIN; ++t) {
        const int idx = min(tid + 256 * t, NEL - 1);
        const int r = idx / LW, c = idx - r * LW;
        const int gy = ty0 + r - 1, gx = tx0 + c - 1;
        sval[t] = tid + 256 * t < NEL && gy >= 0 && gy < H && gx >= 0 && gx < W;
        cgy[t] = min(max(gy, 0), H - 1);
        cgx[t] = min(max(gx, 0), W - 1);
    }

    f32x16 acc[CT][PT];
    {   // accumulators start at the bias
        const float4* __restrict__ bp = reinterpret_cast<const float4*>(a.bpk);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 bq = bp[T0 * 8 + 2 * g + h];
#pragma unroll
            for (int pt = 0; pt < PT; ++pt) {
                acc[0][pt][4 * g + 0] = bq.x; acc[0][pt][4 * g + 1] = bq.y;
                acc[0][pt][4 * g + 2] = bq.z; acc[0][pt][4 * g + 3] = bq.w;
            }
        }
    }

    const int nchunks = a.kq >> 2;
    const bf16x8* __restrict__ wp = reinterpret_cast<const bf16x8*>(a.wsplit16);
    cu32x2 rq0[NIN], rq1[NIN], rq2[NIN], rq3[NIN];
    bf16x8 rws[NWS];
    const float* qb0; const float* qb1; const float* qb2; const float* qb3;
    int qrs0, qrs1, qrs2, qrs3, qcs0, qcs1, qcs2, qcs3, qm0 = 0, qm1 = 0, qm2 = 0, qm3 = 0;
#define CRFP_QDESC(QB_, QRS, QCS, QM, QI, CH)                                                             \
    {                                                                                                     \
        const QuadDesc d_ = a.qd[4 * (CH) + (QI)];                                                        \
        QB_ = d_.base + (long long)ns * d_.bstride; QRS = d_.rs; QCS = d_.cs; QM = d_.mask;                \
    }
#define CRFP_BF16_ISSUE(CH)                                                                               \
    {                                                                                                     \
        CRFP_QDESC(qb0, qrs0, qcs0, qm0, 0, CH) CRFP_QDESC(qb1, qrs1, qcs1, qm1, 1, CH)                   \
        CRFP_QDESC(qb2, qrs2, qcs2, qm2, 2, CH) CRFP_QDESC(qb3, qrs3, qcs3, qm3, 3, CH)                   \
        _Pragma("unroll") for (int t = 0; t < NIN; ++t) {                                                 \
            rq0[t] = CRFP_LDACT(cu32x2, qb0 + cgy[t] * qrs0 + cgx[t] * qcs0);               \
            rq1[t] = CRFP_LDACT(cu32x2, qb1 + cgy[t] * qrs1 + cgx[t] * qcs1);               \
            rq2[t] = CRFP_LDACT(cu32x2, qb2 + cgy[t] * qrs2 + cgx[t] * qcs2);               \
            rq3[t] = CRFP_LDACT(cu32x2, qb3 + cgy[t] * qrs3 + cgx[t] * qcs3);               \
        }                                                                                                 \
        _Pragma("unroll") for (int k = 0; k < NWS; ++k) {                                                 \
            const int idx = min(tid + 256 * k, WPC - 1);                                                  \
            rws[k] = wp[((long long)T0 * nchunks + (CH)) * WPC + idx];                                    \
        }                                                                                                 \
    }

    CRFP_BF16_ISSUE(0)
    for (int ch = 0; ch < nchunks; ++ch) {
        const int m0 = qm0, m1 = qm1, m2 = qm2, m3 = qm3;
        __syncthreads();  // every wave finished reading the previous chunk
        if ((m0 & m1 & m2 & m3) == 15 && !((m0 | m1 | m2 | m3) & 32)) {   // wave-uniform: 16 real bf16 channels -> plain copy
#pragma unroll
            for (int t = 0; t < NIN; ++t) {
                const int idx = tid + 256 * t;
                if (idx < NEL) {
                    const unsigned km = sval[t] ? 0xffffffffu : 0u;
                    tile[0][idx] = u32x4_t{rq0[t].x & km, rq0[t].y & km, rq1[t].x & km, rq1[t].y & km};
                    tile[1][idx] = u32x4_t{rq2[t].x & km, rq2[t].y & km, rq3[t].x & km, rq3[t].y & km};
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < NIN; ++t) {
                const int idx = tid + 256 * t;
                if (idx < NEL) {
                    const cu32x2 w0 = quad_words(rq0[t], m0, sval[t]), w1 = quad_words(rq1[t], m1, sval[t]);
                    const cu32x2 w2 = quad_words(rq2[t], m2, sval[t]), w3 = quad_words(rq3[t], m3, sval[t]);
                    tile[0][idx] = u32x4_t{w0.x, w0.y, w1.x, w1.y};
                    tile[1][idx] = u32x4_t{w2.x, w2.y, w3.x, w3.y};
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NWS; ++k) {
            const int idx = tid + 256 * k;
            if (idx < WPC) wlds[idx] = rws[k];
        }
        __syncthreads();
        if (ch + 1 < nchunks) CRFP_BF16_ISSUE(ch + 1)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - 3 * ky;
            const bf16x8 wa = wlds[tap * 64 + lane];
#pragma unroll
            for (int pt = 0; pt < PT; ++pt) {
                const int pix = (wave * RPW + (pt >> 1) + ky) * LW + (pt & 1) * 32 + j + kx;
                const bf16x8 bq = __builtin_bit_cast(bf16x8, tile[h][pix]);
                acc[0][pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa, bq, acc[0][pt], 0, 0, 0);
            }
        }
    }
#undef CRFP_BF16_ISSUE
#undef CRFP_QDESC
    const EpiCtx ec = epi_ctx(a, n);
    conv_epilogue<CT, PT, RPW, 2>(ec, acc, T0, tx0, ty0, wave, j, h);
}

// ---------------------------------------------------------------- bf16 storage, 8 waves, two chunks per stage
// The 32-cout layers (one cout tile): workgroup = 8 rows x 64 pixels (wave = one row, two 32-pixel tiles), 450 workgroups for a
// 360 x 640 map = one round at two per CU, and 32 input channels (two 16-channel chunks: tile 42 KB + weights 18 KB) per barrier
// pair -- a 32 -> 32 conv has ONE staging phase instead of two, a 64 -> 32 conv two instead of four.  Same K order, same
// accumulate order per accumulator (chunk-major, taps inside) and the same epilogue as conv3x3_bf16_kernel: identical values.
constexpr int B8_NT = 512, B8_TH = 8, B8_LH = B8_TH + 2, B8_NEL = B8_LH * LW, B8_NIN = (B8_NEL + B8_NT - 1) / B8_NT;
constexpr int B8_WPC = 9 * 64, B8_NWS = (2 * B8_WPC + B8_NT - 1) / B8_NT;

__global__ __launch_bounds__(B8_NT, 2) void conv3x3_bf16x8_kernel(const ConvArgs a) {
    __shared__ u32x4_t tile[2][2][B8_NEL];       // [chunk of the stage][quad pair][halo pixel]: 8 bf16 = 16 B      42.2 KB
    __shared__ bf16x8 wlds[2 * B8_WPC];          // [chunk][tap][lane]                                             18.4 KB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int tiles_x = (a.W + TW - 1) / TW;
    const int ngrp = a.ctiles;
    const int bwork = xcd_band_tile(blockIdx.x, gridDim.x);
    const int btile = bwork / ngrp;
    const int tx0 = (btile % tiles_x) * TW, ty0 = (btile / tiles_x) * B8_TH;
    const int T0 = bwork - btile * ngrp;
    const int n = blockIdx.z;
    const int ns = a.src_bgroup > 0 ? n + n / a.src_bgroup : n;   // source batch item (ConvArgs::src_bgroup)

    int cgy[B8_NIN], cgx[B8_NIN];
    bool sval[B8_NIN];
    halo_coords<B8_NT, B8_NEL, B8_NIN>(tid, ty0, tx0, a.H, a.W, cgy, cgx, sval);

    f32x16 acc[1][2];
    acc_from_bias<2>(acc[0], a.bpk, T0, h);

    const int nchunks = a.kq >> 2, nstages = (nchunks + 1) >> 1;
    const bf16x8* __restrict__ wp = reinterpret_cast<const bf16x8*>(a.wsplit16);
    cu32x2 rq[2][4][B8_NIN];   // [chunk of the stage][quad][halo slot]
    ChunkQuads cq[2];
    bf16x8 rws[B8_NWS];
    // loads of stage ST: its one or two chunks' quads, quad by quad, and weight fragments (consecutive in the packed image; the chunk index
    // is clamped: an odd chunk count repeats the last one, unused)
#define CRFP_B8_ISSUE(ST)                                                                                 \
    {                                                                                                     \
        _Pragma("unroll") for (int c2 = 0; c2 < 2; ++c2) {                                                \
            cq[c2].fetch(a, ns, min(2 * (ST) + c2, nchunks - 1));                                         \
            _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                 \
                _Pragma("unroll") for (int t = 0; t < B8_NIN; ++t)                                        \
                    rq[c2][q][t] = CRFP_LDACT(cu32x2, cq[c2].base[q] + cgy[t] * cq[c2].rs[q] + cgx[t] * cq[c2].cs[q]); \
        }                                                                                                 \
        _Pragma("unroll") for (int k = 0; k < B8_NWS; ++k) {                                              \
            const int idx = min(tid + B8_NT * k, 2 * B8_WPC - 1);                                         \
            const int ch_ = min(2 * (ST) + idx / B8_WPC, nchunks - 1);                                    \
            rws[k] = wp[((long long)T0 * nchunks + ch_) * B8_WPC + (idx % B8_WPC)];                       \
        }                                                                                                 \
    }

    CRFP_B8_ISSUE(0)
    for (int st = 0; st < nstages; ++st) {
        const bool two = 2 * st + 1 < nchunks;   // the last stage of an odd chunk count holds one chunk
        __syncthreads();
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) stage_bf16<B8_NT>(tile[c2], rq[c2], cq[c2].mask, sval, tid);
        stage_weights<B8_NT, 2 * B8_WPC>(wlds, rws, tid);
        __syncthreads();
        if (st + 1 < nstages) CRFP_B8_ISSUE(st + 1)
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) {
            if (c2 == 1 && !two) break;   // workgroup-uniform
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ky = tap / 3, kx = tap - 3 * ky;
                const bf16x8 wa = wlds[c2 * B8_WPC + tap * 64 + lane];
#pragma unroll
                for (int pt = 0; pt < 2; ++pt) {
                    const int pix = (wave + ky) * LW + pt * 32 + j + kx;
                    const bf16x8 bq = __builtin_bit_cast(bf16x8, tile[c2][h][pix]);
                    acc[0][pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa, bq, acc[0][pt], 0, 0, 0);
                }
            }
        }
    }
#undef CRFP_B8_ISSUE
    const EpiCtx ec = epi_ctx(a, n);
    conv_epilogue<1, 2, 1, 2>(ec, acc, T0, tx0, ty0, wave, j, h);
}

// ---------------------------------------------------------------- bf16 storage: TWO 3x3 convs in one launch, the tensor between them in LDS
// conv A (any sources, K in 16-channel chunks, 32 couts, bias + none / relu / lrelu) feeds conv B (32 -> 32) and has no other
// reader: dcn_block.0 -> .2 and res conv1 -> conv2(+x) of every level (model/CRFP.py:331-333, 449-481).  Run separately each
// of them is one round of 450 workgroups whose load / MFMA / store phases add up and the 14.7 MB tensor
// between them is written and read back; here conv A is evaluated on the (8 + 2) x 64 region conv B's 8 x 62 output tile needs
// (halo recompute: 20 pixel tiles of 32 per workgroup instead of 16, 3 + 2 per SIMD), rounded to bf16 exactly where the
// two-kernel path stores it, zeroed outside the image (conv B's zero padding) and kept in LDS as conv B's B-operand image.
// Same K order and per-accumulator accumulation order as conv3x3_bf16_kernel / conv3x3_bf16x8_kernel: identical values.
// LDS 76.7 KB (two workgroups per CU): input chunk tile 25.3 KB (later conv B's 18.4 KB of weights), intermediate 42.2 KB,
// conv A weight stage 9.2 KB.  45 x 11 = 495 workgroups for a 360 x 640 map = one round of the 512 slots.
// (The fp32 build's conv3x3_pair_kernel keeps only ONE 16-channel half of its two-image intermediate in LDS at a time, in the
// dead input tile: 76.5 KB as well)
constexpr int P2_NT = 512, P2_OW = 62, P2_IH = 10, P2_IW = 64, P2_LH = 12, P2_LW = 66;
constexpr int P2_NEL = P2_LH * P2_LW, P2_NIN = (P2_NEL + P2_NT - 1) / P2_NT;   // 792 input halo pixels, 2 per thread
constexpr int P2_MP = P2_IW + 2, P2_MEL = P2_IH * P2_MP;                       // intermediate rows of 64 + 2 zero columns
constexpr int P2_WPC = 9 * 64, P2_NWS = (P2_WPC + P2_NT - 1) / P2_NT, P2_NWB = (2 * P2_WPC + P2_NT - 1) / P2_NT;

struct PairB {          // what conv B adds to conv A's plan: its weights, bias, activation, destinations, residual
    const void* wsplit16;
    const float* bpk;
    const float* resid;
    long long resid_bstride;
    ConvDst dst[CRFP_MAX_DST];
    int ndst, cout, act;
    float post_scale;
};

__global__ __launch_bounds__(P2_NT, 2) void conv3x3_bf16_pair_kernel(const ConvArgs a, const PairB b) {
    __shared__ u32x4_t tileA[2][P2_NEL];         // conv A: [quad pair][input halo pixel] of the current chunk; then conv B's weights
    __shared__ u32x4_t mid[2][2][P2_MEL];        // conv A's output = conv B's input: [chunk][quad pair][pixel], 8 bf16 each
    __shared__ bf16x8 wlds[P2_WPC];              // conv A: [tap][lane] of the current chunk
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int tiles_x = (a.W + P2_OW - 1) / P2_OW;
    const int btile = xcd_band_tile(blockIdx.x, gridDim.x);
    const int tx0 = (btile % tiles_x) * P2_OW, ty0 = (btile / tiles_x) * 8;
    const int n = blockIdx.z;
    const int H = a.H, W = a.W;

    int cgy[P2_NIN], cgx[P2_NIN];
    bool sval[P2_NIN];
    static_assert(P2_LW == LW, "halo_coords walks rows of LW pixels");
    halo_coords<P2_NT, P2_NEL, P2_NIN>(tid, ty0 - 1, tx0 - 1, H, W, cgy, cgx, sval);   // conv A's input: two halo rings
    // the two zero columns behind each intermediate row (read by conv B's taps of the two discarded output columns)
    if (tid < 4 * P2_IH * 2) {
        const int pl = tid / (P2_IH * 2), rc = tid - pl * (P2_IH * 2);
        (&mid[0][0][0])[pl * P2_MEL + (rc >> 1) * P2_MP + P2_IW + (rc & 1)] = u32x4_t{0u, 0u, 0u, 0u};
    }

    // conv A: wave w owns the 32-pixel tiles w, w + 8 (and w + 16 for w < 4) of the 10 x 64 region; tile t = row t >> 1, half t & 1
    const int ntA = wave < 4 ? 3 : 2;
    f32x16 accA[3];
    acc_from_bias<3>(accA, a.bpk, 0, h);
    const int nchunks = a.kq >> 2;
    const bf16x8* __restrict__ wp = reinterpret_cast<const bf16x8*>(a.wsplit16);
    cu32x2 rq[4][P2_NIN];
    bf16x8 rws[P2_NWS];
    ChunkQuads cq;
#define CRFP_P2_ISSUE(CH)                                                                                 \
    {                                                                                                     \
        cq.fetch(a, n, CH);                                                                               \
        _Pragma("unroll") for (int t = 0; t < P2_NIN; ++t)                                                \
            _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                 \
                rq[q][t] = CRFP_LDACT(cu32x2, cq.base[q] + cgy[t] * cq.rs[q] + cgx[t] * cq.cs[q]);        \
        issue_weights<P2_NT, P2_WPC>(rws, wp + (long long)(CH) * P2_WPC, tid);                            \
    }
    CRFP_P2_ISSUE(0)
    bf16x8 rwb[P2_NWB];   // conv B's weights (both chunks), fetched under conv A's last chunk
    for (int ch = 0; ch < nchunks; ++ch) {
        __syncthreads();  // every wave finished reading the previous chunk
        // stage_bf16's two forms, written out: through the helper this kernel takes 136 instead of 134 VGPRs (profiles/r13_conv_mfma_resources.md)
        const int m0 = cq.mask[0], m1 = cq.mask[1], m2 = cq.mask[2], m3 = cq.mask[3];
        if ((m0 & m1 & m2 & m3) == 15 && !((m0 | m1 | m2 | m3) & 32)) {   // wave-uniform: 16 real bf16 channels -> plain copy
#pragma unroll
            for (int t = 0; t < P2_NIN; ++t) {
                const int idx = tid + P2_NT * t;
                if (idx < P2_NEL) {
                    const unsigned km = sval[t] ? 0xffffffffu : 0u;
                    tileA[0][idx] = u32x4_t{rq[0][t].x & km, rq[0][t].y & km, rq[1][t].x & km, rq[1][t].y & km};
                    tileA[1][idx] = u32x4_t{rq[2][t].x & km, rq[2][t].y & km, rq[3][t].x & km, rq[3][t].y & km};
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < P2_NIN; ++t) {
                const int idx = tid + P2_NT * t;
                if (idx < P2_NEL) {
                    const cu32x2 w0 = quad_words(rq[0][t], m0, sval[t]), w1 = quad_words(rq[1][t], m1, sval[t]);
                    const cu32x2 w2 = quad_words(rq[2][t], m2, sval[t]), w3 = quad_words(rq[3][t], m3, sval[t]);
                    tileA[0][idx] = u32x4_t{w0.x, w0.y, w1.x, w1.y};
                    tileA[1][idx] = u32x4_t{w2.x, w2.y, w3.x, w3.y};
                }
            }
        }
        stage_weights<P2_NT, P2_WPC>(wlds, rws, tid);
        __syncthreads();
        if (ch + 1 < nchunks) {
            CRFP_P2_ISSUE(ch + 1)
        } else {
            const bf16x8* __restrict__ wb = reinterpret_cast<const bf16x8*>(b.wsplit16);
            issue_weights<P2_NT, 2 * P2_WPC>(rwb, wb, tid);
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - 3 * ky;
            const bf16x8 wa = wlds[tap * 64 + lane];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (k == 2 && ntA == 2) break;   // wave-uniform
                const int t = wave + 8 * k;
                const int pix = ((t >> 1) + ky) * P2_LW + (t & 1) * 32 + j + kx;
                const bf16x8 bq = __builtin_bit_cast(bf16x8, tileA[h][pix]);
                accA[k] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa, bq, accA[k], 0, 0, 0);
            }
        }
    }
#undef CRFP_P2_ISSUE
    // conv A's epilogue into LDS: activation, zero outside the image, round to bf16 (what the two-kernel path stores), 8 bytes per
    // (cout quad, pixel): channel 8 g + 4 h + r is position 4 h + r of the 8-channel element (chunk g >> 1, quad pair g & 1)
    {
        const float slope = a.act == CRFP_ACT_RELU ? 0.0f : (a.act == CRFP_ACT_LRELU01 ? 0.1f : 1.0f);
        const float post = a.post_scale;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k == 2 && ntA == 2) break;
            const int t = wave + 8 * k, r = t >> 1, c = (t & 1) * 32 + j;
            const int gy = ty0 + r - 1, gx = tx0 + c - 1;
            const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float x = accA[k][4 * g + e];
                    v[e] = in ? fmaxf(x, slope * x) * post : 0.0f;
                }
                cu32x2* dst = reinterpret_cast<cu32x2*>(&mid[g >> 1][g & 1][r * P2_MP + c]) + h;
                *dst = cu32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
            }
        }
    }
    __syncthreads();   // conv A's last reads of tileA / wlds are done (and `mid` is on its way)
    bf16x8* const wb_lds = reinterpret_cast<bf16x8*>(&tileA[0][0]);
    stage_weights<P2_NT, 2 * P2_WPC>(wb_lds, rwb, tid);
    f32x16 acc[1][2];
    acc_from_bias<2>(acc[0], b.bpk, 0, h);
    __syncthreads();
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - 3 * ky;
            const bf16x8 wa = wb_lds[c2 * P2_WPC + tap * 64 + lane];
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) {
                const int pix = (wave + ky) * P2_MP + pt * 32 + j + kx;
                const bf16x8 bq = __builtin_bit_cast(bf16x8, mid[c2][h][pix]);
                acc[0][pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa, bq, acc[0][pt], 0, 0, 0);
            }
        }
    // conv B's epilogue: the shared one, on conv B's destinations / residual / activation, 62 columns per tile
    ConvArgs eb = a;
    eb.cout = b.cout; eb.act = b.act; eb.post_scale = b.post_scale; eb.store = ST_Q4; eb.ps_r = 0;
    eb.resid = b.resid; eb.resid_bstride = b.resid_bstride; eb.s3_dst = nullptr; eb.dst_f32 = 0; eb.ndst = b.ndst;
#pragma unroll
    for (int d = 0; d < CRFP_MAX_DST; ++d) eb.dst[d] = b.dst[d];
    EpiCtx ec = epi_ctx(eb, n);
    ec.xend = min(W, tx0 + P2_OW);
    conv_epilogue<1, 2, 1, 2>(ec, acc, 0, tx0, ty0, wave, j, h);
}

#endif  // CRFP_ACT_BF16

#ifdef CRFP_LAB   // main loops that lost their A/B, their knobs and their dispatch (launch_conv_lab): lab library only (make lab)
#include "conv_mfma_lab.inc"
#endif

// split weight pack: wsplit bf16 index =
//   (((((T*nchunks + ch)*9 + tap)*3 + part)*64 + lane)*8 + jj),  lane = half*32 + row,
//   K-quad = 4*ch + 2*half + (jj>>2), component = jj&3
//   np = 3: bf16 triple (bf16x6 scheme); np = 2: fp16 pair, second term scaled by 2^11 (f16x3 scheme), same index with 3 -> 2
__global__ void conv_pack_split_kernel(const ConvArgs a, const float* __restrict__ w, const float* __restrict__ w2,
                                       int cout_split, unsigned short* __restrict__ wsplit, int np) {
    const int nchunks = a.kq >> 2;
    const long long total = (long long)a.ctiles * nchunks * 9 * 64 * 8;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        long long t = idx;
        const int jj = t & 7; t >>= 3;
        const int lane = t & 63; t >>= 6;
        const int tap = t % 9; t /= 9;
        const int ch = t % nchunks;
        const int T = (int)(t / nchunks);
        const int row = lane & 31, half = lane >> 5;
        const int co = conv_row_to_cout(T * 32 + row, a.cout, a.store, a.ps_r);
        int kql = 4 * ch + 2 * half + (jj >> 2), s = 0;
        while (s < a.nsrc - 1 && kql >= a.src[s].nq) { kql -= a.src[s].nq; ++s; }
        int ci = kql < a.src[s].nq ? conv_k_to_cin(a.src[s].kind, a.src[s].nch, kql, jj & 3) : -1;
        if (ci >= 0) ci += a.src[s].cbase;
        float val = 0.0f;
        if (co >= 0 && ci >= 0 && ci < a.cin_total)
            val = co < cout_split ? w[((long long)co * a.cin_total + ci) * 9 + tap]
                                  : w2[((long long)(co - cout_split) * a.cin_total + ci) * 9 + tap];
        const long long base = (((((long long)T * nchunks + ch) * 9 + tap) * np) * 64 + lane) * 8 + jj;
        if (np == 4) {   // f16x3s: A = fp16(2^11 w), B = fp16(2^11 (w - A / 2^11)), C = fp16(w); image stride as for np == 3
            const long long b3 = (((((long long)T * nchunks + ch) * 9 + tap) * 3) * 64 + lane) * 8 + jj;
            const _Float16 pa = (_Float16)(val * 2048.0f);
            const _Float16 pb = (_Float16)((val - (float)pa * (1.0f / 2048.0f)) * 2048.0f);
            wsplit[b3] = __builtin_bit_cast(unsigned short, pa);
            wsplit[b3 + 64 * 8] = __builtin_bit_cast(unsigned short, pb);
            wsplit[b3 + 2 * 64 * 8] = __builtin_bit_cast(unsigned short, (_Float16)val);
        } else if (np == 1) {   // bf16 build: the weight IS its bf16 rounding
            wsplit[base] = __builtin_bit_cast(unsigned short, (__bf16)val);
        } else if (np == 3) {
            const __bf16 p0 = (__bf16)val;
            const float r = val - (float)p0;
            const __bf16 p1 = (__bf16)r;
            const __bf16 p2 = (__bf16)(r - (float)p1);
            wsplit[base] = __builtin_bit_cast(unsigned short, p0);
            wsplit[base + 64 * 8] = __builtin_bit_cast(unsigned short, p1);
            wsplit[base + 2 * 64 * 8] = __builtin_bit_cast(unsigned short, p2);
        } else {
            const _Float16 p0 = (_Float16)val;
            const _Float16 p1 = (_Float16)((val - (float)p0) * 2048.0f);   // F16_RES_SCALE
            wsplit[base] = __builtin_bit_cast(unsigned short, p0);
            wsplit[base + 64 * 8] = __builtin_bit_cast(unsigned short, p1);
        }
    }
}

// product build: the fp16 pair image only; lab build: bf16 triple image followed by the fp16 pair image
#ifdef CRFP_LAB
size_t conv_split_weight_bytes(const ConvArgs& a) { return (size_t)a.ctiles * (a.kq >> 2) * 9 * (3 + 2 + 3) * 64 * 16; }
size_t conv_split16_offset_bytes(const ConvArgs& a) { return (size_t)a.ctiles * (a.kq >> 2) * 9 * 3 * 64 * 16; }
#elif defined(CRFP_ACT_BF16)
size_t conv_split_weight_bytes(const ConvArgs& a) { return (size_t)a.ctiles * (a.kq >> 2) * 9 * 1 * 64 * 16; }   // one bf16 image
size_t conv_split16_offset_bytes(const ConvArgs&) { return 0; }
#else
// the fp16 pair image (4-wave kernel), then the three images of the single-accumulator scheme (8-wave kernel)
size_t conv_split_weight_bytes(const ConvArgs& a) { return (size_t)a.ctiles * (a.kq >> 2) * 9 * (2 + 3) * 64 * 16; }
size_t conv_split16_offset_bytes(const ConvArgs&) { return 0; }
#endif
#ifndef CRFP_ACT_BF16
static size_t conv_split_sa_offset_bytes(const ConvArgs& a) {
#ifdef CRFP_LAB
    return (size_t)a.ctiles * (a.kq >> 2) * 9 * 5 * 64 * 16;
#else
    return (size_t)a.ctiles * (a.kq >> 2) * 9 * 2 * 64 * 16;
#endif
}
#endif

int launch_conv_pack_split(const ConvArgs& a, const float* w, const float* w2, int cout_split, void* wsplit,
                           hipStream_t s) {
    if (a.kq & 3) { set_error("conv_pack_split: kq %d not a multiple of 4", a.kq); return CRFP_E_BADARG; }
    const long long total = (long long)a.ctiles * (a.kq >> 2) * 9 * 64 * 8;
    const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
#ifdef CRFP_LAB
    conv_pack_split_kernel<<<blocks, 256, 0, s>>>(a, w, w2, w2 ? cout_split : a.cout, (unsigned short*)wsplit, 3);
    CRFP_CHECK_LAUNCH();
#endif
    conv_pack_split_kernel<<<blocks, 256, 0, s>>>(a, w, w2, w2 ? cout_split : a.cout,
                                                  (unsigned short*)((char*)wsplit + conv_split16_offset_bytes(a)), kActBf16 ? 1 : 2);
    CRFP_CHECK_LAUNCH();
#ifndef CRFP_ACT_BF16
    conv_pack_split_kernel<<<blocks, 256, 0, s>>>(a, w, w2, w2 ? cout_split : a.cout,
                                                  (unsigned short*)((char*)wsplit + conv_split_sa_offset_bytes(a)), 4);
    CRFP_CHECK_LAUNCH();
#endif
    return 0;
}

// ---------------------------------------------------------------- weight packing (device side)
// wpk float index = ((((T*npairs + pair)*9 + tap)*2 + half)*32 + row)*4 + comp
// Rows whose reference channel is >= cout_split come from a second weight tensor (w2/bias2): used to
// run dcn_offset and dcn_mask (same input, model/CRFP.py:337,339) as ONE convolution.
__global__ void conv_pack_kernel(const ConvArgs a, const float* __restrict__ w, const float* __restrict__ bias,
                                 const float* __restrict__ w2, const float* __restrict__ bias2, int cout_split,
                                 float* __restrict__ wpk, float* __restrict__ bpk) {
    const int npairs = a.kq >> 1;
    const long long total = (long long)a.ctiles * npairs * 9 * 64 * 4;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        long long t = idx;
        const int comp = t & 3; t >>= 2;
        const int row = t & 31; t >>= 5;
        const int half = t & 1; t >>= 1;
        const int tap = t % 9; t /= 9;
        const int pair = t % npairs;
        const int T = (int)(t / npairs);
        const int co = conv_row_to_cout(T * 32 + row, a.cout, a.store, a.ps_r);
        int kql = 2 * pair + half, s = 0;
        while (s < a.nsrc - 1 && kql >= a.src[s].nq) { kql -= a.src[s].nq; ++s; }
        int ci = kql < a.src[s].nq ? conv_k_to_cin(a.src[s].kind, a.src[s].nch, kql, comp) : -1;
        if (ci >= 0) ci += a.src[s].cbase;
        float val = 0.0f;
        if (co >= 0 && ci >= 0 && ci < a.cin_total)
            val = co < cout_split ? w[((long long)co * a.cin_total + ci) * 9 + tap]
                                  : w2[((long long)(co - cout_split) * a.cin_total + ci) * 9 + tap];
        if (kActBf16) val = (float)(__bf16)val;   // bf16 build: every conv weight of the engine is a bf16 value
        wpk[idx] = val;
    }
    const int nb = a.ctiles * 32;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < nb; r += gridDim.x * blockDim.x) {
        const int co = conv_row_to_cout(r, a.cout, a.store, a.ps_r);
        bpk[r] = co < 0 ? 0.0f : (co < cout_split ? (bias ? bias[co] : 0.0f) : bias2[co - cout_split]);
    }
}

size_t conv_packed_weight_floats(const ConvArgs& a) { return (size_t)a.ctiles * (a.kq >> 1) * 9 * 64 * 4; }

int launch_conv_pack(const ConvArgs& a, const float* w, const float* bias, const float* w2, const float* bias2,
                     int cout_split, float* wpk, float* bpk, hipStream_t s) {
    const long long total = (long long)conv_packed_weight_floats(a);
    const int blocks = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
    conv_pack_kernel<<<blocks, 256, 0, s>>>(a, w, bias, w2, bias2, w2 ? cout_split : a.cout, wpk, bpk);
    CRFP_CHECK_LAUNCH();
    return 0;
}

// Precision of the engine's wide convolutions and of dcn_g8's GEMM.  Default: the split-fp16 scheme (fp32-grade, needs
// |operand| < 65504, guarded by the overflow word, see ConvArgs::ovf).  Strict: plain fp32 MFMA everywhere -- selected per
// call through ConvArgs::strict (CRFP_DSV_STRICT_F32 of the C-ABI) or for the whole process with CRFP_PRECISION=f32
// (read once; the per-family knobs of round 1, CRFP_CONV_MODE=f32 / CRFP_DCN_MODE=f32, are read by the lab library only).
#ifndef CRFP_ACT_BF16

}  // namespace CRFP_NS
namespace crfp {
bool precision_env_strict(int family) {
    const char* p = getenv("CRFP_PRECISION");
    if (p && !strcmp(p, "f32")) return true;
    // the round-1 per-family knobs live on in the lab library only
    const char* l = family == 0 ? CRFP_LAB_ENV("CRFP_CONV_MODE") : CRFP_LAB_ENV("CRFP_DCN_MODE");
    return l && !strcmp(l, "f32");
}
}  // namespace crfp
namespace CRFP_NS {
#endif

// SRC_S3 sources / s3_dst are understood by conv3x3_split_kernel<1,1,2> (the default) only
bool conv_s3_supported() {
    static const bool ok = [] {
        if (kActBf16 || precision_env_strict(0)) return false;
#ifdef CRFP_LAB
        if (!lab_conv_s3_supported()) return false;
#endif
        return true;
    }();
    return ok;
}

// per-quad load descriptors (wave-uniform in the kernels: one s_load per quad); filled into the caller's private plan copy
static int build_quad_descs(ConvArgs& am, const char* name) {
    const ConvArgs& a = am;
    {
        int q = 0;
        for (int i = 0; i < a.nsrc; ++i)
            for (int k = 0; k < a.src[i].nq; ++k, ++q) {
                const ConvSrc& sr = a.src[i];
                QuadDesc& d = am.qd[q];
                d.bstride = sr.bstride; d.rsv = 0;
                // strides and offsets are in FLOATS (4 bytes) for both builds: an activation quad spans kQuadBytes / 4 of them
                constexpr int QF = kQuadBytes / 4;
                if (sr.kind == SRC_Q4) {
                    d.bstride = sr.bstride * (long long)sizeof(act_t) / 4;
                    d.rs = (a.W + sr.pad) * QF; d.cs = QF; d.mask = 15;
                    d.base = sr.p + (long long)k * (a.H + sr.pad) * d.rs;
                } else if (sr.kind == SRC_UNSHUF4) {
                    const int W4 = 4 * a.W + sr.pad, ij = k & 15;
                    d.bstride = sr.bstride * (long long)sizeof(act_t) / 4;
                    d.rs = 4 * W4 * QF; d.cs = 4 * QF; d.mask = 15;
                    d.base = sr.p + ((long long)(k >> 4) * (4 * a.H + sr.pad) * W4 + (ij >> 2) * W4 + (ij & 3)) * QF;
                } else if (sr.kind == SRC_FLOW2) {
                    d.rs = 2 * a.W; d.cs = 2; d.mask = kActBf16 ? (32 | 3) : 3; d.base = sr.p;   // bit 5: fp32 (dx, dy) pair
                } else if (sr.kind == SRC_S3) {
                    // chunk-local quad qi -> 16-byte plane: qi 0/1 = x0 image, channels 0..7 / 8..15 of the chunk; qi 2/3 = x1s image
                    if ((q & 3) != (k & 3) || (sr.nq & 3) || sr.pad) {
                        set_error("conv_mfma %s: an SRC_S3 source must start on a 16-channel chunk, hold whole chunks and be unpadded", name);
                        return CRFP_E_BADARG;
                    }
                    const int qi = k & 3, plane = (qi >> 1) * (sr.nq >> 1) + 2 * (k >> 2) + (qi & 1);
                    d.rs = a.W * 4; d.cs = 4; d.mask = 16 | 15;
                    d.base = sr.p + (long long)plane * a.H * d.rs;
                } else {
                    d.rs = 0; d.cs = 0; d.mask = 0; d.base = a.wpk; d.bstride = 0;
                }
            }
    }
    return 0;
}

// algorithmic work of one conv for ProfScope: activations in and out in the storage type plus the fp32 weights; 2 flops per multiply-add
struct ConvWork { double px, in_ch, bytes, flops; };
static ConvWork conv_work(const ConvArgs& a) {
    ConvWork w;
    w.px = (double)a.N * a.H * a.W;
    w.in_ch = 0;
    for (int i = 0; i < a.nsrc; ++i) w.in_ch += a.src[i].kind == SRC_ZERO ? 0 : a.src[i].nch;
    w.bytes = w.px * (w.in_ch + a.cout) * (double)sizeof(act_t) + (double)a.cout * w.in_ch * 9 * 4.0;
    w.flops = 2.0 * w.px * a.cout * w.in_ch * 9.0;
    return w;
}

// what a launcher derives in its private, mutable plan copy before the kernel reads it: no stamps, the weight images behind a.wsplit, the
// per-quad load descriptors
static int prepare_plan(ConvArgs& am, const char* name) {
    am.stamps = nullptr;
    am.wsplit16 = am.wsplit ? (const char*)am.wsplit + conv_split16_offset_bytes(am) : nullptr;
#ifndef CRFP_ACT_BF16
    am.wsplit_sa = am.wsplit ? (const char*)am.wsplit + conv_split_sa_offset_bytes(am) : nullptr;
#endif
    return am.kq <= CRFP_MAX_KQ ? build_quad_descs(am, name) : 0;
}

// whether launch_conv_mfma runs plan a on a split-operand kernel (fp32 build: f16x3, bf16 build: bf16 operands) instead of the fp32 MFMA
static bool conv_plan_splits(const ConvArgs& a) {
    static const bool env_strict = precision_env_strict(0);
    bool nchw_src = false;
    for (int i = 0; i < a.nsrc; ++i) nchw_src |= a.src[i].kind == SRC_NCHW || a.src[i].kind == SRC_NCHW_SHIFT;
    return a.wsplit && !(env_strict || a.strict) && (a.kq & 3) == 0 && !nchw_src && a.kq <= CRFP_MAX_KQ;
}

// The kernel launch_conv_mfma runs for a plan that passed its checks (the lab library's experiments branch off before this is asked)
ConvKernel conv_select_kernel(const ConvArgs& a) {
    const bool split = conv_plan_splits(a);
    const bool ct2 = !split && a.ctiles % 2 == 0;  // split: <2,1> needs 93 KB of LDS (1 workgroup per CU): slower than 2 x <1,1>
    if (split) {
#ifdef CRFP_ACT_BF16
        // (8-row tiles, conv3x3_bf16_kernel<2>: 1.25 instead of 1.5 ds_read_b128 per MFMA and half the weight staging, but 450
        // workgroups on 256 CUs -- measured neutral to -8 % per conv, so 4-row tiles stay.  A register prefetch two chunks deep
        // (126 VGPRs, still 4 workgroups per CU) was also slower: 32->32 conv 15.2 -> 16.3 us, offset / mask head 70.8 -> 74.0.)
        // 8-wave kernel, two chunks per staging phase, for the 32-cout layers with an even chunk count: same-box 32 -> 32 convs 16.0 ->
        // 15.1 us, conv2(+x) 17.7 -> 17.0, conv_fuse 22.2 -> 21.6, identical values; block0 (5 chunks: a half-empty last stage) 25.4 -> 26.0,
        // so odd chunk counts keep the 4-wave kernel
        // (for layers with several cout tiles it loses: FNet dec2a 36 -> 43 us, enc3b 22 -> 26, the pixel-shuffle heads +0..1 us)
        // ... and only while its 8-row tiles fill no more than one round of the chip's 512 slots (two 60 KB workgroups per CU): a lock-step
        // batch of clips is several rounds, where tile granularity no longer matters and the 4-wave kernel's four workgroups per CU overlap
        // more of each other's load / MFMA / store phases (round 4, same box, 4 clips: res.main0 15.1 -> 14.1 us per clip, conv_fuse 14.7 -> 14.0,
        // conv1 9.9 -> 9.2)
        constexpr int x8_max_wgs = 512;   // fixed in the product: the x8 / 4-wave choice is part of the per-clip bit-identity contract
        if (a.ctiles == 1 && ((a.kq >> 2) & 1) == 0 && (long long)a.N * ((a.W + TW - 1) / TW) * ((a.H + B8_TH - 1) / B8_TH) <= x8_max_wgs)
            return CK_BF16_X8;
        return CK_BF16_4W;
#else
        // 8-wave single-accumulator kernel for the convs with one cout tile (the 32-cout layers: one round of 450 workgroups
        // instead of 1.17 rounds of 900; same-box: conv1 26.4 -> 24.6 us, conv2 28.7 -> 26.1, block0 46.0 -> 43.2, main0 40.0 ->
        // 38.0, clip -1.5 %); with several cout tiles the 4-wave kernel stays (offset/mask head 114.0 vs 117.7 us)
        return a.ctiles == 1 ? CK_SPLIT8 : CK_SPLIT4;
#endif
    }
    if (a.src[0].kind == SRC_NCHW_SHIFT) return ct2 ? CK_MFMA_SHIFT_CT2 : CK_MFMA_SHIFT;   // SPyNet's 7x7-as-3x3 convolutions: 18 ... 144 K-quads, two chunks per staging phase
    if (ct2) return CK_MFMA_CT2;
    // few 8-row tiles (the LR-resolution convs of a single streamed frame: 115 workgroups for 180 x 320): 4-row tiles spread the
    // same latency-bound work over twice as many CUs
    const int tiles = ((a.W + TW - 1) / TW) * ((a.H + 7) / 8);
    return (long long)tiles * a.ctiles * a.N < 512 ? CK_MFMA_ROWS4 : CK_MFMA_ROWS8;
}

int launch_conv_mfma(const ConvArgs& a, const char* name, hipStream_t s) {
    if (a.kq & 1 || a.kq < 2 || a.ctiles < 1 || a.nsrc < 1 || a.nsrc > CRFP_MAX_SRC) {
        set_error("conv_mfma %s: bad plan (kq=%d ctiles=%d nsrc=%d)", name, a.kq, a.ctiles, a.nsrc);
        return CRFP_E_BADARG;
    }
    if (a.store == ST_PS && ((a.ps_r != 2 && a.ps_r != 4) || a.act == CRFP_ACT_TANH || a.act == CRFP_ACT_SIGMOID)) {
        set_error("conv_mfma %s: pixel-shuffle store supports r in {2, 4} with none/relu/lrelu (r=%d act=%d)", name, a.ps_r, a.act);
        return CRFP_E_UNSUPPORTED;
    }
    if (a.ksplit > 0) {
        // K split over blockIdx.z exists in ONE launch branch (the fp32-MFMA kernel over SRC_NCHW_SHIFT views, two K-quads per step) and
        // writes raw partial sums: anything else would drop trailing chunks, apply bias / activation once per slice, or keep grid.z = N
        bool shift_only = true;
        for (int i = 0; i < a.nsrc; ++i) shift_only = shift_only && a.src[i].kind == SRC_NCHW_SHIFT;
        if (!shift_only || ((a.kq >> 1) % a.ksplit) != 0 || a.act != CRFP_ACT_NONE || a.post_scale != 1.0f || a.resid || a.store != ST_NCHW) {
            set_error("conv_mfma %s: ksplit = %d needs SRC_NCHW_SHIFT sources only, (kq / 2) %% ksplit == 0 (kq = %d), no activation / scale / residual "
                      "and an NCHW store of the partial sums", name, a.ksplit, a.kq);
            return CRFP_E_UNSUPPORTED;
        }
    }
    static const bool env_strict = precision_env_strict(0);
    bool s3_src = false;
    for (int i = 0; i < a.nsrc; ++i) s3_src |= a.src[i].kind == SRC_S3;
    const bool split = conv_plan_splits(a);
    const bool uses_s3 = a.s3_dst != nullptr || s3_src;
    if (uses_s3 && (!split || !conv_s3_supported() || (a.s3_dst && (a.store != ST_Q4 || (a.cout & 7))))) {
        set_error("conv_mfma %s: SRC_S3 / s3_dst need the default f16x3 kernel, ST_Q4 and cout %% 8 == 0", name);
        return CRFP_E_UNSUPPORTED;
    }
    const ConvWork work = conv_work(a);
    ProfScope prof(name, s, work.bytes, work.flops);
    ConvArgs& am = const_cast<ConvArgs&>(a);  // callers pass a private, mutable plan copy
    if (env_strict || a.strict) am.ovf = nullptr;   // nothing downstream turns this output into an fp16 operand
    {
        const int rc = prepare_plan(am, name);
        if (rc) return rc;
    }
#ifdef CRFP_LAB
    {
        bool done = false;
        const int rc = launch_conv_lab(am, name, split, s, &done);
        if (rc || done) return rc;
    }
#endif
    const int tw = (a.W + TW - 1) / TW;
    const int tiles4 = tw * ((a.H + 3) / 4), tiles8 = tw * ((a.H + 7) / 8);   // 4-row / 8-row tiles of 64 columns
    const int nz = a.N * (a.ksplit > 0 ? a.ksplit : 1);
    switch (conv_select_kernel(a)) {
#ifdef CRFP_ACT_BF16
        case CK_BF16_X8: {
            static_assert(B8_TH == 8, "conv3x3_bf16x8_kernel walks 8-row tiles");
            conv3x3_bf16x8_kernel<<<dim3(tiles8 * a.ctiles, 1, a.N), B8_NT, 0, s>>>(am);
            break;
        }
        case CK_BF16_4W: conv3x3_bf16_kernel<1><<<dim3(tiles4 * a.ctiles, 1, a.N), 256, 0, s>>>(am); break;
#else
        case CK_SPLIT8: {
            static_assert(S8_TH == 8, "conv3x3_split8_kernel<8> walks 8-row tiles");
            conv3x3_split8_kernel<S8_TH><<<dim3(tiles8 * a.ctiles, 1, a.N), 64 * S8_TH, 0, s>>>(am);
            break;
        }
        case CK_SPLIT4: conv3x3_split_kernel<1, 1, 2><<<dim3(tiles4 * a.ctiles, 1, a.N), 256, 0, s>>>(am); break;
#endif
        case CK_MFMA_SHIFT_CT2: conv3x3_mfma_kernel<2, 1, 2><<<dim3(tiles4 * (a.ctiles / 2), 1, nz), 256, 0, s>>>(a); break;
        case CK_MFMA_SHIFT: conv3x3_mfma_kernel<1, 1, 2><<<dim3(tiles4 * a.ctiles, 1, nz), 256, 0, s>>>(a); break;
        case CK_MFMA_CT2: conv3x3_mfma_kernel<2, 1><<<dim3(tiles4 * (a.ctiles / 2), 1, a.N), 256, 0, s>>>(a); break;
        case CK_MFMA_ROWS4: conv3x3_mfma_kernel<1, 1><<<dim3(tiles4 * a.ctiles, 1, a.N), 256, 0, s>>>(a); break;
        case CK_MFMA_ROWS8: conv3x3_mfma_kernel<1, 2><<<dim3(tiles8 * a.ctiles, 1, a.N), 256, 0, s>>>(a); break;
        default: set_error("conv_mfma %s: no kernel for this plan in this build", name); return CRFP_E_UNSUPPORTED;
    }
    CRFP_CHECK_LAUNCH();
    return 0;
}


// Two convs of the same shape in one launch (fp32 build: conv3x3_split_dual_kernel); anything it does not cover runs as two launches.
// The decision: CK_SPLIT_DUAL, or CK_NONE for two launches.
ConvKernel conv_select_dual(const ConvArgs& a0, const ConvArgs& a1) {
#ifndef CRFP_ACT_BF16
    auto plain_split = [](const ConvArgs& a) {
        bool q4 = true;
        for (int i = 0; i < a.nsrc; ++i) q4 = q4 && (a.src[i].kind == SRC_Q4 || a.src[i].kind == SRC_S3 || a.src[i].kind == SRC_ZERO);
        return a.wsplit && !a.strict && !precision_env_strict(0) && (a.kq & 3) == 0 && a.kq <= CRFP_MAX_KQ && a.ctiles > 1 && q4 && !a.s3_dst &&
               (a.store != ST_PS || ((a.ps_r == 2 || a.ps_r == 4) && a.act != CRFP_ACT_TANH && a.act != CRFP_ACT_SIGMOID));
    };
    bool lab = false;
#ifdef CRFP_LAB
    lab = true;   // the lab library keeps its kernel-selection knobs: two launches
#endif
    if (!lab && plain_split(a0) && plain_split(a1) && a0.N == a1.N && a0.H == a1.H && a0.W == a1.W && a0.ctiles == a1.ctiles &&
        conv_s3_supported()) {
        const int tiles = ((a0.W + TW - 1) / TW) * ((a0.H + 3) / 4), w0 = tiles * a0.ctiles;
        if ((w0 & 7) == 0) return CK_SPLIT_DUAL;
    }
#else
    (void)a0; (void)a1;
#endif
    return CK_NONE;
}

int launch_conv_mfma_dual(const ConvArgs& a0, const char* name0, const ConvArgs& a1, const char* name1, const char* name_both, hipStream_t s) {
    switch (conv_select_dual(a0, a1)) {
#ifndef CRFP_ACT_BF16
        case CK_SPLIT_DUAL: {
            const int tiles = ((a0.W + TW - 1) / TW) * ((a0.H + 3) / 4), w0 = tiles * a0.ctiles;
            const ConvWork w0k = conv_work(a0), w1k = conv_work(a1);
            ProfScope prof(name_both, s, w0k.bytes + w1k.bytes, w0k.flops + w1k.flops);
            ConvArgs* am[2] = {&const_cast<ConvArgs&>(a0), &const_cast<ConvArgs&>(a1)};   // callers pass private, mutable plan copies
            const char* nm[2] = {name0, name1};
            for (int k = 0; k < 2; ++k) {
                const int rc = prepare_plan(*am[k], nm[k]);
                if (rc) return rc;
            }
            conv3x3_split_dual_kernel<1, 1, 2><<<dim3(2 * w0, 1, a0.N), 256, 0, s>>>(*am[0], *am[1], w0);
            CRFP_CHECK_LAUNCH();
            return 0;
        }
#endif
        default: {
            const int rc = launch_conv_mfma(a0, name0, s);
            return rc ? rc : launch_conv_mfma(a1, name1, s);
        }
    }
}

#ifdef CRFP_ACT_BF16
// conv A -> conv B in one launch (conv3x3_bf16_pair_kernel); both plans as launch_conv_mfma takes them.  Conv A's output tensor is
// never written: it must have no other reader.
int launch_conv_pair(const ConvArgs& a, const ConvArgs& b, const char* name, hipStream_t s) {
    if ((a.kq & 3) || a.kq > CRFP_MAX_KQ || a.ctiles != 1 || a.cout != 32 || a.store != ST_Q4 || !a.wsplit || a.act == CRFP_ACT_TANH ||
        a.act == CRFP_ACT_SIGMOID || b.nsrc != 1 || b.src[0].kind != SRC_Q4 || b.kq != 8 || b.ctiles != 1 || b.cout != 32 || b.store != ST_Q4 ||
        !b.wsplit || b.act == CRFP_ACT_TANH || b.act == CRFP_ACT_SIGMOID || b.s3_dst || b.dst_f32 || a.N != b.N || a.H != b.H || a.W != b.W) {
        set_error("conv_pair %s: unsupported pair (A: kq=%d cout=%d store=%d; B: nsrc=%d kq=%d cout=%d store=%d)", name, a.kq, a.cout, a.store,
                  b.nsrc, b.kq, b.cout, b.store);
        return CRFP_E_UNSUPPORTED;
    }
    for (int i = 0; i < a.nsrc; ++i)
        if (a.src[i].kind == SRC_NCHW || a.src[i].kind == SRC_S3) { set_error("conv_pair %s: NCHW / S3 sources are not supported", name); return CRFP_E_UNSUPPORTED; }
    const ConvWork w = conv_work(a);
    // algorithmic work of the PAIR: A's inputs + B's outputs (+ residual) cross HBM, the 32-channel tensor between them does not
    ProfScope prof(name, s, w.px * (w.in_ch + 32 + (b.resid ? 32 : 0)) * (double)sizeof(act_t) + (32.0 * w.in_ch + 32.0 * 32.0) * 9 * 4.0,
                   2.0 * w.px * 32 * (w.in_ch + 32) * 9.0);
    ConvArgs am = a;
    const int rc = prepare_plan(am, name);
    if (rc) return rc;
    PairB pb;
    memset(&pb, 0, sizeof(pb));
    pb.wsplit16 = (const char*)b.wsplit + conv_split16_offset_bytes(b);
    pb.bpk = b.bpk; pb.resid = b.resid; pb.resid_bstride = b.resid_bstride;
    for (int d = 0; d < CRFP_MAX_DST; ++d) pb.dst[d] = b.dst[d];
    pb.ndst = b.ndst; pb.cout = b.cout; pb.act = b.act; pb.post_scale = b.post_scale;
    am.ovf = b.ovf; am.ovf_div = b.ovf_div; am.ovf_add = b.ovf_add;
    const int tiles = ((a.W + P2_OW - 1) / P2_OW) * ((a.H + 7) / 8);
    conv3x3_bf16_pair_kernel<<<dim3(tiles, 1, a.N), P2_NT, 0, s>>>(am, pb);
    CRFP_CHECK_LAUNCH();
    return 0;
}
#else
// conv A -> conv B in one launch (conv3x3_pair_kernel), default split-fp16 mode only; both plans as launch_conv_mfma takes them.  Conv A's
// output tensor is never written: it must have no other reader.  Conv B may also (or only) write its SRC_S3 image.
int launch_conv_pair(const ConvArgs& a, const ConvArgs& b, const char* name, hipStream_t s) {
    if ((a.kq & 3) || a.kq > CRFP_MAX_KQ || a.ctiles != 1 || a.cout != 32 || a.store != ST_Q4 || !a.wsplit || a.act == CRFP_ACT_TANH ||
        a.act == CRFP_ACT_SIGMOID || a.resid || a.s3_dst || b.nsrc != 1 || b.src[0].kind != SRC_Q4 || b.kq != 8 || b.ctiles != 1 || b.cout != 32 ||
        b.store != ST_Q4 || !b.wsplit || b.act == CRFP_ACT_TANH || b.act == CRFP_ACT_SIGMOID || b.dst_f32 || a.N != b.N || a.H != b.H || a.W != b.W) {
        set_error("conv_pair %s: unsupported pair (A: kq=%d cout=%d store=%d; B: nsrc=%d kq=%d cout=%d store=%d)", name, a.kq, a.cout, a.store,
                  b.nsrc, b.kq, b.cout, b.store);
        return CRFP_E_UNSUPPORTED;
    }
    if (a.strict || b.strict || precision_env_strict(0)) { set_error("conv_pair %s: the pair kernel exists in the split-fp16 mode only", name); return CRFP_E_UNSUPPORTED; }
    if (b.s3_dst && !conv_s3_supported()) { set_error("conv_pair %s: s3_dst needs the default f16x3 kernels", name); return CRFP_E_UNSUPPORTED; }
    for (int i = 0; i < a.nsrc; ++i)
        if (a.src[i].kind == SRC_NCHW || a.src[i].kind == SRC_NCHW_SHIFT) { set_error("conv_pair %s: NCHW sources are not supported", name); return CRFP_E_UNSUPPORTED; }
    const ConvWork w = conv_work(a);
    // algorithmic work of the PAIR: A's inputs + B's outputs (+ residual) cross HBM, the 32-channel tensor between them does not
    ProfScope prof(name, s, w.px * (w.in_ch + 32 + (b.resid ? 32 : 0)) * (double)sizeof(act_t) + (32.0 * w.in_ch + 32.0 * 32.0) * 9 * 4.0,
                   2.0 * w.px * 32 * (w.in_ch + 32) * 9.0);
    ConvArgs am = a;
    const int rc = prepare_plan(am, name);
    if (rc) return rc;
    PairB pb;
    memset(&pb, 0, sizeof(pb));
    pb.wsplit_sa = (const char*)b.wsplit + conv_split_sa_offset_bytes(b);
    pb.bpk = b.bpk; pb.resid = b.resid; pb.resid_bstride = b.resid_bstride;
    for (int d = 0; d < CRFP_MAX_DST; ++d) pb.dst[d] = b.dst[d];
    pb.ndst = b.ndst; pb.cout = b.cout; pb.act = b.act; pb.post_scale = b.post_scale;
    pb.s3_dst = b.s3_dst; pb.s3_bstride = b.s3_bstride;
    pb.ovf = b.ovf; pb.ovf_div = b.ovf_div; pb.ovf_add = b.ovf_add; pb.ovf_skip0 = b.ovf_skip0;
    const int tiles = ((a.W + PF_OW - 1) / PF_OW) * ((a.H + 7) / 8);
    conv3x3_pair_kernel<<<dim3(tiles, 1, a.N), PF_NT, 0, s>>>(am, pb);
    CRFP_CHECK_LAUNCH();
    return 0;
}
#endif

}  // namespace CRFP_NS
