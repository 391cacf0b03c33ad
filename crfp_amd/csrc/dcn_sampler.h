// The per-lane bilinear gather of padded (P4) planes and the pairwise dcn_g8 sampler built on it: shared by gather.hip (warps,
// dcn_g8_pipe_kernel, dcn_3) and dcn_fused.hip (the offset head + dcn_g8 in one launch).
#pragma once
#include "crfp_common.h"

namespace CRFP_NS {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ---- P4 sources ("padded Q4"): planes are (H+1) x (W+1) with a zero pad row (y == H) and a zero pad
// column (x == W).  With the sample position clamped to [-1, size] every one of the 4 bilinear
// corners either hits real data, a zero pad element (x == -1 is the pad column of the previous row,
// y == -1 the pad row of the previous plane) or falls outside the buffer, where the hardware range
// check of a raw buffer load returns 0.  No per-corner validity logic and no 64-bit address math is
// left on the VALU: one 32-bit byte offset per sample, the other three corners ride on the scalar
// offset operand (+16, +pitch, +pitch+16).
constexpr int kGatherAux = 0;   // cache-policy bits of the gather loads (gfx942+: 1 = sc0, 2 = nt, 16 = sc1)
// one pixel quad (16 bytes of fp32 / 8 bytes of bf16) at byte offset voff + soff; out-of-range reads return 0
__device__ __forceinline__ f32x4 bload(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
#ifdef CRFP_ACT_BF16
    return quad_from_bits(__builtin_bit_cast(cu32x2, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, kGatherAux)));
#else
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, kGatherAux));
#endif
}
constexpr int QB = kQuadBytes;   // bytes per pixel quad of a gathered plane

// The two horizontally adjacent corners (x0, x0 + 1) of a bilinear sample are adjacent in memory -- also across the row end,
// where x0 + 1 is the zero pad column, and at x0 = -1, which is the pad column of the previous row.  In the bf16 build the
// pair is 16 bytes = ONE buffer_load_dwordx4 (dword alignment is all a buffer load needs): half the gather instructions of
// the fp32 build, which matters because these kernels are bound by the texture-address / L1 rate of their per-lane gathers,
// not by bytes (dcn_g8: 66 M lane-loads per launch @A).
#ifdef CRFP_ACT_BF16
typedef u32x4 pairraw_t;
__device__ __forceinline__ pairraw_t bload_pair(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, kGatherAux);
}
__device__ __forceinline__ f32x4 pair_lo(const pairraw_t& p) { return quad_from_bits(cu32x2{p.x, p.y}); }
__device__ __forceinline__ f32x4 pair_hi(const pairraw_t& p) { return quad_from_bits(cu32x2{p.z, p.w}); }
#else
struct pairraw_t { f32x4 lo, hi; };
__device__ __forceinline__ pairraw_t bload_pair(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    pairraw_t p;
    p.lo = bload(r, voff, soff);
    p.hi = bload(r, voff, soff + 16);
    return p;
}
__device__ __forceinline__ f32x4 pair_lo(const pairraw_t& p) { return p.lo; }
__device__ __forceinline__ f32x4 pair_hi(const pairraw_t& p) { return p.hi; }
#endif

// ---------------------------------------------------------------- the dcn_g8 sampler, one pair of sampling positions at a time
// (dcn_g8_pipe_kernel in gather.hip describes the mapping: wave = 32 pixels of a row, lane half = 4 deformable groups, 36 sampling
// positions per lane, consumed in 18 pairs)
typedef _Float16 dcn_f16x8 __attribute__((ext_vector_type(8)));

struct DcnPair {
    pairraw_t tp[2], bt[2];   // [position]: top / bottom corner pairs as loaded
    float w[2][4];            // modulated bilinear weights
};

struct DcnOff { f32x4 m4, oa, ob; };   // masks of 4 positions, (dy,dx) of positions (0,1) and (2,3)

// one sampling position (p36 = 9 * group-in-half + tap, compile-time) into slot pi of P: coordinates, modulated bilinear weights,
// the two 2-corner gathers
__device__ __forceinline__ void dcn_issue_one(DcnPair& P, int pi, __amdgpu_buffer_rsrc_t rx, float dy, float dx, float mm, int p36,
                                              float fy0, float fx0, float fH, float fW, int PW, int pitch, int plane_b, int hbase) {
    const int gi = p36 / 9, tap = p36 - 9 * gi, ky = tap / 3, kx = tap - 3 * ky;
    // (float)(cy-1) + (float)ky is exact, so this equals the reference's (float)(y - pad + ky) + dy
    float sy = (fy0 + (float)ky) + dy;
    float sx = (fx0 + (float)kx) + dx;
    sy = __builtin_amdgcn_fmed3f(sy, -1.0f, fH);   // = min(max(sy, -1), H) in one instruction (the offsets are finite)
    sx = __builtin_amdgcn_fmed3f(sx, -1.0f, fW);
    const float fy = floorf(sy), fx = floorf(sx);
    const float ly = sy - fy, lx = sx - fx;
    const float a = (1.0f - ly) * mm, b = ly * mm, hx = 1.0f - lx;
    P.w[pi][0] = a * hx; P.w[pi][1] = a * lx; P.w[pi][2] = b * hx; P.w[pi][3] = b * lx;
    // element index fy * PW + fx in float (exact below 2^24: a 2x-resolution plane has < 2^22 elements), one conversion
    const int vo = (int)__builtin_fmaf(fy, (float)PW, fx) * QB + hbase + gi * plane_b;
    P.tp[pi] = bload_pair(rx, vo, 0);
    P.bt[pi] = bload_pair(rx, vo, pitch);
}

__device__ __forceinline__ void dcn_issue_pair(DcnPair& P, __amdgpu_buffer_rsrc_t rx, const DcnOff& O, int hb, int v, float fy0,
                                               float fx0, float fH, float fW, int PW, int pitch, int plane_b, int hbase) {
    const float dyv[4] = {O.oa.x, O.oa.z, O.ob.x, O.ob.z};
    const float dxv[4] = {O.oa.y, O.oa.w, O.ob.y, O.ob.w};
    const float mmv[4] = {O.m4.x, O.m4.y, O.m4.z, O.m4.w};
#pragma unroll
    for (int pi = 0; pi < 2; ++pi)
        dcn_issue_one(P, pi, rx, dyv[hb + pi], dxv[hb + pi], mmv[hb + pi], 4 * v + hb + pi, fy0, fx0, fH, fW, PW, pitch, plane_b, hbase);
}

// bilinear blend of position pi of a pair into xs[4 pi .. 4 pi + 3] (one multiply + three FMAs per channel)
__device__ __forceinline__ void dcn_lerp_one(const DcnPair& P, int pi, float (&xs)[8]) {
    f32x4 val = pair_lo(P.tp[pi]) * P.w[pi][0];
    val = __builtin_elementwise_fma(pair_hi(P.tp[pi]), f32x4{P.w[pi][1], P.w[pi][1], P.w[pi][1], P.w[pi][1]}, val);
    val = __builtin_elementwise_fma(pair_lo(P.bt[pi]), f32x4{P.w[pi][2], P.w[pi][2], P.w[pi][2], P.w[pi][2]}, val);
    val = __builtin_elementwise_fma(pair_hi(P.bt[pi]), f32x4{P.w[pi][3], P.w[pi][3], P.w[pi][3], P.w[pi][3]}, val);
    xs[4 * pi + 0] = val.x; xs[4 * pi + 1] = val.y; xs[4 * pi + 2] = val.z; xs[4 * pi + 3] = val.w;
}

// the sampled pair (8 values = one K = 16 step of the lane) split exactly into two fp16 terms and multiplied into the DCN sums
__device__ __forceinline__ void dcn_split_mfma(const float (&xs)[8], f32x16& acc, f32x16& acl, const f32x4* wl, int u, int lane) {
    // the exact two-term split in its 3-op-per-value form (conv_mfma.hip split_f16x8_fast): one v_cvt_pk_f16_f32 per pair of
    // values, x - x0 as one v_fma_mix_f32, the scaled residuals through a second pack -- the same values as the scalar form
    typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
    typedef float f2_t __attribute__((ext_vector_type(2)));
    typedef unsigned u4_t __attribute__((ext_vector_type(4)));
    u4_t hi4, lo4;
    float negone = -1.0f;
    asm("" : "+v"(negone));   // opaque: keeps fma(x0, -1, x) one v_fma_mix_f32
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const h2_t h2 = __builtin_convertvector(f2_t{xs[2 * i], xs[2 * i + 1]}, h2_t);
        const float r0 = __builtin_fmaf((float)h2[0], negone, xs[2 * i]);
        const float r1 = __builtin_fmaf((float)h2[1], negone, xs[2 * i + 1]);
        const h2_t l2 = __builtin_convertvector(f2_t{r0 * 2048.0f, r1 * 2048.0f}, h2_t);
        hi4[i] = __builtin_bit_cast(unsigned, h2);
        lo4[i] = __builtin_bit_cast(unsigned, l2);
    }
    const dcn_f16x8 b0 = __builtin_bit_cast(dcn_f16x8, hi4), b1 = __builtin_bit_cast(dcn_f16x8, lo4);
    const dcn_f16x8 w0 = __builtin_bit_cast(dcn_f16x8, wl[(2 * u) * 64 + lane]);
    const dcn_f16x8 w1 = __builtin_bit_cast(dcn_f16x8, wl[(2 * u + 1) * 64 + lane]);
    acl = __builtin_amdgcn_mfma_f32_32x32x16_f16(w0, b1, acl, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(w0, b0, acc, 0, 0, 0);
    acl = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1, b0, acl, 0, 0, 0);
}

__device__ __forceinline__ void dcn_consume_pair(const DcnPair& P, f32x16& acc, f32x16& acl, const f32x4* wl, int u, int lane) {
    float xs[8];
    dcn_lerp_one(P, 0, xs);
    dcn_lerp_one(P, 1, xs);
    dcn_split_mfma(xs, acc, acl, wl, u, lane);
}

// The output epilogue of dcn_g8 in its three kernels (dcn_g8_pipe_kernel, dcn_fused_kernel, lab: dcn_fused2_kernel): the hi / lo sums
// combine, the lane half's four output quads get their bias and are stored, and one flag is raised when a value leaves the fp16 range
// (ConvArgs::ovf: the aligned features feed a split-fp16 conv).  Text, not a function: a function with the same statements moves a few
// instructions of dcn_fused_kernel.  Reads acc, acl, h, n, px, py, W and plane of the kernel it stands in.
#define DCN_G8_EPILOGUE(OUT, OB, BIAS, OVF, OVF_DIV)                                                      \
    _Pragma("unroll") for (int e = 0; e < 16; ++e) acc[e] += acl[e] * (1.0f / 2048.0f);                   \
    act_t* o = as_act(OUT) + (long long)n * (OB) + ((long long)py * W + px) * 4;                          \
    float vmax = 0.0f;                                                                                    \
    _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                       \
        const int cq = 2 * g + h;                                                                         \
        const float4 bb = *reinterpret_cast<const float4*>((BIAS) + 4 * cq);                              \
        const float4 v = make_float4(acc[4 * g] + bb.x, acc[4 * g + 1] + bb.y, acc[4 * g + 2] + bb.z, acc[4 * g + 3] + bb.w); \
        vmax = fmaxf(fmaxf(vmax, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));          \
        stq(o + cq * plane, cf32x4{v.x, v.y, v.z, v.w});                                                  \
    }                                                                                                     \
    if ((OVF) && !(vmax < 65504.0f)) atomicOr(ovf_word((OVF), (OVF_DIV), 0, n), 1u);

}  // namespace CRFP_NS
