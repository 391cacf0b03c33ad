// Streaming helpers of the CRFP path (all HBM-bound, 16 B per lane where the layout allows):
// layout conversion NCHW <-> Q4, bilinear resize (nn.Upsample / F.interpolate, align_corners=False:
// reference model/CRFP.py:776,783,790,808-812,1471-1478), flow upsample + rescale (:1565-1566),
// AvgPool2d(2,2) (:755,762,769), the x8 LR upsample + fovea blend in front of encoder_hr
// (:1538,1542-1547) and the squared-error reduction behind PSNR (utils.py:166-185,328-330).
#include "crfp_common.h"
#include "resample_index.h"

namespace CRFP_NS {

using crfp_index::src_index;   // PyTorch's source index for align_corners=False (shared with the resize backward)

// pad = 1: destination / source planes are (H+1) x (W+1) ("P4"); pads are not touched here
__global__ void nchw_to_q4_kernel(const float* __restrict__ x, act_t* __restrict__ out, int C, int H, int W, int pad, unsigned* __restrict__ ovf,
                                  int ovf_div) {
    const long long HW = (long long)H * W, PHW = (long long)(H + pad) * (W + pad);
    const int nq = (C + 3) / 4;
    const long long total = (long long)nq * HW;
    const int n = blockIdx.y;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int q = (int)(idx / HW);
        const long long pix = idx - (long long)q * HW;
        const long long y = pix / W, xx = pix - y * W;
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = 4 * q + c < C ? x[((long long)n * C + 4 * q + c) * HW + pix] : 0.0f;
        stq(out + (((long long)n * nq + q) * PHW + y * (W + pad) + xx) * 4, cf32x4{v[0], v[1], v[2], v[3]});
        if (ovf && !(fabsf(v[0]) < 65504.0f && fabsf(v[1]) < 65504.0f && fabsf(v[2]) < 65504.0f && fabsf(v[3]) < 65504.0f))
            atomicOr(ovf_word(ovf, ovf_div, 0, n), 1u);   // also true for NaN
    }
}

__global__ void q4_to_nchw_kernel(const act_t* __restrict__ x, float* __restrict__ out, int C, int H, int W, int pad) {
    const long long HW = (long long)H * W, PHW = (long long)(H + pad) * (W + pad);
    const int nq = (C + 3) / 4;
    const long long total = (long long)nq * HW;
    const int n = blockIdx.y;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int q = (int)(idx / HW);
        const long long pix = idx - (long long)q * HW;
        const long long y = pix / W, xx = pix - y * W;
        const cf32x4 v = ldq(x + (((long long)n * nq + q) * PHW + y * (W + pad) + xx) * 4);
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (4 * q + c < C) out[((long long)n * C + 4 * q + c) * HW + pix] = vv[c];
    }
}

static inline int grid_for(long long total) {
    long long b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

int launch_nchw_to_q4(const float* x, float* out, int N, int C, int H, int W, int pad, hipStream_t s, unsigned* ovf, int ovf_div) {
    const long long total = (long long)((C + 3) / 4) * H * W;
    ProfScope prof("nchw_to_q4", s, (double)N * H * W * (C + 4.0 * ((C + 3) / 4)) * 4.0, 0);
    nchw_to_q4_kernel<<<dim3(grid_for(total), N), 256, 0, s>>>(x, as_act(out), C, H, W, pad, ovf, ovf_div);
    CRFP_CHECK_LAUNCH();
    return 0;
}

int launch_q4_to_nchw(const float* x, float* out, int N, int C, int H, int W, int pad, hipStream_t s) {
    const long long total = (long long)((C + 3) / 4) * H * W;
    ProfScope prof("q4_to_nchw", s, (double)N * H * W * (C + 4.0 * ((C + 3) / 4)) * 4.0, 0);
    q4_to_nchw_kernel<<<dim3(grid_for(total), N), 256, 0, s>>>(as_act(x), out, C, H, W, pad);
    CRFP_CHECK_LAUNCH();
    return 0;
}

#ifndef CRFP_ACT_BF16   // per-operator API helper: fp32 build only
// offset[N,noff,H,W] + mask[N,nmask,H,W] (dcn_v2 API tensors) -> Q4 [offset | mask]
__global__ void offmask_to_q4_kernel(const float* __restrict__ off, const float* __restrict__ msk,
                                     float* __restrict__ out, int noff, int nmask, int H, int W) {
    const long long HW = (long long)H * W;
    const int nq = (noff + nmask) / 4;
    const long long total = (long long)nq * HW;
    const int n = blockIdx.y;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int q = (int)(idx / HW);
        const long long pix = idx - (long long)q * HW;
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int ch = 4 * q + c;
            v[c] = ch < noff ? off[((long long)n * noff + ch) * HW + pix] : msk[((long long)n * nmask + ch - noff) * HW + pix];
        }
        *reinterpret_cast<float4*>(out + ((long long)n * nq * HW + idx) * 4) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

int launch_offmask_nchw_to_q4(const float* offset, const float* mask, float* out, int N, int noff, int nmask, int H,
                              int W, hipStream_t s) {
    const long long total = (long long)((noff + nmask) / 4) * H * W;
    ProfScope prof("offmask_nchw_to_q4", s, (double)N * H * W * (noff + nmask) * 8.0, 0);
    offmask_to_q4_kernel<<<dim3(grid_for(total), N), 256, 0, s>>>(offset, mask, out, noff, nmask, H, W);
    CRFP_CHECK_LAUNCH();
    return 0;
}

#endif

// bilinear resize of a Q4 tensor; out = mul * (l0y*(l0x*v00 + l1x*v01) + l1y*(l0x*v10 + l1x*v11))
// out_bgroup > 0: batch item n WRITES destination item n + n / out_bgroup (see ConvArgs::src_bgroup: FNet's per-clip pair mapping)
__global__ void upsample_q4_kernel(const act_t* __restrict__ x, long long xb, act_t* __restrict__ out, long long ob,
                                   int nq, int H, int W, int OH, int OW, float sh, float sw, float mul, int out_bgroup) {
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63);
    const int oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox >= OW || oy >= OH) return;
    const int q = blockIdx.z % nq, n = blockIdx.z / nq;
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    src_index(oy, sh, H, y0, y1, ly0, ly1);
    src_index(ox, sw, W, x0, x1, lx0, lx1);
    const act_t* p = x + (long long)n * xb + (long long)q * H * W * 4;
    const cf32x4 a = ldq(p + ((long long)y0 * W + x0) * 4);
    const cf32x4 b = ldq(p + ((long long)y0 * W + x1) * 4);
    const cf32x4 c = ldq(p + ((long long)y1 * W + x0) * 4);
    const cf32x4 d = ldq(p + ((long long)y1 * W + x1) * 4);
    cf32x4 r;
    r.x = mul * (ly0 * (lx0 * a.x + lx1 * b.x) + ly1 * (lx0 * c.x + lx1 * d.x));
    r.y = mul * (ly0 * (lx0 * a.y + lx1 * b.y) + ly1 * (lx0 * c.y + lx1 * d.y));
    r.z = mul * (ly0 * (lx0 * a.z + lx1 * b.z) + ly1 * (lx0 * c.z + lx1 * d.z));
    r.w = mul * (ly0 * (lx0 * a.w + lx1 * b.w) + ly1 * (lx0 * c.w + lx1 * d.w));
    const int no = out_bgroup > 0 ? n + n / out_bgroup : n;
    stq(out + (long long)no * ob + (((long long)q * OH + oy) * OW + ox) * 4, r);
}

int launch_upsample_q4(const float* x, long long xb, float* out, long long ob, int N, int nq, int H, int W, int OH,
                       int OW, float sh, float sw, float mul, hipStream_t s, int out_bgroup) {
    ProfScope prof("upsample_bilinear_q4", s, (double)N * nq * 16.0 * ((double)H * W + (double)OH * OW), 0);
    dim3 grid((OW + 63) / 64, (OH + 3) / 4, N * nq);
    upsample_q4_kernel<<<grid, 256, 0, s>>>(as_act(x), xb, as_act(out), ob, nq, H, W, OH, OW, sh, sw, mul, out_bgroup);
    CRFP_CHECK_LAUNCH();
    return 0;
}

#ifndef CRFP_ACT_BF16   // float-only helpers (API tensors, flow fields): compiled once, the bf16 engine calls crfp::launch_upflow
__global__ void upsample_nchw_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W, int OH,
                                     int OW, float sh, float sw, float mul) {
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63);
    const int oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox >= OW || oy >= OH) return;
    const long long nc = blockIdx.z;
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    src_index(oy, sh, H, y0, y1, ly0, ly1);
    src_index(ox, sw, W, x0, x1, lx0, lx1);
    const float* p = x + nc * H * W;
    out[(nc * OH + oy) * OW + ox] = mul * (ly0 * (lx0 * p[(long long)y0 * W + x0] + lx1 * p[(long long)y0 * W + x1]) +
                                           ly1 * (lx0 * p[(long long)y1 * W + x0] + lx1 * p[(long long)y1 * W + x1]));
}

int launch_upsample_nchw(const float* x, float* out, int N, int C, int H, int W, int OH, int OW, float sh, float sw,
                         float mul, hipStream_t s) {
    ProfScope prof("upsample_bilinear_nchw", s, (double)N * C * 4.0 * ((double)H * W + (double)OH * OW), 0);
    dim3 grid((OW + 63) / 64, (OH + 3) / 4, N * C);
    upsample_nchw_kernel<<<grid, 256, 0, s>>>(x, out, H, W, OH, OW, sh, sw, mul);
    CRFP_CHECK_LAUNCH();
    return 0;
}

// LR flow (Q4 quad: dx,dy,0,0) -> [rH][rW][2] = r * bilinear_xr(flow)   (img_upsample_rx(flow) * r)
__global__ void upflow_kernel(const float* __restrict__ f, long long fb, float* __restrict__ out, long long ob, int H,
                              int W, int r) {
    const int OW = W * r, OH = H * r;
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63);
    const int oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int n = blockIdx.z;
    if (ox >= OW || oy >= OH) return;
    const float sc = 1.0f / (float)r, mul = (float)r;
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    src_index(oy, sc, H, y0, y1, ly0, ly1);
    src_index(ox, sc, W, x0, x1, lx0, lx1);
    const float* p = f + (long long)n * fb;
    const float2 a = *reinterpret_cast<const float2*>(p + ((long long)y0 * W + x0) * 4);
    const float2 b = *reinterpret_cast<const float2*>(p + ((long long)y0 * W + x1) * 4);
    const float2 c = *reinterpret_cast<const float2*>(p + ((long long)y1 * W + x0) * 4);
    const float2 d = *reinterpret_cast<const float2*>(p + ((long long)y1 * W + x1) * 4);
    float2 o;
    o.x = (ly0 * (lx0 * a.x + lx1 * b.x) + ly1 * (lx0 * c.x + lx1 * d.x)) * mul;
    o.y = (ly0 * (lx0 * a.y + lx1 * b.y) + ly1 * (lx0 * c.y + lx1 * d.y)) * mul;
    *reinterpret_cast<float2*>(out + (long long)n * ob + ((long long)oy * OW + ox) * 2) = o;
}

int launch_upflow(const float* flow_q4, long long fb, float* out_nhw2, long long ob, int N, int H, int W, int r,
                  hipStream_t s) {
    ProfScope prof(r == 8 ? "upflow_x8" : "upflow_x2", s, (double)N * H * W * (8.0 + 8.0 * r * r), 0);
    dim3 grid((W * r + 63) / 64, (H * r + 3) / 4, N);
    upflow_kernel<<<grid, 256, 0, s>>>(flow_q4, fb, out_nhw2, ob, H, W, r);
    CRFP_CHECK_LAUNCH();
    return 0;
}

#endif

// AvgPool2d(2,2), floor mode: out = (v00 + v01 + v10 + v11) / 4 in that order
__global__ void avgpool2_q4_kernel(const act_t* __restrict__ x, long long xb, act_t* __restrict__ out, long long ob,
                                   int nq, int H, int W) {
    const int OH = H / 2, OW = W / 2;
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63);
    const int oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox >= OW || oy >= OH) return;
    const int q = blockIdx.z % nq, n = blockIdx.z / nq;
    const act_t* p = x + (long long)n * xb + (long long)q * H * W * 4;
    const cf32x4 a = ldq(p + ((long long)(2 * oy) * W + 2 * ox) * 4);
    const cf32x4 b = ldq(p + ((long long)(2 * oy) * W + 2 * ox + 1) * 4);
    const cf32x4 c = ldq(p + ((long long)(2 * oy + 1) * W + 2 * ox) * 4);
    const cf32x4 d = ldq(p + ((long long)(2 * oy + 1) * W + 2 * ox + 1) * 4);
    cf32x4 r;
    r.x = (((a.x + b.x) + c.x) + d.x) / 4.0f;
    r.y = (((a.y + b.y) + c.y) + d.y) / 4.0f;
    r.z = (((a.z + b.z) + c.z) + d.z) / 4.0f;
    r.w = (((a.w + b.w) + c.w) + d.w) / 4.0f;
    stq(out + (long long)n * ob + (((long long)q * OH + oy) * OW + ox) * 4, r);
}

int launch_avgpool2_q4(const float* x, long long xb, float* out, long long ob, int N, int nq, int H, int W,
                       hipStream_t s) {
    ProfScope prof("avgpool2_q4", s, (double)N * nq * 16.0 * ((double)H * W * 1.25), 0);
    dim3 grid((W / 2 + 63) / 64, (H / 2 + 3) / 4, N * nq);
    avgpool2_q4_kernel<<<grid, 256, 0, s>>>(as_act(x), xb, as_act(out), ob, nq, H, W);
    CRFP_CHECK_LAUNCH();
    return 0;
}

// One frame: lr[3,h,w], fv[3,8h,8w] NCHW, mk[8h,8w] u8 -> Q4 2 quads at (8h,8w):
//   quad 0 = (mk ? fv : up8(lr)) rgb, 0     (fvs*mk + lrs_lv3*(1-mk) with mk in {0,1} is a select)
//   quad 1 = up8(lr) rgb, 0                 (also the base of the output head)
__global__ void hr_prep_kernel(const float* __restrict__ lr, const float* __restrict__ fv,
                               const uint8_t* __restrict__ mk, act_t* __restrict__ out, int h, int w, long long lr_b,
                               long long fv_b, long long mk_b, long long out_b, const uint8_t* __restrict__ gate, long long gate_b) {
    const int OH = 8 * h, OW = 8 * w;
    const long long n = blockIdx.z;
    // a 64 x 4 block lies inside the 64 x 16 gate tile (blockIdx.x, blockIdx.y / 4)
    if (gate && !gate[n * gate_b + 4 * ((long long)(blockIdx.y >> 2) * gridDim.x + blockIdx.x) + 3]) return;
    lr += n * lr_b; fv += n * fv_b; mk += n * mk_b; out += n * out_b;
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63);
    const int oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox >= OW || oy >= OH) return;
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    src_index(oy, 0.125f, h, y0, y1, ly0, ly1);
    src_index(ox, 0.125f, w, x0, x1, lx0, lx1);
    float u[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = lr + (long long)c * h * w;
        u[c] = ly0 * (lx0 * p[y0 * w + x0] + lx1 * p[y0 * w + x1]) + ly1 * (lx0 * p[y1 * w + x0] + lx1 * p[y1 * w + x1]);
    }
    const long long pix = (long long)oy * OW + ox, plane = (long long)OH * OW;
    const bool m = mk[pix] != 0;
    cf32x4 a = cf32x4{u[0], u[1], u[2], 0.0f};
    if (m) a = cf32x4{fv[pix], fv[plane + pix], fv[2 * plane + pix], 0.0f};
    stq(out + pix * 4, a);
    stq(out + (plane + pix) * 4, cf32x4{u[0], u[1], u[2], 0.0f});
}

int launch_hr_prep(const float* lr, const float* fv, const uint8_t* mk, float* out_q4, int h, int w, hipStream_t s, int N, long long lr_b,
                   long long fv_b, long long mk_b, long long out_b, const uint8_t* gate, long long gate_b) {
    ProfScope prof("hr_prep_up8_blend", s, gate ? 0.0 : (double)N * 64 * h * w * (12 + 1 + 32.0), 0);   // gated: a data-dependent share of the frame
    dim3 grid((8 * w + 63) / 64, (8 * h + 3) / 4, N);
    hr_prep_kernel<<<grid, 256, 0, s>>>(lr, fv, mk, as_act(out_q4), h, w, lr_b, fv_b, mk_b, out_b, gate, gate_b);
    CRFP_CHECK_LAUNCH();
    return 0;
}

// dst (P4 planes) = lrelu_0.1(src) for one quad per batch item: the new recurrent state wherever the fovea mask is clear
// (model/CRFP.py:1674-1675 with mk = 0); the gated conv_tttf launch then rewrites the tiles that hold mask pixels.  The state feeds a
// split-fp16 conv: the range guard of the blend kernel applies here as well.
__global__ void lrelu_q4_to_p4_kernel(const act_t* __restrict__ src, long long src_b, act_t* __restrict__ dst, long long dst_b, int H, int W,
                                      unsigned* __restrict__ ovf, int ovf_div) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), n = blockIdx.z;
    if (x >= W || y >= H) return;
    const cf32x4 v = ldq(src + n * src_b + ((long long)y * W + x) * 4);
    const cf32x4 o = cf32x4{v.x > 0.0f ? v.x : 0.1f * v.x, v.y > 0.0f ? v.y : 0.1f * v.y, v.z > 0.0f ? v.z : 0.1f * v.z, v.w > 0.0f ? v.w : 0.1f * v.w};
    stq(dst + n * dst_b + ((long long)y * (W + 1) + x) * 4, o);
    const float vmax = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w)));
    unsigned* w = ovf_word(ovf, ovf_div, 0, n);
    if (w && !(vmax < 65504.0f)) atomicOr(w, 1u);
}

int launch_lrelu_q4_to_p4(const float* src, long long src_b, float* dst, long long dst_b, int N, int H, int W, unsigned* ovf, int ovf_div, hipStream_t s) {
    ProfScope prof("state_lrelu_copy", s, (double)N * H * W * 8.0 * sizeof(act_t), 0);
    lrelu_q4_to_p4_kernel<<<dim3((W + 63) / 64, (H + 3) / 4, N), 256, 0, s>>>(as_act(src), src_b, as_act(dst), dst_b, H, W, ovf, ovf_div);
    CRFP_CHECK_LAUNCH();
    return 0;
}

// The fovea mask as a tile gate.  The fovea blend is a select (model/CRFP.py:1543-1544,1674), so everything computed only to be
// deselected -- the x8 frame stack, encoder_hr and conv_tttf away from the fovea -- can be skipped tile by tile with identical results.
// Per 64 x 16 tile (the tile grid of the 8x stencil kernels) 4 flag bytes: byte 0 = "a mask pixel is set inside the tile" (conv_tttf has work
// there), byte k = "... inside a tile at most k tiles away" (Chebyshev).  A 3 x 3 conv on an active tile reads its input one pixel into the
// neighbouring tiles, so each producer up the chain runs on one more ring of tiles and no launch ever reads a tile nobody wrote.
__global__ void mask_gate_kernel(const uint8_t* __restrict__ mk, long long mk_b, uint8_t* __restrict__ gate, long long gate_b, int H, int W) {
    const int tile_x = blockIdx.x, tile_y = blockIdx.y, n = blockIdx.z;
    const uint8_t* m = mk + n * mk_b;
    int mine = 0;
    for (int i = threadIdx.x; i < 64 * 16 / 4; i += blockDim.x) {   // 4 mask bytes per thread and step (W is a multiple of 8: 4-byte aligned)
        const int ry = i >> 4, rx = (i & 15) * 4;
        const int y = tile_y * 16 + ry, x = tile_x * 64 + rx;
        if (y < H && x < W) mine |= *reinterpret_cast<const unsigned*>(m + (long long)y * W + x) != 0u;
    }
    const int any = __syncthreads_or(mine);
    if (threadIdx.x == 0) gate[n * gate_b + 4 * ((long long)tile_y * gridDim.x + tile_x)] = any ? 1 : 0;
}

__global__ void mask_gate_rings_kernel(uint8_t* __restrict__ gate, long long gate_b, int tiles_x, int tiles_y) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
    if (t >= tiles_x * tiles_y) return;
    uint8_t* g = gate + n * gate_b;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    // all 49 flags first (clamped addresses, independent loads), then the distance to the nearest tile with mask pixels (4 = none within 3)
    uint8_t f[7][7];
#pragma unroll
    for (int dy = -3; dy <= 3; ++dy)
#pragma unroll
        for (int dx = -3; dx <= 3; ++dx) f[dy + 3][dx + 3] = g[4 * (min(max(ty + dy, 0), tiles_y - 1) * tiles_x + min(max(tx + dx, 0), tiles_x - 1))];
    int ring = 4;
#pragma unroll
    for (int dy = -3; dy <= 3; ++dy)
#pragma unroll
        for (int dx = -3; dx <= 3; ++dx) {
            const bool inb = ty + dy >= 0 && ty + dy < tiles_y && tx + dx >= 0 && tx + dx < tiles_x;
            if (inb && f[dy + 3][dx + 3]) ring = min(ring, max(abs(dy), abs(dx)));
        }
    for (int k = 1; k < 4; ++k) g[4 * t + k] = ring <= k ? 1 : 0;
}

int launch_mask_gate(const uint8_t* mk, long long mk_b, uint8_t* gate, long long gate_b, int N, int H8, int W8, hipStream_t s) {
    const int tiles_x = (W8 + 63) / 64, tiles_y = (H8 + 15) / 16;
    {
        ProfScope prof("mask_gate", s, (double)N * H8 * W8, 0);
        mask_gate_kernel<<<dim3(tiles_x, tiles_y, N), 64, 0, s>>>(mk, mk_b, gate, gate_b, H8, W8);
        CRFP_CHECK_LAUNCH();
    }
    ProfScope prof("mask_gate_rings", s, (double)N * tiles_x * tiles_y * 8.0, 0);
    mask_gate_rings_kernel<<<dim3((tiles_x * tiles_y + 255) / 256, N), 256, 0, s>>>(gate, gate_b, tiles_x, tiles_y);
    CRFP_CHECK_LAUNCH();
    return 0;
}

#ifndef CRFP_ACT_BF16
// Regional mask of the streaming variant (reference model/CRFP_test.py:2296-2298): fg [8h,8w] (bool) ->
// nn.Upsample(scale_factor=0.25, bilinear, align_corners=False) = mean of the centre 2x2 of each 4x4 block
// (source index 4*d + 1.5 -> taps 4d+1, 4d+2 with weight 0.5 each), at 2x resolution.
__global__ void fg_prep_kernel(const uint8_t* __restrict__ fg, float* __restrict__ fg2, int H2, int W2) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W2 || y >= H2) return;
    const int W8 = 4 * W2;
    const uint8_t* p = fg + (long long)(4 * y + 1) * W8 + 4 * x + 1;
    const float a = p[0] ? 1.0f : 0.0f, b = p[1] ? 1.0f : 0.0f, c = p[W8] ? 1.0f : 0.0f, d = p[W8 + 1] ? 1.0f : 0.0f;
    fg2[(long long)y * W2 + x] = 0.5f * (0.5f * a + 0.5f * b) + 0.5f * (0.5f * c + 0.5f * d);
}

int launch_fg_prep(const uint8_t* fg, float* fg2, int H8, int W8, hipStream_t s) {
    const int H2 = H8 / 4, W2 = W8 / 4;
    ProfScope prof("fg_prep", s, (double)H8 * W8 + 4.0 * H2 * W2, 0);
    fg_prep_kernel<<<dim3((W2 + 63) / 64, (H2 + 3) / 4), 256, 0, s>>>(fg, fg2, H2, W2);
    CRFP_CHECK_LAUNCH();
    return 0;
}

#endif

__global__ void scale_q4_kernel(const act_t* __restrict__ src, int src_pad, act_t* __restrict__ dst, int H, int W,
                                const float* __restrict__ sf, const uint8_t* __restrict__ su) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), q = blockIdx.z;
    if (x >= W || y >= H) return;
    const long long pix = (long long)y * W + x;
    const float sc = sf ? sf[pix] : (su[pix] ? 1.0f : 0.0f);
    const cf32x4 v = ldq(src + (((long long)q * (H + src_pad) + y) * (W + src_pad) + x) * 4);
    stq(dst + ((long long)q * H * W + pix) * 4, v * sc);
}

int launch_scale_q4(const float* src, int src_pad, float* dst, int nq, int H, int W, const float* scale_f,
                    const uint8_t* scale_u8, hipStream_t s) {
    ProfScope prof("scale_q4_fg", s, (double)nq * H * W * 32.0, 0);
    scale_q4_kernel<<<dim3((W + 63) / 64, (H + 3) / 4, nq), 256, 0, s>>>(as_act(src), src_pad, as_act(dst), H, W, scale_f, scale_u8);
    CRFP_CHECK_LAUNCH();
    return 0;
}

// CRFP_DSV_CRA's cross-resolution fusion at one 2x level (reference model/CRFP.py:2533-2535 and twins): out = mk2 * fused + (1 - mk2) * y with
// mk2 = F.interpolate(mk.float(), scale_factor=0.25, bilinear) -- at that ratio the mean of the centre 2 x 2 pixels of every 4 x 4 block
// (source coordinate 4 d + 1.5, weights 1/2, 1/2) -- and the 32 output channels split into the propagated 24 (plain Q4) and the
// carried 8 (P4 planes), exactly where the residual block's second conv puts them in the plain CRFP_DSV wiring
__global__ void cra_blend_kernel(const act_t* __restrict__ y, long long y_b, const act_t* __restrict__ f, long long f_b,
                                 const uint8_t* __restrict__ mk, long long mk_b, act_t* __restrict__ prop, long long prop_b,
                                 act_t* __restrict__ carry, long long carry_b, int H, int W) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), yy = blockIdx.y * 4 + (threadIdx.x >> 6), n = blockIdx.z;
    if (x >= W || yy >= H) return;
    const uint8_t* m = mk + n * mk_b + (long long)(4 * yy + 1) * (4 * W) + 4 * x + 1;
    const float a = m[0] ? 1.0f : 0.0f, b = m[1] ? 1.0f : 0.0f, c = m[4 * W] ? 1.0f : 0.0f, d = m[4 * W + 1] ? 1.0f : 0.0f;
    const float mk2 = (a * 0.5f + b * 0.5f) * 0.5f + (c * 0.5f + d * 0.5f) * 0.5f, inv = 1.0f - mk2;
    const long long pix = (long long)yy * W + x, plane = (long long)H * W;
    for (int q = 0; q < 8; ++q) {
        const cf32x4 vy = ldq(y + n * y_b + (q * plane + pix) * 4), vf = ldq(f + n * f_b + (q * plane + pix) * 4);
        const cf32x4 o = vf * mk2 + vy * inv;
        if (q < 6) stq(prop + n * prop_b + (q * plane + pix) * 4, o);
        else stq(carry + n * carry_b + (((long long)(q - 6) * (H + 1) + yy) * (W + 1) + x) * 4, o);
    }
}

int launch_cra_blend(const float* y, long long y_b, const float* fused, long long f_b, const uint8_t* mk, long long mk_b, float* prop,
                     long long prop_b, float* carry, long long carry_b, int N, int H, int W, hipStream_t s) {
    ProfScope prof("cra_blend", s, (double)N * H * W * (3.0 * 32 * sizeof(act_t) + 4.0), 0);
    cra_blend_kernel<<<dim3((W + 63) / 64, (H + 3) / 4, N), 256, 0, s>>>(as_act(y), y_b, as_act(fused), f_b, mk, mk_b, as_act(prop), prop_b,
                                                                      as_act(carry), carry_b, H, W);
    CRFP_CHECK_LAUNCH();
    return 0;
}

#ifndef CRFP_ACT_BF16
// nn.AvgPool2d(2, 2) on NCHW planes (floor mode: a trailing odd row / column is dropped) -- FNet's pooling (model/CRFP.py:755)
__global__ void avgpool2_nchw_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W, int OH, int OW) {
    const long long plane = blockIdx.y;
    const float* px = x + plane * H * W;
    float* po = out + plane * OH * OW;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < OH * OW; i += gridDim.x * blockDim.x) {
        const int oy = i / OW, ox = i - oy * OW;
        const float* p = px + (long long)(2 * oy) * W + 2 * ox;
        po[i] = ((p[0] + p[1]) + (p[W] + p[W + 1])) * 0.25f;
    }
}

int launch_avgpool2_nchw(const float* x, float* out, int N, int C, int H, int W, hipStream_t s) {
    const int OH = H / 2, OW = W / 2;
    ProfScope prof("avgpool2_nchw", s, (double)N * C * ((double)H * W + (double)OH * OW) * 4.0, 0);
    int blocks = (OH * OW + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    avgpool2_nchw_kernel<<<dim3(blocks, N * C), 256, 0, s>>>(x, out, H, W, OH, OW);
    CRFP_CHECK_LAUNCH();
    return 0;
}

// acc[0] += sum (a-b)^2 ; acc[1] += sum (Y(a)-Y(b))^2 with Y = 24.966*c0 + 128.553*c1 + 65.481*c2 + 16
__global__ void psnr_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ acc,
                                    int C, long long HW) {
    const int n = blockIdx.y;
    double s0 = 0.0, s1 = 0.0;
    for (long long pix = (long long)blockIdx.x * blockDim.x + threadIdx.x; pix < HW;
         pix += (long long)gridDim.x * blockDim.x) {
        float ya = 16.0f, yb = 16.0f;
        const float wy[3] = {24.966f, 128.553f, 65.481f};
        for (int c = 0; c < C; ++c) {
            const float va = a[((long long)n * C + c) * HW + pix], vb = b[((long long)n * C + c) * HW + pix];
            const float d = va - vb;
            s0 += (double)d * d;
            if (C == 3) { ya += wy[c] * va; yb += wy[c] * vb; }
        }
        if (C == 3) { const float d = ya - yb; s1 += (double)d * d; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_down(s0, o);
        s1 += __shfl_down(s1, o);
    }
    __shared__ double sh[2][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { sh[0][wv] = s0; sh[1][wv] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&acc[0], sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3]);
        atomicAdd(&acc[1], sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3]);
    }
}

int launch_psnr_partial(const float* a, const float* b, double* acc, int N, int C, int H, int W, hipStream_t s) {
    const long long HW = (long long)H * W;
    ProfScope prof("psnr_partial", s, (double)N * C * HW * 8.0, 0);
    int blocks = (int)((HW + 255) / 256);
    if (blocks > 1024) blocks = 1024;
    psnr_partial_kernel<<<dim3(blocks, N), 256, 0, s>>>(a, b, acc, C, HW);
    CRFP_CHECK_LAUNCH();
    return 0;
}
#endif

}  // namespace CRFP_NS
