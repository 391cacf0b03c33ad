// Irregular gathers of the CRFP path on gfx950: bilinear backward warp (reference flow_warp,
// model/CRFP.py:90-130 -> ATen grid_sampler_2d) and the modulated deformable convolution the
// reference imports from the third-party dcn_v2 package (model/CRFP.py:6,318-320,350).
//
// All feature maps are Q4 (4 channels of a pixel = one aligned 16-B element), so every bilinear
// corner is ONE global_load_dwordx4 per lane and neighbouring lanes (neighbouring pixels, smooth
// flow) hit consecutive 16-B elements: the four corner loads of a wave cover two nearly contiguous
// 1-KiB row segments that the CU's L1 serves 3 times out of 4; HBM sees each input line once.
#include "crfp_common.h"
#include "dcn_sampler.h"
#include <atomic>
#include <cstdlib>
#include <cstdio>
#include <cstring>

namespace CRFP_NS {

// ---------------------------------------------------------------- flow_warp
// Coordinate arithmetic restates the reference bit for bit in float32:
//   g = x + flow_x;  gn = 2*g/max(W-1,1) - 1          (model/CRFP.py:118-121)
//   ix = (gn + 1) * ((W-1)/2)                         (ATen CPU grid_sampler, align_corners=True)
// zeros padding: each out-of-range corner contributes 0; border: ix clamped to [0, W-1].
typedef float f32x2_t __attribute__((ext_vector_type(2)));
// flow vectors are read once per launch: non-temporal (the gathered planes keep the cache)
__device__ __forceinline__ float2 ldnt2(const float* p) {
    const f32x2_t v = __builtin_nontemporal_load(reinterpret_cast<const f32x2_t*>(p));
    return make_float2(v.x, v.y);
}

#ifndef CRFP_ACT_BF16   // unpadded Q4 sources (per-operator API, border mode): fp32 build only
template <int BORDER>
__global__ __launch_bounds__(256) void flow_warp_q4_kernel(const float* __restrict__ x, long long xb,
                                                           const float* __restrict__ flow, long long fb,
                                                           float* __restrict__ out, long long ob, int nq, int H,
                                                           int W) {
    const int px = blockIdx.x * 64 + (threadIdx.x & 63);
    const int py = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int n = blockIdx.z;
    if (px >= W || py >= H) return;
    const long long pix = (long long)py * W + px;
    const float2 f = ldnt2(flow + (long long)n * fb + pix * 2);
    const float dw = (float)(W - 1 > 1 ? W - 1 : 1), dh = (float)(H - 1 > 1 ? H - 1 : 1);
    const float gx = 2.0f * ((float)px + f.x) / dw - 1.0f;
    const float gy = 2.0f * ((float)py + f.y) / dh - 1.0f;
    float ix = (gx + 1.0f) * ((float)(W - 1) / 2.0f);
    float iy = (gy + 1.0f) * ((float)(H - 1) / 2.0f);
    if (BORDER) {
        ix = fminf(fmaxf(ix, 0.0f), (float)(W - 1));
        iy = fminf(fmaxf(iy, 0.0f), (float)(H - 1));
    }
    // keep the float->int conversion in range; anything beyond one pixel outside samples zero anyway
    ix = fminf(fmaxf(ix, -2.0f), (float)W + 1.0f);
    iy = fminf(fmaxf(iy, -2.0f), (float)H + 1.0f);
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
    const float lx = ix - fx, ly = iy - fy, hx = 1.0f - lx, hy = 1.0f - ly;
    const bool vx0 = x0 >= 0 && x0 < W, vx1 = x1 >= 0 && x1 < W, vy0 = y0 >= 0 && y0 < H, vy1 = y1 >= 0 && y1 < H;
    const float w00 = (vy0 && vx0) ? hy * hx : 0.0f, w01 = (vy0 && vx1) ? hy * lx : 0.0f;
    const float w10 = (vy1 && vx0) ? ly * hx : 0.0f, w11 = (vy1 && vx1) ? ly * lx : 0.0f;
    const int cx0 = min(max(x0, 0), W - 1), cx1 = min(max(x1, 0), W - 1);
    const int cy0 = min(max(y0, 0), H - 1), cy1 = min(max(y1, 0), H - 1);
    const long long o00 = ((long long)cy0 * W + cx0) * 4, o01 = ((long long)cy0 * W + cx1) * 4;
    const long long o10 = ((long long)cy1 * W + cx0) * 4, o11 = ((long long)cy1 * W + cx1) * 4;
    const float* xs = x + (long long)n * xb;
    float* os = out + (long long)n * ob + pix * 4;
    const long long plane = (long long)H * W * 4;
    for (int q = 0; q < nq; ++q) {
        const float* p = xs + q * plane;
        const float4 a = *reinterpret_cast<const float4*>(p + o00);
        const float4 b = *reinterpret_cast<const float4*>(p + o01);
        const float4 c = *reinterpret_cast<const float4*>(p + o10);
        const float4 d = *reinterpret_cast<const float4*>(p + o11);
        float4 r;
        r.x = a.x * w00 + b.x * w01 + c.x * w10 + d.x * w11;
        r.y = a.y * w00 + b.y * w01 + c.y * w10 + d.y * w11;
        r.z = a.z * w00 + b.z * w01 + c.z * w10 + d.z * w11;
        r.w = a.w * w00 + b.w * w01 + c.w * w10 + d.w * w11;
        *reinterpret_cast<float4*>(os + q * plane) = r;
    }
}

#endif

// The per-pixel program of the P4 warp, written once for its two callers: flow_warp_p4_kernel (U = 1) and the warp workgroups of a fused DCN
// launch (dcn_fused.inc, U pixels of a lane in flight).  Pixel u of the lane is (px[u], py[u]) of batch item n[u] (n, py: wave-uniform); every
// lane computes and loads -- the caller hands lanes without a pixel the coordinates of one that exists -- and st[u] says whether it stores.
// Per quad all U flow reads, then all 4 U corner loads go out before the first blend.
template <int U>
__device__ __forceinline__ void flow_warp_p4_pixels(const float* __restrict__ x, long long xb, const float* __restrict__ flow, long long fb,
                                                    float* __restrict__ out, long long ob, int nq, int H, int W, const int (&n)[U],
                                                    const int (&px)[U], const int (&py)[U], const bool (&st)[U]) {
    const float dw = (float)(W - 1 > 1 ? W - 1 : 1), dh = (float)(H - 1 > 1 ? H - 1 : 1);
    const int PW = W + 1, pitch = PW * QB, plane_b = (H + 1) * pitch;
    // the descriptor starts one pad row + one element BEFORE plane 0 (zeroed guard that every P4
    // allocation carries) so that (y0,x0) = (-1,-1) is still a non-negative offset
    const int guard = pitch + QB;
    const long long oplane = (long long)H * W * 4;
    float2 f[U];
#pragma unroll
    for (int u = 0; u < U; ++u) f[u] = ldnt2(flow + (long long)n[u] * fb + ((long long)py[u] * W + px[u]) * 2);
    float w00[U], w01[U], w10[U], w11[U];
    int voff[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const float gx = 2.0f * ((float)px[u] + f[u].x) / dw - 1.0f;
        const float gy = 2.0f * ((float)py[u] + f[u].y) / dh - 1.0f;
        float ix = (gx + 1.0f) * ((float)(W - 1) / 2.0f);
        float iy = (gy + 1.0f) * ((float)(H - 1) / 2.0f);
        ix = fminf(fmaxf(ix, -1.0f), (float)W);
        iy = fminf(fmaxf(iy, -1.0f), (float)H);
        const float fx = floorf(ix), fy = floorf(iy);
        const float lx = ix - fx, ly = iy - fy, hx = 1.0f - lx, hy = 1.0f - ly;
        w00[u] = hy * hx; w01[u] = hy * lx; w10[u] = ly * hx; w11[u] = ly * lx;
        voff[u] = ((int)fy * PW + (int)fx) * QB + guard;
    }
    for (int q = 0; q < nq; ++q) {
        pairraw_t tp[U], bt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
                (char*)const_cast<act_t*>(as_act(x) + (long long)n[u] * xb) - guard, 0, nq * plane_b + guard, 0x00020000);
            const int vo = voff[u] + q * plane_b;
            tp[u] = bload_pair(r, vo, 0); bt[u] = bload_pair(r, vo, pitch);
        }
        if (U > 1) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            act_t* os = as_act(out) + (long long)n[u] * ob + ((long long)py[u] * W + px[u]) * 4;
            if (st[u]) stq(os + q * oplane, pair_lo(tp[u]) * w00[u] + pair_hi(tp[u]) * w01[u] + pair_lo(bt[u]) * w10[u] + pair_hi(bt[u]) * w11[u]);
        }
    }
}

__global__ __launch_bounds__(256) void flow_warp_p4_kernel(const float* __restrict__ x, long long xb,
                                                           const float* __restrict__ flow, long long fb,
                                                           float* __restrict__ out, long long ob, int nq, int H,
                                                           int W) {
    const int px = blockIdx.x * 64 + (threadIdx.x & 63);
    const int py = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (px >= W || py >= H) return;
    flow_warp_p4_pixels<1>(x, xb, flow, fb, out, ob, nq, H, W, {(int)blockIdx.z}, {px}, {py}, {true});
}

// Two P4 tensors warped by the same flow field in one launch (the engine warps prev2 [8 quads] and the carried features
// [6 quads] with flow2 every frame: model/CRFP.py:1570-1582): the flow read and the coordinate arithmetic are shared, and
// the corner gathers go out in batches of up to 4 quads (16 loads in flight) instead of one quad at a time -- the
// runtime-nq loop above waits for every quad's four loads before it issues the next four.
template <int NQ>
__device__ __forceinline__ void warp_quads(__amdgpu_buffer_rsrc_t r, int voff, int pitch, int plane_b, float w00, float w01,
                                           float w10, float w11, act_t* os, long long oplane) {
#pragma unroll
    for (int q0 = 0; q0 < NQ; q0 += 4) {
        constexpr int B = 4;
        pairraw_t tp[B], bt[B];
#pragma unroll
        for (int i = 0; i < B; ++i)
            if (q0 + i < NQ) {
                const int vo = voff + (q0 + i) * plane_b;
                tp[i] = bload_pair(r, vo, 0); bt[i] = bload_pair(r, vo, pitch);
            }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < B; ++i)
            if (q0 + i < NQ)
                stq(os + (q0 + i) * oplane, pair_lo(tp[i]) * w00 + pair_hi(tp[i]) * w01 + pair_lo(bt[i]) * w10 + pair_hi(bt[i]) * w11);
    }
}

// NW waves = NW rows x 64 pixels per workgroup: with 4-row tiles the source window of a tile (rows + shift + 1 bilinear row) is
// 1.27x the tile and neighbouring tiles sit on different XCDs (no shared L2): PMC 127.6 MB for 106.9 MB algorithmic (round 2).
// 8-row tiles (window 1.14x) were measured in round 3 and are no faster (26.5 vs 26.0-26.4 us same box): the kernel is latency-, not
// byte-bound.
template <int NQA, int NQB, int NW>
__global__ __launch_bounds__(64 * NW) void flow_warp_p4_dual_kernel(const float* __restrict__ xa, const float* __restrict__ xb_,
                                                                    const float* __restrict__ flow, float* __restrict__ outa,
                                                                    float* __restrict__ outb, int H, int W, const WarpDualStrides bs) {
    const int px = blockIdx.x * 64 + (threadIdx.x & 63);
    const int py = blockIdx.y * NW + (threadIdx.x >> 6);
    if (px >= W || py >= H) return;
    const long long n = blockIdx.z;   // batch item: strides in elements of each tensor's own type
    flow += n * bs.flow;
    const long long pix = (long long)py * W + px;
    const float2 f = ldnt2(flow + pix * 2);
    const float dw = (float)(W - 1 > 1 ? W - 1 : 1), dh = (float)(H - 1 > 1 ? H - 1 : 1);
    const float gx = 2.0f * ((float)px + f.x) / dw - 1.0f;
    const float gy = 2.0f * ((float)py + f.y) / dh - 1.0f;
    float ix = (gx + 1.0f) * ((float)(W - 1) / 2.0f);
    float iy = (gy + 1.0f) * ((float)(H - 1) / 2.0f);
    ix = fminf(fmaxf(ix, -1.0f), (float)W);
    iy = fminf(fmaxf(iy, -1.0f), (float)H);
    const float fx = floorf(ix), fy = floorf(iy);
    const float lx = ix - fx, ly = iy - fy, hx = 1.0f - lx, hy = 1.0f - ly;
    const float w00 = hy * hx, w01 = hy * lx, w10 = ly * hx, w11 = ly * lx;
    const int PW = W + 1, pitch = PW * QB, plane_b = (H + 1) * pitch;
    const int guard = pitch + QB;   // see flow_warp_p4_kernel
    const int voff = ((int)fy * PW + (int)fx) * QB + guard;
    const long long oplane = (long long)H * W * 4;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((char*)const_cast<act_t*>(as_act(xa) + n * bs.xa) - guard, 0,
                                                                        NQA * plane_b + guard, 0x00020000);
    warp_quads<NQA>(ra, voff, pitch, plane_b, w00, w01, w10, w11, as_act(outa) + n * bs.outa + pix * 4, oplane);
    if (NQB > 0) {
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((char*)const_cast<act_t*>(as_act(xb_) + n * bs.xb) - guard, 0,
                                                                            NQB * plane_b + guard, 0x00020000);
        warp_quads<NQB>(rb, voff, pitch, plane_b, w00, w01, w10, w11, as_act(outb) + n * bs.outb + pix * 4, oplane);
    }
}

// Round 5: the same launch with the quads of a pixel SPLIT over blockIdx.z groups of GQ quads.  The kernel above walks its 14 quads in
// four dependent batches (16 gathers, 4 stores, next batch): ~4 memory round trips per thread on a grid that fills 44 % of the chip's wave
// slots (900 workgroups of 4 waves on 256 CUs), which is why it sat at 0.50-0.56 of the HBM rate while the one-quad warp of the 8x state
// (one batch per thread, 57 600 workgroups) reaches 0.70.  Here every thread owns ONE batch: group g of a pixel = GQ quads of prev2 or of
// the carry, all its gathers in flight at once, (GA + GB) x as many workgroups; flow read and coordinate arithmetic are repeated per
// group (8 of ~470 bytes per pixel).  Same operations on the same values per output element: bit-identical.
template <int NQA, int NQB, int GQ>
__global__ __launch_bounds__(256) void flow_warp_p4_dual_split_kernel(const float* __restrict__ xa, const float* __restrict__ xb_,
                                                                      const float* __restrict__ flow, float* __restrict__ outa,
                                                                      float* __restrict__ outb, int H, int W, const WarpDualStrides bs) {
    constexpr int GA = (NQA + GQ - 1) / GQ, GB = (NQB + GQ - 1) / GQ, NG = GA + GB;
    const int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    const int px = bx * 64 + (threadIdx.x & 63);
    const int py = by * 4 + (threadIdx.x >> 6);
    if (px >= W || py >= H) return;
    const int g = bz % NG;
    const long long n = bz / NG;
    flow += n * bs.flow;
    const long long pix = (long long)py * W + px;
    const float2 f = ldnt2(flow + pix * 2);
    const float dw = (float)(W - 1 > 1 ? W - 1 : 1), dh = (float)(H - 1 > 1 ? H - 1 : 1);
    const float gx = 2.0f * ((float)px + f.x) / dw - 1.0f;
    const float gy = 2.0f * ((float)py + f.y) / dh - 1.0f;
    float ix = (gx + 1.0f) * ((float)(W - 1) / 2.0f);
    float iy = (gy + 1.0f) * ((float)(H - 1) / 2.0f);
    ix = fminf(fmaxf(ix, -1.0f), (float)W);
    iy = fminf(fmaxf(iy, -1.0f), (float)H);
    const float fx = floorf(ix), fy = floorf(iy);
    const float lx = ix - fx, ly = iy - fy, hx = 1.0f - lx, hy = 1.0f - ly;
    const float w00 = hy * hx, w01 = hy * lx, w10 = ly * hx, w11 = ly * lx;
    const int PW = W + 1, pitch = PW * QB, plane_b = (H + 1) * pitch;
    const int guard = pitch + QB;   // see flow_warp_p4_kernel
    const long long oplane = (long long)H * W * 4;
    const bool isb = g >= GA;       // workgroup-uniform
    const int q0 = (isb ? g - GA : g) * GQ, nq = isb ? NQB : NQA;
    const act_t* src = isb ? as_act(xb_) + n * bs.xb : as_act(xa) + n * bs.xa;
    act_t* os = (isb ? as_act(outb) + n * bs.outb : as_act(outa) + n * bs.outa) + pix * 4 + q0 * oplane;
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((char*)const_cast<act_t*>(src) - guard, 0, nq * plane_b + guard, 0x00020000);
    const int voff = ((int)fy * PW + (int)fx) * QB + guard + q0 * plane_b;
    const int cnt = min(GQ, nq - q0);
    if (cnt == GQ) warp_quads<GQ>(r, voff, pitch, plane_b, w00, w01, w10, w11, os, oplane);
    else if (GQ > 1 && cnt == 1) warp_quads<1>(r, voff, pitch, plane_b, w00, w01, w10, w11, os, oplane);
    else if (GQ > 2 && cnt == 2) warp_quads<2>(r, voff, pitch, plane_b, w00, w01, w10, w11, os, oplane);
    else if (GQ > 3 && cnt == 3) warp_quads<3>(r, voff, pitch, plane_b, w00, w01, w10, w11, os, oplane);
}

bool flow_warp_dual_split(int N) { return N * 4 <= 65535; }

// prev2 (8 quads) + carry (6 quads) by flow2, one launch; zeros padding, P4 sources
int launch_flow_warp_p4_dual_8_6(const float* xa, const float* xb, const float* flow, float* outa, float* outb, int H, int W,
                                 hipStream_t s, int N, const WarpDualStrides& bs) {
    const double px = (double)N * H * W;
    ProfScope prof("flow_warp_q4_c32+c24", s, px * (2.0 * 14 * 4 * sizeof(act_t) + 8), px * 14 * 4 * 7.0);
    const dim3 g4((W + 63) / 64, (H + 3) / 4, N);
    if (flow_warp_dual_split(N)) flow_warp_p4_dual_split_kernel<8, 6, 4><<<dim3(g4.x, g4.y, N * 4), 256, 0, s>>>(xa, xb, flow, outa, outb, H, W, bs);
    else flow_warp_p4_dual_kernel<8, 6, 4><<<g4, 256, 0, s>>>(xa, xb, flow, outa, outb, H, W, bs);
    CRFP_CHECK_LAUNCH();
    return 0;
}

int launch_flow_warp_q4(const float* x, long long xb, const float* flow, long long fb, float* out, long long ob,
                        int N, int nq, int H, int W, int border, int src_pad, hipStream_t s) {
    const double px = (double)N * H * W;
    ProfScope prof(nq == 1 ? "flow_warp_q4_c4" : (nq == 8 ? "flow_warp_q4_c32" : "flow_warp_q4_c24"), s,
                   px * (2.0 * nq * 4 * sizeof(act_t) + 8), px * nq * 4 * 7.0);
    dim3 grid((W + 63) / 64, (H + 3) / 4, N);
    if (src_pad && !border)
        flow_warp_p4_kernel<<<grid, 256, 0, s>>>(x, xb, flow, fb, out, ob, nq, H, W);
    else if (src_pad) {
        set_error("flow_warp: border padding on a P4 source is not implemented");
        return CRFP_E_UNSUPPORTED;
    }
#ifndef CRFP_ACT_BF16
    else if (border)
        flow_warp_q4_kernel<1><<<grid, 256, 0, s>>>(x, xb, flow, fb, out, ob, nq, H, W);
    else
        flow_warp_q4_kernel<0><<<grid, 256, 0, s>>>(x, xb, flow, fb, out, ob, nq, H, W);
#else
    else {
        set_error("flow_warp: the bf16 build warps padded (P4) sources only");
        return CRFP_E_UNSUPPORTED;
    }
#endif
    CRFP_CHECK_LAUNCH();
    return 0;
}

#ifndef CRFP_ACT_BF16   // generic / fp32-MFMA DCN kernels of the per-operator API: fp32 build only
// ---------------------------------------------------------------- DCNv2 sampling helper
// Published DCNv2 semantics: p = (y - pad + ky*dil + dy, x - pad + kx*dil + dx); value 0 unless
// -1 < p < size; bilinear with every out-of-range corner contributing 0.
struct Corner4 {
    long long o00, o01, o10, o11;
    float w00, w01, w10, w11;
};

__device__ __forceinline__ Corner4 dcn_corners(float py, float px, int H, int W) {
    Corner4 c;
    const bool inside = py > -1.0f && px > -1.0f && py < (float)H && px < (float)W;
    py = fminf(fmaxf(py, -2.0f), (float)H + 1.0f);
    px = fminf(fmaxf(px, -2.0f), (float)W + 1.0f);
    const float fy = floorf(py), fx = floorf(px);
    const int y0 = (int)fy, x0 = (int)fx, y1 = y0 + 1, x1 = x0 + 1;
    const float ly = py - fy, lx = px - fx, hy = 1.0f - ly, hx = 1.0f - lx;
    const bool vy0 = inside && y0 >= 0, vy1 = inside && y1 <= H - 1, vx0 = x0 >= 0, vx1 = x1 <= W - 1;
    c.w00 = (vy0 && vx0) ? hy * hx : 0.0f;
    c.w01 = (vy0 && vx1) ? hy * lx : 0.0f;
    c.w10 = (vy1 && vx0) ? ly * hx : 0.0f;
    c.w11 = (vy1 && vx1) ? ly * lx : 0.0f;
    const int cy0 = min(max(y0, 0), H - 1), cy1 = min(max(y1, 0), H - 1);
    const int cx0 = min(max(x0, 0), W - 1), cx1 = min(max(x1, 0), W - 1);
    c.o00 = ((long long)cy0 * W + cx0) * 4;
    c.o01 = ((long long)cy0 * W + cx1) * 4;
    c.o10 = ((long long)cy1 * W + cx0) * 4;
    c.o11 = ((long long)cy1 * W + cx1) * 4;
    return c;
}

__device__ __forceinline__ float4 sample_quad(const float* __restrict__ plane, const Corner4& c) {
    const float4 a = *reinterpret_cast<const float4*>(plane + c.o00);
    const float4 b = *reinterpret_cast<const float4*>(plane + c.o01);
    const float4 d = *reinterpret_cast<const float4*>(plane + c.o10);
    const float4 e = *reinterpret_cast<const float4*>(plane + c.o11);
    float4 r;
    r.x = c.w00 * a.x + c.w01 * b.x + c.w10 * d.x + c.w11 * e.x;
    r.y = c.w00 * a.y + c.w01 * b.y + c.w10 * d.y + c.w11 * e.y;
    r.z = c.w00 * a.z + c.w01 * b.z + c.w10 * d.z + c.w11 * e.z;
    r.w = c.w00 * a.w + c.w01 * b.w + c.w10 * d.w + c.w11 * e.w;
    return r;
}

#endif

// ---------------------------------------------------------------- DCNv2 32->32, 8 deformable groups
// (dcn_0/1/2 of CRFP_DSV at 2x resolution).  x: Q4 8 quads (quad g = the 4 channels of deformable
// group g).  offmask: Q4 54 quads = the reference's [offset(144) | mask(72)] channel order:
// quad u<36: (dy,dx) of sampling positions 2u, 2u+1 (position p = g*9 + tap); quad 36+v: masks of
// positions 4v..4v+3.  One wave = 32 pixels of a row; lane (pixel, half) samples the 36 positions of
// groups 4*half..4*half+3 and feeds each sampled quad straight into 4 fp32 MFMAs as the B operand
// (K index = (group, tap, channel)); the im2col matrix never exists in memory.
// offset / mask quads are read once per launch (199 MB per dcn_g8): non-temporal, so that they do not push the gathered
// feature planes out of L2 (dcn_g8 93.1 -> 92.2 us)
__device__ __forceinline__ f32x4 ldg4(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)); }

// x is P4 (see above).  VALU budget per sampling position: position (2), clamp (4), floor/frac (6),
// modulated bilinear weights (6), byte offset (4), 16 FMAs for the 4-channel sample.
// The 32x32 GEMM on the fp32 MFMA: the C-ABI op and strict fp32.  (The engine's default is dcn_g8_pipe_kernel below, on the fp16 MFMA
// with the exact two-term split of conv_mfma.hip.)  4 waves = 4 rows per workgroup, sampling positions consumed in pairs.
#ifndef CRFP_ACT_BF16
__global__ __launch_bounds__(256, 4) void dcn_g8_kernel(const float* __restrict__ x, long long xb,
                                                        const float* __restrict__ offmask, long long omb,
                                                        const float* __restrict__ wpk, const float* __restrict__ bias,
                                                        float* __restrict__ out, long long ob, int H, int W) {
    // packed DCN weights (36 KB) are shared by the 4 waves of the workgroup through LDS
    __shared__ f32x4 wl[36 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NP = 2;   // sampling positions whose 8 corner loads are issued back to back
    for (int i = tid; i < 36 * 64; i += 256) wl[i] = reinterpret_cast<const f32x4*>(wpk)[i];
    const int j = lane & 31, h = lane >> 5;
    // (XCD-banded tile order measured here: traffic 316 -> 268 MB but +1.8 % time; the gathers keep the natural order)
    const int px = blockIdx.x * 32 + j, py = blockIdx.y * 4 + wave;
    const int n = blockIdx.z;
    const bool valid = px < W && py < H;
    const int cx = min(px, W - 1), cy = min(py, H - 1);
    const long long plane = (long long)H * W * 4;
    const float* om = offmask + (long long)n * omb + ((long long)cy * W + cx) * 4;
    const int PW = W + 1, pitch = PW * 16, plane_b = (H + 1) * pitch;
    const int guard = pitch + 16;  // zeroed guard in front of plane 0 (see flow_warp_p4_kernel)
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(x + (long long)n * xb) - (guard >> 2), 0, 8 * plane_b + guard, 0x00020000);
    const float fy0 = (float)(cy - 1), fx0 = (float)(cx - 1), fH = (float)H, fW = (float)W;
    const int hbase = 4 * h * plane_b + guard;

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;

    // software pipeline: the (dy,dx) pairs and masks of iteration v+1 are in flight while the 16 corner
    // loads of iteration v (4 sampling positions x 4 corners, issued back to back) are consumed
    f32x4 m4 = ldg4(om + (36 + 9 * h) * plane);
    f32x4 oa = ldg4(om + (18 * h) * plane);
    f32x4 ob4 = ldg4(om + (18 * h + 1) * plane);
    __syncthreads();
#pragma unroll 1
    for (int v = 0; v < 9; ++v) {
        const float dy[4] = {oa.x, oa.z, ob4.x, ob4.z};
        const float dx[4] = {oa.y, oa.w, ob4.y, ob4.w};
        const float mm[4] = {m4.x, m4.y, m4.z, m4.w};
        if (v < 8) {
            m4 = ldg4(om + (36 + 9 * h + v + 1) * plane);
            oa = ldg4(om + (18 * h + 2 * v + 2) * plane);
            ob4 = ldg4(om + (18 * h + 2 * v + 3) * plane);
        }
#pragma unroll
        for (int hb = 0; hb < 4; hb += NP) {
            float w00[NP], w01[NP], w10[NP], w11[NP];
            f32x4 q00[NP], q01[NP], q10[NP], q11[NP];
#pragma unroll
            for (int pi = 0; pi < NP; ++pi) {
                const int pp = hb + pi;
                const int p36 = 4 * v + pp, gi = p36 / 9, tap = p36 - 9 * gi, ky = tap / 3, kx = tap - 3 * ky;
                // (float)(cy-1) + (float)ky is exact, so this equals the reference's (float)(y - pad + ky) + dy
                float sy = (fy0 + (float)ky) + dy[pp];
                float sx = (fx0 + (float)kx) + dx[pp];
                sy = fminf(fmaxf(sy, -1.0f), fH);
                sx = fminf(fmaxf(sx, -1.0f), fW);
                const float fy = floorf(sy), fx = floorf(sx);
                const float ly = sy - fy, lx = sx - fx;
                const float a = (1.0f - ly) * mm[pp], b = ly * mm[pp], hx = 1.0f - lx;
                w00[pi] = a * hx; w01[pi] = a * lx; w10[pi] = b * hx; w11[pi] = b * lx;
                const int vo = ((int)fy * PW + (int)fx) * 16 + hbase + gi * plane_b;
                q00[pi] = bload(rx, vo, 0);
                q01[pi] = bload(rx, vo, 16);
                q10[pi] = bload(rx, vo, pitch);
                q11[pi] = bload(rx, vo, pitch + 16);
            }
#pragma unroll
            for (int pi = 0; pi < NP; ++pi) {
                f32x4 val = q00[pi] * w00[pi];
                val = __builtin_elementwise_fma(q01[pi], f32x4{w01[pi], w01[pi], w01[pi], w01[pi]}, val);
                val = __builtin_elementwise_fma(q10[pi], f32x4{w10[pi], w10[pi], w10[pi], w10[pi]}, val);
                val = __builtin_elementwise_fma(q11[pi], f32x4{w11[pi], w11[pi], w11[pi], w11[pi]}, val);
                const f32x4 wa = wl[(4 * v + hb + pi) * 64 + lane];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa.x, val.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa.y, val.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa.z, val.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa.w, val.w, acc, 0, 0, 0);
            }
        }
    }
    if (!valid) return;
    float* o = out + (long long)n * ob + ((long long)py * W + px) * 4;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int cq = 2 * g + h;
        const float4 bb = *reinterpret_cast<const float4*>(bias + 4 * cq);
        *reinterpret_cast<float4*>(o + cq * plane) =
            make_float4(acc[4 * g] + bb.x, acc[4 * g + 1] + bb.y, acc[4 * g + 2] + bb.z, acc[4 * g + 3] + bb.w);
    }
}

#endif   // fp32 build only

// ---------------------------------------------------------------- dcn_g8, software-pipelined (engine path, f16x3)
// Same mapping as dcn_g8_kernel (wave = 32 pixels of a row, lane half = 4 deformable groups, 36 sampling positions per
// lane, consumed in 18 pairs), but the 8 corner loads of pair b+1 are issued BEFORE pair b is interpolated, split and
// multiplied, and the (dy,dx)/mask quads run two iterations ahead.  In the straight version every pair waited for its own
// gathers, and its VALU (~33 us of instruction issue), gather (~32 us of L1 bandwidth: 1.06 GB of 16-B corner reads) and
// offset traffic (199 MB of HBM) added up instead of overlapping (96 us).
__global__ __launch_bounds__(256, 3) void dcn_g8_pipe_kernel(const float* __restrict__ x, long long xb,
                                                             const float* __restrict__ offmask, long long omb,
                                                             const float* __restrict__ wpk, const float* __restrict__ bias,
                                                             float* __restrict__ out, long long ob, int H, int W,
                                                             unsigned* __restrict__ ovf, int probe, int ovf_div) {
    __shared__ f32x4 wl[36 * 64];   // split-fp16 weight image (36 KB), shared by the 4 waves
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 36 * 64; i += 256) wl[i] = reinterpret_cast<const f32x4*>(wpk)[i];
    const int j = lane & 31, h = lane >> 5;
    const int px = blockIdx.x * 32 + j, py = blockIdx.y * 4 + wave;
    const int n = blockIdx.z;
    const bool valid = px < W && py < H;
    const int cx = min(px, W - 1), cy = min(py, H - 1);
    const long long plane = (long long)H * W * 4;
    // probe == 1 (lab timing experiment, results wrong): every workgroup reads the offsets / masks of the first 4 x 32 pixels
    const float* om = offmask + (long long)n * omb + (probe == 1 ? ((long long)(cy & 3) * W + (cx & 31)) * 4 : ((long long)cy * W + cx) * 4);
    const int PW = W + 1, pitch = PW * QB, plane_b = (H + 1) * pitch;
    const int guard = pitch + QB;  // zeroed guard in front of plane 0 (see flow_warp_p4_kernel)
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        (char*)const_cast<act_t*>(as_act(x) + (long long)n * xb) - guard, 0, 8 * plane_b + guard, 0x00020000);
    const float fy0 = (float)(cy - 1), fx0 = (float)(cx - 1), fH = (float)H, fW = (float)W;
    const int hbase = 4 * h * plane_b + guard;

    f32x16 acc, acl;
#pragma unroll
    for (int e = 0; e < 16; ++e) { acc[e] = 0.0f; acl[e] = 0.0f; }

#define CRFP_DCN_LOAD_OFF(O, V)                                                                           \
    {                                                                                                     \
        const int v_ = min((V), 8);   /* the two look-ahead loads past the end are clamped (unused) */     \
        O.m4 = ldg4(om + (36 + 9 * h + v_) * plane);                                                      \
        O.oa = ldg4(om + (18 * h + 2 * v_) * plane);                                                      \
        O.ob = ldg4(om + (18 * h + 2 * v_ + 1) * plane);                                                  \
    }
#define CRFP_DCN_ISSUE(P, O, HB, V) dcn_issue_pair(P, rx, O, HB, V, fy0, fx0, fH, fW, PW, pitch, plane_b, hbase);
    DcnOff O0, O1, O2;
    DcnPair QA, QB;
    CRFP_DCN_LOAD_OFF(O0, 0)
    CRFP_DCN_LOAD_OFF(O1, 1)
    __syncthreads();
    CRFP_DCN_ISSUE(QA, O0, 0, 0)
    // iteration v: OC = offsets(v) (in registers), ON = offsets(v+1) (landing), OF receives offsets(v+2)
#define CRFP_DCN_ITER(V, OC, ON, OF)                                                                      \
    {                                                                                                     \
        CRFP_DCN_LOAD_OFF(OF, (V) + 2)                                                                    \
        CRFP_DCN_ISSUE(QB, OC, 2, V)                                                                      \
        __builtin_amdgcn_sched_barrier(0);   /* keep the gathers ahead of the math: hipcc otherwise sinks them */ \
        dcn_consume_pair(QA, acc, acl, wl, 2 * (V), lane);                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        if ((V) < 8) CRFP_DCN_ISSUE(QA, ON, 0, (V) + 1)                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        dcn_consume_pair(QB, acc, acl, wl, 2 * (V) + 1, lane);                                            \
        __builtin_amdgcn_sched_barrier(0);                                                                \
    }
#pragma unroll 1
    for (int v3 = 0; v3 < (probe == 2 ? 0 : 9); v3 += 3) {   // probe == 2 (lab): no sampling at all = the fixed cost
        CRFP_DCN_ITER(v3, O0, O1, O2)
        CRFP_DCN_ITER(v3 + 1, O1, O2, O0)
        CRFP_DCN_ITER(v3 + 2, O2, O0, O1)
    }
#undef CRFP_DCN_ITER
#undef CRFP_DCN_ISSUE
#undef CRFP_DCN_LOAD_OFF
    if (!valid) return;
    DCN_G8_EPILOGUE(out, ob, bias, ovf, ovf_div)
}

// the 32 -> 216 offset / mask head + dcn_g8 in one kernel (dcn_fused_kernel, launch_dcn_fused, dcn_fused_enabled)
#include "dcn_fused.inc"

// wpk[((p36*2 + half)*32 + row)*4 + i] = W[row][4*(4*half + p36/9) + i][p36 % 9]
#ifndef CRFP_ACT_BF16
__global__ void dcn_g8_pack_kernel(const float* __restrict__ w, float* __restrict__ wpk) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 36 * 2 * 32 * 4) return;
    const int i = idx & 3, row = (idx >> 2) & 31, half = (idx >> 7) & 1, p36 = idx >> 8;
    const int ci = 4 * (4 * half + p36 / 9) + i, tap = p36 % 9;
    wpk[idx] = w[(row * 32 + ci) * 9 + tap];
}

#endif

// f16 image, same 36 864 bytes: wpk16[((u*2 + part)*64 + lane)*8 + i], lane = half*32 + row, i < 4: position 2u, else 2u+1
__global__ void dcn_g8_pack16_kernel(const float* __restrict__ w, unsigned short* __restrict__ wpk) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 18 * 64 * 8) return;
    const int i = idx & 7, lane = (idx >> 3) & 63, u = idx >> 9;
    const int row = lane & 31, half = lane >> 5;
    const int p36 = 2 * u + (i >> 2), ch = i & 3;
    const int ci = 4 * (4 * half + p36 / 9) + ch, tap = p36 % 9;
    float val = w[(row * 32 + ci) * 9 + tap];
    if (kActBf16) val = (float)(__bf16)val;   // bf16 build: weights are bf16 values (same rule for every conv of the engine)
    const _Float16 p0 = (_Float16)val;
    const _Float16 p1 = (_Float16)((val - (float)p0) * 2048.0f);
    wpk[((u * 2 + 0) * 64 + lane) * 8 + i] = __builtin_bit_cast(unsigned short, p0);
    wpk[((u * 2 + 1) * 64 + lane) * 8 + i] = __builtin_bit_cast(unsigned short, p1);
}

bool dcn_g8_use_f16() {
    static const bool f16 = !precision_env_strict(1);
    return f16;
}

// f16 = true: the engine's split-fp16 image; false: the fp32 image of the per-op C-ABI
int launch_dcn_g8_pack(const float* w, float* wpk, hipStream_t s, bool f16) {
#ifdef CRFP_ACT_BF16
    if (!f16) { set_error("dcn_g8_pack: the bf16 build has the split-fp16 GEMM only"); return CRFP_E_UNSUPPORTED; }
    dcn_g8_pack16_kernel<<<(18 * 64 * 8 + 255) / 256, 256, 0, s>>>(w, (unsigned short*)wpk);
#else
    if (f16) dcn_g8_pack16_kernel<<<(18 * 64 * 8 + 255) / 256, 256, 0, s>>>(w, (unsigned short*)wpk);
    else dcn_g8_pack_kernel<<<(36 * 2 * 32 * 4 + 255) / 256, 256, 0, s>>>(w, wpk);
#endif
    CRFP_CHECK_LAUNCH();
    return 0;
}

int launch_dcn_g8(const float* x, long long xb, const float* offmask, long long omb, const float* wpk,
                  const float* bias, float* out, long long ob, int N, int H, int W, hipStream_t s, bool f16, unsigned* ovf, int ovf_div) {
    if ((long long)(H + 1) * (W + 1) >= (1ll << 24)) { set_error("dcn_g8: plane of %d x %d exceeds the sampler's 2^24-element index range", H, W); return CRFP_E_UNSUPPORTED; }
    const double px = (double)N * H * W;
    ProfScope prof("dcnv2_g8_c32", s, px * ((32 + 32) * sizeof(act_t) + (144 + 72) * 4.0) + 32.0 * 32 * 9 * 4, 2.0 * px * 32 * 32 * 9 + px * 288 * 7);
    const int probe = CRFP_LAB_KNOB("CRFP_DCN_PROBE", 0);
    // measured 89.1 vs 91.7 us for the software-pipelined kernel (and no gain at all until sched_barrier pinned the gathers
    // ahead of the math): mostly bound by the L1 line rate of the 16-B corner gathers and VALU issue
#ifdef CRFP_ACT_BF16
    if (!f16) { set_error("dcn_g8: the bf16 build has the split-fp16 GEMM only"); return CRFP_E_UNSUPPORTED; }
    dcn_g8_pipe_kernel<<<dim3((W + 31) / 32, (H + 3) / 4, N), 256, 0, s>>>(x, xb, offmask, omb, wpk, bias, out, ob, H, W, ovf, probe, ovf_div);
#else
    if (f16)
        dcn_g8_pipe_kernel<<<dim3((W + 31) / 32, (H + 3) / 4, N), 256, 0, s>>>(x, xb, offmask, omb, wpk, bias, out, ob, H, W, ovf, probe, ovf_div);
    else
        dcn_g8_kernel<<<dim3((W + 31) / 32, (H + 3) / 4, N), 256, 0, s>>>(x, xb, offmask, omb, wpk, bias, out, ob, H, W);
#endif
    CRFP_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------- DCNv2 4->4, 1 group, offsets and mask
// shared by the 9 taps (dcn_3 of CRFP_DSV at 8x resolution; the reference tiles the 2+1 channels 9x,
// model/CRFP.py:341-347 -- here they stay compact: offmask3 quad = (dy, dx, mask, -)).
// HBM-bound by bytes: 16 B in (gathered) + 16 B offmask (or, FUSE, the offset feature) + 16 B out per pixel.
//
// Against the round-2 kernel (one tile per workgroup, 144 v_fma_f32 for the channel mix; its LDS staging of the sampling window lost
// to the direct gathers, 96-106 against 73-78 us -- DESIGN.md):
//  * the 4x4 channel mix of the 9 sampled quads runs on v_mfma_f32_4x4x1_16b_f32 like the offset conv above it: lane l
//    supplies A = the weight row of cout l&3 and B = its own pixel's sampled channel, and receives the 4 couts of its own
//    pixel -- 36 MFMAs instead of 144 v_fma_f32, same products in the same order (fp32 in, fp32 accumulate: exact);
//    the weights sit in LDS as [tap][cout] -> float4 over cin (they used to occupy 100 SGPRs);
//  * the bilinear blend of a tap is one multiply and three FMAs per channel (fused, as the CUDA kernel the reference
//    links does it), not 4 mul + 3 add;
//  * a workgroup walks a strip of NT vertically adjacent 4 x 64 tiles: FUSE stages the offset feature's (4 NT + 2) x 66 halo
//    once (one global-load latency and one barrier per NT tiles, the shared halo rows read once), the flow / offset quads of
//    all NT tiles are in flight from the start.
// FUSE: the 4 -> 3 offset / mask conv of dcn_3 (model/CRFP.py:337-347, NE_OFFMASK3 of conv_narrow.hip) runs inside this kernel: `offmask3`
// is then the conv's INPUT (the dcn_3 offset feature g2, one Q4 quad), staged as an fp32 halo tile in LDS; every thread
// computes its own pixel's (dy, dx, mask) with the narrow kernel's 4x4x1-MFMA form in the same order (fp32 build: bit-identical to the
// two-kernel path) and samples at once -- the 59 MB offset / mask tensor and one launch per frame disappear.
__device__ __forceinline__ f32x4 bilerp4(const f32x4& n00, const f32x4& n01, const f32x4& n10, const f32x4& n11, float w00, float w01,
                                         float w10, float w11) {
    f32x4 v;
    v.x = __builtin_fmaf(n11.x, w11, __builtin_fmaf(n10.x, w10, __builtin_fmaf(n01.x, w01, n00.x * w00)));
    v.y = __builtin_fmaf(n11.y, w11, __builtin_fmaf(n10.y, w10, __builtin_fmaf(n01.y, w01, n00.y * w00)));
    v.z = __builtin_fmaf(n11.z, w11, __builtin_fmaf(n10.z, w10, __builtin_fmaf(n01.z, w01, n00.z * w00)));
    v.w = __builtin_fmaf(n11.w, w11, __builtin_fmaf(n10.w, w10, __builtin_fmaf(n01.w, w01, n00.w * w00)));
    return v;
}
// acc(4 couts of the lane's pixel) += W[:, :, tap] . v   on the 4x4x1 MFMA; wv = this lane's cout row over the 4 input channels
__device__ __forceinline__ f32x4 mix4(const f32x4& wv, const f32x4& v, f32x4 a) {
    a = __builtin_amdgcn_mfma_f32_4x4x1f32(wv.x, v.x, a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_4x4x1f32(wv.y, v.y, a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_4x4x1f32(wv.z, v.z, a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_4x4x1f32(wv.w, v.w, a, 0, 0, 0);
    return a;
}

constexpr int DCN3_NT = 3;   // tiles per workgroup strip (12 rows x 64 pixels)
template <bool FUSE>
__global__ __launch_bounds__(256) void dcn3_kernel(const float* __restrict__ x, long long xb,
                                                   const float* __restrict__ offmask3, long long omb,
                                                   const float* __restrict__ w, const float* __restrict__ bias,
                                                   float* __restrict__ out, long long ob, int H, int W,
                                                   const float* __restrict__ flow, const float* __restrict__ wom,
                                                   const float* __restrict__ bom, long long fb) {
    constexpr int NT = DCN3_NT, TR = 4 * NT;         // rows of the strip
    __shared__ f32x4 wmix[36];                       // dcn weight: [tap][cout] -> float4 over the 4 input channels
    __shared__ f32x4 gt[FUSE ? TR + 2 : 1][66];      // FUSE: halo tile of the offset feature
    __shared__ f32x4 wlo[FUSE ? 36 : 1];             // FUSE: offset / mask conv weight, same layout
    const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
    const int n = blockIdx.z;
    const int bx0 = blockIdx.x * 64, by0 = blockIdx.y * TR;
    const int px = bx0 + tx;
    const int cpx = min(px, W - 1);
    if (tid < 36) {
        const int tap = tid >> 2, co = tid & 3;
        wmix[tid] = f32x4{w[(co * 4 + 0) * 9 + tap], w[(co * 4 + 1) * 9 + tap], w[(co * 4 + 2) * 9 + tap], w[(co * 4 + 3) * 9 + tap]};
        if constexpr (FUSE) {
            const float4 wv = reinterpret_cast<const float4*>(wom)[tid];   // packed (tap, comp) -> 4 couts (narrow_pack_kernel, kq = 1)
            float* wf = reinterpret_cast<float*>(wlo) + (tid >> 2) * 16 + (tid & 3);
            wf[0] = wv.x; wf[4] = wv.y; wf[8] = wv.z; wf[12] = wv.w;
        }
    }
    // per-tile inputs of all NT tiles in flight from the start: flow (FUSE) or the compact offset / mask quad
    float2 fl[NT];
    f32x4 omq[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const int cpy = min(by0 + 4 * k + ty, H - 1);
        const long long pix = (long long)cpy * W + cpx;
        if constexpr (FUSE) fl[k] = ldnt2(flow + (long long)n * fb + pix * 2);
        else omq[k] = ldg4(offmask3 + (long long)n * omb + pix * 4);   // read once: non-temporal
    }
    if constexpr (FUSE) {
        const act_t* g2 = as_act(offmask3) + (long long)n * omb;
#pragma unroll
        for (int t = 0; t < ((TR + 2) * 66 + 255) / 256; ++t) {
            const int idx = tid + 256 * t;
            if (idx < (TR + 2) * 66) {
                const int r = idx / 66, c = idx - r * 66;
                const int gy = by0 + r - 1, gx = bx0 + c - 1;
                const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
                const cf32x4 v = ldq(g2 + ((long long)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1)) * 4);
                (&gt[0][0])[idx] = ok ? v : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            }
        }
    }
    __syncthreads();
    const int PW = W + 1, pitch = PW * QB, plane_b = (H + 1) * pitch;
    const int guard = pitch + QB;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        (char*)const_cast<act_t*>(as_act(x) + (long long)n * xb) - guard, 0, plane_b + guard, 0x00020000);
    const float fx0 = (float)(cpx - 1), fH = (float)H, fW = (float)W;
    const float4 bo = *reinterpret_cast<const float4*>(bias);
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const int py = by0 + 4 * k + ty;
        if (by0 + 4 * k >= H) break;                 // workgroup-uniform: the strip's last tiles may lie below the image
        const int cpy = min(py, H - 1);
        f32x4 om;
        if constexpr (FUSE) {
            const float4 b4 = *reinterpret_cast<const float4*>(bom);
            f32x4 a4 = f32x4{b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
                    a4 = mix4(wlo[(ky * 3 + kx) * 4 + (tx & 3)], gt[4 * k + ty + ky][tx + kx], a4);
            om = f32x4{tanh10_plus(a4.x, 10.0f + fl[k].y), tanh10_plus(a4.y, 10.0f + fl[k].x), fast_sigmoid(a4.z), 0.0f};
        } else {
            om = omq[k];
        }
        const float fy0 = (float)(cpy - 1);
        // per-row / per-column sampling coordinates exactly as the reference forms them per tap:
        // (float)(y - 1 + ky) + dy, clamped into [-1, H] (outside that range the sample is 0 either way)
        float ly[3], lx[3];
        int iy[3], ix[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float sy = fminf(fmaxf((fy0 + (float)q) + om.x, -1.0f), fH);
            const float sx = fminf(fmaxf((fx0 + (float)q) + om.y, -1.0f), fW);
            const float fy = floorf(sy), fx = floorf(sx);
            ly[q] = sy - fy; lx[q] = sx - fx;
            iy[q] = (int)fy; ix[q] = (int)fx;
        }
        f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        // The 9 taps share one (dy,dx): away from the borders their integer parts advance by exactly one
        // per tap, so the 36 bilinear corners are a 4x4 neighbourhood -> 16 loads instead of 36.  The
        // fractional parts stay per row / column (float rounding of y-1+ky+dy differs per ky).
        const bool regular = iy[1] == iy[0] + 1 && iy[2] == iy[0] + 2 && ix[1] == ix[0] + 1 && ix[2] == ix[0] + 2;
        if (__all(regular)) {
            const int vo = (iy[0] * PW + ix[0]) * QB + guard;
            pairraw_t nbp[4][2];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c) nbp[r][c] = bload_pair(rx, vo, r * pitch + 2 * c * QB);
            __builtin_amdgcn_sched_barrier(0);   // all gathers in flight together (hipcc otherwise issues and waits row by row)
            f32x4 nb[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                nb[r][0] = pair_lo(nbp[r][0]); nb[r][1] = pair_hi(nbp[r][0]);
                nb[r][2] = pair_lo(nbp[r][1]); nb[r][3] = pair_hi(nbp[r][1]);
            }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float hy = 1.0f - ly[ky], hx = 1.0f - lx[kx];
                    const f32x4 v = bilerp4(nb[ky][kx], nb[ky][kx + 1], nb[ky + 1][kx], nb[ky + 1][kx + 1], hy * hx, hy * lx[kx],
                                            ly[ky] * hx, ly[ky] * lx[kx]);
                    acc = mix4(wmix[(ky * 3 + kx) * 4 + (tx & 3)], v, acc);
                }
                __builtin_amdgcn_sched_barrier(0);   // one tap row's weights live at a time (registers)
            }
        } else {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float hy = 1.0f - ly[ky], hx = 1.0f - lx[kx];
                    const int vo = (iy[ky] * PW + ix[kx]) * QB + guard;
                    const pairraw_t tp = bload_pair(rx, vo, 0), bt = bload_pair(rx, vo, pitch);
                    const f32x4 v = bilerp4(pair_lo(tp), pair_hi(tp), pair_lo(bt), pair_hi(bt), hy * hx, hy * lx[kx], ly[ky] * hx,
                                            ly[ky] * lx[kx]);
                    acc = mix4(wmix[(ky * 3 + kx) * 4 + (tx & 3)], v, acc);
                }
        }
        if (px < W && py < H)
            stq(as_act(out) + (long long)n * ob + ((long long)py * W + px) * 4,
                cf32x4{acc.x * om.z + bo.x, acc.y * om.z + bo.y, acc.z * om.z + bo.z, acc.w * om.z + bo.w});
        __builtin_amdgcn_sched_barrier(0);   // keep the next tile's work out of this one (registers: 5 waves per SIMD)
    }
}

int launch_dcn3(const float* x, long long xb, const float* offmask3, long long omb, const float* w,
                const float* bias, float* out, long long ob, int N, int H, int W, hipStream_t s) {
    const double px = (double)N * H * W;
    // algorithmic bytes reported BOTH ways in DESIGN.md; the profiler record carries the compact
    // figure (4 in + 2 off + 1 mask + 4 out floats per pixel) that this kernel actually needs
    ProfScope prof("dcnv2_shared_c4", s, px * ((4 + 4) * sizeof(act_t) + (2 + 1) * 4.0), px * (2.0 * 4 * 4 * 9 + 36 * 7));
    dim3 grid((W + 63) / 64, (H + 4 * DCN3_NT - 1) / (4 * DCN3_NT), N);
    dcn3_kernel<false><<<grid, 256, 0, s>>>(x, xb, offmask3, omb, w, bias, out, ob, H, W, nullptr, nullptr, nullptr, 0);
    CRFP_CHECK_LAUNCH();
    return 0;
}

// dcn_3 with its offset / mask conv inside: g2 = the conv's input (one Q4 quad), wom / bom = its narrow-packed weights and bias
int launch_dcn3_fused(const float* x, long long xb, const float* g2, long long gb, const float* flow, const float* wom, const float* bom,
                      const float* w, const float* bias, float* out, long long ob, int N, int H, int W, hipStream_t s, long long fb) {
    const double px = (double)N * H * W;
    ProfScope prof("dcnv2_shared_c4_fused", s, px * ((4 + 4 + 4) * sizeof(act_t) + 2 * 4.0), px * (2.0 * 4 * 4 * 9 + 36 * 7 + 2.0 * 4 * 3 * 9));
    dim3 grid((W + 63) / 64, (H + 4 * DCN3_NT - 1) / (4 * DCN3_NT), N);
    dcn3_kernel<true><<<grid, 256, 0, s>>>(x, xb, g2, gb, w, bias, out, ob, H, W, flow, wom, bom, fb);
    CRFP_CHECK_LAUNCH();
    return 0;
}

#ifndef CRFP_ACT_BF16
// ---------------------------------------------------------------- generic DCNv2 (any C / groups), NCHW API tensors
// One thread per (pixel, output channel block of 4).  Correct for every configuration the dcn_v2
// module API accepts with k=3,pad=1,dil=1,stride=1; not a tuned path.
__global__ void dcn_generic_kernel(const float* __restrict__ x, const float* __restrict__ offset,
                                   const float* __restrict__ mask, const float* __restrict__ w,
                                   const float* __restrict__ b, float* __restrict__ out, int cin, int cout, int H, int W,
                                   int dg) {
    const int px = blockIdx.x * 64 + (threadIdx.x & 63);
    const int py = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int n = blockIdx.z;
    if (px >= W || py >= H) return;
    const long long HW = (long long)H * W, pix = (long long)py * W + px;
    const int cpg = cin / dg;
    for (int o0 = 0; o0 < cout; o0 += 4) {
        float acc[4] = {0, 0, 0, 0};
        for (int g = 0; g < dg; ++g)
            for (int tap = 0; tap < 9; ++tap) {
                const float dy = offset[((long long)n * 2 * dg * 9 + 2 * (g * 9 + tap)) * HW + pix];
                const float dx = offset[((long long)n * 2 * dg * 9 + 2 * (g * 9 + tap) + 1) * HW + pix];
                const float m = mask[((long long)n * dg * 9 + g * 9 + tap) * HW + pix];
                Corner4 c = dcn_corners((float)(py - 1 + tap / 3) + dy, (float)(px - 1 + tap % 3) + dx, H, W);
                for (int cc = 0; cc < cpg; ++cc) {
                    const int ci = g * cpg + cc;
                    const float* p = x + ((long long)n * cin + ci) * HW;
                    const float v = (c.w00 * p[c.o00 >> 2] + c.w01 * p[c.o01 >> 2] + c.w10 * p[c.o10 >> 2] +
                                     c.w11 * p[c.o11 >> 2]) * m;
                    for (int o = 0; o < 4; ++o)
                        if (o0 + o < cout) acc[o] = fmaf(w[((long long)(o0 + o) * cin + ci) * 9 + tap], v, acc[o]);
                }
            }
        for (int o = 0; o < 4; ++o)
            if (o0 + o < cout) out[((long long)n * cout + o0 + o) * HW + pix] = acc[o] + b[o0 + o];
    }
}

int launch_dcn_generic(const float* x, const float* offset, const float* mask, const float* w, const float* b,
                       float* out, int N, int cin, int cout, int H, int W, int dg, hipStream_t s) {
    const double px = (double)N * H * W;
    ProfScope prof("dcnv2_generic_nchw", s, px * (cin + 27.0 * dg + cout) * 4.0, 2.0 * px * cin * cout * 9);
    dim3 grid((W + 63) / 64, (H + 3) / 4, N);
    dcn_generic_kernel<<<grid, 256, 0, s>>>(x, offset, mask, w, b, out, cin, cout, H, W, dg);
    CRFP_CHECK_LAUNCH();
    return 0;
}
#endif

}  // namespace CRFP_NS
