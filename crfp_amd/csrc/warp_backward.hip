// flow_warp backward (NCHW fp32 API tensors): the two gradients of crfp_flow_warp_f32 for the autograd form of the flow_warp drop-in
// (crfp_amd/ops.py).  fp32 on the VALU throughout.
//
// The function differentiated is the one flow_warp_q4_kernel<BORDER> (gather.hip) computes, and warp_axis() below restates its coordinate
// arithmetic operation for operation, so that the backward picks the forward's cell and the forward's four weights:
//   g = 2 * (p + f) / max(S - 1, 1) - 1;  i = (g + 1) * ((S - 1) / 2);  border: i clamped to [0, S - 1];  then the range clamp to
//   [-2, S + 1] that keeps the float -> int conversion defined (NaN goes where fmaxf / fminf send it: to the lower bound).
// Only after those clamps is a cell formed, and only a corner inside the plane gets its 64-bit index: a non-finite or huge flow has the
// gradient of the constant the forward computes there (zeros: nothing; border: grad_out at the clamped pixel; grad_flow = 0 in both).
//
//   grad_x     a scatter: grad_out[c] * w_corner added at each valid corner of the (cleared) plane.  A workgroup sums its scatter in an
//              LDS window (its 4 x 64 tile + 8 px on every side, WB_CH channels at a time) and adds the window to memory in contiguous
//              rows, zeros skipped; corners beyond the window add to memory directly.  A warp's targets are the tile displaced by a
//              smooth flow, so the window sits at the tile displaced by the (floored) flow of the tile's centre pixel -- a window on the
//              undisplaced tile loses everything once the motion exceeds the halo (`displaced` = 0 keeps that form for measurement).
//              A float atomic sum: not bitwise reproducible.
//   grad_flow  a gather with one owner per element and one plain store, bitwise reproducible:
//              d/dix = sum_c grad_out[c] * (hy * (x01 - x00) + ly * (x11 - x10)), an invalid corner's value taken as 0 (d/diy likewise),
//              times the chain factor ((S - 1) / 2) * (2 / max(S - 1, 1)) formed in fp32 (1 for S > 1, 0 for S = 1), times 0 in border
//              mode where the unclamped coordinate is <= 0 or >= S - 1 (ATen's clip_coordinates_set_grad).  At an integer position the
//              floor's cell is used, as ATen does.
// All global indices are 64-bit.  Every thread of a workgroup reaches every barrier: pixels outside the frame only skip the sampling.
#include "crfp_common.h"

namespace crfp {

constexpr int WB_HALO = 8;                                         // the LDS window: the 4 x 64 pixel tile plus this many pixels on every side,
constexpr int WB_WH = 4 + 2 * WB_HALO, WB_WW = 64 + 2 * WB_HALO;   // 20 x 80 elements per channel,
constexpr int WB_CH = 4;                                           // for this many channels at a time (25.6 KB)

// one axis of the forward's coordinate arithmetic: the clamped sample coordinate, and the factor d(coordinate) / d(flow) of that axis
template <int BORDER>
__device__ __forceinline__ float warp_axis(int p, float f, int S, float& scale) {
    const float d = (float)(S - 1 > 1 ? S - 1 : 1);
    const float g = 2.0f * ((float)p + f) / d - 1.0f;
    float i = (g + 1.0f) * ((float)(S - 1) / 2.0f);
    scale = ((float)(S - 1) / 2.0f) * (2.0f / d);
    if (BORDER) {
        if (!(i > 0.0f && i < (float)(S - 1))) scale = 0.0f;   // also for NaN
        i = fminf(fmaxf(i, 0.0f), (float)(S - 1));
    }
    return fminf(fmaxf(i, -2.0f), (float)S + 1.0f);
}

// whole pixels by which the window follows the flow of the tile's centre; a flow beyond the frame (or not finite) displaces nothing
__device__ __forceinline__ int warp_window_shift(float f, int S) {
    if (!(fabsf(f) <= (float)S)) return 0;
    return (int)floorf(f);
}

// one corner's share of grad_x: into the workgroup's LDS window when it lies inside, straight to memory otherwise
__device__ __forceinline__ void warp_scatter(float (*win)[WB_WW], int ty0, int tx0, float* gplane, int y, int x, long long idx, float v) {
    const int wy = y - ty0, wx = x - tx0;
    // workgroup scope for the LDS add: it keeps the two adds two instructions (ds_add_f32 / global_atomic_add_f32), not one flat one
    if (wy >= 0 && wy < WB_WH && wx >= 0 && wx < WB_WW) __hip_atomic_fetch_add(&win[wy][wx], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else atomicAdd(gplane + idx, v);
}

// One thread per pixel, workgroup = 4 rows x 64 pixels (the forward's); x, go, gx are NCHW, so their rows are contiguous over lanes.
template <int BORDER>
__global__ void __launch_bounds__(256) flow_warp_bwd_kernel(const float* __restrict__ x, const float* __restrict__ flow,
                                                            const float* __restrict__ go, float* gx, float* __restrict__ gflow, int C, int H,
                                                            int W, int displaced) {
    __shared__ float win[WB_CH][WB_WH][WB_WW];
    const int tid = threadIdx.x;
    const int px = blockIdx.x * 64 + (tid & 63);
    const int py = blockIdx.y * 4 + (tid >> 6);
    const int n = blockIdx.z;
    const bool active = px < W && py < H;
    const long long HW = (long long)H * W, pix = (long long)py * W + px;   // pix: used by active threads only
    const float* fl = flow + (long long)n * HW * 2;
    int tx0 = blockIdx.x * 64 - WB_HALO, ty0 = blockIdx.y * 4 - WB_HALO;
    if (gx && displaced) {   // workgroup-uniform: the centre pixel of the tile (of its part inside the frame)
        const int cy = min((int)blockIdx.y * 4 + 2, H - 1), cx = min((int)blockIdx.x * 64 + 32, W - 1);
        const float* fc = fl + ((long long)cy * W + cx) * 2;   // dword accesses: the C-ABI asks for no 8-byte alignment of flow / grad_flow
        tx0 += warp_window_shift(fc[0], W);
        ty0 += warp_window_shift(fc[1], H);
    }
    bool v00 = false, v01 = false, v10 = false, v11 = false;
    long long i00 = 0, i01 = 0, i10 = 0, i11 = 0;
    int x0 = 0, y0 = 0;
    float hx = 0.0f, hy = 0.0f, lx = 0.0f, ly = 0.0f, scx = 0.0f, scy = 0.0f;
    if (active) {
        const float f_x = fl[pix * 2], f_y = fl[pix * 2 + 1];
        const float ix = warp_axis<BORDER>(px, f_x, W, scx), iy = warp_axis<BORDER>(py, f_y, H, scy);   // in [-2, size + 1]: the conversion is safe
        const float fx = floorf(ix), fy = floorf(iy);
        x0 = (int)fx; y0 = (int)fy;
        lx = ix - fx; ly = iy - fy; hx = 1.0f - lx; hy = 1.0f - ly;
        const bool vx0 = x0 >= 0 && x0 < W, vx1 = x0 + 1 >= 0 && x0 + 1 < W, vy0 = y0 >= 0 && y0 < H, vy1 = y0 + 1 >= 0 && y0 + 1 < H;
        v00 = vy0 && vx0; v01 = vy0 && vx1; v10 = vy1 && vx0; v11 = vy1 && vx1;
        if (v00) i00 = (long long)y0 * W + x0;
        if (v01) i01 = (long long)y0 * W + (x0 + 1);
        if (v10) i10 = (long long)(y0 + 1) * W + x0;
        if (v11) i11 = (long long)(y0 + 1) * W + (x0 + 1);
    }
    const float w00 = v00 ? hy * hx : 0.0f, w01 = v01 ? hy * lx : 0.0f, w10 = v10 ? ly * hx : 0.0f, w11 = v11 ? ly * lx : 0.0f;   // the forward's weights
    float* const winf = &win[0][0][0];
    float ax = 0.0f, ay = 0.0f;
    for (int c0 = 0; c0 < C; c0 += WB_CH) {
        const int nch = min(WB_CH, C - c0);
        if (gx) {
            for (int i = tid; i < nch * WB_WH * WB_WW; i += 256) winf[i] = 0.0f;
            __syncthreads();
        }
        if (active)
            for (int cc = 0; cc < nch; ++cc) {
                const long long plane = ((long long)n * C + c0 + cc) * HW;
                const float g = go[plane + pix];
                if (gx) {
                    if (v00) warp_scatter(win[cc], ty0, tx0, gx + plane, y0, x0, i00, g * w00);
                    if (v01) warp_scatter(win[cc], ty0, tx0, gx + plane, y0, x0 + 1, i01, g * w01);
                    if (v10) warp_scatter(win[cc], ty0, tx0, gx + plane, y0 + 1, x0, i10, g * w10);
                    if (v11) warp_scatter(win[cc], ty0, tx0, gx + plane, y0 + 1, x0 + 1, i11, g * w11);
                }
                if (gflow) {
                    const float x00 = v00 ? x[plane + i00] : 0.0f, x01 = v01 ? x[plane + i01] : 0.0f;
                    const float x10 = v10 ? x[plane + i10] : 0.0f, x11 = v11 ? x[plane + i11] : 0.0f;
                    ax = fmaf(g, hy * (x01 - x00) + ly * (x11 - x10), ax);
                    ay = fmaf(g, hx * (x10 - x00) + lx * (x11 - x01), ay);
                }
            }
        if (gx) {
            __syncthreads();   // the window holds the chunk's sums
            for (int i = tid; i < nch * WB_WH * WB_WW; i += 256) {
                const float v = winf[i];
                const int cc = i / (WB_WH * WB_WW), r = i - cc * (WB_WH * WB_WW), y = ty0 + r / WB_WW, xx = tx0 + r % WB_WW;
                if (v != 0.0f && y >= 0 && y < H && xx >= 0 && xx < W)
                    atomicAdd(gx + ((long long)n * C + c0 + cc) * HW + (long long)y * W + xx, v);
            }
            __syncthreads();   // read out before the next chunk clears it
        }
    }
    if (gflow && active) {
        float* const q = gflow + ((long long)n * HW + pix) * 2;
        q[0] = ax * scx;
        q[1] = ay * scy;
    }
}

bool flow_warp_backward_shape_ok(int n, int c, int h, int w) {
    if (!(n >= 1 && n <= 65535 && c >= 1 && h >= 1 && w >= 1 && h <= 4 * 65535 && w <= (1 << 30))) return false;
    // every tensor's element count (and byte count) stays far inside 64 bits
    return (long long)h * w <= (1LL << 58) / ((long long)n * (2LL + c));
}

int launch_flow_warp_backward(const float* x, const float* flow, const float* go, float* gx, float* gflow, int N, int C, int H, int W,
                              int border, int displaced, hipStream_t s) {
    const double px = (double)N * H * W;
    ProfScope prof("flow_warp_backward_nchw", s, px * (3.0 * C + 4.0) * 4.0, px * C * 16.0);
    if (gx && hipMemsetAsync(gx, 0, (size_t)N * C * H * W * sizeof(float), s) != hipSuccess) { set_error("flow_warp_backward: memset failed"); return 1; }
    dim3 grid((W + 63) / 64, (H + 3) / 4, N);
    if (border) flow_warp_bwd_kernel<1><<<grid, 256, 0, s>>>(x, flow, go, gx, gflow, C, H, W, displaced);
    else flow_warp_bwd_kernel<0><<<grid, 256, 0, s>>>(x, flow, go, gx, gflow, C, H, W, displaced);
    CRFP_CHECK_LAUNCH();
    return 0;
}

}  // namespace crfp
