// DCNv2 backward (stride 1, k = 3, pad = 1, dil = 1; NCHW fp32 API tensors): the five gradients of crfp_dcnv2_forward_f32 for the autograd
// form of the dcn_v2 drop-in (crfp_amd/ops.py).  fp32 on the VALU throughout; not a tuned path.
//
// Forward semantics (oracle/crfp_oracle.py::dcnv2): offsets are (dy, dx) interleaved per (group, tap); the sample of tap k at
// pixel (y, x) sits at py = (float)(y - 1 + ky) + dy, px = (float)(x - 1 + kx) + dx and counts only when -1 < py < H and -1 < px < W; each of its
// four corners is zero-padded on its own; the bilinear value is multiplied by the mask.  bwd_sample() is the one place that turns a position
// into corners: it decides validity BEFORE an index is formed (a NaN or infinite position fails the comparisons and counts as outside) and
// returns plane indices as 64-bit values, so an unbounded offset (FNet emits +-2048 px at 8x) can never produce an address.
//
// With gcol[c,k] = sum_o weight[o,c,k] * grad_out[o] and val[c,k] the unmodulated bilinear sample:
//   dcn_bwd_pixel_kernel   one thread per pixel: grad_offset, grad_mask (plain stores: every element has one owner) and grad_x (one
//                          float atomic add per valid corner: a data-dependent scatter, summed per workgroup in an LDS window of the tile
//                          and its surroundings and added to memory from there; corners beyond the window add to memory directly).  The derivative of val is taken in the cell the
//                          forward's floor picked (d/dpy = hx (x10 - x00) + lx (x11 - x01) over the VALID corners), i.e. the right-hand
//                          derivative at integer positions; dropped corners and samples contribute exactly 0.
//   dcn_bwd_weight_kernel  grad_weight / grad_bias reduce over all pixels: workgroup (j, c) walks the 256-pixel tiles j, j + J, ... in order,
//                          stages col[c,k] = mask * val and grad_out in LDS and keeps its sums over pixels in registers; its partial slab
//                          goes to the workspace.
//   dcn_bwd_slab_sum_kernel  adds the J slabs of each element in slab order.
// Determinism: grad_offset, grad_mask, grad_weight and grad_bias are bitwise reproducible from run to run (fixed summation orders, no
// atomics; J depends on the shape alone).  grad_x is NOT: a float atomic sum depends on the order in which the adds arrive.
// All global indices are 64-bit; weight reads are wave-uniform.
// The same kernels in their compile-time SHARED form are the backward of crfp_dcnv2_shared_f32 (4 -> 4, one (dy, dx) and one mask per
// pixel for the 9 taps): grad_offset [n,2,h,w] and grad_mask [n,1,h,w] are the sums over the taps, formed in registers.
#include "crfp_common.h"

namespace crfp {

constexpr int DB_MAXC = 64;          // cin, cout <= 64
constexpr int DB_TILE = 256;         // pixels per tile of the weight pass = threads per workgroup
constexpr int DB_OT = 32;            // output channels staged in LDS at a time
constexpr int DB_GS = DB_TILE + 1;   // row pitch of the staged grad_out (odd: the 32 channels of a read fall in 32 banks)
constexpr int DB_HALO = 8;           // the pixel kernel's LDS window: its 4 x 64 pixel tile plus this many pixels on every side,
constexpr int DB_WH = 4 + 2 * DB_HALO, DB_WW = 64 + 2 * DB_HALO;   // 20 x 80 elements per channel,
constexpr int DB_CH = 4;             // for up to this many channels of a deformable group at a time (25.6 KB)

struct BwdSample {
    bool v00, v01, v10, v11;            // corner counts (inside the plane, sample inside (-1, size))
    long long i00, i01, i10, i11;       // plane index of a corner; formed only where the corner counts, 0 otherwise
    int y0, x0;                         // the cell's top-left corner, in [-1, size - 1] (0 for a dropped sample: no corner counts then)
    float hy, hx, ly, lx;
};

__device__ __forceinline__ BwdSample bwd_sample(float py, float px, int H, int W) {
    BwdSample s;
    s.v00 = s.v01 = s.v10 = s.v11 = false;
    s.i00 = s.i01 = s.i10 = s.i11 = 0;
    s.y0 = s.x0 = 0;
    s.hy = s.hx = s.ly = s.lx = 0.0f;
    // false for NaN; +-inf fails one side.  Inside the test the position is finite and within (-1, size): floor and int conversion are safe
    if (!(py > -1.0f && px > -1.0f && py < (float)H && px < (float)W)) return s;
    const float fy = floorf(py), fx = floorf(px);
    const int y0 = (int)fy, x0 = (int)fx;   // in [-1, size - 1]
    s.y0 = y0; s.x0 = x0;
    s.ly = py - fy; s.lx = px - fx; s.hy = 1.0f - s.ly; s.hx = 1.0f - s.lx;
    const bool vy0 = y0 >= 0 && y0 <= H - 1, vy1 = y0 + 1 >= 0 && y0 + 1 <= H - 1;
    const bool vx0 = x0 >= 0 && x0 <= W - 1, vx1 = x0 + 1 >= 0 && x0 + 1 <= W - 1;
    s.v00 = vy0 && vx0; s.v01 = vy0 && vx1; s.v10 = vy1 && vx0; s.v11 = vy1 && vx1;
    if (s.v00) s.i00 = (long long)y0 * W + x0;
    if (s.v01) s.i01 = (long long)y0 * W + (x0 + 1);
    if (s.v10) s.i10 = (long long)(y0 + 1) * W + x0;
    if (s.v11) s.i11 = (long long)(y0 + 1) * W + (x0 + 1);
    return s;
}

// weight [cout, cin, 3, 3] -> wt [cin * 9][CO], zero for o >= cout: the o-sum of gcol reads one contiguous, wave-uniform row
__global__ void dcn_bwd_wt_kernel(const float* __restrict__ w, float* __restrict__ wt, int cin, int cout, int CO) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cin * 9 * CO) return;
    const int o = i % CO, ck = i / CO;
    wt[i] = o < cout ? w[(long long)o * cin * 9 + ck] : 0.0f;
}

// one corner's share of grad_x: into the workgroup's LDS window when it lies inside, straight to memory otherwise (large motion)
__device__ __forceinline__ void bwd_scatter(float (*win)[DB_WW], int ty0, int tx0, float* gplane, int y, int x, long long idx, float v) {
    const int wy = y - ty0, wx = x - tx0;
    // workgroup scope for the LDS add: right for LDS, and it keeps the two adds two instructions (ds_add_f32 / global_atomic_add_f32), not one flat one
    if (wy >= 0 && wy < DB_WH && wx >= 0 && wx < DB_WW) __hip_atomic_fetch_add(&win[wy][wx], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else atomicAdd(gplane + idx, v);
}

// One thread per pixel, workgroup = 4 rows x 64 pixels; the channels of a deformable group go through in chunks of DB_CH.  grad_x of a
// chunk is summed in the LDS window first (LDS float atomics) and the window is then added to memory row by row -- 6.25 global atomics per
// thread and channel in contiguous rows instead of 36 scattered ones; corners outside the window (offsets beyond ~6 px) go to memory
// directly.  Every thread of the workgroup reaches every barrier: pixels outside the frame only skip the sampling.
// SHARED: the compact form of crfp_dcnv2_shared_f32 -- one group, offset [n,2,h,w] and mask [n,1,h,w] read by all 9 taps; the owning
// thread adds the taps' d/dy, d/dx and d/dmask in tap order in registers and stores once (the tiled tensors never exist).
template <int CO, bool SHARED>
__global__ void __launch_bounds__(256) dcn_bwd_pixel_kernel(const float* __restrict__ x, const float* __restrict__ offset,
                                                            const float* __restrict__ mask, const float* __restrict__ wt,
                                                            const float* __restrict__ go, float* gx, float* __restrict__ goff,
                                                            float* __restrict__ gmask, int cin, int cout, int H, int W, int dg) {
    __shared__ float win[DB_CH][DB_WH][DB_WW];
    const int tid = threadIdx.x;
    const int px = blockIdx.x * 64 + (tid & 63);
    const int py = blockIdx.y * 4 + (tid >> 6);
    const int tx0 = blockIdx.x * 64 - DB_HALO, ty0 = blockIdx.y * 4 - DB_HALO;
    const int n = blockIdx.z;
    const bool active = px < W && py < H;
    const long long HW = (long long)H * W, pix = (long long)py * W + px;   // used by active threads only
    const int cpg = cin / dg;
    float* const winf = &win[0][0][0];
    float g[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) g[o] = (active && o < cout) ? go[((long long)n * cout + o) * HW + pix] : 0.0f;
    for (int gi = 0; gi < dg; ++gi)
        for (int c0 = 0; c0 < cpg; c0 += DB_CH) {
            const int nch = min(DB_CH, cpg - c0);
            if (gx) {
                for (int i = tid; i < nch * DB_WH * DB_WW; i += 256) winf[i] = 0.0f;
                __syncthreads();
            }
            if (active) {
                float s_y = 0.0f, s_x = 0.0f, s_m = 0.0f;   // SHARED: the sums over the taps
                for (int tap = 0; tap < 9; ++tap) {
                    const long long och = SHARED ? (long long)n * 2 : (long long)n * 2 * dg * 9 + 2 * (gi * 9 + tap);
                    const long long mch = SHARED ? (long long)n : (long long)n * dg * 9 + gi * 9 + tap;
                    const float dy = offset[och * HW + pix], dx = offset[(och + 1) * HW + pix], m = mask[mch * HW + pix];
                    const BwdSample s = bwd_sample((float)(py - 1 + tap / 3) + dy, (float)(px - 1 + tap % 3) + dx, H, W);
                    const float w00 = s.hy * s.hx, w01 = s.hy * s.lx, w10 = s.ly * s.hx, w11 = s.ly * s.lx;
                    float a_m = 0.0f, a_y = 0.0f, a_x = 0.0f;
                    for (int cc = 0; cc < nch; ++cc) {
                        const int ci = gi * cpg + c0 + cc;
                        const float* wr = wt + (long long)(ci * 9 + tap) * CO;
                        float gc = 0.0f;
#pragma unroll
                        for (int o = 0; o < CO; ++o) gc = fmaf(wr[o], g[o], gc);
                        const long long plane = ((long long)n * cin + ci) * HW;
                        const float x00 = s.v00 ? x[plane + s.i00] : 0.0f, x01 = s.v01 ? x[plane + s.i01] : 0.0f;
                        const float x10 = s.v10 ? x[plane + s.i10] : 0.0f, x11 = s.v11 ? x[plane + s.i11] : 0.0f;
                        const float val = w00 * x00 + w01 * x01 + w10 * x10 + w11 * x11;
                        const float dvy = s.hx * (x10 - x00) + s.lx * (x11 - x01);
                        const float dvx = s.hy * (x01 - x00) + s.ly * (x11 - x10);
                        a_m = fmaf(gc, val, a_m);
                        a_y = fmaf(gc, dvy, a_y);
                        a_x = fmaf(gc, dvx, a_x);
                        if (gx) {
                            const float gm = gc * m;
                            if (s.v00) bwd_scatter(win[cc], ty0, tx0, gx + plane, s.y0, s.x0, s.i00, gm * w00);
                            if (s.v01) bwd_scatter(win[cc], ty0, tx0, gx + plane, s.y0, s.x0 + 1, s.i01, gm * w01);
                            if (s.v10) bwd_scatter(win[cc], ty0, tx0, gx + plane, s.y0 + 1, s.x0, s.i10, gm * w10);
                            if (s.v11) bwd_scatter(win[cc], ty0, tx0, gx + plane, s.y0 + 1, s.x0 + 1, s.i11, gm * w11);
                        }
                    }
                    // a group of more than DB_CH channels: the owning thread adds its later chunks to what it stored (a fixed order)
                    if (SHARED) {
                        s_y += a_y * m; s_x += a_x * m; s_m += a_m;
                        if (tap < 8) continue;
                    }
                    if (goff) {
                        float* const qy = goff + och * HW + pix;
                        float* const qx = goff + (och + 1) * HW + pix;
                        const float vy = SHARED ? s_y : a_y * m, vx = SHARED ? s_x : a_x * m;
                        *qy = c0 ? *qy + vy : vy;
                        *qx = c0 ? *qx + vx : vx;
                    }
                    if (gmask) {
                        float* const qm = gmask + mch * HW + pix;
                        const float vm = SHARED ? s_m : a_m;
                        *qm = c0 ? *qm + vm : vm;
                    }
                }
            }
            if (gx) {
                __syncthreads();   // the window holds the chunk's sums
                for (int i = tid; i < nch * DB_WH * DB_WW; i += 256) {
                    const float v = winf[i];
                    const int cc = i / (DB_WH * DB_WW), r = i - cc * (DB_WH * DB_WW), y = ty0 + r / DB_WW, xx = tx0 + r % DB_WW;
                    if (v != 0.0f && y >= 0 && y < H && xx >= 0 && xx < W)
                        atomicAdd(gx + ((long long)n * cin + gi * cpg + c0 + cc) * HW + (long long)y * W + xx, v);
                }
                __syncthreads();   // read out before the next chunk clears it
            }
        }
}

// Workgroup (j = blockIdx.x of J, c = blockIdx.y).  Per tile: thread t samples channel c at pixel tile * 256 + t for the 9 taps into
// col[k][t] (row 9: 1 for a real pixel -- the "tap" whose sum over pixels is grad_bias); then, 32 output channels at a time, thread t
// owns the sums q = t, t + 256 of the 32 x 10 (o, k) pairs, o = q % 32, k = q / 32, and adds the tile's 256 products in a fixed order (four interleaved chains).
template <bool SHARED>
__global__ void __launch_bounds__(DB_TILE) dcn_bwd_weight_kernel(const float* __restrict__ x, const float* __restrict__ offset,
                                                                 const float* __restrict__ mask, const float* __restrict__ go,
                                                                 float* __restrict__ wslab, float* __restrict__ bslab, int N, int cin,
                                                                 int cout, int H, int W, int dg, long long tiles) {
    __shared__ float col[10][DB_TILE];
    __shared__ float gs[DB_OT][DB_GS];
    const int t = threadIdx.x, c = blockIdx.y, J = gridDim.x, j = blockIdx.x;
    const long long HW = (long long)H * W, total = (long long)N * HW;
    const int gi = c / (cin / dg);
    const int n_ot = (cout + DB_OT - 1) / DB_OT;   // 1 or 2
    float acc[2][2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};   // [o tile][q slot]
    for (long long tile = j; tile < tiles; tile += J) {
        const long long p = tile * DB_TILE + t;
        const bool real = p < total;
        const long long n = real ? p / HW : 0, pix = real ? p - n * HW : 0;
        const int py = (int)(pix / W), px = (int)(pix - (long long)py * W);
        for (int tap = 0; tap < 9; ++tap) {
            float v = 0.0f;
            if (real) {
                const long long och = SHARED ? n * 2 : n * 2 * dg * 9 + 2 * (gi * 9 + tap), mch = SHARED ? n : n * dg * 9 + gi * 9 + tap;
                const float dy = offset[och * HW + pix], dx = offset[(och + 1) * HW + pix], m = mask[mch * HW + pix];
                const BwdSample s = bwd_sample((float)(py - 1 + tap / 3) + dy, (float)(px - 1 + tap % 3) + dx, H, W);
                const long long plane = (n * cin + c) * HW;
                const float x00 = s.v00 ? x[plane + s.i00] : 0.0f, x01 = s.v01 ? x[plane + s.i01] : 0.0f;
                const float x10 = s.v10 ? x[plane + s.i10] : 0.0f, x11 = s.v11 ? x[plane + s.i11] : 0.0f;
                v = (s.hy * s.hx * x00 + s.hy * s.lx * x01 + s.ly * s.hx * x10 + s.ly * s.lx * x11) * m;
            }
            col[tap][t] = v;
        }
        col[9][t] = real ? 1.0f : 0.0f;
#pragma unroll
        for (int ot = 0; ot < 2; ++ot) {
            if (ot < n_ot) {
                __syncthreads();   // col complete (ot = 0); the previous channel tile's readers are done with gs
                for (int oo = 0; oo < DB_OT; ++oo) {
                    const int o = ot * DB_OT + oo;
                    gs[oo][t] = (real && o < cout) ? go[(n * cout + o) * HW + pix] : 0.0f;
                }
                __syncthreads();
#pragma unroll
                for (int sl = 0; sl < 2; ++sl) {
                    const int q = t + sl * DB_TILE;
                    if (q < DB_OT * 10) {
                        const int oo = q % DB_OT, k = q / DB_OT;
                        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;   // four short chains per tile: less rounding than one long sum
                        for (int i = 0; i < DB_TILE; i += 4) {
                            a0 = fmaf(gs[oo][i], col[k][i], a0);
                            a1 = fmaf(gs[oo][i + 1], col[k][i + 1], a1);
                            a2 = fmaf(gs[oo][i + 2], col[k][i + 2], a2);
                            a3 = fmaf(gs[oo][i + 3], col[k][i + 3], a3);
                        }
                        acc[ot][sl] += (a0 + a1) + (a2 + a3);
                    }
                }
            }
        }
        __syncthreads();   // this tile's readers are done with col and gs
    }
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            const int q = t + sl * DB_TILE;
            if (ot < n_ot && q < DB_OT * 10) {
                const int o = ot * DB_OT + q % DB_OT, k = q / DB_OT;
                if (o < cout) {
                    if (k < 9) wslab[(((long long)j * cout + o) * cin + c) * 9 + k] = acc[ot][sl];
                    else if (c == 0) bslab[(long long)j * cout + o] = acc[ot][sl];
                }
            }
        }
}

// element e of grad_weight (e < nw) or grad_bias (nw <= e < nw + nb): its J slab values added in slab order
__global__ void dcn_bwd_slab_sum_kernel(const float* __restrict__ wslab, const float* __restrict__ bslab, float* __restrict__ gw,
                                        float* __restrict__ gb, int nw, int nb, int J) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nw + nb) return;
    const bool isw = e < nw;
    if (isw ? gw == nullptr : gb == nullptr) return;
    const float* src = isw ? wslab + e : bslab + (e - nw);
    const long long pitch = isw ? nw : nb;
    float a = 0.0f;
    for (int j = 0; j < J; ++j) a += src[j * pitch];
    if (isw) gw[e] = a; else gb[e - nw] = a;
}

static int bwd_co(int cout) { return cout <= 8 ? 8 : cout <= 32 ? 32 : DB_MAXC; }

// slabs of the weight pass: enough workgroups (J * cin) to fill the chip, never more than there are tiles; a function of the shape alone
static int bwd_slabs(int n, int cin, int h, int w) {
    const long long tiles = ((long long)n * h * w + DB_TILE - 1) / DB_TILE;
    const long long want = (2048 + cin - 1) / cin;
    return (int)(tiles < want ? tiles : want);
}

static size_t bwd_wt_bytes(int cin, int cout) { return align_up((size_t)cin * 9 * bwd_co(cout) * sizeof(float), 256); }
static size_t bwd_wslab_bytes(int n, int cin, int cout, int h, int w) {
    return align_up((size_t)bwd_slabs(n, cin, h, w) * cout * cin * 9 * sizeof(float), 256);
}

bool dcn_backward_shape_ok(int n, int cin, int cout, int h, int w, int dg) {
    if (!(n >= 1 && n <= 65535 && cin >= 1 && cout >= 1 && cin <= DB_MAXC && cout <= DB_MAXC && h >= 1 && w >= 1 && h <= 4 * 65535 && dg >= 1 &&
          cin % dg == 0))
        return false;
    // every tensor's element count (and byte count) stays far inside 64 bits
    return (long long)h * w <= (1LL << 58) / ((long long)n * (18 * dg + cin + cout));
}

size_t dcn_backward_workspace_bytes(int n, int cin, int cout, int h, int w, int dg) {
    if (!dcn_backward_shape_ok(n, cin, cout, h, w, dg)) return 0;
    return bwd_wt_bytes(cin, cout) + bwd_wslab_bytes(n, cin, cout, h, w) + align_up((size_t)bwd_slabs(n, cin, h, w) * cout * sizeof(float), 256);
}

int launch_dcn_backward(const float* x, const float* offset, const float* mask, const float* weight, const float* go, float* gx, float* goff,
                        float* gmask, float* gw, float* gb, int N, int cin, int cout, int H, int W, int dg, int shared, void* workspace, hipStream_t s) {
    const double px = (double)N * H * W;
    ProfScope prof(shared ? "dcnv2_shared_backward_nchw" : "dcnv2_backward_nchw", s, px * (2.0 * cin + (shared ? 6.0 : 54.0 * dg) + cout) * 4.0,
                   6.0 * px * cin * cout * 9);
    char* p = (char*)workspace;
    float* wt = (float*)p; p += bwd_wt_bytes(cin, cout);
    float* wslab = (float*)p; p += bwd_wslab_bytes(N, cin, cout, H, W);
    float* bslab = (float*)p;
    if (gx || goff || gmask) {
        const int CO = bwd_co(cout), nwt = cin * 9 * CO;
        if (gx && hipMemsetAsync(gx, 0, (size_t)N * cin * H * W * sizeof(float), s) != hipSuccess) { set_error("dcnv2_backward: memset failed"); return 1; }
        dcn_bwd_wt_kernel<<<(nwt + 255) / 256, 256, 0, s>>>(weight, wt, cin, cout, CO);
        CRFP_CHECK_LAUNCH();
        dim3 grid((W + 63) / 64, (H + 3) / 4, N);
        if (shared) dcn_bwd_pixel_kernel<8, true><<<grid, 256, 0, s>>>(x, offset, mask, wt, go, gx, goff, gmask, cin, cout, H, W, dg);   // 4 -> 4: CO = 8
        else if (CO == 8) dcn_bwd_pixel_kernel<8, false><<<grid, 256, 0, s>>>(x, offset, mask, wt, go, gx, goff, gmask, cin, cout, H, W, dg);
        else if (CO == 32) dcn_bwd_pixel_kernel<32, false><<<grid, 256, 0, s>>>(x, offset, mask, wt, go, gx, goff, gmask, cin, cout, H, W, dg);
        else dcn_bwd_pixel_kernel<DB_MAXC, false><<<grid, 256, 0, s>>>(x, offset, mask, wt, go, gx, goff, gmask, cin, cout, H, W, dg);
        CRFP_CHECK_LAUNCH();
    }
    if (gw || gb) {
        const int J = bwd_slabs(N, cin, H, W), nw = cout * cin * 9;
        const long long tiles = ((long long)N * H * W + DB_TILE - 1) / DB_TILE;
        if (shared) dcn_bwd_weight_kernel<true><<<dim3(J, cin), DB_TILE, 0, s>>>(x, offset, mask, go, wslab, bslab, N, cin, cout, H, W, dg, tiles);
        else dcn_bwd_weight_kernel<false><<<dim3(J, cin), DB_TILE, 0, s>>>(x, offset, mask, go, wslab, bslab, N, cin, cout, H, W, dg, tiles);
        CRFP_CHECK_LAUNCH();
        dcn_bwd_slab_sum_kernel<<<(nw + cout + 255) / 256, 256, 0, s>>>(wslab, bslab, gw, gb, nw, cout, J);
        CRFP_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace crfp
