// conv3x3 backward (stride 1, pad 1; NCHW fp32 API tensors): the four gradients of crfp_conv3x3_ex_f32 for the autograd form of
// ops.conv3x3 / ops.conv3x3_ex (crfp_amd/ops.py).  fp32 throughout, one rounding per product: the matrix-shaped parts run on the exact
// f32-input MFMA (v_mfma_f32_16x16x4_f32: bit for bit a k-ordered fmaf chain), the elementwise parts on the VALU.  No split-fp16: a gradient
// has no bounded range (a mean-reduced loss at 1440 x 2560 hands over values near 1e-7), so the forward's operand-range check has nothing to
// hold on to.  Not a tuned path.
//
// Forward: out = act(conv3x3(cat(x, x2)) + bias) * post_scale (+ residual), x read through pixel_unshuffle(4) when unshuffle_r = 4, out
// stored through pixel_shuffle(r) when shuffle_r > 1.  The residual's gradient is grad_out itself and needs no kernel.
//
//   conv_bwd_gz_kernel      gz[n,co,y,x] = grad_out * post_scale * act'(.), grad_out and out read through the inverse of the store's
//                           pixel-shuffle; the activation's derivative is taken from the saved `out` (relu / lrelu: its sign; tanh:
//                           1 - (out/s)^2; sigmoid: (out/s)(1 - out/s)).  Written once into the workspace as plain [n,cout,h,w].
//   conv_bwd_bias_kernel    grad_bias: workgroup (j, co) adds the pixels j*256 + t, (j + JB)*256 + t, ... of channel co per thread, then the
//                           256 thread sums in a fixed tree; one value per (j, co) goes to the workspace.
//   conv_bwd_wt_kernel      weight [cout, cin_t, 3, 3] -> wt [tap][co (padded to 4)][ci (padded)], zeros in the padding.
//   conv_bwd_input_kernel   g[ci, pixel] = sum over (tap, co) of wt[tap][co][ci] * gz[co, y - ky + 1, x - kx + 1]: an implicit GEMM,
//                           a wave owns 16 pixels of a row x up to 64 input channels (4 MFMA tiles, each with two accumulators: the
//                           even and the odd taps, added at the end).  Operands come straight from memory (gz zero outside the frame);
//                           every output element has one owner and one plain store.  Channels [0, cin) go to grad_x (through the
//                           pixel_shuffle(4) scatter when unshuffle_r = 4), [cin, cin + cin2) to grad_x2; a NULL output's channels are
//                           not computed.
//   conv_bwd_weight_kernel  gw[co, ci, tap] = sum over pixels of gz[co, y, x] * in[ci, y + ky - 1, x + kx - 1]: workgroup (j, 16 input
//                           channels, 32 output channels) walks the 64-pixel row tiles j, j + J, ... in order; per tile it stages gz
//                           [32][64] and the input rows y - 1 .. y + 1 [16][3][66] (zero-padded, x read through the unshuffle) in LDS,
//                           and each of its 4 waves sums 16 of the 64 pixels on the MFMA (2 x 9 accumulators: output-channel tile x
//                           tap).  The waves' sums are added in wave order and the slab goes to the workspace.
//   conv_bwd_slab_sum_kernel  adds the J weight slabs / JB bias slabs of each element in slab order.
// Determinism: all four gradients are bitwise reproducible from run to run and do not depend on which other outputs are asked for (fixed
// summation orders, no atomics; J and JB depend on the shape alone).
// All global indices are 64-bit; every kernel walks its work items in a grid-stride loop, so no grid dimension depends on the frame size
// beyond its cap.  Every thread of a workgroup reaches every barrier.
#include "crfp_common.h"

namespace crfp {

constexpr int CB_MAXC = 1024;                 // cin + cin2, cout <= 1024
constexpr int CB_NT = 4;                      // input-channel MFMA tiles per wave of the input kernel
constexpr int CW_CO = 32, CW_CI = 16;         // the weight kernel's output / input channels per workgroup
constexpr int CW_GS = 68;                     // row pitch of the staged gz (64 pixels + 4)
constexpr int CW_RS = 68, CW_CS = 3 * CW_RS + 1;   // staged input: row pitch (66 pixels + 2), channel pitch (odd)
constexpr int CW_LDS = CW_CO * CW_GS + CW_CI * CW_CS;   // 5456 floats (21.3 KB) >= the 18 * 256 floats of the wave reduction
static_assert(CW_LDS >= 18 * 256, "the wave reduction reuses the staging buffer");

// element (n, ci, yy, xx) of cat(x, x2), x read through pixel_unshuffle(4) when unshuf; the caller checks the frame
__device__ __forceinline__ float cb_in(const float* __restrict__ x, const float* __restrict__ x2, long long n, int ci, int yy, int xx, int cin,
                                       int cin2, int H, int W, int unshuf) {
    if (ci < cin) {
        if (unshuf) {
            const int c = ci >> 4, i = (ci & 15) >> 2, j = ci & 3;
            return x[((n * (cin >> 4) + c) * (4LL * H) + (4LL * yy + i)) * (4LL * W) + (4LL * xx + j)];
        }
        return x[((n * cin + ci) * H + yy) * W + xx];
    }
    return x2[((n * cin2 + (ci - cin)) * H + yy) * W + xx];
}

__global__ void __launch_bounds__(256) conv_bwd_gz_kernel(const float* __restrict__ go, const float* __restrict__ out, float* __restrict__ gz,
                                                          int cout, int H, int W, int r, int act, float s, long long total) {
    const long long HW = (long long)H * W;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long src = i;
        if (r > 1) {   // gz (n, co, y, x) <- (n, co / r^2, y r + (co % r^2) / r, x r + co % r) of the shuffled tensor
            const long long plane = i / HW, pix = i - plane * HW, n = plane / cout;
            const int co = (int)(plane - n * cout), y = (int)(pix / W), x = (int)(pix - (long long)y * W);
            const int c = co / (r * r), ij = co - c * (r * r), ii = ij / r, jj = ij - ii * r;
            src = ((n * (cout / (r * r)) + c) * ((long long)H * r) + ((long long)y * r + ii)) * ((long long)W * r) + ((long long)x * r + jj);
        }
        float d = s;
        if (act == CRFP_ACT_RELU) d = out[src] > 0.0f ? s : 0.0f;
        else if (act == CRFP_ACT_LRELU01) d = out[src] > 0.0f ? s : 0.1f * s;
        else if (act == CRFP_ACT_TANH) { const float t = out[src] / s; d = s * (1.0f - t * t); }
        else if (act == CRFP_ACT_SIGMOID) { const float t = out[src] / s; d = s * (t * (1.0f - t)); }
        gz[i] = go[src] * d;
    }
}

__global__ void __launch_bounds__(256) conv_bwd_bias_kernel(const float* __restrict__ gz, float* __restrict__ bslab, int cout, long long HW,
                                                            long long total) {
    __shared__ float red[256];
    const int t = threadIdx.x, co = blockIdx.y, j = blockIdx.x, J = gridDim.x;
    float a = 0.0f;
    for (long long p = (long long)j * 256 + t; p < total; p += (long long)J * 256) {
        const long long n = p / HW, pix = p - n * HW;
        a += gz[(n * cout + co) * HW + pix];
    }
    red[t] = a;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    if (t == 0) bslab[(long long)j * cout + co] = red[0];
}

// weight [cout, cin_t, 3, 3] -> wt [9][coP][ciP], zero for co >= cout or ci >= cin_t
__global__ void conv_bwd_wt_kernel(const float* __restrict__ w, float* __restrict__ wt, int cin_t, int cout, int coP, int ciP) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 9 * coP * ciP) return;
    const int ci = i % ciP, co = (i / ciP) % coP, tap = i / (ciP * coP);
    wt[i] = (co < cout && ci < cin_t) ? w[((long long)co * cin_t + ci) * 9 + tap] : 0.0f;
}

// Work item = (row of an image, 64-pixel segment of it, group of 64 input channels from c_lo on); wave w of the workgroup owns the
// segment's pixels [16 w, 16 w + 16).  D[ci][pixel] = A[ci][co] B[co][pixel]: lane l holds A at (ci = l & 15, co = l >> 4), B at
// (co = l >> 4, pixel = l & 15) and D at (pixel = l & 15, ci = 4 (l >> 4) + reg).  No barrier in this kernel.
__global__ void __launch_bounds__(256) conv_bwd_input_kernel(const float* __restrict__ gz, const float* __restrict__ wt, float* __restrict__ gx,
                                                             float* __restrict__ gx2, int cin, int cin2, int cout, int coP, int ciP, int H, int W,
                                                             int unshuf, int c_lo, int c_hi, int ncg, long long items) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lk = lane >> 4, lc = lane & 15;
    const int xt = (W + 63) / 64;
    const long long HW = (long long)H * W;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int cg = (int)(it % ncg);
        const long long rest = it / ncg, row = rest / xt, n = row / H;
        const int xb = (int)(rest - row * xt), y = (int)(row - n * H);
        const int x0 = xb * 64 + wave * 16;
        if (x0 >= W) continue;   // wave-uniform
        const int cbase = c_lo + cg * 16 * CB_NT;
        const int nt = min(CB_NT, (c_hi - cbase + 15) / 16);
        cf32x4 acc[CB_NT][2];
#pragma unroll
        for (int t = 0; t < CB_NT; ++t) acc[t][0] = acc[t][1] = cf32x4{0.0f, 0.0f, 0.0f, 0.0f};
        const float* const gzn = gz + n * cout * HW;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int yy = y - tap / 3 + 1, xx = x0 + lc - tap % 3 + 1;
            const bool inb = yy >= 0 && yy < H && xx >= 0 && xx < W;
            const long long gpix = inb ? (long long)yy * W + xx : 0;
            const float* const wr = wt + ((long long)tap * coP + lk) * ciP + cbase + lc;
            for (int cb = 0; cb < coP; cb += 4) {
                const int co = cb + lk;
                const float b = (inb && co < cout) ? gzn[co * HW + gpix] : 0.0f;
#pragma unroll
                for (int t = 0; t < CB_NT; ++t)
                    if (t < nt) acc[t][tap & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[(long long)cb * ciP + 16 * t], b, acc[t][tap & 1], 0, 0, 0);
            }
        }
        const int xp = x0 + lc;
        if (xp < W) {
#pragma unroll
            for (int t = 0; t < CB_NT; ++t)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int ci = cbase + 16 * t + 4 * lk + reg;
                    if (t < nt && ci < c_hi) {
                        const float v = acc[t][0][reg] + acc[t][1][reg];
                        if (ci >= cin) gx2[((n * cin2 + (ci - cin)) * H + y) * W + xp] = v;
                        else if (unshuf)
                            gx[((n * (cin >> 4) + (ci >> 4)) * (4LL * H) + (4LL * y + ((ci & 15) >> 2))) * (4LL * W) + (4LL * xp + (ci & 3))] = v;
                        else gx[((n * cin + ci) * H + y) * W + xp] = v;
                    }
                }
        }
    }
}

// Workgroup (j = blockIdx.x of J, input channels [16 blockIdx.y, +16), output channels [32 blockIdx.z, +32)).  D[co][ci] = A[co][pixel]
// B[pixel][ci] per tap: lane l holds A at (co = l & 15, pixel = l >> 4), B at (pixel = l >> 4, ci = l & 15) and D at (ci = l & 15,
// co = 4 (l >> 4) + reg).  Wave w takes the tile's pixels [16 w, 16 w + 16) in four steps of 4.
__global__ void __launch_bounds__(256) conv_bwd_weight_kernel(const float* __restrict__ gz, const float* __restrict__ x, const float* __restrict__ x2,
                                                              float* __restrict__ wslab, int cin, int cin2, int cout, int H, int W, int unshuf,
                                                              long long tiles) {
    __shared__ float lds[CW_LDS];
    float* const gzs = lds;
    float* const ins = lds + CW_CO * CW_GS;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lk = lane >> 4, lc = lane & 15;
    const int j = blockIdx.x, J = gridDim.x, ci0 = blockIdx.y * CW_CI, co0 = blockIdx.z * CW_CO;
    const int cin_t = cin + cin2, xt = (W + 63) / 64;
    const bool mt2 = cout - co0 > 16;   // workgroup-uniform: a second tile of 16 output channels
    cf32x4 acc[2][9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) acc[0][tap] = acc[1][tap] = cf32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (long long tile = j; tile < tiles; tile += J) {
        const long long row = tile / xt, n = row / H;
        const int x0 = (int)(tile - row * xt) * 64, y = (int)(row - n * H);
        __syncthreads();   // the previous tile's readers are done
        for (int i = t; i < CW_CO * 64; i += 256) {
            const int c = i >> 6, p = i & 63, co = co0 + c, xx = x0 + p;
            gzs[c * CW_GS + p] = (co < cout && xx < W) ? gz[((n * cout + co) * H + y) * W + xx] : 0.0f;
        }
        for (int i = t; i < CW_CI * 3 * 66; i += 256) {
            const int c = i / 198, r = i - c * 198, ry = r / 66, p = r - ry * 66;
            const int ci = ci0 + c, yy = y + ry - 1, xx = x0 + p - 1;
            ins[c * CW_CS + ry * CW_RS + p] = (ci < cin_t && yy >= 0 && yy < H && xx >= 0 && xx < W) ? cb_in(x, x2, n, ci, yy, xx, cin, cin2, H, W, unshuf) : 0.0f;
        }
        __syncthreads();
        if (x0 + wave * 16 < W) {   // wave-uniform: pixels beyond the row add nothing
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int px = wave * 16 + s * 4 + lk;
                const float a0 = gzs[lc * CW_GS + px], a1 = gzs[(16 + lc) * CW_GS + px];
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const float b = ins[lc * CW_CS + (tap / 3) * CW_RS + px + tap % 3];
                    acc[0][tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b, acc[0][tap], 0, 0, 0);
                    if (mt2) acc[1][tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b, acc[1][tap], 0, 0, 0);
                }
            }
        }
    }
    // the four waves' sums, added in wave order by wave 0
    for (int w = 1; w < 4; ++w) {
        __syncthreads();   // staging reads (w = 1) / wave 0's adds of the previous round are done
        if (wave == w) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) lds[((m * 9 + tap) * 4 + reg) * 64 + lane] = acc[m][tap][reg];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) acc[m][tap][reg] += lds[((m * 9 + tap) * 4 + reg) * 64 + lane];
        }
    }
    if (wave == 0) {
        const int ci = ci0 + lc;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int co = co0 + 16 * m + 4 * lk + reg;
                    if (co < cout && ci < cin_t) wslab[(((long long)j * cout + co) * cin_t + ci) * 9 + tap] = acc[m][tap][reg];
                }
    }
}

// element e of grad_weight (e < nw, J slabs) or grad_bias (nw <= e < nw + nb, JB slabs): its slab values added in slab order
__global__ void conv_bwd_slab_sum_kernel(const float* __restrict__ wslab, const float* __restrict__ bslab, float* __restrict__ gw,
                                         float* __restrict__ gb, int nw, int nb, int J, int JB) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nw + nb) return;
    const bool isw = e < nw;
    if (isw ? gw == nullptr : gb == nullptr) return;
    const float* src = isw ? wslab + e : bslab + (e - nw);
    const long long pitch = isw ? nw : nb;
    const int cnt = isw ? J : JB;
    float a = 0.0f;
    for (int j = 0; j < cnt; ++j) a += src[j * pitch];
    if (isw) gw[e] = a; else gb[e - nw] = a;
}

static long long cb_tiles(int n, int h, int w) { return (long long)n * h * ((w + 63) / 64); }
static int cb_cop(int cout) { return (cout + 3) / 4 * 4; }
static int cb_cip(int cin_t) { return (cin_t + 15) / 16 * 16 + 16; }   // a tile that starts at any channel stays inside the row

// slabs of the weight pass: enough workgroups to fill the chip, each walking four tiles or more where there are that many; a function of
// the shape alone
static int cb_slabs(int n, int cin_t, int cout, int h, int w) {
    const long long tiles = cb_tiles(n, h, w), blocks = (long long)((cin_t + CW_CI - 1) / CW_CI) * ((cout + CW_CO - 1) / CW_CO);
    const long long want = (2048 + blocks - 1) / blocks, cap = (tiles + 3) / 4;
    return (int)(cap < want ? cap : want);
}

// slabs of the bias pass
static int cb_bias_slabs(int n, int cout, int h, int w) {
    const long long chunks = ((long long)n * h * w + 255) / 256, want = (1024 + cout - 1) / cout;
    return (int)(chunks < want ? chunks : want);
}

static size_t cb_gz_bytes(int n, int cout, int h, int w) { return align_up((size_t)n * cout * h * w * sizeof(float), 256); }
static size_t cb_wt_bytes(int cin_t, int cout) { return align_up((size_t)9 * cb_cop(cout) * cb_cip(cin_t) * sizeof(float), 256); }
static size_t cb_wslab_bytes(int n, int cin_t, int cout, int h, int w) {
    return align_up((size_t)cb_slabs(n, cin_t, cout, h, w) * cout * cin_t * 9 * sizeof(float), 256);
}
static size_t cb_bslab_bytes(int n, int cout, int h, int w) { return align_up((size_t)cb_bias_slabs(n, cout, h, w) * cout * sizeof(float), 256); }

bool conv3x3_backward_shape_ok(int n, int cin_t, int cout, int h, int w) {
    if (!(n >= 1 && n <= 65535 && cin_t >= 1 && cout >= 1 && cin_t <= CB_MAXC && cout <= CB_MAXC && h >= 1 && w >= 1 && h <= 4 * 65535 && w <= (1 << 30)))
        return false;
    // every tensor's element count (and byte count, the slabs' included) stays far inside 64 bits
    return (long long)h * w <= (1LL << 58) / ((long long)n * (cin_t + 2LL * cout));
}

size_t conv3x3_backward_workspace_bytes(int n, int cin_t, int cout, int h, int w) {
    if (!conv3x3_backward_shape_ok(n, cin_t, cout, h, w)) return 0;
    return cb_gz_bytes(n, cout, h, w) + cb_wt_bytes(cin_t, cout) + cb_wslab_bytes(n, cin_t, cout, h, w) + cb_bslab_bytes(n, cout, h, w);
}

int launch_conv3x3_backward(const float* x, int cin, const float* x2, int cin2, const float* weight, const float* out, const float* go, float* gx,
                            float* gx2, float* gw, float* gb, int N, int cout, int H, int W, int act, float post_scale, int unshuffle_r,
                            int shuffle_r, void* workspace, hipStream_t s) {
    const int cin_t = cin + cin2, unshuf = unshuffle_r == 4, r = shuffle_r > 1 ? shuffle_r : 1;
    const double px = (double)N * H * W;
    ProfScope prof("conv3x3_backward_nchw", s, px * (2.0 * cin_t + 4.0 * cout) * 4.0, 2.0 * px * cin_t * cout * 9 * ((gx || gx2 ? 1 : 0) + (gw ? 1 : 0)));
    char* p = (char*)workspace;
    float* gz = (float*)p; p += cb_gz_bytes(N, cout, H, W);
    float* wt = (float*)p; p += cb_wt_bytes(cin_t, cout);
    float* wslab = (float*)p; p += cb_wslab_bytes(N, cin_t, cout, H, W);
    float* bslab = (float*)p;
    const long long HW = (long long)H * W, total = (long long)N * cout * HW;
    {
        const long long blocks = (total + 255) / 256;
        conv_bwd_gz_kernel<<<(unsigned)(blocks < 8192 ? blocks : 8192), 256, 0, s>>>(go, out, gz, cout, H, W, r, act, post_scale, total);
        CRFP_CHECK_LAUNCH();
    }
    if (gx || gx2) {
        const int coP = cb_cop(cout), ciP = cb_cip(cin_t), nwt = 9 * coP * ciP;
        conv_bwd_wt_kernel<<<(nwt + 255) / 256, 256, 0, s>>>(weight, wt, cin_t, cout, coP, ciP);
        CRFP_CHECK_LAUNCH();
        const int c_lo = gx ? 0 : cin, c_hi = gx2 ? cin_t : cin;
        const int ncg = (c_hi - c_lo + 16 * CB_NT - 1) / (16 * CB_NT);
        const long long items = (long long)N * H * ((W + 63) / 64) * ncg;
        conv_bwd_input_kernel<<<(unsigned)(items < (1 << 20) ? items : (1 << 20)), 256, 0, s>>>(gz, wt, gx, gx2, cin, cin2, cout, coP, ciP, H, W, unshuf,
                                                                                               c_lo, c_hi, ncg, items);
        CRFP_CHECK_LAUNCH();
    }
    const int J = cb_slabs(N, cin_t, cout, H, W), JB = cb_bias_slabs(N, cout, H, W);
    if (gw) {
        conv_bwd_weight_kernel<<<dim3(J, (cin_t + CW_CI - 1) / CW_CI, (cout + CW_CO - 1) / CW_CO), 256, 0, s>>>(gz, x, x2, wslab, cin, cin2, cout, H, W,
                                                                                                            unshuf, cb_tiles(N, H, W));
        CRFP_CHECK_LAUNCH();
    }
    if (gb) {
        conv_bwd_bias_kernel<<<dim3(JB, cout), 256, 0, s>>>(gz, bslab, cout, HW, (long long)N * HW);
        CRFP_CHECK_LAUNCH();
    }
    if (gw || gb) {
        const int nw = cout * cin_t * 9;
        conv_bwd_slab_sum_kernel<<<(nw + cout + 255) / 256, 256, 0, s>>>(wslab, bslab, gw, gb, nw, cout, J, JB);
        CRFP_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace crfp
