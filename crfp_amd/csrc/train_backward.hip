// The backward passes that close the training graph of CRFP_DSV's per-operator route, and its loss (NCHW fp32 API tensors; fp32 build only):
//   upsample_bilinear backward   adjoint of crfp_upsample_bilinear_f32 (align_corners=False; scale and size mode, downscaling included)
//   avgpool2 backward            adjoint of crfp_avgpool2_f32 (floor mode)
//   charbonnier / its backward   the reference's masked Charbonnier loss (loss/loss.py:26-68,115-124) as per-sample float64 sums
// Plain streaming kernels, one owner per output element and one plain store: no atomics, every result bitwise reproducible.  All
// global indices are 64-bit.
#include "crfp_common.h"
#include "resample_index.h"

namespace crfp {

using crfp_index::src_index;

// ---- bilinear resize backward, written as a gather: the thread that owns input pixel (iy, ix) walks the outputs whose footprint can
// include it and keeps those for which the forward's own src_index names (iy, ix).
//
// Candidate outputs of input index i on one axis: src = scale * (o + 0.5) - 0.5 must fall in [i - 1, i + 1), i.e.
// o in [(i - 0.5) / scale - 0.5, (i + 1.5) / scale - 0.5), widened by one on each side against the rounding of the float arithmetic.
// The two clamps of src_index make index 0 the home of every src < 0 (the range starts at output 0) and index in - 1 the home of every
// src >= in - 1 (the range ends at the last output).  The bounds are clamped as floats before the conversion, so any positive finite
// scale is safe.
__device__ __forceinline__ void candidate_range(int i, float scale, int in_size, int out_size, int& lo, int& hi) {
    const float last = (float)(out_size - 1);
    const float flo = floorf(((float)i - 0.5f) / scale - 0.5f) - 1.0f;
    const float fhi = ceilf(((float)i + 1.5f) / scale - 0.5f) + 1.0f;
    lo = i == 0 ? 0 : (int)fminf(fmaxf(flo, 0.0f), last);
    hi = i == in_size - 1 ? out_size - 1 : (int)fminf(fmaxf(fhi, 0.0f), last);
}

// the forward's weight of input index i in output o of one axis; false: o does not read i.  At a clamped edge i0 == i1 and both
// weights land on the same input: their sum.
__device__ __forceinline__ bool axis_weight(int o, float scale, int in_size, int i, float& wgt) {
    int i0, i1;
    float l0, l1;
    src_index(o, scale, in_size, i0, i1, l0, l1);
    if (i0 != i && i1 != i) return false;
    wgt = (i0 == i ? l0 : 0.0f) + (i1 == i ? l1 : 0.0f);
    return true;
}

// One thread per input pixel, workgroup = 4 rows x 64 pixels (rows contiguous over lanes); grid.z = plane (n * c).
__global__ void __launch_bounds__(256) upsample_bilinear_bwd_kernel(const float* __restrict__ go, float* __restrict__ gx, int H, int W, int OH,
                                                                    int OW, float sh, float sw, float mul) {
    const int ix = blockIdx.x * 64 + (threadIdx.x & 63);
    const int iy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ix >= W || iy >= H) return;
    const long long nc = blockIdx.z;
    const float* g = go + nc * OH * OW;
    int ylo, yhi, xlo, xhi;
    candidate_range(iy, sh, H, OH, ylo, yhi);
    candidate_range(ix, sw, W, OW, xlo, xhi);
    float acc = 0.0f;   // an input no output reads keeps this exact zero
    for (int oy = ylo; oy <= yhi; ++oy) {
        float wy;
        if (!axis_weight(oy, sh, H, iy, wy)) continue;
        const float* row = g + (long long)oy * OW;
        float racc = 0.0f;
        for (int ox = xlo; ox <= xhi; ++ox) {
            float wx;
            if (axis_weight(ox, sw, W, ix, wx)) racc += wx * row[ox];
        }
        acc += wy * racc;
    }
    gx[(nc * H + iy) * W + ix] = mul * acc;
}

bool train_backward_plane_shape_ok(int n, int c, int h, int w, int oh, int ow) {
    if (!((long long)n * c <= 65535 && h <= 4 * 65535 && w <= (1 << 30) && oh <= (1 << 30) && ow <= (1 << 30))) return false;
    const long long planes = (long long)n * c;
    return (long long)h * w <= (1LL << 58) / planes && (long long)oh * ow <= (1LL << 58) / planes;
}

int launch_upsample_bilinear_backward(const float* go, float* gx, int N, int C, int H, int W, int OH, int OW, float sh, float sw, float mul,
                                      hipStream_t s) {
    ProfScope prof("upsample_bilinear_backward_nchw", s, (double)N * C * 4.0 * ((double)H * W + (double)OH * OW), 0);
    dim3 grid((W + 63) / 64, (H + 3) / 4, N * C);
    upsample_bilinear_bwd_kernel<<<grid, 256, 0, s>>>(go, gx, H, W, OH, OW, sh, sw, mul);
    CRFP_CHECK_LAUNCH();
    return 0;
}

// ---- AvgPool2d(2, 2) backward: every input pixel of the pooled area gets a quarter of its output's gradient, the odd trailing row or
// column that floor mode drops an exact zero.
__global__ void __launch_bounds__(256) avgpool2_bwd_kernel(const float* __restrict__ go, float* __restrict__ gx, int H, int W) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const long long nc = blockIdx.z;
    const int OH = H / 2, OW = W / 2;
    float v = 0.0f;
    if (y < 2 * OH && x < 2 * OW) v = 0.25f * go[(nc * OH + (y >> 1)) * OW + (x >> 1)];
    gx[(nc * H + y) * W + x] = v;
}

int launch_avgpool2_backward(const float* go, float* gx, int N, int C, int H, int W, hipStream_t s) {
    ProfScope prof("avgpool2_backward_nchw", s, (double)N * C * 4.0 * ((double)H * W * 1.25), 0);
    avgpool2_bwd_kernel<<<dim3((W + 63) / 64, (H + 3) / 4, N * C), 256, 0, s>>>(go, gx, H, W);
    CRFP_CHECK_LAUNCH();
    return 0;
}

// ---- Charbonnier loss: sums[n][0] = sum sqrt(d^2 + eps) * w, sums[n][1] = sum w over the sample (w expanded over c; 1 without a weight),
// d = pred - target.  Elements in fp32 (the reference's arithmetic), sums in float64.  Two launches: per-workgroup partials into the
// workspace, then one wave per sample adds them in a fixed order -- the grid depends on the shape alone, so the sums are reproducible.
constexpr int CB_MAX_BLOCKS = 512;

int charbonnier_blocks(int c, int h, int w) {
    const long long chw = (long long)c * h * w, b = (chw + 1023) / 1024;   // about four elements per thread
    return (int)(b < 1 ? 1 : (b > CB_MAX_BLOCKS ? CB_MAX_BLOCKS : b));
}

size_t charbonnier_workspace_bytes(int n, int c, int h, int w) {
    return align_up((size_t)n * charbonnier_blocks(c, h, w) * 2 * sizeof(double), 256);
}

// the weight of element e = (ch, pix) of a sample: wc = 0 none, 1 one plane per sample, c one per channel
__device__ __forceinline__ float cb_weight(const float* __restrict__ wgt, int wc, long long HW, long long e) {
    if (wc == 0) return 1.0f;
    return wc == 1 ? wgt[e % HW] : wgt[e];
}

__global__ void __launch_bounds__(256) charbonnier_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                  const float* __restrict__ wgt, int wc, double* __restrict__ part, int C,
                                                                  long long HW, float eps) {
    const int n = blockIdx.y;
    const long long chw = (long long)C * HW;
    const float* p = pred + n * chw;
    const float* t = target + n * chw;
    const float* wn = wgt ? wgt + (long long)n * wc * HW : nullptr;
    double s0 = 0.0, s1 = 0.0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < chw; e += (long long)gridDim.x * 256) {
        const float d = p[e] - t[e];
        const float wv = cb_weight(wn, wc, HW, e);
        s0 += (double)(sqrtf(d * d + eps) * wv);
        s1 += (double)wv;
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
        double* q = part + ((long long)n * gridDim.x + blockIdx.x) * 2;
        q[0] = ((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3];
        q[1] = ((sh[1][0] + sh[1][1]) + sh[1][2]) + sh[1][3];
    }
}

__global__ void __launch_bounds__(64) charbonnier_final_kernel(const double* __restrict__ part, double* __restrict__ sums, int blocks) {
    const int n = blockIdx.x;
    const double* q = part + (long long)n * blocks * 2;
    double s0 = 0.0, s1 = 0.0;
    for (int b = threadIdx.x; b < blocks; b += 64) { s0 += q[2 * b]; s1 += q[2 * b + 1]; }
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_down(s0, o);
        s1 += __shfl_down(s1, o);
    }
    if (threadIdx.x == 0) { sums[2 * n] = s0; sums[2 * n + 1] = s1; }
}

int launch_charbonnier(const float* pred, const float* target, const float* wgt, int wc, double* sums, int N, int C, int H, int W, float eps,
                       void* workspace, hipStream_t s) {
    const long long HW = (long long)H * W;
    const int blocks = charbonnier_blocks(C, H, W);
    double* part = reinterpret_cast<double*>(workspace);
    {
        ProfScope prof("charbonnier_partial", s, (double)N * HW * (2.0 * C + wc) * 4.0, 0);
        charbonnier_partial_kernel<<<dim3(blocks, N), 256, 0, s>>>(pred, target, wgt, wc, part, C, HW, eps);
        CRFP_CHECK_LAUNCH();
    }
    ProfScope prof("charbonnier_final", s, (double)N * blocks * 16.0, 0);
    charbonnier_final_kernel<<<N, 64, 0, s>>>(part, sums, blocks);
    CRFP_CHECK_LAUNCH();
    return 0;
}

// grad_pred = scale[n] * w * d / sqrt(d^2 + eps)
__global__ void __launch_bounds__(256) charbonnier_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                              const float* __restrict__ wgt, int wc, const float* __restrict__ scale,
                                                              float* __restrict__ gp, int C, long long HW, float eps) {
    const int n = blockIdx.y;
    const long long chw = (long long)C * HW;
    const float* p = pred + n * chw;
    const float* t = target + n * chw;
    const float* wn = wgt ? wgt + (long long)n * wc * HW : nullptr;
    float* g = gp + n * chw;
    const float sc = scale[n];
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < chw; e += (long long)gridDim.x * 256) {
        const float d = p[e] - t[e];
        g[e] = sc * cb_weight(wn, wc, HW, e) * (d / sqrtf(d * d + eps));
    }
}

int launch_charbonnier_backward(const float* pred, const float* target, const float* wgt, int wc, const float* scale, float* gp, int N, int C,
                                int H, int W, float eps, hipStream_t s) {
    const long long HW = (long long)H * W, chw = (long long)C * HW;
    ProfScope prof("charbonnier_backward", s, (double)N * HW * (3.0 * C + wc) * 4.0, 0);
    long long blocks = (chw + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    charbonnier_bwd_kernel<<<dim3((int)blocks, N), 256, 0, s>>>(pred, target, wgt, wc, scale, gp, C, HW, eps);
    CRFP_CHECK_LAUNCH();
    return 0;
}

}  // namespace crfp
