// Image-quality metrics of the eval path, three kernel families (the third, the frame metrics table, is described where it starts).
//
// 1. psnr_ssim_partial_kernel: masked PSNR + SSIM partial sums in one pass over an image pair.
// Replaces utils.calc_psnr_and_ssim_cuda -> psnr_cuda / ssim_cuda / _ssim (reference utils.py:166-185,187-240,242-254):
//   x' = x*mul + add                              (the data-dependent range conversion of utils.py:244-250, chosen by the host)
//   mse  = sum_c,p m(p) (a'-b')^2 / (sum_p m(p) * C)
//   ssim = sum_c,p m(p) S_c(p)    / (sum_p m(p) * C),   S from the 11x11 gaussian (sigma 1.5) windowed means, zero padding,
//          C1 = 0.01^2, C2 = 0.03^2 (image range [0,1]).
// The reference filters with the 121-tap outer-product window; here the window is applied separably (rows, then columns) in
// fp32 -- same weights g[i]*g[j] up to fp32 rounding order.  acc[0] += sum m (a'-b')^2, acc[1] += sum m S, acc[2] += sum m.
//
// 2. window_probe_kernel + window_scores_kernel: the foveated score maps of the video rig (reference test_video.py:23-63
// foveated_metric -> the batch_avg=True branches of utils.py:166-172,197-221,242-254): PSNR and mean SSIM of every k x k window at
// stride s, each window treated as an image of its own (zero padding at the WINDOW's border).  The reference unfolds both images
// (300 floats per window) and runs five grouped convolutions over the patches; here a workgroup keeps one channel of a tile of the
// image pair in LDS, nothing per window is ever written to memory, and the data-dependent range conversion is decided on the
// device (no host synchronisation).
#include "crfp_common.h"

namespace crfp {

constexpr int SW = 64, SH = 16, SR = 5, SLW = SW + 2 * SR, SLH = SH + 2 * SR;   // output tile, window radius, halo tile

struct SsimWin { float g[11]; };

__global__ __launch_bounds__(256) void psnr_ssim_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                const uint8_t* __restrict__ mask, double* __restrict__ acc,
                                                                int C, int H, int W, float mul, float add, SsimWin win) {
    __shared__ float ta[SLH][SLW], tb[SLH][SLW];
    __shared__ float hb[5][SLH][SW];        // row-filtered a, b, a^2, b^2, ab
    __shared__ double red[3][4];
    const int tid = threadIdx.x;
    const int nc = blockIdx.z, n = nc / C;
    const int x0 = blockIdx.x * SW, y0 = blockIdx.y * SH;
    const float* pa = a + (long long)nc * H * W;
    const float* pb = b + (long long)nc * H * W;
    for (int i = tid; i < SLH * SLW; i += 256) {
        const int r = i / SLW, c = i - r * SLW;
        const int gy = y0 + r - SR, gx = x0 + c - SR;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;   // F.conv2d zero padding applies to the converted image
        ta[r][c] = in ? pa[(long long)gy * W + gx] * mul + add : 0.0f;
        tb[r][c] = in ? pb[(long long)gy * W + gx] * mul + add : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < SLH * SW; i += 256) {
        const int r = i / SW, c = i - r * SW;
        float s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const float va = ta[r][c + k], vb = tb[r][c + k], g = win.g[k];
            s0 += g * va; s1 += g * vb; s2 += g * (va * va); s3 += g * (vb * vb); s4 += g * (va * vb);
        }
        hb[0][r][c] = s0; hb[1][r][c] = s1; hb[2][r][c] = s2; hb[3][r][c] = s3; hb[4][r][c] = s4;
    }
    __syncthreads();
    double se = 0.0, ss = 0.0, sm = 0.0;
    for (int i = tid; i < SH * SW; i += 256) {
        const int r = i / SW, c = i - r * SW;
        const int gy = y0 + r, gx = x0 + c;
        if (gy >= H || gx >= W) continue;
        float m[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const float g = win.g[k];
#pragma unroll
            for (int q = 0; q < 5; ++q) m[q] += g * hb[q][r + k][c];
        }
        const float mu1 = m[0], mu2 = m[1];
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const float s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu12;
        const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
        const float S = ((2.0f * mu12 + C1) * (2.0f * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
        const float mk = mask ? (mask[(long long)n * H * W + (long long)gy * W + gx] ? 1.0f : 0.0f) : 1.0f;
        const float d = ta[r + SR][c + SR] - tb[r + SR][c + SR];
        se += (double)(mk * d * d);
        ss += (double)(mk * S);
        if (nc - n * C == 0) sm += (double)mk;     // the mask is shared by the C channels: count it once
    }
    for (int o = 32; o > 0; o >>= 1) { se += __shfl_down(se, o); ss += __shfl_down(ss, o); sm += __shfl_down(sm, o); }
    const int lane = tid & 63, wv = tid >> 6;
    if (lane == 0) { red[0][wv] = se; red[1][wv] = ss; red[2][wv] = sm; }
    __syncthreads();
    if (tid == 0) {
        atomicAdd(&acc[0], red[0][0] + red[0][1] + red[0][2] + red[0][3]);
        atomicAdd(&acc[1], red[1][0] + red[1][1] + red[1][2] + red[1][3]);
        atomicAdd(&acc[2], red[2][0] + red[2][1] + red[2][2] + red[2][3]);
    }
}

static void ssim_window(SsimWin& win) {
    // utils.gaussian(11, 1.5): float32 tensor of exp(...) normalised by its float32 sum.  torch's sum of the 11 taps is the correctly
    // rounded one (3.7592328), taken here through double; adding them one by one in fp32 lands one ulp below it and makes every tap
    // 1.1e-7 larger -- invisible on noise in [0, 1], 6e-6 of SSIM on smooth frames and 6e-3 on unconverted luma near 125, where
    // E[x^2] - mu^2 carries 15 625 times the window's excess weight.
    float g[11];
    double sum = 0.0;
    for (int x = 0; x < 11; ++x) { g[x] = (float)exp(-(double)((x - 5) * (x - 5)) / (2.0 * 1.5 * 1.5)); sum += (double)g[x]; }
    for (int x = 0; x < 11; ++x) win.g[x] = g[x] / (float)sum;
}

int launch_psnr_ssim_partial(const float* a, const float* b, const uint8_t* mask, double* acc, int N, int C, int H, int W,
                             float mul, float add, hipStream_t s) {
    SsimWin win;
    ssim_window(win);
    ProfScope prof("psnr_ssim_partial", s, (double)N * C * H * W * 8.0, (double)N * C * H * W * 2.0 * 5 * 22);
    dim3 grid((W + SW - 1) / SW, (H + SH - 1) / SH, N * C);
    psnr_ssim_partial_kernel<<<grid, 256, 0, s>>>(a, b, mask, acc, C, H, W, mul, add, win);
    CRFP_CHECK_LAUNCH();
    return 0;
}


// ---------------------------------------------------------------------------------------------------- window score maps
constexpr int WS_THREADS = 256;
constexpr int WS_PROBE_BLOCKS = 256;   // partial (min, max) pairs per image; = WS_THREADS so that one load per thread folds them
constexpr int WS_KMAX = 16;            // largest window side (the accumulators of one window column live in registers)
constexpr int WS_PIX = 4096;           // LDS floats per image for the pixel tile of one channel (16 KiB each)
constexpr int WS_ITEMS = 1280;         // (window, column) pairs per workgroup: 128 windows of 10 columns = 5 full passes of 256 lanes

// torch.min / torch.max semantics: a NaN wins and stays
__device__ __forceinline__ float ws_min(float a, float b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ float ws_max(float a, float b) { return (b > a || b != b) ? b : a; }

// (min, max) of the pixels of `b` that some window covers (rows < hc, columns < wc), all channels of image blockIdx.y:
// stage one of two, one pair per workgroup into part[n][WS_PROBE_BLOCKS][2]; window_scores_kernel folds the pairs.
__global__ __launch_bounds__(WS_THREADS) void window_probe_kernel(const float* __restrict__ b, float* __restrict__ part,
                                                                  int C, int H, int W, int hc, int wc) {
    __shared__ float red[2][WS_THREADS / 64];
    const int tid = threadIdx.x, n = blockIdx.y;
    const float* pb = b + (long long)n * C * H * W;
    float mn = pb[0], mx = mn;   // pixel (0, 0) is covered by window (0, 0)
    for (int row = blockIdx.x; row < C * hc; row += WS_PROBE_BLOCKS) {
        const int c = row / hc, r = row - c * hc;
        const float* pr = pb + ((long long)c * H + r) * W;
        for (int x = tid; x < wc; x += WS_THREADS) { const float v = pr[x]; mn = ws_min(mn, v); mx = ws_max(mx, v); }
    }
    for (int o = 32; o > 0; o >>= 1) { mn = ws_min(mn, __shfl_down(mn, o)); mx = ws_max(mx, __shfl_down(mx, o)); }
    if ((tid & 63) == 0) { red[0][tid >> 6] = mn; red[1][tid >> 6] = mx; }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < WS_THREADS / 64; ++i) { mn = ws_min(mn, red[0][i]); mx = ws_max(mx, red[1][i]); }
        float* o = part + ((long long)n * WS_PROBE_BLOCKS + blockIdx.x) * 2;
        o[0] = mn; o[1] = mx;
    }
}

struct WinScoreArgs {
    int C, H, W, k, s, Hr, Wr;     // image, window side, stride, score-map size
    int twx, twy, cols, rows;      // windows per workgroup tile; its pixel tile = (twy-1)*s+k rows of (twx-1)*s+k columns
    float floor_db;                // PSNR of a window with mse == 0 (utils.py:171)
    SsimWin win;
};

// One workgroup = twy x twx windows of image blockIdx.z.  Per channel: the pixel tile of both images goes to LDS (rows
// coalesced, range-converted on load); then one lane per (window, column x) walks the window's k rows: the row-filtered
// a, b, a^2, b^2, ab at (r, x) from <= 11 LDS taps (truncated at the window's border = the reference's zero padding of the
// patch), pushed at once into the <= 11 column accumulators they belong to (registers; rows and columns fully unrolled so
// that every gaussian weight is an immediate).  After the last row the lane owns the SSIM map of its column; it adds the
// column's sum of S and of (a-b)^2 to its own LDS slot.  After the last channel one lane per window adds the k slots in
// order and writes the two scores: one store each, no atomics.
__global__ __launch_bounds__(WS_THREADS) void window_scores_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                   const float* __restrict__ part, float* __restrict__ psnr,
                                                                   float* __restrict__ ssim, WinScoreArgs A) {
    __shared__ float ta[WS_PIX], tb[WS_PIX];
    __shared__ double pse[WS_ITEMS], pss[WS_ITEMS];
    __shared__ float red[2][WS_THREADS / 64];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int k = A.k, s = A.s, cols = A.cols;
    // ---- range conversion of utils.py:244-250 from the probe's partial pairs (every workgroup folds the same 256 pairs in the same order)
    float mn = part[((long long)n * WS_PROBE_BLOCKS + tid) * 2], mx = part[((long long)n * WS_PROBE_BLOCKS + tid) * 2 + 1];
    for (int o = 32; o > 0; o >>= 1) { mn = ws_min(mn, __shfl_down(mn, o)); mx = ws_max(mx, __shfl_down(mx, o)); }
    if ((tid & 63) == 0) { red[0][tid >> 6] = mn; red[1][tid >> 6] = mx; }
    __syncthreads();
    mn = red[0][0]; mx = red[1][0];
    for (int i = 1; i < WS_THREADS / 64; ++i) { mn = ws_min(mn, red[0][i]); mx = ws_max(mx, red[1][i]); }
    const float span = mx - mn;
    const int mode = span > 2.0f ? 2 : (span > 1.0f ? 1 : 0);   // NaN span: no conversion, as the reference's comparisons

    const int wx0 = blockIdx.x * A.twx, wy0 = blockIdx.y * A.twy;
    const int px0 = wx0 * s, py0 = wy0 * s;
    const int nwx = min(A.twx, A.Wr - wx0), nwy = min(A.twy, A.Hr - wy0);      // windows of this tile that exist
    const int ucols = (nwx - 1) * s + k, urows = (nwy - 1) * s + k;              // pixels they cover: inside the image by construction
    const int items = nwx * nwy * k;
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    for (int c = 0; c < A.C; ++c) {
        const float* pa = a + ((long long)n * A.C + c) * A.H * A.W;
        const float* pb = b + ((long long)n * A.C + c) * A.H * A.W;
        if (c) __syncthreads();   // the previous channel's lanes are done with the tile
        for (int i = tid; i < urows * ucols; i += WS_THREADS) {
            const int r = i / ucols, x = i - r * ucols;
            const long long g = (long long)(py0 + r) * A.W + px0 + x;
            float va = pa[g], vb = pb[g];
            if (mode == 2) { va = va / 255.0f; vb = vb / 255.0f; }
            else if (mode == 1) { va = (va + 1.0f) * 0.5f; vb = (vb + 1.0f) * 0.5f; }
            ta[r * cols + x] = va; tb[r * cols + x] = vb;
        }
        __syncthreads();
        for (int it = tid; it < items; it += WS_THREADS) {
            const int wl = it / k, x = it - wl * k;
            const int wyl = wl / nwx, wxl = wl - wyl * nwx;
            const int base = wyl * s * cols + wxl * s;
            float wr[11]; int qo[11];        // row taps of column x: weight (0 outside the window) and tile offset
#pragma unroll
            for (int j = 0; j < 11; ++j) {
                const int q = x - 5 + j;
                const bool in = q >= 0 && q < k;
                wr[j] = in ? A.win.g[j] : 0.0f;
                qo[j] = base + (in ? q : x);
            }
            float acc[WS_KMAX][5];
#pragma unroll
            for (int y = 0; y < WS_KMAX; ++y)
#pragma unroll
                for (int q = 0; q < 5; ++q) acc[y][q] = 0.0f;
            double se = 0.0;
#pragma unroll
            for (int r = 0; r < WS_KMAX; ++r) {
                if (r < k) {
                    const int ro = r * cols;
                    float h0 = 0, h1 = 0, h2 = 0, h3 = 0, h4 = 0;
#pragma unroll
                    for (int j = 0; j < 11; ++j) {
                        const float va = ta[ro + qo[j]], vb = tb[ro + qo[j]], g = wr[j];
                        h0 = fmaf(g, va, h0); h1 = fmaf(g, vb, h1);
                        h2 = fmaf(g, va * va, h2); h3 = fmaf(g, vb * vb, h3); h4 = fmaf(g, va * vb, h4);
                    }
                    const float d = ta[ro + base + x] - tb[ro + base + x];
                    se += (double)(d * d);
#pragma unroll
                    for (int y = 0; y < WS_KMAX; ++y) {
                        if (y - r <= 5 && r - y <= 5) {     // compile-time: the column taps of row r
                            const float g = A.win.g[r - y + 5];
                            acc[y][0] = fmaf(g, h0, acc[y][0]); acc[y][1] = fmaf(g, h1, acc[y][1]);
                            acc[y][2] = fmaf(g, h2, acc[y][2]); acc[y][3] = fmaf(g, h3, acc[y][3]);
                            acc[y][4] = fmaf(g, h4, acc[y][4]);
                        }
                    }
                }
            }
            double ss = 0.0;
#pragma unroll
            for (int y = 0; y < WS_KMAX; ++y) {
                if (y < k) {
                    const float mu1 = acc[y][0], mu2 = acc[y][1];
                    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
                    const float s1 = acc[y][2] - mu1_sq, s2 = acc[y][3] - mu2_sq, s12 = acc[y][4] - mu12;
                    ss += (double)(((2.0f * mu12 + C1) * (2.0f * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2)));
                }
            }
            // the same lane owns slot `it` for every channel
            pse[it] = c ? pse[it] + se : se;
            pss[it] = c ? pss[it] + ss : ss;
        }
    }
    __syncthreads();
    const double cnt = (double)A.C * k * k;
    for (int wl = tid; wl < nwx * nwy; wl += WS_THREADS) {
        double se = 0.0, ss = 0.0;
        for (int x = 0; x < k; ++x) { se += pse[wl * k + x]; ss += pss[wl * k + x]; }
        const int wyl = wl / nwx, wxl = wl - wyl * nwx;
        const long long o = ((long long)n * A.Hr + wy0 + wyl) * A.Wr + wx0 + wxl;
        // every square is an fp32 number and their sum is exact enough in double that se == 0 <=> the fp32 sum is 0 <=> all are 0
        psnr[o] = se == 0.0 ? A.floor_db : (float)(-10.0 * log10(se / cnt));
        ssim[o] = (float)(ss / cnt);
    }
}

size_t window_scores_workspace_bytes(int N) { return N < 1 ? 0 : (size_t)N * WS_PROBE_BLOCKS * 2 * sizeof(float); }

// hr, sr: [N,C,H,W]; psnr, ssim: [N,Hr,Wr].  The caller has checked 1 <= k <= WS_KMAX, k <= H, k <= W, s >= 1.
int launch_window_scores(const float* hr, const float* sr, float* psnr, float* ssim, int N, int C, int H, int W, int k, int stride,
                         float* part, hipStream_t s) {
    WinScoreArgs A;
    A.C = C; A.H = H; A.W = W; A.k = k; A.s = stride;
    A.Hr = (H - k) / stride + 1; A.Wr = (W - k) / stride + 1;
    ssim_window(A.win);
    A.floor_db = (float)(-20.0 * log10(sqrt((1.0 / 255.0) * (1.0 / 255.0) / ((double)C * k * k))));
    // the tile: as many windows as the LDS budget holds (1 x 1 always fits: k*k <= 256), then the fewest pixels, then the widest rows
    long long best = -1;
    A.twx = A.twy = 1;
    for (int ty = 1; ty <= std::min(A.Hr, 64); ++ty)
        for (int tx = 1; tx <= std::min(A.Wr, 64); ++tx) {
            const long long pc = (long long)(tx - 1) * stride + k, pr = (long long)(ty - 1) * stride + k;
            if (pc * pr > WS_PIX || tx * ty * k > WS_ITEMS) break;   // wider tiles of this row only grow
            const long long score = ((long long)tx * ty << 32) + ((long long)(WS_PIX - pc * pr) << 8) + tx;
            if (score > best) { best = score; A.twx = tx; A.twy = ty; }
        }
    A.cols = (A.twx - 1) * stride + k; A.rows = (A.twy - 1) * stride + k;
    const int hc = (A.Hr - 1) * stride + k, wc = (A.Wr - 1) * stride + k;
    const double px = (double)N * C * H * W, wins = (double)N * A.Hr * A.Wr;
    {
        ProfScope prof("window_probe", s, px * 4.0, px * 2.0);
        window_probe_kernel<<<dim3(WS_PROBE_BLOCKS, N), WS_THREADS, 0, s>>>(sr, part, C, H, W, hc, wc);
        CRFP_CHECK_LAUNCH();
    }
    ProfScope prof("window_scores", s, px * 8.0 + wins * 8.0, wins * C * k * k * 2.0 * (8.0 * 11 + 5.0 * 11));
    dim3 grid((A.Wr + A.twx - 1) / A.twx, (A.Hr + A.twy - 1) / A.twy, N);
    window_scores_kernel<<<grid, WS_THREADS, 0, s>>>(hr, sr, part, psnr, ssim, A);
    CRFP_CHECK_LAUNCH();
    return 0;
}


// ---------------------------------------------------------------------------------------------------- frame metrics table
// 3. frame_probe_kernel + frame_sums_kernel + frame_final_kernel: PSNR / SSIM / PSNR-Y / SSIM-Y of every frame of a batch, for the
// whole frame and m byte masks, from ONE read of the image pair (the figures of trainer.py:348-369 and of the video rig's regions,
// test_video.py:360-370; definitions utils.py:166-185,242-254,328-330).  The SSIM map of a channel does not depend on the region and
// luma is a per-pixel function of the three channels, so one workgroup owns a 64 x 16 tile of one frame and walks the channels: the
// masks are read once per pixel, the luma of the tile (with its halo) accumulates in registers while the channels pass and is scored
// as a fourth channel, and every (region, quantity) leaves the workgroup as one double.  No atomics, nothing to initialise, no host
// synchronisation; every frame's figures depend on that frame alone.
constexpr int FM_THREADS = 256;
constexpr int FM_PROBE_BLOCKS = 256;   // partial (min, max, luma min, luma max) quadruples per frame; = FM_THREADS: one load per thread folds them
constexpr int FM_MAX_MASKS = 7;
constexpr int FM_Q = 5;                // per (tile, region): sum se, sum S, sum mask, sum se of luma, sum S of luma
constexpr int FM_LOADS = (SLH * SLW + FM_THREADS - 1) / FM_THREADS;   // halo-tile pixels per lane (8)

// utils.bgr2ycbcr(y_only=True) in fp32 on the channels as they arrive; the probe and the sums kernel share the expression bit for bit
__device__ __forceinline__ float fm_luma_step(int ch, float v, float y) {
    return ch == 0 ? 24.966f * v : (ch == 1 ? fmaf(128.553f, v, y) : fmaf(65.481f, v, y) + 16.0f);
}
// the conversion of utils.py:244-250 for a span; a NaN span converts nothing, as the reference's comparisons
__device__ __forceinline__ int fm_mode(float mn, float mx) { const float span = mx - mn; return span > 2.0f ? 2 : (span > 1.0f ? 1 : 0); }
__device__ __forceinline__ float fm_convert(int mode, float v) { return mode == 2 ? v / 255.0f : (mode == 1 ? (v + 1.0f) * 0.5f : v); }

// (min, max) of hr over all channels and pixels of frame blockIdx.y and, with luma, of luma(hr): one quadruple per workgroup.
__global__ __launch_bounds__(FM_THREADS) void frame_probe_kernel(const float* __restrict__ hr, float* __restrict__ part, int C,
                                                                 long long HW, int luma) {
    __shared__ float red[4][FM_THREADS / 64];
    const int tid = threadIdx.x, n = blockIdx.y;
    const float* p = hr + (long long)n * C * HW;
    float mn = p[0], mx = mn, ymn = 0.0f, ymx = 0.0f;
    if (luma) { ymn = fm_luma_step(2, p[2 * HW], fm_luma_step(1, p[HW], fm_luma_step(0, p[0], 0.0f))); ymx = ymn; }
    for (long long i = (long long)blockIdx.x * FM_THREADS + tid; i < HW; i += (long long)FM_PROBE_BLOCKS * FM_THREADS) {
        float y = 0.0f;
        for (int c = 0; c < C; ++c) {
            const float v = p[c * HW + i];
            mn = ws_min(mn, v); mx = ws_max(mx, v);
            if (luma) y = fm_luma_step(c, v, y);
        }
        if (luma) { ymn = ws_min(ymn, y); ymx = ws_max(ymx, y); }
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn = ws_min(mn, __shfl_down(mn, o)); mx = ws_max(mx, __shfl_down(mx, o));
        ymn = ws_min(ymn, __shfl_down(ymn, o)); ymx = ws_max(ymx, __shfl_down(ymx, o));
    }
    if ((tid & 63) == 0) { red[0][tid >> 6] = mn; red[1][tid >> 6] = mx; red[2][tid >> 6] = ymn; red[3][tid >> 6] = ymx; }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < FM_THREADS / 64; ++i) {
            mn = ws_min(mn, red[0][i]); mx = ws_max(mx, red[1][i]); ymn = ws_min(ymn, red[2][i]); ymx = ws_max(ymx, red[3][i]);
        }
        float* o = part + ((long long)n * FM_PROBE_BLOCKS + blockIdx.x) * 4;
        o[0] = mn; o[1] = mx; o[2] = ymn; o[3] = ymx;
    }
}

// One workgroup = tile (blockIdx.x, blockIdx.y) of frame blockIdx.z.  Lane (wave wv, column c) owns the four pixels of column c in
// rows 4 wv .. 4 wv + 3: the column filter slides over the 14 row-filtered rows they share (70 LDS reads for 4 pixels instead of 220).
__global__ __launch_bounds__(FM_THREADS) void frame_sums_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                const uint8_t* __restrict__ masks, const float* __restrict__ probe,
                                                                double* __restrict__ partial, int C, int M, int H, int W, int luma,
                                                                SsimWin win) {
    __shared__ float ta[SLH][SLW], tb[SLH][SLW];
    __shared__ float hb[5][SLH][SW];        // row-filtered a, b, a^2, b^2, ab
    __shared__ float pr[4][FM_THREADS / 64];
    __shared__ double red[1 + FM_MAX_MASKS][FM_Q][FM_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = blockIdx.z;
    const long long HW = (long long)H * W;
    // ---- the frame's conversions from the probe's quadruples (every workgroup folds the same 256 in the same order)
    int mode_rgb, mode_y;
    {
        const float* q = probe + ((long long)n * FM_PROBE_BLOCKS + tid) * 4;
        float mn = q[0], mx = q[1], ymn = luma ? q[2] : 0.0f, ymx = luma ? q[3] : 0.0f;
        for (int o = 32; o > 0; o >>= 1) {
            mn = ws_min(mn, __shfl_down(mn, o)); mx = ws_max(mx, __shfl_down(mx, o));
            ymn = ws_min(ymn, __shfl_down(ymn, o)); ymx = ws_max(ymx, __shfl_down(ymx, o));
        }
        if (lane == 0) { pr[0][wv] = mn; pr[1][wv] = mx; pr[2][wv] = ymn; pr[3][wv] = ymx; }
        __syncthreads();
        mn = pr[0][0]; mx = pr[1][0]; ymn = pr[2][0]; ymx = pr[3][0];
        for (int i = 1; i < FM_THREADS / 64; ++i) {
            mn = ws_min(mn, pr[0][i]); mx = ws_max(mx, pr[1][i]); ymn = ws_min(ymn, pr[2][i]); ymx = ws_max(ymx, pr[3][i]);
        }
        mode_rgb = fm_mode(mn, mx); mode_y = fm_mode(ymn, ymx);
    }
    const int x0 = blockIdx.x * SW, y0 = blockIdx.y * SH;
    const int gx = x0 + lane, gyb = y0 + 4 * wv;          // this lane's pixels: (gyb + o, gx), o = 0..3
    // ---- region membership of the four pixels, one bit per (pixel, region); region 0 = inside the image
    unsigned member[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const bool valid = gx < W && gyb + o < H;
        unsigned bits = valid ? 1u : 0u;
        if (valid)
            for (int k = 0; k < M; ++k)
                bits |= masks[((long long)n * M + k) * HW + (long long)(gyb + o) * W + gx] ? (2u << k) : 0u;
        member[o] = bits;
    }
    float ya[FM_LOADS], yb[FM_LOADS];        // unconverted luma of the halo-tile pixels this lane loads
#pragma unroll
    for (int it = 0; it < FM_LOADS; ++it) ya[it] = yb[it] = 0.0f;
    double pse[4] = {0, 0, 0, 0}, pss[4] = {0, 0, 0, 0}, yse[4] = {0, 0, 0, 0}, yss[4] = {0, 0, 0, 0};
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const int passes = C + (luma ? 1 : 0);
    for (int ch = 0; ch < passes; ++ch) {
        const bool isy = ch == C;
        const int mode = isy ? mode_y : mode_rgb;
        const float* pa = a + ((long long)n * C + (isy ? 0 : ch)) * HW;
        const float* pb = b + ((long long)n * C + (isy ? 0 : ch)) * HW;
        if (ch) __syncthreads();   // the previous pass is done with the tiles
#pragma unroll
        for (int it = 0; it < FM_LOADS; ++it) {
            const int i = tid + it * FM_THREADS;
            if (i < SLH * SLW) {
                const int r = i / SLW, c = i - r * SLW;
                const int gy = y0 + r - SR, gxx = x0 + c - SR;
                const bool in = gy >= 0 && gy < H && gxx >= 0 && gxx < W;   // zero padding applies to the converted image
                float va = 0.0f, vb = 0.0f;
                if (isy) { va = ya[it]; vb = yb[it]; }
                else if (in) {
                    va = pa[(long long)gy * W + gxx]; vb = pb[(long long)gy * W + gxx];
                    if (luma) { ya[it] = fm_luma_step(ch, va, ya[it]); yb[it] = fm_luma_step(ch, vb, yb[it]); }
                }
                ta[r][c] = in ? fm_convert(mode, va) : 0.0f;
                tb[r][c] = in ? fm_convert(mode, vb) : 0.0f;
            }
        }
        __syncthreads();
        for (int i = tid; i < SLH * SW; i += FM_THREADS) {
            const int r = i / SW, c = i - r * SW;
            float s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const float va = ta[r][c + k], vb = tb[r][c + k], g = win.g[k];
                s0 += g * va; s1 += g * vb; s2 += g * (va * va); s3 += g * (vb * vb); s4 += g * (va * vb);
            }
            hb[0][r][c] = s0; hb[1][r][c] = s1; hb[2][r][c] = s2; hb[3][r][c] = s3; hb[4][r][c] = s4;
        }
        __syncthreads();
        float m[4][5];
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int q = 0; q < 5; ++q) m[o][q] = 0.0f;
#pragma unroll
        for (int j = 0; j < 14; ++j) {
            float v[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) v[q] = hb[q][4 * wv + j][lane];
#pragma unroll
            for (int o = 0; o < 4; ++o)
                if (j - o >= 0 && j - o < 11) {        // compile-time: tap j - o of pixel o, taps in rising order as psnr_ssim_partial_kernel
                    const float g = win.g[j - o];
#pragma unroll
                    for (int q = 0; q < 5; ++q) m[o][q] += g * v[q];
                }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const float mu1 = m[o][0], mu2 = m[o][1];
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float s1 = m[o][2] - mu1_sq, s2 = m[o][3] - mu2_sq, s12 = m[o][4] - mu12;
            const float S = ((2.0f * mu12 + C1) * (2.0f * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
            const float d = ta[4 * wv + o + SR][lane + SR] - tb[4 * wv + o + SR][lane + SR];
            if (isy) { yse[o] = (double)(d * d); yss[o] = (double)S; }
            else { pse[o] += (double)(d * d); pss[o] += (double)S; }
        }
    }
    // ---- per region: the workgroup's sums, lanes in shuffle order, waves in rising order
    for (int k = 0; k <= M; ++k) {
        double v[FM_Q] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            if (member[o] & 1u) {      // pixels outside the image hold filter values of the padding: they belong to no region
                const double mk = (member[o] >> k) & 1u ? 1.0 : 0.0;
                v[0] += mk * pse[o]; v[1] += mk * pss[o]; v[2] += mk; v[3] += mk * yse[o]; v[4] += mk * yss[o];
            }
        }
#pragma unroll
        for (int q = 0; q < FM_Q; ++q) {
            for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_down(v[q], o);
            if (lane == 0) red[k][q][wv] = v[q];
        }
    }
    __syncthreads();
    if (tid < (M + 1) * FM_Q) {
        const int k = tid / FM_Q, q = tid - k * FM_Q;
        const long long tile = ((long long)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[(tile * (M + 1) + k) * FM_Q + q] = ((red[k][q][0] + red[k][q][1]) + red[k][q][2]) + red[k][q][3];
    }
}

// One workgroup per (region blockIdx.x, frame blockIdx.y): the tiles' partials added in a fixed order, then the four figures.
__global__ __launch_bounds__(FM_THREADS) void frame_final_kernel(const double* __restrict__ partial, double* __restrict__ out,
                                                                 int tiles, int C, int M, int luma, double floor_rgb, double floor_y) {
    __shared__ double red[FM_Q][FM_THREADS / 64];
    const int tid = threadIdx.x, k = blockIdx.x, n = blockIdx.y;
    double v[FM_Q] = {0, 0, 0, 0, 0};
    for (int t = tid; t < tiles; t += FM_THREADS) {
        const double* p = partial + (((long long)n * tiles + t) * (M + 1) + k) * FM_Q;
#pragma unroll
        for (int q = 0; q < FM_Q; ++q) v[q] += p[q];
    }
#pragma unroll
    for (int q = 0; q < FM_Q; ++q) {
        for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_down(v[q], o);
        if ((tid & 63) == 0) red[q][tid >> 6] = v[q];
    }
    __syncthreads();
    if (tid == 0) {
        double s[FM_Q];
        for (int q = 0; q < FM_Q; ++q) s[q] = ((red[q][0] + red[q][1]) + red[q][2]) + red[q][3];
        double* o = out + ((long long)n * (M + 1) + k) * 4;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        const double msum = s[2];
        // utils._psnr_from / calc_psnr_and_ssim_cuda; an empty region divides by zero there and is NaN here
        const double mse = s[0] / (msum * C), msey = s[3] / msum;
        o[0] = msum == 0.0 ? nan : (mse == 0.0 ? floor_rgb : -20.0 * log10(sqrt(mse)));
        o[1] = msum == 0.0 ? nan : s[1] / (msum * C);
        o[2] = (msum == 0.0 || !luma) ? nan : (msey == 0.0 ? floor_y : -20.0 * log10(sqrt(msey)));
        o[3] = (msum == 0.0 || !luma) ? nan : s[4] / msum;
    }
}

long long frame_metrics_tiles(int H, int W) { return (((long long)W + SW - 1) / SW) * (((long long)H + SH - 1) / SH); }

// probe quadruples [N][FM_PROBE_BLOCKS][4] floats, then the tiles' partials [N][tiles][1 + M][FM_Q] doubles
size_t frame_metrics_workspace_bytes(int N, int M, int H, int W) {
    if (N < 1 || M < 0 || M > FM_MAX_MASKS || H < 1 || W < 1) return 0;
    return (size_t)N * FM_PROBE_BLOCKS * 4 * sizeof(float) + (size_t)N * frame_metrics_tiles(H, W) * (M + 1) * FM_Q * sizeof(double);
}

// sr, hr: [N,C,H,W]; masks: [N,M,H,W] bytes; out: [N,1+M,4] doubles.  The caller has checked the arguments and the workspace size.
int launch_frame_metrics(const float* sr, const float* hr, const uint8_t* masks, double* out, int N, int C, int M, int H, int W,
                         int luma, void* workspace, hipStream_t s) {
    SsimWin win;
    ssim_window(win);
    float* probe = (float*)workspace;
    double* partial = (double*)((char*)workspace + (size_t)N * FM_PROBE_BLOCKS * 4 * sizeof(float));
    const long long tiles = frame_metrics_tiles(H, W);
    const double px = (double)N * C * H * W, hw = (double)N * H * W;
    {
        ProfScope prof("frame_metrics_probe", s, px * 4.0, px * 2.0);
        frame_probe_kernel<<<dim3(FM_PROBE_BLOCKS, N), FM_THREADS, 0, s>>>(hr, probe, C, (long long)H * W, luma);
        CRFP_CHECK_LAUNCH();
    }
    {
        ProfScope prof("frame_metrics_sums", s, px * 8.0 + hw * M, (px + (luma ? hw : 0.0)) * 2.0 * 5 * 22);
        dim3 grid((unsigned)(((long long)W + SW - 1) / SW), (H + SH - 1) / SH, N);
        frame_sums_kernel<<<grid, FM_THREADS, 0, s>>>(sr, hr, masks, probe, partial, C, M, H, W, luma, win);
        CRFP_CHECK_LAUNCH();
    }
    const double inv = (1.0 / 255.0) * (1.0 / 255.0);
    const double floor_rgb = -20.0 * log10(sqrt(inv / ((double)C * H * W))), floor_y = -20.0 * log10(sqrt(inv / ((double)H * W)));
    ProfScope prof("frame_metrics_final", s, (double)N * tiles * (M + 1) * FM_Q * 8.0, 0.0);
    frame_final_kernel<<<dim3(M + 1, N), FM_THREADS, 0, s>>>(partial, out, (int)tiles, C, M, luma, floor_rgb, floor_y);
    CRFP_CHECK_LAUNCH();
    return 0;
}

}  // namespace crfp
