// PIL's 8-bit bicubic resize (Image.resize(..., BICUBIC) on an 8-bit RGB image; libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc,
// ImagingResampleHorizontal_8bpc / Vertical_8bpc), byte for byte: the reference's baseline frames and y_only chroma frames (test_video.py:241,
// 396-402; dataset/reds.py:281,394,480; trainer.py:331-335).  The arithmetic on pixels is integer -- 22-bit fixed-point taps, an 8-bit
// intermediate image, x before y -- and only the tap tables need IEEE double, so a kernel can reproduce it exactly.
//
// Tables.  bicubic_taps_at is the one function that writes an output index' first source index, tap count and fixed-point taps; the host entry
// point crfp_bicubic_taps and bicubic_taps_kernel (one thread per output column and row, both axes in one launch, into the caller's workspace)
// both run it.  Built with -ffp-contract=off; plain `/`, which is the correctly rounded division for doubles on both sides.
// Two-pass path, any geometry: bicubic_rows_kernel src [N,h,w,3] -> tmp [N,h,W,3] in the workspace, bicubic_cols_kernel tmp -> the epilogue; one
// thread per output pixel.
// Fused path, H >= h and W >= w (then ksize = 5 and at most 4 taps count): bicubic_up_kernel, one workgroup per 32 x 64 output tile.  The
// source columns of the tile are [xmin(first), xmin(last) + cnt(last)) -- at most tile + 3 of them, because xmin and xmin + cnt do not
// decrease with the index and the centres of the tile's ends lie less than tile - 1 sources apart -- and likewise the rows: a patch of at most
// 35 x 67 pixels (5 x 11 at x8).  The workgroup stages the patch in LDS, writes its x-resampled rows [patch rows, 64] as bytes to LDS, and a
// thread then resamples 4 pixels (1 in the one-pixel form) along y from three 4-byte LDS reads per tap row and stores them through its
// epilogue.  16.6 KB of LDS per workgroup, one __shared__ object.
// Epilogues (bc_store): bytes [N,H,W,3]; fp32 planes [N,3,H,W] = io_unit(byte); the y_only merge: io_merge on io_unit of the byte triple under
// a luma plane, io_q -- frame_export_kernel's c = 1 branch on a chroma frame that is never written.  The BGR flag names the order of the 8-bit
// side: bytes in and bytes out swap alike, so a byte-to-byte resize does not depend on it.
// Every output byte is written exactly once; no atomics; all global indices are 64-bit.
#include "frameio_px.h"

#include <math.h>

namespace crfp {

constexpr int BC_BITS = 22;                                 // PRECISION_BITS = 32 - 8 - 2
constexpr int BC_TH = 32, BC_TW = 64;                       // output tile of a workgroup
constexpr int BC_PH = BC_TH + 4, BC_PW = BC_TW + 4;         // its patch (<= tile + 3 per axis; one spare keeps the rows of `in` 4-byte sized)
constexpr int BC_UP_KSIZE = 5, BC_UP_TAPS = 4;              // an axis that does not shrink: support 2, ksize 5, cnt <= 4

__host__ __device__ inline double bc_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

__host__ __device__ inline long long bc_ksize(int in, int out) {
    const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale;
    return (long long)ceil(2.0 * fs) * 2 + 1;
}

// bounds[0] = xmin, bounds[1] = cnt, taps[0 .. ksize): the fixed-point taps of output index xx, zero from cnt on.  The two conversions to int
// are guarded where C leaves them undefined (a negative start is 0 after the clamp anyway; an end at or beyond `in` is `in`).
__host__ __device__ inline void bicubic_taps_at(int in, int out, int xx, int ksize, int* bounds, int* taps) {
    const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale, support = 2.0 * fs, ss = 1.0 / fs;
    const double center = (xx + 0.5) * scale;
    const double lo = center - support + 0.5, hi = center + support + 0.5;
    const int xmin = lo < 1.0 ? 0 : (int)lo;
    const int xmax = hi >= (double)in ? in : (int)hi;
    int cnt = xmax - xmin;
    cnt = cnt < 0 ? 0 : cnt > ksize ? ksize : cnt;
    double ww = 0.0;
    for (int x = 0; x < cnt; ++x) ww += bc_filter((x + xmin - center + 0.5) * ss);
    for (int x = 0; x < cnt; ++x) {
        double w = bc_filter((x + xmin - center + 0.5) * ss);   // the same value as in the sum: nothing to keep per tap
        if (ww != 0.0) w /= ww;
        taps[x] = w < 0 ? (int)(-0.5 + w * (1 << BC_BITS)) : (int)(0.5 + w * (1 << BC_BITS));
    }
    for (int x = cnt; x < ksize; ++x) taps[x] = 0;
    bounds[0] = xmin;
    bounds[1] = cnt;
}

long long bicubic_ksize(int in, int out) { return bc_ksize(in, out); }

void bicubic_taps_host(int in, int out, int ksize, int* bounds, int* taps) {
    for (int xx = 0; xx < out; ++xx) bicubic_taps_at(in, out, xx, ksize, bounds + 2 * (size_t)xx, taps + (size_t)ksize * xx);
}

// threads [0, W): the columns' tables; [W, W + H): the rows'
__global__ __launch_bounds__(256) void bicubic_taps_kernel(int* __restrict__ bx, int* __restrict__ kx, int* __restrict__ by, int* __restrict__ ky,
                                                           int h, int w, int H, int W, int ksx, int ksy) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < W) {
        bicubic_taps_at(w, W, (int)t, ksx, bx + 2 * t, kx + t * ksx);
    } else if (t < (long long)W + H) {
        const long long y = t - W;
        bicubic_taps_at(h, H, (int)y, ksy, by + 2 * y, ky + y * ksy);
    }
}

// clamp(acc >> 22, 0, 255), written as a clamp of acc to [0, 2^30) and a logical shift.  The shift-then-clamp form is what hipcc (ROCm 7.2)
// turns into gfx950's v_ashr_pk_u8_i32 when two results are packed into bytes, and it takes the instruction's upper 16 destination bits for
// zero; on the MI355X they keep the register's old contents, which were then OR-ed into bytes 2 and 3 of every stored word.
__device__ __forceinline__ unsigned bc_clip(int acc) { return (unsigned)min(max(acc, 0), (256 << BC_BITS) - 1) >> BC_BITS; }

// px[c][i] = byte c (memory order of the 8-bit side) of pixel i -> NPX pixels at pixel index p (= Y * W + X) of frame n.  NPX == 4: the
// launcher has checked W % 4 == 0 and the pointers' alignment, and X % 4 == 0.
template <int EPI, int NPX>
__device__ __forceinline__ void bc_store(const unsigned (&px)[3][NPX], void* __restrict__ dst, const float* __restrict__ luma, long long n,
                                         long long HW, long long p, int bgr) {
    if constexpr (EPI == BC_EPI_U8) {
        uint8_t* o = static_cast<uint8_t*>(dst) + (n * HW + p) * 3;
        if constexpr (NPX == 4) {
            unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 12; ++k) w[k / 4] |= px[k % 3][k / 3] << 8 * (k % 4);
            unsigned* o4 = reinterpret_cast<unsigned*>(o);
            o4[0] = w[0]; o4[1] = w[1]; o4[2] = w[2];
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = (uint8_t)px[c][0];
        }
    } else if constexpr (EPI == BC_EPI_F32) {
        float* d = static_cast<float*>(dst) + n * 3 * HW + p;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[NPX];
#pragma unroll
            for (int i = 0; i < NPX; ++i) v[i] = io_unit(px[c][i]);
            io_store_plane<NPX>(d + (bgr ? 2 - c : c) * HW, v);
        }
    } else {
        float yy[NPX], ch[3][NPX];
        io_load_plane<NPX>(luma + n * HW + p, yy);
#pragma unroll
        for (int i = 0; i < NPX; ++i)
            io_merge(yy[i], io_unit(px[bgr ? 2 : 0][i]), io_unit(px[1][i]), io_unit(px[bgr ? 0 : 2][i]), ch[0][i], ch[1][i], ch[2][i]);
        io_store_px<NPX>(static_cast<uint8_t*>(dst) + (n * HW + p) * 3, ch, bgr);
    }
}

// ---------------------------------------------------------------------------------------------------------------- two passes
// src [N,h,w,3] -> tmp [N,h,W,3]; hW = h * W threads per frame
__global__ __launch_bounds__(256) void bicubic_rows_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ tmp, const int* __restrict__ bx,
                                                           const int* __restrict__ kx, int ksx, int w, int W, long long hW) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= hW) return;
    const long long n = blockIdx.z, y = t / W, hh = hW / W;
    const int X = (int)(t - y * W);
    const int x0 = bx[2 * X], cnt = bx[2 * X + 1];
    const int* __restrict__ k = kx + (long long)X * ksx;
    const uint8_t* __restrict__ s = src + ((n * hh + y) * w + x0) * 3;   // x0 + cnt <= w
    int acc[3] = {1 << (BC_BITS - 1), 1 << (BC_BITS - 1), 1 << (BC_BITS - 1)};
    for (int i = 0; i < cnt; ++i) {
        const int kk = k[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += (int)s[3 * i + c] * kk;
    }
    uint8_t* d = tmp + (n * hW + t) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = (uint8_t)bc_clip(acc[c]);
}

// tmp [N,h,W,3] -> the epilogue; HW = H * W threads per frame
template <int EPI>
__global__ __launch_bounds__(256) void bicubic_cols_kernel(const uint8_t* __restrict__ tmp, void* __restrict__ dst, const int* __restrict__ by,
                                                           const int* __restrict__ ky, int ksy, int h, int W, long long HW, int bgr) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= HW) return;
    const long long n = blockIdx.z, Y = t / W, X = t - Y * W;
    const int y0 = by[2 * Y], cnt = by[2 * Y + 1];
    const int* __restrict__ k = ky + Y * ksy;
    const uint8_t* __restrict__ s = tmp + ((n * h + y0) * W + X) * 3;      // y0 + cnt <= h
    int acc[3] = {1 << (BC_BITS - 1), 1 << (BC_BITS - 1), 1 << (BC_BITS - 1)};
    for (int i = 0; i < cnt; ++i) {
        const int kk = k[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += (int)s[(long long)i * W * 3 + c] * kk;
    }
    const unsigned px[3][1] = {{bc_clip(acc[0])}, {bc_clip(acc[1])}, {bc_clip(acc[2])}};
    bc_store<EPI, 1>(px, dst, nullptr, n, HW, t, bgr);
}

// ---------------------------------------------------------------------------------------------------------------- fused, H >= h and W >= w
struct BcTile {
    int kx[BC_TW][BC_UP_TAPS], ky[BC_TH][BC_UP_TAPS];   // taps of the tile's columns and rows, zero from cnt on
    int x0[BC_TW], xn[BC_TW], y0[BC_TH], yn[BC_TH];     // first source index relative to the patch, and cnt
    uint8_t mid[BC_PH][BC_TW * 3];                      // the patch's rows resampled along x; rows are 192 bytes, so a 4-pixel group is 4-byte aligned
    uint8_t in[BC_PH][BC_PW * 3];                       // the patch
};

template <int EPI, bool VEC>
__global__ __launch_bounds__(256) void bicubic_up_kernel(const uint8_t* __restrict__ src, void* __restrict__ dst, const float* __restrict__ luma,
                                                         const int* __restrict__ bx, const int* __restrict__ kx, const int* __restrict__ by,
                                                         const int* __restrict__ ky, int h, int w, int H, int W, int bgr) {
    constexpr int NPX = VEC ? 4 : 1;
    __shared__ BcTile T;
    const int tid = threadIdx.x;
    const int X0 = blockIdx.x * BC_TW, Y0 = blockIdx.y * BC_TH;
    const int tw = min(BC_TW, W - X0), th = min(BC_TH, H - Y0);
    const long long n = blockIdx.z;
    // the patch: uniform over the workgroup.  The min() never cuts (see the head of the file); it keeps every LDS index inside its array
    const int px0 = bx[2 * X0], py0 = by[2 * Y0];
    const int pw = min(bx[2 * (X0 + tw - 1)] + bx[2 * (X0 + tw - 1) + 1] - px0, BC_PW);
    const int ph = min(by[2 * (Y0 + th - 1)] + by[2 * (Y0 + th - 1) + 1] - py0, BC_PH);
    if (tid < tw) {
        const int X = X0 + tid, cnt = min(bx[2 * X + 1], BC_UP_TAPS);
        T.x0[tid] = bx[2 * X] - px0;
        T.xn[tid] = cnt;
#pragma unroll
        for (int k = 0; k < BC_UP_TAPS; ++k) T.kx[tid][k] = k < cnt ? kx[(long long)X * BC_UP_KSIZE + k] : 0;
    } else if (tid >= BC_TW && tid - BC_TW < th) {
        const int r = tid - BC_TW, Y = Y0 + r, cnt = min(by[2 * Y + 1], BC_UP_TAPS);
        T.y0[r] = by[2 * Y] - py0;
        T.yn[r] = cnt;
#pragma unroll
        for (int k = 0; k < BC_UP_TAPS; ++k) T.ky[r][k] = k < cnt ? ky[(long long)Y * BC_UP_KSIZE + k] : 0;
    }
    const int pwb = pw * 3;
    for (int i = tid; i < ph * pwb; i += 256) {   // rows [py0, py0 + ph) <= h, byte columns [3 px0, 3 px0 + pwb) <= 3 w
        const int r = i / pwb, j = i - r * pwb;
        T.in[r][j] = src[((n * h + py0 + r) * w + px0) * 3 + j];
    }
    __syncthreads();
    for (int i = tid; i < ph * tw; i += 256) {
        const int r = i / tw, c = i - r * tw;
        const uint8_t* s = &T.in[r][T.x0[c] * 3];   // x0 + cnt <= pw
        const int cnt = T.xn[c];
        int acc[3] = {1 << (BC_BITS - 1), 1 << (BC_BITS - 1), 1 << (BC_BITS - 1)};
        for (int k = 0; k < cnt; ++k) {
            const int kk = T.kx[c][k];
#pragma unroll
            for (int b = 0; b < 3; ++b) acc[b] += (int)s[3 * k + b] * kk;
        }
#pragma unroll
        for (int b = 0; b < 3; ++b) T.mid[r][3 * c + b] = (uint8_t)bc_clip(acc[b]);
    }
    __syncthreads();
    const int tq = tw / NPX;   // VEC: W % 4 == 0, so tw % 4 == 0
    const long long HW = (long long)H * W;
    for (int i = tid; i < th * tq; i += 256) {
        const int r = i / tq, c = (i - r * tq) * NPX;
        const int y0 = T.y0[r], cnt = T.yn[r];   // y0 + cnt <= ph
        int acc[3 * NPX];
#pragma unroll
        for (int b = 0; b < 3 * NPX; ++b) acc[b] = 1 << (BC_BITS - 1);
        for (int k = 0; k < cnt; ++k) {
            const int kk = T.ky[r][k];
            if constexpr (VEC) {
                const unsigned* m = reinterpret_cast<const unsigned*>(&T.mid[y0 + k][3 * c]);
                const unsigned q[3] = {m[0], m[1], m[2]};
#pragma unroll
                for (int b = 0; b < 12; ++b) acc[b] += (int)io_byte(q, b) * kk;
            } else {
#pragma unroll
                for (int b = 0; b < 3; ++b) acc[b] += (int)T.mid[y0 + k][3 * c + b] * kk;
            }
        }
        unsigned px[3][NPX];
#pragma unroll
        for (int b = 0; b < 3 * NPX; ++b) px[b % 3][b / 3] = bc_clip(acc[b]);
        bc_store<EPI, NPX>(px, dst, luma, n, HW, (long long)(Y0 + r) * W + X0 + c, bgr);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
namespace {
struct BcLayout {
    int ksx, ksy;
    size_t bx, kx, by, ky, tmp, total;   // byte offsets into the workspace
};

// false: sizes < 1, or an axis' table beyond an int
bool bc_layout(int N, int h, int w, int H, int W, BcLayout* L) {
    if (N < 1 || h < 1 || w < 1 || H < 1 || W < 1) return false;
    const long long ksx = bc_ksize(w, W), ksy = bc_ksize(h, H);
    if (ksx * W > 0x7fffffffLL || ksy * H > 0x7fffffffLL) return false;
    L->ksx = (int)ksx;
    L->ksy = (int)ksy;
    L->bx = 0;
    L->kx = L->bx + 8 * (size_t)W;
    L->by = L->kx + 4 * (size_t)ksx * W;
    L->ky = L->by + 8 * (size_t)H;
    L->tmp = align_up(L->ky + 4 * (size_t)ksy * H, 16);
    L->total = L->tmp + (size_t)N * h * W * 3;
    return true;
}

bool bc_fits_grid(int N, int h, int H, int W) {
    const long long rows = ((long long)h * W + 255) / 256, cols = ((long long)H * W + 255) / 256;
    return N <= 65535 && rows <= 0x7fffffffLL && cols <= 0x7fffffffLL && (H + BC_TH - 1) / BC_TH <= 65535;
}
}  // namespace

size_t bicubic_workspace_bytes(int N, int h, int w, int H, int W) {
    BcLayout L;
    return bc_layout(N, h, w, H, W, &L) && bc_fits_grid(N, h, H, W) ? L.total : 0;
}

template <int EPI>
static void launch_bicubic_up(bool vec, dim3 grid, hipStream_t s, const uint8_t* src, void* dst, const float* luma, const int* bx, const int* kx,
                              const int* by, const int* ky, int h, int w, int H, int W, int bgr) {
    if (vec) bicubic_up_kernel<EPI, true><<<grid, 256, 0, s>>>(src, dst, luma, bx, kx, by, ky, h, w, H, W, bgr);
    else bicubic_up_kernel<EPI, false><<<grid, 256, 0, s>>>(src, dst, luma, bx, kx, by, ky, h, w, H, W, bgr);
}

// The caller has checked the arguments and the workspace's size (api.hip).  luma: given exactly when epi == BC_EPI_MERGE.
int launch_bicubic(const uint8_t* src, void* dst, const float* luma, int N, int h, int w, int H, int W, int epi, int bgr, int two_pass,
                   void* workspace, hipStream_t s) {
    BcLayout L;
    if (!bc_layout(N, h, w, H, W, &L) || !bc_fits_grid(N, h, H, W)) {
        set_error("resize_bicubic: more than 65535 frames per call, tap tables beyond an int or a frame beyond the launch grid");
        return CRFP_E_UNSUPPORTED;
    }
    const bool fused = !two_pass && H >= h && W >= w;
    if (epi == BC_EPI_MERGE && !fused) {
        set_error("frame_export_y_bicubic: the merge runs on the fused path only, which needs H >= h and W >= w (got %d x %d -> %d x %d)", h, w, H, W);
        return CRFP_E_UNSUPPORTED;
    }
    char* ws = static_cast<char*>(workspace);
    int* bx = reinterpret_cast<int*>(ws + L.bx);
    int* kx = reinterpret_cast<int*>(ws + L.kx);
    int* by = reinterpret_cast<int*>(ws + L.by);
    int* ky = reinterpret_cast<int*>(ws + L.ky);
    const long long HW = (long long)H * W, hW = (long long)h * W;
    {
        ProfScope prof("bicubic_taps", s, 4.0 * ((2.0 + L.ksx) * W + (2.0 + L.ksy) * H), 0.0);
        bicubic_taps_kernel<<<dim3((unsigned)(((long long)W + H + 255) / 256)), 256, 0, s>>>(bx, kx, by, ky, h, w, H, W, L.ksx, L.ksy);
        CRFP_CHECK_LAUNCH();
    }
    const double out_bytes = (double)N * HW * (epi == BC_EPI_F32 ? 12.0 : epi == BC_EPI_MERGE ? 7.0 : 3.0);
    if (fused) {
        // the 4-pixel form: rows start on a 4-pixel boundary and the pointers carry the alignment launch_frame_export asks for
        const bool vec = W % 4 == 0 && (epi == BC_EPI_F32 ? (uintptr_t)dst % 16 == 0 : (uintptr_t)dst % 4 == 0) && (uintptr_t)luma % 16 == 0;
        const dim3 grid((unsigned)((W + BC_TW - 1) / BC_TW), (unsigned)((H + BC_TH - 1) / BC_TH), (unsigned)N);
        ProfScope prof("bicubic_up", s, out_bytes + (double)N * h * w * 3.0, 0.0);
        if (epi == BC_EPI_U8) launch_bicubic_up<BC_EPI_U8>(vec, grid, s, src, dst, luma, bx, kx, by, ky, h, w, H, W, bgr);
        else if (epi == BC_EPI_F32) launch_bicubic_up<BC_EPI_F32>(vec, grid, s, src, dst, luma, bx, kx, by, ky, h, w, H, W, bgr);
        else launch_bicubic_up<BC_EPI_MERGE>(vec, grid, s, src, dst, luma, bx, kx, by, ky, h, w, H, W, bgr);
        CRFP_CHECK_LAUNCH();
        return 0;
    }
    uint8_t* tmp = reinterpret_cast<uint8_t*>(ws + L.tmp);
    {
        ProfScope prof("bicubic_rows", s, (double)N * 3.0 * ((double)h * w + (double)hW), 0.0);
        bicubic_rows_kernel<<<dim3((unsigned)((hW + 255) / 256), 1, (unsigned)N), 256, 0, s>>>(src, tmp, bx, kx, L.ksx, w, W, hW);
        CRFP_CHECK_LAUNCH();
    }
    {
        ProfScope prof("bicubic_cols", s, out_bytes + (double)N * hW * 3.0, 0.0);
        const dim3 grid((unsigned)((HW + 255) / 256), 1, (unsigned)N);
        if (epi == BC_EPI_U8) bicubic_cols_kernel<BC_EPI_U8><<<grid, 256, 0, s>>>(tmp, dst, by, ky, L.ksy, h, W, HW, bgr);
        else bicubic_cols_kernel<BC_EPI_F32><<<grid, 256, 0, s>>>(tmp, dst, by, ky, L.ksy, h, W, HW, bgr);
        CRFP_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace crfp
