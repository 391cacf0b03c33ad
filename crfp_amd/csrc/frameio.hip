// 8-bit frame I/O around the engines' fp32 API tensors: what the reference does on the host in NumPy (dataset/reds.py:306,409 `astype(float32) /
// 255.`; :196-203 Ref = HR inside the window, 0 outside; test_video.py:396-410 y_only chroma merge, `(sr * 255.).clip(0., 255.)`, round, uint8, HWC,
// RGB -> BGR) as pure stream kernels, so that a host uploads an 8-bit LR frame, a fovea crop and one rectangle and downloads an 8-bit frame.
//
// Ingest is two launches.  frame_ingest_lr_kernel: lr_u8 [n,h,w,3] -> lr [n,3,h,w], lr = (float)byte / 255.0f with IEEE division (a multiplication
// by the reciprocal differs on 126 of the 256 codes).  frame_ingest_fovea_kernel: crop_u8 [n,fh,fw,3] and rects [n,4] (y, x, flags, 0) -> fv
// [n,3,H,W], mk [n,1,H,W]: with R = [y, y + fh) x [x, x + fw) intersected with the frame (gaze_clip, 64-bit; empty without the HAS_FOVEA bit),
// fv = crop / 255.0f and mk = 1 inside R, fv = +0 and mk = 0 outside.  blockIdx.z = frame, whose rectangle is read with uniform indices.  A thread
// loads crop bytes only for its pixels inside R, which also keeps every crop address inside the crop; everywhere else it stores zeros and issues
// no load.
// Export is one launch.  frame_export_kernel: sr [n,c,H,W] (c = 3, or c = 1 with chroma [n,3,H,W]) -> out_u8 [n,H,W,3],
// q(v) = (uint8)rintf(fminf(fmaxf(v * 255.0f, 0.0f), 255.0f)): round half to even, NaN -> 0.  c = 1 is test_video.py:100-127,401-402 in fp32, one
// rounding per operation (-ffp-contract=off): u, v of the chroma frame under the model's luma, back to RGB.
// VEC: a thread owns 4 consecutive pixels -- one 16-byte access per fp32 plane, three 4-byte accesses of interleaved bytes, one 4-byte mask store;
// the scalar form (sizes off a multiple of 4 or pointers off their alignment) owns one pixel.  Every output byte is written exactly once; no
// atomics, no LDS, nothing to initialise.
#include "frameio_px.h"
#include "rects.h"

namespace crfp {

// NPX pixels of interleaved bytes at `s` -> ch[c][i] = channel c (memory order) of pixel i, as a fraction of 255
template <int NPX>
__device__ __forceinline__ void io_load_px(const uint8_t* __restrict__ s, float (&ch)[3][NPX]) {
    if constexpr (NPX == 4) {
        const unsigned* s4 = reinterpret_cast<const unsigned*>(s);
        const unsigned w[3] = {s4[0], s4[1], s4[2]};
#pragma unroll
        for (int k = 0; k < 12; ++k) ch[k % 3][k / 3] = io_unit(io_byte(w, k));
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) ch[c][0] = io_unit(s[c]);
    }
}

// hw = h * w pixels per plane; VEC: hw % 4 == 0, src 4-byte and dst 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(256) void frame_ingest_lr_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, long long hw, int bgr) {
    constexpr int NPX = VEC ? 4 : 1;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= hw / NPX) return;
    const long long p = t * NPX, n = blockIdx.z;
    float ch[3][NPX];
    io_load_px<NPX>(src + (n * hw + p) * 3, ch);
    float* d = dst + n * 3 * hw + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) io_store_plane<NPX>(d + (bgr ? 2 - c : c) * hw, ch[c]);
}

// VEC: W % 4 == 0, fv 16-byte and mk 4-byte aligned
template <bool VEC>
__global__ __launch_bounds__(256) void frame_ingest_fovea_kernel(const uint8_t* __restrict__ crop, const int* __restrict__ rects,
                                                                 float* __restrict__ fv, uint8_t* __restrict__ mk, int fh, int fw, int H, int W,
                                                                 int bgr) {
    constexpr int NPX = VEC ? 4 : 1;
    const long long n = blockIdx.z;
    const int* __restrict__ q = rects + n * CRFP_IO_RECT_INTS;
    const int oy = q[0], ox = q[1];
    const GazeRect R = gaze_clip(oy, ox, fh, fw, 0, q[2] & CRFP_IO_HAS_FOVEA, H, W);
    const long long HW = (long long)H * W;
    const int wq = VEC ? W / 4 : W;                                          // threads per image row
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)H * wq) return;
    const int y = (int)(t / wq), x = (int)(t - (long long)y * wq) * NPX;
    const unsigned in = gaze_bits<NPX>(R, y, x);
    const long long p = (long long)y * W + x;
    float ch[3][NPX];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < NPX; ++i) ch[c][i] = 0.0f;
    if (in) {   // a pixel inside R has 0 <= y - oy < fh and 0 <= x + i - ox < fw
        const uint8_t* row = crop + ((n * fh + ((long long)y - oy)) * fw + ((long long)x - ox)) * 3;
#pragma unroll
        for (int i = 0; i < NPX; ++i)
            if (in >> i & 1u) {
#pragma unroll
                for (int c = 0; c < 3; ++c) ch[c][i] = io_unit(row[3 * i + c]);
            }
    }
    float* d = fv + n * 3 * HW + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) io_store_plane<NPX>(d + (bgr ? 2 - c : c) * HW, ch[c]);
    if constexpr (VEC) *reinterpret_cast<unsigned*>(mk + n * HW + p) = gaze_bytes(in);
    else mk[n * HW + p] = (uint8_t)in;
}

// hw = H * W pixels per plane; VEC: hw % 4 == 0, sr / chroma 16-byte and out 4-byte aligned
template <bool VEC>
__global__ __launch_bounds__(256) void frame_export_kernel(const float* __restrict__ sr, const float* __restrict__ chroma, uint8_t* __restrict__ out,
                                                           int C, long long hw, int bgr) {
    constexpr int NPX = VEC ? 4 : 1;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= hw / NPX) return;
    const long long p = t * NPX, n = blockIdx.z;
    const float* a = sr + n * C * hw + p;
    float ch[3][NPX];   // R, G, B
    if (chroma) {       // c = 1: sr is the luma, u and v come from the chroma frame
        const float* b = chroma + n * 3 * hw + p;
        float yy[NPX], r[NPX], g[NPX], bl[NPX];
        io_load_plane<NPX>(a, yy); io_load_plane<NPX>(b, r); io_load_plane<NPX>(b + hw, g); io_load_plane<NPX>(b + 2 * hw, bl);
#pragma unroll
        for (int i = 0; i < NPX; ++i) {
            io_merge(yy[i], r[i], g[i], bl[i], ch[0][i], ch[1][i], ch[2][i]);
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) io_load_plane<NPX>(a + c * hw, ch[c]);
    }
    io_store_px<NPX>(out + (n * hw + p) * 3, ch, bgr);
}

// grid of one thread per NPX pixels of `threads` per frame; false (with the error set) beyond the launch grid
static bool io_grid(const char* what, int N, long long threads, dim3* grid) {
    const long long blocks = (threads + 255) / 256;
    if (N > 65535 || blocks > 0x7fffffffLL) {
        set_error("%s: more than 65535 frames per call or a frame beyond the launch grid", what);
        return false;
    }
    *grid = dim3((unsigned)blocks, 1, N);
    return true;
}

// The caller has checked the arguments (api.hip).  lr_u8 / lr: both given or both null; crop_u8 / rects / fv / mk: all given or all null.
int launch_frame_ingest(const uint8_t* lr_u8, const uint8_t* crop_u8, const int* rects, float* lr, float* fv, uint8_t* mk, int N, int h, int w,
                        int fh, int fw, int H, int W, int bgr, hipStream_t s) {
    const long long hw = (long long)h * w, HW = (long long)H * W;
    const bool vec_lr = hw % 4 == 0 && (uintptr_t)lr_u8 % 4 == 0 && (uintptr_t)lr % 16 == 0;
    const bool vec_fv = W % 4 == 0 && (uintptr_t)fv % 16 == 0 && (uintptr_t)mk % 4 == 0;
    dim3 grid_lr, grid_fv;
    if (lr && !io_grid("frame_ingest", N, vec_lr ? hw / 4 : hw, &grid_lr)) return CRFP_E_UNSUPPORTED;
    if (fv && !io_grid("frame_ingest", N, vec_fv ? HW / 4 : HW, &grid_fv)) return CRFP_E_UNSUPPORTED;
    if (lr) {
        ProfScope prof("frame_ingest_lr", s, (double)N * hw * 15.0, 0.0);
        if (vec_lr) frame_ingest_lr_kernel<true><<<grid_lr, 256, 0, s>>>(lr_u8, lr, hw, bgr);
        else frame_ingest_lr_kernel<false><<<grid_lr, 256, 0, s>>>(lr_u8, lr, hw, bgr);
        CRFP_CHECK_LAUNCH();
    }
    if (fv) {
        ProfScope prof("frame_ingest_fovea", s, (double)N * (HW * 13.0 + (double)fh * fw * 3.0), 0.0);
        if (vec_fv) frame_ingest_fovea_kernel<true><<<grid_fv, 256, 0, s>>>(crop_u8, rects, fv, mk, fh, fw, H, W, bgr);
        else frame_ingest_fovea_kernel<false><<<grid_fv, 256, 0, s>>>(crop_u8, rects, fv, mk, fh, fw, H, W, bgr);
        CRFP_CHECK_LAUNCH();
    }
    return 0;
}

// The caller has checked the arguments (api.hip).  chroma: given exactly when C == 1.
int launch_frame_export(const float* sr, const float* chroma, uint8_t* out_u8, int N, int C, int H, int W, int bgr, hipStream_t s) {
    const long long hw = (long long)H * W;
    const bool vec = hw % 4 == 0 && ((uintptr_t)sr | (uintptr_t)chroma) % 16 == 0 && (uintptr_t)out_u8 % 4 == 0;
    dim3 grid;
    if (!io_grid("frame_export", N, vec ? hw / 4 : hw, &grid)) return CRFP_E_UNSUPPORTED;
    ProfScope prof("frame_export", s, (double)N * hw * (4.0 * (chroma ? 4 : 3) + 3.0), 0.0);
    if (vec) frame_export_kernel<true><<<grid, 256, 0, s>>>(sr, chroma, out_u8, C, hw, bgr);
    else frame_export_kernel<false><<<grid, 256, 0, s>>>(sr, chroma, out_u8, C, hw, bgr);
    CRFP_CHECK_LAUNCH();
    return 0;
}

}  // namespace crfp
