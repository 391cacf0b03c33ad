// The gaze rig's per-frame inputs from rectangles: one streaming writer instead of the rig's host-built composition (reference
// test_video.py:335-358,371-375: zeros + slice writes, ten 3x3 ones convolutions with a clamp, logical ops, the three-frame history).
//
// Nothing of a frame's masks depends on data: every one is a function of at most four rectangles -- this frame's fovea window and the
// three previous ones -- and of the regional box.  Ten (3x3 ones conv, zero padding, clamp) passes over ONE rectangle grow it by 10
// pixels on every side, clipped to the frame.  With R_e = entry e's rectangle intersected with the frame, G_e = the rectangle grown by
// `dilate` on all four sides intersected with the frame (both empty when the entry does not exist or has h < 1 or w < 1):
//   fovea = p in R_0;  mk = bit1_0 and p in R_0;  outskirt = p in G_0 and not mk;
//   past  = OR over e = 1..3 of (p in G_e and not (bit1_e and p in R_e));  fg = p in box;  fv = mk ? gt : +0.
// gaze_prep_kernel<VEC>: blockIdx.z = batch item, whose row of CRFP_GAZE_ROW_INTS ints is read with uniform indices, so the clipped
// rectangles live in scalar registers.  VEC: a thread owns 4 consecutive pixels of a row -- one 16-byte store per fv channel, one
// 4-byte store per mask plane -- and loads gt only when its four pixels touch the mk rectangle; everywhere else it stores zeros and
// issues no load.  The scalar form (W % 4 != 0 or a pointer off 16 bytes) owns one pixel.  Every output byte is written exactly once;
// no atomics, no LDS, nothing to initialise.  Every rectangle is intersected with the frame in 64-bit arithmetic before use, so no
// row content can move an address outside the planes.
#include "rects.h"

namespace crfp {

template <bool VEC>
__global__ __launch_bounds__(256) void gaze_prep_kernel(const float* __restrict__ gt, const int* __restrict__ rows, float* __restrict__ fv,
                                                        uint8_t* __restrict__ mk, uint8_t* __restrict__ regions, uint8_t* __restrict__ fg,
                                                        int C, int H, int W, int dilate) {
    constexpr int NPX = VEC ? 4 : 1;
    const int n = blockIdx.z;
    const int* __restrict__ row = rows + (long long)n * CRFP_GAZE_ROW_INTS;
    const GazeRect box{max(min(row[0], H), 0), max(min(row[1], H), 0), max(min(row[2], W), 0), max(min(row[3], W), 0)};   // bounds, not sizes
    GazeRect R[4], G[4];
    bool counts[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int* q = row + 4 + 5 * e;
        const int flags = q[4];
        R[e] = gaze_clip(q[0], q[1], q[2], q[3], 0, flags & 1, H, W);
        G[e] = gaze_clip(q[0], q[1], q[2], q[3], dilate, flags & 1, H, W);
        counts[e] = (flags & 2) != 0;
    }
    const long long HW = (long long)H * W;
    const int wq = VEC ? W / 4 : W;                                          // threads per image row
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)H * wq) return;
    const int y = (int)(t / wq), x = (int)(t - (long long)y * wq) * NPX;
    const unsigned fovea = gaze_bits<NPX>(R[0], y, x);
    const unsigned mkb = counts[0] ? fovea : 0u;
    const unsigned outskirt = gaze_bits<NPX>(G[0], y, x) & ~mkb;
    unsigned past = 0;
#pragma unroll
    for (int e = 1; e < 4; ++e) past |= gaze_bits<NPX>(G[e], y, x) & ~(counts[e] ? gaze_bits<NPX>(R[e], y, x) : 0u);
    const unsigned fgb = gaze_bits<NPX>(box, y, x);
    const long long p = (long long)y * W + x;
    uint8_t* rg = regions + (long long)n * 3 * HW + p;
    if (VEC) {
        *reinterpret_cast<unsigned*>(mk + (long long)n * HW + p) = gaze_bytes(mkb);
        *reinterpret_cast<unsigned*>(rg) = gaze_bytes(fovea);
        *reinterpret_cast<unsigned*>(rg + HW) = gaze_bytes(outskirt);
        *reinterpret_cast<unsigned*>(rg + 2 * HW) = gaze_bytes(past);
        *reinterpret_cast<unsigned*>(fg + (long long)n * HW + p) = gaze_bytes(fgb);
    } else {
        mk[(long long)n * HW + p] = (uint8_t)mkb;
        rg[0] = (uint8_t)fovea; rg[HW] = (uint8_t)outskirt; rg[2 * HW] = (uint8_t)past;
        fg[(long long)n * HW + p] = (uint8_t)fgb;
    }
    if (!fv) return;
    const long long base = (long long)n * C * HW + p;
    for (int c = 0; c < C; ++c) {
        const long long o = base + (long long)c * HW;
        if (VEC) {
            cf32x4 v = cf32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (mkb) {
                const cf32x4 g = *reinterpret_cast<const cf32x4*>(gt + o);
                v = cf32x4{mkb & 1u ? g.x : 0.0f, mkb & 2u ? g.y : 0.0f, mkb & 4u ? g.z : 0.0f, mkb & 8u ? g.w : 0.0f};
            }
            *reinterpret_cast<cf32x4*>(fv + o) = v;
        } else {
            fv[o] = mkb ? gt[o] : 0.0f;
        }
    }
}

// The caller has checked the arguments (api.hip).  gt / fv: both given or both null (masks only).
int launch_gaze_prep(const float* gt, const int* rows, float* fv, uint8_t* mk, uint8_t* regions, uint8_t* fg, int N, int C, int H, int W,
                     int dilate, hipStream_t s) {
    const uintptr_t ptrs = (uintptr_t)gt | (uintptr_t)fv | (uintptr_t)mk | (uintptr_t)regions | (uintptr_t)fg;
    const bool vec = W % 4 == 0 && ptrs % 16 == 0;
    const long long threads = (long long)H * (vec ? W / 4 : W), blocks = (threads + 255) / 256;
    if (N > 65535 || blocks > 0x7fffffffLL) {
        set_error("gaze_prep: more than 65535 frames per call or a frame beyond the launch grid");
        return CRFP_E_UNSUPPORTED;
    }
    const double hw = (double)N * H * W;
    ProfScope prof("gaze_prep", s, hw * 5.0 + (fv ? hw * C * 4.0 : 0.0), 0.0);
    const dim3 grid((unsigned)blocks, 1, N);
    if (vec) gaze_prep_kernel<true><<<grid, 256, 0, s>>>(gt, rows, fv, mk, regions, fg, C, H, W, dilate);
    else gaze_prep_kernel<false><<<grid, 256, 0, s>>>(gt, rows, fv, mk, regions, fg, C, H, W, dilate);
    CRFP_CHECK_LAUNCH();
    return 0;
}

}  // namespace crfp
