// Rectangles against a frame, shared by the stream kernels that rasterise them (gaze.hip, frameio.hip).  Every rectangle is intersected with the
// frame in 64-bit arithmetic before use, so no origin or size a caller passes can move an address outside the planes.
#pragma once
#include "crfp_common.h"

namespace crfp {

struct GazeRect { int y0, y1, x0, x1; };   // half-open, inside the frame; empty when y0 >= y1 or x0 >= x1

// [y - grow, y + h + grow) x [x - grow, x + w + grow) intersected with the frame
__device__ __forceinline__ GazeRect gaze_clip(int y, int x, int h, int w, int grow, bool on, int H, int W) {
    if (!on || h < 1 || w < 1) return GazeRect{0, 0, 0, 0};
    const long long y0 = (long long)y - grow, y1 = (long long)y + h + grow, x0 = (long long)x - grow, x1 = (long long)x + w + grow;
    GazeRect r;
    r.y0 = (int)max(min(y0, (long long)H), 0LL); r.y1 = (int)max(min(y1, (long long)H), 0LL);
    r.x0 = (int)max(min(x0, (long long)W), 0LL); r.x1 = (int)max(min(x1, (long long)W), 0LL);
    return r;
}

// bit i (i < NPX) = pixel (y, x + i) lies in r
template <int NPX>
__device__ __forceinline__ unsigned gaze_bits(const GazeRect& r, int y, int x) {
    if (y < r.y0 || y >= r.y1) return 0u;
    unsigned b = 0;
#pragma unroll
    for (int i = 0; i < NPX; ++i) b |= (x + i >= r.x0 && x + i < r.x1) ? 1u << i : 0u;
    return b;
}

// 4 pixel bits -> 4 bytes of 0 / 1, pixel i in byte i
__device__ __forceinline__ unsigned gaze_bytes(unsigned b) { return (b & 1u) | (b & 2u) << 7 | (b & 4u) << 14 | (b & 8u) << 21; }

}  // namespace crfp
