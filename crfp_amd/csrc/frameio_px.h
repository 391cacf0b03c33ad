// Pixel helpers shared by the 8-bit frame kernels (frameio.hip, bicubic.hip): byte <-> unit conversions, the y_only chroma merge and the
// 1- / 4-pixel loads and stores.  Every expression is written once here, so that the kernels that must agree bit for bit cannot drift apart.
#pragma once
#include "crfp_common.h"

namespace crfp {

__device__ __forceinline__ float io_unit(unsigned byte) { return (float)byte / 255.0f; }
__device__ __forceinline__ unsigned io_q(float v) { return (unsigned)rintf(fminf(fmaxf(v * 255.0f, 0.0f), 255.0f)); }
// byte k (k < 12) of three little-endian words
__device__ __forceinline__ unsigned io_byte(const unsigned (&w)[3], int k) { return w[k / 4] >> 8 * (k % 4) & 0xffu; }

// test_video.py:100-127,401-402 in fp32, one rounding per operation: u, v of the chroma pixel (r, g, b) under the luma yy, back to RGB
__device__ __forceinline__ void io_merge(float yy, float r, float g, float b, float& R, float& G, float& B) {
    const float u = ((-0.147f * r) - (0.289f * g)) + (0.436f * b);
    const float v = ((0.615f * r) - (0.515f * g)) - (0.100f * b);
    R = yy + (1.14f * v);
    G = (yy + (-0.396f * u)) - (0.581f * v);
    B = yy + (2.029f * u);
}

// NPX consecutive floats of a plane
template <int NPX>
__device__ __forceinline__ void io_load_plane(const float* __restrict__ s, float (&v)[NPX]) {
    if constexpr (NPX == 4) {
        const cf32x4 q = *reinterpret_cast<const cf32x4*>(s);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = *s;
    }
}

// ... and their store
template <int NPX>
__device__ __forceinline__ void io_store_plane(float* __restrict__ d, const float (&v)[NPX]) {
    if constexpr (NPX == 4) *reinterpret_cast<cf32x4*>(d) = cf32x4{v[0], v[1], v[2], v[3]};
    else *d = v[0];
}

// ch[c][i] = channel c (R, G, B) of pixel i -> NPX pixels of interleaved bytes at `o`, each io_q of its value; NPX == 4: `o` is 4-byte aligned
template <int NPX>
__device__ __forceinline__ void io_store_px(uint8_t* __restrict__ o, const float (&ch)[3][NPX], int bgr) {
    if constexpr (NPX == 4) {
        unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 12; ++k) w[k / 4] |= io_q(bgr ? ch[2 - k % 3][k / 3] : ch[k % 3][k / 3]) << 8 * (k % 4);
        unsigned* o4 = reinterpret_cast<unsigned*>(o);
        o4[0] = w[0]; o4[1] = w[1]; o4[2] = w[2];
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[bgr ? 2 - c : c] = (uint8_t)io_q(ch[c][0]);
    }
}

}  // namespace crfp
