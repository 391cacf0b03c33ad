// The source index of the bilinear resize with align_corners=False, shared by the forward kernels (resample.hip) and the resize backward
// (train_backward.hip): the backward keeps an output as a contributor of an input exactly when THIS function names that input, and takes
// the forward's own weight bits.
#pragma once

namespace crfp_index {

// PyTorch's source index for align_corners=False (area_pixel_compute_source_index + guard):
//   src = scale*(dst+0.5)-0.5, clamped at 0; i0 = min(floor(src), in-1); i1 = min(i0+1, in-1);
//   l1 = clamp(src - i0, 0, 1); l0 = 1 - l1
__device__ __forceinline__ void src_index(int dst, float scale, int in_size, int& i0, int& i1, float& l0, float& l1) {
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.0f) src = 0.0f;
    i0 = min((int)floorf(src), in_size - 1);
    i1 = min(i0 + 1, in_size - 1);
    l1 = fminf(fmaxf(src - (float)i0, 0.0f), 1.0f);
    l0 = 1.0f - l1;
}

}  // namespace crfp_index
