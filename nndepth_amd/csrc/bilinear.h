// Source index and weights of F.interpolate(mode="bilinear", align_corners=False), shared by prepost.hip (nnd_resize_normalize)
// and repvit.hip (the FeatureFusionBlock upsample); the align_corners=True pair beside it is scene.hip's.
#pragma once
#include "common.h"

namespace nnd {

// ATen: area_pixel_compute_source_index (align_corners = false, not cubic) + guard_index_and_lambda
__device__ __forceinline__ void src_index(float scale, int dst, int in_size, int& i0, int& i1, float& l0, float& l1) {
    float real = fmaf(scale, (float)dst + 0.5f, -0.5f);  // ATen's x86 build contracts scale*(dst+0.5)-0.5 into one fma; the
                                                         // weight is sensitive to that rounding (measured against torch CPU)
    real = real < 0.f ? 0.f : real;
    i0 = min((int)floorf(real), in_size - 1);
    l1 = fminf(fmaxf(real - (float)i0, 0.f), 1.f);
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l0 = 1.f - l1;
}

// ATen: area_pixel_compute_scale with align_corners = true
__device__ __forceinline__ float ac_scale(int in_size, int out_size) {
    return out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.f;
}

// ATen: area_pixel_compute_source_index (align_corners = true: scale * dst) + guard_index_and_lambda
__device__ __forceinline__ void src_index_ac(float scale, int dst, int in_size, int& i0, int& i1, float& l0, float& l1) {
    const float real = scale * (float)dst;
    i0 = min((int)floorf(real), in_size - 1);
    l1 = fminf(fmaxf(real - (float)i0, 0.f), 1.f);
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l0 = 1.f - l1;
}

}  // namespace nnd
