// The input contract of the disparity / depth map operations (geometry.hip, speckle.hip, warp.hip, median.hip, photometric.hip),
// stated once.
//   map     (B,1,H,W) fp32 with dense rows; sample b starts bstride >= H*W floats after sample b-1 (a channel slice of a 2-channel
//           output, half of a stacked batch).  1 <= B <= 65535 (a grid dimension), H, W > 0.
//   mask    optional, B*H*W dense bytes; any non-zero byte is "set".  valid_is_one != 0: set = valid (a valid mask); == 0: set =
//           invalid (an occlusion mask).  No mask: every pixel is mask-valid.
//   ok      = mask-valid && isfinite(value).
//   out     a mask that an operation writes is in the polarity of the mask it read: mask_byte(valid, valid_is_one).
// The kernels keep pointer, stride, mask and polarity as separate arguments; an operation with a stricter shape limit of its own
// (H*W < 2^31, B*H <= 2^25, a tile count) states it beside the launch that needs it.
#pragma once
#include "common.h"

namespace nnd {

// mask-valid alone: for the operations that test the magnitude (isfinite(m) && m >= 0) and not the value
__device__ __forceinline__ bool mask_valid(const unsigned char* __restrict__ mask, long p, int valid_is_one) {
    return !mask || (mask[p] != 0) == (valid_is_one != 0);
}

__device__ __forceinline__ bool map_ok(float v, const unsigned char* __restrict__ mask, long p, int valid_is_one) {
    return mask_valid(mask, p, valid_is_one) && isfinite(v);
}

__device__ __forceinline__ unsigned char mask_byte(bool valid, int valid_is_one) { return (valid == (valid_is_one != 0)) ? 1 : 0; }

static inline bool map_shape_ok(int B, int H, int W) { return B > 0 && B <= 65535 && H > 0 && W > 0; }  // the *_workspace_bytes' test

static inline int check_map(const char* what, int B, int H, int W, int64_t bstride) {
    NND_REQUIRE(map_shape_ok(B, H, W), "%s: bad shape (%d,1,%d,%d) (1 <= B <= 65535)", what, B, H, W);
    NND_REQUIRE(bstride >= (int64_t)H * W, "%s: batch stride %lld is less than H*W = %lld", what, (long long)bstride, (long long)H * W);
    return NND_OK;
}

static inline int check_workspace(const char* what, const void* workspace, int64_t bytes, int64_t need, int alignment) {
    NND_REQUIRE(bytes >= need, "%s: workspace of %lld bytes, %lld needed", what, (long long)bytes, (long long)need);
    NND_REQUIRE(((size_t)workspace & (size_t)(alignment - 1)) == 0, "%s: the workspace is not %d-byte aligned", what, alignment);
    return NND_OK;
}

}  // namespace nnd
