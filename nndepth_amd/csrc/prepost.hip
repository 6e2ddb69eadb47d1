// Pre- / post-processing of the inference scripts on the device: no host round trip between decoding a
// frame and the first convolution.
//
//   resize_normalize : preprocess_frame  nndepth/models/raft_stereo/scripts/inference.py:55-60
//                      F.interpolate(frame, HW, mode="bilinear") (align_corners=False, no antialias) then (x - 127.5) / 127.5;
//                      source either float NCHW or the decoded uint8 HWC image itself
//   replicate_pad    : Padder.pad / unpad   nndepth/data/dataloaders/utils.py:5-21 (F.pad mode="replicate"; crop)
// Both HBM-bound element-wise kernels.  Compiled with -ffp-contract=off (the bilinear weights follow
// ATen's compute_source_index_and_lambda step by step).
#include "common.h"
#include "bilinear.h"

namespace nnd {

// one thread per output pixel, loops the C channels; u8hwc: src is (B,h,w,C) uint8, else (B,C,h,w) float
__global__ void __launch_bounds__(256) resize_normalize_kernel(const void* __restrict__ src, float* __restrict__ dst, int C, int h,
                                                               int w, int H, int W, float sub, float div, int u8hwc) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)H * W) return;
    const int b = blockIdx.y;
    const int y = (int)(idx / W), x = (int)(idx - (long)y * W);
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    src_index(sy, y, h, y0, y1, ly0, ly1);
    src_index(sx, x, w, x0, x1, lx0, lx1);
    for (int c = 0; c < C; ++c) {
        float v00, v01, v10, v11;
        if (u8hwc) {
            const unsigned char* s = (const unsigned char*)src + (long)b * h * w * C;
            v00 = (float)s[((long)y0 * w + x0) * C + c];
            v01 = (float)s[((long)y0 * w + x1) * C + c];
            v10 = (float)s[((long)y1 * w + x0) * C + c];
            v11 = (float)s[((long)y1 * w + x1) * C + c];
        } else {
            const float* s = (const float*)src + ((long)b * C + c) * h * w;
            v00 = s[(long)y0 * w + x0];
            v01 = s[(long)y0 * w + x1];
            v10 = s[(long)y1 * w + x0];
            v11 = s[(long)y1 * w + x1];
        }
        // ATen's interpolate<2> accumulates `out += src * weight` per tap, which its AVX2 build contracts to fma
        const float t0 = fmaf(v01, lx1, v00 * lx0);
        const float t1 = fmaf(v11, lx1, v10 * lx0);
        const float v = fmaf(t1, ly1, t0 * ly0);
        dst[((long)b * C + c) * H * W + idx] = (v - sub) / div;
    }
}

// dst (B*C, Ho, Wo) <- src (B*C, H, W): dst[y, x] = src[clamp(y - top), clamp(x - left)]; a negative pad crops
__global__ void __launch_bounds__(256) replicate_pad_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W,
                                                            int Ho, int Wo, int left, int top) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)Ho * Wo) return;
    const int y = (int)(idx / Wo), x = (int)(idx - (long)y * Wo);
    const int sy = min(max(y - top, 0), H - 1), sx = min(max(x - left, 0), W - 1);
    dst[(long)blockIdx.y * Ho * Wo + idx] = src[(long)blockIdx.y * H * W + (long)sy * W + sx];
}

}  // namespace nnd

using namespace nnd;

extern "C" {

int nnd_resize_normalize(const void* src, int src_is_u8_hwc, float* dst, int B, int C, int h, int w, int H, int W, float sub,
                         float div, void* stream) {
    NND_REQUIRE(src && dst, "resize_normalize: null pointer");
    NND_REQUIRE(B > 0 && C > 0 && h > 0 && w > 0 && H > 0 && W > 0 && div != 0.f, "resize_normalize: bad argument");
    hipLaunchKernelGGL(resize_normalize_kernel, dim3((unsigned)cdiv64((int64_t)H * W, 256), B), dim3(256), 0, (hipStream_t)stream, src,
                       dst, C, h, w, H, W, sub, div, src_is_u8_hwc);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_replicate_pad(const float* src, float* dst, int B, int C, int H, int W, int left, int right, int top, int bottom,
                      void* stream) {
    NND_REQUIRE(src && dst && B > 0 && C > 0 && H > 0 && W > 0, "replicate_pad: bad argument");
    const int Ho = H + top + bottom, Wo = W + left + right;
    NND_REQUIRE(Ho > 0 && Wo > 0, "replicate_pad: padding (%d,%d,%d,%d) leaves nothing of a %dx%d map", left, right, top, bottom, H, W);
    hipLaunchKernelGGL(replicate_pad_kernel, dim3((unsigned)cdiv64((int64_t)Ho * Wo, 256), B * C), dim3(256), 0, (hipStream_t)stream,
                       src, dst, H, W, Ho, Wo, left, top);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

}  // extern "C"
