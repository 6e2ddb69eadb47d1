// Device code shared by the VALU kernels of repvit.hip and mbv3.hip: the depthwise tap loop and the stem's patch gather.  The
// kernels themselves stay apart: their epilogues round differently (repvit.hip applies GELU to the fp32-rounded sum and its stem
// accumulates in fp32; mbv3.hip activates in float64 before the one rounding), and mbv3.hip's depthwise kernel carries the
// squeeze-excite reduction.
#pragma once
#include <hip/hip_runtime.h>

namespace nnd {

// sum over the K x K taps of one output pixel, window origin (iy0, ix0) in the Hin x Win plane xp, taps outside the plane skipped
// (zero padding); (dy, dx) order, float64 accumulation
template <int K>
__device__ __forceinline__ double dw_taps(const float* __restrict__ xp, const float* __restrict__ wp, int iy0, int ix0, int Hin, int Win) {
    double acc = 0.0;
#pragma unroll
    for (int dy = 0; dy < K; ++dy) {
        const int iy = iy0 + dy;
        if (iy < 0 || iy >= Hin) continue;
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
            const int ix = ix0 + dx;
            if (ix < 0 || ix >= Win) continue;
            acc = fma((double)wp[dy * K + dx], (double)xp[(long)iy * Win + ix], acc);
        }
    }
    return acc;
}

// the 3 x 3 x 3 input patch of output pixel (oy, ox) of a 3-channel frame xp, zero outside the frame: in[(ci * 3 + dy) * 3 + dx];
// pt / pl: the padding before the data
__device__ __forceinline__ void stem_gather(const float* __restrict__ xp, int oy, int ox, int stride, int pt, int pl, int Hin, int Win,
                                            float (&in)[27]) {
#pragma unroll
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int iy = oy * stride - pt + dy, ix = ox * stride - pl + dx;
                const bool ok = iy >= 0 && iy < Hin && ix >= 0 && ix < Win;
                in[(ci * 3 + dy) * 3 + dx] = ok ? xp[((long)ci * Hin + iy) * Win + ix] : 0.f;
            }
}

}  // namespace nnd
