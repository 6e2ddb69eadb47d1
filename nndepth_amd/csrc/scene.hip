// The scene types of the reference on the device (nndepth/scene/disparity.py, depth.py, frame.py): the tail of every inference
// script (Disparity(...).get_view / Depth(...).get_view) and the resizes of the dataloaders, without the float map going back
// to the host.
//
//   view_range      : min / max per batch element of the map get_view colours (|disp| with occluded pixels at 0; depth over
//                     its valid pixels), two passes like se_partial_kernel / se_final_kernel of stereo_eval.hip, result left in device memory
//   colorize        : matplotlib.colors.Normalize(vmin, vmax, clip=True) + Colormap.__call__ + (rgb * 255).astype(uint8) as
//                     one closed form.  matplotlib normalises an fp32 map in float64 (its vmin / vmax are float64 scalars), and
//                     the table index is a truncation, so the normalisation here is float64 too: in fp32 a handful of pixels
//                     per map fall into the neighbouring table entry.
//   pool_abs        : maxpool_disp / minpool_disp / maxpool_depth / minpool_depth (max_pool2d of |x| or -|x| with
//                     return_indices, the sign, the occlusion gather through the indices, data * W_new / W_old)
//   resize_bilinear : F.interpolate(mode="bilinear") for both align_corners modes (+ the disparity rescale, the occlusion's
//                     cast back to its dtype, Depth.resize's valid mask = isfinite(resized))
//   depth_inverse   : Depth.inverse
// All bandwidth-bound element-wise kernels of a few MB; at 544x960 they sit at the launch-latency floor.  Compiled with
// -ffp-contract=off: every rounding step is written out.
#include "common.h"
#include "bilinear.h"

namespace nnd {

constexpr int RANGE_BLOCKS = 128;  // partial blocks per batch element
constexpr int MAX_TABLE = 4096;

// v of get_view for element i of batch element b; `use` = false: the pixel does not enter the range (depth, not valid)
__device__ __forceinline__ float view_value(float x, const unsigned char* mask, long i, int kind, bool& use) {
    use = true;
    if (kind == 0) {
        x = fabsf(x);
        if (mask && mask[i] == 1) x = 0.f;
    } else if (mask && mask[i] != 1) {
        use = false;
    }
    return x;
}

// pass 1: partial[b][block] = {min, max} over a grid-strided share of batch element b
__global__ void __launch_bounds__(256) view_range_partial_kernel(const float* __restrict__ data, const unsigned char* __restrict__ mask,
                                                                 int kind, long per, float* __restrict__ partial) {
    __shared__ float sh[256][2];
    const int b = blockIdx.y;
    const float* d = data + (long)b * per;
    const unsigned char* m = mask ? mask + (long)b * per : nullptr;
    float lo = INFINITY, hi = -INFINITY;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
        bool use;
        const float v = view_value(d[i], m, i, kind, use);
        if (use) {
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
    sh[threadIdx.x][0] = lo;
    sh[threadIdx.x][1] = hi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sh[threadIdx.x][0] = fminf(sh[threadIdx.x][0], sh[threadIdx.x + s][0]);
            sh[threadIdx.x][1] = fmaxf(sh[threadIdx.x][1], sh[threadIdx.x + s][1]);
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) partial[((long)b * gridDim.x + blockIdx.x) * 2 + threadIdx.x] = sh[0][threadIdx.x];
}

// pass 2: one block per batch element
__global__ void __launch_bounds__(RANGE_BLOCKS) view_range_final_kernel(const float* __restrict__ partial, int nblocks,
                                                                        float* __restrict__ range) {
    __shared__ float sh[RANGE_BLOCKS][2];
    const int b = blockIdx.x, t = threadIdx.x;
    sh[t][0] = t < nblocks ? partial[((long)b * nblocks + t) * 2] : INFINITY;
    sh[t][1] = t < nblocks ? partial[((long)b * nblocks + t) * 2 + 1] : -INFINITY;
    __syncthreads();
    for (int s = RANGE_BLOCKS / 2; s > 0; s >>= 1) {
        if (t < s) {
            sh[t][0] = fminf(sh[t][0], sh[t + s][0]);
            sh[t][1] = fmaxf(sh[t][1], sh[t + s][1]);
        }
        __syncthreads();
    }
    if (t < 2) range[b * 2 + t] = sh[0][t];
}

struct ColorArgs {
    double lo, hi;
    int has_lo, has_hi, reverse, kind, N;
};

// Each thread colours four consecutive pixels of one row of channel 0 and writes their 12 bytes as three dwords where the
// address allows it (always when W % 4 == 0), byte by byte otherwise (row tail, rows that start off a dword).
__global__ void __launch_bounds__(256) colorize_kernel(const float* __restrict__ data, const unsigned char* __restrict__ mask,
                                                       const float* __restrict__ range, const unsigned char* __restrict__ table,
                                                       unsigned char* __restrict__ out, int C, int H, int W, long quads, ColorArgs a) {
    __shared__ unsigned tab[MAX_TABLE];  // r | g << 8 | b << 16
    for (int i = threadIdx.x; i < a.N; i += 256)
        tab[i] = (unsigned)table[3 * i] | ((unsigned)table[3 * i + 1] << 8) | ((unsigned)table[3 * i + 2] << 16);
    __syncthreads();
    const int qpr = (W + 3) >> 2;  // quads per row
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long)gridDim.x * 256) {
        const int xq = (int)(q % qpr);
        const long row = q / qpr;  // b * H + y
        const int b = (int)(row / H), y = (int)(row - (long)b * H);
        const int x0 = xq * 4, n = min(4, W - x0);
        const long src = ((long)b * C * H + y) * W + x0;  // channel 0 of batch element b
        double lo = a.lo, hi = a.hi;
        float fill = 0.f;
        if (range) {
            const float rlo = range[2 * b], rhi = range[2 * b + 1];
            fill = rlo;
            if (!a.has_lo) lo = (double)rlo;
            if (!a.has_hi) hi = (double)rhi;
        }
        const double span = hi - lo;
        unsigned rgb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < n) {
                bool use;
                float v = view_value(data[src + j], mask, src + j, a.kind, use);
                if (!use) v = fill;
                double x = (double)v;
                x = x < lo ? lo : x;  // np.clip
                x = x > hi ? hi : x;
                double nrm = lo == hi ? 0.0 : (x - lo) / span;
                if (a.reverse) nrm = 1.0 - nrm;
                const double t = nrm * (double)a.N;
                int idx = t == (double)a.N ? a.N - 1 : (int)t;
                idx = idx < 0 ? 0 : (idx > a.N - 1 ? a.N - 1 : idx);  // a non-finite value gives a wrong colour, never a read outside
                rgb[j] = tab[idx];
            } else {
                rgb[j] = 0;
            }
        }
        unsigned char* o = out + (row * W + x0) * 3;
        if (n == 4 && ((size_t)o & 3) == 0) {
            unsigned* o4 = (unsigned*)o;
            o4[0] = rgb[0] | (rgb[1] << 24);
            o4[1] = (rgb[1] >> 8) | (rgb[2] << 16);
            o4[2] = (rgb[2] >> 16) | (rgb[3] << 8);
        } else {
            for (int j = 0; j < n; ++j) {
                o[3 * j] = (unsigned char)rgb[j];
                o[3 * j + 1] = (unsigned char)(rgb[j] >> 8);
                o[3 * j + 2] = (unsigned char)(rgb[j] >> 16);
            }
        }
    }
}

struct PoolArgs {
    int H, W, kh, kw, Hp, Wp, is_min, negate, rescale;
    float mul, div;
};

// One thread per pooled pixel.  ATen's max_pool2d: the running extreme starts at -inf with the window's first offset and is
// replaced by `val > max || isnan(val)`, so the first extreme in row-major window order wins and a NaN wins over everything.
// The occlusion is read at the plane-local index from the start of the whole mask: every plane reads plane 0.
__global__ void __launch_bounds__(256) pool_abs_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                       long long* __restrict__ indices, const unsigned char* __restrict__ mask,
                                                       unsigned char* __restrict__ mask_out, unsigned char* __restrict__ finite_out,
                                                       PoolArgs a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)a.Hp * a.Wp) return;
    const long plane = blockIdx.y;
    const int oy = (int)(idx / a.Wp), ox = (int)(idx - (long)oy * a.Wp);
    const float* s = src + plane * a.H * a.W;
    const int y0 = oy * a.kh, x0 = ox * a.kw;
    float best = -INFINITY;
    long at = (long)y0 * a.W + x0;
    for (int dy = 0; dy < a.kh; ++dy)
        for (int dx = 0; dx < a.kw; ++dx) {
            const long p = (long)(y0 + dy) * a.W + (x0 + dx);
            float v = fabsf(s[p]);
            if (a.is_min) v = -v;
            if (v > best || v != v) {
                best = v;
                at = p;
            }
        }
    float r = a.is_min ? -best : best;
    if (a.negate) r *= -1.f;
    if (a.rescale) r = (r * a.mul) / a.div;
    const long o = plane * a.Hp * a.Wp + idx;
    dst[o] = r;
    if (indices) indices[o] = at;
    if (mask_out) mask_out[o] = mask[at];
    if (finite_out) finite_out[o] = isfinite(r) ? 1 : 0;
}

struct ResizeArgs {
    int h, w, H, W, align_corners, src_u8, rescale, u8_mode;
    float mul, div;
};

// one thread per output pixel of one plane; the taps and their order as in resize_normalize_kernel (ATen's interpolate<2>)
__global__ void __launch_bounds__(256) scene_resize_kernel(const void* __restrict__ src, float* __restrict__ dst,
                                                           unsigned char* __restrict__ u8_out, unsigned char* __restrict__ finite_out,
                                                           ResizeArgs a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)a.H * a.W) return;
    const long plane = blockIdx.y;
    const int y = (int)(idx / a.W), x = (int)(idx - (long)y * a.W);
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    if (a.align_corners) {
        src_index_ac(ac_scale(a.h, a.H), y, a.h, y0, y1, ly0, ly1);
        src_index_ac(ac_scale(a.w, a.W), x, a.w, x0, x1, lx0, lx1);
    } else {
        src_index((float)a.h / (float)a.H, y, a.h, y0, y1, ly0, ly1);
        src_index((float)a.w / (float)a.W, x, a.w, x0, x1, lx0, lx1);
    }
    float v00, v01, v10, v11;
    const long base = plane * a.h * a.w;
    if (a.src_u8) {
        const unsigned char* s = (const unsigned char*)src + base;
        v00 = (float)s[(long)y0 * a.w + x0];
        v01 = (float)s[(long)y0 * a.w + x1];
        v10 = (float)s[(long)y1 * a.w + x0];
        v11 = (float)s[(long)y1 * a.w + x1];
    } else {
        const float* s = (const float*)src + base;
        v00 = s[(long)y0 * a.w + x0];
        v01 = s[(long)y0 * a.w + x1];
        v10 = s[(long)y1 * a.w + x0];
        v11 = s[(long)y1 * a.w + x1];
    }
    const float t0 = fmaf(v01, lx1, v00 * lx0);
    const float t1 = fmaf(v11, lx1, v10 * lx0);
    float v = fmaf(t1, ly1, t0 * ly0);
    if (a.rescale) v = (v * a.mul) / a.div;
    const long o = plane * a.H * a.W + idx;
    if (dst) dst[o] = v;
    if (u8_out) u8_out[o] = a.u8_mode == 1 ? (v != 0.f ? 1 : 0) : (unsigned char)(int)fminf(fmaxf(v, 0.f), 255.f);
    if (finite_out) finite_out[o] = isfinite(v) ? 1 : 0;
}

__global__ void __launch_bounds__(256) depth_inverse_kernel(const float* __restrict__ src, float* __restrict__ dst, long n, float eps,
                                                            int has_max, float cmax, int has_min, float cmin) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = 1.f / (src[i] + eps);
    if (has_max) v = v > cmax ? cmax : v;  // torch.clamp keeps a NaN
    if (has_min) v = v < cmin ? cmin : v;
    dst[i] = v;
}

static bool planes_ok(int64_t planes) { return planes > 0 && planes <= 65535; }

}  // namespace nnd

using namespace nnd;

extern "C" {

int64_t nnd_view_range_workspace_bytes(int B) { return B > 0 ? (int64_t)B * RANGE_BLOCKS * 2 * sizeof(float) : (int64_t)NND_ERR_INVALID; }

int nnd_view_range(const float* data, const unsigned char* mask, int kind, int B, int C, int H, int W, void* workspace, float* range,
                   void* stream) {
    NND_REQUIRE(data && workspace && range, "view_range: null pointer");
    NND_REQUIRE(kind == 0 || kind == 1, "view_range: kind %d is neither 0 (disparity) nor 1 (depth)", kind);
    NND_REQUIRE(B > 0 && B <= 65535 && C > 0 && H > 0 && W > 0, "view_range: bad shape (%d,%d,%d,%d)", B, C, H, W);
    const long per = (long)C * H * W;
    const int nblocks = (int)(cdiv64(per, 256) < RANGE_BLOCKS ? cdiv64(per, 256) : RANGE_BLOCKS);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(view_range_partial_kernel, dim3(nblocks, B), dim3(256), 0, s, data, mask, kind, per, (float*)workspace);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(view_range_final_kernel, dim3(B), dim3(RANGE_BLOCKS), 0, s, (const float*)workspace, nblocks, range);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_colorize(const float* data, const unsigned char* mask, int kind, int B, int C, int H, int W, const float* range, int has_lo,
                 double lo, int has_hi, double hi, int reverse, const unsigned char* table, int N, unsigned char* out, void* stream) {
    NND_REQUIRE(data && table && out, "colorize: null pointer");
    NND_REQUIRE(kind == 0 || kind == 1, "colorize: kind %d is neither 0 (disparity) nor 1 (depth)", kind);
    NND_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "colorize: bad shape (%d,%d,%d,%d)", B, C, H, W);
    NND_REQUIRE(N >= 2 && N <= MAX_TABLE, "colorize: a table of %d colours (2 <= N <= %d)", N, MAX_TABLE);
    NND_REQUIRE(range || (has_lo && has_hi && !(kind == 1 && mask)),
                "colorize: no range buffer, but a bound is missing or the depth map has a valid mask (run nnd_view_range)");
    NND_REQUIRE(!(has_lo && has_hi) || lo <= hi, "colorize: min %g must be less than or equal to max %g", lo, hi);
    ColorArgs a;
    a.lo = has_lo ? lo : 0.0;
    a.hi = has_hi ? hi : 0.0;
    a.has_lo = has_lo != 0;
    a.has_hi = has_hi != 0;
    a.reverse = reverse != 0;
    a.kind = kind;
    a.N = N;
    const long quads = (long)B * H * ((W + 3) / 4);
    const int nblocks = (int)(cdiv64(quads, 256) < 2048 ? cdiv64(quads, 256) : 2048);
    hipLaunchKernelGGL(colorize_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, data, mask, range, table, out, C, H, W, quads, a);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_pool_abs(const float* src, float* dst, int64_t* indices, const unsigned char* mask, unsigned char* mask_out,
                 unsigned char* finite_out, int B, int C, int H, int W, int kh, int kw, int is_min, int negate, int rescale, float mul,
                 float div, void* stream) {
    NND_REQUIRE(src && dst, "pool_abs: null pointer");
    NND_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && planes_ok((int64_t)B * C), "pool_abs: bad shape (%d,%d,%d,%d)", B, C, H, W);
    NND_REQUIRE(kh >= 1 && kw >= 1 && kh <= H && kw <= W, "pool_abs: window %dx%d on a %dx%d map (pooling only shrinks)", kh, kw, H, W);
    NND_REQUIRE((mask == nullptr) == (mask_out == nullptr), "pool_abs: mask and mask_out go together");
    NND_REQUIRE(!rescale || div != 0.f, "pool_abs: rescale by a zero width");
    PoolArgs a{H, W, kh, kw, H / kh, W / kw, is_min != 0, negate != 0, rescale != 0, mul, div};
    hipLaunchKernelGGL(pool_abs_kernel, dim3((unsigned)cdiv64((int64_t)a.Hp * a.Wp, 256), B * C), dim3(256), 0, (hipStream_t)stream, src,
                       dst, (long long*)indices, mask, mask_out, finite_out, a);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_resize_bilinear(const void* src, int src_is_u8, float* dst, unsigned char* u8_out, int u8_mode, unsigned char* finite_out,
                        int planes, int h, int w, int H, int W, int align_corners, int rescale, float mul, float div, void* stream) {
    NND_REQUIRE(src && (dst || u8_out || finite_out), "resize_bilinear: null pointer");
    NND_REQUIRE(planes_ok(planes) && h > 0 && w > 0 && H > 0 && W > 0, "resize_bilinear: bad shape (%d planes, %dx%d -> %dx%d)", planes, h,
                w, H, W);
    NND_REQUIRE(!u8_out || u8_mode == 1 || u8_mode == 2, "resize_bilinear: u8_mode %d is neither 1 (non-zero) nor 2 (truncate)", u8_mode);
    NND_REQUIRE(!rescale || div != 0.f, "resize_bilinear: rescale by a zero width");
    ResizeArgs a{h, w, H, W, align_corners != 0, src_is_u8 != 0, rescale != 0, u8_mode, mul, div};
    hipLaunchKernelGGL(scene_resize_kernel, dim3((unsigned)cdiv64((int64_t)H * W, 256), planes), dim3(256), 0, (hipStream_t)stream, src,
                       dst, u8_out, finite_out, a);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_depth_inverse(const float* src, float* dst, int64_t n, float eps, int has_max, float clip_max, int has_min, float clip_min,
                      void* stream) {
    NND_REQUIRE(src && dst, "depth_inverse: null pointer");
    NND_REQUIRE(n > 0 && cdiv64(n, 256) <= 0x7fffffff, "depth_inverse: bad element count");
    hipLaunchKernelGGL(depth_inverse_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, (long)n, eps,
                       has_max, clip_max, has_min, clip_min);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

}  // extern "C"
