// View synthesis and the photometric error of a disparity map: the OTHER picture sampled back into this view along the row, and
// the L1 + SSIM error of that reconstruction against this view's picture in the Monodepth form, with its per-sample sums over the
// pixels that can be trusted.  Beyond the reference, whose inference scripts have no such step.  The contract is a closed form
// (include/nndepth_amd.h), every step one rounded fp32 operation (built with -ffp-contract=off), so the maps are held to equality.
//
// nnd_synthesize_view: ONE launch, a thread per pixel, the channels in a loop.
// nnd_photometric_error: ONE launch for the maps and the per-workgroup partials, and with `stats` a second small one that adds the
// partials in a fixed order.  No atomics.  A workgroup of 256 threads owns a tile of PH_TH x PH_TW outputs:
//   1  the tile plus a halo of one pixel in LDS: per channel the target picture and the reconstruction, and per pixel the `in` flag.
//      A halo position outside the frame holds what its REFLECTED pixel holds (-1 reads 1, H reads H-2), reconstructed at that pixel's
//      own column.  The gather runs along the row only, two adjacent columns of `other` per channel; consecutive lanes stage
//      consecutive columns of a halo row, and where the map is smooth they read neighbouring addresses.  A tap that is not `in`
//      stores 0 and is never used: its pixel and every pixel whose window holds it is not valid.
//   2  after ONE barrier a thread computes PH_ROWS pixels of its column: per channel the row sums of t, rec, t*t, rec*rec, t*rec of
//      the PH_ROWS + 2 halo rows it needs (each once), then the boxes, the SSIM term and the L1 term.  A wave reads 64 consecutive
//      words of a halo row per tap: no bank conflict whatever the pitch (it is odd all the same, for the staging's writes).
//   3  the partials {count, sum e, sum l1, sum ds} of the tile in double: a thread's pixels in row order, a butterfly over the wave,
//      the four waves in order through LDS; slot (sample, tile) of the workspace is written unconditionally.
//
// Bounds.  A global index is formed from (b, y, x) with b < B (the grid), 0 <= y < H, 0 <= x < W: the halo's rows and columns are
// reflected and then clamped into the frame where they are formed (a position beyond the reflection belongs to outputs outside
// the frame, which are not written), the two gather columns are i0 in [0, W-1] (xr was tested) and i1 = min(i0+1, W-1), and the
// stores test y < H && x < W.  An LDS index is < PH_PA * 2 C words + PH_PA bytes, which is what the launch asks for.
#include "map_ops.h"  // the contract of map, stride, mask and its polarity, in and out

namespace nnd {

constexpr int PH_TH = 16, PH_TW = 64;  // the output tile of a workgroup
constexpr int PH_BLOCK = 256, PH_ROWS = PH_TH / (PH_BLOCK / 64);  // rows per thread
constexpr int PH_MAX_C = 4;
constexpr int PH_PW = PH_TW + 2 + 1, PH_PH = PH_TH + 2, PH_PA = PH_PW * PH_PH;  // the halo tile; rows padded to an odd pitch
constexpr int SYN_BLOCK = 256;

constexpr size_t ph_lds_bytes(int C) { return (size_t)PH_PA * 4 * 2 * C + (size_t)((PH_PA + 15) / 16 * 16); }
static_assert(ph_lds_bytes(PH_MAX_C) <= 64 * 1024, "the halo tile of the largest channel count fits the default dynamic LDS limit");

static inline int64_t ph_tiles(int H, int W) { return (int64_t)cdiv(H, PH_TH) * cdiv(W, PH_TW); }
static inline bool ph_shape_ok(int B, int H, int W) { return map_shape_ok(B, H, W) && H >= 2 && W >= 2 && (int64_t)H * W <= 0x7fffffff; }
static inline int64_t ph_workspace_bytes(int B, int H, int W) { return (int64_t)B * ph_tiles(H, W) * 4 * (int64_t)sizeof(double); }

// steps 1 - 3 of the contract for the pixel in column x: whether it is `in`, and its two taps and their weight
struct PhTap {
    bool in;
    int i0, i1;
    float f;
};

__device__ __forceinline__ PhTap ph_tap(float d, bool mask_ok, int negative, int target_is_left, int x, int W) {
    PhTap t;
    const float m = (negative ? -d : d) + 0.0f;
    const bool src_ok = mask_ok && isfinite(m) && m >= 0.f;
    const float xr = target_is_left ? (float)x - m : (float)x + m;
    t.in = src_ok && xr >= 0.f && xr <= (float)(W - 1);
    t.i0 = t.i1 = 0;
    t.f = 0.f;
    if (t.in) {  // xr is finite and in [0, W-1]: so are both taps
        const float fl = floorf(xr);
        t.i0 = (int)fl;
        t.i1 = t.i0 + 1 < W - 1 ? t.i0 + 1 : W - 1;
        t.f = xr - fl;
    }
    return t;
}

__device__ __forceinline__ float ph_sample(const float* __restrict__ row, const PhTap& t) {
    const float a = row[t.i0] * (1.0f - t.f);
    const float c = row[t.i1] * t.f;
    return a + c;
}

// a NaN stays a NaN, as in torch.clamp: a non-finite picture value makes every window that holds it not valid; for every number
// the bits of fminf(fmaxf(v, 0), 1)
__device__ __forceinline__ float ph_clamp01(float v) { return v < 0.f ? 0.f : v > 1.f ? 1.f : v; }

// grid (cdiv(H*W, SYN_BLOCK), B)
__global__ void __launch_bounds__(SYN_BLOCK) synthesize_kernel(const float* __restrict__ other, const float* __restrict__ disp, long dbs,
                                                              const unsigned char* __restrict__ mask, int valid_is_one, int negative,
                                                              int target_is_left, float fill, float* __restrict__ recon,
                                                              unsigned char* __restrict__ valid_out, int C, int W, long per) {
    const long i = (long)blockIdx.x * SYN_BLOCK + threadIdx.x;
    if (i >= per) return;
    const int b = blockIdx.y;
    const long row0 = i / W * W;
    const int x = (int)(i - row0);
    const PhTap t = ph_tap(disp[(long)b * dbs + i], mask_valid(mask, (long)b * per + i, valid_is_one), negative, target_is_left, x, W);
    for (int c = 0; c < C; ++c) {
        const long plane = ((long)b * C + c) * per;
        recon[plane + i] = t.in ? ph_sample(other + plane + row0, t) : fill;
    }
    if (valid_out) valid_out[(long)b * per + i] = mask_byte(t.in, valid_is_one);
}

__device__ __forceinline__ double ph_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);  // a butterfly: the same order on every run
    return v;
}

// grid (tiles_x * tiles_y, B); dynamic LDS ph_lds_bytes(C): C planes of the target, C of the reconstruction, the flags
template <bool SSIM>
__global__ void __launch_bounds__(PH_BLOCK) photometric_kernel(const float* __restrict__ target, const float* __restrict__ other,
                                                               const float* __restrict__ disp, long dbs,
                                                               const unsigned char* __restrict__ mask, int valid_is_one, int negative,
                                                               int target_is_left, float ssim_weight, float c1, float c2, float inv_range,
                                                               float fill, float* __restrict__ error, float* __restrict__ l1_out,
                                                               float* __restrict__ dssim_out, unsigned char* __restrict__ valid_out,
                                                               double* __restrict__ partials, int C, int H, int W, int tiles_x) {
    extern __shared__ float ph_lds[];
    float* tl = ph_lds;                                              // [c][PH_PA]
    float* rl = ph_lds + (size_t)C * PH_PA;                          // [c][PH_PA]
    unsigned char* inl = (unsigned char*)(ph_lds + (size_t)2 * C * PH_PA);  // [PH_PA]
    __shared__ double red[PH_BLOCK / 64][4];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int y0 = ((int)blockIdx.x / tiles_x) * PH_TH, x0 = ((int)blockIdx.x % tiles_x) * PH_TW;
    const long per = (long)H * W;

    for (int i = tid; i < PH_PH * (PH_PW - 1); i += PH_BLOCK) {
        const int hy = i / (PH_PW - 1), hx = i % (PH_PW - 1);
        int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
        gy = gy < 0 ? -gy : gy >= H ? 2 * H - 2 - gy : gy;  // reflected: -1 reads 1, H reads H-2
        gx = gx < 0 ? -gx : gx >= W ? 2 * W - 2 - gx : gx;
        gy = gy < 0 ? 0 : gy > H - 1 ? H - 1 : gy;          // beyond the reflection: a position no written output reads
        gx = gx < 0 ? 0 : gx > W - 1 ? W - 1 : gx;
        const long p = (long)gy * W + gx;
        const PhTap t = ph_tap(disp[(long)b * dbs + p], mask_valid(mask, (long)b * per + p, valid_is_one), negative, target_is_left, gx, W);
        const int l = hy * PH_PW + hx;
        inl[l] = t.in ? 1 : 0;
        for (int c = 0; c < C; ++c) {
            const long plane = ((long)b * C + c) * per;
            tl[c * PH_PA + l] = target[plane + p];
            rl[c * PH_PA + l] = t.in ? ph_sample(other + plane + (long)gy * W, t) : 0.f;
        }
    }
    __syncthreads();

    const int lx = tid & 63, x = x0 + lx, ly0 = (tid >> 6) * PH_ROWS;
    const float inv9 = (float)(1.0 / 9.0), invC = 1.0f / (float)C;
    float ds[PH_ROWS], l1[PH_ROWS];
    bool in9[PH_ROWS];
    {
        // the flags of the PH_ROWS + 2 halo rows, three columns each
        bool rowin[PH_ROWS + 2], cin[PH_ROWS + 2];
#pragma unroll
        for (int r = 0; r < PH_ROWS + 2; ++r) {
            const unsigned char* q = inl + (ly0 + r) * PH_PW + lx;
            cin[r] = q[1] != 0;
            rowin[r] = q[0] != 0 && q[1] != 0 && q[2] != 0;
        }
#pragma unroll
        for (int j = 0; j < PH_ROWS; ++j) in9[j] = SSIM ? (rowin[j] && rowin[j + 1] && rowin[j + 2]) : cin[j + 1];
    }
    for (int c = 0; c < C; ++c) {
        const float* tp = tl + c * PH_PA + ly0 * PH_PW + lx;
        const float* rp = rl + c * PH_PA + ly0 * PH_PW + lx;
        float st[PH_ROWS + 2], sr[PH_ROWS + 2], stt[PH_ROWS + 2], srr[PH_ROWS + 2], str[PH_ROWS + 2], tc[PH_ROWS + 2], rc[PH_ROWS + 2];
#pragma unroll
        for (int r = 0; r < PH_ROWS + 2; ++r) {
            const float t0 = tp[r * PH_PW], t1 = tp[r * PH_PW + 1], t2 = tp[r * PH_PW + 2];
            const float r0 = rp[r * PH_PW], r1 = rp[r * PH_PW + 1], r2 = rp[r * PH_PW + 2];
            tc[r] = t1;
            rc[r] = r1;
            if (SSIM) {
                st[r] = (t0 + t1) + t2;
                sr[r] = (r0 + r1) + r2;
                stt[r] = (t0 * t0 + t1 * t1) + t2 * t2;
                srr[r] = (r0 * r0 + r1 * r1) + r2 * r2;
                str[r] = (t0 * r0 + t1 * r1) + t2 * r2;
            }
        }
#pragma unroll
        for (int j = 0; j < PH_ROWS; ++j) {
            const float l1c = fabsf(tc[j + 1] - rc[j + 1]) * inv_range;
            l1[j] = c == 0 ? l1c : l1[j] + l1c;
            if (SSIM) {
                const float mx = ((st[j] + st[j + 1]) + st[j + 2]) * inv9;
                const float my = ((sr[j] + sr[j + 1]) + sr[j + 2]) * inv9;
                const float sx = ((stt[j] + stt[j + 1]) + stt[j + 2]) * inv9 - mx * mx;
                const float sy = ((srr[j] + srr[j + 1]) + srr[j + 2]) * inv9 - my * my;
                const float sxy = ((str[j] + str[j + 1]) + str[j + 2]) * inv9 - mx * my;
                const float n = (2.0f * mx * my + c1) * (2.0f * sxy + c2);
                const float dn = (mx * mx + my * my + c1) * (sx + sy + c2);
                const float dsc = ph_clamp01((1.0f - n / dn) * 0.5f);
                ds[j] = c == 0 ? dsc : ds[j] + dsc;
            }
        }
    }

    double cnt = 0.0, se = 0.0, sl = 0.0, sd = 0.0;
#pragma unroll
    for (int j = 0; j < PH_ROWS; ++j) {
        const int y = y0 + ly0 + j;
        const float l1m = l1[j] * invC;
        const float dsm = SSIM ? ds[j] * invC : 0.f;
        float e = l1m;
        if (SSIM) {
            const float a = ssim_weight * dsm;
            const float c = (1.0f - ssim_weight) * l1m;
            e = a + c;
        }
        const bool valid = in9[j] && isfinite(e);
        if (y < H && x < W) {
            const long o = (long)b * per + (long)y * W + x;
            error[o] = valid ? e : fill;
            if (l1_out) l1_out[o] = valid ? l1m : fill;
            if (dssim_out) dssim_out[o] = (SSIM && valid) ? dsm : fill;
            if (valid_out) valid_out[o] = mask_byte(valid, valid_is_one);
            if (valid) {
                cnt = cnt + 1.0;
                se = se + (double)e;
                sl = sl + (double)l1m;
                sd = sd + (double)dsm;
            }
        }
    }
    if (partials) {  // uniform over the launch
        cnt = ph_wave_sum(cnt);
        se = ph_wave_sum(se);
        sl = ph_wave_sum(sl);
        sd = ph_wave_sum(sd);
        if ((tid & 63) == 0) {
            red[tid >> 6][0] = cnt;
            red[tid >> 6][1] = se;
            red[tid >> 6][2] = sl;
            red[tid >> 6][3] = sd;
        }
        __syncthreads();
        if (tid < 4) {
            double v = red[0][tid];
#pragma unroll
            for (int w = 1; w < PH_BLOCK / 64; ++w) v = v + red[w][tid];
            partials[((long)b * gridDim.x + blockIdx.x) * 4 + tid] = v;  // this workgroup's own slot, whatever it held
        }
    }
}

// grid (B): the partials of sample b's tiles in a fixed order: thread t takes the tiles t, t + 256, ..., then the butterfly, then the
// waves in order
__global__ void __launch_bounds__(PH_BLOCK) photometric_stats_kernel(const double* __restrict__ partials, double* __restrict__ stats,
                                                                     int tiles) {
    __shared__ double red[PH_BLOCK / 64][4];
    const int tid = threadIdx.x, b = blockIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = tid; t < tiles; t += PH_BLOCK) {
        const double* p = partials + ((long)b * tiles + t) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] + p[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = ph_wave_sum(v[k]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) red[tid >> 6][k] = v[k];
    }
    __syncthreads();
    if (tid < 4) {
        double s = red[0][tid];
#pragma unroll
        for (int w = 1; w < PH_BLOCK / 64; ++w) s = s + red[w][tid];
        stats[(long)b * 4 + tid] = s;
    }
}

static inline bool ph_positive_finite(float v) { return v > 0.f && v <= 3.402823466e+38f; }  // false for a NaN

// what the two entry points check alike
static int ph_check(const char* what, int B, int C, int H, int W, int64_t bstride) {
    int rc;
    NND_TRY(check_map(what, B, H, W, bstride));
    NND_REQUIRE(H >= 2 && W >= 2 && (int64_t)H * W <= 0x7fffffff, "%s: bad shape (%d,1,%d,%d) (H, W >= 2: the reflected border; H*W < 2^31)",
                what, B, H, W);
    NND_REQUIRE(C >= 1 && C <= PH_MAX_C, "%s: bad picture channels %d (1 <= C <= %d, nnd_photometric_limit)", what, C, PH_MAX_C);
    return NND_OK;
}

}  // namespace nnd

using namespace nnd;

extern "C" {

int nnd_photometric_limit(int which) {
    return which == 0 ? PH_MAX_C : which == 1 ? PH_TH : which == 2 ? PH_TW : (int)NND_ERR_INVALID;
}

int64_t nnd_photometric_workspace_bytes(int B, int H, int W) {
    if (!ph_shape_ok(B, H, W)) return (int64_t)NND_ERR_INVALID;
    return ph_workspace_bytes(B, H, W);
}

int nnd_synthesize_view(const float* other, const float* disp, int64_t disp_bstride, const unsigned char* mask, int mask_valid_is_one,
                        int negative, int target_is_left, float fill, float* recon, unsigned char* valid_out, int B, int C, int H, int W,
                        void* stream) {
    const char* what = "synthesize_view";
    NND_REQUIRE(other && disp && recon, "%s: null pointer: no picture, no map or no reconstruction", what);
    NND_REQUIRE(recon != other && recon != disp, "%s: the reconstruction must not be an input", what);
    int rc;
    NND_TRY(ph_check(what, B, C, H, W, disp_bstride));
    const long per = (long)H * W;
    hipLaunchKernelGGL(synthesize_kernel, dim3((unsigned)cdiv64(per, SYN_BLOCK), B), dim3(SYN_BLOCK), 0, (hipStream_t)stream, other, disp,
                       (long)disp_bstride, mask, mask_valid_is_one != 0, negative != 0, target_is_left != 0, fill, recon, valid_out, C, W, per);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_photometric_error(const float* target, const float* other, const float* disp, int64_t disp_bstride, const unsigned char* mask,
                          int mask_valid_is_one, int negative, int target_is_left, float ssim_weight, float c1, float c2, float inv_range,
                          float fill, float* error, float* l1_out, float* dssim_out, unsigned char* valid_out, double* stats,
                          void* workspace, int64_t workspace_bytes, int B, int C, int H, int W, void* stream) {
    const char* what = "photometric_error";
    NND_REQUIRE(target && other && disp && error, "%s: null pointer: no target, no other picture, no map or no error map", what);
    NND_REQUIRE(error != target && error != other && error != disp, "%s: the error map must not be an input", what);
    int rc;
    NND_TRY(ph_check(what, B, C, H, W, disp_bstride));
    NND_REQUIRE(ssim_weight >= 0.f && ssim_weight <= 1.f, "%s: ssim_weight is outside [0, 1]", what);  // false for a NaN
    NND_REQUIRE(ph_positive_finite(c1), "%s: c1 is not finite or not above 0", what);
    NND_REQUIRE(ph_positive_finite(c2), "%s: c2 is not finite or not above 0", what);
    NND_REQUIRE(ph_positive_finite(inv_range), "%s: inv_range is not finite or not above 0", what);
    if (stats) {
        NND_REQUIRE(workspace, "%s: null pointer: stats without a workspace", what);
        NND_TRY(check_workspace(what, workspace, workspace_bytes, ph_workspace_bytes(B, H, W), 8));
    }
    const hipStream_t s = (hipStream_t)stream;
    const int tx = cdiv(W, PH_TW), tiles = (int)ph_tiles(H, W);  // H*W < 2^31: so are the tiles
    double* partials = stats ? (double*)workspace : nullptr;
    const dim3 grid((unsigned)tiles, B);
    if (ssim_weight > 0.f)
        hipLaunchKernelGGL(photometric_kernel<true>, grid, dim3(PH_BLOCK), ph_lds_bytes(C), s, target, other, disp, (long)disp_bstride, mask,
                           mask_valid_is_one != 0, negative != 0, target_is_left != 0, ssim_weight, c1, c2, inv_range, fill, error, l1_out,
                           dssim_out, valid_out, partials, C, H, W, tx);
    else
        hipLaunchKernelGGL(photometric_kernel<false>, grid, dim3(PH_BLOCK), ph_lds_bytes(C), s, target, other, disp, (long)disp_bstride, mask,
                           mask_valid_is_one != 0, negative != 0, target_is_left != 0, ssim_weight, c1, c2, inv_range, fill, error, l1_out,
                           dssim_out, valid_out, partials, C, H, W, tx);
    NND_LAUNCH_CHECK();
    if (stats) {
        hipLaunchKernelGGL(photometric_stats_kernel, dim3(B), dim3(PH_BLOCK), 0, s, (const double*)partials, stats, tiles);
        NND_LAUNCH_CHECK();
    }
    return NND_OK;
}

}  // extern "C"
