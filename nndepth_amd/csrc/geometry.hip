// Stereo geometry on the device: what a caller of a stereo model does with the disparity map next, without the map going back
// to the host.  The reference stores what this consumes and never uses it on a predicted map — Disparity.baseline
// (nndepth/scene/disparity.py:79-108), Camera.intrinsic (nndepth/scene/camera.py:5-8), Disparity.occlusion (only ever filled from
// ground truth, kitti_stereo_2015.py:188-194: 1 = no valid disparity) — and has one conversion of this kind, TartanAir's
// disparity = -BASELINE * FX / (depth + 1e-8) (nndepth/data/datasets/tartanair_dataset.py:30,239-241).
//
//   disparity_to_depth : z = fx * baseline / m in double, rounded once to fp32; the valid mask beside it
//   depth_to_disparity : the TartanAir line in its own fp32 order
//   depth_to_points    : the pinhole back-projection in double, dense (B,3,H,W)
//   points_compact     : the same points for the valid pixels only, row-major per sample, with per-sample offsets: count per
//                        workgroup (wave ballot + popcount), one exclusive scan, write.  Plain integer arithmetic, no atomics, no
//                        workgroup ever waits on another one: three launches, the same bytes every run
//   lr_consistency     : left-right check against the right view's disparity (stored as it is, or mirrored in W as
//                        pair_both_views makes the model produce it) -> occlusion mask, 1 = occluded (the KITTI polarity)
//   pair_both_views    : [left ; flipW(right)] and [right ; flipW(left)] for one forward of batch 2B
// Bandwidth-bound element-wise kernels of a few MB.  Compiled with -ffp-contract=off: every rounding step is written out, and
// the contracts are closed forms that the tests match bit for bit.  Every global index is checked against the element count before
// it is used; the one computed gather index (lr_consistency) lies in [0, W-1] by the tests that precede it.
#include "map_ops.h"  // the contract of map, stride and mask; the masks here are valid masks

namespace nnd {

constexpr int GEO_BLOCK = 256;                   // threads per workgroup = pixels per workgroup
constexpr int GEO_WAVES = GEO_BLOCK / 64;
constexpr int SCAN_BLOCK = 1024;                 // threads of the one workgroup that scans the workgroup counts

struct Cam {
    double fx, fy, cx, cy;
};

__device__ __forceinline__ Cam load_cam(const float* __restrict__ cam, int cam_stride, int b) {
    const float* c = cam + (long)b * cam_stride;
    return Cam{(double)c[0], (double)c[1], (double)c[2], (double)c[3]};
}

// X, Y of pixel (v, u) at depth z: ((u - cx) * Z) / fx in double, one rounding to fp32
__device__ __forceinline__ void back_project(const Cam& c, int u, int v, float z, float& X, float& Y) {
    X = (float)((((double)u - c.cx) * (double)z) / c.fx);
    Y = (float)((((double)v - c.cy) * (double)z) / c.fy);
}

__global__ void __launch_bounds__(GEO_BLOCK) disparity_to_depth_kernel(const float* __restrict__ disp, long dbs,
                                                                       const unsigned char* __restrict__ mask_in,
                                                                       const float* __restrict__ cam, int cam_stride, double baseline,
                                                                       int negative, float min_disp, int has_max, float max_depth,
                                                                       float* __restrict__ depth, unsigned char* __restrict__ valid_out,
                                                                       long per) {
    const long i = (long)blockIdx.x * GEO_BLOCK + threadIdx.x;
    if (i >= per) return;
    const int b = blockIdx.y;
    const float d = disp[(long)b * dbs + i];
    const float m = negative ? -d : d;
    const double fx = (double)cam[(long)b * cam_stride];
    const float z = (float)((fx * baseline) / (double)m);
    bool ok = mask_valid(mask_in, (long)b * per + i, 1) && isfinite(m) && m > min_disp;
    if (has_max) ok = ok && z <= max_depth;
    depth[(long)b * per + i] = ok ? z : 0.f;
    valid_out[(long)b * per + i] = mask_byte(ok, 1);
}

__global__ void __launch_bounds__(GEO_BLOCK) depth_to_disparity_kernel(const float* __restrict__ depth, long dbs,
                                                                       const float* __restrict__ cam, int cam_stride, double baseline,
                                                                       int negative, float eps, float* __restrict__ disp, long per) {
    const long i = (long)blockIdx.x * GEO_BLOCK + threadIdx.x;
    if (i >= per) return;
    const int b = blockIdx.y;
    const float c = (float)(-baseline * (double)cam[(long)b * cam_stride]);
    const float d = c / (depth[(long)b * dbs + i] + eps);
    disp[(long)b * per + i] = negative ? d : -d;
}

__global__ void __launch_bounds__(GEO_BLOCK) depth_to_points_kernel(const float* __restrict__ depth, long dbs,
                                                                    const unsigned char* __restrict__ valid,
                                                                    const float* __restrict__ cam, int cam_stride,
                                                                    float* __restrict__ points, int W, long per) {
    const long i = (long)blockIdx.x * GEO_BLOCK + threadIdx.x;
    if (i >= per) return;
    const int b = blockIdx.y;
    const int v = (int)(i / W), u = (int)(i - (long)v * W);
    float X = 0.f, Y = 0.f, Z = 0.f;
    if (mask_valid(valid, (long)b * per + i, 1)) {
        Z = depth[(long)b * dbs + i];
        back_project(load_cam(cam, cam_stride, b), u, v, Z, X, Y);
    }
    float* o = points + (long)b * 3 * per + i;
    o[0] = X;
    o[per] = Y;
    o[2 * per] = Z;
}

// ---- compaction.  Workgroup k of sample b owns pixels [k * 256, (k + 1) * 256) of that sample; nblk workgroups per sample.
// launch 1: counts[b * nblk + k] = valid pixels of the workgroup
__global__ void __launch_bounds__(GEO_BLOCK) compact_count_kernel(const unsigned char* __restrict__ valid, long per,
                                                                  int* __restrict__ counts) {
    __shared__ int wave_n[GEO_WAVES];
    const long i = (long)blockIdx.x * GEO_BLOCK + threadIdx.x;
    const int b = blockIdx.y;
    const bool ok = i < per && mask_valid(valid, (long)b * per + i, 1);
    const unsigned long long bal = __ballot(ok);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int w = 0; w < GEO_WAVES; ++w) n += wave_n[w];
        counts[(long)b * gridDim.x + blockIdx.x] = n;
    }
}

// launch 2, ONE workgroup: block_off[j] = sum of counts[0 .. j), offsets[b] = block_off[b * nblk], offsets[B] = the total.  Thread t
// sums the contiguous chunk [t * chunk, (t + 1) * chunk); the chunk sums are scanned across the wave with shuffles and across the
// 16 waves through LDS; each thread then walks its chunk again from its exclusive prefix.
__global__ void __launch_bounds__(SCAN_BLOCK) compact_scan_kernel(const int* __restrict__ counts, long n, int nblk, int B,
                                                                  long long* __restrict__ block_off, long long* __restrict__ offsets) {
    __shared__ long long wave_total[SCAN_BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long chunk = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const long lo = (long)t * chunk, hi = lo + chunk < n ? lo + chunk : n;
    long long s = 0;
    for (long j = lo; j < hi; ++j) s += counts[j];
    long long inc = s;  // inclusive scan over the lanes of the wave
    for (int d = 1; d < 64; d <<= 1) {
        const long long below = __shfl_up(inc, d);
        if (lane >= d) inc += below;
    }
    if (lane == 63) wave_total[wave] = inc;
    __syncthreads();
    long long run = inc - s;
    for (int w = 0; w < wave; ++w) run += wave_total[w];
    if (t == SCAN_BLOCK - 1) offsets[B] = run + s;
    for (long j = lo; j < hi; ++j) {
        block_off[j] = run;
        if (j % nblk == 0) offsets[j / nblk] = run;
        run += counts[j];
    }
}

// launch 3: row = block_off + valid pixels of the earlier waves of the workgroup + valid lanes below this one
__global__ void __launch_bounds__(GEO_BLOCK) compact_write_kernel(const float* __restrict__ depth, long dbs,
                                                                  const unsigned char* __restrict__ valid,
                                                                  const float* __restrict__ cam, int cam_stride,
                                                                  const float* __restrict__ features, int C,
                                                                  const long long* __restrict__ block_off, float* __restrict__ points,
                                                                  float* __restrict__ feats_out, int W, long per) {
    __shared__ int wave_n[GEO_WAVES];
    const long i = (long)blockIdx.x * GEO_BLOCK + threadIdx.x;
    const int b = blockIdx.y;
    const bool ok = i < per && mask_valid(valid, (long)b * per + i, 1);
    const unsigned long long bal = __ballot(ok);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_n[wave] = __popcll(bal);
    __syncthreads();
    if (!ok) return;
    long long row = block_off[(long)b * gridDim.x + blockIdx.x] + __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) row += wave_n[w];
    const int v = (int)(i / W), u = (int)(i - (long)v * W);
    const float Z = depth[(long)b * dbs + i];
    float X, Y;
    back_project(load_cam(cam, cam_stride, b), u, v, Z, X, Y);
    float* o = points + row * 3;
    o[0] = X;
    o[1] = Y;
    o[2] = Z;
    if (features) {
        const float* f = features + (long)b * C * per + i;
        float* fo = feats_out + row * C;
        for (int c = 0; c < C; ++c) fo[c] = f[(long)c * per];
    }
}

__global__ void __launch_bounds__(GEO_BLOCK) lr_consistency_kernel(const float* __restrict__ dl, long lbs, const float* __restrict__ dr,
                                                                   long rbs, int left_negative, int right_negative, int right_flipped,
                                                                   float threshold, unsigned char* __restrict__ occluded,
                                                                   float* __restrict__ err_out, int W, long per) {
    const long i = (long)blockIdx.x * GEO_BLOCK + threadIdx.x;
    if (i >= per) return;
    const int b = blockIdx.y;
    const int y = (int)(i / W), x = (int)(i - (long)y * W);
    const float d = dl[(long)b * lbs + i];
    const float mL = left_negative ? -d : d;
    float err = INFINITY;
    bool occ = true;
    if (isfinite(mL) && !(mL < 0.f)) {
        const float xr = (float)x - mL;
        const float last = (float)(W - 1);
        if (!(xr < 0.f) && !(xr > last)) {  // xr is finite and in [0, W-1]: so are both taps
            const float fl = floorf(xr);
            const int i0 = (int)fl, i1 = i0 + 1 < W - 1 ? i0 + 1 : W - 1;
            const float f = xr - fl;
            const float* row = dr + (long)b * rbs + (long)y * W;
            const float r0 = row[right_flipped ? W - 1 - i0 : i0], r1 = row[right_flipped ? W - 1 - i1 : i1];
            const float m0 = right_negative ? -r0 : r0, m1 = right_negative ? -r1 : r1;
            const float a = m0 * (1.f - f);
            const float c = m1 * f;
            const float s = a + c;
            err = fabsf(mL - s);
            occ = !(err <= threshold);
        }
    }
    occluded[(long)b * per + i] = occ ? 1 : 0;
    if (err_out) err_out[(long)b * per + i] = err;
}

// one thread per element of (B*C*H, W): the plain copy into the first half, the mirrored copy of the other view into the second
__global__ void __launch_bounds__(GEO_BLOCK) pair_both_views_kernel(const float* __restrict__ left, const float* __restrict__ right,
                                                                    float* __restrict__ f1, float* __restrict__ f2, int W, long n) {
    const long i = (long)blockIdx.x * GEO_BLOCK + threadIdx.x;
    if (i >= n) return;
    const long r = i / W;
    const int x = (int)(i - r * W);
    const long j = n + r * W + (W - 1 - x);
    const float l = left[i], rr = right[i];
    f1[i] = l;
    f2[i] = rr;
    f1[j] = rr;
    f2[j] = l;
}

// check_map, and blocks.x = workgroups per sample
static int geo_blocks(const char* what, int B, int H, int W, int64_t bstride, unsigned& blocks) {
    int rc;
    NND_TRY(check_map(what, B, H, W, bstride));
    NND_REQUIRE(cdiv64((int64_t)H * W, GEO_BLOCK) <= 0x7fffffff, "%s: map too large", what);
    blocks = (unsigned)cdiv64((int64_t)H * W, GEO_BLOCK);
    return NND_OK;
}

static int check_cam(const char* what, const float* cam, int cam_stride) {
    NND_REQUIRE(cam, "%s: null camera", what);
    NND_REQUIRE(cam_stride == 0 || cam_stride >= 4, "%s: cam_stride %d is neither 0 (one camera) nor >= 4", what, cam_stride);
    return NND_OK;
}

}  // namespace nnd

using namespace nnd;

extern "C" {

int nnd_disparity_to_depth(const float* disp, int64_t disp_bstride, const unsigned char* mask_in, const float* cam, int cam_stride,
                           double baseline, int negative, float min_disp, int has_max, float max_depth, float* depth,
                           unsigned char* valid_out, int B, int H, int W, void* stream) {
    NND_REQUIRE(disp && depth && valid_out, "disparity_to_depth: null pointer");
    int rc;
    unsigned blocks;
    NND_TRY(check_cam("disparity_to_depth", cam, cam_stride));
    NND_TRY(geo_blocks("disparity_to_depth", B, H, W, disp_bstride, blocks));
    NND_REQUIRE(baseline == baseline && min_disp == min_disp && (!has_max || max_depth == max_depth),
                "disparity_to_depth: baseline, min_disp or max_depth is NaN");
    hipLaunchKernelGGL(disparity_to_depth_kernel, dim3(blocks, B), dim3(GEO_BLOCK), 0, (hipStream_t)stream, disp, (long)disp_bstride,
                       mask_in, cam, cam_stride, baseline, negative != 0, min_disp, has_max != 0, max_depth, depth, valid_out,
                       (long)H * W);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_depth_to_disparity(const float* depth, int64_t depth_bstride, const float* cam, int cam_stride, double baseline, int negative,
                           double eps, float* disp, int B, int H, int W, void* stream) {
    NND_REQUIRE(depth && disp, "depth_to_disparity: null pointer");
    int rc;
    unsigned blocks;
    NND_TRY(check_cam("depth_to_disparity", cam, cam_stride));
    NND_TRY(geo_blocks("depth_to_disparity", B, H, W, depth_bstride, blocks));
    NND_REQUIRE(baseline == baseline && eps == eps, "depth_to_disparity: baseline or eps is NaN");
    hipLaunchKernelGGL(depth_to_disparity_kernel, dim3(blocks, B), dim3(GEO_BLOCK), 0, (hipStream_t)stream, depth, (long)depth_bstride,
                       cam, cam_stride, baseline, negative != 0, (float)eps, disp, (long)H * W);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_depth_to_points(const float* depth, int64_t depth_bstride, const unsigned char* valid, const float* cam, int cam_stride,
                        float* points, int B, int H, int W, void* stream) {
    NND_REQUIRE(depth && points, "depth_to_points: null pointer");
    int rc;
    unsigned blocks;
    NND_TRY(check_cam("depth_to_points", cam, cam_stride));
    NND_TRY(geo_blocks("depth_to_points", B, H, W, depth_bstride, blocks));
    hipLaunchKernelGGL(depth_to_points_kernel, dim3(blocks, B), dim3(GEO_BLOCK), 0, (hipStream_t)stream, depth, (long)depth_bstride, valid,
                       cam, cam_stride, points, W, (long)H * W);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

// block_off (int64 per workgroup), then counts (int32 per workgroup)
int64_t nnd_points_compact_workspace_bytes(int B, int H, int W) {
    if (!map_shape_ok(B, H, W)) return (int64_t)NND_ERR_INVALID;
    return (int64_t)B * cdiv64((int64_t)H * W, GEO_BLOCK) * 12;
}

int nnd_points_compact(const float* depth, int64_t depth_bstride, const unsigned char* valid, const float* cam, int cam_stride,
                       const float* features, int C, float* points, float* feats_out, int64_t* offsets, void* workspace,
                       int64_t workspace_bytes, int B, int H, int W, void* stream) {
    NND_REQUIRE(depth && points && offsets && workspace, "points_compact: null pointer");
    int rc;
    unsigned blocks;
    NND_TRY(check_cam("points_compact", cam, cam_stride));
    NND_TRY(geo_blocks("points_compact", B, H, W, depth_bstride, blocks));
    NND_REQUIRE((features == nullptr) == (feats_out == nullptr), "points_compact: features and feats_out go together");
    NND_REQUIRE(!features || C > 0, "points_compact: features of %d channels", C);
    NND_TRY(check_workspace("points_compact", workspace, workspace_bytes, nnd_points_compact_workspace_bytes(B, H, W), 8));
    const long n = (long)B * blocks;
    long long* block_off = (long long*)workspace;
    int* counts = (int*)(block_off + n);
    const long per = (long)H * W;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(compact_count_kernel, dim3(blocks, B), dim3(GEO_BLOCK), 0, s, valid, per, counts);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(SCAN_BLOCK), 0, s, (const int*)counts, n, (int)blocks, B, block_off,
                       (long long*)offsets);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(compact_write_kernel, dim3(blocks, B), dim3(GEO_BLOCK), 0, s, depth, (long)depth_bstride, valid, cam, cam_stride,
                       features, C, (const long long*)block_off, points, feats_out, W, per);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_lr_consistency(const float* disp_left, int64_t left_bstride, const float* disp_right, int64_t right_bstride, int left_negative,
                       int right_negative, int right_flipped, float threshold, unsigned char* occluded, float* err_out, int B, int H,
                       int W, void* stream) {
    NND_REQUIRE(disp_left && disp_right && occluded, "lr_consistency: null pointer");
    int rc;
    unsigned blocks;
    NND_TRY(geo_blocks("lr_consistency", B, H, W, left_bstride, blocks));
    NND_TRY(geo_blocks("lr_consistency", B, H, W, right_bstride, blocks));
    NND_REQUIRE(W < (1 << 24), "lr_consistency: W = %d columns are not exact in fp32", W);
    NND_REQUIRE(threshold == threshold, "lr_consistency: the threshold is NaN");
    hipLaunchKernelGGL(lr_consistency_kernel, dim3(blocks, B), dim3(GEO_BLOCK), 0, (hipStream_t)stream, disp_left, (long)left_bstride,
                       disp_right, (long)right_bstride, left_negative != 0, right_negative != 0, right_flipped != 0, threshold, occluded,
                       err_out, W, (long)H * W);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_pair_both_views(const float* left, const float* right, float* frames1, float* frames2, int B, int C, int H, int W,
                        void* stream) {
    NND_REQUIRE(left && right && frames1 && frames2, "pair_both_views: null pointer");
    NND_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "pair_both_views: bad shape (%d,%d,%d,%d)", B, C, H, W);
    const int64_t n = (int64_t)B * C * H * W;
    NND_REQUIRE(cdiv64(n, GEO_BLOCK) <= 0x7fffffff, "pair_both_views: frames too large");
    hipLaunchKernelGGL(pair_both_views_kernel, dim3((unsigned)cdiv64(n, GEO_BLOCK)), dim3(GEO_BLOCK), 0, (hipStream_t)stream, left, right,
                       frames1, frames2, W, (long)n);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

}  // extern "C"
