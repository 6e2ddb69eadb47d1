// The monocular evaluation criterion on the device: no host round trip between the model's depth map and its
// metrics.
//
//   depth_eval            : DepthEvalCriterion.__call__  nndepth/models/midas/scripts/evaluate.py:48-211 with
//                           scale_shift_estimation / ssi_depth / normalize_01_depth  nndepth/models/midas/loss.py:6-59
//   depth_eval_accumulate : the dataset mean's bookkeeping  nndepth/models/midas/scripts/evaluate.py:300-302
//
// The criterion is a chain of masked reductions in which each needs the one before it, so it is a chain of small launches
// (grid = (G blocks, B samples) unless said otherwise), every one a per-block partial in double that the NEXT launch adds up in
// index order (every block redundantly, G <= 64 values), as se_partial_kernel / se_final_kernel of stereo_eval.hip do:
//
//   1 fit_mean    n, sum p, sum g over the ORIGINAL mask                                  -> P1[b][blk][3]
//   2 fit_moment  means from P1; sum (p-pm)^2, sum (p-pm)(g-gm)                           -> P2[b][blk][2]
//   3 metrics     scale / shift from P1, P2 (-> FIT[b]); over the METRIC mask (original & 0.1f < g < (float)max_depth):
//                 count, the four error sums, the three delta counts, min / max of g and of the aligned p
//                                                                                         -> P3[b][blk][12]
//   4 median      grid (2 maps, B), one workgroup each: the lower median of the sample's g, and of its aligned p, over the
//                 metric mask: radix select on the order-preserving integer key of the fp32 value, 4 passes of 8 bits with
//                 an LDS histogram (integer atomics only; rank_select of eval_chain.h, shared with midas_loss.hip).  The fit is
//                 monotone (decreasing for scale < 0), so the aligned map's median is the aligned value of the raw p at the
//                 rank, mirrored if scale < 0                                                       -> MED[b][2]
//   5 ssi_scale   batch-global min / max from P3 (all samples), shift = normalised median; sum |xn - shift| for both maps
//                                                                                         -> P5[b][blk][2]
//   6 ssi_error   scale = mean |xn - shift| from P5 (0 -> 1); sum |ssi_p - ssi_g|, sum (.)^2 -> P6[b][blk][2]
//   7 final       one block: everything added in (sample, block) order -> the 9 metrics + the count
//
// Every loop's trip count is fixed by the shape, no kernel waits on another workgroup, nothing retries, no floating-point atomics:
// the ten doubles are the same bits run to run.  Inputs are fp32; everything after the load is double.  Compiled with
// -ffp-contract=off: aligned = p * scale + shift is a rounded product and a rounded sum, as the float64 statement of the
// contract has it (the delta counts are compared with it exactly).
#include "eval_chain.h"

namespace nnd {

constexpr int DE_MED_T = 1024;  // threads of a median workgroup
constexpr int DE_MED_U = 8;     // pixels a median thread has in flight
constexpr int DE_N1 = 3, DE_N2 = 2, DE_N3 = 12, DE_N5 = 2, DE_N6 = 2;
// P3 slots
enum { M_CNT = 0, M_ABS_REL, M_SQ_REL, M_SQ, M_LOG, M_D1, M_D2, M_D3, M_GMIN, M_GMAX, M_AMIN, M_AMAX };

struct DeWs {  // the workspace, in doubles
    double *p1, *p2, *fit, *p3, *med, *p5, *p6;
};
static inline int64_t de_ws_doubles(int B) {
    return (int64_t)B * (DE_GMAX * (DE_N1 + DE_N2 + DE_N3 + DE_N5 + DE_N6) + 4);
}
static inline DeWs de_ws(void* workspace, int B) {
    DeWs w;
    double* p = (double*)workspace;
    w.p1 = p, p += (int64_t)B * DE_GMAX * DE_N1;
    w.p2 = p, p += (int64_t)B * DE_GMAX * DE_N2;
    w.fit = p, p += (int64_t)B * 2;
    w.p3 = p, p += (int64_t)B * DE_GMAX * DE_N3;
    w.med = p, p += (int64_t)B * 2;
    w.p5 = p, p += (int64_t)B * DE_GMAX * DE_N5;
    w.p6 = p;
    return w;
}

struct DeIn {
    const float* pred;
    const float* gt;
    const unsigned char* mask;  // may be null
    long HW;
    float lo, hi;  // 0.1f, (float)max_depth
};

__device__ __forceinline__ bool de_valid(const DeIn& a, long i) { return !a.mask || a.mask[i] != 0; }
__device__ __forceinline__ bool de_metric(const DeIn& a, long i, float g) { return de_valid(a, i) && g > a.lo && g < a.hi; }

// scale, shift of sample b from the two stages of partial sums (evaluate.py:129-145): unaligned (1, 0) up to 100 valid pixels;
// a constant prediction c takes the minimum-norm solution torch.linalg.lstsq returns on the CPU
__device__ __forceinline__ void de_fit(const double* t1, const double* t2, double& scale, double& shift) {
    const double n = t1[0];
    scale = 1.0, shift = 0.0;
    if (n > 100.0) {
        const double pm = t1[1] / n, gm = t1[2] / n;
        if (t2[0] == 0.0) {
            scale = pm * gm / (pm * pm + 1.0);
            shift = gm / (pm * pm + 1.0);
        } else {
            scale = t2[1] / t2[0];
            shift = gm - scale * pm;
        }
    }
}

__global__ void __launch_bounds__(DE_T) de_fit_mean_kernel(DeIn a, double* __restrict__ p1) {
    __shared__ double sh[DE_T][DE_N1];
    const int b = blockIdx.y;
    const float* p = a.pred + (long)b * a.HW;
    const float* g = a.gt + (long)b * a.HW;
    DeIn s = a;
    if (s.mask) s.mask += (long)b * a.HW;
    double acc[DE_N1] = {0.0, 0.0, 0.0};
    for (long i = (long)blockIdx.x * DE_T + threadIdx.x; i < a.HW; i += (long)gridDim.x * DE_T)
        if (de_valid(s, i)) {
            acc[0] += 1.0;
            acc[1] += (double)p[i];
            acc[2] += (double)g[i];
        }
    de_block_sum<DE_N1>(acc, sh);
    if (threadIdx.x < DE_N1) p1[((long)b * gridDim.x + blockIdx.x) * DE_N1 + threadIdx.x] = sh[0][threadIdx.x];
}

__global__ void __launch_bounds__(DE_T) de_fit_moment_kernel(DeIn a, const double* __restrict__ p1, double* __restrict__ p2) {
    __shared__ double sh[DE_T][DE_N2];
    __shared__ double t1[DE_N1];
    const int b = blockIdx.y, G = gridDim.x;
    de_sum_partials<DE_N1>(p1 + (long)b * G * DE_N1, G, t1);
    const float* p = a.pred + (long)b * a.HW;
    const float* g = a.gt + (long)b * a.HW;
    DeIn s = a;
    if (s.mask) s.mask += (long)b * a.HW;
    const double n = t1[0] > 0.0 ? t1[0] : 1.0, pm = t1[1] / n, gm = t1[2] / n;
    double acc[DE_N2] = {0.0, 0.0};
    for (long i = (long)blockIdx.x * DE_T + threadIdx.x; i < a.HW; i += (long)gridDim.x * DE_T)
        if (de_valid(s, i)) {
            const double dp = (double)p[i] - pm;
            acc[0] += dp * dp;
            acc[1] += dp * ((double)g[i] - gm);
        }
    de_block_sum<DE_N2>(acc, sh);
    if (threadIdx.x < DE_N2) p2[((long)b * G + blockIdx.x) * DE_N2 + threadIdx.x] = sh[0][threadIdx.x];
}

__global__ void __launch_bounds__(DE_T) de_metrics_kernel(DeIn a, const double* __restrict__ p1, const double* __restrict__ p2,
                                                          double* __restrict__ fit, double* __restrict__ p3) {
    __shared__ double sh[DE_T][DE_N3];
    __shared__ double t1[DE_N1], t2[DE_N2];
    const int b = blockIdx.y, G = gridDim.x;
    de_sum_partials<DE_N1>(p1 + (long)b * G * DE_N1, G, t1);
    de_sum_partials<DE_N2>(p2 + (long)b * G * DE_N2, G, t2);
    double scale, shift;
    de_fit(t1, t2, scale, shift);
    if (blockIdx.x == 0 && threadIdx.x == 0) fit[2 * b] = scale, fit[2 * b + 1] = shift;
    const float* p = a.pred + (long)b * a.HW;
    const float* g = a.gt + (long)b * a.HW;
    DeIn s = a;
    if (s.mask) s.mask += (long)b * a.HW;
    double acc[DE_N3];
#pragma unroll
    for (int i = 0; i < DE_N3; ++i) acc[i] = 0.0;
    acc[M_GMIN] = acc[M_AMIN] = INFINITY;
    acc[M_GMAX] = acc[M_AMAX] = -INFINITY;
    for (long i = (long)blockIdx.x * DE_T + threadIdx.x; i < a.HW; i += (long)gridDim.x * DE_T) {
        const float gf = g[i];
        if (!de_metric(s, i, gf)) continue;
        const double gd = (double)gf, ad = (double)p[i] * scale + shift, d = ad - gd;
        acc[M_CNT] += 1.0;
        acc[M_ABS_REL] += fabs(d) / gd;
        acc[M_SQ_REL] += d * d / gd;
        acc[M_SQ] += d * d;
        const double l = log(ad) - log(gd);  // a non-positive aligned value: NaN, as in the reference
        acc[M_LOG] += l * l;
        const double r1 = ad / gd, r2 = gd / ad, r = r1 > r2 ? r1 : r2;
        acc[M_D1] += r < 1.25 ? 1.0 : 0.0;
        acc[M_D2] += r < 1.25 * 1.25 ? 1.0 : 0.0;
        acc[M_D3] += r < 1.25 * 1.25 * 1.25 ? 1.0 : 0.0;
        acc[M_GMIN] = fmin(acc[M_GMIN], gd);
        acc[M_GMAX] = fmax(acc[M_GMAX], gd);
        acc[M_AMIN] = fmin(acc[M_AMIN], ad);
        acc[M_AMAX] = fmax(acc[M_AMAX], ad);
    }
#pragma unroll
    for (int i = 0; i < DE_N3; ++i) sh[threadIdx.x][i] = acc[i];
    __syncthreads();
    for (int st = DE_T / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            double* x = sh[threadIdx.x];
            const double* y = sh[threadIdx.x + st];
#pragma unroll
            for (int i = 0; i < M_GMIN; ++i) x[i] += y[i];
            x[M_GMIN] = fmin(x[M_GMIN], y[M_GMIN]);
            x[M_GMAX] = fmax(x[M_GMAX], y[M_GMAX]);
            x[M_AMIN] = fmin(x[M_AMIN], y[M_AMIN]);
            x[M_AMAX] = fmax(x[M_AMAX], y[M_AMAX]);
        }
        __syncthreads();
    }
    if (threadIdx.x < DE_N3) p3[((long)b * G + blockIdx.x) * DE_N3 + threadIdx.x] = sh[0][threadIdx.x];
}

// blockIdx.x: 0 = gt, 1 = prediction; blockIdx.y: sample.  med[2b + map] = the raw fp32 value whose (aligned) value is the lower
// median, position (n - 1) / 2 of the sorted values, of the sample's n pixels in the metric mask; untouched if n == 0
__global__ void __launch_bounds__(DE_MED_T) de_median_kernel(DeIn a, int G, const double* __restrict__ fit, const double* __restrict__ p3,
                                                             double* __restrict__ med) {
    __shared__ RankSelectLds<unsigned> lds;
    __shared__ unsigned s_rank;
    __shared__ int s_n;
    const int map = blockIdx.x, b = blockIdx.y;
    if (threadIdx.x == 0) {
        double n = 0.0;
        for (int k = 0; k < G; ++k) n += p3[((long)b * G + k) * DE_N3 + M_CNT];
        s_n = (int)n;
        unsigned rank = n > 0.0 ? (unsigned)(((long)n - 1) / 2) : 0u;
        if (map == 1 && fit[2 * b] < 0.0) rank = (unsigned)((long)n - 1) - rank;  // decreasing fit: count from the other end
        s_rank = rank;
    }
    __syncthreads();
    if (s_n == 0) return;  // the whole block
    const float* v = (map ? a.pred : a.gt) + (long)b * a.HW;
    const float* g = a.gt + (long)b * a.HW;
    DeIn s = a;
    if (s.mask) s.mask += (long)b * a.HW;
    const unsigned key = rank_select<unsigned, DE_MED_T, DE_MED_U>(
        a.HW, s_rank,
        [&](long i, unsigned& k) {
            const float gv = g[i];
            k = de_key(v[i]);
            return de_valid(s, i) && gv > a.lo && gv < a.hi;
        },
        lds);
    if (threadIdx.x == 0) med[2 * b + map] = (double)de_unkey(key);
}

// the batch-global range of g and of the aligned p over the metric mask, from every sample's partials; r[0..4) = gmin, gmax,
// amin, amax
__device__ __forceinline__ void de_global_range(const double* __restrict__ p3, int nparts, double (*sh)[4], double* r) {
    double x[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
    for (int k = threadIdx.x; k < nparts; k += DE_T) {
        const double* q = p3 + (long)k * DE_N3;
        x[0] = fmin(x[0], q[M_GMIN]);
        x[1] = fmax(x[1], q[M_GMAX]);
        x[2] = fmin(x[2], q[M_AMIN]);
        x[3] = fmax(x[3], q[M_AMAX]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) sh[threadIdx.x][i] = x[i];
    __syncthreads();
    for (int st = DE_T / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                sh[threadIdx.x][i] = (i & 1) ? fmax(sh[threadIdx.x][i], sh[threadIdx.x + st][i]) : fmin(sh[threadIdx.x][i], sh[threadIdx.x + st][i]);
        __syncthreads();
    }
    if (threadIdx.x < 4) r[threadIdx.x] = sh[0][threadIdx.x];
    __syncthreads();
}

// normalize_01_depth (loss.py:56-58): (x - min) / (max - min + 1e-6)
__device__ __forceinline__ double de_norm(double x, double lo, double hi) { return (x - lo) / (hi - lo + 1e-6); }

__global__ void __launch_bounds__(DE_T) de_ssi_scale_kernel(DeIn a, const double* __restrict__ fit, const double* __restrict__ p3,
                                                            const double* __restrict__ med, double* __restrict__ p5) {
    __shared__ double sh[DE_T][DE_N5];
    __shared__ double shr[DE_T][4];
    __shared__ double r[4];
    const int b = blockIdx.y, G = gridDim.x;
    de_global_range(p3, G * gridDim.y, shr, r);
    const double scale = fit[2 * b], shift = fit[2 * b + 1];
    const double sg = de_norm(med[2 * b], r[0], r[1]), sa = de_norm(med[2 * b + 1] * scale + shift, r[2], r[3]);
    const float* p = a.pred + (long)b * a.HW;
    const float* g = a.gt + (long)b * a.HW;
    DeIn s = a;
    if (s.mask) s.mask += (long)b * a.HW;
    double acc[DE_N5] = {0.0, 0.0};
    for (long i = (long)blockIdx.x * DE_T + threadIdx.x; i < a.HW; i += (long)gridDim.x * DE_T) {
        const float gf = g[i];
        if (!de_metric(s, i, gf)) continue;
        acc[0] += fabs(de_norm((double)gf, r[0], r[1]) - sg);
        acc[1] += fabs(de_norm((double)p[i] * scale + shift, r[2], r[3]) - sa);
    }
    de_block_sum<DE_N5>(acc, sh);
    if (threadIdx.x < DE_N5) p5[((long)b * G + blockIdx.x) * DE_N5 + threadIdx.x] = sh[0][threadIdx.x];
}

__global__ void __launch_bounds__(DE_T) de_ssi_error_kernel(DeIn a, const double* __restrict__ fit, const double* __restrict__ p3,
                                                            const double* __restrict__ med, const double* __restrict__ p5,
                                                            double* __restrict__ p6) {
    __shared__ double sh[DE_T][DE_N6];
    __shared__ double shr[DE_T][4];
    __shared__ double r[4], t5[DE_N5], t3[DE_N3];
    const int b = blockIdx.y, G = gridDim.x;
    de_global_range(p3, G * gridDim.y, shr, r);
    de_sum_partials<DE_N5>(p5 + (long)b * G * DE_N5, G, t5);
    de_sum_partials<DE_N3>(p3 + (long)b * G * DE_N3, G, t3);  // only the count is a sum; the other slots are not read
    const double n = t3[M_CNT];
    double acc[DE_N6] = {0.0, 0.0};
    if (n > 0.0) {  // a sample without a pixel in the mask contributes nothing (the whole block takes the same branch)
        const double scale = fit[2 * b], shift = fit[2 * b + 1];
        const double sg = de_norm(med[2 * b], r[0], r[1]), sa = de_norm(med[2 * b + 1] * scale + shift, r[2], r[3]);
        double cg = t5[0] / n, ca = t5[1] / n;  // scale_shift_estimation (loss.py:22-23); ssi_depth: scale[scale == 0] = 1
        if (cg == 0.0) cg = 1.0;
        if (ca == 0.0) ca = 1.0;
        const float* p = a.pred + (long)b * a.HW;
        const float* g = a.gt + (long)b * a.HW;
        DeIn s = a;
        if (s.mask) s.mask += (long)b * a.HW;
        for (long i = (long)blockIdx.x * DE_T + threadIdx.x; i < a.HW; i += (long)gridDim.x * DE_T) {
            const float gf = g[i];
            if (!de_metric(s, i, gf)) continue;
            const double yg = (de_norm((double)gf, r[0], r[1]) - sg) / cg;
            const double ya = (de_norm((double)p[i] * scale + shift, r[2], r[3]) - sa) / ca;
            const double d = ya - yg;
            acc[0] += fabs(d);
            acc[1] += d * d;
        }
    }
    de_block_sum<DE_N6>(acc, sh);
    if (threadIdx.x < DE_N6) p6[((long)b * G + blockIdx.x) * DE_N6 + threadIdx.x] = sh[0][threadIdx.x];
}

// one block: thread q < 8 adds slot q of P3 over all (sample, block) partials in index order, threads 8, 9 the two of P6
__global__ void __launch_bounds__(64) de_final_kernel(const double* __restrict__ p3, const double* __restrict__ p6, int nparts,
                                                      double* __restrict__ out) {
    __shared__ double t[10];
    const int q = threadIdx.x;
    if (q < 10) {
        double s = 0.0;
        if (q < 8)
            for (int k = 0; k < nparts; ++k) s += p3[(long)k * DE_N3 + q];
        else
            for (int k = 0; k < nparts; ++k) s += p6[(long)k * DE_N6 + (q - 8)];
        t[q] = s;
    }
    __syncthreads();
    if (q != 0) return;
    const double n = t[M_CNT];
    out[9] = n;
    if (n == 0.0) {  // _empty_metrics (evaluate.py:193-210)
        for (int i = 0; i < 9; ++i) out[i] = (i >= 4 && i <= 6) ? 0.0 : (double)INFINITY;
        return;
    }
    out[0] = t[M_ABS_REL] / n;
    out[1] = t[M_SQ_REL] / n;
    out[2] = sqrt(t[M_SQ] / n);
    out[3] = sqrt(t[M_LOG] / n);
    out[4] = t[M_D1] / n;
    out[5] = t[M_D2] / n;
    out[6] = t[M_D3] / n;
    out[7] = t[8] / n;
    out[8] = sqrt(t[9] / n);
}

__global__ void de_accumulate_kernel(const double* __restrict__ metrics, double* __restrict__ sums, double* __restrict__ counts) {
    const int i = threadIdx.x;
    if (i >= 9) return;
    const double m = metrics[i];
    if (isfinite(m)) {
        sums[i] += m;
        counts[i] += 1.0;
    }
}

}  // namespace nnd

using namespace nnd;

extern "C" {

int64_t nnd_depth_eval_workspace_bytes(int B) {
    if (B <= 0 || B > 65535) {
        set_error("depth_eval_workspace_bytes: bad batch size %d (1 .. 65535)", B);
        return (int64_t)NND_ERR_INVALID;
    }
    return de_ws_doubles(B) * (int64_t)sizeof(double);
}

int nnd_depth_eval(const float* pred, const float* gt, const unsigned char* valid_mask, int B, int H, int W, float max_depth,
                   void* workspace, int64_t workspace_bytes, double* out, void* stream) {
    NND_REQUIRE(pred && gt && workspace && out, "depth_eval: null pointer");
    NND_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "depth_eval: bad shape (%d,1,%d,%d)", B, H, W);
    NND_REQUIRE((int64_t)B * H * W < ((int64_t)1 << 31), "depth_eval: bad shape (%d,1,%d,%d): B*H*W must be below 2^31", B, H, W);
    NND_REQUIRE(workspace_bytes >= de_ws_doubles(B) * (int64_t)sizeof(double),
                "depth_eval: workspace of %lld bytes, nnd_depth_eval_workspace_bytes(%d) = %lld", (long long)workspace_bytes, B,
                (long long)(de_ws_doubles(B) * (int64_t)sizeof(double)));
    NND_REQUIRE(((uintptr_t)workspace & 7) == 0, "depth_eval: the workspace must be 8-byte aligned");
    DeIn a;
    a.pred = pred, a.gt = gt, a.mask = valid_mask;
    a.HW = (long)H * W;
    a.lo = 0.1f, a.hi = max_depth;
    const DeWs w = de_ws(workspace, B);
    const int G = (int)(cdiv64(a.HW, DE_T) < DE_GMAX ? cdiv64(a.HW, DE_T) : DE_GMAX);
    const dim3 grid(G, B), blk(DE_T);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(de_fit_mean_kernel, grid, blk, 0, s, a, w.p1);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(de_fit_moment_kernel, grid, blk, 0, s, a, (const double*)w.p1, w.p2);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(de_metrics_kernel, grid, blk, 0, s, a, (const double*)w.p1, (const double*)w.p2, w.fit, w.p3);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(de_median_kernel, dim3(2, B), dim3(DE_MED_T), 0, s, a, G, (const double*)w.fit, (const double*)w.p3, w.med);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(de_ssi_scale_kernel, grid, blk, 0, s, a, (const double*)w.fit, (const double*)w.p3, (const double*)w.med, w.p5);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(de_ssi_error_kernel, grid, blk, 0, s, a, (const double*)w.fit, (const double*)w.p3, (const double*)w.med,
                       (const double*)w.p5, w.p6);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(de_final_kernel, dim3(1), dim3(64), 0, s, (const double*)w.p3, (const double*)w.p6, G * B, out);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_depth_eval_accumulate(const double* metrics, double* sums, double* counts, void* stream) {
    NND_REQUIRE(metrics && sums && counts, "depth_eval_accumulate: null pointer");
    hipLaunchKernelGGL(de_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, metrics, sums, counts);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

}  // extern "C"
