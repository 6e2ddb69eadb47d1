// The value of the monocular training loss on the device: what the trainer's validation loop scores a checkpoint on,
// with no host round trip between the model's prediction and the four numbers.  Forward only.
//
//   midas_loss            : MiDasLoss.forward  nndepth/models/midas/loss.py:62-221 (mae_loss, trim_loss, average_loss,
//                           gradient_regulizer) with scale_shift_estimation / ssi_depth / normalize_01_depth  loss.py:6-59
//   midas_loss_accumulate : the validation loop's lists  nndepth/models/midas/trainer.py:341-350
//
// Like depth_eval.hip a chain of small launches (grid = (G blocks, B samples) unless said otherwise), every one a per-block partial
// in double that the NEXT launch adds up in index order (eval_chain.h):
//
//   1 stats    n_b, min / max of t over the valid pixels                                             -> P1[b][blk][3]
//   2 median   grid (2 maps, B), one workgroup each: the lower median of the sample's raw fp32 t, and of its p, over the valid
//              pixels (rank_select on the fp32 key; t -> tn is increasing, so tn's median is the normalised one); NaN for a sample
//              without a valid pixel                                                                 -> MED[b][2]
//   3 scale    batch-global tmin / tmax from P1; sum |tn - shift_t|, sum |p - shift_p|              -> P2[b][blk][2]
//   4 level 0  scales from P2 (0 -> 1); e = |sp - st| of every valid pixel -> E (one double per pixel) and its sum; the gradient
//              term of level 0; T, P, M of level 1 (2x2 max pool with the mask at the arg-max, 2x2 mean)
//                                                                                                    -> PE[b][blk][2], L1
//   5-7 level 1, 2, 3  the gradient term of the level from its maps in the workspace; the next level's maps (not after level 3)
//                                                                                                    -> PG[l][b][blk], L2, L3
//   8 trim     grid (B), one workgroup each: k_b = n_b - (int64)(n_b * 0.1) computed here; tau = the e of rank k_b - 1
//              (rank_select on the 64-bit key of the double); sum of e < tau + (k_b - count) * tau   -> TR[b][2]
//   9 final    one block of five waves, one per quantity: everything added in (level, sample, block) order -> the six doubles
//
// The pooled levels are WRITTEN to the workspace (together less than a third of a map in elements) rather than recomputed per tile
// with a halo: every level's kernel is then the same short loop, and level l+1's arg-max mask needs no 8x8-aligned tiling.
// Every loop's trip count is fixed by the shape, no kernel waits on another workgroup, nothing retries, no floating-point atomics:
// the six doubles are the same bits run to run.  Every workspace element that is read was written earlier in the same call.
// Inputs are fp32; everything after the load is double.  Compiled with -ffp-contract=off.
#include "eval_chain.h"

namespace nnd {

constexpr int ML_SEL_T = 1024;  // threads of a select workgroup
constexpr int ML_MED_U = 8;     // pixels a median thread has in flight
constexpr int ML_TRIM_U = 8;    // ... a trim thread
constexpr int ML_N1 = 3, ML_N2 = 2, ML_NE = 2;
constexpr int ML_LEVELS = 4;
enum { S_CNT = 0, S_TMIN, S_TMAX };

struct MlIn {
    const float* pred;  // (b, y, x) at pred[b * psb + y * psy + x]
    long psb, psy;
    const float* tgt;           // contiguous
    const unsigned char* mask;  // contiguous
    int H, W;
    long HW;
};

struct MlWs {
    double *p1, *med, *p2, *pe, *pg[ML_LEVELS - 1], *tr, *e, *T[ML_LEVELS - 1], *P[ML_LEVELS - 1];
    unsigned char* M[ML_LEVELS - 1];
    long hw[ML_LEVELS];  // pixels of a map of level l
};
static inline int64_t ml_coarse_pixels(int H, int W) {
    int64_t n = 0;
    for (int l = 1; l < ML_LEVELS; ++l) n += (int64_t)(H >> l) * (W >> l);
    return n;
}
static inline int64_t ml_ws_bytes(int B, int H, int W) {
    const int64_t doubles = (int64_t)B * (DE_GMAX * (ML_N1 + ML_N2 + ML_NE + (ML_LEVELS - 1)) + 4) + (int64_t)B * H * W +
                            2 * (int64_t)B * ml_coarse_pixels(H, W);
    return doubles * 8 + (((int64_t)B * ml_coarse_pixels(H, W) + 7) & ~(int64_t)7);
}
static inline MlWs ml_ws(void* workspace, int B, int H, int W) {
    MlWs w;
    double* p = (double*)workspace;
    w.p1 = p, p += (int64_t)B * DE_GMAX * ML_N1;
    w.med = p, p += (int64_t)B * 2;
    w.p2 = p, p += (int64_t)B * DE_GMAX * ML_N2;
    w.pe = p, p += (int64_t)B * DE_GMAX * ML_NE;
    for (int l = 0; l < ML_LEVELS - 1; ++l) w.pg[l] = p, p += (int64_t)B * DE_GMAX;
    w.tr = p, p += (int64_t)B * 2;
    w.e = p, p += (int64_t)B * H * W;
    w.hw[0] = (long)H * W;
    for (int l = 1; l < ML_LEVELS; ++l) {
        w.hw[l] = (long)(H >> l) * (W >> l);
        w.T[l - 1] = p, p += (int64_t)B * w.hw[l];
        w.P[l - 1] = p, p += (int64_t)B * w.hw[l];
    }
    unsigned char* m = (unsigned char*)p;
    for (int l = 1; l < ML_LEVELS; ++l) w.M[l - 1] = m, m += (int64_t)B * w.hw[l];
    return w;
}

__global__ void __launch_bounds__(DE_T) ml_stats_kernel(MlIn a, double* __restrict__ p1) {
    __shared__ double sh[DE_T][ML_N1];
    const int b = blockIdx.y;
    const float* t = a.tgt + (long)b * a.HW;
    const unsigned char* m = a.mask + (long)b * a.HW;
    double cnt = 0.0, lo = INFINITY, hi = -INFINITY;
    for (long i = (long)blockIdx.x * DE_T + threadIdx.x; i < a.HW; i += (long)gridDim.x * DE_T)
        if (m[i]) {
            const double td = (double)t[i];
            cnt += 1.0;
            lo = fmin(lo, td);
            hi = fmax(hi, td);
        }
    sh[threadIdx.x][S_CNT] = cnt, sh[threadIdx.x][S_TMIN] = lo, sh[threadIdx.x][S_TMAX] = hi;
    __syncthreads();
    for (int st = DE_T / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            double* x = sh[threadIdx.x];
            const double* y = sh[threadIdx.x + st];
            x[S_CNT] += y[S_CNT];
            x[S_TMIN] = fmin(x[S_TMIN], y[S_TMIN]);
            x[S_TMAX] = fmax(x[S_TMAX], y[S_TMAX]);
        }
        __syncthreads();
    }
    if (threadIdx.x < ML_N1) p1[((long)b * gridDim.x + blockIdx.x) * ML_N1 + threadIdx.x] = sh[0][threadIdx.x];
}

// blockIdx.x: 0 = target, 1 = prediction; blockIdx.y: sample.  med[2b + map] = the raw fp32 value at position (n_b - 1) / 2 of the
// sample's sorted valid values; NaN if it has none (the median of nothing, loss.py:22)
__global__ void __launch_bounds__(ML_SEL_T) ml_median_kernel(MlIn a, int G, const double* __restrict__ p1, double* __restrict__ med) {
    __shared__ RankSelectLds<unsigned> lds;
    __shared__ long s_n;
    const int map = blockIdx.x, b = blockIdx.y;
    if (threadIdx.x == 0) {
        double n = 0.0;
        for (int k = 0; k < G; ++k) n += p1[((long)b * G + k) * ML_N1 + S_CNT];
        s_n = (long)n;
    }
    __syncthreads();
    const long n = s_n;
    if (n == 0) {  // the whole block
        if (threadIdx.x == 0) med[2 * b + map] = (double)NAN;
        return;
    }
    const float* t = a.tgt + (long)b * a.HW;
    const float* p = a.pred + (long)b * a.psb;
    const unsigned char* m = a.mask + (long)b * a.HW;
    const int W = a.W;
    const long psy = a.psy;
    const unsigned key = rank_select<unsigned, ML_SEL_T, ML_MED_U>(
        a.HW, (unsigned)((n - 1) / 2),
        [&](long i, unsigned& k) {
            const int ii = (int)i, y = ii / W, x = ii - y * W;
            k = de_key(map ? p[(long)y * psy + x] : t[i]);
            return m[i] != 0;
        },
        lds);
    if (threadIdx.x == 0) med[2 * b + map] = (double)de_unkey(key);
}

// the batch's min / max of t over its valid pixels, from every sample's partials: r[0] = tmin, r[1] = tmax
__device__ __forceinline__ void ml_global_range(const double* __restrict__ p1, int nparts, double (*sh)[2], double* r) {
    double lo = INFINITY, hi = -INFINITY;
    for (int k = threadIdx.x; k < nparts; k += DE_T) {
        lo = fmin(lo, p1[(long)k * ML_N1 + S_TMIN]);
        hi = fmax(hi, p1[(long)k * ML_N1 + S_TMAX]);
    }
    sh[threadIdx.x][0] = lo, sh[threadIdx.x][1] = hi;
    __syncthreads();
    for (int st = DE_T / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            sh[threadIdx.x][0] = fmin(sh[threadIdx.x][0], sh[threadIdx.x + st][0]);
            sh[threadIdx.x][1] = fmax(sh[threadIdx.x][1], sh[threadIdx.x + st][1]);
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) r[threadIdx.x] = sh[0][threadIdx.x];
    __syncthreads();
}

__global__ void __launch_bounds__(DE_T) ml_scale_kernel(MlIn a, const double* __restrict__ p1, const double* __restrict__ med,
                                                        double* __restrict__ p2) {
    __shared__ double sh[DE_T][ML_N2];
    __shared__ double shr[DE_T][2];
    __shared__ double r[2];
    const int b = blockIdx.y, G = gridDim.x;
    ml_global_range(p1, G * gridDim.y, shr, r);
    const double tmin = r[0], den = r[1] - r[0] + 1e-6;  // normalize_01_depth (loss.py:56-58)
    const double sh_t = (med[2 * b] - tmin) / den, sh_p = med[2 * b + 1];
    const float* t = a.tgt + (long)b * a.HW;
    const float* p = a.pred + (long)b * a.psb;
    const unsigned char* m = a.mask + (long)b * a.HW;
    double acc[ML_N2] = {0.0, 0.0};
    for (long i = (long)blockIdx.x * DE_T + threadIdx.x; i < a.HW; i += (long)gridDim.x * DE_T)
        if (m[i]) {
            const int ii = (int)i, y = ii / a.W, x = ii - y * a.W;
            acc[0] += fabs(((double)t[i] - tmin) / den - sh_t);
            acc[1] += fabs((double)p[(long)y * a.psy + x] - sh_p);
        }
    de_block_sum<ML_N2>(acc, sh);
    if (threadIdx.x < ML_N2) p2[((long)b * G + blockIdx.x) * ML_N2 + threadIdx.x] = sh[0][threadIdx.x];
}

// the first maximum of the 2x2 window in row-major order, a NaN wins: max_pool2d(return_indices=True), as pool_abs_kernel of
// scene.hip restates it.  v[0..4) in window order; returns the position in the window
__device__ __forceinline__ int ml_argmax4(const double (&v)[4], double& best) {
    best = -INFINITY;
    int at = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (v[k] > best || v[k] != v[k]) {
            best = v[k];
            at = k;
        }
    return at;
}

// G blocks per sample also serve level 1's pool: the grid is sized for level 0
__global__ void __launch_bounds__(DE_T) ml_level0_kernel(MlIn a, const double* __restrict__ p1, const double* __restrict__ med,
                                                         const double* __restrict__ p2, double* __restrict__ e_out, double* __restrict__ T1,
                                                         double* __restrict__ P1, unsigned char* __restrict__ M1, double* __restrict__ pe) {
    __shared__ double sh[DE_T][ML_NE];
    __shared__ double shr[DE_T][2];
    __shared__ double r[2], t1[ML_N1], t2[ML_N2];
    const int b = blockIdx.y, G = gridDim.x;
    ml_global_range(p1, G * gridDim.y, shr, r);
    de_sum_partials<ML_N1>(p1 + (long)b * G * ML_N1, G, t1);  // only the count is a sum; the other slots are not read
    de_sum_partials<ML_N2>(p2 + (long)b * G * ML_N2, G, t2);
    const double n = t1[S_CNT];
    const double tmin = r[0], den = r[1] - r[0] + 1e-6;
    const double sh_t = (med[2 * b] - tmin) / den, sh_p = med[2 * b + 1];
    double sc_t = t2[0] / n, sc_p = t2[1] / n;  // scale_shift_estimation (loss.py:23); a sample without a valid pixel: NaN, as there
    if (sc_t == 0.0) sc_t = 1.0;                // ssi_depth: scale[scale == 0] = 1
    if (sc_p == 0.0) sc_p = 1.0;
    const float* t = a.tgt + (long)b * a.HW;
    const float* p = a.pred + (long)b * a.psb;
    const unsigned char* m = a.mask + (long)b * a.HW;
    const int H = a.H, W = a.W;
    const long psy = a.psy;
    auto Tn = [&](long i) { return ((double)t[i] - tmin) / den; };
    auto Tz = [&](long i) { return m[i] ? Tn(i) : 0.0; };  // normalized_target[~valid_mask] = 0 (loss.py:150)
    auto Pv = [&](int y, int x) { return ((double)p[(long)y * psy + x] - sh_p) / sc_p; };
    auto Rv = [&](int y, int x) { return Pv(y, x) - Tz((long)y * W + x); };
    double acc[ML_NE] = {0.0, 0.0};
    double* eb = e_out + (long)b * a.HW;
    for (long i = (long)blockIdx.x * DE_T + threadIdx.x; i < a.HW; i += (long)gridDim.x * DE_T) {
        const int ii = (int)i, y = ii / W, x = ii - y * W;
        if (m[i]) {
            const double e = fabs(Pv(y, x) - (Tn(i) - sh_t) / sc_t);
            eb[i] = e;
            acc[0] += e;
        }
        if (y < H - 1 && x < W - 1 && m[i + W + 1]) {  // the reference's shifted mask valid_mask[1:, 1:] (loss.py:156), selected
            const double r0 = Rv(y, x);
            acc[1] += fabs(r0 - Rv(y, x + 1)) + fabs(r0 - Rv(y + 1, x));
        }
    }
    const int h1 = H >> 1, w1 = W >> 1;
    const long hw1 = (long)h1 * w1;
    for (long j = (long)blockIdx.x * DE_T + threadIdx.x; j < hw1; j += (long)gridDim.x * DE_T) {
        const int jj = (int)j, oy = jj / w1, ox = jj - oy * w1, y = 2 * oy, x = 2 * ox;
        const long i00 = (long)y * W + x;
        const long at[4] = {i00, i00 + 1, i00 + W, i00 + W + 1};
        const double tv[4] = {Tz(at[0]), Tz(at[1]), Tz(at[2]), Tz(at[3])};
        double best;
        const int k = ml_argmax4(tv, best);
        T1[(long)b * hw1 + j] = best;
        M1[(long)b * hw1 + j] = m[at[k]];
        P1[(long)b * hw1 + j] = (((Pv(y, x) + Pv(y, x + 1)) + Pv(y + 1, x)) + Pv(y + 1, x + 1)) / 4.0;
    }
    de_block_sum<ML_NE>(acc, sh);
    if (threadIdx.x < ML_NE) pe[((long)b * G + blockIdx.x) * ML_NE + threadIdx.x] = sh[0][threadIdx.x];
}

struct MlLevel {
    const double *T, *P;
    const unsigned char* M;
    int h, w;
    double *Tn, *Pn;  // the next level's maps; null after the last level
    unsigned char* Mn;
};

__global__ void __launch_bounds__(DE_T) ml_level_kernel(MlLevel a, double* __restrict__ pg) {
    __shared__ double sh[DE_T][1];
    const int b = blockIdx.y, G = gridDim.x, h = a.h, w = a.w;
    const long hw = (long)h * w;
    const double* T = a.T + (long)b * hw;
    const double* P = a.P + (long)b * hw;
    const unsigned char* M = a.M + (long)b * hw;
    double acc[1] = {0.0};
    for (long i = (long)blockIdx.x * DE_T + threadIdx.x; i < hw; i += (long)gridDim.x * DE_T) {
        const int ii = (int)i, y = ii / w, x = ii - y * w;
        if (y < h - 1 && x < w - 1 && M[i + w + 1]) {
            const double r0 = P[i] - T[i];
            acc[0] += fabs(r0 - (P[i + 1] - T[i + 1])) + fabs(r0 - (P[i + w] - T[i + w]));
        }
    }
    if (a.Tn) {
        const int h1 = h >> 1, w1 = w >> 1;
        const long hw1 = (long)h1 * w1;
        for (long j = (long)blockIdx.x * DE_T + threadIdx.x; j < hw1; j += (long)gridDim.x * DE_T) {
            const int jj = (int)j, oy = jj / w1, ox = jj - oy * w1;
            const long i00 = (long)(2 * oy) * w + 2 * ox;
            const long at[4] = {i00, i00 + 1, i00 + w, i00 + w + 1};
            const double tv[4] = {T[at[0]], T[at[1]], T[at[2]], T[at[3]]};
            double best;
            const int k = ml_argmax4(tv, best);
            a.Tn[(long)b * hw1 + j] = best;
            a.Mn[(long)b * hw1 + j] = M[at[k]];
            a.Pn[(long)b * hw1 + j] = (((P[at[0]] + P[at[1]]) + P[at[2]]) + P[at[3]]) / 4.0;
        }
    }
    de_block_sum<1>(acc, sh);
    if (threadIdx.x == 0) pg[(long)b * G + blockIdx.x] = sh[0][0];
}

// blockIdx.x: sample.  tr[2b] = the sum of the sample's k_b smallest e, tr[2b + 1] = k_b; both 0 if int(n_b * 0.1) == 0: the
// reference's loss[:-0] is empty (loss.py:99-101)
__global__ void __launch_bounds__(ML_SEL_T) ml_trim_kernel(const double* __restrict__ e_in, const unsigned char* __restrict__ mask, long HW,
                                                           int G, const double* __restrict__ p1, double* __restrict__ tr) {
    __shared__ RankSelectLds<unsigned long long> lds;
    __shared__ double shs[ML_SEL_T];
    __shared__ unsigned shc[ML_SEL_T];
    __shared__ long s_k;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        double n = 0.0;
        for (int k = 0; k < G; ++k) n += p1[((long)b * G + k) * ML_N1 + S_CNT];
        const long trim = (long)(n * 0.1);  // int(loss.shape[-1] * trim_ratio), on the device: n_b is device data
        s_k = trim == 0 ? 0 : (long)n - trim;
    }
    __syncthreads();
    const long k = s_k;
    if (k == 0) {  // the whole block
        if (threadIdx.x == 0) tr[2 * b] = 0.0, tr[2 * b + 1] = 0.0;
        return;
    }
    const double* e = e_in + (long)b * HW;
    const unsigned char* m = mask + (long)b * HW;
    const unsigned long long key = rank_select<unsigned long long, ML_SEL_T, ML_TRIM_U>(
        HW, (unsigned)(k - 1),
        [&](long i, unsigned long long& kk) {
            const bool ok = m[i] != 0;
            kk = de_key(ok ? e[i] : 0.0);  // E holds a value only where the mask is set
            return ok;
        },
        lds);
    const double tau = de_unkey(key);
    double s = 0.0;
    unsigned c = 0u;
    for (long i = threadIdx.x; i < HW; i += ML_SEL_T)
        if (m[i]) {
            const double v = e[i];
            if (v < tau) s += v, c += 1u;
        }
    shs[threadIdx.x] = s, shc[threadIdx.x] = c;
    __syncthreads();
    for (int st = ML_SEL_T / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) shs[threadIdx.x] += shs[threadIdx.x + st], shc[threadIdx.x] += shc[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        tr[2 * b] = shs[0] + (double)(k - (long)shc[0]) * tau;  // the values equal to tau that fill the k_b places
        tr[2 * b + 1] = (double)k;
    }
}

struct MlFinal {
    const double *p1, *pe, *pg[ML_LEVELS - 1], *tr;
    int B, G[ML_LEVELS];
    double c_trim, c_grad;
};

// s + part[off], part[stride + off], ... (n values) added in index order; every lane of the wave returns the same sum.  64 values are
// loaded at a time, one per lane, and read back lane by lane: the order of the additions is the index order, the loads are not a
// chain of dependent round trips to memory
__device__ __forceinline__ double ml_wave_ordered_sum(double s, const double* __restrict__ part, int stride, int off, int n) {
    const int lane = threadIdx.x & 63;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int k = c0 + lane, m = n - c0 < 64 ? n - c0 : 64;
        const double v = k < n ? part[(long)k * stride + off] : 0.0;
        for (int l = 0; l < m; ++l) s += __shfl(v, l);
    }
    return s;
}

// one block of five waves, wave q adds quantity q: n, sum e, the gradient sums, sum_b sum_b, sum_b k_b
__global__ void __launch_bounds__(320) ml_final_kernel(MlFinal a, double* __restrict__ out) {
    __shared__ double t[5];
    const int q = threadIdx.x >> 6;
    const int n0 = a.B * a.G[0];
    double s = 0.0;
    if (q == 0)
        s = ml_wave_ordered_sum(s, a.p1, ML_N1, S_CNT, n0);
    else if (q == 1)
        s = ml_wave_ordered_sum(s, a.pe, ML_NE, 0, n0);
    else if (q == 2) {
        s = ml_wave_ordered_sum(s, a.pe, ML_NE, 1, n0);
        for (int l = 1; l < ML_LEVELS; ++l) s = ml_wave_ordered_sum(s, a.pg[l - 1], 1, 0, a.B * a.G[l]);
    } else
        s = ml_wave_ordered_sum(s, a.tr, 2, q - 3, a.B);
    if ((threadIdx.x & 63) == 0) t[q] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double n = t[0];
    if (n == 0.0) {  // the reference raises here; the device answers NaN and two zero counts
        for (int i = 0; i < 4; ++i) out[i] = (double)NAN;
        out[4] = 0.0, out[5] = 0.0;
        return;
    }
    const double trimmed = t[3] / t[4], grad = t[2] / n;  // 0 / 0 = NaN: no sample with 10 valid pixels (average_loss of nothing)
    out[0] = trimmed * a.c_trim + grad * a.c_grad;
    out[1] = trimmed;
    out[2] = grad;
    out[3] = t[1] / n;
    out[4] = n;
    out[5] = t[4];
}

__global__ void ml_accumulate_kernel(const double* __restrict__ values, double* __restrict__ sums, double* __restrict__ count) {
    const int i = threadIdx.x;
    if (i < 6) sums[i] += values[i];
    if (i == 6) count[0] += 1.0;
}

static inline int ml_grid(long hw) { return (int)(cdiv64(hw, DE_T) < DE_GMAX ? cdiv64(hw, DE_T) : DE_GMAX); }

static int ml_check_shape(const char* what, int B, int H, int W) {
    NND_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "%s: bad shape (%d,1,%d,%d)", what, B, H, W);
    NND_REQUIRE(H >= 16 && W >= 16, "%s: bad shape (%d,1,%d,%d): H and W must be at least 16 (four levels of 2x2 pooling)", what, B, H, W);
    NND_REQUIRE((int64_t)B * H * W < ((int64_t)1 << 31), "%s: bad shape (%d,1,%d,%d): B*H*W must be below 2^31", what, B, H, W);
    return NND_OK;
}

}  // namespace nnd

using namespace nnd;

extern "C" {

int64_t nnd_midas_loss_workspace_bytes(int B, int H, int W) {
    const int rc = ml_check_shape("midas_loss_workspace_bytes", B, H, W);
    if (rc != NND_OK) return (int64_t)rc;
    return ml_ws_bytes(B, H, W);
}

int nnd_midas_loss(const float* pred, const float* target, const unsigned char* valid_mask, int B, int H, int W, int64_t pred_stride_b,
                   int64_t pred_stride_row, double trimmed_coef, double gradient_coef, void* workspace, int64_t workspace_bytes,
                   double* out, void* stream) {
    NND_REQUIRE(pred && target && valid_mask && workspace && out, "midas_loss: null pointer (the valid mask is required)");
    int rc;
    NND_TRY(ml_check_shape("midas_loss", B, H, W));
    NND_REQUIRE(pred_stride_row >= W && pred_stride_b >= 0, "midas_loss: bad strides of pred (batch %lld, row %lld; rows may not overlap)",
                (long long)pred_stride_b, (long long)pred_stride_row);
    NND_REQUIRE(workspace_bytes >= ml_ws_bytes(B, H, W), "midas_loss: workspace of %lld bytes, nnd_midas_loss_workspace_bytes(%d,%d,%d) = %lld",
                (long long)workspace_bytes, B, H, W, (long long)ml_ws_bytes(B, H, W));
    NND_REQUIRE(((uintptr_t)workspace & 7) == 0, "midas_loss: the workspace must be 8-byte aligned");
    MlIn a;
    a.pred = pred, a.psb = (long)pred_stride_b, a.psy = (long)pred_stride_row;
    a.tgt = target, a.mask = valid_mask;
    a.H = H, a.W = W, a.HW = (long)H * W;
    const MlWs w = ml_ws(workspace, B, H, W);
    MlFinal f;
    for (int l = 0; l < ML_LEVELS; ++l) f.G[l] = ml_grid(w.hw[l]);
    const int G = f.G[0];
    const dim3 grid(G, B), blk(DE_T);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ml_stats_kernel, grid, blk, 0, s, a, w.p1);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(ml_median_kernel, dim3(2, B), dim3(ML_SEL_T), 0, s, a, G, (const double*)w.p1, w.med);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(ml_scale_kernel, grid, blk, 0, s, a, (const double*)w.p1, (const double*)w.med, w.p2);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(ml_level0_kernel, grid, blk, 0, s, a, (const double*)w.p1, (const double*)w.med, (const double*)w.p2, w.e, w.T[0],
                       w.P[0], w.M[0], w.pe);
    NND_LAUNCH_CHECK();
    for (int l = 1; l < ML_LEVELS; ++l) {
        MlLevel lv;
        lv.T = w.T[l - 1], lv.P = w.P[l - 1], lv.M = w.M[l - 1];
        lv.h = H >> l, lv.w = W >> l;
        const bool last = l == ML_LEVELS - 1;
        lv.Tn = last ? nullptr : w.T[l], lv.Pn = last ? nullptr : w.P[l], lv.Mn = last ? nullptr : w.M[l];
        hipLaunchKernelGGL(ml_level_kernel, dim3(f.G[l], B), blk, 0, s, lv, w.pg[l - 1]);
        NND_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ml_trim_kernel, dim3(B), dim3(ML_SEL_T), 0, s, (const double*)w.e, valid_mask, a.HW, G, (const double*)w.p1, w.tr);
    NND_LAUNCH_CHECK();
    f.p1 = w.p1, f.pe = w.pe, f.tr = w.tr;
    for (int l = 0; l < ML_LEVELS - 1; ++l) f.pg[l] = w.pg[l];
    f.B = B;
    f.c_trim = trimmed_coef, f.c_grad = gradient_coef;
    hipLaunchKernelGGL(ml_final_kernel, dim3(1), dim3(320), 0, s, f, out);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_midas_loss_accumulate(const double* values, double* sums, double* count, void* stream) {
    NND_REQUIRE(values && sums && count, "midas_loss_accumulate: null pointer");
    hipLaunchKernelGGL(ml_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, values, sums, count);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

}  // extern "C"
