// The stereo evaluation criterion on the device for every output of a forward in one call.
//
//   stereo_eval            : EvalCriterion.__call__  nndepth/models/raft_stereo/scripts/evaluate.py:48-83 (the same lines in
//                            igev_stereo/ and cre_stereo/scripts/evaluate.py) per output, and the sequence loss with its
//                            metrics, RAFTLoss / CREStereoLoss  nndepth/models/raft_stereo/loss.py:15-52
//   stereo_eval_accumulate : the dataset mean's bookkeeping  nndepth/models/raft_stereo/scripts/evaluate.py:141-169
//   min_pool_nearest       : the ground truth at a coarse output's size  evaluate.py:63-66, loss.py:23-26
//
// Outputs are grouped by (C, h, w); a group is ONE launch of se_partial_kernel, grid = (G pixel tiles, outputs of the group),
// and one launch of se_final_kernel reduces every group: 2 launches for a RAFT-Stereo forward, 4 for CREStereo's three sizes,
// however many maps there are.  The per-output pointers and strides travel in the kernel arguments (no table on the device, no
// copy).  A workgroup leaves one partial in the workspace: the sums of epe and of valid * |p - g| in double, and the counts
// (valid pixels, epe > above[k], epe < below[k]) as 32-bit integers; the final kernel adds the partials of an output in index
// order (counts in 64 bits) and divides.  Every loop's trip count is fixed by the shapes, nothing waits on another workgroup, no
// floating-point atomics: the same bits run to run, and a row does not depend on which other outputs share the call.
//
// A thread's unit of work is a quad: 4 consecutive pixels of a row (the last quad of a row may be ragged).  The quad -> thread
// assignment depends on (B, h, w) alone, and the 16-byte path (rows, strides and base pointers that allow it) differs from the
// scalar path in the loads only, so a cropped view gives the bits of its contiguous copy.
//
// Compiled with -ffp-contract=off: d * d and g * g are rounded products added in channel order, as torch.sum(x ** 2, dim=1) has
// them; sqrtf and the division by (float)s are correctly rounded.
#include "common.h"

namespace nnd {

constexpr int SE_T = 256;                              // threads of a partial workgroup
constexpr int SE_GMAX = 64;                            // workgroups (partials) per output at most
constexpr int SE_MAXO = NND_STEREO_EVAL_MAX_OUTPUTS;   // 64
constexpr int SE_NTHR = NND_STEREO_EVAL_MAX_THRESHOLDS;  // 8 per side
constexpr int SE_NCNT = 1 + 2 * SE_NTHR;               // valid, above[8], below[8]
constexpr int SE_NSUM = 2;                             // sum epe, sum valid * |p - g|
constexpr int SE_SLOT = SE_NSUM + (SE_NCNT + 1) / 2;   // a partial, in 8-byte words: 2 doubles, 17 (+1) uint32
constexpr int SE_FINAL_T = 1024;

static inline int64_t se_ws_bytes(int n) { return (int64_t)n * SE_GMAX * SE_SLOT * 8; }

struct SeOut {
    const float* p;
    long sb, sc, sr;  // batch, channel and row strides in elements
};

struct SeGroup {  // one size group: the arguments of one partial launch
    const float* gt;
    const unsigned char* mask;  // (B, h, w) bytes or null
    int Cg, H, W;               // of the ground truth
    int Cp, h, w;               // of the group's outputs
    int s, Hp, Wp;              // pool size, pooled map
    float fs, ry, rx;           // (float)s; (float)Hp / h, (float)Wp / w: nearest_idx of F.interpolate
    int Wq, nquads, G;          // quads per row, in all, workgroups per output
    float max_flow;
    float above[SE_NTHR], below[SE_NTHR];  // unused entries: +inf / -inf (never counted)
    unsigned char slot[SE_MAXO];           // index of the output in the call: where its partials go
    unsigned char vec[SE_MAXO];            // 16-byte loads are allowed for this output (and the group's gt / mask)
    SeOut outs[SE_MAXO];
};

struct SeFinal {
    int N, K, n_above, n_below;
    int G[SE_MAXO];
    double elems[SE_MAXO];  // B * C * h * w
    double wgt[SE_MAXO];    // gamma^(N - 1 - i)
};

// the source index F.interpolate(mode="nearest") picks (UpSampleKernel.cpp: nearest_idx); ratio = (float)in / (float)out
__device__ __forceinline__ int se_nearest(int dst, float ratio, int in) {
    const int v = (int)floorf((float)dst * ratio);
    return v < in - 1 ? v : in - 1;
}

// -max_pool2d(-gt, s)[sy][sx] / s on one plane: max over the window in row-major order, NaN wins (as torch's kernel has it)
__device__ __forceinline__ float se_pool(const float* __restrict__ plane, int W, int s, float fs, int sy, int sx) {
    const float* p = plane + (long)sy * s * W + (long)sx * s;
    float best = -INFINITY;
    for (int dy = 0; dy < s; ++dy)
        for (int dx = 0; dx < s; ++dx) {
            const float v = -p[(long)dy * W + dx];
            if (v > best || v != v) best = v;
        }
    return (-best) / fs;
}

template <class T>
__device__ __forceinline__ T se_wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

struct SeAcc {  // a thread's sums
    double es, l1;
    unsigned cnt, ab[SE_NTHR], be[SE_NTHR];
};

struct SeQuad {  // the per-pixel values of one quad
    float se[4], sg[4];  // sum_c (p_c - g_c)^2, sum_c g_c^2
    double t[4];         // sum_c |p_c - g_c|
    unsigned mk;         // the four mask bytes
    int nv;              // pixels of the quad inside the row
};

// Loads quad q of output o and takes the fp32 steps.  CP / CG: the channel counts when they are known at compile time (CP == 0:
// a.Cp, a.Cg); VEC: 16-byte loads; MASK: a mask is given.  No branch in the VEC instances, so the loads of several quads can be
// in flight together.
template <bool SAME, int CP, int CG, bool VEC, bool MASK>
__device__ __forceinline__ void se_fetch(const SeGroup& a, const SeOut& o, int q, SeQuad& r) {
    const int Cp = CP ? CP : a.Cp, Cg = CP ? CG : a.Cg;
    const int row = q / a.Wq, x0 = (q - row * a.Wq) * 4;
    const int b = row / a.h, y = row - b * a.h;
    const int nv = VEC ? 4 : (a.w - x0 < 4 ? a.w - x0 : 4);
    r.nv = nv;
    r.mk = 0x01010101u;
    if (MASK) {
        const unsigned char* mp = a.mask + ((long)b * a.h + y) * a.w + x0;
        if (VEC) {
            r.mk = *(const unsigned*)mp;
        } else {
            r.mk = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) r.mk |= (j < nv ? (unsigned)mp[j] : 0u) << (8 * j);
        }
    }
    int sy = 0, sx[4] = {0, 0, 0, 0};
    if (!SAME) {
        sy = se_nearest(y, a.ry, a.Hp);
#pragma unroll
        for (int j = 0; j < 4; ++j) sx[j] = se_nearest(x0 + j < a.w ? x0 + j : a.w - 1, a.rx, a.Wp);
    }
    float gv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) r.se[j] = 0.f, r.sg[j] = 0.f, r.t[j] = 0.0;
    const long gplane = (long)a.H * a.W;
    for (int c = 0; c < Cp; ++c) {  // a constant trip count where CP != 0: unrolled
        if (c < Cg) {  // Cg == 1: the one channel, loaded once, serves every output channel
            const float* gp = a.gt + ((long)b * Cg + c) * gplane;
            if (SAME) {
                gp += (long)y * a.W + x0;
                if (VEC) {
                    const float4 v = *(const float4*)gp;
                    gv[0] = v.x, gv[1] = v.y, gv[2] = v.z, gv[3] = v.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) gv[j] = j < nv ? gp[j] : 0.f;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) gv[j] = se_pool(gp, a.W, a.s, a.fs, sy, sx[j]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) r.sg[j] += gv[j] * gv[j];
        }
        const float* pp = o.p + (long)b * o.sb + (long)c * o.sc + (long)y * o.sr + x0;
        float pv[4];
        if (VEC) {
            const float4 v = *(const float4*)pp;
            pv[0] = v.x, pv[1] = v.y, pv[2] = v.z, pv[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) pv[j] = j < nv ? pp[j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = pv[j] - gv[j];
            r.se[j] += d * d;
            r.t[j] += (double)fabsf(d);
        }
    }
}

__device__ __forceinline__ void se_consume(const SeGroup& a, const SeQuad& r, SeAcc& acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float epe = sqrtf(r.se[j]);
        const bool valid = j < r.nv && sqrtf(r.sg[j]) < a.max_flow && ((r.mk >> (8 * j)) & 0xffu) != 0u;
        if (valid) {
            acc.es += (double)epe;
            acc.l1 += r.t[j];
            acc.cnt += 1u;
#pragma unroll
            for (int k = 0; k < SE_NTHR; ++k) {
                acc.ab[k] += epe > a.above[k] ? 1u : 0u;
                acc.be[k] += epe < a.below[k] ? 1u : 0u;
            }
        }
    }
}

// A thread's quads, SE_U per trip where the channel counts are compile-time constants: all their loads are issued before the
// first is consumed.  The quads are consumed in increasing order whatever SE_U is, so every instance adds in the same order.
constexpr int SE_U = 4;
template <bool SAME, int CP, int CG, bool VEC, bool MASK>
__device__ __forceinline__ void se_run(const SeGroup& a, const SeOut& o, SeAcc& acc) {
    const int stride = a.G * SE_T;
    int q = blockIdx.x * SE_T + threadIdx.x;
    if (CP != 0) {
        for (; q + (SE_U - 1) * stride < a.nquads; q += SE_U * stride) {
            SeQuad r[SE_U];
#pragma unroll
            for (int u = 0; u < SE_U; ++u) se_fetch<SAME, CP, CG, VEC, MASK>(a, o, q + u * stride, r[u]);
#pragma unroll
            for (int u = 0; u < SE_U; ++u) se_consume(a, r[u], acc);
        }
    }
    for (; q < a.nquads; q += stride) {
        SeQuad r;
        se_fetch<SAME, CP, CG, VEC, MASK>(a, o, q, r);
        se_consume(a, r, acc);
    }
}

// SAME: the group's outputs have the ground truth's size (g is the ground truth itself); CP, CG: see se_fetch
template <bool SAME, int CP, int CG>
__global__ void __launch_bounds__(SE_T) se_partial_kernel(SeGroup a, double* __restrict__ ws) {
    __shared__ double shd[SE_T / 64][SE_NSUM];
    __shared__ unsigned shu[SE_T / 64][SE_NCNT];
    const int m = blockIdx.y;
    const SeOut o = a.outs[m];
    SeAcc acc;
    acc.es = acc.l1 = 0.0, acc.cnt = 0u;
#pragma unroll
    for (int k = 0; k < SE_NTHR; ++k) acc.ab[k] = acc.be[k] = 0u;
    if (a.vec[m] != 0) {
        if (a.mask) se_run<SAME, CP, CG, true, true>(a, o, acc);
        else se_run<SAME, CP, CG, true, false>(a, o, acc);
    } else {
        if (a.mask) se_run<SAME, CP, CG, false, true>(a, o, acc);
        else se_run<SAME, CP, CG, false, false>(a, o, acc);
    }
    double es = acc.es, l1 = acc.l1;
    unsigned cnt = acc.cnt, ab[SE_NTHR], be[SE_NTHR];
#pragma unroll
    for (int k = 0; k < SE_NTHR; ++k) ab[k] = acc.ab[k], be[k] = acc.be[k];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    es = se_wave_sum(es), l1 = se_wave_sum(l1), cnt = se_wave_sum(cnt);
#pragma unroll
    for (int k = 0; k < SE_NTHR; ++k) ab[k] = se_wave_sum(ab[k]), be[k] = se_wave_sum(be[k]);
    if (lane == 0) {
        shd[wave][0] = es, shd[wave][1] = l1;
        shu[wave][0] = cnt;
#pragma unroll
        for (int k = 0; k < SE_NTHR; ++k) shu[wave][1 + k] = ab[k], shu[wave][1 + SE_NTHR + k] = be[k];
    }
    __syncthreads();
    double* part = ws + ((long)a.slot[m] * SE_GMAX + blockIdx.x) * SE_SLOT;
    const int i = threadIdx.x;
    if (i < SE_NSUM) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < SE_T / 64; ++k) v += shd[k][i];
        part[i] = v;
    } else if (i < SE_NSUM + SE_NCNT) {
        unsigned v = 0u;
#pragma unroll
        for (int k = 0; k < SE_T / 64; ++k) v += shu[k][i - SE_NSUM];
        ((unsigned*)(part + SE_NSUM))[i - SE_NSUM] = v;
    }
}

// one workgroup: a thread per (output, slot) adds the output's partials in index order, then a thread per (output, column)
// divides, and thread 0 adds the weighted l1 terms in output order
__global__ void __launch_bounds__(SE_FINAL_T) se_final_kernel(SeFinal f, const double* __restrict__ ws, double* __restrict__ out) {
    __shared__ double sd[SE_MAXO][SE_NSUM];
    __shared__ unsigned long long su[SE_MAXO][SE_NCNT];
    constexpr int NS = SE_NSUM + SE_NCNT;
    for (int j = threadIdx.x; j < f.N * NS; j += SE_FINAL_T) {
        const int i = j / NS, q = j - i * NS;
        const double* base = ws + (long)i * SE_GMAX * SE_SLOT;
        const int G = f.G[i];
        if (q < SE_NSUM) {  // 16 loads in flight, added in index order
            double s = 0.0;
            for (int k0 = 0; k0 < G; k0 += 16) {
                double v[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) v[k] = base[(long)(k0 + k < G ? k0 + k : 0) * SE_SLOT + q];
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (k0 + k < G) s += v[k];
            }
            sd[i][q] = s;
        } else {
            unsigned long long s = 0ull;
            for (int k0 = 0; k0 < G; k0 += 16) {
                unsigned v[16];
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    v[k] = ((const unsigned*)(base + (long)(k0 + k < G ? k0 + k : 0) * SE_SLOT + SE_NSUM))[q - SE_NSUM];
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (k0 + k < G) s += v[k];
            }
            su[i][q - SE_NSUM] = s;
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < f.N * f.K; j += SE_FINAL_T) {
        const int i = j / f.K, c = j - i * f.K;
        const double n = (double)su[i][0];
        double v;
        if (c == 0) v = sd[i][0] / n;  // no valid pixel: 0 / 0 = NaN, the reference's empty mean
        else if (c == 1) v = n;
        else if (c == 2) v = sd[i][1] / f.elems[i];
        else if (c < 3 + f.n_above) v = (double)su[i][1 + (c - 3)] / n;
        else v = (double)su[i][1 + SE_NTHR + (c - 3 - f.n_above)] / n;
        out[j] = v;
    }
    if (threadIdx.x == 0) {
        double loss = 0.0;
        for (int i = 0; i < f.N; ++i) loss += f.wgt[i] * (sd[i][1] / f.elems[i]);
        out[(long)f.N * f.K] = loss;
    }
}

__global__ void se_accumulate_kernel(const double* __restrict__ metrics, int n, double* __restrict__ sums) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sums[i] += metrics[i];
}

__global__ void __launch_bounds__(256) min_pool_nearest_kernel(const float* __restrict__ gt, float* __restrict__ dst, int H, int W, int h,
                                                               int w, int s, float fs, int Hp, int Wp, float ry, float rx) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= h * w) return;
    const int y = idx / w, x = idx - y * w;
    dst[(long)blockIdx.y * h * w + idx] =
        se_pool(gt + (long)blockIdx.y * H * W, W, s, fs, se_nearest(y, ry, Hp), se_nearest(x, rx, Wp));
}

template <bool SAME>
static void se_launch_partial_same(const SeGroup& g, int n, double* ws, hipStream_t st) {
    const dim3 grid(g.G, n), blk(SE_T);
    if (g.Cp == 1 && g.Cg == 1) hipLaunchKernelGGL((se_partial_kernel<SAME, 1, 1>), grid, blk, 0, st, g, ws);
    else if (g.Cp == 2 && g.Cg == 1) hipLaunchKernelGGL((se_partial_kernel<SAME, 2, 1>), grid, blk, 0, st, g, ws);
    else if (g.Cp == 2 && g.Cg == 2) hipLaunchKernelGGL((se_partial_kernel<SAME, 2, 2>), grid, blk, 0, st, g, ws);
    else hipLaunchKernelGGL((se_partial_kernel<SAME, 0, 0>), grid, blk, 0, st, g, ws);
}
static void se_launch_partial(bool same, const SeGroup& g, int n, double* ws, hipStream_t st) {
    if (same) se_launch_partial_same<true>(g, n, ws, st);
    else se_launch_partial_same<false>(g, n, ws, st);
}

// s, Hp, Wp of a (h, w) output against a (H, W) ground truth; false: refused (the message is set)
static bool se_pool_geometry(const char* what, int H, int W, int h, int w, int* s, int* Hp, int* Wp) {
    *s = W / w;
    if (*s == 0) {
        set_error("%s: an output of %dx%d is wider than the %dx%d ground truth (scale = W_gt // w = 0)", what, h, w, H, W);
        return false;
    }
    *Hp = H / *s, *Wp = W / *s;
    if (*Hp == 0) {
        set_error("%s: a %dx%d ground truth pooled by %d (= W_gt // w for a %dx%d output) has no row left", what, H, W, *s, h, w);
        return false;
    }
    return true;
}

}  // namespace nnd

using namespace nnd;

extern "C" {

int64_t nnd_stereo_eval_workspace_bytes(int num_outputs) {
    if (num_outputs <= 0 || num_outputs > SE_MAXO) {
        set_error("stereo_eval_workspace_bytes: bad number of outputs %d (1 .. %d)", num_outputs, SE_MAXO);
        return (int64_t)NND_ERR_INVALID;
    }
    return se_ws_bytes(num_outputs);
}

int nnd_stereo_eval(const nnd_stereo_eval_desc* d, void* workspace, int64_t workspace_bytes, double* out, void* stream) {
    int rc;
    NND_TRY(check_desc(d, 0u, "stereo_eval"));
    NND_REQUIRE(d->gt && workspace && out, "stereo_eval: null pointer");
    NND_REQUIRE(d->B > 0 && d->Cg > 0 && d->H > 0 && d->W > 0, "stereo_eval: bad ground-truth shape (%d,%d,%d,%d)", d->B, d->Cg, d->H,
                d->W);
    NND_REQUIRE((int64_t)d->B * d->Cg * d->H * d->W < ((int64_t)1 << 31),
                "stereo_eval: bad ground-truth shape (%d,%d,%d,%d): B*C*H*W must be below 2^31", d->B, d->Cg, d->H, d->W);
    const int N = d->num_outputs;
    NND_REQUIRE(N > 0 && N <= SE_MAXO, "stereo_eval: bad number of outputs %d (1 .. %d)", N, SE_MAXO);
    NND_REQUIRE(d->n_above >= 0 && d->n_above <= SE_NTHR && d->n_below >= 0 && d->n_below <= SE_NTHR,
                "stereo_eval: at most %d thresholds per side; got %d above, %d below", SE_NTHR, d->n_above, d->n_below);
    NND_REQUIRE(workspace_bytes >= se_ws_bytes(N), "stereo_eval: workspace of %lld bytes, nnd_stereo_eval_workspace_bytes(%d) = %lld",
                (long long)workspace_bytes, N, (long long)se_ws_bytes(N));
    NND_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out & 7) == 0, "stereo_eval: the workspace and out must be 8-byte aligned");
    NND_REQUIRE(!d->mask || (d->mask_h > 0 && d->mask_w > 0), "stereo_eval: bad valid_mask size %dx%d", d->mask_h, d->mask_w);
    for (int i = 0; i < N; ++i) {
        const nnd_stereo_eval_output& o = d->outputs[i];
        NND_REQUIRE(o.data, "stereo_eval: output %d: null pointer", i);
        NND_REQUIRE(o.C > 0 && o.h > 0 && o.w > 0, "stereo_eval: output %d: bad shape (%d,%d,%d,%d)", i, d->B, o.C, o.h, o.w);
        NND_REQUIRE(d->Cg == o.C || d->Cg == 1, "stereo_eval: output %d has %d channels, the ground truth %d (equal, or 1 to broadcast)", i,
                    o.C, d->Cg);
        NND_REQUIRE(o.stride_b >= 0 && o.stride_c >= 0 && o.stride_row >= 0, "stereo_eval: output %d: negative stride", i);
        NND_REQUIRE((int64_t)d->B * o.C * o.h * o.w < ((int64_t)1 << 31),
                    "stereo_eval: output %d: bad shape (%d,%d,%d,%d): B*C*h*w must be below 2^31", i, d->B, o.C, o.h, o.w);
        NND_REQUIRE((int64_t)d->B * o.h * cdiv(o.w, 4) < ((int64_t)1 << 31) - 2 * SE_U * SE_GMAX * SE_T,  // the quad index never wraps
                    "stereo_eval: output %d: bad shape (%d,%d,%d,%d): too many rows", i, d->B, o.C, o.h, o.w);
        int s, Hp, Wp;
        if ((o.h != d->H || o.w != d->W) && !se_pool_geometry("stereo_eval", d->H, d->W, o.h, o.w, &s, &Hp, &Wp)) return NND_ERR_INVALID;
        NND_REQUIRE(!d->mask || (o.h == d->mask_h && o.w == d->mask_w),
                    "stereo_eval: valid_mask is %dx%d but output %d is %dx%d: a mask needs every output of the call at its size", d->mask_h,
                    d->mask_w, i, o.h, o.w);
    }

    SeFinal f;
    f.N = N, f.n_above = d->n_above, f.n_below = d->n_below, f.K = 3 + d->n_above + d->n_below;
    hipStream_t st = (hipStream_t)stream;
    bool done[SE_MAXO] = {};
    for (int i0 = 0; i0 < N; ++i0) {
        if (done[i0]) continue;
        const nnd_stereo_eval_output& o0 = d->outputs[i0];
        SeGroup g;
        g.gt = d->gt, g.mask = d->mask;
        g.Cg = d->Cg, g.H = d->H, g.W = d->W;
        g.Cp = o0.C, g.h = o0.h, g.w = o0.w;
        const bool same = o0.h == d->H && o0.w == d->W;
        g.s = 1, g.Hp = d->H, g.Wp = d->W;
        if (!same) se_pool_geometry("stereo_eval", d->H, d->W, o0.h, o0.w, &g.s, &g.Hp, &g.Wp);
        g.fs = (float)g.s, g.ry = (float)g.Hp / (float)g.h, g.rx = (float)g.Wp / (float)g.w;
        g.Wq = cdiv(g.w, 4);
        g.nquads = d->B * g.h * g.Wq;
        g.G = (int)(cdiv64(g.nquads, SE_T) < SE_GMAX ? cdiv64(g.nquads, SE_T) : SE_GMAX);
        g.max_flow = d->max_flow;
        for (int k = 0; k < SE_NTHR; ++k) {
            g.above[k] = k < d->n_above ? d->above[k] : INFINITY;
            g.below[k] = k < d->n_below ? d->below[k] : -INFINITY;
        }
        const bool group_vec = g.w % 4 == 0 && (!same || ((uintptr_t)d->gt & 15) == 0) && (!d->mask || ((uintptr_t)d->mask & 3) == 0);
        int n = 0;
        for (int i = i0; i < N; ++i) {
            const nnd_stereo_eval_output& o = d->outputs[i];
            if (done[i] || o.C != o0.C || o.h != o0.h || o.w != o0.w) continue;
            done[i] = true;
            g.slot[n] = (unsigned char)i;
            g.outs[n].p = o.data, g.outs[n].sb = (long)o.stride_b, g.outs[n].sc = (long)o.stride_c, g.outs[n].sr = (long)o.stride_row;
            g.vec[n] = group_vec && ((uintptr_t)o.data & 15) == 0 && o.stride_b % 4 == 0 && o.stride_c % 4 == 0 && o.stride_row % 4 == 0;
            f.G[i] = g.G;
            f.elems[i] = (double)d->B * o.C * o.h * o.w;
            ++n;
        }
        for (int k = n; k < SE_MAXO; ++k) g.slot[k] = 0, g.vec[k] = 0, g.outs[k] = g.outs[0];
        se_launch_partial(same, g, n, (double*)workspace, st);
        NND_LAUNCH_CHECK();
    }
    for (int i = 0; i < SE_MAXO; ++i) {
        f.wgt[i] = i < N ? std::pow((double)d->gamma, (double)(N - 1 - i)) : 0.0;
        if (i >= N) f.G[i] = 0, f.elems[i] = 1.0;
    }
    hipLaunchKernelGGL(se_final_kernel, dim3(1), dim3(SE_FINAL_T), 0, st, f, (const double*)workspace, out);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_stereo_eval_accumulate(const double* metrics, int n, double* sums, void* stream) {
    NND_REQUIRE(metrics && sums, "stereo_eval_accumulate: null pointer");
    NND_REQUIRE(n > 0 && n <= SE_MAXO * (3 + 2 * SE_NTHR) + 1, "stereo_eval_accumulate: bad length %d (1 .. %d)", n,
                SE_MAXO * (3 + 2 * SE_NTHR) + 1);
    hipLaunchKernelGGL(se_accumulate_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, metrics, n, sums);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_min_pool_nearest(const float* gt, float* dst, int B, int C, int H, int W, int h, int w, void* stream) {
    NND_REQUIRE(gt && dst, "min_pool_nearest: null pointer");
    NND_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && h > 0 && w > 0 && (int64_t)B * C <= 65535, "min_pool_nearest: bad shape (%d,%d,%d,%d) -> %dx%d",
                B, C, H, W, h, w);
    NND_REQUIRE((int64_t)B * C * H * W < ((int64_t)1 << 31) && (int64_t)B * C * h * w < ((int64_t)1 << 31),
                "min_pool_nearest: bad shape (%d,%d,%d,%d) -> %dx%d: the maps must have fewer than 2^31 elements", B, C, H, W, h, w);
    int s, Hp, Wp;
    if (!se_pool_geometry("min_pool_nearest", H, W, h, w, &s, &Hp, &Wp)) return NND_ERR_INVALID;
    hipLaunchKernelGGL(min_pool_nearest_kernel, dim3((unsigned)cdiv64((int64_t)h * w, 256), B * C), dim3(256), 0, (hipStream_t)stream, gt, dst,
                       H, W, h, w, s, (float)s, Hp, Wp, (float)Hp / (float)h, (float)Wp / (float)w);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

}  // extern "C"
