// Encoder side of IGEVStereoMBNet in ONE C-ABI call (nnd_mbv3_forward): the MobileNetV3-Large backbone of timm's
// tf_mobilenetv3_large_100(features_only=True) as MobilenetV3LargeEncoder runs it (nndepth/encoders/mobilenetv3_encoder.py), then
// fnet_proj / cnet_proj and the guide split of IGEVStereoMBNet.forward_fnet (nndepth/models/igev_stereo/model.py:163-203).  Exact
// fp32 throughout: no split arithmetic, no calibration.
//
// Every BatchNorm is folded into its conv on the host (ops.MobileNetV3Engine, float64, cast once to fp32), so the device runs:
//   conv_stem + bn1 + hard-swish   3x3 dense (3 -> 16), stride 2, TF "same" padding     mbv3_stem_kernel (VALU, float64 taps)
//   DepthwiseSeparable (stage 0)   depthwise 3x3 + ReLU                                   mbv3_dw_kernel<3>
//                                  1x1 (16 -> 16), x + (.)                               conv_mfma, EPI_AFFINE + residual
//   InvertedResidual               1x1 expand + act                                       conv_mfma, EPI_RELU / EPI_HSWISH
//                                  depthwise k x k (3, 5), stride 1 / 2, same padding,    mbv3_dw_kernel<k> (+ per-workgroup sums of
//                                  act                                                    the SE mean where the block has SE)
//                                  [SE: mean -> reduce + ReLU -> expand -> hard-sigmoid]  mbv3_se_kernel (one workgroup per sample)
//                                  [x * gate, in place]                                   mbv3_gate_kernel
//                                  1x1 project, [x + (.)]                                 conv_mfma, EPI_AFFINE [+ residual]
//   fnet_proj / cnet_proj          3x3 (24 -> 2 hidden / 2 context), padding 1, ReLU     mbv3_proj_kernel (VALU: fp32 9-tap chains
//                                                                                         summed in float64)
// Only the right frames' stage-1 map is needed (fmap2): stages 0-1 run on both frames, stages 2-5 on the left frames only, and
// stage 6 (whose output the reference discards) never runs.  Eval BatchNorm is per sample, so this changes no output.
// Every conv_mfma launch fixes its split-K factor per layer (enc_plan.h: enc_run_mfma), so a pair's maps do not depend on the batch it
// runs in.  The SE mean is reduced in a fixed order (workgroup tree, then the workgroups in order): no
// float atomics, bit-reproducible.  Activations are NCHW in the caller's workspace.
// The layer plan, the packer and the conv_mfma launcher are enc_plan.h's, shared with repvit.hip and midas.hip; the backbone walk
// (mb_walk, declared in mbv3.h) also serves midas.hip; the depthwise tap loop and the stem's patch gather are enc_valu.h's.
#include "mbv3.h"
#include "enc_valu.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace nnd {

// torch's hardswish / hardsigmoid: x * min(max(x + 3, 0), 6) / 6, min(max(x + 3, 0), 6) / 6
__device__ __forceinline__ double mb_act(double v, int act) {
    if (act == MB_RELU) return v > 0.0 ? v : 0.0;
    if (act == MB_HSWISH) return v * fmin(fmax(v + 3.0, 0.0), 6.0) / 6.0;
    return v;
}


// ------------------------------------------------------------------------------------------ depthwise k x k
// One thread per output pixel of one (sample, channel) plane; taps in (dy, dx) order, float64 accumulation rounded once after
// bias and activation.  partial != nullptr (SE blocks): each workgroup also writes the sum of its outputs (as stored, fp32 values
// summed in float64 in a fixed tree order) to partial[(n * C + c) * gridDim.x + blockIdx.x].  grid (ceil(Ho*Wo / 256), C, N)
constexpr int MB_DW_T = 256;
template <int K>
__global__ void __launch_bounds__(MB_DW_T) mbv3_dw_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ w,
                                                          const float* __restrict__ bias, double* __restrict__ partial, int C, int Hin,
                                                          int Win, int Ho, int Wo, int stride, int pt, int pl, int act) {
    __shared__ double red[MB_DW_T];
    const int idx = blockIdx.x * MB_DW_T + threadIdx.x;
    const int c = blockIdx.y, n = blockIdx.z;
    const bool ok = idx < Ho * Wo;
    float out = 0.f;
    if (ok) {
        const int oy = idx / Wo, ox = idx - oy * Wo;
        const float* xp = x + ((long)n * C + c) * Hin * Win;
        const float* wp = w + (long)c * K * K;
        const int iy0 = oy * stride - pt, ix0 = ox * stride - pl;
        const double acc = dw_taps<K>(xp, wp, iy0, ix0, Hin, Win);
        out = (float)mb_act(acc + (double)bias[c], act);
        y[((long)n * C + c) * Ho * Wo + idx] = out;
    }
    if (partial == nullptr) return;  // uniform over the workgroup
    red[threadIdx.x] = (double)out;
    __syncthreads();
    for (int s = MB_DW_T / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[((long)n * C + c) * gridDim.x + blockIdx.x] = red[0];
}

// ------------------------------------------------------------------------------------------ squeeze-excite gate
// One workgroup per sample: mean[c] = (sum of the nblk partials of (n, c), in order) / P; h = relu(Wr mean + br);
// gate[n, c] = hardsigmoid(We h + be).  float64 throughout, rounded once.  C <= MB_SE_MAXC, rd <= MB_SE_MAXR.
constexpr int MB_SE_MAXC = 1024, MB_SE_MAXR = 256;
__global__ void __launch_bounds__(256) mbv3_se_kernel(const double* __restrict__ partial, int nblk, int P, const float* __restrict__ wr,
                                                      const float* __restrict__ br, const float* __restrict__ we,
                                                      const float* __restrict__ be, float* __restrict__ gate, int C, int rd) {
    __shared__ double mean[MB_SE_MAXC];
    __shared__ double hid[MB_SE_MAXR];
    const int n = blockIdx.x, t = threadIdx.x;
    for (int c = t; c < C; c += 256) {
        const double* p = partial + ((long)n * C + c) * nblk;
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s += p[b];
        mean[c] = s / (double)P;
    }
    __syncthreads();
    for (int r = t; r < rd; r += 256) {
        const float* wp = wr + (long)r * C;
        double acc = 0.0;
        for (int c = 0; c < C; ++c) acc = fma((double)wp[c], mean[c], acc);
        acc += (double)br[r];
        hid[r] = acc > 0.0 ? acc : 0.0;
    }
    __syncthreads();
    for (int c = t; c < C; c += 256) {
        const float* wp = we + (long)c * rd;
        double acc = 0.0;
        for (int r = 0; r < rd; ++r) acc = fma((double)wp[r], hid[r], acc);
        acc += (double)be[c];
        gate[(long)n * C + c] = (float)(fmin(fmax(acc + 3.0, 0.0), 6.0) / 6.0);
    }
}

// y[n, c, :] *= gate[n, c] in place.  grid (ceil(P / 256), C, N)
__global__ void __launch_bounds__(256) mbv3_gate_kernel(float* __restrict__ y, const float* __restrict__ gate, int C, int P) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= P) return;
    const int c = blockIdx.y, n = blockIdx.z;
    y[((long)n * C + c) * P + idx] *= gate[(long)n * C + c];
}

// ------------------------------------------------------------------------------------------ conv_stem: 3x3 dense, 3 -> 16, stride 2
// Samples n < nsplit read `x`, the others `x1` (the two frame tensors where they lie).  One thread per output pixel, all 16
// output channels; float64 taps, bias and hard-swish, rounded once; the 27 x 16 weights sit in LDS.
__global__ void __launch_bounds__(256) mbv3_stem_kernel(const float* __restrict__ x, const float* __restrict__ x1, int nsplit,
                                                        float* __restrict__ y, const float* __restrict__ w, const float* __restrict__ bias,
                                                        int Hin, int Win, int Ho, int Wo, int pt, int pl) {
    __shared__ float ws[MB_STEM_C * 28];
    for (int i = threadIdx.x; i < MB_STEM_C * 28; i += 256) ws[i] = i < MB_STEM_C * 27 ? w[i] : bias[i - MB_STEM_C * 27];
    __syncthreads();
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= Ho * Wo) return;
    const int n = blockIdx.z;
    const int oy = idx / Wo, ox = idx - oy * Wo;
    const float* xp = n < nsplit ? x + (long)n * 3 * Hin * Win : x1 + (long)(n - nsplit) * 3 * Hin * Win;
    float in[27];
    stem_gather(xp, oy, ox, 2, pt, pl, Hin, Win, in);
    float* yp = y + (long)n * MB_STEM_C * Ho * Wo + idx;
#pragma unroll 4
    for (int co = 0; co < MB_STEM_C; ++co) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 27; ++k) acc = fma((double)ws[co * 27 + k], (double)in[k], acc);
        yp[(long)co * Ho * Wo] = (float)mb_act(acc + (double)ws[MB_STEM_C * 27 + co], MB_HSWISH);
    }
}

// ------------------------------------------------------------------------------------------ fnet_proj / cnet_proj: 3x3, padding 1
// y = relu(conv3x3(x) + bias), Cin <= MB_PJ_MAXCI.  One thread per output pixel and MB_PJ_CO output channels (grid.y); per input
// channel the 9 taps are one fp32 chain, the Cin chain results are summed in float64 with the bias and rounded once.  On conv_mfma
// (K = 216 in 16-channel chunks) this layer's error was up to 2.1x PyTorch's own fp32 error at 544x960; here it is ~1 ulp.
// grid (ceil(H*W / 256), ceil(Cout / MB_PJ_CO), N); the layer's weights for the block sit in LDS.
constexpr int MB_PJ_CO = 16, MB_PJ_MAXCI = 64;
__global__ void __launch_bounds__(256) mbv3_proj_kernel(const float* __restrict__ x, int64_t xbs, float* __restrict__ y,
                                                        const float* __restrict__ w, const float* __restrict__ bias, int Cin, int Cout,
                                                        int H, int W) {
    __shared__ float ws[MB_PJ_CO * MB_PJ_MAXCI * 9];
    const int co0 = blockIdx.y * MB_PJ_CO;
    const int nco = min(MB_PJ_CO, Cout - co0);
    for (int i = threadIdx.x; i < MB_PJ_CO * Cin * 9; i += 256) ws[i] = i < nco * Cin * 9 ? w[(long)co0 * Cin * 9 + i] : 0.f;
    __syncthreads();
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= H * W) return;
    const int n = blockIdx.z;
    const int oy = idx / W, ox = idx - oy * W;
    const float* xp = x + (long)n * xbs;
    double acc[MB_PJ_CO];
#pragma unroll
    for (int j = 0; j < MB_PJ_CO; ++j) acc[j] = 0.0;
    for (int ci = 0; ci < Cin; ++ci) {
        float in[9];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int iy = oy - 1 + dy, ix = ox - 1 + dx;
                in[dy * 3 + dx] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? xp[((long)ci * H + iy) * W + ix] : 0.f;
            }
#pragma unroll
        for (int j = 0; j < MB_PJ_CO; ++j) {
            const float* wp = ws + (j * Cin + ci) * 9;
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < 9; ++t) s = fmaf(wp[t], in[t], s);
            acc[j] += (double)s;
        }
    }
    float* yp = y + ((long)n * Cout + co0) * H * W + idx;
#pragma unroll
    for (int j = 0; j < MB_PJ_CO; ++j)
        if (j < nco) {
            const double v = acc[j] + (double)bias[co0 + j];
            yp[(long)j * H * W] = (float)(v > 0.0 ? v : 0.0);
        }
}

// ------------------------------------------------------------------------------------------ plan
// The backbone is fixed (tf_mobilenetv3_large_100, stages 0..5 as decoded by timm; nndepth_amd/mobilenetv3.py:block_table)
const MbBlock MB_BLOCKS[] = {
    {0, 16, 16, 16, 3, 1, 0, MB_RELU, 1, 0},
    {1, 16, 64, 24, 3, 2, 0, MB_RELU, 0, 1},      {1, 24, 72, 24, 3, 1, 0, MB_RELU, 1, 1},
    {1, 24, 72, 40, 5, 2, 24, MB_RELU, 0, 2},     {1, 40, 120, 40, 5, 1, 32, MB_RELU, 1, 2},   {1, 40, 120, 40, 5, 1, 32, MB_RELU, 1, 2},
    {1, 40, 240, 80, 3, 2, 0, MB_HSWISH, 0, 3},   {1, 80, 200, 80, 3, 1, 0, MB_HSWISH, 1, 3},  {1, 80, 184, 80, 3, 1, 0, MB_HSWISH, 1, 3},
    {1, 80, 184, 80, 3, 1, 0, MB_HSWISH, 1, 3},
    {1, 80, 480, 112, 3, 1, 120, MB_HSWISH, 0, 4}, {1, 112, 672, 112, 3, 1, 168, MB_HSWISH, 1, 4},
    {1, 112, 672, 160, 5, 2, 168, MB_HSWISH, 0, 5}, {1, 160, 960, 160, 5, 1, 240, MB_HSWISH, 1, 5}, {1, 160, 960, 160, 5, 1, 240, MB_HSWISH, 1, 5},
};
const int MB_NBLOCKS = (int)(sizeof(MB_BLOCKS) / sizeof(MB_BLOCKS[0]));
constexpr int MB_S1_C = 24;  // stage 1's width: fnet_proj / cnet_proj input

static int mb_check(const nnd_mbv3_desc* d) {
    if (int rc = check_desc(d, 0, "mbv3")) return rc;
    NND_REQUIRE(d->fnet_dim >= 1 && d->fnet_dim <= 4096, "mbv3: fnet_dim %d (fnet_proj output channels, 1..4096)", d->fnet_dim);
    NND_REQUIRE(d->cnet_dim >= 1 && d->cnet_dim <= 4096, "mbv3: cnet_dim %d (cnet_proj output channels, 1..4096)", d->cnet_dim);
    return NND_OK;
}

static void mb_add_dense(EncPlan& p, int kind, int cin, int cout, int k, int stride, int act) {  // stem / projection: (cout, cin, k, k) + bias
    enc_add_raw(p, kind, cin, cout, k, stride, act, (int64_t)cout * cin * k * k + cout);
}

void mb_plan_backbone(EncPlan& p) {
    mb_add_dense(p, ENC_STEM, 3, MB_STEM_C, 3, 2, MB_HSWISH);
    for (int i = 0; i < MB_NBLOCKS; ++i) {
        const MbBlock& b = MB_BLOCKS[i];
        if (b.ir) enc_add_mfma(p, b.cin, b.mid, 1, 1, b.act);
        enc_add_raw(p, ENC_DW, b.mid, b.mid, b.k, b.stride, b.act, (int64_t)b.mid * b.k * b.k + b.mid);
        if (b.rd) {  // SE reduce (rd, C) / expand (C, rd) 1x1 with bias
            enc_add_raw(p, MB_SE_R, b.mid, b.rd, 1, 1, MB_RELU, (int64_t)b.rd * b.mid + b.rd);
            enc_add_raw(p, MB_SE_E, b.rd, b.mid, 1, 1, MB_NONE, (int64_t)b.mid * b.rd + b.mid);
        }
        enc_add_mfma(p, b.mid, b.cout, 1, 1, MB_NONE);
    }
}

// layer order (= the tensor order of nnd_mbv3_pack): the backbone (mb_plan_backbone) | fnet_proj 3x3 | cnet_proj 3x3
static int mb_plan(const nnd_mbv3_desc* d, EncPlan* p) {
    if (int rc = mb_check(d)) return rc;
    mb_plan_backbone(*p);
    mb_add_dense(*p, MB_PROJ, MB_S1_C, d->fnet_dim, 3, 1, MB_RELU);
    mb_add_dense(*p, MB_PROJ, MB_S1_C, d->cnet_dim, 3, 1, MB_RELU);
    return NND_OK;
}

// ------------------------------------------------------------------------------------------ launchers
static int run_dw(const float* x, const float* w, const float* bias, float* y, double* partial, int N, int C, int Hin, int Win, int k,
                  int stride, int act, hipStream_t st) {
    const int Ho = same_out(Hin, stride), Wo = same_out(Win, stride);
    const int pt = stride == 1 ? k / 2 : same_pad_before(Hin, k, 2), pl = stride == 1 ? k / 2 : same_pad_before(Win, k, 2);
    dim3 grid((unsigned)cdiv(Ho * Wo, MB_DW_T), (unsigned)C, (unsigned)N);
    if (k == 3)
        hipLaunchKernelGGL(mbv3_dw_kernel<3>, grid, dim3(MB_DW_T), 0, st, x, y, w, bias, partial, C, Hin, Win, Ho, Wo, stride, pt, pl, act);
    else
        hipLaunchKernelGGL(mbv3_dw_kernel<5>, grid, dim3(MB_DW_T), 0, st, x, y, w, bias, partial, C, Hin, Win, Ho, Wo, stride, pt, pl, act);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

static int run_se(float* y, const double* partial, const float* wr, const float* br, const float* we, const float* be, float* gate, int N,
                  int C, int rd, int H, int W, hipStream_t st) {
    const int P = H * W;
    hipLaunchKernelGGL(mbv3_se_kernel, dim3((unsigned)N), dim3(256), 0, st, partial, cdiv(P, MB_DW_T), P, wr, br, we, be, gate, C, rd);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(mbv3_gate_kernel, dim3((unsigned)cdiv(P, 256), (unsigned)C, (unsigned)N), dim3(256), 0, st, y, gate, C, P);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

static int run_stem(const float* x, const float* x1, int nsplit, const float* w, const float* bias, float* y, int N, int H, int W,
                    hipStream_t st) {
    const int Ho = same_out(H, 2), Wo = same_out(W, 2);
    hipLaunchKernelGGL(mbv3_stem_kernel, dim3((unsigned)cdiv(Ho * Wo, 256), 1, (unsigned)N), dim3(256), 0, st, x, x1, nsplit, y, w, bias, H,
                       W, Ho, Wo, same_pad_before(H, 3, 2), same_pad_before(W, 3, 2));
    NND_LAUNCH_CHECK();
    return NND_OK;
}

static int run_proj(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Cout, int H, int W, hipStream_t st) {
    dim3 grid((unsigned)cdiv(H * W, 256), (unsigned)cdiv(Cout, MB_PJ_CO), (unsigned)N);
    hipLaunchKernelGGL(mbv3_proj_kernel, grid, dim3(256), 0, st, x, (int64_t)Cin * H * W, y, w, bias, Cin, Cout, H, W);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int mb_run_pw(const EncLayer& l, const float* blob, const float* x, float* y, const float* res, int N, int H, int W, hipStream_t st) {
    const int epi = l.act == MB_RELU ? EPI_RELU : l.act == MB_HSWISH ? EPI_HSWISH : EPI_AFFINE;
    return enc_run_mfma(l, blob, x, (int64_t)l.cin * H * W, y, (int64_t)l.cout * H * W, res, epi, 0, N, H, W, H, W, st);
}

// ------------------------------------------------------------------------------------------ the backbone walk
// workspace: running activations A, B (ping-pong), expanded E, depthwise D, SE gate, SE partials (doubles); s1: stage 1's map of
// the n01 samples (the caller's own region where it keeps it: nnd_mbv3_forward)
struct MbWs {
    int64_t act, e, d, gate, part, s1;  // floats (part: doubles)
    int64_t walk() const { return 2 * enc_align(act) + enc_align(e) + enc_align(d) + enc_align(gate) + 2 * enc_align(part); }
};

static MbWs mb_ws(int n01, int n25, int H, int W) {
    MbWs r{};
    int h = same_out(H, 2), w = same_out(W, 2);
    r.act = (int64_t)n01 * MB_STEM_C * h * w;
    for (int i = 0; i < MB_NBLOCKS; ++i) {
        const MbBlock& b = MB_BLOCKS[i];
        const int64_t nb = b.stage <= 1 ? n01 : n25;
        const int ho = same_out(h, b.stride), wo = same_out(w, b.stride);
        r.act = std::max(r.act, nb * b.cout * ho * wo);
        r.e = std::max(r.e, nb * b.mid * h * w);
        r.d = std::max(r.d, nb * b.mid * ho * wo);
        if (b.rd) {
            r.gate = std::max(r.gate, nb * b.mid);
            r.part = std::max(r.part, nb * b.mid * cdiv(ho * wo, MB_DW_T));
        }
        if (b.stage == 1) r.s1 = nb * MB_S1_C * ho * wo;
        h = ho; w = wo;
    }
    return r;
}

int64_t mb_walk_ws(int n01, int n25, int H, int W) { return mb_ws(n01, n25, H, W).walk(); }

int mb_walk(const EncPlan& p, const float* packed, const float* frame1, const float* frame2, int nsplit, int n01, int n25,
            float* const* keep, float* workspace, int H, int W, hipStream_t st) {
    const MbWs r = mb_ws(n01, n25, H, W);
    float* q = workspace;
    float* bufA = q; q += enc_align(r.act);
    float* bufB = q; q += enc_align(r.act);
    float* E = q; q += enc_align(r.e);
    float* D = q; q += enc_align(r.d);
    float* gate = q; q += enc_align(r.gate);
    double* part = reinterpret_cast<double*>(q);  // 64-float aligned
    size_t li = 0;
    auto L = [&]() -> const EncLayer& { return p.layers[li++]; };
    auto P = [&](const EncLayer& l) { return packed + l.off; };                  // a raw layer's weights
    auto Pb = [&](const EncLayer& l) { return packed + l.off + l.floats - l.cout; };  // ... its bias
    int rc;
    int h = same_out(H, 2), w = same_out(W, 2);
    const EncLayer& l0 = L();
    if ((rc = run_stem(frame1, frame2, nsplit, P(l0), Pb(l0), bufA, n01, H, W, st))) return rc;
    const float* x = bufA;
    for (int i = 0; i < MB_NBLOCKS; ++i) {
        const MbBlock& b = MB_BLOCKS[i];
        const int nb = b.stage <= 1 ? n01 : n25;  // nnd_mbv3_forward: stages 2..5 on the left frames (the first B samples) only
        const int ho = same_out(h, b.stride), wo = same_out(w, b.stride);
        const bool last = i + 1 == MB_NBLOCKS || MB_BLOCKS[i + 1].stage != b.stage;
        float* out = last && keep[b.stage] ? keep[b.stage] : (x == bufA ? bufB : bufA);
        const float* dwin = x;
        if (b.ir) {
            if ((rc = mb_run_pw(L(), packed, x, E, nullptr, nb, h, w, st))) return rc;
            dwin = E;
        }
        const EncLayer& dw = L();
        if ((rc = run_dw(dwin, P(dw), Pb(dw), D, b.rd ? part : nullptr, nb, dw.cout, h, w, dw.k, dw.stride, dw.act, st))) return rc;
        if (b.rd) {
            const EncLayer& lr = L();
            const EncLayer& le = L();
            if ((rc = run_se(D, part, P(lr), Pb(lr), P(le), Pb(le), gate, nb, b.mid, b.rd, ho, wo, st))) return rc;
        }
        if ((rc = mb_run_pw(L(), packed, D, out, b.skip ? x : nullptr, nb, ho, wo, st))) return rc;
        x = out;
        h = ho; w = wo;
    }
    return NND_OK;
}

}  // namespace nnd

using namespace nnd;

extern "C" {

// ---- the encoder side's kernels one at a time (the launchers nnd_mbv3_forward uses; per-kernel tests and profiles)
int nnd_mbv3_depthwise(const float* x, const float* w, const float* bias, float* y, double* partial, int N, int C, int H, int W, int k,
                       int stride, int act, void* stream) {
    NND_REQUIRE(x && w && bias && y, "mbv3_depthwise: null pointer");
    NND_REQUIRE(k == 3 || k == 5, "mbv3_depthwise: kernel %d not built (3, 5)", k);
    NND_REQUIRE(stride == 1 || stride == 2, "mbv3_depthwise: stride %d not built (1, 2)", stride);
    NND_REQUIRE(act >= MB_NONE && act <= MB_HSWISH, "mbv3_depthwise: activation %d (0 none, 1 ReLU, 2 hard-swish)", act);
    NND_REQUIRE(N >= 1 && C >= 1 && H >= 1 && W >= 1 && C <= 65535 && N <= 65535, "mbv3_depthwise: bad size %dx%dx%dx%d", N, C, H, W);
    return run_dw(x, w, bias, y, partial, N, C, H, W, k, stride, act, (hipStream_t)stream);
}

int64_t nnd_mbv3_se_partials(int N, int C, int H, int W) {
    NND_REQUIRE(N >= 1 && C >= 1 && H >= 1 && W >= 1, "mbv3_se_partials: bad size %dx%dx%dx%d", N, C, H, W);
    return (int64_t)N * C * cdiv(H * W, MB_DW_T);
}

int nnd_mbv3_se(float* y, const double* partial, const float* wr, const float* br, const float* we, const float* be, float* gate, int N,
                int C, int rd, int H, int W, void* stream) {
    NND_REQUIRE(y && partial && wr && br && we && be && gate, "mbv3_se: null pointer");
    NND_REQUIRE(N >= 1 && N <= 65535 && C >= 1 && C <= MB_SE_MAXC && rd >= 1 && rd <= MB_SE_MAXR && H >= 1 && W >= 1,
                "mbv3_se: bad size N %d C %d rd %d %dx%d (C <= %d, rd <= %d)", N, C, rd, H, W, MB_SE_MAXC, MB_SE_MAXR);
    return run_se(y, partial, wr, br, we, be, gate, N, C, rd, H, W, (hipStream_t)stream);
}

int nnd_mbv3_stem(const float* x, const float* x1, int nsplit, const float* w, const float* bias, float* y, int N, int H, int W,
                  void* stream) {
    NND_REQUIRE(x && w && bias && y, "mbv3_stem: null pointer");
    NND_REQUIRE(N >= 1 && H >= 1 && W >= 1 && N <= 65535, "mbv3_stem: bad size %dx%dx%d", N, H, W);
    if (!x1) nsplit = N;
    NND_REQUIRE(nsplit >= 1 && nsplit <= N, "mbv3_stem: nsplit %d of %d", nsplit, N);
    return run_stem(x, x1 ? x1 : x, nsplit, w, bias, y, N, H, W, (hipStream_t)stream);
}

int nnd_mbv3_proj(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Cout, int H, int W, void* stream) {
    NND_REQUIRE(x && w && bias && y, "mbv3_proj: null pointer");
    NND_REQUIRE(N >= 1 && N <= 65535 && Cin >= 1 && Cin <= MB_PJ_MAXCI && Cout >= 1 && H >= 1 && W >= 1,
                "mbv3_proj: bad size N %d Cin %d Cout %d %dx%d (Cin <= %d)", N, Cin, Cout, H, W, MB_PJ_MAXCI);
    return run_proj(x, w, bias, y, N, Cin, Cout, H, W, (hipStream_t)stream);
}

int64_t nnd_mbv3_pointwise_packed_floats(int Cout, int Cin, int k) {
    NND_REQUIRE(Cout >= 1 && Cin >= 1, "mbv3_pointwise: channels %d -> %d", Cin, Cout);
    NND_REQUIRE(k == 1 || k == 3, "mbv3_pointwise: kernel %d not built (1, 3)", k);
    return enc_align(enc_mfma_layer(Cin, Cout, k, 1, MB_NONE).floats);
}

int nnd_mbv3_pointwise_pack(int Cout, int Cin, int k, const float* w, const float* bias, float* packed_host) {
    NND_REQUIRE(Cout >= 1 && Cin >= 1 && w && bias && packed_host, "mbv3_pointwise_pack: bad argument");
    NND_REQUIRE(k == 1 || k == 3, "mbv3_pointwise_pack: kernel %d not built (1, 3)", k);
    const EncLayer l = enc_mfma_layer(Cin, Cout, k, 1, MB_NONE);
    memset(packed_host, 0, sizeof(float) * enc_align(l.floats));
    enc_pack_mfma(l, w, bias, nullptr, packed_host);
    return NND_OK;
}

int nnd_mbv3_pointwise(int Cout, int Cin, int k, const float* packed_dev, const float* x, const float* residual, float* y, int N, int H,
                       int W, int act, void* stream) {
    NND_REQUIRE(packed_dev && x && y && N >= 1 && H >= 1 && W >= 1, "mbv3_pointwise: bad argument");
    NND_REQUIRE(Cout >= 1 && Cin >= 1 && (k == 1 || k == 3), "mbv3_pointwise: %dx%d %d -> %d not built", k, k, Cin, Cout);
    NND_REQUIRE(act >= MB_NONE && act <= MB_HSWISH, "mbv3_pointwise: activation %d (0 none, 1 ReLU, 2 hard-swish)", act);
    NND_REQUIRE(!(act && residual), "mbv3_pointwise: an activation and a residual are not built together");
    return mb_run_pw(enc_mfma_layer(Cin, Cout, k, 1, act), packed_dev, x, y, residual, N, H, W, (hipStream_t)stream);
}

int nnd_mbv3_num_tensors(const nnd_mbv3_desc* desc) {
    EncPlan p;
    if (int rc = mb_plan(desc, &p)) return rc;
    return 2 * (int)p.layers.size();
}

int64_t nnd_mbv3_packed_floats(const nnd_mbv3_desc* desc) {
    EncPlan p;
    if (int rc = mb_plan(desc, &p)) return rc;
    return p.total;
}

int64_t nnd_mbv3_workspace_floats(const nnd_mbv3_desc* desc, int B, int H, int W) {
    if (int rc = mb_check(desc)) return rc;
    NND_REQUIRE(B >= 1 && H >= 1 && W >= 1 && B <= 32767, "mbv3: bad size %dx%dx%d", B, H, W);
    const MbWs r = mb_ws(2 * B, B, H, W);
    return r.walk() + enc_align(r.s1);
}

int nnd_mbv3_pack(const nnd_mbv3_desc* desc, const float* const* t, float* packed_host) {
    EncPlan p;
    if (int rc = mb_plan(desc, &p)) return rc;
    return enc_pack(p, 2, t, packed_host, "mbv3_pack");
}

int nnd_mbv3_forward(const nnd_mbv3_desc* desc, const float* packed, const float* frame1, const float* frame2, float* fmap1, float* fmap2,
                     float* cnet1, float* guide0, float* guide1, float* guide2, float* workspace, int B, int H, int W, void* stream) {
    EncPlan p;
    if (int rc = mb_plan(desc, &p)) return rc;
    NND_REQUIRE(packed && frame1 && frame2 && fmap1 && fmap2 && cnet1 && guide0 && guide1 && guide2 && workspace,
                "mbv3_forward: null pointer");
    NND_REQUIRE(B >= 1 && H >= 1 && W >= 1 && B <= 32767, "mbv3_forward: bad size %dx%dx%d", B, H, W);
    hipStream_t st = (hipStream_t)stream;
    // stages 0..1 on both frames (2B samples), 2..5 on the left frames; stage 1's map of both frames lies behind the walk's workspace
    float* s1 = workspace + mb_walk_ws(2 * B, B, H, W);
    float* const keep[MB_NSTAGES] = {nullptr, s1, guide0, guide1, nullptr, guide2};
    int rc;
    if ((rc = mb_walk(p, packed, frame1, frame2, B, 2 * B, B, keep, workspace, H, W, st))) return rc;
    // fnet_proj on both frames' stage-1 map, cnet_proj on the left frames'
    const int h1 = same_out(same_out(H, 2), 2), w1 = same_out(same_out(W, 2), 2);
    const EncLayer& fp = p.layers[p.layers.size() - 2];
    const EncLayer& cp = p.layers[p.layers.size() - 1];
    const int64_t sbs = (int64_t)MB_S1_C * h1 * w1;
    const float *fw = packed + fp.off, *fb = fw + fp.floats - fp.cout, *cw = packed + cp.off, *cb = cw + cp.floats - cp.cout;
    if ((rc = run_proj(s1, fw, fb, fmap1, B, MB_S1_C, fp.cout, h1, w1, st))) return rc;
    if ((rc = run_proj(s1 + B * sbs, fw, fb, fmap2, B, MB_S1_C, fp.cout, h1, w1, st))) return rc;
    return run_proj(s1, cw, cb, cnet1, B, MB_S1_C, cp.cout, h1, w1, st);
}

}  // extern "C"
