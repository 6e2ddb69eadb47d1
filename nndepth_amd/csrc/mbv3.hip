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
// Every conv_mfma launch fixes its split-K factor per layer (2 from two K chunks on, else 1; as repvit.hip), so a pair's maps do not
// depend on the batch it runs in.  The SE mean is reduced in a fixed order (workgroup tree, then the workgroups in order): no
// float atomics, bit-reproducible.  Activations are NCHW in the caller's workspace.
#include "mbv3.h"

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
#pragma unroll
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int iy = oy * 2 - pt + dy, ix = ox * 2 - pl + dx;
                const bool ok = iy >= 0 && iy < Hin && ix >= 0 && ix < Win;
                in[(ci * 3 + dy) * 3 + dx] = ok ? xp[((long)ci * Hin + iy) * Win + ix] : 0.f;
            }
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




void mb_add(MbPlan& p, int kind, int cin, int cout, int k, int stride, int act) {
    MbLayer l{};
    l.kind = kind; l.cin = cin; l.cout = cout; l.k = k; l.stride = stride; l.act = act;
    l.off = p.total;
    if (kind == MB_PW) {
        ConvLayer L;
        L.KH = k; L.KW = k; L.Cin = cin; L.Cout = cout; L.stride = 1; L.arith = 0;
        // 1x1: 32-channel K chunks (conv_ci_t would take 128 from Cin = 128 on), so that split-K 2 applies from Cin = 64 (as repvit.hip)
        L.CI_T = k == 1 ? 32 : conv_ci_t(k, k, cin, 1, cout);
        L.nchunks = cdiv(cin, L.CI_T);
        L.ncb = cdiv(cout, 32);
        int64_t off = 0;
        L.w_off = off; off += L.w_floats();
        L.b_off = off; off += L.b_floats();
        L.s_off = off; off += L.b_floats();
        l.cl = L;
        l.floats = off;
    } else if (kind == MB_STEM || kind == MB_PROJ) {
        l.floats = (int64_t)cout * cin * k * k + cout;
    } else if (kind == MB_DW) {
        l.floats = (int64_t)cout * k * k + cout;
    } else {  // SE reduce (rd, C) / expand (C, rd) 1x1 with bias
        l.floats = (int64_t)cout * cin + cout;
    }
    p.total += (l.floats + 63) / 64 * 64;
    p.layers.push_back(l);
}

static int mb_check(const nnd_mbv3_desc* d) {
    NND_REQUIRE(d, "mbv3: null descriptor");
    NND_REQUIRE(d->struct_size == (int)sizeof(nnd_mbv3_desc), "mbv3: struct_size %d != sizeof(nnd_mbv3_desc) %d (header mismatch)",
                d->struct_size, (int)sizeof(nnd_mbv3_desc));
    NND_REQUIRE(d->flags == 0, "mbv3: unknown flags 0x%x", d->flags);
    NND_REQUIRE(d->fnet_dim >= 1 && d->fnet_dim <= 4096, "mbv3: fnet_dim %d (fnet_proj output channels, 1..4096)", d->fnet_dim);
    NND_REQUIRE(d->cnet_dim >= 1 && d->cnet_dim <= 4096, "mbv3: cnet_dim %d (cnet_proj output channels, 1..4096)", d->cnet_dim);
    return NND_OK;
}

// layer order (= the tensor order of nnd_mbv3_pack): stem | per block: [IR: expand 1x1] depthwise [SE reduce, SE expand] project 1x1 |
// fnet_proj 3x3 | cnet_proj 3x3
void mb_plan_backbone(MbPlan& p) {
    mb_add(p, MB_STEM, 3, MB_STEM_C, 3, 2, MB_HSWISH);
    for (int i = 0; i < MB_NBLOCKS; ++i) {
        const MbBlock& b = MB_BLOCKS[i];
        if (b.ir) mb_add(p, MB_PW, b.cin, b.mid, 1, 1, b.act);
        mb_add(p, MB_DW, b.mid, b.mid, b.k, b.stride, b.act);
        if (b.rd) {
            mb_add(p, MB_SE_R, b.mid, b.rd, 1, 1, MB_RELU);
            mb_add(p, MB_SE_E, b.rd, b.mid, 1, 1, MB_NONE);
        }
        mb_add(p, MB_PW, b.mid, b.cout, 1, 1, MB_NONE);
    }
}

static int mb_plan(const nnd_mbv3_desc* d, MbPlan* p) {
    if (int rc = mb_check(d)) return rc;
    p->layers.clear();
    p->total = 0;
    mb_plan_backbone(*p);
    mb_add(*p, MB_PROJ, MB_S1_C, d->fnet_dim, 3, 1, MB_RELU);
    mb_add(*p, MB_PROJ, MB_S1_C, d->cnet_dim, 3, 1, MB_RELU);
    return NND_OK;
}

int64_t mb_align(int64_t n) { return (n + 63) / 64 * 64; }

// workspace: running activations A, B (ping-pong), expanded E, depthwise D, stage 1's map of both frames, SE gate, SE partials
struct MbWs {
    int64_t act, e, d, s1, gate, part;  // floats (part: doubles)
};

static MbWs mb_ws(int B, int H, int W) {
    MbWs r{};
    int h = same_out(H, 2), w = same_out(W, 2);
    r.act = (int64_t)2 * B * MB_STEM_C * h * w;
    for (int i = 0; i < MB_NBLOCKS; ++i) {
        const MbBlock& b = MB_BLOCKS[i];
        const int64_t nb = b.stage <= 1 ? 2 * B : B;
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

int run_dw(const MbLayer& l, const float* blob, const float* x, float* y, double* partial, int N, int Hin, int Win,
                  hipStream_t st) {
    const int Ho = same_out(Hin, l.stride), Wo = same_out(Win, l.stride);
    const int pt = l.stride == 1 ? l.k / 2 : same_pad_before(Hin, l.k, 2), pl = l.stride == 1 ? l.k / 2 : same_pad_before(Win, l.k, 2);
    const float* w = blob + l.off;
    const float* b = w + (int64_t)l.cout * l.k * l.k;
    dim3 grid((unsigned)cdiv(Ho * Wo, MB_DW_T), (unsigned)l.cout, (unsigned)N);
    if (l.k == 3)
        hipLaunchKernelGGL(mbv3_dw_kernel<3>, grid, dim3(MB_DW_T), 0, st, x, y, w, b, partial, l.cout, Hin, Win, Ho, Wo, l.stride, pt, pl, l.act);
    else
        hipLaunchKernelGGL(mbv3_dw_kernel<5>, grid, dim3(MB_DW_T), 0, st, x, y, w, b, partial, l.cout, Hin, Win, Ho, Wo, l.stride, pt, pl, l.act);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int run_se(const MbLayer& lr, const MbLayer& le, const float* blob, float* y, const double* partial, float* gate, int N, int H,
                  int W, hipStream_t st) {
    const int C = lr.cin, rd = lr.cout, P = H * W;
    const float* wr = blob + lr.off;
    const float* we = blob + le.off;
    hipLaunchKernelGGL(mbv3_se_kernel, dim3((unsigned)N), dim3(256), 0, st, partial, cdiv(P, MB_DW_T), P, wr, wr + (int64_t)rd * C, we,
                       we + (int64_t)C * rd, gate, C, rd);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(mbv3_gate_kernel, dim3((unsigned)cdiv(P, 256), (unsigned)C, (unsigned)N), dim3(256), 0, st, y, gate, C, P);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

// 1x1 / 3x3 stride-1 conv on conv_mfma (NCHW in / out); res: the residual (same shape as y), MB_NONE layers only
int run_pw(const MbLayer& l, const float* blob, const float* x, int64_t xbs, float* y, int64_t ybs, const float* res, int N, int H,
                  int W, hipStream_t st) {
    ConvIO io{};
    io.src0 = Act{const_cast<float*>(x), xbs, l.cin};
    io.out0 = Act{y, ybs, l.cout};
    if (res) io.aux0 = Act{const_cast<float*>(res), ybs, l.cout};
    io.Hin = H; io.Win = W;
    io.force_ks = l.cl.nchunks >= 2 ? 2 : 1;  // fixed per layer: a pair's outputs do not depend on the batch
    const int epi = l.act == MB_RELU ? EPI_RELU : l.act == MB_HSWISH ? EPI_HSWISH : EPI_AFFINE;
    return launch_conv(l.cl, blob + l.off, io, epi, N, H, W, st);
}

static int run_proj(const MbLayer& l, const float* blob, const float* x, int64_t xbs, float* y, int N, int H, int W, hipStream_t st) {
    const float* w = blob + l.off;
    dim3 grid((unsigned)cdiv(H * W, 256), (unsigned)cdiv(l.cout, MB_PJ_CO), (unsigned)N);
    hipLaunchKernelGGL(mbv3_proj_kernel, grid, dim3(256), 0, st, x, xbs, y, w, w + (int64_t)l.cout * l.cin * 9, l.cin, l.cout, H, W);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

void pack_pw(const MbLayer& l, const float* w, const float* b, float* base) {
    const float* ws[1] = {w};
    const float* bs[1] = {b};
    int co[1] = {l.cout};
    pack_conv(l.cl, 1, ws, bs, co, base);
    for (int c = 0; c < l.cl.ncb * 32; ++c) base[l.cl.s_off + c] = c < l.cout ? 1.f : 0.f;
}

// ------------------------------------------------------------------------------------------ one frame tensor (midas.hip)
// workspace: running activations A, B (ping-pong), expanded E, depthwise D, SE gate, SE partials (doubles)
struct MbWs1 {
    int64_t act, e, d, gate, part;
};

static MbWs1 mb_ws1(int B, int H, int W) {
    MbWs1 r{};
    int h = same_out(H, 2), w = same_out(W, 2);
    r.act = (int64_t)B * MB_STEM_C * h * w;
    for (int i = 0; i < MB_NBLOCKS; ++i) {
        const MbBlock& b = MB_BLOCKS[i];
        const int ho = same_out(h, b.stride), wo = same_out(w, b.stride);
        r.act = std::max(r.act, (int64_t)B * b.cout * ho * wo);
        r.e = std::max(r.e, (int64_t)B * b.mid * h * w);
        r.d = std::max(r.d, (int64_t)B * b.mid * ho * wo);
        if (b.rd) {
            r.gate = std::max(r.gate, (int64_t)B * b.mid);
            r.part = std::max(r.part, (int64_t)B * b.mid * cdiv(ho * wo, MB_DW_T));
        }
        h = ho; w = wo;
    }
    return r;
}

int64_t mb_single_ws(int B, int H, int W) {
    const MbWs1 r = mb_ws1(B, H, W);
    return 2 * mb_align(r.act) + mb_align(r.e) + mb_align(r.d) + mb_align(r.gate) + 2 * mb_align(r.part);
}

int mb_single_forward(const MbPlan& p, const float* packed, const float* frame, float* const* taps, float* workspace, int B, int H, int W,
                      hipStream_t st) {
    const MbWs1 r = mb_ws1(B, H, W);
    float* q = workspace;
    float* bufA = q; q += mb_align(r.act);
    float* bufB = q; q += mb_align(r.act);
    float* E = q; q += mb_align(r.e);
    float* D = q; q += mb_align(r.d);
    float* gate = q; q += mb_align(r.gate);
    double* part = reinterpret_cast<double*>(q);  // 64-float aligned
    size_t li = 0;
    auto L = [&]() -> const MbLayer& { return p.layers[li++]; };
    int rc;
    int h = same_out(H, 2), w = same_out(W, 2);
    {
        const MbLayer& l0 = L();
        hipLaunchKernelGGL(mbv3_stem_kernel, dim3((unsigned)cdiv(h * w, 256), 1, (unsigned)B), dim3(256), 0, st, frame, frame, B, bufA,
                           packed + l0.off, packed + l0.off + MB_STEM_C * 27, H, W, h, w, same_pad_before(H, 3, 2), same_pad_before(W, 3, 2));
        NND_LAUNCH_CHECK();
    }
    const float* x = bufA;
    for (int i = 0; i < MB_NBLOCKS; ++i) {
        const MbBlock& b = MB_BLOCKS[i];
        const int ho = same_out(h, b.stride), wo = same_out(w, b.stride);
        const bool last = i + 1 == MB_NBLOCKS || MB_BLOCKS[i + 1].stage != b.stage;
        float* keep = !last ? nullptr : b.stage == 1 ? taps[0] : b.stage == 2 ? taps[1] : b.stage == 4 ? taps[2] : b.stage == 5 ? taps[3] : nullptr;
        float* out = keep ? keep : (x == bufA ? bufB : bufA);
        const float* dwin = x;
        if (b.ir) {
            if ((rc = run_pw(L(), packed, x, (int64_t)b.cin * h * w, E, (int64_t)b.mid * h * w, nullptr, B, h, w, st))) return rc;
            dwin = E;
        }
        if ((rc = run_dw(L(), packed, dwin, D, b.rd ? part : nullptr, B, h, w, st))) return rc;
        if (b.rd) {
            const MbLayer& lr = L();
            const MbLayer& le = L();
            if ((rc = run_se(lr, le, packed, D, part, gate, B, ho, wo, st))) return rc;
        }
        if ((rc = run_pw(L(), packed, D, (int64_t)b.mid * ho * wo, out, (int64_t)b.cout * ho * wo, b.skip ? x : nullptr, B, ho, wo, st)))
            return rc;
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
    const int Ho = same_out(H, stride), Wo = same_out(W, stride);
    const int pt = stride == 1 ? k / 2 : same_pad_before(H, k, 2), pl = stride == 1 ? k / 2 : same_pad_before(W, k, 2);
    dim3 grid((unsigned)cdiv(Ho * Wo, MB_DW_T), (unsigned)C, (unsigned)N);
    hipStream_t st = (hipStream_t)stream;
    if (k == 3)
        hipLaunchKernelGGL(mbv3_dw_kernel<3>, grid, dim3(MB_DW_T), 0, st, x, y, w, bias, partial, C, H, W, Ho, Wo, stride, pt, pl, act);
    else
        hipLaunchKernelGGL(mbv3_dw_kernel<5>, grid, dim3(MB_DW_T), 0, st, x, y, w, bias, partial, C, H, W, Ho, Wo, stride, pt, pl, act);
    NND_LAUNCH_CHECK();
    return NND_OK;
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
    const int P = H * W;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mbv3_se_kernel, dim3((unsigned)N), dim3(256), 0, st, partial, cdiv(P, MB_DW_T), P, wr, br, we, be, gate, C, rd);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(mbv3_gate_kernel, dim3((unsigned)cdiv(P, 256), (unsigned)C, (unsigned)N), dim3(256), 0, st, y, gate, C, P);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_mbv3_stem(const float* x, const float* x1, int nsplit, const float* w, const float* bias, float* y, int N, int H, int W,
                  void* stream) {
    NND_REQUIRE(x && w && bias && y, "mbv3_stem: null pointer");
    NND_REQUIRE(N >= 1 && H >= 1 && W >= 1 && N <= 65535, "mbv3_stem: bad size %dx%dx%d", N, H, W);
    if (!x1) nsplit = N;
    NND_REQUIRE(nsplit >= 1 && nsplit <= N, "mbv3_stem: nsplit %d of %d", nsplit, N);
    const int Ho = same_out(H, 2), Wo = same_out(W, 2);
    hipLaunchKernelGGL(mbv3_stem_kernel, dim3((unsigned)cdiv(Ho * Wo, 256), 1, (unsigned)N), dim3(256), 0, (hipStream_t)stream, x,
                       x1 ? x1 : x, nsplit, y, w, bias, H, W, Ho, Wo, same_pad_before(H, 3, 2), same_pad_before(W, 3, 2));
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_mbv3_proj(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Cout, int H, int W, void* stream) {
    NND_REQUIRE(x && w && bias && y, "mbv3_proj: null pointer");
    NND_REQUIRE(N >= 1 && N <= 65535 && Cin >= 1 && Cin <= MB_PJ_MAXCI && Cout >= 1 && H >= 1 && W >= 1,
                "mbv3_proj: bad size N %d Cin %d Cout %d %dx%d (Cin <= %d)", N, Cin, Cout, H, W, MB_PJ_MAXCI);
    hipLaunchKernelGGL(mbv3_proj_kernel, dim3((unsigned)cdiv(H * W, 256), (unsigned)cdiv(Cout, MB_PJ_CO), (unsigned)N), dim3(256), 0,
                       (hipStream_t)stream, x, (int64_t)Cin * H * W, y, w, bias, Cin, Cout, H, W);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int64_t nnd_mbv3_pointwise_packed_floats(int Cout, int Cin, int k) {
    NND_REQUIRE(Cout >= 1 && Cin >= 1, "mbv3_pointwise: channels %d -> %d", Cin, Cout);
    NND_REQUIRE(k == 1 || k == 3, "mbv3_pointwise: kernel %d not built (1, 3)", k);
    MbPlan p;
    mb_add(p, MB_PW, Cin, Cout, k, 1, MB_NONE);
    return p.total;
}

int nnd_mbv3_pointwise_pack(int Cout, int Cin, int k, const float* w, const float* bias, float* packed_host) {
    NND_REQUIRE(Cout >= 1 && Cin >= 1 && w && bias && packed_host, "mbv3_pointwise_pack: bad argument");
    NND_REQUIRE(k == 1 || k == 3, "mbv3_pointwise_pack: kernel %d not built (1, 3)", k);
    MbPlan p;
    mb_add(p, MB_PW, Cin, Cout, k, 1, MB_NONE);
    memset(packed_host, 0, sizeof(float) * p.total);
    pack_pw(p.layers[0], w, bias, packed_host);
    return NND_OK;
}

int nnd_mbv3_pointwise(int Cout, int Cin, int k, const float* packed_dev, const float* x, const float* residual, float* y, int N, int H,
                       int W, int act, void* stream) {
    NND_REQUIRE(packed_dev && x && y && N >= 1 && H >= 1 && W >= 1, "mbv3_pointwise: bad argument");
    NND_REQUIRE(Cout >= 1 && Cin >= 1 && (k == 1 || k == 3), "mbv3_pointwise: %dx%d %d -> %d not built", k, k, Cin, Cout);
    NND_REQUIRE(act >= MB_NONE && act <= MB_HSWISH, "mbv3_pointwise: activation %d (0 none, 1 ReLU, 2 hard-swish)", act);
    NND_REQUIRE(!(act && residual), "mbv3_pointwise: an activation and a residual are not built together");
    MbPlan p;
    mb_add(p, MB_PW, Cin, Cout, k, 1, act);
    return run_pw(p.layers[0], packed_dev, x, (int64_t)Cin * H * W, y, (int64_t)Cout * H * W, residual, N, H, W, (hipStream_t)stream);
}

int nnd_mbv3_num_tensors(const nnd_mbv3_desc* desc) {
    MbPlan p;
    if (int rc = mb_plan(desc, &p)) return rc;
    return 2 * (int)p.layers.size();
}

int64_t nnd_mbv3_packed_floats(const nnd_mbv3_desc* desc) {
    MbPlan p;
    if (int rc = mb_plan(desc, &p)) return rc;
    return p.total;
}

int64_t nnd_mbv3_workspace_floats(const nnd_mbv3_desc* desc, int B, int H, int W) {
    if (int rc = mb_check(desc)) return rc;
    NND_REQUIRE(B >= 1 && H >= 1 && W >= 1 && B <= 32767, "mbv3: bad size %dx%dx%d", B, H, W);
    const MbWs r = mb_ws(B, H, W);
    return 2 * mb_align(r.act) + mb_align(r.e) + mb_align(r.d) + mb_align(r.s1) + mb_align(r.gate) + 2 * mb_align(r.part);
}

int nnd_mbv3_pack(const nnd_mbv3_desc* desc, const float* const* t, float* packed_host) {
    MbPlan p;
    if (int rc = mb_plan(desc, &p)) return rc;
    NND_REQUIRE(t && packed_host, "mbv3_pack: null pointer");
    memset(packed_host, 0, sizeof(float) * p.total);
    for (size_t i = 0; i < p.layers.size(); ++i) {
        const MbLayer& l = p.layers[i];
        const float *w = t[2 * i], *b = t[2 * i + 1];
        NND_REQUIRE(w && b, "mbv3_pack: layer %zu: weight / bias missing", i);
        float* base = packed_host + l.off;
        if (l.kind == MB_PW) {
            pack_pw(l, w, b, base);
        } else {
            const int64_t nw = l.floats - l.cout;
            memcpy(base, w, sizeof(float) * nw);
            memcpy(base + nw, b, sizeof(float) * l.cout);
        }
    }
    return NND_OK;
}

int nnd_mbv3_forward(const nnd_mbv3_desc* desc, const float* packed, const float* frame1, const float* frame2, float* fmap1, float* fmap2,
                     float* cnet1, float* guide0, float* guide1, float* guide2, float* workspace, int B, int H, int W, void* stream) {
    MbPlan p;
    if (int rc = mb_plan(desc, &p)) return rc;
    NND_REQUIRE(packed && frame1 && frame2 && fmap1 && fmap2 && cnet1 && guide0 && guide1 && guide2 && workspace,
                "mbv3_forward: null pointer");
    NND_REQUIRE(B >= 1 && H >= 1 && W >= 1 && B <= 32767, "mbv3_forward: bad size %dx%dx%d", B, H, W);
    hipStream_t st = (hipStream_t)stream;
    const MbWs r = mb_ws(B, H, W);
    float* q = workspace;
    float* bufA = q; q += mb_align(r.act);
    float* bufB = q; q += mb_align(r.act);
    float* E = q; q += mb_align(r.e);
    float* D = q; q += mb_align(r.d);
    float* s1 = q; q += mb_align(r.s1);
    float* gate = q; q += mb_align(r.gate);
    double* part = reinterpret_cast<double*>(q);  // 64-float aligned
    const int N = 2 * B;
    size_t li = 0;
    auto L = [&]() -> const MbLayer& { return p.layers[li++]; };
    int rc;
    int h = same_out(H, 2), w = same_out(W, 2);
    {
        const MbLayer& l0 = L();
        hipLaunchKernelGGL(mbv3_stem_kernel, dim3((unsigned)cdiv(h * w, 256), 1, (unsigned)N), dim3(256), 0, st, frame1, frame2, B, bufA,
                           packed + l0.off, packed + l0.off + MB_STEM_C * 27, H, W, h, w, same_pad_before(H, 3, 2), same_pad_before(W, 3, 2));
        NND_LAUNCH_CHECK();
    }
    const float* x = bufA;
    for (int i = 0; i < MB_NBLOCKS; ++i) {
        const MbBlock& b = MB_BLOCKS[i];
        const int nb = b.stage <= 1 ? N : B;  // stages 2..5: the left frames (the first B samples) only
        const int ho = same_out(h, b.stride), wo = same_out(w, b.stride);
        const bool last = i + 1 == MB_NBLOCKS || MB_BLOCKS[i + 1].stage != b.stage;
        float* keep = !last ? nullptr : b.stage == 1 ? s1 : b.stage == 2 ? guide0 : b.stage == 3 ? guide1 : b.stage == 5 ? guide2 : nullptr;
        float* out = keep ? keep : (x == bufA ? bufB : bufA);
        const float* dwin = x;
        if (b.ir) {
            if ((rc = run_pw(L(), packed, x, (int64_t)b.cin * h * w, E, (int64_t)b.mid * h * w, nullptr, nb, h, w, st))) return rc;
            dwin = E;
        }
        if ((rc = run_dw(L(), packed, dwin, D, b.rd ? part : nullptr, nb, h, w, st))) return rc;
        if (b.rd) {
            const MbLayer& lr = L();
            const MbLayer& le = L();
            if ((rc = run_se(lr, le, packed, D, part, gate, nb, ho, wo, st))) return rc;
        }
        if ((rc = run_pw(L(), packed, D, (int64_t)b.mid * ho * wo, out, (int64_t)b.cout * ho * wo, b.skip ? x : nullptr, nb, ho, wo, st)))
            return rc;
        x = out;
        h = ho; w = wo;
        if (b.stage == 1 && last) {  // fnet_proj on both frames' stage-1 map, cnet_proj on the left frames'
            const int h1 = h, w1 = w;
            const MbLayer& fp = p.layers[p.layers.size() - 2];
            const MbLayer& cp = p.layers[p.layers.size() - 1];
            const int64_t sbs = (int64_t)MB_S1_C * h1 * w1;
            if ((rc = run_proj(fp, packed, s1, sbs, fmap1, B, h1, w1, st))) return rc;
            if ((rc = run_proj(fp, packed, s1 + B * sbs, sbs, fmap2, B, h1, w1, st))) return rc;
            if ((rc = run_proj(cp, packed, s1, sbs, cnet1, B, h1, w1, st))) return rc;
        }
    }
    NND_REQUIRE(li + 2 == p.layers.size(), "mbv3_forward: %zu of %zu layers consumed (plan mismatch)", li, p.layers.size());
    return NND_OK;
}

}  // extern "C"
