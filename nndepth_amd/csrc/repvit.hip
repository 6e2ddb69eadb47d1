// Encoder side of Coarse2FineGroupRepViTRAFTStereo in ONE C-ABI call (nnd_repvit_forward): the RepViT backbone
// (nndepth/encoders/rep_vit.py:482-744), the three MobileOne cnet_proj blocks (nndepth/models/raft_stereo/model.py:216-222) and
// the two FeatureFusionBlocks (model.py:223-228, nndepth/blocks/conv.py:549-567).  Exact fp32 throughout: no split arithmetic,
// no calibration.
//
// Every train-time branch is folded on the host (ops.RepViTEngine, float64, cast once to fp32), so the device runs a plain chain:
//   stem.0   3x3 dense (3 -> 16), stride s0, GELU        stem_conv_kernel (VALU: 29.5 us for a 512x960 pair, 114 VGPRs, no
//                                                        scratch; conv_mfma on the same shape, K = 27 in 16-channel stride-2
//                                                        chunks, 193 us)
//   stem.1   3x3 depthwise, stride s1, GELU              dwconv_kernel<3>
//   stem.2   1x1 (16 -> 16), stride s2, GELU             conv_mfma, EPI_GELU
//   stage i  patch embed: k x k depthwise (small 3x3 folded in), stride d_i, NO activation (conv.py:454)   dwconv_kernel<k>
//            1x1 (-> C_i) + GELU                                                                           conv_mfma, EPI_GELU
//            RepFormerBlock: token mixer = ONE 3x3 depthwise (identity, mixer and norm folded)             dwconv_kernel<3>
//                            [FFN: fc1 + GELU; fc2 with x + ls * (.) in the epilogue]                       conv_mfma EPI_GELU / EPI_AFFINE
//            AttentionBlock: qkv_proj (BatchNorm folded in) -> linear attention -> out_proj, x + ls1 * (.)  conv_mfma, linattn_kernel
//                            FFN as above with ls2
//   fusion   relu(conv3(cat[conv1(up(a)), conv2(b)])) with 1x1 convs = relu(up(A a + a0) + B b + b0): conv3's halves composed with
//            conv1 / conv2 on the host, A applied at the coarse resolution (a 1x1 conv commutes with the bilinear upsample, whose
//            weights sum to 1), no torch.cat materialised                          conv_mfma x 2, upsample_add_relu_kernel
//   cnet_proj[j] 1x1 + GELU on the left frames' map                                conv_mfma, EPI_GELU
// The layer scales ride in EPI_AFFINE's per-channel scale (y = residual + acc * ls + ls * bias): the epilogue already carries a
// per-channel scale, so the weights stay as trained and no new epilogue mode is needed.
// Every conv_mfma launch fixes its split-K factor per layer (ConvIO::force_ks: 2 from two 32-channel K chunks on, else 1): each output
// has the same K order whatever the batch, so a pair's maps do not depend on the batch it runs in, and the two half-K chains keep the
// fp32 accumulation error at PyTorch's level.  The depthwise kernels accumulate in float64 and round once.  Activations are NCHW in the caller's workspace.
#include "common.h"
#include "bilinear.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace nnd {

__device__ __forceinline__ float gelu_exact(float v) { return v * 0.5f * (1.0f + erff(v * 0.707106781186547524f)); }

// ------------------------------------------------------------------------------------------ depthwise k x k
// One thread per output pixel of one (sample, channel) plane; padding k/2, output (Hin - 1) / stride + 1 (PyTorch's formula for
// padding k/2, odd k).  Taps in (dy, dx) order, bias, optional GELU.  grid (ceil(Ho*Wo / 256), C, N)
template <int K>
__global__ void __launch_bounds__(256) dwconv_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ w,
                                                     const float* __restrict__ bias, int C, int Hin, int Win, int Ho, int Wo, int stride,
                                                     int gelu) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= Ho * Wo) return;
    const int c = blockIdx.y, n = blockIdx.z;
    const int oy = idx / Wo, ox = idx - oy * Wo;
    const float* xp = x + ((long)n * C + c) * Hin * Win;
    const float* wp = w + (long)c * K * K;
    const int iy0 = oy * stride - K / 2, ix0 = ox * stride - K / 2;
    // float64 accumulation, rounded once: a 49-tap fp32 chain was 3-4.5x PyTorch's own fp32 error at k = 7 (per-kernel test); the
    // kernel is bound by latency / HBM, not by its 2 x 49 flops per output
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
    float v = (float)(acc + (double)bias[c]);
    if (gelu) v = gelu_exact(v);
    y[((long)n * C + c) * Ho * Wo + idx] = v;
}

// ------------------------------------------------------------------------------------------ stem.0: 3x3 dense, 3 -> STEM_C
// Samples n < nsplit read `x`, the others `x1` (the two frame tensors where they lie).  One thread per output pixel, all STEM_C
// output channels; the 27 x STEM_C weights sit in LDS.
constexpr int STEM_C = 16;
__global__ void __launch_bounds__(256) stem_conv_kernel(const float* __restrict__ x, const float* __restrict__ x1, int nsplit,
                                                        float* __restrict__ y, const float* __restrict__ w, const float* __restrict__ bias,
                                                        int Hin, int Win, int Ho, int Wo, int stride) {
    __shared__ float ws[STEM_C * 27 + STEM_C];
    for (int i = threadIdx.x; i < STEM_C * 28; i += 256) ws[i] = i < STEM_C * 27 ? w[i] : bias[i - STEM_C * 27];
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
                const int iy = oy * stride - 1 + dy, ix = ox * stride - 1 + dx;
                const bool ok = iy >= 0 && iy < Hin && ix >= 0 && ix < Win;
                in[(ci * 3 + dy) * 3 + dx] = ok ? xp[((long)ci * Hin + iy) * Win + ix] : 0.f;
            }
    float* yp = y + (long)n * STEM_C * Ho * Wo + idx;
#pragma unroll 4
    for (int co = 0; co < STEM_C; ++co) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 27; ++k) acc = fmaf(ws[co * 27 + k], in[k], acc);
        yp[(long)co * Ho * Wo] = gelu_exact(acc + ws[STEM_C * 27 + co]);
    }
}

// ------------------------------------------------------------------------------------------ linear self-attention
// LinearSelfAttention.forward (nndepth/blocks/attn_block.py:151-169) on the 4-D map: per (sample, row) the softmax over W of the
// query channel, context[c] = sum_w key[c, w] * score[w], out[c, w] = relu(value[c, w]) * context[c].
// qkv (N, 1 + 2C, H, W) -> out (N, C, H, W).  One workgroup per (row, sample); scores in LDS (W <= LINATTN_MAXW).
constexpr int LINATTN_MAXW = 4096;
__global__ void __launch_bounds__(256) linattn_kernel(const float* __restrict__ qkv, float* __restrict__ out, int C, int H, int W) {
    __shared__ float sc[LINATTN_MAXW];
    __shared__ float red[256];
    const int row = blockIdx.x, n = blockIdx.y, t = threadIdx.x;
    const long plane = (long)H * W;
    const float* q = qkv + (long)n * (1 + 2 * C) * plane + (long)row * W;
    float m = -INFINITY;
    for (int w = t; w < W; w += 256) m = fmaxf(m, q[w]);
    red[t] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] = fmaxf(red[t], red[t + s]);
        __syncthreads();
    }
    m = red[0];
    __syncthreads();
    float part = 0.f;
    for (int w = t; w < W; w += 256) {
        const float e = expf(q[w] - m);
        sc[w] = e;
        part += e;
    }
    red[t] = part;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const float sum = red[0];
    for (int w = t; w < W; w += 256) sc[w] = sc[w] / sum;
    __syncthreads();
    for (int c = t; c < C; c += 256) {
        const float* k = q + (long)(1 + c) * plane;
        const float* v = q + (long)(1 + C + c) * plane;
        float ctx = 0.f;
        for (int w = 0; w < W; ++w) ctx = fmaf(k[w], sc[w], ctx);
        float* o = out + ((long)n * C + c) * plane + (long)row * W;
        for (int w = 0; w < W; ++w) o[w] = fmaxf(v[w], 0.f) * ctx;
    }
}

// ------------------------------------------------------------------------------------------ fusion: y = relu(y + up(a))
// up = F.interpolate(a, size=(H, W), mode="bilinear", align_corners=False) with the sampling of nnd_resize_normalize (bilinear.h).
// a (N, C, h, w), y (N, C, H, W) in place.  grid (ceil(H*W / 256), C, N)
__global__ void __launch_bounds__(256) upsample_add_relu_kernel(const float* __restrict__ a, float* __restrict__ y, int C, int h, int w,
                                                                int H, int W) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= H * W) return;
    const int c = blockIdx.y, n = blockIdx.z;
    const int oy = idx / W, ox = idx - oy * W;
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    src_index((float)h / (float)H, oy, h, y0, y1, ly0, ly1);
    src_index((float)w / (float)W, ox, w, x0, x1, lx0, lx1);
    const float* s = a + ((long)n * C + c) * h * w;
    const float t0 = fmaf(s[(long)y0 * w + x1], lx1, s[(long)y0 * w + x0] * lx0);
    const float t1 = fmaf(s[(long)y1 * w + x1], lx1, s[(long)y1 * w + x0] * lx0);
    const float up = fmaf(t1, ly1, t0 * ly0);
    float* yp = y + ((long)n * C + c) * H * W + idx;
    *yp = fmaxf(*yp + up, 0.f);
}

// ------------------------------------------------------------------------------------------ plan
enum RvKind { RV_STEM = 0, RV_DW = 1, RV_PW = 2 };
enum RvAct { RV_NONE = 0, RV_GELU = 1, RV_RESID = 2 };  // RV_RESID: y = x_in + scale * (acc + bias) (EPI_AFFINE, residual)

struct RvLayer {
    int kind, cin, cout, k, stride, act;
    ConvLayer cl;         // RV_PW: conv_mfma layout
    int64_t off, floats;  // blob offset / size (RV_STEM, RV_DW: weights then bias)
};

struct RvPlan {
    std::vector<RvLayer> layers;
    int64_t total = 0;
};

static int rv_add(RvPlan& p, int kind, int cin, int cout, int k, int stride, int act) {
    RvLayer l{};
    l.kind = kind; l.cin = cin; l.cout = cout; l.k = k; l.stride = stride; l.act = act;
    l.off = p.total;
    if (kind == RV_PW) {
        NND_REQUIRE(stride == 1 || stride == 2, "repvit: stride %d", stride);
        ConvLayer L;
        L.KH = 1; L.KW = 1; L.Cin = cin; L.Cout = cout; L.stride = stride; L.arith = 0;
        // 32-channel K chunks at stride 1 (conv_ci_t would take 128 from Cin = 128 on), so that split-K 2 (run_pw) applies from Cin = 64
        L.CI_T = stride == 1 ? 32 : conv_ci_t(1, 1, cin, stride, cout);
        L.nchunks = cdiv(cin, L.CI_T);
        L.ncb = cdiv(cout, 32);
        int64_t off = 0;
        L.w_off = off; off += L.w_floats();
        L.b_off = off; off += L.b_floats();
        L.s_off = off; off += L.b_floats();
        l.cl = L;
        l.floats = off;
    } else {
        l.floats = (int64_t)cout * (kind == RV_STEM ? cin : 1) * k * k + cout;
    }
    p.total += (l.floats + 63) / 64 * 64;
    p.layers.push_back(l);
    return NND_OK;
}

static int rv_check(const nnd_repvit_desc* d) {
    NND_REQUIRE(d, "repvit: null descriptor");
    NND_REQUIRE(d->struct_size == (int)sizeof(nnd_repvit_desc), "repvit: struct_size %d != sizeof(nnd_repvit_desc) %d (header mismatch)",
                d->struct_size, (int)sizeof(nnd_repvit_desc));
    NND_REQUIRE(d->flags == 0, "repvit: unknown flags 0x%x", d->flags);
    for (int i = 0; i < 3; ++i)
        NND_REQUIRE(d->stem_strides[i] == 1 || d->stem_strides[i] == 2, "repvit: stem stride %d not built (1 or 2, as (1, 1) / (2, 2))",
                    d->stem_strides[i]);
    NND_REQUIRE(d->patch_size == 3 || d->patch_size == 5 || d->patch_size == 7,
                "repvit: patch_size %d not built (odd 3, 5, 7: the depthwise kernels; an even size has no centred small kernel)", d->patch_size);
    for (int i = 0; i < 4; ++i) {
        NND_REQUIRE(d->down_strides[i] == 1 || d->down_strides[i] == 2, "repvit: downsample stride %d not built (1 or 2)", d->down_strides[i]);
        NND_REQUIRE(d->channels[i] >= 1 && d->channels[i] <= 1024, "repvit: stage %d channels %d", i, d->channels[i]);
        NND_REQUIRE(d->num_blocks[i] >= 0 && d->num_blocks[i] <= 64, "repvit: stage %d blocks %d", i, d->num_blocks[i]);
        NND_REQUIRE(d->mixer[i] == 0 || d->mixer[i] == 1, "repvit: stage %d token mixer %d (0 repmixer, 1 attention)", i, d->mixer[i]);
        NND_REQUIRE(d->ffn_hidden[i] >= 0 && d->ffn_hidden[i] <= 8192, "repvit: stage %d ffn hidden %d", i, d->ffn_hidden[i]);
        NND_REQUIRE(d->mixer[i] == 0 || d->ffn_hidden[i] > 0, "repvit: attention stage %d needs its FFN", i);
    }
    NND_REQUIRE(d->cnet_dim >= 1 && d->fusion_dim[0] >= 1 && d->fusion_dim[1] >= 1, "repvit: cnet / fusion channels");
    return NND_OK;
}

static int rv_plan(const nnd_repvit_desc* d, RvPlan* p) {
    if (int rc = rv_check(d)) return rc;
    p->layers.clear();
    p->total = 0;
    rv_add(*p, RV_STEM, 3, STEM_C, 3, d->stem_strides[0], RV_GELU);
    rv_add(*p, RV_DW, STEM_C, STEM_C, 3, d->stem_strides[1], RV_GELU);
    if (int rc = rv_add(*p, RV_PW, STEM_C, STEM_C, 1, d->stem_strides[2], RV_GELU)) return rc;
    int cin = STEM_C;
    for (int i = 0; i < 4; ++i) {
        const int c = d->channels[i];
        rv_add(*p, RV_DW, cin, cin, d->patch_size, d->down_strides[i], RV_NONE);
        rv_add(*p, RV_PW, cin, c, 1, 1, RV_GELU);
        for (int b = 0; b < d->num_blocks[i]; ++b) {
            if (d->mixer[i] == 0) {
                rv_add(*p, RV_DW, c, c, 3, 1, RV_NONE);
            } else {
                rv_add(*p, RV_PW, c, 1 + 2 * c, 1, 1, RV_NONE);  // qkv_proj (norm folded)
                rv_add(*p, RV_PW, c, c, 1, 1, RV_RESID);         // out_proj, x + ls1 * (.)
            }
            if (d->ffn_hidden[i] > 0) {
                rv_add(*p, RV_PW, c, d->ffn_hidden[i], 1, 1, RV_GELU);  // fc1
                rv_add(*p, RV_PW, d->ffn_hidden[i], c, 1, 1, RV_RESID);  // fc2, x + ls * (.)
            }
        }
        cin = c;
    }
    const int f0 = d->fusion_dim[0], f1 = d->fusion_dim[1];
    rv_add(*p, RV_PW, d->channels[3], d->cnet_dim, 1, 1, RV_GELU);  // cnet_proj[0..2]
    rv_add(*p, RV_PW, f0, d->cnet_dim, 1, 1, RV_GELU);
    rv_add(*p, RV_PW, f0, d->cnet_dim, 1, 1, RV_GELU);
    rv_add(*p, RV_PW, d->channels[3], f0, 1, 1, RV_NONE);  // fusion 0: coarse (stage 3) / fine (stage 1) halves
    rv_add(*p, RV_PW, d->channels[1], f0, 1, 1, RV_NONE);
    rv_add(*p, RV_PW, f0, f1, 1, 1, RV_NONE);              // fusion 1: coarse (fused 1) / fine (stem)
    rv_add(*p, RV_PW, STEM_C, f1, 1, 1, RV_NONE);
    return NND_OK;
}

static inline int conv_out(int n, int stride) { return (n - 1) / stride + 1; }  // padding k/2, odd k: PyTorch's formula

struct RvShapes {
    int h[6], w[6];  // 0: frames, 1: stem, 2..5: stages 0..3
    int h_stem0, w_stem0, h_stem1, w_stem1;
};

static RvShapes rv_shapes(const nnd_repvit_desc* d, int H, int W) {
    RvShapes s;
    s.h[0] = H; s.w[0] = W;
    s.h_stem0 = conv_out(H, d->stem_strides[0]); s.w_stem0 = conv_out(W, d->stem_strides[0]);
    s.h_stem1 = conv_out(s.h_stem0, d->stem_strides[1]); s.w_stem1 = conv_out(s.w_stem0, d->stem_strides[1]);
    s.h[1] = conv_out(s.h_stem1, d->stem_strides[2]); s.w[1] = conv_out(s.w_stem1, d->stem_strides[2]);
    for (int i = 0; i < 4; ++i) {
        s.h[i + 2] = conv_out(s.h[i + 1], d->down_strides[i]);
        s.w[i + 2] = conv_out(s.w[i + 1], d->down_strides[i]);
    }
    return s;
}

// workspace: 4 general buffers of `m` floats + the stem output + stage 1's output + the two coarse fusion halves
struct RvWs {
    int64_t m, stem, s1, a0, a1;
};

static RvWs rv_ws(const nnd_repvit_desc* d, int N, int H, int W) {
    const RvShapes s = rv_shapes(d, H, W);
    int64_t m = (int64_t)STEM_C * s.h_stem0 * s.w_stem0;
    m = std::max<int64_t>(m, (int64_t)STEM_C * s.h_stem1 * s.w_stem1);
    int cin = STEM_C;
    for (int i = 0; i < 4; ++i) {
        const int64_t pin = (int64_t)s.h[i + 1] * s.w[i + 1], pout = (int64_t)s.h[i + 2] * s.w[i + 2];
        const int c = d->channels[i];
        m = std::max<int64_t>(m, cin * pin);
        const int widest = std::max({c, d->ffn_hidden[i], d->mixer[i] ? 1 + 2 * c : 0, cin});
        m = std::max<int64_t>(m, (int64_t)widest * pout);
        cin = c;
    }
    RvWs r;
    r.m = m * N;
    r.stem = (int64_t)N * STEM_C * s.h[1] * s.w[1];
    r.s1 = (int64_t)N * d->channels[1] * s.h[3] * s.w[3];
    r.a0 = (int64_t)N * d->fusion_dim[0] * s.h[5] * s.w[5];
    r.a1 = (int64_t)N * d->fusion_dim[1] * s.h[3] * s.w[3];
    return r;
}

static int64_t rv_align(int64_t n) { return (n + 63) / 64 * 64; }

static int run_dw(const RvLayer& l, const float* blob, const float* x, float* y, int N, int Hin, int Win, hipStream_t st) {
    const int Ho = conv_out(Hin, l.stride), Wo = conv_out(Win, l.stride);
    const float* w = blob + l.off;
    const float* b = w + (int64_t)l.cout * l.k * l.k;
    dim3 grid((unsigned)cdiv(Ho * Wo, 256), (unsigned)l.cout, (unsigned)N);
    const int g = l.act == RV_GELU;
    if (l.k == 3) hipLaunchKernelGGL(dwconv_kernel<3>, grid, dim3(256), 0, st, x, y, w, b, l.cout, Hin, Win, Ho, Wo, l.stride, g);
    else if (l.k == 5) hipLaunchKernelGGL(dwconv_kernel<5>, grid, dim3(256), 0, st, x, y, w, b, l.cout, Hin, Win, Ho, Wo, l.stride, g);
    else hipLaunchKernelGGL(dwconv_kernel<7>, grid, dim3(256), 0, st, x, y, w, b, l.cout, Hin, Win, Ho, Wo, l.stride, g);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

// 1x1 conv on conv_mfma (NCHW in / out); res: the residual of RV_RESID (same shape as y)
static int run_pw(const RvLayer& l, const float* blob, const float* x, int64_t xbs, float* y, int64_t ybs, const float* res, int N, int Hin,
                  int Win, hipStream_t st) {
    const int Ho = conv_out(Hin, l.stride), Wo = conv_out(Win, l.stride);
    ConvIO io{};
    io.src0 = Act{const_cast<float*>(x), xbs, l.cin};
    io.out0 = Act{y, ybs, l.cout};
    if (res) io.aux0 = Act{const_cast<float*>(res), ybs, l.cout};
    io.Hin = Hin; io.Win = Win;
    // split-K fixed per layer (2 where the layer has 2+ chunks): the two half-K partial tiles are summed in wave order, which halves
    // the MFMA accumulation chain (a 128- / 384-deep chain was up to 2.7x PyTorch's own fp32 error), and a fixed ks keeps every
    // output's K order independent of the batch
    io.force_ks = l.cl.nchunks >= 2 ? 2 : 1;
    return launch_conv(l.cl, blob + l.off, io, l.act == RV_GELU ? EPI_GELU : EPI_AFFINE, N, Ho, Wo, st);
}

}  // namespace nnd

using namespace nnd;

extern "C" {

// ---- the encoder side's kernels one at a time (the launchers nnd_repvit_forward uses; per-kernel tests and profiles)
int nnd_repvit_depthwise(const float* x, const float* w, const float* bias, float* y, int N, int C, int H, int W, int k, int stride,
                         int gelu, void* stream) {
    NND_REQUIRE(x && w && bias && y, "repvit_depthwise: null pointer");
    NND_REQUIRE(k == 3 || k == 5 || k == 7, "repvit_depthwise: kernel %d not built (3, 5, 7)", k);
    NND_REQUIRE(stride == 1 || stride == 2, "repvit_depthwise: stride %d not built (1, 2)", stride);
    NND_REQUIRE(N >= 1 && C >= 1 && H >= 1 && W >= 1 && C <= 65535 && N <= 65535, "repvit_depthwise: bad size %dx%dx%dx%d", N, C, H, W);
    const int Ho = conv_out(H, stride), Wo = conv_out(W, stride);
    dim3 grid((unsigned)cdiv(Ho * Wo, 256), (unsigned)C, (unsigned)N);
    hipStream_t st = (hipStream_t)stream;
    if (k == 3) hipLaunchKernelGGL(dwconv_kernel<3>, grid, dim3(256), 0, st, x, y, w, bias, C, H, W, Ho, Wo, stride, gelu ? 1 : 0);
    else if (k == 5) hipLaunchKernelGGL(dwconv_kernel<5>, grid, dim3(256), 0, st, x, y, w, bias, C, H, W, Ho, Wo, stride, gelu ? 1 : 0);
    else hipLaunchKernelGGL(dwconv_kernel<7>, grid, dim3(256), 0, st, x, y, w, bias, C, H, W, Ho, Wo, stride, gelu ? 1 : 0);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_repvit_stem(const float* x, const float* x1, int nsplit, const float* w, const float* bias, float* y, int N, int H, int W, int stride,
                    void* stream) {
    NND_REQUIRE(x && w && bias && y, "repvit_stem: null pointer");
    NND_REQUIRE(stride == 1 || stride == 2, "repvit_stem: stride %d not built (1, 2)", stride);
    NND_REQUIRE(N >= 1 && H >= 1 && W >= 1 && N <= 65535, "repvit_stem: bad size %dx%dx%d", N, H, W);
    if (!x1) nsplit = N;
    NND_REQUIRE(nsplit >= 1 && nsplit <= N, "repvit_stem: nsplit %d of %d", nsplit, N);
    const int Ho = conv_out(H, stride), Wo = conv_out(W, stride);
    hipLaunchKernelGGL(stem_conv_kernel, dim3((unsigned)cdiv(Ho * Wo, 256), 1, (unsigned)N), dim3(256), 0, (hipStream_t)stream, x,
                       x1 ? x1 : x, nsplit, y, w, bias, H, W, Ho, Wo, stride);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int64_t nnd_repvit_pointwise_packed_floats(int Cout, int Cin, int stride) {
    RvPlan p;
    NND_REQUIRE(Cout >= 1 && Cin >= 1, "repvit_pointwise: channels %d -> %d", Cin, Cout);
    if (int rc = rv_add(p, RV_PW, Cin, Cout, 1, stride, RV_NONE)) return rc;
    return p.total;
}

int nnd_repvit_pointwise_pack(int Cout, int Cin, int stride, const float* w, const float* bias, const float* scale, float* packed_host) {
    RvPlan p;
    NND_REQUIRE(Cout >= 1 && Cin >= 1 && w && bias && packed_host, "repvit_pointwise_pack: bad argument");
    if (int rc = rv_add(p, RV_PW, Cin, Cout, 1, stride, RV_NONE)) return rc;
    const RvLayer& l = p.layers[0];
    memset(packed_host, 0, sizeof(float) * p.total);
    const float* ws[1] = {w};
    const float* bs[1] = {bias};
    int co[1] = {Cout};
    pack_conv(l.cl, 1, ws, bs, co, packed_host);
    for (int c = 0; c < l.cl.ncb * 32; ++c) packed_host[l.cl.s_off + c] = c < Cout ? (scale ? scale[c] : 1.f) : 0.f;
    return NND_OK;
}

int nnd_repvit_pointwise(int Cout, int Cin, int stride, const float* packed_dev, const float* x, const float* residual, float* y, int N,
                         int H, int W, int gelu, void* stream) {
    RvPlan p;
    NND_REQUIRE(packed_dev && x && y && N >= 1 && H >= 1 && W >= 1, "repvit_pointwise: bad argument");
    NND_REQUIRE(!(gelu && residual), "repvit_pointwise: GELU and a residual are not built together");
    if (int rc = rv_add(p, RV_PW, Cin, Cout, 1, stride, gelu ? RV_GELU : (residual ? RV_RESID : RV_NONE))) return rc;
    const int Ho = conv_out(H, stride), Wo = conv_out(W, stride);
    return run_pw(p.layers[0], packed_dev, x, (int64_t)Cin * H * W, y, (int64_t)Cout * Ho * Wo, residual, N, H, W, (hipStream_t)stream);
}

int nnd_repvit_linear_attention(const float* qkv, float* out, int N, int C, int H, int W, void* stream) {
    NND_REQUIRE(qkv && out && N >= 1 && C >= 1 && H >= 1 && W >= 1 && N <= 65535, "repvit_linear_attention: bad argument");
    NND_REQUIRE(W <= LINATTN_MAXW, "repvit_linear_attention: row of %d > %d columns", W, LINATTN_MAXW);
    hipLaunchKernelGGL(linattn_kernel, dim3((unsigned)H, (unsigned)N), dim3(256), 0, (hipStream_t)stream, qkv, out, C, H, W);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_repvit_upsample_add_relu(const float* a, float* y, int N, int C, int h, int w, int H, int W, void* stream) {
    NND_REQUIRE(a && y && N >= 1 && C >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1 && C <= 65535 && N <= 65535,
                "repvit_upsample_add_relu: bad argument");
    dim3 grid((unsigned)cdiv(H * W, 256), (unsigned)C, (unsigned)N);
    hipLaunchKernelGGL(upsample_add_relu_kernel, grid, dim3(256), 0, (hipStream_t)stream, a, y, C, h, w, H, W);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_repvit_num_tensors(const nnd_repvit_desc* desc) {
    RvPlan p;
    if (int rc = rv_plan(desc, &p)) return rc;
    return 3 * (int)p.layers.size();
}

int64_t nnd_repvit_packed_floats(const nnd_repvit_desc* desc) {
    RvPlan p;
    if (int rc = rv_plan(desc, &p)) return rc;
    return p.total;
}

int64_t nnd_repvit_workspace_floats(const nnd_repvit_desc* desc, int N, int H, int W) {
    if (int rc = rv_check(desc)) return rc;
    NND_REQUIRE(N >= 1 && H >= 1 && W >= 1, "repvit: bad size %dx%dx%d", N, H, W);
    const RvWs r = rv_ws(desc, N, H, W);
    return 4 * rv_align(r.m) + rv_align(r.stem) + rv_align(r.s1) + rv_align(r.a0) + rv_align(r.a1);
}

int nnd_repvit_pack(const nnd_repvit_desc* desc, const float* const* t, float* packed_host) {
    RvPlan p;
    if (int rc = rv_plan(desc, &p)) return rc;
    NND_REQUIRE(t && packed_host, "repvit_pack: null pointer");
    memset(packed_host, 0, sizeof(float) * p.total);
    for (size_t i = 0; i < p.layers.size(); ++i) {
        const RvLayer& l = p.layers[i];
        const float *w = t[3 * i], *b = t[3 * i + 1], *s = t[3 * i + 2];
        NND_REQUIRE(w && b, "repvit_pack: layer %zu: weight / bias missing", i);
        float* base = packed_host + l.off;
        if (l.kind == RV_PW) {
            const float* ws[1] = {w};
            const float* bs[1] = {b};
            int co[1] = {l.cout};
            pack_conv(l.cl, 1, ws, bs, co, base);
            for (int c = 0; c < l.cl.ncb * 32; ++c) base[l.cl.s_off + c] = c < l.cout ? (s ? s[c] : 1.f) : 0.f;
        } else {
            NND_REQUIRE(!s, "repvit_pack: layer %zu (depthwise / stem) takes no scale", i);
            const int64_t nw = (int64_t)l.cout * (l.kind == RV_STEM ? l.cin : 1) * l.k * l.k;
            memcpy(base, w, sizeof(float) * nw);
            memcpy(base + nw, b, sizeof(float) * l.cout);
        }
    }
    return NND_OK;
}

int nnd_repvit_forward(const nnd_repvit_desc* desc, const float* packed, const float* frames, const float* frames_b, int nsplit,
                       float* feat0, float* feat1, float* feat2, float* cnet0, float* cnet1, float* cnet2, float* workspace, int N, int H,
                       int W, void* stream) {
    RvPlan p;
    if (int rc = rv_plan(desc, &p)) return rc;
    NND_REQUIRE(packed && frames && feat0 && feat1 && feat2 && cnet0 && cnet1 && cnet2 && workspace, "repvit_forward: null pointer");
    NND_REQUIRE(N >= 1 && H >= 1 && W >= 1, "repvit_forward: bad size %dx%dx%d", N, H, W);
    if (!frames_b) nsplit = N;
    NND_REQUIRE(nsplit >= 1 && nsplit <= N, "repvit_forward: nsplit %d of %d samples", nsplit, N);
    const int B = frames_b ? nsplit : N;  // cnets: the left frames (the first half with frames_b)
    hipStream_t st = (hipStream_t)stream;
    const RvShapes s = rv_shapes(desc, H, W);
    const RvWs r = rv_ws(desc, N, H, W);
    float* buf[4];
    float* q = workspace;
    for (int i = 0; i < 4; ++i, q += rv_align(r.m)) buf[i] = q;
    float* stem = q; q += rv_align(r.stem);
    float* s1 = q; q += rv_align(r.s1);
    float* a0 = q; q += rv_align(r.a0);
    float* a1 = q;
    size_t li = 0;
    auto L = [&]() -> const RvLayer& { return p.layers[li++]; };
    auto bs = [](int c, int h, int w) { return (int64_t)c * h * w; };
    int rc;
    {   // stem
        const RvLayer& l0 = L();
        dim3 grid((unsigned)cdiv(s.h_stem0 * s.w_stem0, 256), 1, (unsigned)N);
        hipLaunchKernelGGL(stem_conv_kernel, grid, dim3(256), 0, st, frames, frames_b ? frames_b : frames, nsplit, buf[0], packed + l0.off,
                           packed + l0.off + STEM_C * 27, H, W, s.h_stem0, s.w_stem0, l0.stride);
        NND_LAUNCH_CHECK();
        if ((rc = run_dw(L(), packed, buf[0], buf[1], N, s.h_stem0, s.w_stem0, st))) return rc;
        if ((rc = run_pw(L(), packed, buf[1], bs(STEM_C, s.h_stem1, s.w_stem1), stem, bs(STEM_C, s.h[1], s.w[1]), nullptr, N, s.h_stem1,
                         s.w_stem1, st))) return rc;
    }
    const float* x = stem;
    int cin = STEM_C;
    int cur = 0;  // buf[cur]: the running activation once a stage has started; buf[2], buf[3]: hidden / qkv / attention
    for (int i = 0; i < 4; ++i) {
        const int c = desc->channels[i], hi = s.h[i + 1], wi = s.w[i + 1], ho = s.h[i + 2], wo = s.w[i + 2];
        const int64_t P = bs(1, ho, wo);
        if ((rc = run_dw(L(), packed, x, buf[2], N, hi, wi, st))) return rc;
        if ((rc = run_pw(L(), packed, buf[2], cin * bs(1, ho, wo), buf[cur], c * P, nullptr, N, ho, wo, st))) return rc;
        for (int b = 0; b < desc->num_blocks[i]; ++b) {
            if (desc->mixer[i] == 0) {
                if ((rc = run_dw(L(), packed, buf[cur], buf[cur ^ 1], N, ho, wo, st))) return rc;
                cur ^= 1;
            } else {
                if ((rc = run_pw(L(), packed, buf[cur], c * P, buf[2], (1 + 2 * c) * P, nullptr, N, ho, wo, st))) return rc;
                NND_REQUIRE(wo <= LINATTN_MAXW, "repvit: attention row of %d > %d columns", wo, LINATTN_MAXW);
                hipLaunchKernelGGL(linattn_kernel, dim3((unsigned)ho, (unsigned)N), dim3(256), 0, st, buf[2], buf[3], c, ho, wo);
                NND_LAUNCH_CHECK();
                if ((rc = run_pw(L(), packed, buf[3], c * P, buf[cur ^ 1], c * P, buf[cur], N, ho, wo, st))) return rc;
                cur ^= 1;
            }
            if (desc->ffn_hidden[i] > 0) {
                const int hid = desc->ffn_hidden[i];
                if ((rc = run_pw(L(), packed, buf[cur], c * P, buf[2], hid * P, nullptr, N, ho, wo, st))) return rc;
                if ((rc = run_pw(L(), packed, buf[2], hid * P, buf[cur ^ 1], c * P, buf[cur], N, ho, wo, st))) return rc;
                cur ^= 1;
            }
        }
        float* keep = i == 1 ? s1 : i == 3 ? feat0 : nullptr;  // stage 1 feeds fusion 0, stage 3 is feats[0]
        if (keep) NND_HIP_CHECK(hipMemcpyAsync(keep, buf[cur], sizeof(float) * N * c * P, hipMemcpyDeviceToDevice, st));
        x = buf[cur];
        cur ^= 1;  // the next stage's patch embed writes its 1x1 result into the other buffer (x stays readable)
        cin = c;
    }
    const RvLayer& cp0 = L();
    const RvLayer& cp1 = L();
    const RvLayer& cp2 = L();
    const RvLayer& fa0 = L();
    const RvLayer& fb0 = L();
    const RvLayer& fa1 = L();
    const RvLayer& fb1 = L();
    const int c1 = desc->channels[1], c3 = desc->channels[3], f0 = desc->fusion_dim[0], f1 = desc->fusion_dim[1];
    {   // fusion 0: relu(up(A s3 + a) + B s1 + b) at stage 1's resolution
        const int h = s.h[5], w = s.w[5], Hh = s.h[3], Ww = s.w[3];
        if ((rc = run_pw(fa0, packed, feat0, bs(c3, h, w), a0, bs(f0, h, w), nullptr, N, h, w, st))) return rc;
        if ((rc = run_pw(fb0, packed, s1, bs(c1, Hh, Ww), feat1, bs(f0, Hh, Ww), nullptr, N, Hh, Ww, st))) return rc;
        dim3 grid((unsigned)cdiv(Hh * Ww, 256), (unsigned)f0, (unsigned)N);
        hipLaunchKernelGGL(upsample_add_relu_kernel, grid, dim3(256), 0, st, a0, feat1, f0, h, w, Hh, Ww);
        NND_LAUNCH_CHECK();
    }
    {   // fusion 1 at the stem's resolution
        const int h = s.h[3], w = s.w[3], Hh = s.h[1], Ww = s.w[1];
        if ((rc = run_pw(fa1, packed, feat1, bs(f0, h, w), a1, bs(f1, h, w), nullptr, N, h, w, st))) return rc;
        if ((rc = run_pw(fb1, packed, stem, bs(STEM_C, Hh, Ww), feat2, bs(f1, Hh, Ww), nullptr, N, Hh, Ww, st))) return rc;
        dim3 grid((unsigned)cdiv(Hh * Ww, 256), (unsigned)f1, (unsigned)N);
        hipLaunchKernelGGL(upsample_add_relu_kernel, grid, dim3(256), 0, st, a1, feat2, f1, h, w, Hh, Ww);
        NND_LAUNCH_CHECK();
    }
    const int cd = desc->cnet_dim;
    if ((rc = run_pw(cp0, packed, feat0, bs(c3, s.h[5], s.w[5]), cnet0, bs(cd, s.h[5], s.w[5]), nullptr, B, s.h[5], s.w[5], st))) return rc;
    if ((rc = run_pw(cp1, packed, feat1, bs(f0, s.h[3], s.w[3]), cnet1, bs(cd, s.h[3], s.w[3]), nullptr, B, s.h[3], s.w[3], st))) return rc;
    if ((rc = run_pw(cp2, packed, feat2, bs(f1, s.h[1], s.w[1]), cnet2, bs(cd, s.h[1], s.w[1]), nullptr, B, s.h[1], s.w[1], st))) return rc;
    return NND_OK;
}

}  // extern "C"
