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
// Every conv_mfma launch fixes its split-K factor per layer (enc_plan.h: enc_run_mfma; 2 from two 32-channel K chunks on, else 1): each output
// has the same K order whatever the batch, so a pair's maps do not depend on the batch it runs in, and the two half-K chains keep the
// fp32 accumulation error at PyTorch's level.  The depthwise kernels accumulate in float64 and round once.  Activations are NCHW in the caller's workspace.
// The layer plan, the packer and the conv_mfma launcher are enc_plan.h's, shared with mbv3.hip and midas.hip; the depthwise tap loop
// and the stem's patch gather are enc_valu.h's, shared with mbv3.hip.
#include "enc_plan.h"
#include "enc_valu.h"
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
    const double acc = dw_taps<K>(xp, wp, iy0, ix0, Hin, Win);
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
    stem_gather(xp, oy, ox, stride, 1, 1, Hin, Win, in);
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
enum RvAct { RV_NONE = 0, RV_GELU = 1, RV_RESID = 2 };  // RV_RESID: y = x_in + scale * (acc + bias) (EPI_AFFINE, residual)

static void rv_add_raw(EncPlan& p, int kind, int cin, int cout, int k, int stride, int act) {
    enc_add_raw(p, kind, cin, cout, k, stride, act, (int64_t)cout * (kind == ENC_STEM ? cin : 1) * k * k + cout);
}

static int rv_check(const nnd_repvit_desc* d) {
    if (int rc = check_desc(d, 0, "repvit")) return rc;
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

static int rv_plan(const nnd_repvit_desc* d, EncPlan* p) {
    if (int rc = rv_check(d)) return rc;
    rv_add_raw(*p, ENC_STEM, 3, STEM_C, 3, d->stem_strides[0], RV_GELU);
    rv_add_raw(*p, ENC_DW, STEM_C, STEM_C, 3, d->stem_strides[1], RV_GELU);
    enc_add_mfma(*p, STEM_C, STEM_C, 1, d->stem_strides[2], RV_GELU);
    int cin = STEM_C;
    for (int i = 0; i < 4; ++i) {
        const int c = d->channels[i];
        rv_add_raw(*p, ENC_DW, cin, cin, d->patch_size, d->down_strides[i], RV_NONE);
        enc_add_mfma(*p, cin, c, 1, 1, RV_GELU);
        for (int b = 0; b < d->num_blocks[i]; ++b) {
            if (d->mixer[i] == 0) {
                rv_add_raw(*p, ENC_DW, c, c, 3, 1, RV_NONE);
            } else {
                enc_add_mfma(*p, c, 1 + 2 * c, 1, 1, RV_NONE);  // qkv_proj (norm folded)
                enc_add_mfma(*p, c, c, 1, 1, RV_RESID);         // out_proj, x + ls1 * (.)
            }
            if (d->ffn_hidden[i] > 0) {
                enc_add_mfma(*p, c, d->ffn_hidden[i], 1, 1, RV_GELU);   // fc1
                enc_add_mfma(*p, d->ffn_hidden[i], c, 1, 1, RV_RESID);  // fc2, x + ls * (.)
            }
        }
        cin = c;
    }
    const int f0 = d->fusion_dim[0], f1 = d->fusion_dim[1];
    enc_add_mfma(*p, d->channels[3], d->cnet_dim, 1, 1, RV_GELU);  // cnet_proj[0..2]
    enc_add_mfma(*p, f0, d->cnet_dim, 1, 1, RV_GELU);
    enc_add_mfma(*p, f0, d->cnet_dim, 1, 1, RV_GELU);
    enc_add_mfma(*p, d->channels[3], f0, 1, 1, RV_NONE);  // fusion 0: coarse (stage 3) / fine (stage 1) halves
    enc_add_mfma(*p, d->channels[1], f0, 1, 1, RV_NONE);
    enc_add_mfma(*p, f0, f1, 1, 1, RV_NONE);              // fusion 1: coarse (fused 1) / fine (stem)
    enc_add_mfma(*p, STEM_C, f1, 1, 1, RV_NONE);
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

// ------------------------------------------------------------------------------------------ launchers
static int run_dw(const float* x, const float* w, const float* bias, float* y, int N, int C, int Hin, int Win, int k, int stride, int gelu,
                  hipStream_t st) {
    const int Ho = conv_out(Hin, stride), Wo = conv_out(Win, stride);
    dim3 grid((unsigned)cdiv(Ho * Wo, 256), (unsigned)C, (unsigned)N);
    if (k == 3) hipLaunchKernelGGL(dwconv_kernel<3>, grid, dim3(256), 0, st, x, y, w, bias, C, Hin, Win, Ho, Wo, stride, gelu);
    else if (k == 5) hipLaunchKernelGGL(dwconv_kernel<5>, grid, dim3(256), 0, st, x, y, w, bias, C, Hin, Win, Ho, Wo, stride, gelu);
    else hipLaunchKernelGGL(dwconv_kernel<7>, grid, dim3(256), 0, st, x, y, w, bias, C, Hin, Win, Ho, Wo, stride, gelu);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

static int run_stem(const float* x, const float* x1, int nsplit, const float* w, const float* bias, float* y, int N, int H, int W,
                    int stride, hipStream_t st) {
    const int Ho = conv_out(H, stride), Wo = conv_out(W, stride);
    hipLaunchKernelGGL(stem_conv_kernel, dim3((unsigned)cdiv(Ho * Wo, 256), 1, (unsigned)N), dim3(256), 0, st, x, x1, nsplit, y, w, bias, H,
                       W, Ho, Wo, stride);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

static int run_linattn(const float* qkv, float* out, int N, int C, int H, int W, hipStream_t st) {
    hipLaunchKernelGGL(linattn_kernel, dim3((unsigned)H, (unsigned)N), dim3(256), 0, st, qkv, out, C, H, W);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

static int run_upsample_add_relu(const float* a, float* y, int N, int C, int h, int w, int H, int W, hipStream_t st) {
    dim3 grid((unsigned)cdiv(H * W, 256), (unsigned)C, (unsigned)N);
    hipLaunchKernelGGL(upsample_add_relu_kernel, grid, dim3(256), 0, st, a, y, C, h, w, H, W);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

// 1x1 conv on conv_mfma (NCHW in / out, dense); res: the residual of RV_RESID (same shape as y)
static int run_pw(const EncLayer& l, const float* blob, const float* x, float* y, const float* res, int N, int Hin, int Win, hipStream_t st) {
    const int Ho = conv_out(Hin, l.stride), Wo = conv_out(Win, l.stride);
    return enc_run_mfma(l, blob, x, (int64_t)l.cin * Hin * Win, y, (int64_t)l.cout * Ho * Wo, res, l.act == RV_GELU ? EPI_GELU : EPI_AFFINE, 0,
                        N, Hin, Win, Ho, Wo, st);
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
    return run_dw(x, w, bias, y, N, C, H, W, k, stride, gelu ? 1 : 0, (hipStream_t)stream);
}

int nnd_repvit_stem(const float* x, const float* x1, int nsplit, const float* w, const float* bias, float* y, int N, int H, int W, int stride,
                    void* stream) {
    NND_REQUIRE(x && w && bias && y, "repvit_stem: null pointer");
    NND_REQUIRE(stride == 1 || stride == 2, "repvit_stem: stride %d not built (1, 2)", stride);
    NND_REQUIRE(N >= 1 && H >= 1 && W >= 1 && N <= 65535, "repvit_stem: bad size %dx%dx%d", N, H, W);
    if (!x1) nsplit = N;
    NND_REQUIRE(nsplit >= 1 && nsplit <= N, "repvit_stem: nsplit %d of %d", nsplit, N);
    return run_stem(x, x1 ? x1 : x, nsplit, w, bias, y, N, H, W, stride, (hipStream_t)stream);
}

int64_t nnd_repvit_pointwise_packed_floats(int Cout, int Cin, int stride) {
    NND_REQUIRE(Cout >= 1 && Cin >= 1, "repvit_pointwise: channels %d -> %d", Cin, Cout);
    NND_REQUIRE(stride == 1 || stride == 2, "repvit: stride %d", stride);
    return enc_align(enc_mfma_layer(Cin, Cout, 1, stride, RV_NONE).floats);
}

int nnd_repvit_pointwise_pack(int Cout, int Cin, int stride, const float* w, const float* bias, const float* scale, float* packed_host) {
    NND_REQUIRE(Cout >= 1 && Cin >= 1 && w && bias && packed_host, "repvit_pointwise_pack: bad argument");
    NND_REQUIRE(stride == 1 || stride == 2, "repvit: stride %d", stride);
    const EncLayer l = enc_mfma_layer(Cin, Cout, 1, stride, RV_NONE);
    memset(packed_host, 0, sizeof(float) * enc_align(l.floats));
    enc_pack_mfma(l, w, bias, scale, packed_host);
    return NND_OK;
}

int nnd_repvit_pointwise(int Cout, int Cin, int stride, const float* packed_dev, const float* x, const float* residual, float* y, int N,
                         int H, int W, int gelu, void* stream) {
    NND_REQUIRE(packed_dev && x && y && N >= 1 && H >= 1 && W >= 1, "repvit_pointwise: bad argument");
    NND_REQUIRE(!(gelu && residual), "repvit_pointwise: GELU and a residual are not built together");
    NND_REQUIRE(stride == 1 || stride == 2, "repvit: stride %d", stride);
    const EncLayer l = enc_mfma_layer(Cin, Cout, 1, stride, gelu ? RV_GELU : (residual ? RV_RESID : RV_NONE));
    return run_pw(l, packed_dev, x, y, residual, N, H, W, (hipStream_t)stream);
}

int nnd_repvit_linear_attention(const float* qkv, float* out, int N, int C, int H, int W, void* stream) {
    NND_REQUIRE(qkv && out && N >= 1 && C >= 1 && H >= 1 && W >= 1 && N <= 65535, "repvit_linear_attention: bad argument");
    NND_REQUIRE(W <= LINATTN_MAXW, "repvit_linear_attention: row of %d > %d columns", W, LINATTN_MAXW);
    return run_linattn(qkv, out, N, C, H, W, (hipStream_t)stream);
}

int nnd_repvit_upsample_add_relu(const float* a, float* y, int N, int C, int h, int w, int H, int W, void* stream) {
    NND_REQUIRE(a && y && N >= 1 && C >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1 && C <= 65535 && N <= 65535,
                "repvit_upsample_add_relu: bad argument");
    return run_upsample_add_relu(a, y, N, C, h, w, H, W, (hipStream_t)stream);
}

int nnd_repvit_num_tensors(const nnd_repvit_desc* desc) {
    EncPlan p;
    if (int rc = rv_plan(desc, &p)) return rc;
    return 3 * (int)p.layers.size();
}

int64_t nnd_repvit_packed_floats(const nnd_repvit_desc* desc) {
    EncPlan p;
    if (int rc = rv_plan(desc, &p)) return rc;
    return p.total;
}

int64_t nnd_repvit_workspace_floats(const nnd_repvit_desc* desc, int N, int H, int W) {
    if (int rc = rv_check(desc)) return rc;
    NND_REQUIRE(N >= 1 && H >= 1 && W >= 1, "repvit: bad size %dx%dx%d", N, H, W);
    const RvWs r = rv_ws(desc, N, H, W);
    return 4 * enc_align(r.m) + enc_align(r.stem) + enc_align(r.s1) + enc_align(r.a0) + enc_align(r.a1);
}

int nnd_repvit_pack(const nnd_repvit_desc* desc, const float* const* t, float* packed_host) {
    EncPlan p;
    if (int rc = rv_plan(desc, &p)) return rc;
    return enc_pack(p, 3, t, packed_host, "repvit_pack");
}

int nnd_repvit_forward(const nnd_repvit_desc* desc, const float* packed, const float* frames, const float* frames_b, int nsplit,
                       float* feat0, float* feat1, float* feat2, float* cnet0, float* cnet1, float* cnet2, float* workspace, int N, int H,
                       int W, void* stream) {
    EncPlan p;
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
    for (int i = 0; i < 4; ++i, q += enc_align(r.m)) buf[i] = q;
    float* stem = q; q += enc_align(r.stem);
    float* s1 = q; q += enc_align(r.s1);
    float* a0 = q; q += enc_align(r.a0);
    float* a1 = q;
    size_t li = 0;
    auto L = [&]() -> const EncLayer& { return p.layers[li++]; };
    auto dw = [&](const EncLayer& l, const float* x, float* y, int h, int w) {  // the next depthwise layer on all N samples
        const float* wt = packed + l.off;
        return run_dw(x, wt, wt + l.floats - l.cout, y, N, l.cout, h, w, l.k, l.stride, l.act == RV_GELU, st);
    };
    auto pw = [&](const EncLayer& l, const float* x, float* y, const float* res, int n, int h, int w) {
        return run_pw(l, packed, x, y, res, n, h, w, st);
    };
    int rc;
    {   // stem
        const EncLayer& l0 = L();
        const float* wt = packed + l0.off;
        if ((rc = run_stem(frames, frames_b ? frames_b : frames, nsplit, wt, wt + l0.floats - l0.cout, buf[0], N, H, W, l0.stride, st)))
            return rc;
        if ((rc = dw(L(), buf[0], buf[1], s.h_stem0, s.w_stem0))) return rc;
        if ((rc = pw(L(), buf[1], stem, nullptr, N, s.h_stem1, s.w_stem1))) return rc;
    }
    const float* x = stem;
    int cur = 0;  // buf[cur]: the running activation once a stage has started; buf[2], buf[3]: hidden / qkv / attention
    for (int i = 0; i < 4; ++i) {
        const int c = desc->channels[i], hi = s.h[i + 1], wi = s.w[i + 1], ho = s.h[i + 2], wo = s.w[i + 2];
        if ((rc = dw(L(), x, buf[2], hi, wi))) return rc;
        if ((rc = pw(L(), buf[2], buf[cur], nullptr, N, ho, wo))) return rc;
        for (int b = 0; b < desc->num_blocks[i]; ++b) {
            if (desc->mixer[i] == 0) {
                if ((rc = dw(L(), buf[cur], buf[cur ^ 1], ho, wo))) return rc;
                cur ^= 1;
            } else {
                if ((rc = pw(L(), buf[cur], buf[2], nullptr, N, ho, wo))) return rc;
                NND_REQUIRE(wo <= LINATTN_MAXW, "repvit: attention row of %d > %d columns", wo, LINATTN_MAXW);
                if ((rc = run_linattn(buf[2], buf[3], N, c, ho, wo, st))) return rc;
                if ((rc = pw(L(), buf[3], buf[cur ^ 1], buf[cur], N, ho, wo))) return rc;
                cur ^= 1;
            }
            if (desc->ffn_hidden[i] > 0) {
                if ((rc = pw(L(), buf[cur], buf[2], nullptr, N, ho, wo))) return rc;
                if ((rc = pw(L(), buf[2], buf[cur ^ 1], buf[cur], N, ho, wo))) return rc;
                cur ^= 1;
            }
        }
        float* keep = i == 1 ? s1 : i == 3 ? feat0 : nullptr;  // stage 1 feeds fusion 0, stage 3 is feats[0]
        if (keep) NND_HIP_CHECK(hipMemcpyAsync(keep, buf[cur], sizeof(float) * N * c * ho * wo, hipMemcpyDeviceToDevice, st));
        x = buf[cur];
        cur ^= 1;  // the next stage's patch embed writes its 1x1 result into the other buffer (x stays readable)
    }
    const EncLayer& cp0 = L();
    const EncLayer& cp1 = L();
    const EncLayer& cp2 = L();
    const EncLayer& fa0 = L();
    const EncLayer& fb0 = L();
    const EncLayer& fa1 = L();
    const EncLayer& fb1 = L();
    {   // fusion 0: relu(up(A s3 + a) + B s1 + b) at stage 1's resolution
        const int h = s.h[5], w = s.w[5], Hh = s.h[3], Ww = s.w[3];
        if ((rc = pw(fa0, feat0, a0, nullptr, N, h, w))) return rc;
        if ((rc = pw(fb0, s1, feat1, nullptr, N, Hh, Ww))) return rc;
        if ((rc = run_upsample_add_relu(a0, feat1, N, desc->fusion_dim[0], h, w, Hh, Ww, st))) return rc;
    }
    {   // fusion 1 at the stem's resolution
        const int h = s.h[3], w = s.w[3], Hh = s.h[1], Ww = s.w[1];
        if ((rc = pw(fa1, feat1, a1, nullptr, N, h, w))) return rc;
        if ((rc = pw(fb1, stem, feat2, nullptr, N, Hh, Ww))) return rc;
        if ((rc = run_upsample_add_relu(a1, feat2, N, desc->fusion_dim[1], h, w, Hh, Ww, st))) return rc;
    }
    if ((rc = pw(cp0, feat0, cnet0, nullptr, B, s.h[5], s.w[5]))) return rc;
    if ((rc = pw(cp1, feat1, cnet1, nullptr, B, s.h[3], s.w[3]))) return rc;
    return pw(cp2, feat2, cnet2, nullptr, B, s.h[1], s.w[1]);
}

}  // extern "C"
