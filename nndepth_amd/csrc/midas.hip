// MobileNetV3DepthModel (the reference's MiDaS-style monocular model, nndepth/models/midas/models/mobilenet_v3.py) in ONE C-ABI
// call (nnd_midas_forward): the MobileNetV3-Large backbone on one frame tensor (mbv3.hip's walk mb_walk, declared in mbv3.h, with
// the taps of stages 1, 2, 4, 5 kept; layer plan, packer and conv_mfma launcher from enc_plan.h),
// BaseDecoder (nndepth/decoders/base_decoder.py) with its four UpsamplerBlocks (nndepth/blocks/upsampler_block.py) and the
// last_conv head.  Exact fp32 throughout: no split arithmetic, no calibration; every BatchNorm is folded on the host
// (ops.MidasEngine, float64, cast once to fp32).
//
//   skip_layers[i]        3x3 (24 / 40 / 112 / 160 -> C) + ReLU                        conv_mfma, EPI_RELU
//   UpsamplerBlock i      m = feat + relu(bn1(conv1(skip)))   (i < 3; block 3 has none)  conv_mfma, EPI_AFFINE: ReLU, then + feat
//                         a = relu(bn2(conv2(m)))                                       conv_mfma, EPI_RELU
//                         o = relu(out_conv(up2x(a)))                                   midas_up_conv_kernel<1, P, false>
//   last_conv.0           t = conv3x3(o0) + bias   (no activation)                      conv_mfma, EPI_AFFINE
//   last_conv.1 .. 5      depth = relu(conv1x1_{C->1}(relu(conv3x3(up2x(t)))))          midas_up_conv_kernel<3, P, true>
//
// midas_up_conv_kernel is the one new kernel: a k x k (1 or 3) conv over the x2 bilinear upsample (align_corners=False) of its
// input, on the fp32 MFMA.  The upsample is evaluated while the input tile is staged into LDS, so the upsampled C-channel map
// never exists in memory; as the head (HEAD = true) its epilogue also applies ReLU, the C -> 1 conv and the final ReLU from the
// accumulators, so the 3x3's full-resolution C-channel output never exists either: per image the head reads t (C, H/2, W/2)
// and writes one channel.
#include "mbv3.h"
#include "bilinear.h"

#include <cstring>

namespace nnd {

typedef float md_f32x16 __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------------------------------ k x k conv over up2x(x)
// Output tile: MD_TH x MD_TW pixels = 8 MFMA column blocks of 4 rows x 8 cols (lane l & 31 -> (r, c) = (l31 / 8, l31 % 8)); a wave
// owns one 32-channel output block (cbi) and P of the 8 column blocks; workgroup = ncb x (8 / P) waves.
// K loop: chunks of MD_CI input channels.  Per chunk the upsampled, zero-padded patch (MD_TH + k - 1) x (MD_TW + k - 1) of those
// channels is staged into one of two LDS buffers (each element: 4 loads of x and the 2 x 2 weights of torch's formula, which
// depend only on the output coordinate's parity and the border clamp); chunk K + 1 is staged before chunk K is multiplied, one
// barrier per chunk.  A = weights, streamed from global memory in fragment order (md_pack_conv); B = one LDS word per MFMA with
// an immediate offset per (channel pair, tap, column block).  The row stride MD_S = 40 puts the 32 lanes (r, c) on 32 banks.
// Rounding: each chunk (MD_CI * k * k terms) is one fp32 MFMA chain from zero; the chunk sums, the bias and — in the head — the
// C -> 1 reduction are accumulated in float64 and rounded once per value the reference rounds (the 3x3's output, the depth).
constexpr int MD_CI = 16, MD_TH = 8, MD_TW = 32, MD_S = 40, MD_MAXC = 128;

struct MdArgs {
    const float* x;    // (N, Cin, h, w)
    const float* wpk;  // md_pack_conv: fragments, then bias (ncb * 32)
    const float* w4;   // head: (ncb * 32) weights of the C -> 1 conv, then its bias
    float* y;          // (N, Cout, 2h, 2w); head: (N, 1, 2h, 2w)
    float* pre;        // head, optional: the map before the final ReLU
    int Cin, Cout, h, w, ncb;
};

template <int K, int P, bool HEAD>
__global__ void __launch_bounds__(512) midas_up_conv_kernel(MdArgs a) {
    constexpr int NT = K * K, PR = MD_TH + K - 1, PC = MD_TW + K - 1, NPOS = PR * PC, PATCH = PR * MD_S;
    __shared__ __attribute__((aligned(16))) float lds[2 * MD_CI * PATCH];
    const int tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ncb = a.ncb;
    const int cbi = wave % ncb, pg = wave / ncb;
    const int h2 = lane >> 5, l31 = lane & 31, r = l31 >> 3, c = l31 & 7;
    const int h = a.h, w = a.w, H = 2 * h, W = 2 * w;
    const int tx0 = blockIdx.x * MD_TW, ty0 = blockIdx.y * MD_TH, n = blockIdx.z;
    const int nchunks = a.Cin / MD_CI;
    const float* xn = a.x + (long)n * a.Cin * h * w;

    auto stage = [&](int ch) {
        float* buf = lds + (ch & 1) * (MD_CI * PATCH);
        const float* xc = xn + (long)ch * MD_CI * h * w;
        for (int e = tid; e < MD_CI * NPOS; e += nthr) {
            const int ci = e / NPOS, pos = e - ci * NPOS;
            const int py = pos / PC, px = pos - py * PC;
            const int gy = ty0 + py - K / 2, gx = tx0 + px - K / 2;
            float v = 0.f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                int y0, y1, x0, x1;
                float ly0, ly1, lx0, lx1;
                src_index(0.5f, gy, h, y0, y1, ly0, ly1);
                src_index(0.5f, gx, w, x0, x1, lx0, lx1);
                const float* p = xc + (long)ci * h * w;
                const float v00 = p[y0 * w + x0], v01 = p[y0 * w + x1], v10 = p[y1 * w + x0], v11 = p[y1 * w + x1];
                v = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);  // torch's upsample_bilinear2d
            }
            buf[ci * PATCH + py * MD_S + px] = v;
        }
    };

    int sto[P];  // LDS offset of this wave's column blocks
#pragma unroll
    for (int pp = 0; pp < P; ++pp) {
        const int st = pg * P + pp;
        sto[pp] = (st >> 2) * 4 * MD_S + (st & 3) * 8;
    }
    double sum[P][16];
#pragma unroll
    for (int pp = 0; pp < P; ++pp)
#pragma unroll
        for (int i = 0; i < 16; ++i) sum[pp][i] = 0.0;

    const float4* wbase = reinterpret_cast<const float4*>(a.wpk) + (size_t)cbi * nchunks * (NT * 2 * 64) + lane;
    stage(0);
    __syncthreads();
    for (int ch = 0; ch < nchunks; ++ch) {
        if (ch + 1 < nchunks) stage(ch + 1);
        const float* xb = lds + (ch & 1) * (MD_CI * PATCH) + h2 * PATCH + r * MD_S + c;
        const float4* wc = wbase + (size_t)ch * (NT * 2 * 64);
        md_f32x16 acc[P];
#pragma unroll
        for (int pp = 0; pp < P; ++pp)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[pp][i] = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int dy = t / K, dx = t % K;
            const float4 a0 = wc[t * 128], a1 = wc[t * 128 + 64];
#pragma unroll
            for (int pair = 0; pair < 8; ++pair) {
                const float4 av = pair < 4 ? a0 : a1;
                const float a_s = (pair % 4 == 0) ? av.x : (pair % 4 == 1) ? av.y : (pair % 4 == 2) ? av.z : av.w;
#pragma unroll
                for (int pp = 0; pp < P; ++pp) {
                    const float b_s = xb[pair * 2 * PATCH + dy * MD_S + dx + sto[pp]];
                    acc[pp] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_s, b_s, acc[pp], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int pp = 0; pp < P; ++pp)
#pragma unroll
            for (int i = 0; i < 16; ++i) sum[pp][i] += (double)acc[pp][i];
        __syncthreads();
    }

    // accumulator layout: lane = pixel (l31) of the column block, register reg = output channel cb*32 + (reg & 3) + 8*(reg >> 2) + 4*h2
    const float* bias = a.wpk + (size_t)ncb * nchunks * NT * 2 * 64 * 4;
    if constexpr (!HEAD) {
#pragma unroll
        for (int pp = 0; pp < P; ++pp) {
            const int st = pg * P + pp;
            const int y = ty0 + (st >> 2) * 4 + r, x = tx0 + (st & 3) * 8 + c;
            if (y >= H || x >= W) continue;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int co = cbi * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h2;
                if (co >= a.Cout) continue;
                const float v = (float)(sum[pp][reg] + (double)bias[co]);
                a.y[(((long)n * a.Cout + co) * H + y) * W + x] = fmaxf(v, 0.f);
            }
        }
    } else {
        double* red = reinterpret_cast<double*>(lds);  // [ncb][256]; the patch buffers are free after the last barrier
#pragma unroll
        for (int pp = 0; pp < P; ++pp) {
            double s = 0.0;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int co = cbi * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h2;  // < ncb * 32: bias / w4 are padded with zeros
                const float v = fmaxf((float)(sum[pp][reg] + (double)bias[co]), 0.f);
                s = fma((double)a.w4[co], (double)v, s);
            }
            s += __shfl_xor(s, 32);
            if (h2 == 0) red[cbi * 256 + (pg * P + pp) * 32 + l31] = s;
        }
        __syncthreads();
        if (tid < 256) {
            const int st = tid >> 5, l = tid & 31;
            const int y = ty0 + (st >> 2) * 4 + (l >> 3), x = tx0 + (st & 3) * 8 + (l & 7);
            double s = (double)a.w4[ncb * 32];
            for (int k = 0; k < ncb; ++k) s += red[k * 256 + tid];
            if (y < H && x < W) {
                const float v = (float)s;
                const long o = ((long)n * H + y) * W + x;
                if (a.pre) a.pre[o] = v;
                a.y[o] = fmaxf(v, 0.f);
            }
        }
    }
}

static inline int md_ncb(int Cout) { return cdiv(Cout, 32); }
static inline int64_t md_conv_wfloats(int Cout, int Cin, int k) { return (int64_t)md_ncb(Cout) * (Cin / MD_CI) * k * k * 2 * 64 * 4; }
static inline int64_t md_conv_floats(int Cout, int Cin, int k) { return md_conv_wfloats(Cout, Cin, k) + md_ncb(Cout) * 32; }
static inline int64_t md_head1_floats(int C) { return md_ncb(C) * 32 + 1; }

static int md_check_c(const char* what, int C) {
    NND_REQUIRE(C >= 16 && C <= MD_MAXC && C % 16 == 0, "%s: %d channels not built (multiples of 16 up to %d)", what, C, MD_MAXC);
    return NND_OK;
}

// w (Cout, Cin, k, k), b (Cout) -> A fragments [cb][chunk][tap][q][lane][4]: element j of fragment q of lane l is
// w[cb*32 + (l & 31)][chunk*16 + (q*4 + j)*2 + (l >> 5)][tap]; then the bias, both zero-padded to 32-channel blocks
static void md_pack_conv(int Cout, int Cin, int k, const float* w, const float* b, float* out) {
    const int ncb = md_ncb(Cout), nch = Cin / MD_CI, NT = k * k;
    float* p = out;
    for (int cb = 0; cb < ncb; ++cb)
        for (int ch = 0; ch < nch; ++ch)
            for (int t = 0; t < NT; ++t)
                for (int q = 0; q < 2; ++q)
                    for (int l = 0; l < 64; ++l)
                        for (int j = 0; j < 4; ++j) {
                            const int co = cb * 32 + (l & 31), ci = ch * MD_CI + (q * 4 + j) * 2 + (l >> 5);
                            *p++ = co < Cout ? w[((int64_t)co * Cin + ci) * NT + t] : 0.f;
                        }
    for (int co = 0; co < ncb * 32; ++co) *p++ = co < Cout ? b[co] : 0.f;
}

static void md_pack_head1(int C, const float* w4, const float* b4, float* out) {
    const int n = md_ncb(C) * 32;
    for (int co = 0; co < n; ++co) out[co] = co < C ? w4[co] : 0.f;
    out[n] = b4[0];
}

template <int K, bool HEAD>
static int md_launch(const MdArgs& a, int N, hipStream_t st) {
    const int P = a.ncb <= 2 ? 2 : 4;
    dim3 grid((unsigned)cdiv(2 * a.w, MD_TW), (unsigned)cdiv(2 * a.h, MD_TH), (unsigned)N), block((unsigned)(64 * a.ncb * (8 / P)));
    if (P == 2)
        hipLaunchKernelGGL((midas_up_conv_kernel<K, 2, HEAD>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((midas_up_conv_kernel<K, 4, HEAD>), grid, block, 0, st, a);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

static int md_check_size(const char* what, int N, int h, int w) {
    NND_REQUIRE(N >= 1 && N <= 65535 && h >= 1 && w >= 1 && h <= 16384 && w <= 16384 && cdiv(2 * h, MD_TH) <= 65535,
                "%s: bad size N %d, input %dx%d", what, N, h, w);
    return NND_OK;
}

// relu(out_conv(up2x(x))): x (N, Cin, h, w) -> y (N, Cout, 2h, 2w)
static int run_up_pw(int Cout, int Cin, const float* packed, const float* x, float* y, int N, int h, int w, hipStream_t st) {
    MdArgs a{};
    a.x = x; a.wpk = packed; a.y = y; a.Cin = Cin; a.Cout = Cout; a.h = h; a.w = w; a.ncb = md_ncb(Cout);
    return md_launch<1, false>(a, N, st);
}

static int run_head(int C, const float* packed3, const float* packed1, const float* t, float* depth, float* pre, int N, int h, int w,
                    hipStream_t st) {
    MdArgs a{};
    a.x = t; a.wpk = packed3; a.w4 = packed1; a.y = depth; a.pre = pre; a.Cin = C; a.Cout = C; a.h = h; a.w = w; a.ncb = md_ncb(C);
    return md_launch<3, true>(a, N, st);
}

// k x k conv on conv_mfma (mbv3.hip's pointwise layer): y = act(conv + bias), or with `add`: y = add + relu(conv + bias)
static int run_conv(const EncLayer& l, const float* blob, const float* x, float* y, const float* add, int N, int H, int W, hipStream_t st) {
    if (!add) return mb_run_pw(l, blob, x, y, nullptr, N, H, W, st);
    // flags 1: ReLU BEFORE the addition (UpsamplerBlock: feat + relu(bn1(conv1(skip))))
    return enc_run_mfma(l, blob, x, (int64_t)l.cin * H * W, y, (int64_t)l.cout * H * W, add, EPI_AFFINE, 1, N, H, W, H, W, st);
}

// ------------------------------------------------------------------------------------------ plan
enum MdKind { MD_UP = 16, MD_HEAD3 = 17, MD_HEAD1 = 18 };
constexpr int MD_TAP_C[4] = {24, 40, 112, 160};

static int md_check(const nnd_midas_desc* d) {
    if (int rc = check_desc(d, NND_MIDAS_KEEP_PRE, "midas")) return rc;
    return md_check_c("midas: feature_channels", d->feature_channels);
}

// layer order (= the tensor order of nnd_midas_pack): the backbone (mb_plan_backbone) | skip_layers.0..3 | per UpsamplerBlock 0..3:
// [conv1 + bn1 (blocks 0..2)] conv2 + bn2, out_conv | last_conv.0, last_conv.2, last_conv.4
struct MdPlan {
    EncPlan p;
    size_t skip0, up0, last0;  // layer indices
};

static int md_plan(const nnd_midas_desc* d, MdPlan* m) {
    if (int rc = md_check(d)) return rc;
    const int C = d->feature_channels;
    EncPlan& p = m->p;
    mb_plan_backbone(p);
    m->skip0 = p.layers.size();
    for (int i = 0; i < 4; ++i) enc_add_mfma(p, MD_TAP_C[i], C, 3, 1, MB_RELU);
    m->up0 = p.layers.size();
    for (int i = 0; i < 4; ++i) {
        if (i < 3) enc_add_mfma(p, C, C, 3, 1, MB_RELU);
        enc_add_mfma(p, C, C, 3, 1, MB_RELU);
        enc_add_raw(p, MD_UP, C, C, 1, 1, MB_RELU, md_conv_floats(C, C, 1));
    }
    m->last0 = p.layers.size();
    enc_add_mfma(p, C, C, 3, 1, MB_NONE);
    enc_add_raw(p, MD_HEAD3, C, C, 3, 1, MB_RELU, md_conv_floats(C, C, 3));
    enc_add_raw(p, MD_HEAD1, C, 1, 1, 1, MB_RELU, md_head1_floats(C));
    return NND_OK;
}

// the layers only this model has (enc_pack's special cases): the up2x convs' fragment layout and the C -> 1 head
static bool md_pack_special(const EncLayer& l, const float* w, const float* b, float* base) {
    if (l.kind == MD_UP || l.kind == MD_HEAD3) md_pack_conv(l.cout, l.cin, l.k, w, b, base);
    else if (l.kind == MD_HEAD1) md_pack_head1(l.cin, w, b, base);
    else return false;
    return true;
}

static int md_check_hw(const char* what, int B, int H, int W) {
    NND_REQUIRE(B >= 1 && B <= 32767 && H >= 32 && W >= 32 && H <= 16384 && W <= 16384, "%s: bad size %dx%dx%d", what, B, H, W);
    NND_REQUIRE(H % 32 == 0 && W % 32 == 0,
                "%s: H %d / W %d must be multiples of 32 (the decoder's x2 upsamples must meet the backbone's 1/4 .. 1/32 maps)", what, H, W);
    return NND_OK;
}

// workspace regions (floats, each 64-float aligned), in order
enum MdRegion { MDR_TAP0 = 0, MDR_SKIP0 = 4, MDR_M = 8, MDR_A = 9, MDR_O3 = 10, MDR_O2 = 11, MDR_O1 = 12, MDR_DEC = 13, MDR_T = 14, MDR_PRE = 15,
                MDR_BACKBONE = 16, MDR_COUNT = 17 };

static void md_regions(int C, int B, int H, int W, int64_t* off) {  // off[MDR_COUNT + 1]
    int64_t sz[MDR_COUNT];
    for (int i = 0; i < 4; ++i) {
        const int64_t px = (int64_t)B * (H >> (i + 2)) * (W >> (i + 2));
        sz[MDR_TAP0 + i] = px * MD_TAP_C[i];
        sz[MDR_SKIP0 + i] = px * C;
    }
    const int64_t q = (int64_t)B * C * (H / 4) * (W / 4);
    sz[MDR_M] = q; sz[MDR_A] = q;
    sz[MDR_O3] = q / 16; sz[MDR_O2] = q / 4; sz[MDR_O1] = q;
    sz[MDR_DEC] = 4 * q; sz[MDR_T] = 4 * q;
    sz[MDR_PRE] = (int64_t)B * H * W;
    sz[MDR_BACKBONE] = mb_walk_ws(B, B, H, W);
    off[0] = 0;
    for (int i = 0; i < MDR_COUNT; ++i) off[i + 1] = off[i] + enc_align(sz[i]);
}

}  // namespace nnd

using namespace nnd;

extern "C" {

// ---- the new kernels one at a time (the launchers nnd_midas_forward uses)
int64_t nnd_midas_up2x_pw_packed_floats(int Cout, int Cin) {
    if (int rc = md_check_c("midas_up2x_pw: Cout", Cout)) return rc;
    if (int rc = md_check_c("midas_up2x_pw: Cin", Cin)) return rc;
    return md_conv_floats(Cout, Cin, 1);
}

int nnd_midas_up2x_pw_pack(int Cout, int Cin, const float* w, const float* bias, float* packed_host) {
    if (int rc = md_check_c("midas_up2x_pw_pack: Cout", Cout)) return rc;
    if (int rc = md_check_c("midas_up2x_pw_pack: Cin", Cin)) return rc;
    NND_REQUIRE(w && bias && packed_host, "midas_up2x_pw_pack: null pointer");
    md_pack_conv(Cout, Cin, 1, w, bias, packed_host);
    return NND_OK;
}

int nnd_midas_up2x_pw(int Cout, int Cin, const float* packed_dev, const float* x, float* y, int N, int h, int w, void* stream) {
    if (int rc = md_check_c("midas_up2x_pw: Cout", Cout)) return rc;
    if (int rc = md_check_c("midas_up2x_pw: Cin", Cin)) return rc;
    NND_REQUIRE(packed_dev && x && y, "midas_up2x_pw: null pointer");
    if (int rc = md_check_size("midas_up2x_pw", N, h, w)) return rc;
    return run_up_pw(Cout, Cin, packed_dev, x, y, N, h, w, (hipStream_t)stream);
}

int64_t nnd_midas_head_packed_floats(int C) {
    if (int rc = md_check_c("midas_head", C)) return rc;
    return enc_align(md_conv_floats(C, C, 3)) + md_head1_floats(C);
}

int nnd_midas_head_pack(int C, const float* w2, const float* b2, const float* w4, const float* b4, float* packed_host) {
    if (int rc = md_check_c("midas_head_pack", C)) return rc;
    NND_REQUIRE(w2 && b2 && w4 && b4 && packed_host, "midas_head_pack: null pointer");
    memset(packed_host, 0, sizeof(float) * (enc_align(md_conv_floats(C, C, 3)) + md_head1_floats(C)));
    md_pack_conv(C, C, 3, w2, b2, packed_host);
    md_pack_head1(C, w4, b4, packed_host + enc_align(md_conv_floats(C, C, 3)));
    return NND_OK;
}

int nnd_midas_head(int C, const float* packed_dev, const float* t, float* depth, float* pre_relu, int N, int h, int w, void* stream) {
    if (int rc = md_check_c("midas_head", C)) return rc;
    NND_REQUIRE(packed_dev && t && depth, "midas_head: null pointer");
    if (int rc = md_check_size("midas_head", N, h, w)) return rc;
    return run_head(C, packed_dev, packed_dev + enc_align(md_conv_floats(C, C, 3)), t, depth, pre_relu, N, h, w, (hipStream_t)stream);
}

int nnd_midas_conv_add(int Cout, int Cin, int k, const float* packed_dev, const float* x, const float* feat, float* y, int N, int H, int W,
                       void* stream) {
    NND_REQUIRE(packed_dev && x && feat && y && N >= 1 && H >= 1 && W >= 1, "midas_conv_add: bad argument");
    NND_REQUIRE(Cout >= 1 && Cin >= 1 && (k == 1 || k == 3), "midas_conv_add: %dx%d %d -> %d not built", k, k, Cin, Cout);
    return run_conv(enc_mfma_layer(Cin, Cout, k, 1, MB_RELU), packed_dev, x, y, feat, N, H, W, (hipStream_t)stream);
}

// ---- the model
int nnd_midas_num_tensors(const nnd_midas_desc* desc) {
    MdPlan m;
    if (int rc = md_plan(desc, &m)) return rc;
    return 2 * (int)m.p.layers.size();
}

int64_t nnd_midas_packed_floats(const nnd_midas_desc* desc) {
    MdPlan m;
    if (int rc = md_plan(desc, &m)) return rc;
    return m.p.total;
}

int64_t nnd_midas_workspace_floats(const nnd_midas_desc* desc, int B, int H, int W) {
    if (int rc = md_check(desc)) return rc;
    if (int rc = md_check_hw("midas", B, H, W)) return rc;
    int64_t off[MDR_COUNT + 1];
    md_regions(desc->feature_channels, B, H, W, off);
    return off[MDR_COUNT];
}

int64_t nnd_midas_workspace_offset(const nnd_midas_desc* desc, int which, int B, int H, int W) {
    if (int rc = md_check(desc)) return rc;
    if (int rc = md_check_hw("midas", B, H, W)) return rc;
    NND_REQUIRE(which >= 0 && which <= 5, "midas_workspace_offset: map %d (0..3 taps, 4 decoder output, 5 map before the final ReLU)", which);
    int64_t off[MDR_COUNT + 1];
    md_regions(desc->feature_channels, B, H, W, off);
    return off[which < 4 ? MDR_TAP0 + which : which == 4 ? MDR_DEC : MDR_PRE];
}

int nnd_midas_pack(const nnd_midas_desc* desc, const float* const* t, float* packed_host) {
    MdPlan m;
    if (int rc = md_plan(desc, &m)) return rc;
    return enc_pack(m.p, 2, t, packed_host, "midas_pack", md_pack_special);
}

int nnd_midas_forward(const nnd_midas_desc* desc, const float* packed, const float* x, float* depth, float* workspace, int B, int H, int W,
                      void* stream) {
    MdPlan m;
    if (int rc = md_plan(desc, &m)) return rc;
    NND_REQUIRE(packed && x && depth && workspace, "midas_forward: null pointer");
    if (int rc = md_check_hw("midas_forward", B, H, W)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int C = desc->feature_channels;
    const EncPlan& p = m.p;
    int64_t off[MDR_COUNT + 1];
    md_regions(C, B, H, W, off);
    auto R = [&](int i) { return workspace + off[i]; };
    int rc;
    float* taps[4] = {R(MDR_TAP0), R(MDR_TAP0 + 1), R(MDR_TAP0 + 2), R(MDR_TAP0 + 3)};
    float* const keep[MB_NSTAGES] = {nullptr, taps[0], taps[1], nullptr, taps[2], taps[3]};  // one frame tensor, B samples throughout
    if ((rc = mb_walk(p, packed, x, x, B, B, B, keep, R(MDR_BACKBONE), H, W, st))) return rc;
    for (int i = 0; i < 4; ++i)
        if ((rc = run_conv(p.layers[m.skip0 + i], packed, taps[i], R(MDR_SKIP0 + i), nullptr, B, H >> (i + 2), W >> (i + 2), st))) return rc;
    // UpsamplerBlocks 3 (no skip input: its conv1 / bn1 are never run), 2, 1, 0
    const float* feat = R(MDR_SKIP0 + 3);
    float* outs[4] = {R(MDR_DEC), R(MDR_O1), R(MDR_O2), R(MDR_O3)};
    for (int i = 3; i >= 0; --i) {
        const int h = H >> (i + 2), w = W >> (i + 2);
        size_t li = m.up0 + 3 * i;
        if (i < 3) {
            if ((rc = run_conv(p.layers[li], packed, R(MDR_SKIP0 + i), R(MDR_M), feat, B, h, w, st))) return rc;
            feat = R(MDR_M);
            ++li;
        }
        if ((rc = run_conv(p.layers[li], packed, feat, R(MDR_A), nullptr, B, h, w, st))) return rc;
        if ((rc = run_up_pw(C, C, packed + p.layers[li + 1].off, R(MDR_A), outs[i], B, h, w, st))) return rc;
        feat = outs[i];
    }
    if ((rc = run_conv(p.layers[m.last0], packed, R(MDR_DEC), R(MDR_T), nullptr, B, H / 2, W / 2, st))) return rc;
    return run_head(C, packed + p.layers[m.last0 + 1].off, packed + p.layers[m.last0 + 2].off, R(MDR_T), depth,
                    (desc->flags & NND_MIDAS_KEEP_PRE) ? R(MDR_PRE) : nullptr, B, H / 2, W / 2, st);
}

}  // extern "C"
