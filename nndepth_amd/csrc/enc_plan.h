// The layer plan, the host packer and the conv_mfma launcher shared by the three folded encoder sides: RepViT (repvit.hip),
// MobileNetV3 for IGEVStereoMBNet (mbv3.hip) and MobileNetV3DepthModel (midas.hip).  A plan is the model's layers in pack order;
// each layer owns a 64-float aligned slice of the packed blob.  Two layouts exist: "raw" (weights then bias, read by the VALU
// kernels) and conv_mfma's (a ConvLayer: fragments, bias, per-channel scale).
#pragma once
#include "common.h"
#include "conv_layer.h"

#include <cstdint>
#include <cstring>
#include <vector>

namespace nnd {
inline namespace encside {  // encoder.hip has an unrelated nnd::EncPlan of its own: keep the two types apart for the linker

enum EncKind { ENC_STEM = 0, ENC_DW = 1, ENC_MFMA = 2 };  // a model's own raw kinds follow from 3 on

struct EncLayer {
    int kind, cin, cout, k, stride, act;
    ConvLayer cl;         // ENC_MFMA: conv_mfma layout
    int64_t off, floats;  // blob offset / size (raw kinds: weights then bias)
};

struct EncPlan {
    std::vector<EncLayer> layers;
    int64_t total = 0;
};

inline int64_t enc_align(int64_t n) { return (n + 63) / 64 * 64; }

inline void enc_add(EncPlan& p, EncLayer l) {
    l.off = p.total;
    p.total += enc_align(l.floats);
    p.layers.push_back(l);
}

// appends a "weights then bias" layer of `floats` floats (the last `cout` of them the bias)
inline void enc_add_raw(EncPlan& p, int kind, int cin, int cout, int k, int stride, int act, int64_t floats) {
    EncLayer l{};
    l.kind = kind; l.cin = cin; l.cout = cout; l.k = k; l.stride = stride; l.act = act;
    l.floats = floats;
    enc_add(p, l);
}

// a k x k conv of stride 1 or 2 on conv_mfma, at blob offset 0 (the per-kernel entry points run one on its own)
inline EncLayer enc_mfma_layer(int cin, int cout, int k, int stride, int act) {
    EncLayer l{};
    l.kind = ENC_MFMA; l.cin = cin; l.cout = cout; l.k = k; l.stride = stride; l.act = act;
    // a stride-1 1x1 takes 32-channel K chunks (conv_ci_t would take 128 from Cin = 128 on), so that split-K 2 (enc_run_mfma) applies
    // from Cin = 64
    l.cl = make_conv_layer(k, k, cin, cout, stride, 0, (k == 1 && stride == 1) ? 32 : 0, true, &l.floats);
    return l;
}

inline void enc_add_mfma(EncPlan& p, int cin, int cout, int k, int stride, int act) { enc_add(p, enc_mfma_layer(cin, cout, k, stride, act)); }

// scale: the per-channel scale of EPI_AFFINE (nullptr: 1); the padded channels take scale 0 here, not the 1 of the folded-norm
// packers (kept as it was: the blob's bytes are pinned, tests/test_pack_pins_cpu.py and the encoder sides' own pins)
inline void enc_pack_mfma(const EncLayer& l, const float* w, const float* b, const float* scale, float* base) {
    const float* ws[1] = {w};
    const float* bs[1] = {b};
    int co[1] = {l.cout};
    pack_conv(l.cl, 1, ws, bs, co, base);
    pack_affine(l.cl, base, l.cout, [&](int c) { return Affine{scale ? scale[c] : 1.f, b[c]}; }, 0.f);
}

inline void enc_pack_raw(const EncLayer& l, const float* w, const float* b, float* base) {
    const int64_t nw = l.floats - l.cout;
    memcpy(base, w, sizeof(float) * nw);
    memcpy(base + nw, b, sizeof(float) * l.cout);
}

// Packs every layer of the plan.  t: `tpl` host tensors per layer (weight, bias [, scale: ENC_MFMA only, may be null]).  `special`
// packs the kinds only its model knows and returns false for the others.
typedef bool (*EncPackSpecial)(const EncLayer& l, const float* w, const float* b, float* base);
inline int enc_pack(const EncPlan& p, int tpl, const float* const* t, float* packed_host, const char* who, EncPackSpecial special = nullptr) {
    NND_REQUIRE(t && packed_host, "%s: null pointer", who);
    memset(packed_host, 0, sizeof(float) * p.total);
    for (size_t i = 0; i < p.layers.size(); ++i) {
        const EncLayer& l = p.layers[i];
        const float *w = t[tpl * i], *b = t[tpl * i + 1], *s = tpl > 2 ? t[tpl * i + 2] : nullptr;
        NND_REQUIRE(w && b, "%s: layer %zu: weight / bias missing", who, i);
        float* base = packed_host + l.off;
        if (l.kind == ENC_MFMA) {
            enc_pack_mfma(l, w, b, s, base);
            continue;
        }
        NND_REQUIRE(!s, "%s: layer %zu (depthwise / stem) takes no scale", who, i);
        if (!(special && special(l, w, b, base))) enc_pack_raw(l, w, b, base);
    }
    return NND_OK;
}

// One ENC_MFMA layer on conv_mfma, NCHW in / out.  aux: the residual / addend of EPI_AFFINE (the shape of y) or nullptr; io_flags:
// ConvIO::flags.  Input Hin x Win, output Ho x Wo (they differ at stride 2).
inline int enc_run_mfma(const EncLayer& l, const float* blob, const float* x, int64_t xbs, float* y, int64_t ybs, const float* aux, int epi,
                        int io_flags, int N, int Hin, int Win, int Ho, int Wo, hipStream_t st) {
    ConvIO io{};
    io.src0 = Act{const_cast<float*>(x), xbs, l.cin};
    io.out0 = Act{y, ybs, l.cout};
    if (aux) io.aux0 = Act{const_cast<float*>(aux), ybs, l.cout};
    io.Hin = Hin; io.Win = Win;
    io.flags = io_flags;
    // split-K fixed per layer (2 where the layer has 2+ chunks): the two half-K partial tiles are summed in wave order, which halves
    // the MFMA accumulation chain (a 128- / 384-deep chain was up to 2.7x PyTorch's own fp32 error), and a fixed ks keeps every
    // output's K order independent of the batch: a pair's maps do not depend on the batch it runs in
    io.force_ks = l.cl.nchunks >= 2 ? 2 : 1;
    return launch_conv(l.cl, blob + l.off, io, epi, N, Ho, Wo, st);
}

}  // namespace encside
}  // namespace nnd
