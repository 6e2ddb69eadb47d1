// Host only: where a ConvLayer lies inside a packed parameter blob, and how a folded norm fills its bias / scale slots.  Every plan
// builder and packer goes through these two, so pack and forward cannot disagree about a layer's layout.
//   blob of one layer:  w_off: w_floats() | b_off: b_floats() [| s_off: b_floats()   (EPI_AFFINE layers: the per-channel scale)]
#pragma once
#include "common.h"

#include <cmath>

namespace nnd {

// The layer at *off, which advances past it (a caller that wants base-relative offsets starts at 0 and keeps the base itself).
// arith: the split arithmetic asked for; shapes conv_split.hip does not build fall back to the exact fp32 kernel (a caller with
// further reasons to veto it passes 0).  ci_t: input channels per K-chunk, 0 = 16 for a split arithmetic, else conv_ci_t's rule.
inline ConvLayer make_conv_layer(int KH, int KW, int Cin, int Cout, int stride, int arith, int ci_t, bool scale_slot, int64_t* off) {
    ConvLayer l;
    if (arith != 0 && !conv_split_supported(KH, KW, Cin, stride, arith, Cout)) arith = 0;
    l.KH = KH; l.KW = KW; l.Cin = Cin; l.Cout = Cout; l.stride = stride; l.arith = arith;
    l.CI_T = ci_t ? ci_t : (arith ? 16 : conv_ci_t(KH, KW, Cin, stride, Cout));
    l.nchunks = cdiv(Cin, l.CI_T);
    l.ncb = cdiv(Cout, 32);
    l.w_off = *off; *off += l.w_floats();
    l.b_off = *off; *off += l.b_floats();
    if (scale_slot) { l.s_off = *off; *off += l.b_floats(); }
    return l;
}

// y = acc * scale + shift
struct Affine {
    float scale, shift;
};

// Channel c's conv bias and eval-mode BatchNorm folded in double: scale = gamma / sqrt(var + eps), shift = (bias - mean) * scale +
// beta.  bias == nullptr: 0; gamma == nullptr: no norm (scale 1, shift = bias).
inline Affine fold_norm(int c, const float* bias, const float* gamma, const float* beta, const float* mean, const float* var, float eps) {
    const double b = bias ? (double)bias[c] : 0.0;
    if (!gamma) return {1.f, (float)b};
    const double sc = (double)gamma[c] / std::sqrt((double)var[c] + (double)eps);
    return {(float)sc, (float)((b - (double)mean[c]) * sc + (double)beta[c])};
}

// Fills the layer's b_off (shift) and s_off (scale) slots: channel c < L.Cout takes rule(c % period), the padded channels up to
// ncb * 32 take shift 0 and scale pad_scale.  (period < Cout: Conv3d's grouped layer repeats its Cout channels J times.)
template <class Rule>
inline void pack_affine(const ConvLayer& L, float* base, int period, Rule rule, float pad_scale = 1.f) {
    for (int c = 0; c < L.ncb * 32; ++c) {
        const Affine a = c < L.Cout ? rule(c % period) : Affine{pad_scale, 0.f};
        base[L.s_off + c] = a.scale;
        base[L.b_off + c] = a.shift;
    }
}

}  // namespace nnd
