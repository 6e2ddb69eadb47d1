// MobileNetV3-Large backbone pieces shared by the two models that run it: the encoder side of IGEVStereoMBNet (mbv3.hip,
// nnd_mbv3_forward: two frames, stages 2..5 on the left frames only) and MobileNetV3DepthModel (midas.hip, nnd_midas_forward: one
// frame tensor, taps of stages 1, 2, 4, 5).  The kernels and launchers live in mbv3.hip; this header only declares them.
#pragma once
#include "common.h"

#include <algorithm>
#include <cstdint>
#include <vector>

namespace nnd {

enum MbAct { MB_NONE = 0, MB_RELU = 1, MB_HSWISH = 2 };

// TF "same" padding before the data along one axis (timm pad_same): total max((ceil(n / s) - 1) * s + k - n, 0), half before
static inline int same_out(int n, int s) { return (n + s - 1) / s; }
static inline int same_pad_before(int n, int k, int s) { return std::max((same_out(n, s) - 1) * s + k - n, 0) / 2; }

struct MbBlock {
    int ir;  // 0: DepthwiseSeparable, 1: InvertedResidual
    int cin, mid, cout, k, stride, rd, act, skip, stage;
};
extern const MbBlock MB_BLOCKS[];
extern const int MB_NBLOCKS;
constexpr int MB_STEM_C = 16;

enum MbKind { MB_STEM = 0, MB_DW = 1, MB_PW = 2, MB_SE_R = 3, MB_SE_E = 4, MB_PROJ = 5 };

struct MbLayer {
    int kind, cin, cout, k, stride, act;
    ConvLayer cl;         // MB_PW (1x1 or 3x3, stride 1): conv_mfma layout
    int64_t off, floats;  // blob offset / size (the others: weights then bias)
};

struct MbPlan {
    std::vector<MbLayer> layers;
    int64_t total = 0;
};

int64_t mb_align(int64_t n);
// appends one layer to the plan (blob offsets 64-float aligned); MB_PW: the conv_mfma layout of a k x k stride-1 conv
void mb_add(MbPlan& p, int kind, int cin, int cout, int k, int stride, int act);
// stem | per block: [IR: expand 1x1] depthwise [SE reduce, SE expand] project 1x1 — the backbone's layers in pack order
void mb_plan_backbone(MbPlan& p);
void pack_pw(const MbLayer& l, const float* w, const float* b, float* base);

int run_dw(const MbLayer& l, const float* blob, const float* x, float* y, double* partial, int N, int Hin, int Win, hipStream_t st);
int run_se(const MbLayer& lr, const MbLayer& le, const float* blob, float* y, const double* partial, float* gate, int N, int H, int W,
           hipStream_t st);
int run_pw(const MbLayer& l, const float* blob, const float* x, int64_t xbs, float* y, int64_t ybs, const float* res, int N, int H, int W,
           hipStream_t st);

// The backbone on ONE frame tensor x (B,3,H,W), stages 0..5, with the outputs of stages 1, 2, 4, 5 written to taps[0..3]
// (B, 24 / 40 / 112 / 160, ceil(H / 4) ... ceil(H / 32)).  `layers`: the plan's backbone layers from index 0 on; workspace:
// mb_single_ws(B, H, W) floats.  The same launchers, kernels and per-layer split-K as nnd_mbv3_forward.
int64_t mb_single_ws(int B, int H, int W);
int mb_single_forward(const MbPlan& p, const float* packed, const float* x, float* const* taps, float* workspace, int B, int H, int W,
                      hipStream_t st);

}  // namespace nnd
