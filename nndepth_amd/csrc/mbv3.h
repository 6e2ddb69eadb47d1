// The MobileNetV3-Large backbone shared by the two models that run it: the encoder side of IGEVStereoMBNet (mbv3.hip,
// nnd_mbv3_forward: two frames, stages 2..5 on the left frames only) and MobileNetV3DepthModel (midas.hip, nnd_midas_forward: one
// frame tensor, taps of stages 1, 2, 4, 5).  The block table, the kernels and the walk live in mbv3.hip; the layer plan is
// enc_plan.h's.
#pragma once
#include "enc_plan.h"

#include <algorithm>

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
constexpr int MB_NSTAGES = 6;  // stages 0..5 (stage 6's output is never used)

enum MbKind { MB_SE_R = 3, MB_SE_E = 4, MB_PROJ = 5 };  // after ENC_STEM, ENC_DW, ENC_MFMA

// stem | per block: [IR: expand 1x1] depthwise [SE reduce, SE expand] project 1x1 — the backbone's layers in pack order
void mb_plan_backbone(EncPlan& p);

// 1x1 / 3x3 stride-1 conv on conv_mfma (NCHW in / out, dense): y = act(conv + bias); res: the residual (same shape as y), MB_NONE
// layers only
int mb_run_pw(const EncLayer& l, const float* blob, const float* x, float* y, const float* res, int N, int H, int W, hipStream_t st);

// The backbone, stages 0..5.  Samples n < nsplit of the stem read frame1 (B,3,H,W), the others frame2; stages 0..1 run on n01
// samples, stages 2..5 on the first n25 of them.  keep[s]: where stage s's output goes ((n, C_s, ceil(H / 2^..), ..) dense), or
// nullptr for the ping-pong buffers.  `p`: a plan whose first layers are mb_plan_backbone's; workspace: mb_walk_ws(...) floats.
int64_t mb_walk_ws(int n01, int n25, int H, int W);
int mb_walk(const EncPlan& p, const float* packed, const float* frame1, const float* frame2, int nsplit, int n01, int n25,
            float* const* keep, float* workspace, int H, int W, hipStream_t st);

}  // namespace nnd
