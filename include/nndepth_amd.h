/*
 * nndepth_amd — C-ABI of the MI355X (gfx950) stereo-disparity hot path.
 *
 * The reference (anhtu293/nndepth) is pure Python/PyTorch and has no FFI layer; its seams
 * for this path are three duck-typed Python objects on the model instance.
 * Each entry point below replaces the ATen-op composition behind one of those seams and
 * cites the reference lines it stands in for (paths relative to the reference root).
 *
 * Conventions
 *   - all tensors are fp32, NCHW, contiguous, resident in device (HBM) memory unless a
 *     parameter says "host";
 *   - the caller owns every buffer including workspaces — the library never allocates or
 *     frees device memory and never synchronises;
 *   - workspaces, scratch buffers and output buffers may hold anything on entry, NaN and inf included (fresh hipMalloc memory, the
 *     leftovers of an earlier call at another shape): no result depends on it (tests/test_gpu_history.py);
 *   - all work is enqueued on the caller-supplied hipStream_t (`stream`, may be NULL);
 *   - return value: 0 on success, negative nnd_status on failure (never throws);
 *     nnd_last_error() gives a thread-local message for the last failure;
 *   - threading: every entry point may be called concurrently from several host threads as long as the calls
 *     use distinct streams and distinct output / workspace buffers.  The library keeps no mutable global state:
 *     every kernel of a call — the fused loops' too — is enqueued on the caller's `stream` and nowhere else
 *     (rounds 1-2 ran one branch of the loop on an internal side stream; measured equal, removed);
 *   - diagnostic environment switches (read ONCE when the library is loaded and again only by nnd_reload_switches(), never
 *     on the hot path; they select between kernels that the parity tests prove equivalent, never a non-HIP path; none of them
 *     changes the layout of a packed blob — which convolutions of the update block take a split arithmetic is part of the
 *     descriptor, nnd_update_block_desc.split_layers): NND_NO_FUSED_UPSAMPLE (mask.2 and convex upsample as two launches), NND_NO_FOLDED_FLOW_HEAD (flow_head.conv2 + the recurrence update as their own launch in front of the fused mask / upsample launch instead of inside it),
 *     NND_NO_FUSED_LOOKUP (lookup and convc1 as two launches), NND_NO_MERGED_FB_LOOKUP (flow branch and lookup + convc1 as two launches instead of one launch of two kinds of workgroups), NND_DEBUG_LDS_POISON / NND_DEBUG_LDS_SLACK (diagnostics of the round-3 reproducibility study: pattern-fill every CU's LDS between the loop's launches / ask for more dynamic LDS), NND_SPLIT_NO_FAST (the generic conv_split kernel wherever one exists: every stride-1 shape; the stride-2 kernels are FAST-only and keep running), NND_NO_FUSED_FLOW_BRANCH (convf1 and convf2 as two launches when
 *     arithmetic = 3), NND_SPLIT_CFG (force the workgroup shape of the split kernel), NND_NO_CONV1X1_STREAM (1x1 shortcuts through the
 *     staged conv kernel), NND_CORR_BUILD_V1 (register-operand correlation build), NND_CORR_BUILD_NO_KSPLIT (small grids through the LDS-staged build instead of the k-split one), NND_IGEV_SQUEEZE_V1 / NND_IGEV_SQUEEZE_WALK (cv_squeezer + soft-argmin: the one-row kernel always / the row-walking kernel whenever it can run), NND_AGCL_V1 (one-pixel-per-lane AGCL kernels), NND_AGCL_PB (pixels per workgroup of the channels-last offset kernel), NND_CONV_CFG / NND_CONV_P
 *     (force a tile configuration), NND_CONV_VERBOSE (print the chosen configuration), NND_DEBUG_SYNC
 *     (synchronise and name every launch of the update block on stderr), NND_NO_THIN3D (the regulariser's 8- / 16-channel
 *     Conv3d layers through the MFMA formulation instead of csrc/thin3d.hip), NND_NO_SLAB3D (the same layers at stride 1 with
 *     arithmetic = 2 through the round-2 formulations instead of the depth-marching MFMA kernel csrc/slab3d.hip),
 *     NND_SLAB3D_ROUNDS (depth segments of that kernel: grid of about this many resident sets), NND_NO_C4 (planar instead of 4-channel-
 *     interleaved layout of the update block's conv-only workspace tensors), NND_ENC_NO_C4 (the same for the encoder's activations
 *     with a split arithmetic), NND_NO_FUSED_ENC_BLOCK (the encoder's layer1 and layer2 residual blocks as conv1, shortcut and
 *     conv2 + add launches instead of the one launch of csrc/enc_block.hip).
 */
#ifndef NNDEPTH_AMD_H
#define NNDEPTH_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NND_VERSION 105 /* 0.1.5: 102 descriptors carry struct_size and flags, per-layer fp16x2 activation scales + calibration; 103 group-RAFT entry points; 104 nnd_profile_mfma16_peak (the nnd_midas_* entry points are additions within 104: nothing existing changed its signature or meaning); 105 the single-output EPE criterion's two symbols (the entry point and its workspace query) are removed: nnd_stereo_eval with one output is that criterion (nnd_igev_init_disparity_dev — any G <= 64, D <= 4096, parameters read from device memory — with its queries nnd_igev_init_disparity_supported / _chunk / _kernel, nnd_resize_nearest_scaled and the stereo-geometry entry points nnd_disparity_to_depth ... nnd_pair_both_views are additions within 105: nothing existing changed its signature or meaning) */

/* Descriptors start with `struct_size` = sizeof(the descriptor type) of the header the caller was compiled against; every entry
 * point that takes one refuses another size (NND_ERR_INVALID), so a caller and a library of different versions cannot
 * misread each other's fields.  `flags` is a bit set of NND_FLAG_*.                                                        */
#define NND_FLAG_CALIBRATE 1 /* fp16x2 only: besides its normal work, the call records — for every layer it runs in that
                                arithmetic — the largest |activation| the layer stages, in the layer's slot of the packed blob
                                (`packed_dev` is WRITTEN by such a call; the extra kernels run on `stream` like everything
                                else).  nnd_*_calibration_finish then fixes the layers' activation scales.  See "fp16x2
                                activation range" below.                                                                    */
#define NND_FLAG_LAST_UPSAMPLE_ONLY 2 /* update block, the four nnd_*_refine entry points only (every other entry point that computes
                                refuses it; sizing and packing accept it, the blob layout does not depend on it): the loop computes
                                the upsampled map of the LAST iteration alone — every other iteration runs flow_head.conv1 (without
                                mask.0), flow_head.conv2 and the advance, no mask head and no convex upsample.  up_out receives that
                                one map and up_iter_stride must be 0 (else NND_ERR_INVALID).  up_out, low_out and net_out are
                                bit-identical to those of the call without the flag.  Ignored by a call that also carries
                                NND_FLAG_CALIBRATE (the mask head records its range over every iteration: the whole schedule runs).
                                A library without the flag refuses it as unknown (nnd_update_block_packed_floats < 0).        */

typedef enum {
    NND_OK = 0,
    NND_ERR_INVALID = -1,     /* bad argument / unsupported shape */
    NND_ERR_HIP = -2,         /* a HIP runtime call or launch failed */
    NND_ERR_UNSUPPORTED = -3, /* configuration not built */
    NND_ERR_NO_DEVICE = -4
} nnd_status;

int nnd_version(void);
const char* nnd_last_error(void);
/* number of visible HIP devices (0 when none / on a CPU-only host); never raises */
int nnd_device_count(void);
/* re-reads the NND_* diagnostic switches from the environment (tests and tuning scripts that toggle them in-process);
 * not to be called concurrently with other entry points */
int nnd_reload_switches(void);

/* ------------------------------------------------------------------ correlation pyramid
 * Replaces CorrBlock1D.__init__ + CorrBlock1D.corr
 *   nndepth/models/raft_stereo/cost_volume.py:12-34,55-61
 * level 0: corr[b,h,w1,w2] = sum_c f1[b,c,h,w1]*f2[b,c,h,w2] / sqrt(C);
 * level i+1 = avg_pool1d(level i, 2) (floor on odd widths).  `num_levels`+1 levels are
 * stored (the reference builds one more than it reads).
 * Layout of `pyramid`: level l is a dense (B*H*W, W_l) row-major matrix starting at float
 * offset level_offsets[l] (W_0 = W, W_{l+1} = W_l / 2).                                  */
int nnd_corr1d_pyramid_layout(int B, int H, int W, int num_levels,
                              int64_t* level_offsets /* [num_levels+1] */,
                              int32_t* level_widths /* [num_levels+1] */,
                              int64_t* total_floats);
int nnd_corr1d_build(const float* fmap1, const float* fmap2, float* pyramid,
                     int B, int C, int H, int W, int num_levels, void* stream);

/* Replaces CorrBlock1D.__call__ + linear_sampler
 *   nndepth/models/raft_stereo/cost_volume.py:36-53, nndepth/models/raft_stereo/utils.py:4-27
 * coords (B,1,H,W) -> out (B, num_levels*(2*radius+1), H, W); border-clamped (Q2).        */
int nnd_corr1d_lookup(const float* pyramid, const float* coords, float* out,
                      int B, int H, int W, int num_levels, int radius, void* stream);

/* ------------------------------------------------------------ IGEV geometry-encoding volume
 * Replaces GeometryAwareCostVolume.build_cost_volume + the avg-pool pyramids + forward (combined lookup)
 *   nndepth/models/igev_stereo/cost_volume.py:81-98, :40-52, :54-79
 * Group g correlates channels [g*group_channels, (g+1)*group_channels) of the Ctot-channel maps (the reference
 * uses only the first num_groups chunks of num_groups channels) and divides by sqrt(group_channels).
 * Pyramids use the layout of nnd_corr1d_pyramid_layout(B*num_groups, H, W, num_levels): rows ordered (b,g,h,w1),
 * so level 0 viewed as (B,G,H,W1,W2) is the tensor the 3-D regulariser (nnd_conv3d_*) consumes.
 * num_levels = 0 writes level 0 alone (the fused refinement loop reads the interleaved copy below, which pools for itself).
 * nnd_pyramid_from_level0 fills levels 1..num_levels of a pyramid whose level 0 was written by the caller (the
 * regularised volume, or a feature volume built with num_levels = 0).  nnd_igev_lookup: coords (B,1,H,W) -> out (B, num_levels*2*G*(2r+1), H, W), channel
 * = i*2*G*T + v*G*T + g*T + k with v = 0 feature / 1 geometry volume.                                   */
int nnd_group_corr_build(const float* fmap1, const float* fmap2, float* pyramid, int B, int Ctot, int H, int W,
                         int num_groups, int group_channels, int num_levels, void* stream);
/* GroupCorrBlock1D of Coarse2FineGroupRepViTRAFTStereo (nndepth/models/raft_stereo/cost_volume.py:64-128; widening):
 * nnd_group_corr_build_scaled = nnd_group_corr_build with the divisor given by the caller — GroupCorrBlock1D.corr (:115-128) splits the
 * maps into chunks of `num_groups` channels, correlates the first `num_groups` chunks and divides by sqrt(C_total):
 * group_channels = num_groups, divisor = sqrt(Ctot).
 * nnd_group_corr1d_lookup = GroupCorrBlock1D.__call__ (:94-113) INCLUDING its view without the group permute (Q6): coords (B,1,H,W) ->
 * out (B, num_levels*G*(2r+1), H, W); pixel (y,x), channel i*G*T + j holds sample j % T of row (y*W + x)*G + j/T of the sample's
 * G*H*W (group, pixel) rows at level i, each row sampled at ITS OWN pixel's coordinate.                                        */
int nnd_group_corr_build_scaled(const float* fmap1, const float* fmap2, float* pyramid, int B, int Ctot, int H, int W,
                                int num_groups, int group_channels, int num_levels, float divisor, void* stream);
int nnd_group_corr1d_lookup(const float* pyramid, const float* coords, float* out, int B, int G, int H, int W, int num_levels,
                            int radius, void* stream);
int nnd_pyramid_from_level0(float* pyramid, int B, int H, int W, int num_levels, void* stream);
int nnd_igev_lookup(const float* feat_pyramid, const float* geo_pyramid, const float* coords, float* out,
                    int B, int G, int H, int W, int num_levels, int radius, void* stream);
/* Group-interleaved copy of the levels 0..num_levels-1 of both pyramids, the layout the refinement loop gathers from:
 * per level  il[((b*H*W + h*W + w1) * w2 + x) * 2G + v*G + g]  (v = 0 feature / 1 geometry volume), so that the
 * 2G*(2r+1) samples of GeometryAwareCostVolume.forward (igev_stereo/cost_volume.py:54-79) for one pixel and level are
 * one contiguous run instead of 2G rows.  Written once per pair; nnd_igev_interleaved_floats = its size.           */
int64_t nnd_igev_interleaved_floats(int B, int G, int H, int W, int num_levels);
int nnd_igev_interleave_pyramids(const float* feat_pyramid, const float* geo_pyramid, float* interleaved,
                                 int B, int G, int H, int W, int num_levels, void* stream);
/* The same interleaved levels from the two level-0 volumes alone (rows (b,g,h,w1) of W floats each): the avg_pool1d cascade
 * of cost_volume.py:46-52 runs in LDS with the pyramid's arithmetic (bit-identical to pooling first), so neither pyramid's
 * pooled levels have to exist.  _supported: 2*G <= 32, every level at least 1 wide, one pixel's levels within 160 KB of LDS. */
int nnd_igev_interleave_level0_supported(int G, int W, int num_levels);
int nnd_igev_interleave_level0(const float* feat_level0, const float* geo_level0, float* interleaved,
                               int B, int G, int H, int W, int num_levels, void* stream);

/* ------------------------------------------------- CREStereo adaptive group correlation (AGCL)
 * Replaces AGCL.corr_iter / get_correlation / corr_att_offset and bilinear_sampler / bilinear_grid_sample
 *   nndepth/models/cre_stereo/cost_volume.py:28-79, :81-154;  nndepth/models/cre_stereo/utils.py:5-20,34-107
 * Channels are split into 4 groups of C/4; the 9 search positions are a 1x9 window (small_patch = 0) or a 3x3
 * window (small_patch = 1, dy outer / dx inner); out (N,36,H,W), channel = g*9 + k.
 * nnd_bilinear_sample : img (N,C,H,W), coords (N,Hg,Wg,2) = (x,y) in pixels -> out (N,C,Hg,Wg); taps outside the
 *                       image read zero (grid_sample zeros/align_corners=True semantics incl. the reference's
 *                       pixel -> [-1,1] -> pixel round trip).
 * nnd_agcl_corr_iter  : flow (N,2,H,W); the right features are warped by grid+flow into `warped` (caller-owned
 *                       scratch, N*C*H*W floats), then correlated over the window of the replicate-padded warped map.
 * nnd_agcl_corr_offset: each search position samples fmap2 at grid + flow + window + extra_offset, extra_offset
 *                       (N,18,H,W) with channel 2k = x, 2k+1 = y of position k.  The optional cross attention of the
 *                       reference (att != None) is applied by the caller to fmap1/fmap2 beforehand.             */
int nnd_bilinear_sample(const float* img, const float* coords, float* out, int N, int C, int H, int W, int Hg, int Wg,
                        void* stream);
int nnd_agcl_corr_iter(const float* fmap1, const float* fmap2, const float* flow, float* warped, float* out,
                       int N, int C, int H, int W, int small_patch, void* stream);
int nnd_agcl_corr_offset(const float* fmap1, const float* fmap2, const float* flow, const float* extra_offset, float* out,
                         int N, int C, int H, int W, int small_patch, void* stream);
/* The same on channels-last copies (N,H,W,C) of the two maps, C == 256 (the maps are constant over the iterations of a
 * cascade stage, the copy is made once): one wave per pixel, every bilinear tap is one 1-KB line.  Sums the 64 channels
 * of a group in a different order than nnd_agcl_corr_offset (<= 1e-7 apart).  nnd_nchw_to_nhwc makes the copy.        */
int nnd_agcl_corr_offset_nhwc(const float* fmap1_nhwc, const float* fmap2_nhwc, const float* flow, const float* extra_offset,
                              float* out, int N, int C, int H, int W, int small_patch, void* stream);
int nnd_nchw_to_nhwc(const float* in, float* out, int N, int C, int H, int W, void* stream);

/* IGEV initial disparity: regress_disparity(softmax over the candidate axis)
 *   nndepth/models/igev_stereo/model.py:92-95,145-146
 * logits (B,D,H,W) = the squeezed geometry volume -> out (B,1,H,W) = -sum_d d * softmax_d(logits).              */
int nnd_softargmin_disparity(const float* logits, float* out, int B, int D, int H, int W, void* stream);
/* cv_squeezer + regress_disparity in one pass (nndepth/models/igev_stereo/model.py:63,144-146): geo_level0 = level 0 of
 * the geometry pyramid, rows (b,g,h,w1) of D floats (GeometryAwareCostVolume.geo_aware_cv[0]); weight = the
 * Conv3d(G,1,3,1,1) kernel (1,G,3,3,3) over (candidate, h, w1), bias (1) or NULL — both HOST pointers (they travel as
 * kernel arguments); out (B,1,H,W) = -sum_d d * softmax_d(conv3d(geo)).  G <= 8, D <= 512, else NND_ERR_UNSUPPORTED.
 * nnd_igev_init_disparity_dev: the same operation for G <= 64 and D <= 4096 (frames up to 16384 px wide at 1/4 resolution), else
 * NND_ERR_UNSUPPORTED (the soft-argmin follows ATen's summation order, which opens another accumulator level beyond 4096 rows;
 * beyond either limit the caller composes a Conv3d of its own with nnd_softargmin_disparity).  weight_dev / bias_dev (bias may
 * be NULL) are DEVICE pointers the caller owns: the kernel stages them to LDS, there is no host copy and no synchronisation, so the
 * call captures into a HIP graph.  It always runs the chunked kernel (the candidate axis walked in chunks of
 * nnd_igev_init_disparity_chunk() candidates, the logits kept in LDS), also at shapes nnd_igev_init_disparity serves; the two
 * entry points agree to within the fp32 order of the 27 G products, not bit for bit.  B <= 65535.
 * nnd_igev_init_disparity_supported(G, D): 1 when one of the two entry points serves the shape (1 <= G <= 64, 1 <= D <= 4096).
 * nnd_igev_init_disparity_kernel: the name of the kernel that serves the shape — nnd_igev_init_disparity's choice for G <= 8 and
 * D <= 512 (under the current NND_IGEV_SQUEEZE_* switches), the chunked kernel otherwise — or NULL for an unsupported one. */
int nnd_igev_init_disparity(const float* geo_level0, const float* weight_host, const float* bias_host, float* out,
                            int B, int G, int H, int W, int D, void* stream);
int nnd_igev_init_disparity_dev(const float* geo_level0, const float* weight_dev, const float* bias_dev, float* out,
                                int B, int G, int H, int W, int D, void* stream);
int nnd_igev_init_disparity_supported(int G, int D);
int nnd_igev_init_disparity_chunk(void);
const char* nnd_igev_init_disparity_kernel(int B, int G, int H, int W, int D);

/* ----------------------------------------------------------------------- convex upsample
 * Replaces RAFTStereo.convex_upsample  nndepth/models/raft_stereo/model.py:93-105
 * (IGEV copy igev_stereo/model.py:103-115; 2-channel CRE copy cre_stereo/model.py:110-122)
 * flow (B,C,H,W), mask (B,9*rate*rate,H,W) -> out (B,C,rate*H,rate*W).                    */
int nnd_convex_upsample(const float* flow, const float* mask, float* out,
                        int B, int C, int H, int W, int rate, void* stream);

/* -------------------------------------------------------------------------- update block
 * Replaces BasicUpdateBlock.forward (+BasicMotionEncoder, SepConvGRU/ConvGRU, FlowHead, mask head)
 *   nndepth/blocks/update_block.py:57-65,26-36,97-112 ; nndepth/blocks/gru.py:22-37,53-61   */
/* fp16x2 activation range (arithmetic = 2; csrc/split_arith.h, csrc/calib.hip).  An fp32 activation x is carried as two fp16
 * pieces of x * 2^xs with xs PER LAYER, stored in the packed blob and read by the kernels at run time.
 *   - a freshly packed blob has xs = 2 for every layer: all 22 significand bits for 0.06 <= |x| < 16376, graceful below
 *     (absolute error <= 2^-27), inf / NaN in the output above (never a silently wrong value);
 *   - after a calibration — one or more forwards with NND_FLAG_CALIBRATE on representative inputs, then
 *     nnd_*_calibration_finish — each layer has xs = 11 - ceil(log2(M)), M = the largest |activation| that layer staged
 *     during those forwards: all 22 bits for M * 2^-13 <= |x| <= M, absolute error <= M * 2^-36 below, valid (finite) up to
 *     |x| < 32 * M, inf / NaN in the output beyond — at every output that reads the activation, through the ReLU / sigmoid /
 *     tanh epilogues and the layers behind them (nnd_update_block_forward: and at no output outside the reach of its convs);
 *   - nnd_update_block_scale_slots gives the float offsets of the layers' slots in the blob: slot[1] = 2^xs, so the valid range
 *     of layer i is |x| < 65504 / slot[1] (the Python engines expose it as `activation_ranges()`); nnd_encoder_scale_slots,
 *     nnd_conv3d_scale_slots and nnd_conv2d_scale_slots_ex do the same for the other engines;
 *   - nnd_scales_read / nnd_scales_write move the exponents xs out of and into a blob (set, or widen = per-layer minimum), in
 *     place: a calibration is data — {layer name: xs}, independent of the weights' own scale s — that can be saved, loaded into
 *     another process, merged over ranks and widened; nnd_nonfinite_flag reports an exceeded range from the output.
 * The model classes of nndepth_amd calibrate on their first forward (one extra forward, once) unless a saved state was loaded.
 * arithmetic = 1 ("fp16", one piece) has the same scales, slots, calibration and range behaviour — finite up to 32 * M, inf / NaN
 * beyond, never a finite wrong value — with the precision of ONE piece: 11 significand bits per operand while |x| >= M * 2^-25
 * (an fp16 subnormal below: absolute error <= M * 2^-36).                                                                      */
typedef struct {
    int32_t struct_size;   /* sizeof(nnd_update_block_desc) */
    int32_t hidden_dim;    /* 128; a multiple of 32, at most 192 (160 with 2 flow channels): flow_head.conv2 stages them all in LDS */
    int32_t context_dim;   /* 64 (YAML) or 128 (class default); a multiple of 8 */
    int32_t cor_planes;    /* num_levels*(2r+1) = 36; 576 for IGEV */
    int32_t flow_channels; /* 1 (RAFT/IGEV) or 2 (CRE) */
    int32_t mask_channels; /* 9*rate*rate: 576 (/8) or 144 (/4) */
    int32_t gru_kind;      /* 0 = "sep_conv" (1x5 then 5x1), 1 = "conv_gru" (3x3) */
    int32_t arithmetic;    /* MFMA convolutions of the update block except convc1 (fused with the lookup, exact fp32): mask.2 runs
                              inside the fused mask + upsample kernel and convf1 -> convf2 as one launch in the same arithmetic.
                              0 = exact fp32 (v_mfma_f32_32x32x2_f32); 3 = every fp32 operand carried as 3 bf16 pieces, the 6
                              products x_i*w_j (i + j <= 2) on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (dropped terms
                              <= 2^-24 |x||w|): per-op error vs float64 below the exact kernel's, RAFT-Stereo 544x960 / 32
                              iterations vs the reference 4.3e-5 (exact: 3.6e-5); 2 = every fp32 operand carried as 2 fp16
                              pieces (22 significand bits), the 3 products x0*w0, x0*w1, x1*w0 on v_mfma_f32_32x32x16_f16 with
                              fp32 accumulation — half the matrix work of 3; both operands are range-scaled by exact powers of two
                              (activations x4 while staged, weights per layer at pack time) that the kernel undoes after the K
                              loop, so the low pieces stay out of fp16's subnormals; the activation scale is per layer and
                              calibrated from data, see "fp16x2 activation range" above; csrc/split_arith.h.
                              1 = "fp16", NOT an fp32-parity arithmetic (opt-in): each operand as ONE range-scaled fp16 piece,
                              x^ = fp16_rne(x * 2^xs), w^ = fp16_rne(w * 2^s), one product per K step on v_mfma_f32_32x32x16_f16
                              with fp32 accumulation — a third of the matrix work of 2, half its packed weight bytes.  11
                              significand bits per operand (the bf16 autocast the reference's trainers validate under has 8);
                              valid range as for 2: finite up to 32 x the calibrated maximum of a layer (uncalibrated: |x| <
                              16376), inf / NaN in the output beyond.  Layers the 16-bit kernels do not build (Cin % 16 != 0)
                              stay exact fp32 inside the blob, as under 2 and 3.
                              The packed blob is specific to the value. */
    int32_t split_layers;  /* 0: every convolution the split kernels are built for takes `arithmetic`; else bit i = convolution i
                              (nnd_conv_name) may take it, the others stay exact fp32 (diagnostic: bisecting a difference).  Part
                              of the blob layout, like `arithmetic`: use the same value to pack and to run. */
    int32_t flags;         /* NND_FLAG_* */
} nnd_update_block_desc;

/* Number of weight/bias tensors expected by nnd_update_block_pack, in the order of the
 * reference module's state_dict(): encoder.{convc1,convc2,convf1,convf2,conv},
 * gru.{convz1,convr1,convq1[,convz2,convr2,convq2]}, flow_head.{conv1,conv2}, mask.{0,2};
 * each as (weight, bias).  30 for sep_conv, 24 for conv_gru.                              */
int nnd_update_block_num_tensors(const nnd_update_block_desc* desc);
/* size (floats) of the packed parameter blob */
int64_t nnd_update_block_packed_floats(const nnd_update_block_desc* desc);
/* HOST function (no GPU needed): re-orders PyTorch-layout (Cout,Cin,KH,KW) fp32 weights into
 * the MFMA A-fragment order the kernels stream (see DESIGN.md "packed weights").
 * `tensors_host`: array of host pointers in the order above; `packed_host`: output.       */
int nnd_update_block_pack(const nnd_update_block_desc* desc, const float* const* tensors_host,
                          float* packed_host);
/* workspace (floats) needed by nnd_update_block_forward / nnd_raft_stereo_refine          */
int64_t nnd_update_block_workspace_floats(const nnd_update_block_desc* desc, int B, int H, int W);
/* ONE convolution of the block, `which` in nnd_conv_name order (not convc1 and convf2: those run inside fused kernels), launched
 * exactly as the block launches it — its sources, epilogue (ReLU, GRU z / r and q, bias maps, 0.25 scale), two-source reads and
 * tile-major layouts.  The workspace tensors it touches are filled from in[i] (NCHW, NULL: left as they are) before the launch and
 * copied to out[i] (NULL: not wanted) behind it, i = NND_UB_*:
 *   C1 (B,256,H,W) relu(convc1)        CF (B,256,H,W) [convc2 192 | convf2 64]     HX (B,2*hidden+context,H,W) [h | inp | motion, flow]
 *   Z (B,hidden,H,W)   RH (B,hidden,H,W) r*h   FM (B,3*hidden,H,W) [flow_head.conv1 | mask.0]
 *   CTXB (B,6*hidden,H,W) context terms [zr1 2h | q1 h | zr2 2h | q2 h]            MASK (B,mask_channels,H,W)
 * desc.flags may carry NND_FLAG_CALIBRATE (then nnd_update_block_calibration_finish as usual).  For tests of a single launch. */
enum { NND_UB_C1 = 0, NND_UB_CF, NND_UB_HX, NND_UB_Z, NND_UB_RH, NND_UB_FM, NND_UB_CTXB, NND_UB_MASK, NND_UB_TENSORS };
int nnd_update_block_layer_forward(const nnd_update_block_desc* desc, const float* packed_dev, int which, const float* const* in,
                                   float* const* out, float* workspace, int B, int H, int W, void* stream);
/* fp16x2 calibration (see "fp16x2 activation range"): after one or more calls of nnd_update_block_forward / nnd_*_refine with
 * NND_FLAG_CALIBRATE on this blob, turns the recorded maxima into the layers' activation scales (one tiny kernel on `stream`, no
 * synchronisation) and clears the records.  status_dev: optional device int32 that receives |= 1 if a recorded maximum was
 * inf / NaN (the calibration forward itself overflowed at the old scale: that layer's scale was lowered by 2^12 — calibrate
 * again), |= 2 if some fp16x2 layer of the blob staged nothing (not on the path of those calls: its scale is unchanged).
 * No-op for the other arithmetics.
 * nnd_update_block_scale_slots: float offsets inside the blob of the 4-float slots {2^-(s+xs), 2^xs, record, 2^-s} of the
 * convolutions 0 .. n-1 in nnd_conv_name order (-1 where a convolution is not fp16x2); returns how many convolutions the
 * descriptor has (call with offsets = NULL to size the array).                                                            */
int nnd_update_block_calibration_finish(const nnd_update_block_desc* desc, float* packed_dev, int32_t* status_dev, void* stream);
int nnd_update_block_scale_slots(const nnd_update_block_desc* desc, int64_t* offsets, int n);

/* (net, inp, corr, flow) -> (net_out, mask_out, delta_out); same shapes as the reference:
 * net (B,hidden,H,W) inp (B,context,H,W) corr (B,cor_planes,H,W) flow (B,fc,H,W)
 * mask_out (B,mask_channels,H,W) [already x0.25]  delta_out (B,fc,H,W).
 * mask_out may be NULL (mask head skipped).                                               */
int nnd_update_block_forward(const nnd_update_block_desc* desc, const float* packed_dev,
                             const float* net, const float* inp, const float* corr, const float* flow,
                             float* net_out, float* mask_out, float* delta_out,
                             float* workspace, int B, int H, int W, void* stream);

/* ------------------------------------------------------------------- generic convolution
 * The implicit-GEMM fp32-MFMA convolution the update block is made of, exposed on its own:
 * stride 1, zero "same" padding (KH/2, KW/2), kernels 1x1, 3x3, 1x5, 5x1.  Stands in for one
 * nn.Conv2d (+ optional ReLU) call, e.g. nndepth/blocks/update_block.py:58.
 * nnd_conv2d_pack is a HOST function: w (Cout,Cin,KH,KW), b (Cout) -> packed blob.            */
int64_t nnd_conv2d_packed_floats(int Cout, int Cin, int KH, int KW);
int nnd_conv2d_pack(const float* w_host, const float* b_host, int Cout, int Cin, int KH, int KW,
                    float* packed_host);
int nnd_conv2d_forward(const float* packed_dev, const float* x, float* y, int B, int Cin, int H, int W,
                       int Cout, int KH, int KW, int relu, void* stream);
/* The same with the arithmetic chosen (see nnd_update_block_desc.arithmetic): 0 = exact fp32 MFMA (identical to the
 * functions above), 3 = fp32 operands as 3 bf16 pieces on the bf16 MFMA, 2 = as 2 range-scaled fp16 pieces on the fp16 MFMA
 * (csrc/conv_split.hip; both need Cin % 16 == 0).
 * The packed blob is specific to the arithmetic it was packed for.                                                  */
int64_t nnd_conv2d_packed_floats_ex(int Cout, int Cin, int KH, int KW, int arithmetic);
int nnd_conv2d_pack_ex(const float* w_host, const float* b_host, int Cout, int Cin, int KH, int KW, int arithmetic,
                       float* packed_host);
int nnd_conv2d_forward_ex(const float* packed_dev, const float* x, float* y, int B, int Cin, int H, int W,
                          int Cout, int KH, int KW, int relu, int arithmetic, void* stream);
/* fp16x2 / fp16 calibration of such a single layer (arithmetic == 2 or 1; no-op otherwise): sets the blob's activation scale from the
 * largest |x| of this input (see "fp16x2 activation range").  status_dev as nnd_update_block_calibration_finish.          */
int nnd_conv2d_calibrate_ex(float* packed_dev, const float* x, int B, int Cin, int H, int W, int Cout, int KH, int KW,
                            int arithmetic, int32_t* status_dev, void* stream);
/* HOST: the one scale slot of such a blob (-1 unless arithmetic is 2 or 1); contract as nnd_encoder_scale_slots, returns 1. */
int nnd_conv2d_scale_slots_ex(int Cout, int Cin, int KH, int KW, int arithmetic, int64_t* offsets, int n);

/* Activation scales as data (see "fp16x2 activation range"): the exponent xs of a layer's scale 2^xs read from and written to the
 * slots that nnd_*_scale_slots enumerate, so that a calibration can be saved, loaded into another process or rank, merged and
 * widened.  `offsets`: a HOST array of n slot offsets (1 <= n <= 64, each >= 0), `xs_dev` n device int32.  One tiny kernel on
 * `stream` each, no synchronisation.
 *   nnd_scales_read   xs_dev[i] = xs of slot i; amax_dev (may be NULL) receives the slot's pending calibration record — the largest
 *                     |activation| staged under NND_FLAG_CALIBRATE since the last finish, 0 if none — which clear_records != 0 then
 *                     clears: a forward under the flag followed by this call instead of nnd_*_calibration_finish measures what
 *                     each layer sees and changes no scale.
 *   nnd_scales_write  mode 0: xs = xs_dev[i]; mode 1: xs = min(current, xs_dev[i]) — the range only grows (each step down doubles the
 *                     largest representable |x| and moves the 13-octave full-precision window up with it).  xs is clamped to
 *                     |xs| <= 60 like a calibration's, and the slot's 2^xs and 2^-(s+xs) are rewritten IN PLACE: the blob is not
 *                     reallocated, so a captured graph that reads it runs with the new scales on its next replay.  A slot listed
 *                     twice is refused.  Must not overlap inference on the same blob from another stream (the kernels read the
 *                     two values separately).  Records are not touched.
 * nnd_nonfinite_flag: *word_dev |= 1 if any of the n floats of x is inf or NaN (n >= 1).  An exceeded range always reaches the
 * output as inf / NaN, so this over a model's final output detects it without a host synchronisation.                       */
int nnd_scales_read(float* packed_dev, const int64_t* offsets, int n, int32_t* xs_dev, float* amax_dev, int clear_records,
                    void* stream);
int nnd_scales_write(float* packed_dev, const int64_t* offsets, int n, const int32_t* xs_dev, int mode, void* stream);
int nnd_nonfinite_flag(const float* x, int64_t n, int32_t* word_dev, void* stream);

/* conv + CREStereo's search-offset activation in the epilogue: y = range * (sigmoid(conv(x)) - 0.5) * 2
 *   nndepth/models/cre_stereo/model.py:158-159,171-172 (conv_offset_16 / conv_offset_8); blob of nnd_conv2d_pack.      */
int nnd_conv2d_offset_forward(const float* packed_dev, const float* x, float* y, int B, int Cin, int H, int W,
                              int Cout, int KH, int KW, float range, void* stream);

/* ------------------------------------------------------------- glue operators of the model forwards (csrc/cascade.hip)
 * nnd_split_tanh_relu    : x (B, Cnet+Cinp, H, W) -> net = tanh(x[:, :Cnet]), inp = relu(x[:, Cnet:])
 *                          nndepth/models/raft_stereo/model.py:119-122 (igev_stereo/model.py:129-131, cre_stereo/model.py:148-151)
 * nnd_avg_pool_2x_4x     : out2 = F.avg_pool2d(x, 2, stride=2) (N,C,H/2,W/2) and out4 = F.avg_pool2d(x, 4, stride=4)
 *                          (N,C,H/4,W/4) in one pass                           cre_stereo/model.py:154-177
 * nnd_resize_bilinear_ac : y (N,C,H,W) = mul * F.interpolate(x (N,C,h,w), (H,W), mode="bilinear", align_corners=True)
 *                          cre_stereo/model.py:205-212,235-241,259-265 (flow hand-over between cascade stages)
 * nnd_resize_nearest_scaled : y (N,1,H,W) = mul * F.interpolate(x (N,1,h,w), size=(H,W)) (mode "nearest"), the frame-size stage
 *                          outputs of the Coarse2Fine cascade, raft_stereo/model.py:309-314: y[n,oy,ox] = mul * x[n, oy*h/H, ox*w/W].
 *                          H % h == 0 and W % w == 0 (integer ratios in both axes), else NND_ERR_INVALID; bit-identical to the
 *                          PyTorch expression, NaN and signed zeros included.
 * nnd_pos_enc_sine_add   : y = x + pe[:, :, :H, :W], PositionEncodingSine.forward  nndepth/blocks/pos_enc.py:22-42 (used at
 *                          cre_stereo/model.py:180-196): the table is generated on the fly, pe[4k+j] = sin / cos (j odd) of
 *                          pos * exp(2k * rate), pos = column + 1 (j < 2) or row + 1, rate = the reference's
 *                          `-log(1e4) / d_model // 2` with Python's precedence (= -1; temp_bug_fix != 0: -log(1e4) / (d_model // 2)).
 *                          x1 / y1 (a second map of the same shape, may both be NULL) get the same table in the same launch.    */
int nnd_split_tanh_relu(const float* x, float* net, float* inp, int B, int Cnet, int Cinp, int H, int W, void* stream);
int nnd_pos_enc_sine_add(const float* x0, const float* x1, float* y0, float* y1, int N, int C, int H, int W, int temp_bug_fix,
                         void* stream);
int nnd_avg_pool_2x_4x(const float* x, float* out2, float* out4, int N, int C, int H, int W, void* stream);
int nnd_resize_bilinear_ac(const float* x, float* y, int N, int C, int h, int w, int H, int W, float mul, void* stream);
int nnd_resize_nearest_scaled(const float* x, float* y, int N, int h, int w, int H, int W, float mul, void* stream);

/* Convolution + folded eval-mode BatchNorm + ReLU / residual epilogue (the building block of the encoder):
 *   y = conv(x; w, stride, "same" padding K/2) ; y = (y + bias - mean) * gamma / sqrt(var + eps) + beta   [norm optional]
 *   if relu: y = max(y, 0);  if residual: y = residual + y;  if relu_after_residual: y = max(y, 0)
 * Stands in for nn.Conv2d [+ nn.BatchNorm2d(eval)] [+ ReLU] and the `relu(x + y)` of
 * nndepth/blocks/residual_block.py:53-60.  Kernels 1x1 / 3x3 at stride 1 or 2 (1x5 / 5x1 at stride 1);
 * x (B,Cin,Hin,Win) -> y (B,Cout,ceil(Hin/stride),ceil(Win/stride)), residual like y.  nnd_conv_pack is a HOST function
 * (the norm is folded in double precision into a per-channel scale / shift); bn_* may be NULL (no norm).          */
typedef struct nnd_conv_desc {
    int Cout, Cin, KH, KW, stride;
} nnd_conv_desc;
int64_t nnd_conv_packed_floats(const nnd_conv_desc* desc);
int nnd_conv_pack(const nnd_conv_desc* desc, const float* w_host, const float* bias_host, const float* bn_gamma,
                  const float* bn_beta, const float* bn_mean, const float* bn_var, float bn_eps, float* packed_host);
int nnd_conv_forward(const nnd_conv_desc* desc, const float* packed_dev, const float* x, const float* residual, float* y,
                     int B, int Hin, int Win, int relu, int relu_after_residual, void* stream);
/* The same layer with the arithmetic chosen (nnd_update_block_desc.arithmetic: 0, 3, 2 or 1; the stride-1 1x1 projections stay
 * exact, as in the encoder) and, with workspace != NULL (nnd_conv_workspace_floats_ex floats), run in the encoder's own layout —
 * tile-major with 4 channels interleaved: x, residual and y are NCHW here and converted on the way.  flags = NND_FLAG_CALIBRATE:
 * the layer's activation scale is set from this input behind the launch (packed_dev is written; status_dev as
 * nnd_update_block_calibration_finish, may be NULL).                                                                      */
int64_t nnd_conv_packed_floats_ex(const nnd_conv_desc* desc, int arithmetic);
int nnd_conv_pack_ex(const nnd_conv_desc* desc, int arithmetic, const float* w_host, const float* bias_host, const float* bn_gamma,
                     const float* bn_beta, const float* bn_mean, const float* bn_var, float bn_eps, float* packed_host);
int64_t nnd_conv_workspace_floats_ex(const nnd_conv_desc* desc, int B, int Hin, int Win);
int nnd_conv_forward_ex(const nnd_conv_desc* desc, int arithmetic, int flags, float* packed_dev, const float* x, const float* residual,
                        float* y, float* workspace, int32_t* status_dev, int B, int Hin, int Win, int relu, int relu_after_residual,
                        void* stream);

/* ------------------------------------------------------------------------- feature encoder
 * Replaces BasicEncoder.forward  nndepth/encoders/basic_encoder.py:71-93 (norm_fn "batch" in eval mode, or "none"),
 * ResidualBlock.forward nndepth/blocks/residual_block.py:53-60 and, optionally, the context projection
 * `cnet_proj` of nndepth/models/raft_stereo/model.py:53-55 applied to the first n_cnet maps (the left frames).
 * norm: 0 = none, 1 = BatchNorm2d (running statistics, folded at pack time), 2 = InstanceNorm2d(affine=False) (CREStereo,
 * cre_stereo/model.py:70-72; per-sample statistics computed on the device).  cnet_dim: channels of cnet_proj, 0 = absent.
 * nnd_encoder_pack (HOST): `tensors` = units of 6 pointers {weight, bias, norm weight, norm bias, running_mean,
 * running_var} (the last four NULL where there is no norm) in the order: conv1 | for each residual block layer1.0,
 * layer1.1, layer2.0, layer2.1, layer3.0, layer3.1: conv1, conv2, downsample.0 (its norm = norm3) | conv2 | cnet_proj.0.
 * nnd_encoder_forward: frames (N,3,H,W) -> fmap (N,output_dim,H/8,W/8); cnet_out (n_cnet,cnet_dim,H/8,W/8) or NULL.
 * workspace: nnd_encoder_workspace_floats(desc, N, H, W) floats, caller-owned.                                     */
typedef struct nnd_encoder_desc {
    int32_t struct_size; /* sizeof(nnd_encoder_desc) */
    int32_t output_dim, norm, cnet_dim;
    int32_t arithmetic; /* 0 = exact fp32 MFMA; 3 / 2 = the 3x3 convolutions at stride 1 and 2, the stride-2 1x1 shortcuts and
                           cnet_proj on the 16-bit MFMA with 3 bf16 / 2 fp16 split operands (see nnd_update_block_desc.arithmetic); 1 = the same
                           layers with ONE range-scaled fp16 piece per operand (11 significand bits; finite up to 32 x a layer's
                           calibrated maximum, inf / NaN beyond);
                           the stem, the stride-1 1x1 shortcuts and the 1x1 output conv stay exact fp32 */
    int32_t flags;      /* NND_FLAG_* */
} nnd_encoder_desc;
int nnd_encoder_num_tensors(const nnd_encoder_desc* desc);
int64_t nnd_encoder_packed_floats(const nnd_encoder_desc* desc);
int64_t nnd_encoder_workspace_floats(const nnd_encoder_desc* desc, int N, int H, int W);
int nnd_encoder_pack(const nnd_encoder_desc* desc, const float* const* tensors_host, float bn_eps, float* packed_host);
int nnd_encoder_forward(const nnd_encoder_desc* desc, const float* packed_dev, const float* frames, float* fmap,
                        float* cnet_out, int n_cnet, float* workspace, int N, int H, int W, void* stream);
/* The same with the batch in two tensors: samples 0 .. nsplit-1 from `frames`, nsplit .. N-1 from `frames_b` — the left and the
 * right frames of a pair batch where they lie, instead of the torch.cat([frame1, frame2]) copy the reference makes
 * (nndepth/encoders/basic_encoder.py:74-76).  frames_b == NULL: as nnd_encoder_forward.                               */
int nnd_encoder_forward2(const nnd_encoder_desc* desc, const float* packed_dev, const float* frames, const float* frames_b, int nsplit,
                         float* fmap, float* cnet_out, int n_cnet, float* workspace, int N, int H, int W, void* stream);
/* fp16x2 calibration of the encoder's layers after forwards with NND_FLAG_CALIBRATE (as nnd_update_block_calibration_finish) */
int nnd_encoder_calibration_finish(const nnd_encoder_desc* desc, float* packed_dev, int32_t* status_dev, void* stream);
/* HOST (no GPU): float offsets inside the blob of the layers' 4-float scale slots (see nnd_update_block_scale_slots), one entry per
 * convolution in nnd_encoder_pack's order, -1 where a convolution is not range-scaled (the stem, conv2, the stand-in shortcuts of
 * the stride-1 blocks; every one under arithmetic 0 / 3).  Returns the number of convolutions; offsets == NULL sizes the array,
 * n smaller than that number is refused.  nnd_encoder_scale_name: the reference's key of convolution `which` — "conv1",
 * "layer1.0.conv1", "layer1.0.conv2", "layer1.0.downsample.0", ..., "conv2", "cnet_proj" — or "" beyond.                  */
int nnd_encoder_scale_slots(const nnd_encoder_desc* desc, int64_t* offsets, int n);
const char* nnd_encoder_scale_name(const nnd_encoder_desc* desc, int which);

/* ------------------------------------------------------------------------- RepViT encoder side (Coarse2Fine)
 * Replaces the encoder side of Coarse2FineGroupRepViTRAFTStereo.forward  nndepth/models/raft_stereo/model.py:275-288: RepViT.forward
 * (nndepth/encoders/rep_vit.py:736-744; stem rep_vit.py:429-479, ConvPatchEmbed 309-360, RepFormerBlock 227-306, RepTokenMixer
 * 117-224, AttentionBlock 363-426, ChannelMixer 69-114), LinearSelfAttention (nndepth/blocks/attn_block.py:151-169), MobileOneBlock
 * (nndepth/blocks/conv.py:130-371), RepLargeKernelConv (conv.py:374-442; no activation, conv.py:454) and FeatureFusionBlock
 * (conv.py:549-567), plus the three MobileOne cnet_proj blocks (model.py:216-222).  Exact fp32 (no split arithmetic, no calibration).
 * The descriptor carries the configuration; strides are 1 or 2 (the reference's (1, 1) / (2, 2)), patch_size 3, 5 or 7.
 * nnd_repvit_pack (HOST): `tensors` = nnd_repvit_num_tensors(desc) pointers, 3 per layer {weight, bias, scale or NULL}, every
 * branch / BatchNorm already folded (ops.RepViTEngine, float64 on the host), in the layer order:
 *   stem.0 (16,3,3,3) | stem.1 (16,1,3,3) | stem.2 (16,16,1,1) | per stage i: patch embed depthwise (C_in,1,k,k), patch embed 1x1
 *   (C_i,C_in,1,1), per block: [repmixer: token mixer depthwise (C_i,1,3,3)] or [attention: qkv (1+2C_i,C_i,1,1), out_proj (C_i,C_i,1,1)
 *   with scale = layer_scale_1], [FFN: fc1 (hid,C_i,1,1), fc2 (C_i,hid,1,1) with scale = layer_scale(_2)] |
 *   cnet_proj.0 (cnet_dim,C_3), cnet_proj.1 (cnet_dim,fusion_dim[0]), cnet_proj.2 (cnet_dim,fusion_dim[0]) |
 *   fusion 0 coarse (fusion_dim[0],C_3), fine (fusion_dim[0],C_1) | fusion 1 coarse (fusion_dim[1],fusion_dim[0]), fine (fusion_dim[1],16)
 * (a fusion block's halves: conv3 composed with conv1 / conv2; the coarse half is applied before the bilinear upsample).
 * A layer with a scale computes residual + scale * (conv + bias) (the caller passes bias already multiplied by the scale).
 * nnd_repvit_forward: frames (nsplit,3,H,W) and frames_b (N - nsplit,3,H,W) where they lie (frames_b NULL: all N from frames) ->
 *   feat0 (N,C_3,H/64,W/64), feat1 (N,fusion_dim[0],H/16,W/16), feat2 (N,fusion_dim[1],H/4,W/4) (at the default strides; each
 *   stride-2 step maps n to (n - 1) / 2 + 1) and cnet0..2 (B,cnet_dim,...) of the first B = nsplit samples (frames_b given) or
 *   all N.  workspace: nnd_repvit_workspace_floats(desc, N, H, W) floats, caller-owned.  All launches on `stream`.            */
typedef struct nnd_repvit_desc {
    int32_t struct_size;     /* sizeof(nnd_repvit_desc) */
    int32_t stem_strides[3]; /* 1 or 2 */
    int32_t patch_size;      /* 3, 5, 7 */
    int32_t down_strides[4]; /* 1 or 2 */
    int32_t channels[4];     /* stage widths (32, 64, 128, 256) */
    int32_t num_blocks[4];
    int32_t mixer[4];        /* 0 = repmixer, 1 = attention */
    int32_t ffn_hidden[4];   /* 0 = no FFN (use_ffn false; attention stages always have one) */
    int32_t cnet_dim;        /* 2 * context_dim */
    int32_t fusion_dim[2];   /* output channels of the two FeatureFusionBlocks (64, 64) */
    int32_t flags;           /* 0 */
} nnd_repvit_desc;
int nnd_repvit_num_tensors(const nnd_repvit_desc* desc);
int64_t nnd_repvit_packed_floats(const nnd_repvit_desc* desc);
int64_t nnd_repvit_workspace_floats(const nnd_repvit_desc* desc, int N, int H, int W);
int nnd_repvit_pack(const nnd_repvit_desc* desc, const float* const* tensors_host, float* packed_host);
int nnd_repvit_forward(const nnd_repvit_desc* desc, const float* packed_dev, const float* frames, const float* frames_b, int nsplit,
                       float* feat0, float* feat1, float* feat2, float* cnet0, float* cnet1, float* cnet2, float* workspace, int N,
                       int H, int W, void* stream);

/* The encoder side's kernels one at a time, as nnd_repvit_forward launches them (NCHW, fp32, all on `stream`):
 *   nnd_repvit_depthwise   y (N,C,Ho,Wo) = [GELU](depthwise k x k conv(x; w (C,1,k,k), bias, stride, padding k/2)), k 3 / 5 / 7,
 *                          stride 1 / 2, Ho = (H - 1) / stride + 1 (PyTorch's output size for padding k/2)
 *   nnd_repvit_stem        y (N,16,Ho,Wo) = GELU(conv 3x3 (3 -> 16, padding 1)(x; w (16,3,3,3), bias)); samples n >= nsplit read x1
 *   nnd_repvit_pointwise*  1x1 conv on conv_mfma: y = GELU(conv + bias) (gelu), residual + scale * conv + bias (residual; pack the
 *                          bias already multiplied by the scale; scale NULL = 1) or conv + bias; pack on the HOST
 *   nnd_repvit_linear_attention   qkv (N,1+2C,H,W) -> out (N,C,H,W): LinearSelfAttention's core per (sample, row), W <= 4096
 *   nnd_repvit_upsample_add_relu  y (N,C,H,W) = relu(y + F.interpolate(a (N,C,h,w), (H,W), "bilinear", align_corners=False)) */
int nnd_repvit_depthwise(const float* x, const float* w, const float* bias, float* y, int N, int C, int H, int W, int k, int stride,
                         int gelu, void* stream);
int nnd_repvit_stem(const float* x, const float* x1, int nsplit, const float* w, const float* bias, float* y, int N, int H, int W,
                    int stride, void* stream);
int64_t nnd_repvit_pointwise_packed_floats(int Cout, int Cin, int stride);
int nnd_repvit_pointwise_pack(int Cout, int Cin, int stride, const float* w, const float* bias, const float* scale, float* packed_host);
int nnd_repvit_pointwise(int Cout, int Cin, int stride, const float* packed_dev, const float* x, const float* residual, float* y, int N,
                         int H, int W, int gelu, void* stream);
int nnd_repvit_linear_attention(const float* qkv, float* out, int N, int C, int H, int W, void* stream);
int nnd_repvit_upsample_add_relu(const float* a, float* y, int N, int C, int h, int w, int H, int W, void* stream);

/* ------------------------------------------------------------------------- MobileNetV3 encoder side (IGEVStereoMBNet)
 * Replaces IGEVStereoMBNet.forward_fnet  nndepth/models/igev_stereo/model.py:163-203: MobilenetV3LargeEncoder
 * (nndepth/encoders/mobilenetv3_encoder.py) over timm's tf_mobilenetv3_large_100(features_only=True) (stages 0..5; TF "same"
 * padding, BatchNorm eps 1e-3), fnet_proj / cnet_proj (Conv2d(24 -> fnet_dim / cnet_dim, 3, padding 1) + ReLU) and the guide split.
 * Exact fp32 (no split arithmetic, no calibration).  The backbone's layout is fixed; the descriptor carries the projections' widths.
 * nnd_mbv3_pack (HOST): `tensors` = nnd_mbv3_num_tensors(desc) pointers, 2 per layer {weight, bias}, every BatchNorm already folded
 * (ops.MobileNetV3Engine, float64 on the host), in the layer order:
 *   conv_stem (16,3,3,3) | per block of stages 0..5: [InvertedResidual: conv_pw (mid,cin,1,1)] conv_dw (mid,1,k,k)
 *   [SE: conv_reduce (rd,mid,1,1), conv_expand (mid,rd,1,1)] conv_pwl / conv_pw (cout,mid,1,1) | fnet_proj (fnet_dim,24,3,3) |
 *   cnet_proj (cnet_dim,24,3,3)
 * nnd_mbv3_forward: frame1, frame2 (B,3,H,W) where they lie -> fmap1, fmap2 (B,fnet_dim,H/4,W/4), cnet1 (B,cnet_dim,H/4,W/4) and
 *   the left frames' guides guide0 (B,40,H/8,W/8), guide1 (B,80,H/16,W/16), guide2 (B,160,H/32,W/32); every stride-2 step maps n to
 *   ceil(n / 2).  workspace: nnd_mbv3_workspace_floats(desc, B, H, W) floats, caller-owned.  All launches on `stream`.        */
typedef struct nnd_mbv3_desc {
    int32_t struct_size; /* sizeof(nnd_mbv3_desc) */
    int32_t fnet_dim;    /* fnet_proj output channels (2 * hidden_dim) */
    int32_t cnet_dim;    /* cnet_proj output channels (2 * context_dim) */
    int32_t flags;       /* 0 */
} nnd_mbv3_desc;
int nnd_mbv3_num_tensors(const nnd_mbv3_desc* desc);
int64_t nnd_mbv3_packed_floats(const nnd_mbv3_desc* desc);
int64_t nnd_mbv3_workspace_floats(const nnd_mbv3_desc* desc, int B, int H, int W);
int nnd_mbv3_pack(const nnd_mbv3_desc* desc, const float* const* tensors_host, float* packed_host);
int nnd_mbv3_forward(const nnd_mbv3_desc* desc, const float* packed_dev, const float* frame1, const float* frame2, float* fmap1,
                     float* fmap2, float* cnet1, float* guide0, float* guide1, float* guide2, float* workspace, int B, int H, int W,
                     void* stream);

/* The encoder side's kernels one at a time, as nnd_mbv3_forward launches them (NCHW, fp32, all on `stream`); act: 0 none, 1 ReLU,
 * 2 hard-swish:
 *   nnd_mbv3_depthwise   y (N,C,Ho,Wo) = act(depthwise k x k conv(x; w (C,1,k,k), bias, stride, TF same padding)), k 3 / 5,
 *                        stride 1 / 2, Ho = ceil(H / stride); partial (optional, nnd_mbv3_se_partials(N,C,Ho,Wo) doubles): the
 *                        per-workgroup sums of y that nnd_mbv3_se reads
 *   nnd_mbv3_se          gate (N,C) = hardsigmoid(conv_expand(relu(conv_reduce(mean_hw(y))))) from the partials; y *= gate in place
 *                        (wr (rd,C), br (rd), we (C,rd), be (C); C <= 1024, rd <= 256)
 *   nnd_mbv3_stem        y (N,16,ceil(H/2),ceil(W/2)) = hardswish(conv 3x3 stride 2, TF same padding (3 -> 16)(x; w, bias));
 *                        samples n >= nsplit read x1
 *   nnd_mbv3_pointwise*  k x k (1 or 3, padding k / 2) stride-1 conv on conv_mfma: y = act(conv + bias), or residual + conv + bias;
 *                        pack on the HOST
 *   nnd_mbv3_proj        fnet_proj / cnet_proj: y (N,Cout,H,W) = relu(conv 3x3, padding 1 (x (N,Cin,H,W); w (Cout,Cin,3,3), bias)),
 *                        Cin <= 64 (VALU, per input channel one fp32 9-tap chain, the channels summed in float64)           */
int nnd_mbv3_depthwise(const float* x, const float* w, const float* bias, float* y, double* partial, int N, int C, int H, int W, int k,
                       int stride, int act, void* stream);
int64_t nnd_mbv3_se_partials(int N, int C, int H, int W);
int nnd_mbv3_se(float* y, const double* partial, const float* wr, const float* br, const float* we, const float* be, float* gate, int N,
                int C, int rd, int H, int W, void* stream);
int nnd_mbv3_stem(const float* x, const float* x1, int nsplit, const float* w, const float* bias, float* y, int N, int H, int W,
                  void* stream);
int64_t nnd_mbv3_pointwise_packed_floats(int Cout, int Cin, int k);
int nnd_mbv3_pointwise_pack(int Cout, int Cin, int k, const float* w, const float* bias, float* packed_host);
int nnd_mbv3_proj(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Cout, int H, int W, void* stream);
int nnd_mbv3_pointwise(int Cout, int Cin, int k, const float* packed_dev, const float* x, const float* residual, float* y, int N, int H,
                       int W, int act, void* stream);

/* ------------------------------------------------------------------------------ MobileNetV3DepthModel (csrc/midas.hip)
 * The reference's monocular model (nndepth/models/midas/models/mobilenet_v3.py) in one call, exact fp32: the MobileNetV3-Large
 * backbone above on ONE frame tensor (stages 0..5, taps of stages 1, 2, 4, 5), BaseDecoder (four skip convs, four UpsamplerBlocks)
 * and the last_conv head.  x (B,3,H,W) -> depth (B,1,H,W); H and W must be multiples of 32 (refused by name otherwise: the
 * decoder's x2 upsamples would not meet the backbone's ceil(n / 2) maps).  feature_channels: multiples of 16 up to 128.
 * nnd_midas_pack (HOST): `tensors` = nnd_midas_num_tensors(desc) pointers, 2 per layer {weight, bias}, every BatchNorm already
 *   folded into its conv, in the order: the backbone's layers as nnd_mbv3_pack takes them (without fnet_proj / cnet_proj) |
 *   decoder.skip_layers.0..3 | per decoder.upsampler_layers.0..3: [conv1 + bn1 (blocks 0..2 only: block 3 runs without a skip
 *   input, its conv1 / bn1 are never evaluated)], conv2 + bn2, out_conv | last_conv.0, last_conv.2, last_conv.4.
 * nnd_midas_forward: all launches on `stream`, no allocation, no synchronisation; workspace = nnd_midas_workspace_floats floats,
 *   caller-owned.  After the call the workspace still holds the four taps, the decoder's output (B,C,H/2,W/2) and — with
 *   NND_MIDAS_KEEP_PRE in desc->flags — the map before the final ReLU (B,1,H,W), at nnd_midas_workspace_offset(desc, which, ...)
 *   floats (which: 0..3 taps, 4 decoder output, 5 pre-ReLU map).                                                             */
#define NND_MIDAS_KEEP_PRE 1
typedef struct nnd_midas_desc {
    int32_t struct_size; /* sizeof(nnd_midas_desc) */
    int32_t feature_channels;
    int32_t flags;       /* NND_MIDAS_KEEP_PRE or 0 */
} nnd_midas_desc;
int nnd_midas_num_tensors(const nnd_midas_desc* desc);
int64_t nnd_midas_packed_floats(const nnd_midas_desc* desc);
int64_t nnd_midas_workspace_floats(const nnd_midas_desc* desc, int B, int H, int W);
int64_t nnd_midas_workspace_offset(const nnd_midas_desc* desc, int which, int B, int H, int W);
int nnd_midas_pack(const nnd_midas_desc* desc, const float* const* tensors_host, float* packed_host);
int nnd_midas_forward(const nnd_midas_desc* desc, const float* packed_dev, const float* x, float* depth, float* workspace, int B, int H,
                      int W, void* stream);
/* The model's new kernels one at a time, as nnd_midas_forward launches them (NCHW, fp32, all on `stream`); channel counts:
 * multiples of 16 up to 128.
 *   nnd_midas_up2x_pw   y (N,Cout,2h,2w) = relu(conv1x1(up2x(x (N,Cin,h,w))) + bias), up2x = F.interpolate(scale_factor=2,
 *                       mode="bilinear", align_corners=False) evaluated while the tile is staged: the upsampled map is never
 *                       written.  packed: nnd_midas_up2x_pw_pack (HOST) of w (Cout,Cin,1,1), bias.
 *   nnd_midas_head      depth (N,1,2h,2w) = relu(conv1x1_{C->1}(relu(conv3x3_{C->C}(up2x(t (N,C,h,w))) + b2)) + b4) in one kernel;
 *                       pre_relu (optional, same shape): the value before the last ReLU.  packed: nnd_midas_head_pack (HOST) of
 *                       w2 (C,C,3,3), b2 (C), w4 (1,C,1,1), b4 (1).
 *   nnd_midas_conv_add  y = feat + relu(conv k x k (1 or 3, padding k / 2)(x) + bias): the activation BEFORE the addition
 *                       (nnd_mbv3_pointwise's residual mode adds first); packed: nnd_mbv3_pointwise_pack.                     */
int64_t nnd_midas_up2x_pw_packed_floats(int Cout, int Cin);
int nnd_midas_up2x_pw_pack(int Cout, int Cin, const float* w, const float* bias, float* packed_host);
int nnd_midas_up2x_pw(int Cout, int Cin, const float* packed_dev, const float* x, float* y, int N, int h, int w, void* stream);
int64_t nnd_midas_head_packed_floats(int C);
int nnd_midas_head_pack(int C, const float* w2, const float* b2, const float* w4, const float* b4, float* packed_host);
int nnd_midas_head(int C, const float* packed_dev, const float* t, float* depth, float* pre_relu, int N, int h, int w, void* stream);
int nnd_midas_conv_add(int Cout, int Cin, int k, const float* packed_dev, const float* x, const float* feat, float* y, int N, int H, int W,
                       void* stream);

/* ------------------------------------------------------------- pre- / post-processing on the device
 * nnd_resize_normalize : preprocess_frame  nndepth/models/raft_stereo/scripts/inference.py:55-60
 *     dst (B,C,H,W) = (bilinear_resize(src) - sub) / div, bilinear as F.interpolate(mode="bilinear") (align_corners=False);
 *     src is float (B,C,h,w), or — src_is_u8_hwc != 0 — the decoded image itself, uint8 (B,h,w,C).
 * nnd_replicate_pad    : Padder.pad / unpad  nndepth/data/dataloaders/utils.py:5-21
 *     dst (B,C,H+top+bottom,W+left+right) = F.pad(src, (left,right,top,bottom), mode="replicate"); negative values crop.
 *   (EvalCriterion.__call__ of raft_stereo/scripts/evaluate.py:48-83 is nnd_stereo_eval with one output, below.)        */
int nnd_resize_normalize(const void* src, int src_is_u8_hwc, float* dst, int B, int C, int h, int w, int H, int W,
                         float sub, float div, void* stream);
int nnd_replicate_pad(const float* src, float* dst, int B, int C, int H, int W, int left, int right, int top, int bottom,
                      void* stream);

/* ------------------------------------------------------------- monocular evaluation criterion on the device (additions within 104)
 * nnd_depth_eval : DepthEvalCriterion.__call__  nndepth/models/midas/scripts/evaluate.py:48-211 with scale_shift_estimation,
 *     ssi_depth and normalize_01_depth  nndepth/models/midas/loss.py:6-59.  pred, gt: (B,1,H,W) fp32; valid_mask: (B,1,H,W) bytes
 *     or NULL (every pixel); B*H*W < 2^31.  In the reference's order, everything after the load in double:
 *       1 per sample with more than 100 pixels in valid_mask: scale, shift = least squares of pred * scale + shift ~ gt over
 *         valid_mask (centred sums; a constant prediction c takes the minimum-norm solution scale = c gm / (c^2 + 1), shift =
 *         gm / (c^2 + 1), gm the mean of gt, as torch.linalg.lstsq returns on the CPU); aligned = pred * scale + shift,
 *         else aligned = pred;
 *       2 metric mask = valid_mask & gt > 0.1f & gt < max_depth (both strict, compared as fp32); no pixel in it: out = inf for
 *         the six errors, 0 for the three deltas (_empty_metrics);
 *       3 over the metric mask of the whole batch: abs_rel, sq_rel, rmse, rmse_log, delta1..3 (max(a/g, g/a) < 1.25^k); a
 *         non-positive aligned value makes rmse_log NaN;
 *       4 x_n = (x - min) / (max - min + 1e-6) for gt and for aligned with the batch's min / max over the metric mask; per
 *         sample shift = lower median (sorted position (n - 1) / 2, torch.median) and scale = mean |x_n - shift| over its
 *         pixels of the metric mask, a scale of exactly 0 becomes 1; ssi = (x_n - shift) / scale; ssi_mae, ssi_rmse over the
 *         metric mask (a sample without a pixel in it contributes nothing).
 *     out (device, 10 doubles) = abs_rel, sq_rel, rmse, rmse_log, delta1, delta2, delta3, ssi_mae, ssi_rmse, number of pixels in
 *     the metric mask.  `workspace` = nnd_depth_eval_workspace_bytes(B) device bytes (8-byte aligned; B <= 65535), checked against
 *     workspace_bytes.  Seven small launches on `stream`, no host synchronisation, no floating-point atomics: the same bits
 *     run to run.  Non-finite inputs inside the mask, and a prediction that is constant only up to rounding, are outside the
 *     contract.
 * nnd_depth_eval_accumulate : the dataset mean's bookkeeping  nndepth/models/midas/scripts/evaluate.py:300-302
 *     for i < 9: if metrics[i] is finite, sums[i] += metrics[i] and counts[i] += 1 (all device doubles).                       */
int64_t nnd_depth_eval_workspace_bytes(int B);
int nnd_depth_eval(const float* pred, const float* gt, const unsigned char* valid_mask, int B, int H, int W, float max_depth,
                   void* workspace, int64_t workspace_bytes, double* out, void* stream);
int nnd_depth_eval_accumulate(const double* metrics, double* sums, double* counts, void* stream);

/* ------------------------------------------------------------- value of the monocular training loss on the device (additions within 105)
 * nnd_midas_loss : MiDasLoss.forward  nndepth/models/midas/loss.py:62-221 (what the trainer's validation loop scores a checkpoint
 *     on, midas/trainer.py:168-180, 321-352).  The VALUE only: there is no backward.
 *     pred (B,1,H,W) fp32 read through its batch and row strides (in elements; the innermost stride is 1; rows do not overlap), so a
 *     cropped view is read where it lies; target (B,1,H,W) fp32 and valid_mask (B,1,H,W) bytes, both contiguous, the mask REQUIRED;
 *     no input is written.  H, W >= 16, B <= 65535, B*H*W < 2^31.  Written p, t, m; everything after the fp32 loads in double:
 *       1 n_b = valid pixels of sample b, n = sum n_b; tmin, tmax = min / max of t over the valid pixels of the whole batch;
 *         tn = (t - tmin) / (tmax - tmin + 1e-6)  (normalize_01_depth, loss.py:56-58);
 *       2 per sample, for tn and for p separately: shift = the lower median over the sample's valid pixels (sorted position
 *         (n_b - 1) / 2, torch.median; tn is increasing in t, so it is the normalised median of the raw t), scale = mean |x - shift|,
 *         a scale of exactly 0 becomes 1;  st = (tn - shift_t) / scale_t,  sp = (p - shift_p) / scale_p  (loss.py:6-43);
 *       3 abs_dev = sum over valid pixels of |sp - st| / n  (loss.py:211-213);
 *       4 trimmed_mae (loss.py:62-122, 201-203): per sample e = |sp - st| on its valid pixels, trim_b = (int64)((double)n_b * 0.1)
 *         (Python's int(n * 0.1), computed on the device); trim_b == 0 (n_b < 10): the sample contributes nothing, the reference's
 *         loss[:-0] being empty (a quirk, kept); otherwise the sum of its k_b = n_b - trim_b smallest e, and k_b pixels;
 *         trimmed_mae = sum_b sum_b / sum_b k_b, 0 / 0 = NaN.  The k_b smallest of the double values: sum(e < tau) +
 *         (k_b - count(e < tau)) * tau with tau the e of rank k_b - 1 (which of several equal values is kept does not matter);
 *       5 gradient_reg (gradient_regulizer, loss.py:125-165) on T = tn with 0 at invalid pixels, P = sp (read at EVERY pixel, as
 *         the reference does), M = m, for four levels: R = P - T; term(y,x) = |R(y,x) - R(y,x+1)| + |R(y,x) - R(y+1,x)| for
 *         y < h-1, x < w-1, summed where M(y+1,x+1) is set (the reference's shifted mask, kept; selected, not multiplied: a NaN
 *         behind a cleared bit does not enter); then T = 2x2 stride-2 max pool (floor sizes), M = M at the arg-max of T (the first
 *         maximum in row-major window order, a NaN wins: max_pool2d(return_indices=True), as nnd_pool_abs restates it), P = 2x2
 *         stride-2 mean over all four pixels.  gradient_reg = the sum over the four levels / n;
 *       6 loss = trimmed_coef * trimmed_mae + gradient_coef * gradient_reg.
 *     out (device, 6 doubles) = loss, trimmed_mae, gradient_reg, abs_dev, n, sum_b k_b.
 *     Where this departs from the reference:  (a) the reference pools a fifth time and raises when H // 16 == 0 or W // 16 == 0:
 *     H < 16 or W < 16 is refused here, before anything is launched;  (b) the reference raises on a batch without any valid pixel
 *     (min() of an empty tensor); the device cannot raise without a synchronisation: out = NaN for the four values, 0 for both
 *     counts;  (c) as in the reference, ONE sample without a valid pixel is no error: its median and scale are NaN, every use of them
 *     is masked, it contributes nothing.
 *     `workspace` = nnd_midas_loss_workspace_bytes(B, H, W) device bytes (8-byte aligned; a little over 1.3 doubles per pixel: e, and
 *     the three pooled levels of T, P, M), checked against workspace_bytes.  Nine small launches on `stream`, no allocation, no host
 *     synchronisation, no floating-point atomics: the same bits run to run, whatever workspace and out held before.  Non-finite
 *     inputs inside the mask are outside the contract.
 * nnd_midas_loss_accumulate : the validation loop's lists  nndepth/models/midas/trainer.py:341-350 as running sums:
 *     sums[i] += values[i] for i < 6, count[0] += 1 (all device doubles); a NaN propagates as np.mean over those lists does.      */
int64_t nnd_midas_loss_workspace_bytes(int B, int H, int W);
int nnd_midas_loss(const float* pred, const float* target, const unsigned char* valid_mask, int B, int H, int W, int64_t pred_stride_b,
                   int64_t pred_stride_row, double trimmed_coef, double gradient_coef, void* workspace, int64_t workspace_bytes,
                   double* out, void* stream);
int nnd_midas_loss_accumulate(const double* values, double* sums, double* count, void* stream);

/* ------------------------------------------------------------- stereo evaluation of a whole forward on the device (additions within 104)
 * nnd_stereo_eval : EvalCriterion.__call__  nndepth/models/raft_stereo/scripts/evaluate.py:48-83 (likewise igev_stereo/ and
 *     cre_stereo/scripts/evaluate.py) for EVERY output of a forward in one call, with the per-output term and the value of the
 *     sequence loss, RAFTLoss / CREStereoLoss  nndepth/models/raft_stereo/loss.py:15-52, cre_stereo/loss.py.
 *     Ground truth (B,Cg,H,W) fp32, contiguous.  Output i: (B,C_i,h_i,w_i) fp32 read through its own batch / channel / row strides
 *     (in elements, >= 0; the innermost stride is 1), so a cropped view or a slice of a stacked tensor is read where it lies.
 *     Cg == C_i, or Cg == 1: the one channel then serves every output channel, which is what the reference's broadcasting does
 *     when cre_stereo/scripts/evaluate.py:144-151 hands it the 2-channel up_disp and a 1-channel ground truth (a quirk, kept).
 *     Per output, every fp32 step as the reference takes it, everything after the per-pixel values in double:
 *       g     = the ground truth at the output's size: itself at equal size; otherwise s = W // w_i (0: refused) and
 *               g = -max_pool2d(-gt, s) / (float)s read through the source pixel F.interpolate(., size=(h_i,w_i)) (nearest) picks
 *               (evaluate.py:63-66, loss.py:23-26), computed on the fly, never written;
 *       epe   = sqrtf(sum_c (p_c - g_c)^2), valid = sqrtf(sum_{c<Cg} g_c^2) < max_flow, and mask != 0 where a mask is given
 *               (bytes, (B,mask_h,mask_w); every output of the call must then have that size);
 *       columns (K = 3 + n_above + n_below doubles):  epe = mean of epe over valid pixels (none: NaN);  count = valid pixels;
 *               l1 = sum of valid * |p_c - g_c| over all B*C_i*h_i*w_i elements / that number (loss.py:30-33);
 *               above[k]: fraction of valid pixels with epe > above[k] (evaluate.py:82);  below[k]: with epe < below[k]
 *               (loss.py:47-50); both strict, fp32 against fp32; a fraction is (double)count_k / (double)count.
 *     out (device, N*K + 1 doubles) = the N rows, then sum_i gamma^(N-1-i) * l1_i added in output order (loss.py:20-33).
 *     Outputs of one (C,h,w) share one launch, one more launch reduces everything: the number of launches is 1 + the number of
 *     distinct sizes.  `workspace` = nnd_stereo_eval_workspace_bytes(num_outputs) device bytes, 8-byte aligned, checked against
 *     workspace_bytes.  Integer counts, partial sums added in index order, no floating-point atomics: the same bits run to run,
 *     and a row does not depend on the other outputs of the call.  Every argument check answers before anything is launched.
 * nnd_stereo_eval_accumulate : sums[j] += metrics[j], j < n (device doubles): the per-pair lists of evaluate.py:141-169 as
 *     running sums; NaN propagates as np.mean over those lists does.
 * nnd_min_pool_nearest : dst (B,C,h,w) = F.interpolate(-F.max_pool2d(-gt, s) / s, size=(h,w)), s = W // w: the three lines of
 *     evaluate.py:63-66 as a map of their own (nnd_stereo_eval's g, bit for bit).                                               */
#define NND_STEREO_EVAL_MAX_OUTPUTS 64
#define NND_STEREO_EVAL_MAX_THRESHOLDS 8
typedef struct nnd_stereo_eval_output {
    const float* data;
    int32_t C, h, w;
    int32_t reserved;                       /* 0 */
    int64_t stride_b, stride_c, stride_row; /* in elements */
} nnd_stereo_eval_output;
typedef struct nnd_stereo_eval_desc {
    int32_t struct_size; /* sizeof(nnd_stereo_eval_desc) */
    int32_t flags;       /* 0 */
    const float* gt;     /* (B,Cg,H,W) */
    int32_t B, Cg, H, W;
    const unsigned char* mask; /* (B,mask_h,mask_w) bytes, or NULL: every pixel */
    int32_t mask_h, mask_w;
    double gamma;   /* the sequence loss's weight base, as the reference's Python float */
    float max_flow; /* compared as fp32, like the thresholds */
    int32_t n_above;
    float above[NND_STEREO_EVAL_MAX_THRESHOLDS];
    int32_t n_below;
    float below[NND_STEREO_EVAL_MAX_THRESHOLDS];
    int32_t num_outputs;
    nnd_stereo_eval_output outputs[NND_STEREO_EVAL_MAX_OUTPUTS];
} nnd_stereo_eval_desc;
int64_t nnd_stereo_eval_workspace_bytes(int num_outputs);
int nnd_stereo_eval(const nnd_stereo_eval_desc* desc, void* workspace, int64_t workspace_bytes, double* out, void* stream);
int nnd_stereo_eval_accumulate(const double* metrics, int n, double* sums, void* stream);
int nnd_min_pool_nearest(const float* gt, float* dst, int B, int C, int H, int W, int h, int w, void* stream);

/* ------------------------------------------------------------- scene types on the device (additions within 104)
 * Disparity / Depth / Frame of nndepth/scene: get_view (disparity.py:187-233, depth.py:166-216) and resize
 * (disparity.py:9-75,113-185, depth.py:9-63,85-146, frame.py:47-99).  Masks are bytes (torch.bool or torch.uint8) of the map's shape.
 * `kind`: 0 = disparity (v = |data|, 0 where mask == 1), 1 = depth (v = data, the minimum over mask == 1 where mask != 1).
 * nnd_view_range   : range[b] = {min, max} of v over all channels of batch element b (depth: over its valid pixels, which is the
 *     range of the filled map and, in range[b][0], the fill value).  `workspace` = nnd_view_range_workspace_bytes(B) device bytes,
 *     `range` = 2 * B device floats.  Deterministic two-pass reduction.
 * nnd_colorize     : out (B,H,W,3) uint8 = table[idx(channel 0)], the closed form of matplotlib's Normalize(clip=True) + Colormap:
 *     lo = has_lo ? lo : range[b][0], hi likewise; x = clip((double)v, lo, hi); n = lo == hi ? 0 : (x - lo) / (hi - lo);
 *     reverse: n = 1 - n; t = n * N; idx = t == N ? N - 1 : (int)t, clamped into the table.  `table` = N * 3 device bytes,
 *     2 <= N <= 4096.  `range` may be NULL when both bounds are given and no depth mask needs the fill value.  Both bounds given
 *     with lo > hi is refused.  Non-finite values in the map are outside the contract: they get some colour of the table.
 * nnd_pool_abs     : dst (B,C,H/kh,W/kw) = max (is_min: min) of |src| over non-overlapping kh x kw windows (the ragged edge is
 *     dropped), negated if `negate`, then (x * mul) / div if `rescale` (data * W_new / W_old).  `indices` (optional, int64): the
 *     plane-local offset y * W + x of the first extreme in row-major window order; a NaN wins (max_pool2d).  `mask` / `mask_out`
 *     (optional, together): mask_out[b,c,i] = mask[indices[b,c,i]] counted from the start of the whole mask — every plane reads
 *     plane 0, as the reference's flatten()[indices.flatten()] does.  `finite_out` (optional): isfinite(dst) as bytes.
 * nnd_resize_bilinear : F.interpolate(src (planes,h,w), (H,W), mode="bilinear", align_corners) with the tap arithmetic of
 *     nnd_resize_normalize; src float, or bytes if src_is_u8.  Optional outputs, at least one: dst (float; (x * mul) / div first
 *     if `rescale`), u8_out (u8_mode 1: x != 0; 2: the C cast of torch's .type(torch.uint8)), finite_out (isfinite(x)).
 * nnd_depth_inverse   : dst = clamp(1 / (src + eps)): max first, then min, each only if has_*; a NaN stays.                    */
int64_t nnd_view_range_workspace_bytes(int B);
int nnd_view_range(const float* data, const unsigned char* mask, int kind, int B, int C, int H, int W, void* workspace, float* range,
                   void* stream);
int nnd_colorize(const float* data, const unsigned char* mask, int kind, int B, int C, int H, int W, const float* range, int has_lo,
                 double lo, int has_hi, double hi, int reverse, const unsigned char* table, int N, unsigned char* out, void* stream);
int nnd_pool_abs(const float* src, float* dst, int64_t* indices, const unsigned char* mask, unsigned char* mask_out,
                 unsigned char* finite_out, int B, int C, int H, int W, int kh, int kw, int is_min, int negate, int rescale, float mul,
                 float div, void* stream);
int nnd_resize_bilinear(const void* src, int src_is_u8, float* dst, unsigned char* u8_out, int u8_mode, unsigned char* finite_out,
                        int planes, int h, int w, int H, int W, int align_corners, int rescale, float mul, float div, void* stream);
int nnd_depth_inverse(const float* src, float* dst, int64_t n, float eps, int has_max, float clip_max, int has_min, float clip_min,
                      void* stream);

/* ------------------------------------------------------------- stereo geometry on the device (additions within 105)
 * What a caller does with a disparity map next: metric depth, 3-D points, a left-right occlusion mask (csrc/geometry.hip).  The
 * reference stores the fields this consumes — Disparity.baseline (nndepth/scene/disparity.py:79-108), Camera.intrinsic
 * (nndepth/scene/camera.py:5-8), Disparity.occlusion (filled from ground truth only, kitti_stereo_2015.py:188-194: 1 = no valid
 * disparity) — and has one conversion of this kind, TartanAir's disparity = -BASELINE * FX / (depth + 1e-8)
 * (nndepth/data/datasets/tartanair_dataset.py:30,239-241).
 * Maps are (B,1,H,W) fp32 with dense rows; `*_bstride` = floats between batch elements (H*W when contiguous; a channel slice of a
 * (B,2,H,W) tensor has 2*H*W).  Outputs are contiguous.  Masks are bytes (B,H,W), non-zero = set.  `cam` = device floats
 * {fx, fy, cx, cy} per batch element, cam_stride floats apart (0: one camera for the whole batch).  `negative` != 0: the map's
 * sign convention is "negative" (m = -d), else m = d.  Every launch on `stream`; no allocation, no synchronisation.
 * nnd_disparity_to_depth : z = (float)((double)fx * baseline / (double)m); valid = mask_in (NULL: set) && isfinite(m) &&
 *     m > min_disp && (!has_max || z <= max_depth); depth = valid ? z : 0; valid_out = valid (0 / 1).
 * nnd_depth_to_disparity : the TartanAir line in its fp32 order: c = (float)(-baseline * (double)fx); d = c / (depth +
 *     (float)eps), both fp32; "positive" (negative == 0): d = -d.
 * nnd_depth_to_points    : points (B,3,H,W): X = (float)(((double)u - cx) * Z / fx), Y = (float)(((double)v - cy) * Z / fy), Z
 *     copied; u = column, v = row; all three 0 where `valid` (optional) is 0.
 * nnd_points_compact     : the same points for the valid pixels only, as rows {X, Y, Z} of `points` (B*H*W rows of 3 floats,
 *     worst case): sample b's valid pixels in row-major order are rows offsets[b] .. offsets[b+1] (offsets: B+1 int64; rows past
 *     offsets[B] are not written).  `features` (optional, (B,C,H,W) contiguous, with `feats_out` (B*H*W rows of C floats)) is
 *     gathered into the same rows.  Three launches — per-workgroup counts (wave ballot + popcount), one exclusive scan of
 *     the counts, the writes — in integer arithmetic: no atomics, no workgroup waits on another, the same bytes every run.
 *     `workspace` = nnd_points_compact_workspace_bytes(B,H,W) device bytes, 8-byte aligned.
 * nnd_lr_consistency     : occluded (B,H,W) bytes, 1 = occluded / inconsistent (the polarity of the KITTI mask).  Per pixel, each
 *     step one rounded fp32 operation: mL = +-dL; !isfinite(mL) || mL < 0 -> 1; xr = (float)x - mL; xr < 0 || xr > W-1 -> 1;
 *     i0 = floor(xr), i1 = min(i0+1, W-1), f = xr - i0; s = mR(i0) * (1 - f) + mR(i1) * f (mul, mul, add); err = |mL - s|;
 *     occluded = !(err <= threshold).  right_flipped: disp_right is stored mirrored in W, mR(i) reads column W-1-i.  `err_out`
 *     (optional, (B,H,W) floats): err, +inf where an earlier test decided.
 * nnd_pair_both_views    : frames1 (2B,C,H,W) = [left ; flipW(right)], frames2 = [right ; flipW(left)] in one launch: the second
 *     half is a rectified pair whose "left" disparity is the right view's, mirrored.                                          */
int nnd_disparity_to_depth(const float* disp, int64_t disp_bstride, const unsigned char* mask_in, const float* cam, int cam_stride,
                           double baseline, int negative, float min_disp, int has_max, float max_depth, float* depth,
                           unsigned char* valid_out, int B, int H, int W, void* stream);
int nnd_depth_to_disparity(const float* depth, int64_t depth_bstride, const float* cam, int cam_stride, double baseline, int negative,
                           double eps, float* disp, int B, int H, int W, void* stream);
int nnd_depth_to_points(const float* depth, int64_t depth_bstride, const unsigned char* valid, const float* cam, int cam_stride,
                        float* points, int B, int H, int W, void* stream);
int64_t nnd_points_compact_workspace_bytes(int B, int H, int W);
int nnd_points_compact(const float* depth, int64_t depth_bstride, const unsigned char* valid, const float* cam, int cam_stride,
                       const float* features, int C, float* points, float* feats_out, int64_t* offsets, void* workspace,
                       int64_t workspace_bytes, int B, int H, int W, void* stream);
int nnd_lr_consistency(const float* disp_left, int64_t left_bstride, const float* disp_right, int64_t right_bstride, int left_negative,
                       int right_negative, int right_flipped, float threshold, unsigned char* occluded, float* err_out, int B, int H,
                       int W, void* stream);
int nnd_pair_both_views(const float* left, const float* right, float* frames1, float* frames2, int B, int C, int H, int W,
                        void* stream);

/* ------------------------------------------------------------- connected regions and the speckle filter (additions within 105)
 * The step after the left-right check: small connected patches whose values hang together but do not belong to the surface around
 * them are removed on the device (csrc/speckle.hip).  Beyond the reference, which has no such step; the shape of OpenCV's
 * filterSpeckles, on fp32 with a mask (no parity with it is claimed).  Maps, strides and masks as above; per sample:
 *   valid[p]   = (mask == NULL || (mask[p] != 0) == (mask_valid_is_one != 0)) && isfinite(d[p])
 *                (mask_valid_is_one == 0: the mask is an occlusion mask, 1 = invalid; != 0: a valid mask, 1 = valid)
 *   p ~ q      for neighbours p, q: both valid && fabsf(d[p] - d[q]) <= max_diff, ONE rounded fp32 subtraction (so a difference
 *                equal to max_diff joins, -0.0 joins 0.0, and with max_diff = +inf an overflowing difference joins too).
 *                Neighbours: left / right / up / down (connectivity 4), and the four diagonals as well (8); a diagonal edge
 *                depends on its own two pixels only.
 *   regions    = the connected components of that graph (the relation is not transitive in value: a ramp of step max_diff is one).
 *   labels[p]  = the smallest row-major index y*W + x of p's region; -1 where !valid[p]
 *   sizes[p]   = the number of pixels of p's region; 0 where !valid[p]
 *   speckle[p] = valid[p] && sizes[p] <= max_size
 *   filtered[p] = speckle[p] ? fill : d[p]     (every other pixel copied bit for bit, invalid ones and NaNs included)
 *   mask_out[p] = in the polarity of mask_valid_is_one: invalid = !valid[p] || speckle[p]  (0: 1 = invalid; != 0: 1 = valid).  A
 *                non-finite pixel counts as invalid here, as it does in valid[p].
 *   speckle_out[p] = speckle[p] (0 / 1)
 * nnd_connected_regions writes labels and / or sizes ((B,H,W) int32, either may be NULL, not both); nnd_speckle_filter is
 * regions + apply in one enqueue: filtered, mask_out, speckle_out (one of them at least) and sizes are optional.  Both enqueue the
 * same four launches whatever the data: the call neither synchronises nor reads anything back, and can be captured into a graph.
 * Only integer atomics (min, add): the same bytes on every run; nothing depends on what the workspace or the outputs held.
 * `workspace` = nnd_connected_regions_workspace_bytes(B,H,W) device bytes (9 per pixel, rounded up), 8-byte aligned, the
 * caller's.  Refused before any HIP call: a null map / workspace / no output, B, H, W out of range (1 <= B <= 65535,
 * H*W < 2^31), a batch stride below H*W, max_diff negative or NaN, connectivity other than 4 or 8, max_size < 0, a workspace too
 * small or misaligned.  nnd_connected_regions_tile: height (which = 0) / width (1) of the tile one workgroup labels in LDS.      */
int64_t nnd_connected_regions_workspace_bytes(int B, int H, int W);
int nnd_connected_regions_tile(int which);
int nnd_connected_regions(const float* map, int64_t map_bstride, const unsigned char* mask, int mask_valid_is_one, float max_diff,
                          int connectivity, int32_t* labels, int32_t* sizes, void* workspace, int64_t workspace_bytes, int B, int H,
                          int W, void* stream);
int nnd_speckle_filter(const float* map, int64_t map_bstride, const unsigned char* mask, int mask_valid_is_one, float max_diff,
                       int connectivity, int max_size, float fill, float* filtered, unsigned char* mask_out,
                       unsigned char* speckle_out, int32_t* sizes, void* workspace, int64_t workspace_bytes, int B, int H, int W,
                       void* stream);

/* ------------------------------------------------------------- view warp, warp occlusion and hole filling (additions within 105)
 * What one disparity map says about the OTHER view, and a dense map from one with holes (csrc/warp.hip).  Beyond the reference,
 * which has neither step.  Maps, strides and masks as above; `negative` != 0: m = -d, else m = d.
 *
 * nnd_warp_disparity: a z-buffered forward warp along the row, nearest column.  Per sample and row y, every step one rounded fp32
 * operation:
 *   m      = (negative ? -d[y,x] : d[y,x]) + 0.0f                        (-0.0 counts as +0.0)
 *   src_ok = (mask == NULL || (mask[y,x] != 0) == (mask_valid_is_one != 0)) && isfinite(m) && m >= 0
 *   xr     = to_right ? (float)x - m : (float)x + m ;  t = rintf(xr)     (ties to even: 1.5 and 2.5 both land on column 2)
 *   lands  = src_ok && t >= 0.0f && t <= (float)(W-1)                    (xr in [-0.5, 0] lands on column 0)
 *   winner of (y,t): among the sources that land there the largest m; among equal m the smallest x
 *   a target with a winner : disp_other = negative ? -m_win : m_win, source = x_win, features_other[:,y,t] = features[:,y,x_win]
 *                            bit for bit; a target without one (a hole): disp_other = fill, source = -1, features 0
 *   valid_other[y,t] = in the polarity of mask_valid_is_one: has a winner (!= 0: 1 = has one; 0: 1 = hole)
 *   occluded[y,x]    = !(lands && (m_win(y,t) - m) <= threshold): 1 = occluded, out of frame or invalid (the polarity of
 *                      nnd_lr_consistency and of the KITTI mask)
 * to_right == 0 takes a right-view map and writes the left view.  threshold >= 0, +inf allowed (only invalid pixels and those that
 * leave the frame are occluded then).  Outputs: disp_other (B,H,W) floats, valid_other / occluded (B,H,W) bytes, source (B,H,W)
 * int32; each may be NULL, not all.  features (B,C,H,W) contiguous, features_other and C > 0 go together.  ONE launch, no
 * workspace: a workgroup per row keeps a 64-bit key per column, bits(m) << 32 | (W - x), in LDS and takes integer maxima, so the
 * result does not depend on the order of arrival and a run gives the same bytes every time.  Refused before any HIP call: a null
 * map, no output, B, H, W out of range (1 <= B <= 65535, H*W < 2^31, B*H <= 2^25), W above nnd_warp_disparity_limit(0), a batch
 * stride below H*W, a negative or NaN threshold, features without C or the other way round.
 * nnd_warp_disparity_limit: the largest width (which = 0); the columns a workgroup handles per pass (1).
 * What the occlusion is NOT: a nearest-column splat leaves one-pixel cracks in a surface that stretches in the other view, and a
 * hidden pixel behind a crack wins that column and counts as visible; it is not the definition of nnd_lr_consistency.
 *
 * nnd_fill_holes: ok[p] = mask-valid[p] && isfinite(map[p]).  rule: 0 min_abs, 1 max_abs, 2 nearest.  A value is always copied bit
 * for bit from a neighbour; nothing is interpolated.
 *   row pass, rows with an ok pixel: a pixel that is not ok has L / R, the nearest ok column to its left / right; with one of them
 *     it takes that one's value; with both, min_abs takes L if fabsf(v_L) <= fabsf(v_R) else R, max_abs L if fabsf(v_L) >=
 *     fabsf(v_R) else R, nearest L if x-L <= R-x else R.
 *   column pass (vertical != 0), rows without an ok pixel: U / D = the nearest rows above / below that have one; the pixel takes the
 *     row-pass result of U or D at its column by the same rule (U on a tie; y-U <= D-y for nearest).
 *   a sample without an ok pixel, and with vertical == 0 every empty row, keeps `fill`.
 *   filled (B,H,W) floats, required, not the input; was_filled (optional bytes): 1 where a value was copied in; mask_out (optional
 *   bytes): in the polarity of mask_valid_is_one, invalid = still without a value.  Pixels that were ok are copied bit for bit.
 * THREE launches whatever the data (the first ok column at or after every chunk of a row, from the right; the row pass, from the left,
 * and for empty rows the search for U and D; the column pass), no atomics.  `workspace` = nnd_fill_holes_workspace_bytes(B,H,W)
 * device bytes (a word per row and chunk of nnd_fill_holes_chunk() columns, two per row), 4-byte aligned, the caller's.  Refused
 * before any HIP call: a null map / workspace / filled, filled == map, B, H, W out of range, a batch stride below H*W, an unknown
 * rule, a workspace too small or misaligned.                                                                                    */
int nnd_warp_disparity_limit(int which);
int nnd_warp_disparity(const float* disp, int64_t disp_bstride, const unsigned char* mask, int mask_valid_is_one, int negative,
                       int to_right, float threshold, float fill, const float* features, int C, float* disp_other,
                       unsigned char* valid_other, unsigned char* occluded, int32_t* source, float* features_other, int B, int H, int W,
                       void* stream);
int nnd_fill_holes_chunk(void);
int64_t nnd_fill_holes_workspace_bytes(int B, int H, int W);
int nnd_fill_holes(const float* map, int64_t map_bstride, const unsigned char* mask, int mask_valid_is_one, int rule, int vertical,
                   float fill, float* filled, unsigned char* was_filled, unsigned char* mask_out, void* workspace,
                   int64_t workspace_bytes, int B, int H, int W, void* stream);

/* ------------------------------------------------------------- masked median and guided weighted median (additions within 105)
 * The edge-preserving step that ends the clean-up chain (csrc/median.hip): a (2r+1) x (2r+1) median over the ok pixels, or a
 * weighted median whose weights come from a picture.  Beyond the reference, which has no such step.  A SELECTION: every output is
 * a copy of input bits.
 * Inputs: map (B,1,H,W) fp32, its batch stride read where it lies; mask: optional bytes, polarity mask_valid_is_one as in
 * nnd_speckle_filter and nnd_fill_holes; radius r; min_count; fill_invalid; fill.  Guide, optional: guide (B,C,H,W) fp32,
 * contiguous, 1 <= C <= 4; inv_step finite and > 0; weights: 256 uint16_t in HOST memory, copied into the launch's arguments: no
 * device table, no host synchronisation, and the call can be captured into a graph.
 *   1  ok[q] = mask-valid[q] && isfinite(map[q]).
 *   2  The window of p = (y,x): the in-frame q with |qy-y| <= r and |qx-x| <= r.  Clipped at the border, no padding.
 *   3  Order on values: key(v) = bits(v) ^ (sign ? 0xFFFFFFFF : 0x80000000), compared as unsigned: -0.0 < +0.0, and denormals are
 *      ordinary values.
 *   4  Tap weight w(p,q): without a guide 1.  With a guide, every step one rounded fp32 operation:
 *        dist = |g0[p]-g0[q]|, then + |g1[p]-g1[q]|, and so on in channel order;  s = dist * inv_step;
 *        b = (s < 255.0f) ? (int)s : 255   (a NaN from a non-finite guide value gives 255);  w = weights[b].
 *   5  Over the ok taps of the window: n their count, T = sum of w, S(v) = sum of w over the ok taps with key <= key(v).  The
 *      weighted lower median v* is the tap value of smallest key with 2 S(v*) >= T; all of it integer arithmetic.  With unit
 *      weights v* is the element of rank (n-1)/2.
 *   6  produced[p] = (ok[p] || fill_invalid) && n >= min_count && T > 0.
 *   7  filtered[p] = v* bit for bit if produced[p]; else map[p] bit for bit if ok[p]; else fill.
 *   8  mask_out[p] (optional bytes), in the polarity of the input mask: valid = ok[p] || produced[p].
 *   9  changed[p] (optional bytes) = 1 where the output bits differ from the input bits, or where a pixel that was not ok got a
 *      value.
 * ONE launch, no workspace, no atomics, the same bytes on every run; nothing depends on what the outputs held before.  Refused
 * before any HIP call: a null map or filtered, filtered == map, B, H, W out of range (as nnd_fill_holes), a batch stride below
 * H*W, a radius outside 1 .. nnd_median_filter_limit(0), min_count outside 1 .. (2r+1)^2, guide, C and weights not given
 * together, C outside 1 .. 4, inv_step not finite or <= 0, weights[0] == 0 (the centre tap must count, or an ok pixel could have
 * T = 0).
 * nnd_median_filter_limit: the largest radius (which = 0; >= 7), the height (1) and width (2) of the output tile of one
 * workgroup; anything else: < 0.                                                                                               */
int nnd_median_filter_limit(int which);
int nnd_median_filter(const float* map, int64_t map_bstride, const unsigned char* mask, int mask_valid_is_one, int radius,
                      int min_count, int fill_invalid, float fill, const float* guide, int C, float inv_step,
                      const uint16_t* weights, float* filtered, unsigned char* mask_out, unsigned char* changed, int B, int H, int W,
                      void* stream);

/* ------------------------------------------------------------- view synthesis and photometric error (additions within 105)
 * The map held against the PICTURES (csrc/photometric.hip): the other picture sampled back into this view by the disparity, the
 * L1 + SSIM error of that reconstruction in the Monodepth form, and its per-sample sums over the pixels that can be trusted.
 * Beyond the reference, whose inference scripts have no such step.
 * Inputs: target, other (B,C,H,W) fp32, contiguous, 1 <= C <= nnd_photometric_limit(0); disp (B,1,H,W) fp32, its batch stride read
 * where it lies; mask: optional bytes, polarity mask_valid_is_one as in nnd_median_filter; negative != 0: m = -d, else m = d;
 * target_is_left != 0: disp belongs to the left picture and `other` is the right one, else the other way round.  H, W >= 2.
 * Per sample, row y, column x, every numbered step one rounded fp32 operation unless it says double:
 *   1  m = (negative ? -d : d) + 0.0f;  src_ok = mask-valid && isfinite(m) && m >= 0.
 *   2  xr = target_is_left ? (float)x - m : (float)x + m;  in = src_ok && xr >= 0 && xr <= (float)(W-1).
 *   3  fl = floorf(xr), i0 = (int)fl, i1 = min(i0+1, W-1), f = xr - fl.  Per channel rec_c = other_c[y,i0] * (1.0f - f) +
 *      other_c[y,i1] * f, computed as mul, mul, add (the sequence of nnd_lr_consistency).  nnd_synthesize_view writes
 *      recon = in ? rec_c : fill and valid_out = in, and stops here.
 *   4  The window is 3 x 3 with reflected borders: index -1 reads 1, index H reads H-2, likewise in W.  box(v) at (y,x) takes row
 *      sums first: r(y') = (v(y',x-1) + v(y',x)) + v(y',x+1), then box = (r(y-1) + r(y)) + r(y+1).
 *   5  Per channel, with inv9 = (float)(1.0/9.0) and t the target picture: mx = box(t)*inv9, my = box(rec)*inv9,
 *      sx = box(t*t)*inv9 - mx*mx, sy = box(rec*rec)*inv9 - my*my, sxy = box(t*rec)*inv9 - mx*my,
 *      n = ((2*mx)*my + c1) * (2*sxy + c2), dn = ((mx*mx + my*my) + c1) * ((sx + sy) + c2),
 *      ds_c = clamp((1.0f - n/dn) * 0.5f, 0, 1): for every number the bits of fminf(fmaxf(v, 0), 1); a NaN stays a NaN, as in
 *      torch.clamp, so that a non-finite picture value makes every window that holds it not valid.  `/` is the correctly rounded
 *      fp32 division.
 *   6  l1_c = fabsf(t_c - rec_c) * inv_range.
 *   7  ds and l1 are the sums over the channels in channel order, times 1.0f / (float)C.
 *   8  e = ssim_weight * ds + (1.0f - ssim_weight) * l1, computed as mul, mul, add.  With ssim_weight == 0: e = l1, ds is not
 *      computed, dssim_out is `fill` everywhere and the sum of ds in `stats` is 0.
 *   9  With ssim_weight > 0: valid = `in` at all nine reflected taps && isfinite(e); with ssim_weight == 0 only the centre tap
 *      counts.  Where not valid, error, l1_out and dssim_out are `fill`.  A reconstruction at a tap that is not `in` is never used.
 *  10  stats[b] = { count of valid pixels, sum e, sum l1, sum ds } over the valid pixels of sample b: every fp32 value converted to
 *      double and added in double, in a fixed order; the count is exact.
 * Outputs of nnd_photometric_error: error (B,H,W) floats, required; optional: l1_out, dssim_out (B,H,W) floats, valid_out (B,H,W)
 * bytes in the polarity of the mask (mask_valid_is_one), stats (B x 4 doubles on the device).  nnd_synthesize_view: recon
 * (B,C,H,W), required; valid_out optional.  `workspace` (needed only with stats) = nnd_photometric_workspace_bytes(B,H,W) device
 * bytes, 8-byte aligned, the caller's: four doubles per workgroup.
 * nnd_synthesize_view is ONE launch without a workspace.  nnd_photometric_error is ONE launch that writes the maps and a partial
 * per workgroup into that workgroup's own slot, and with stats a second small one that adds the partials in a fixed order.  No
 * atomics, no host synchronisation, the same bytes on every run; nothing depends on what the outputs or the workspace held.
 * Refused before any HIP call: a null required pointer, error / recon aliasing an input, B, H, W out of range (1 <= B <= 65535,
 * H, W >= 2, H*W < 2^31), a batch stride below H*W, C outside 1 .. nnd_photometric_limit(0), ssim_weight outside [0, 1] or NaN,
 * c1, c2 or inv_range not finite or <= 0, stats without a workspace of the right size and alignment.
 * nnd_photometric_limit: the largest channel count (which = 0; >= 4), the height (1) and width (2) of the output tile of one
 * workgroup; anything else: < 0.  nnd_photometric_workspace_bytes: < 0 for a shape that is refused.
 * Not here: the edge-aware smoothness term, Monodepth2's identity auto-mask (a zero disparity gives the unwarped error), other
 * window sizes, gradients, 16-bit pictures.                                                                                     */
int nnd_photometric_limit(int which);
int64_t nnd_photometric_workspace_bytes(int B, int H, int W);
int nnd_synthesize_view(const float* other, const float* disp, int64_t disp_bstride, const unsigned char* mask, int mask_valid_is_one,
                        int negative, int target_is_left, float fill, float* recon, unsigned char* valid_out, int B, int C, int H,
                        int W, void* stream);
int nnd_photometric_error(const float* target, const float* other, const float* disp, int64_t disp_bstride, const unsigned char* mask,
                          int mask_valid_is_one, int negative, int target_is_left, float ssim_weight, float c1, float c2,
                          float inv_range, float fill, float* error, float* l1_out, float* dssim_out, unsigned char* valid_out,
                          double* stats, void* workspace, int64_t workspace_bytes, int B, int C, int H, int W, void* stream);

/* ------------------------------------------------------------- LoFTR layer with linear attention (CREStereo)
 * Replaces LoFTREncoderLayer.forward  nndepth/blocks/transformer.py:39-66 with LinearAttention  nndepth/blocks/attn_block.py:23-58
 * (no masks).  The reference's (N, H*W, C) tokens are the (N,C,H,W) maps transposed, so every nn.Linear is a 1x1 conv of
 * the map: x, source, out are (N, d_model, H, W); out = x + norm2(mlp([x | norm1(merge(attention(x, source)))])).
 * d_model / nhead must be 32.  nnd_loftr_pack (HOST): tensors = q_proj.weight, k_proj.weight, v_proj.weight,
 * merge.weight, mlp.0.weight, mlp.2.weight, norm1.weight, norm1.bias, norm2.weight, norm2.bias (state_dict order).      */
int64_t nnd_loftr_packed_floats(int d_model, int nhead);
int64_t nnd_loftr_workspace_floats(int d_model, int nhead, int N, int H, int W);
int nnd_loftr_pack(int d_model, int nhead, const float* const* tensors_host, float* packed_host);
int nnd_loftr_layer_forward(int d_model, int nhead, const float* packed_dev, const float* x, const float* source, float* out,
                            float* workspace, int N, int H, int W, void* stream);

/* ------------------------------------------------------------- LoFTR full (softmax) attention, opt-in (csrc/attention.hip)
 * nnd_full_attention replaces FullAttention.forward  nndepth/blocks/attn_block.py:59-97  (no masks, no dropout), head
 * dimension 32, on channel-major maps: q, out (N, nhead*32, L), k, v (N, nhead*32, S); L and S may differ:
 *   out[n, 32h+d, l] = sum_s softmax_s( (sum_d q[n,32h+d,l] k[n,32h+d,s]) / sqrt(32) ) v[n,32h+d,s]
 * Exact fp32 on the MFMA with an online softmax: the scores never reach memory; no atomics, one evaluation order, the same
 * bits run to run.  q_bs / kv_bs / out_bs are batch strides in floats (>= nhead*32*L, nhead*32*S, nhead*32*L).
 * nnd_loftr_full_layer_forward replaces LoFTREncoderLayer.forward  nndepth/blocks/transformer.py:39-66  of a layer built
 * with attention = "full" (transformer.py:9-27): nnd_loftr_layer_forward with the attention above in place of the linear
 * one; same maps, same blob (nnd_loftr_pack: FullAttention has no parameters), its own workspace size
 * nnd_loftr_full_workspace_floats = 6 * N * d_model * H * W.                                                              */
int nnd_full_attention(const float* q, const float* k, const float* v, float* out, int N, int nhead, int L, int S, int64_t q_bs,
                       int64_t kv_bs, int64_t out_bs, void* stream);
int64_t nnd_loftr_full_workspace_floats(int d_model, int nhead, int N, int H, int W);
int nnd_loftr_full_layer_forward(int d_model, int nhead, const float* packed_dev, const float* x, const float* source, float* out,
                                 float* workspace, int N, int H, int W, void* stream);

/* ------------------------------------------------------------- 3x3x3 Conv3d (IGEV cost-volume regulariser, row a15)
 * ConvBn3D / the conv of Upsampler3D:  nndepth/models/igev_stereo/cost_volume.py:101-130
 *   y = LeakyReLU_slope( BatchNorm3d_eval( conv3d(cat(x0, x1); w, stride, padding 1) + bias ) )        (norm / bias optional)
 * Volumes are DEPTH-MAJOR, (N, D+2, C, H, W) with one zero slice before and after the D real ones
 * (nnd_volume_to_depth_major / nnd_depth_major_to_volume convert from / to the usual (N, C, D, H, W)); a Conv3d is then one
 * launch of the 2-D MFMA convolution per sample over 3*C consecutive planes (csrc/conv3d.hip); the thin layers (8 / 16 output
 * channels) run on a direct VALU kernel (csrc/thin3d.hip; exact arithmetic, stride 2) or, with arithmetic = 2 at stride 1, on the
 * depth-marching 16-bit-MFMA kernel (csrc/slab3d.hip).  Cin1 = 0: single input.
 * nnd_conv3d_pack (HOST): w (Cout, Cin0+Cin1, 3, 3, 3), bias / bn_* may be NULL.  leaky_slope 1 = no activation.          */
typedef struct nnd_conv3d_desc {
    int32_t struct_size; /* sizeof(nnd_conv3d_desc) */
    int32_t Cout, Cin0, Cin1, stride;
    int32_t arithmetic; /* 0 = exact fp32 MFMA; 3 / 2 = 16-bit MFMA with 3 bf16 / 2 fp16 split operands
                           (see nnd_update_block_desc.arithmetic); 1 (one fp16 piece) is not built for Conv3d and is refused */
    int32_t flags;      /* NND_FLAG_* */
} nnd_conv3d_desc;
int64_t nnd_conv3d_packed_floats(const nnd_conv3d_desc* desc);
int nnd_conv3d_pack(const nnd_conv3d_desc* desc, const float* w_host, const float* bias_host, const float* bn_gamma,
                    const float* bn_beta, const float* bn_mean, const float* bn_var, float bn_eps, float* packed_host);
int nnd_conv3d_forward(const nnd_conv3d_desc* desc, const float* packed_dev, const float* x0, const float* x1, float* y,
                       int N, int D, int H, int W, float leaky_slope, void* stream);
/* fp16x2 calibration of the layer after forwards with NND_FLAG_CALIBRATE (as nnd_update_block_calibration_finish) */
int nnd_conv3d_calibration_finish(const nnd_conv3d_desc* desc, float* packed_dev, int32_t* status_dev, void* stream);
/* HOST: the slots of the formulations the blob packs, always 3 entries in the order nnd_conv3d_scale_name(0..2) names them — "plain"
 * (one output slice per launch element), "grouped" (J slices; thin stride-1 layers), "slab" (depth-marching kernel) — with -1 for a
 * formulation this shape does not pack or that is not fp16x2.  They all stage the layer's input: ONE activation range, which
 * nnd_scales_write should give to every one of them (the forward picks the formulation from the depth).  Contract as
 * nnd_encoder_scale_slots.                                                                                                    */
int nnd_conv3d_scale_slots(const nnd_conv3d_desc* desc, int64_t* offsets, int n);
const char* nnd_conv3d_scale_name(int which);
int nnd_volume_to_depth_major(const float* x, float* y, int N, int C, int D, int H, int W, void* stream);
int nnd_depth_major_to_volume(const float* x, float* y, int N, int C, int D, int H, int W, void* stream);
/* the same for a volume stored (N, C, H, W, D), candidate axis contiguous — level 0 of the IGEV pyramids, rows
 * (b, g, h, w1) of w2 floats (igev_stereo/cost_volume.py:40-52): the regulariser reads / writes the pyramids in place */
int nnd_volume_rows_to_depth_major(const float* x, float* y, int N, int C, int D, int H, int W, void* stream);
int nnd_depth_major_to_volume_rows(const float* x, float* y, int N, int C, int D, int H, int W, void* stream);
/* Upsampler3D's F.interpolate(scale_factor=2, mode="trilinear", align_corners=True) (cost_volume.py:128): depth-major
 * x (N,D+2,C,H,W) -> y (N,2D+2,C,2H,2W).  FeatureGuidedBlock (cost_volume.py:133-147): vol *= sigmoid(logits (N,C,H,W)),
 * broadcast over the depth slices, in place.                                                                              */
int nnd_volume_upsample2x(const float* x, float* y, int N, int C, int D, int H, int W, void* stream);
int nnd_volume_gate(float* vol, const float* logits, int N, int C, int D, int H, int W, void* stream);

/* Fused tail of the mask head + convex upsample (the (B, 9*rate^2, H, W) mask is never written):
 *   out = convex_upsample(flow, 0.25 * conv1x1(x; W, b))      x (B,Cin,H,W), flow (B,1,H,W), out (B,1,rate*H,rate*W)
 * Replaces update_block.py:97-101,111 (mask.2, x0.25) + raft_stereo/model.py:93-105.  `packed_dev` is the blob of
 * nnd_conv2d_pack for the (9*rate^2, Cin, 1, 1) weight.  Built for rate 4 / 8 and Cin 128 / 256.            */
int nnd_mask_upsample_forward(const float* packed_dev, const float* x, const float* flow, float* out,
                              int B, int Cin, int H, int W, int rate, void* stream);

/* ------------------------------------------------------------------ fused refinement loop
 * Replaces the `for _ in range(self.iters)` loop of RAFTStereo.forward
 *   nndepth/models/raft_stereo/model.py:126-137 (+ initialize_coords :87-91)
 * net/inp are the tanh/relu halves of cnet (model.py:119-122); `pyramid` comes from
 * nnd_corr1d_build.  coords start at arange(W) (+ disp_init if non-NULL).  Every iteration:
 * lookup -> update block -> coords += delta -> convex upsample of (coords - arange).
 * up_out: iteration i writes (B,1,rate*H,rate*W) at up_out + i*up_iter_stride floats
 *         (stride 0 keeps only the last, but still computes every iteration's map; desc->flags with
 *         NND_FLAG_LAST_UPSAMPLE_ONLY and stride 0 computes the last map alone — for all four
 *         nnd_*_refine entry points); low_out (optional) receives the final 1/rate-res
 *         disparity (B,1,H,W); net_out (optional) the final hidden state.
 * Only flow_channels == 1 (RAFT-Stereo / IGEV-style 1-D disparity).                       */
int nnd_raft_stereo_refine(const nnd_update_block_desc* desc, const float* packed_dev,
                           const float* pyramid, int num_levels, int radius,
                           const float* net, const float* inp, const float* disp_init,
                           float* up_out, int64_t up_iter_stride, float* low_out, float* net_out,
                           float* workspace, int B, int H, int W, int rate, int iters, void* stream);
/* One cascade stage of Coarse2FineGroupRepViTRAFTStereo.forward (nndepth/models/raft_stereo/model.py:297-311): the same loop with
 * nnd_group_corr1d_lookup over `group_pyramid` (nnd_group_corr_build_scaled); disp_init = the previous stage's up_disp (its
 * resolution is this stage's: init_coords = org_coords + up_disp, :316).  The lookup runs as its own kernel (it gathers other
 * pixels' rows, Q6), convc1 behind it; everything else as in nnd_raft_stereo_refine.                                            */
int nnd_raft_stereo_group_refine(const nnd_update_block_desc* desc, const float* packed_dev, const float* group_pyramid, int num_groups,
                                 int num_levels, int radius, const float* net, const float* inp, const float* disp_init, float* up_out,
                                 int64_t up_iter_stride, float* low_out, float* net_out, float* workspace, int B, int H, int W, int rate,
                                 int iters, void* stream);

/* IGEV variant of the loop (nndepth/models/igev_stereo/model.py:148-158): lookup = nnd_igev_lookup over both
 * pyramids, and — reference quirk Q5 — the update block and the convex upsample receive the ABSOLUTE coordinate
 * coords1 = arange(W) + disp_init + sum(delta), not the disparity.  disp_init = the soft-argmin initial disparity
 * (computed by the caller: Conv3d squeezer + softmax, PyTorch).  up_out / low_out hold coordinates accordingly.
 * interleaved: optional (may be NULL) output of nnd_igev_interleave_pyramids for the same pyramids; when given, the
 * per-iteration lookup gathers from it (same values, ~4x fewer HBM lines).  nnd_igev_refine_reads_interleaved = 1 when,
 * given that copy, the loop reads nothing else of the two pyramids (groups / radius the fused lookup is built for and the
 * fused lookup not switched off): their pooled levels may then be left unwritten.                                 */
int nnd_igev_refine_reads_interleaved(int num_groups, int num_levels, int radius);
int nnd_igev_stereo_refine(const nnd_update_block_desc* desc, const float* packed_dev,
                           const float* feat_pyramid, const float* geo_pyramid, const float* interleaved,
                           int num_groups, int num_levels, int radius,
                           const float* net, const float* inp, const float* disp_init,
                           float* up_out, int64_t up_iter_stride, float* low_out, float* net_out,
                           float* workspace, int B, int H, int W, int rate, int iters, void* stream);

/* CREStereo variant of the loop — one stage of the cascade (nndepth/models/cre_stereo/model.py:221-236, 246-259, 270-284):
 * every iteration: AGCL correlation of (fmap1, fmap2) at the current flow -> update block (flow_channels = 2) ->
 * flow += delta -> 2-channel convex upsample.  Iteration i searches a 1x9 window when i is even, 3x3 when odd.
 * `scratch` = caller-owned device buffer of `scratch_floats` floats (the size is part of the contract: the library checks it
 * and never writes past it).
 * extra_offset == NULL: iter mode (nnd_agcl_corr_iter); the scratch receives the warped right map and must hold
 * B*C*H*W floats (else NND_ERR_INVALID);
 * extra_offset (B,18,H,W): offset mode (nnd_agcl_corr_offset; fmap1/fmap2 already attended by the caller); with
 * scratch_floats >= 2*B*C*H*W and C == 256 the two maps are copied channels-last into the scratch once per call and
 * sampled line by line (nnd_agcl_corr_offset_nhwc); with a smaller / NULL scratch or C != 256: the planar kernel, same
 * results to 1e-7, slower.  flow_init (B,2,H,W) or NULL for zero.
 * up_out: iteration i writes (B,2,rate*H,rate*W) at up_out + i*up_iter_stride; low_out (optional) the final flow (B,2,H,W); net_out (optional) the hidden state.   */
int nnd_cre_stereo_refine(const nnd_update_block_desc* desc, const float* packed_dev,
                          const float* fmap1, const float* fmap2, int C, const float* extra_offset,
                          float* scratch, int64_t scratch_floats, const float* net, const float* inp, const float* flow_init,
                          float* up_out, int64_t up_iter_stride, float* low_out, float* net_out,
                          float* workspace, int B, int H, int W, int rate, int iters, void* stream);

/* ------------------------------------------------------------------------------ profiling
 * Times `reps` back-to-back launches of ONE hot-path conv (selected by `which`, see
 * nnd_conv_name) on `stream` with hipEvents recorded on that same stream and returns the
 * average milliseconds per launch in *ms_out and its algorithmic FLOPs in *flops_out.
 * Used by bench.py for the roofline object; inputs are whatever the workspace holds.      */
int nnd_profile_conv(const nnd_update_block_desc* desc, const float* packed_dev, float* workspace,
                     int B, int H, int W, int which, int reps, void* stream,
                     float* ms_out, double* flops_out);
/* The same conv timed where it runs in production: inside the fused RAFT-Stereo loop (arguments as
 * nnd_raft_stereo_refine, only the last up_disp is kept), bracketed by hipEvents on `stream` in every iteration.  *ms_out = average over iterations 2..iters (event-to-event, so it
 * includes the launch gap in front of the kernel).  Synchronises `stream`.  `which` must be one of the stand-alone
 * launches of the loop (not convc1 / mask.2, which are fused into their neighbours).                    */
int nnd_profile_loop_conv(const nnd_update_block_desc* desc, const float* packed_dev, const float* pyramid,
                          int num_levels, int radius, const float* net, const float* inp, float* up_out,
                          float* workspace, int B, int H, int W, int rate, int iters, int which, void* stream,
                          float* ms_out);
/* Calibration of the above: the same loop with BOTH events of every iteration recorded in front of conv `which`, nothing
 * between them.  *ms_out = what an event pair alone measures at that place of the stream (the part of nnd_profile_loop_conv's
 * figure that is not the launch): bench.py reports it beside the raw figure.                                         */
int nnd_profile_loop_event_pair(const nnd_update_block_desc* desc, const float* packed_dev, const float* pyramid,
                                int num_levels, int radius, const float* net, const float* inp, float* up_out,
                                float* workspace, int B, int H, int W, int rate, int iters, int which, void* stream,
                                float* ms_out);
/* Diagnostic: sustained fp32-MFMA rate of this device (dependent v_mfma_f32_32x32x2 chains, no memory
 * traffic) at `waves_per_simd` resident waves; `scratch_dev` is any device buffer of >= 1 float.        */
int nnd_profile_mfma_peak(int waves_per_simd, int iters, void* stream, float* scratch_dev, float* tflops_out);
/* Diagnostic: the same for the 16-bit MFMA of the split arithmetics (v_mfma_f32_32x32x16_f16, or _bf16 with bf16 != 0): 4 independent
 * chains per wave on pseudo-random operands, about `target_ms` of nothing else — the rate the chip SUSTAINS under its power limit on
 * this box and the shader clock it settles at (nominal: 2500 TFLOP/s at 2.4 GHz).  clk_dev: device buffer of >= 512 64-bit words. */
int nnd_profile_mfma16_peak(int bf16, int waves_per_simd, float target_ms, void* stream, float* scratch_dev,
                            unsigned long long* clk_dev, float* tflops_out, float* ghz_out);
/* nnd_num_convs: the loop's launches, `which` of the profiling calls.  nnd_conv_name names those and, behind them, the other
 * convolutions that nnd_update_block_scale_slots lists (the single-call GRU convs, the per-pair context terms); "" beyond. */
int nnd_num_convs(const nnd_update_block_desc* desc);
const char* nnd_conv_name(const nnd_update_block_desc* desc, int which);

#ifdef __cplusplus
}
#endif
#endif /* NNDEPTH_AMD_H */
