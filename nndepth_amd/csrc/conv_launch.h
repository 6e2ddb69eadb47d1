// Host side shared by the two convolution launchers (conv_mfma.hip launch_conv, conv_split.hip launch_conv_split): the checks and the
// ConvArgs fields that depend on neither the kernel nor its tile configuration, and the ConvIO::cout_need restriction of a picked one.
#pragma once
#include "common.h"
#include "conv_epilogue.h"
#include "layout.h"

#include <cstring>

namespace nnd {

// `who`: the message prefix ("conv", "conv_split").  *Hin, *Win: the input size (stride 2: the caller passes it in io)
inline int conv_check_io(const char* who, const ConvLayer& L, const ConvIO& io, int epi, int H, int W, int* Hin, int* Win) {
    NND_REQUIRE(io.src0.C + io.src1.C == L.Cin, "%s: source channels %d+%d != Cin %d", who, io.src0.C, io.src1.C, L.Cin);
    NND_REQUIRE(L.stride == 1 || L.stride == 2, "%s: stride %d not supported", who, L.stride);
    *Hin = io.Hin > 0 ? io.Hin : H, *Win = io.Win > 0 ? io.Win : W;
    NND_REQUIRE(H == (*Hin + L.stride - 1) / L.stride && W == (*Win + L.stride - 1) / L.stride,
                "%s: output %dx%d does not match input %dx%d at stride %d", who, H, W, *Hin, *Win, L.stride);
    NND_REQUIRE(!io.src_c4 || (io.src_tiled && io.src0.C % 4 == 0 && io.src1.C % 4 == 0), "%s: c4 sources need channel counts %% 4 == 0", who);
    NND_REQUIRE(!io.dst_c4 || (io.dst_tiled && (L.Cout % 4 == 0 || (!io.bmap.ptr && !io.aux0.ptr && !io.aux1.ptr && !io.out1.ptr))),
                "%s: c4 destination with per-pixel operands needs Cout %% 4 == 0", who);
    NND_REQUIRE(epi != EPI_AFFINE || L.s_off >= 0, "%s: EPI_AFFINE needs a packed scale vector", who);
    return NND_OK;
}

// every ConvArgs field but the plan's (tiles_x, wco, ks, npos, ngroups; dbg_stamp in stamp builds)
inline void conv_fill_args(const ConvLayer& L, const float* blob, const ConvIO& io, int epi, int H, int W, int Hin, int Win, ConvArgs* out) {
    ConvArgs& a = *out;
    memset(&a, 0, sizeof(a));
    a.src0 = io.src0.ptr; a.bs0 = io.src0.bstride; a.c0 = io.src0.C;
    a.src1 = io.src1.ptr; a.bs1 = io.src1.bstride; a.c1 = io.src1.C;
    a.wpk = blob + L.w_off; a.bias = blob + L.b_off;
    a.out0 = io.out0.ptr; a.obs0 = io.out0.bstride;
    a.out1 = io.out1.ptr; a.obs1 = io.out1.bstride;
    a.aux0 = io.aux0.ptr; a.abs0 = io.aux0.bstride;
    a.aux1 = io.aux1.ptr; a.abs1 = io.aux1.bstride;
    a.bmap = io.bmap.ptr; a.bmbs = io.bmap.bstride;
    a.ls = make_lay(Hin, Win, io.src_tiled, io.src_c4);
    a.ld = make_lay(H, W, io.dst_tiled, io.dst_c4);
    a.H = H; a.W = W; a.Hin = Hin; a.Win = Win; a.Cout = L.Cout; a.nchunks = L.nchunks; a.epi = epi; a.hidden = io.hidden; a.flags = io.flags;
    a.cscale = L.s_off >= 0 ? blob + L.s_off : nullptr; a.scale = io.scale;
}

// ConvIO::cout_need: only output-channel blocks [0, nb) of the layer's ncb are wanted.  The shape picked for the whole layer stays
// (P, ks, CI_T: the K chunks of wave (cbi, kj) and the order the ks partial tiles are summed in), so those channels get the same
// bits.  The workgroups keep their pixels and the grid its rows where it can: each row keeps wco = ceil(nb / ny) of its
// output-channel waves (one row: the waves of the unwanted blocks are dropped), if `can_stage(wco)`: the fewer threads still stage
// the patch.  Otherwise the rows without a wanted block are dropped; with one row and no such staging plan the whole layer runs
// (returns false).  (Dropping rows alone does not make the launch shorter where the whole layer is one workgroup per CU or fewer:
// each workgroup takes as long as before — RAFT-Stereo at 544x960, flow_head.conv1+mask.0: 2 rows of 128 workgroups of 12 waves,
// one row 23.7 us against 23.5 for both.)
template <class CanStage>
inline bool conv_restrict_cout(const ConvLayer& L, int cout_need, int* ny, int* wco, CanStage can_stage) {
    const int nb = cdiv(cout_need, 32);
    if (cout_need <= 0 || nb >= L.ncb) return false;
    const int w = cdiv(nb, *ny), rows = cdiv(nb, *wco);
    if (w < *wco && can_stage(w)) {
        *wco = w;
        *ny = cdiv(nb, w);
        return true;
    }
    if (rows >= *ny) return false;
    *ny = rows;
    return true;
}

}  // namespace nnd
