// One residual block of the feature encoder's first two stages (1x1 projection shortcut) as ONE launch:
//
//   out = relu( relu(norm2(conv2 3x3( relu(norm1(conv1 3x3(x))) ))) + norm3(conv 1x1(x)) )
//
//   layer1.0, layer1.1   64 -> 64, stride 1        layer2.0   64 -> 96, conv1 and the shortcut at stride 2        layer2.1   96 -> 96, stride 1
//
// (nndepth/blocks/residual_block.py:53-60; the norms are eval-mode BatchNorm folded into per-channel scale / shift, or absent.)
// It replaces the three launches encoder.hip makes per block — conv1 (conv_split), the shortcut (stride 1: conv1x1_stream_kernel on
// the exact fp32 MFMA; stride 2: conv_split's 1x1 stride-2 kernel in the split arithmetic), conv2 + add (conv_split) — and computes
// the same bits: each of the three convolutions keeps its packed blob, its K order (16-channel chunks in order, the 9 taps of a
// chunk in order, the pieces' products small ones first, no split K: what pick_split chooses for Cin = 64 always and for Cin = 96
// on maps of about 512 workgroup columns and more — encoder.hip asks the picker and keeps the three launches elsewhere), its
// activation scale (the stride-2 shortcut splits x with its OWN scale: it was calibrated on the positions it reads) and its epilogue
// arithmetic; the map y between the two 3x3 convs is an fp32 value before it is split with conv2's activation scale, exactly what
// conv2 staged from memory.  What goes away is the traffic: y and the shortcut are never written, x is read once from HBM (the
// shortcut's second read of its pixels hits L2).
//
// Workgroup = C / 16 waves on an 8 x 16 output tile (C output channels).  LDS (PS = NS * 32 + 16 bytes per position and 16-channel
// chunk, conv_split's piece layout: piece s of channels 8h .. 8h + 7 at s * 32 + h * 16, so a lane's B operand is one 16-byte read):
//   y   C / 16 chunks x 10 x 18 positions (the tile + conv2's 1-pixel halo)       C / 16 * 180 * PS   (fp16x2: 57 600 B | 86 400 B)
//   x   one 16-channel chunk, single buffer.  Stride 1: 12 x 20 positions (the tile + 2 pixels)       240 * PS   (fp16x2: 19 200 B)
//       stride 2: the 21 x 37 inputs of the y region as 4 parity phases of 11 x 19 positions       836 * PS   (fp16x2: 66 880 B)
// 64 -> 64: 76 800 B, two workgroups of 4 waves per CU, which cover each other's staging, barriers and epilogues.  96 -> 96: 105 600 B,
// 64 -> 96: 153 280 B, one workgroup of 6 waves per CU.  For 96 -> 96, 4 x 16 tiles (64 640 B, two workgroups per CU, twice the conv1
// work per output instead of 1.5 times) measured 111-112 us per launch against 89 at 136x240x2: the halo recompute costs more than
// the second workgroup hides.  The maps are stored as plain rows (no row padding): PS is an odd number of
// 16-byte units, so 16 consecutive positions of a row fall into the 16 different bank groups; at stride 2 the parity phases
// (conv_split_kernel.h's stride-2 patch) give every tap the same unit position stride.
// conv1 numbers the 180 y positions linearly over 6 MFMA column blocks (12 idle lanes; +50 % conv1 work for the halo), a
// wave = (output-channel block, 3 of the column blocks); conv2's column blocks are 2 x 16 pixels with lane_pixel()'s lane order
// (each half of a ds_read_b128's lanes then reads one row), a wave = (output-channel block, 2 of the 4 column blocks).  Each
// weight fragment read from L2 feeds 3 (conv1) or 2 (conv2) column blocks; the fragments of the next kernel row are requested
// while the current row's MFMAs run, the B fragments of the next (tap, column block) unit while the current unit's do.  y positions
// outside the image are conv2's zero padding: they are stored as zeros, not as conv1 evaluated there.
#include "common.h"
#include "conv_epilogue.h"
#include "conv_split_kernel.h"
#include "layout.h"
#include "split_arith.h"

#include <atomic>

namespace nnd {

namespace {
// The shape of one instantiation: NCB 32-channel output blocks (C = 32 NCB channels out, NCH = C / 16 chunks of y), CIN input
// channels (NCH1 = CIN / 16 chunks of x), STR = stride of conv1 and of the shortcut.
template <int NCB_, int CIN_, int STR_>
struct EbShape {
    static constexpr int NCB = NCB_, C = 32 * NCB, NCH = 2 * NCB, CIN = CIN_, NCH1 = CIN / 16, STR = STR_;
    static constexpr int NQ = CIN / 8;  // stride 1: float4 fragments of the shortcut's weights per lane
    static constexpr int TH = 8, TW = 16;                                    // output tile
    static constexpr int YR = TH + 2, YC = TW + 2, NY = YR * YC;             // y region
    // x region.  Stride 1: XR x XC positions (the tile + 2 pixels) in rows of XRW.  Stride 2: the (2 YR + 1) x (2 YC + 1) inputs of
    // the y region as their 4 (row, column) parity phases (conv_split_kernel.h's stride-2 patch), each a grid of (YR + 1) rows of
    // XRW = YC + 1 positions (PHN in all): input (2 r + dy, 2 c + dx) is position (r + dy / 2, c + dx / 2) of phase (dy % 2, dx % 2),
    // so the lanes of a column block read consecutive positions for every tap, as at stride 1.
    static constexpr int XR = TH + 4, XC = TW + 4;
    static constexpr int XRW = STR == 1 ? XC : YC + 1, PHN = STR == 1 ? 0 : (YR + 1) * XRW, NX = STR == 1 ? XR * XC : 4 * PHN;
    static constexpr int B1 = 6, B2 = 4;  // MFMA column blocks of a workgroup: conv1 (y region), conv2 / shortcut (tile)
    // waves per output-channel block (NCB x HV waves in all), each with B1 / HV of conv1's column blocks and B2 / HV of conv2's.
    // Measured for 64 -> 64 with 1 (two waves of 6 / 4 column blocks, 365 VGPRs, half the weight stream from L2): 141-144 us per
    // launch against 136-139 at 272x480x2, so the weight stream is not what the launch waits for; 2 it is.
    static constexpr int HV = 2;
    static constexpr int P1 = B1 / HV, P2 = B2 / HV, NTHR = 64 * NCB * HV;
    static_assert(B1 * 32 >= NY && B2 * 32 == TH * TW, "column blocks cover the y region / the tile");
    static_assert((STR == 1 && CIN == C) || STR == 2, "a stride-1 block keeps its channel count");
    static_assert(NCH1 % 2 == 0, "the weight ring's phase returns to 0 behind conv1");
    static constexpr size_t lds_bytes(int NS) { return (size_t)(NCH * NY + NX) * (NS * 32 + 16); }
};
constexpr int eb_ps(int NS) { return NS * 32 + 16; }

struct EncBlockArgs {
    const float* x;
    float* out;
    long bsx, bs;  // floats between samples of x / out (tile-major, 4 channels interleaved)
    const uint4 *w1, *w2;
    const float4* wd;  // the shortcut's weights: fp32 fragments (stride 1) or split pieces in conv_split's order (stride 2)
    const float *shift1, *scale1, *shift2, *scale2, *shiftd, *scaled;  // SPLIT_TAIL_* of conv1 / conv2 at shift + C
    Lay layx, lay;            // x / out
    int Hx, Wx, H, W, tiles_x;  // size of x / of y and out
};

// the 9 taps of one 16-channel chunk: RW = positions per row of the LDS map, bb[pp] = the lane's byte address of tap (0, 0) for its
// column block pp.  ab: two register sets of one kernel row's fragments (3 taps x NS pieces); set (PAR + dy) & 1 holds row dy, the
// next row — row 0 of `wn`, the following chunk, behind row 2 — is requested before the row's MFMAs.  PHN > 0: the map holds the 4
// parity phases of a stride-2 patch, PHN positions each (EbShape).
template <int NS, int P, int RW, int PAR, int PHN = 0>
__device__ __forceinline__ void eb_walk_chunk(const uint4* wc, const uint4* wn, uint4 (&ab)[2][3][NS], const unsigned char* const (&bb)[P],
                                              f32x16 (&acc)[P]) {
    constexpr int PS = eb_ps(NS), NUNIT = 9 * P;
    // B fragments one unit (tap, column block) ahead, in two register sets: left to the compiler, each unit's reads were issued
    // behind the previous unit's MFMAs and waited for at once (ds_read, s_waitcnt lgkmcnt, v_mfma)
    uint4 b[2][NS];
    auto read_b = [&](int u, uint4(&dst)[NS]) {
        const int t = u / P, pp = u % P;
        const int dy = t / 3, dx = t % 3;
        const int toff = PHN == 0 ? dy * RW + dx : ((dy & 1) * 2 + (dx & 1)) * PHN + (dy >> 1) * RW + (dx >> 1);
#pragma unroll
        for (int s = 0; s < NS; ++s) dst[s] = *reinterpret_cast<const uint4*>(bb[pp] + toff * PS + s * 32);
    };
    read_b(0, b[0]);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        uint4(&cur)[3][NS] = ab[(PAR + dy) & 1];
        uint4(&nxt)[3][NS] = ab[(PAR + dy + 1) & 1];
        const uint4* wr = dy < 2 ? wc + (dy + 1) * 3 * NS * 64 : wn;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
#pragma unroll
            for (int s = 0; s < NS; ++s) nxt[dx][s] = wr[(dx * NS + s) * 64];
        __builtin_amdgcn_sched_barrier(0);  // the requests stay in front of the row's MFMAs
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
#pragma unroll
            for (int pp = 0; pp < P; ++pp) {
                const int u = (dy * 3 + dx) * P + pp;
                if (u + 1 < NUNIT) read_b(u + 1, b[(u + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
                split_mfma_step<NS>(cur[dx], b[u & 1], acc[pp]);  // small products first (split_arith.h)
                __builtin_amdgcn_sched_barrier(0);
            }
    }
}

template <int NS, class S>
__global__ void __launch_bounds__(S::NTHR) __attribute__((amdgpu_waves_per_eu(2))) enc_block_kernel(EncBlockArgs a) {
    constexpr int EB_P1 = S::P1, EB_P2 = S::P2, NTHR = S::NTHR, NU = (2 * S::NX + NTHR - 1) / NTHR;
    constexpr int EB_TH = S::TH, EB_TW = S::TW, EB_YC = S::YC, EB_XC = S::XC, EB_NY = S::NY, EB_NX = S::NX, EB_NCH = S::NCH;
    constexpr int NCB = S::NCB, C = S::C, NQ = S::NQ, STR = S::STR, NCH1 = S::NCH1, XRW = S::XRW, PHN = S::PHN;
    constexpr int PS = eb_ps(NS), YCH = EB_NY * PS, CHW = 9 * NS * 64;  // bytes of a y chunk; uint4s of a chunk's weight fragments
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    unsigned char* const ybuf = lds_raw;
    unsigned char* const xbuf = lds_raw + EB_NCH * YCH;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cb = wave % NCB, half = wave / NCB;
    const int h2 = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.z;
    const int ty0 = (blockIdx.x / a.tiles_x) * EB_TH, tx0 = (blockIdx.x % a.tiles_x) * EB_TW;
    const int H = a.H, W = a.W;
    const int SP = (int)a.lay.plane, SPX = (int)a.layx.plane;
    const float* xs = a.x + b * a.bsx;

    // ---- staging units of this thread: unit = (x position, 8 of the chunk's 16 channels) = two 16-byte loads
    int goff[NU], gstep[NU], loff[NU];
    bool inimg[NU], own[NU];
#pragma unroll
    for (int i = 0; i < NU; ++i) {
        const int u = tid + i * NTHR;
        own[i] = u < 2 * EB_NX;
        const int oct = u / EB_NX, pos = u % EB_NX;
        int gy, gx;
        if constexpr (STR == 1) {
            gy = ty0 - 2 + pos / EB_XC, gx = tx0 - 2 + pos % EB_XC;
        } else {  // position q of phase ph = input (2 (q / XRW) + ph / 2, 2 (q % XRW) + ph % 2) of the region that starts at 2 ty0 - 3
            const int ph = pos / PHN, q = pos % PHN;  // (the odd phases' last row / column is never read)
            gy = 2 * ty0 - 3 + 2 * (q / XRW) + (ph >> 1), gx = 2 * tx0 - 3 + 2 * (q % XRW) + (ph & 1);
        }
        inimg[i] = own[i] && gy >= 0 && gy < a.Hx && gx >= 0 && gx < a.Wx;
        goff[i] = inimg[i] ? oct * 8 * SPX + (int)pix_off(a.layx, gy, gx) : 0;  // clamped to element 0 when masked; zeroed below
        gstep[i] = inimg[i] ? 4 * SPX : 0;
        loff[i] = pos * PS + oct * 16;
    }
    float stage[NU][8];
    auto stage_load = [&](int K) {
        const float* src = xs + (long)K * 16 * SPX;
#pragma unroll
        for (int i = 0; i < NU; ++i)
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const float4 t = *reinterpret_cast<const float4*>(src + (unsigned)(goff[i] + g * gstep[i]));
                stage[i][4 * g] = t.x; stage[i][4 * g + 1] = t.y; stage[i][4 * g + 2] = t.z; stage[i][4 * g + 3] = t.w;
            }
    };
    const float* tail1 = a.shift1 + C;
    const float* tail2 = a.shift2 + C;
    const float oscale1 = tail1[SPLIT_TAIL_OSCALE], xscale1 = tail1[SPLIT_TAIL_XSCALE];
    const float oscale2 = tail2[SPLIT_TAIL_OSCALE], xscale2 = tail2[SPLIT_TAIL_XSCALE];
    auto stage_store = [&]() {
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = inimg[i] ? stage[i][j] : 0.f;
            uint4 pieces[NS];
            split_pieces<NS>(v, pieces, xscale1);
            if (own[i]) {
#pragma unroll
                for (int s = 0; s < NS; ++s) *reinterpret_cast<uint4*>(xbuf + loff[i] + s * 32) = pieces[s];
            }
        }
    };

    // ---- conv1: this lane's y positions (column block half * P1 + pp, lane l31 of it)
    const unsigned char* xb1[EB_P1];
    int ypos[EB_P1];
    bool ywrite[EB_P1], yin[EB_P1];
#pragma unroll
    for (int pp = 0; pp < EB_P1; ++pp) {
        const int p = (half * EB_P1 + pp) * 32 + l31;
        const int pc = min(p, EB_NY - 1);  // the 12 lanes past the region repeat its last position and write nothing
        const int yr = pc / EB_YC, yc = pc % EB_YC;
        ypos[pp] = pc;
        ywrite[pp] = p < EB_NY;
        const int iy = ty0 - 1 + yr, ix = tx0 - 1 + yc;
        yin[pp] = iy >= 0 && iy < H && ix >= 0 && ix < W;
        xb1[pp] = xbuf + (yr * XRW + yc) * PS + h2 * 16;
    }
    const uint4* w1 = a.w1 + (size_t)cb * NCH1 * CHW + lane;
    const uint4* w2 = a.w2 + (size_t)cb * EB_NCH * CHW + lane;

    uint4 ab[2][3][NS];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx)
#pragma unroll
        for (int s = 0; s < NS; ++s) ab[0][dx][s] = w1[(dx * NS + s) * 64];
    stage_load(0);
    stage_store();
    __syncthreads();

    f32x16 acc1[EB_P1];
#pragma unroll
    for (int pp = 0; pp < EB_P1; ++pp)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc1[pp][i] = 0.f;

    auto conv1_chunk = [&](int K, auto par_c) {
        constexpr int PAR = decltype(par_c)::value;
        const bool more = K + 1 < NCH1;
        if (more) stage_load(K + 1);  // in flight behind the chunk's MFMAs
        eb_walk_chunk<NS, EB_P1, XRW, PAR, PHN>(w1 + K * CHW, more ? w1 + (K + 1) * CHW : w2, ab, xb1, acc1);
        __syncthreads();  // every wave has read chunk K
        if (more) {
            stage_store();
            __syncthreads();
        }
    };
    for (int K = 0; K < NCH1; K += 2) {  // 3 rows per chunk: the ring's phase alternates
        conv1_chunk(K, std::integral_constant<int, 0>{});
        conv1_chunk(K + 1, std::integral_constant<int, 1>{});
    }

    // ---- y = relu(acc * scale + shift) in fp32 (conv_split's epilogue), zero outside the image, split with conv2's scale into LDS.
    // Registers 4q .. 4q + 3 of a lane are channels cb * 32 + 8q + 4 h2 + 0..3 of its position: 8 bytes of piece s.
    {
        float sc1[16], sh1[16];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int co = cb * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h2;
            sc1[reg] = a.scale1[co];
            sh1[reg] = a.shift1[co];
        }
#pragma unroll
        for (int pp = 0; pp < EB_P1; ++pp) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float ac = acc1[pp][4 * q + i] * oscale1;  // exact: a power of two
                    const float t = relu_nan(fmaf(ac, sc1[4 * q + i], sh1[4 * q + i]));
                    v[i] = yin[pp] ? t : 0.f;
                }
                uint2 pieces[NS];
                split_pieces_n<NS, 4, uint2>(v, pieces, xscale2);
                if (ywrite[pp]) {
                    unsigned char* d = ybuf + (cb * 2 + (q >> 1)) * YCH + ypos[pp] * PS + ((q & 1) * 8 + 4 * h2) * 2;
#pragma unroll
                    for (int s = 0; s < NS; ++s) *reinterpret_cast<uint2*>(d + s * 32) = pieces[s];
                }
            }
        }
    }
    __syncthreads();

    // ---- conv2 from LDS: column block j = half * P2 + pp = rows 2j, 2j + 1 of the tile, 16 pixels each
    const int pxl = lane_pixel(l31), r2 = pxl >> 4, c2 = pxl & 15;
    int oy[EB_P2];
    const int ox = tx0 + c2;
    int yb2[EB_P2];
#pragma unroll
    for (int pp = 0; pp < EB_P2; ++pp) {
        const int row = 2 * (half * EB_P2 + pp) + r2;
        oy[pp] = ty0 + row;
        yb2[pp] = (row * EB_YC + c2) * PS + h2 * 16;
    }
    f32x16 acc2[EB_P2];
#pragma unroll
    for (int pp = 0; pp < EB_P2; ++pp)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc2[pp][i] = 0.f;
    // the shortcut's operands.  Stride 1: fp32 weight fragments and channel quads; stride 2: the split pieces of the weights (one tap:
    // NS fragments per chunk) and, per pixel, channels 8 h2 .. 8 h2 + 7 of every chunk of input (2 oy, 2 ox) — a lane's B operand
    constexpr int NXQ = STR == 1 ? NQ : 2 * NCH1, NAF = STR == 1 ? NQ : NCH1 * NS;
    float4 xq[EB_P2][NXQ], afr[NAF];
    auto conv2_chunk = [&](int K, auto par_c) {
        constexpr int PAR = decltype(par_c)::value;
        const unsigned char* bb[EB_P2];
#pragma unroll
        for (int pp = 0; pp < EB_P2; ++pp) bb[pp] = ybuf + K * YCH + yb2[pp];
        eb_walk_chunk<NS, EB_P2, EB_YC, PAR>(w2 + K * CHW, w2 + (K + 1 < EB_NCH ? K + 1 : K) * CHW, ab, bb, acc2);
    };
    for (int K = 0; K < EB_NCH - 2; K += 2) {
        conv2_chunk(K, std::integral_constant<int, 0>{});
        conv2_chunk(K + 1, std::integral_constant<int, 1>{});
    }
    conv2_chunk(EB_NCH - 2, std::integral_constant<int, 0>{});
    // requested behind conv2's last chunk (stride 1: the weight fragments are conv1x1_stream_kernel's, NQ float4 per lane; the lower
    // half-wave loads the even channel quads, the upper one the odd ones.  C = 96: 8 of the 12 weight fragments here, the rest behind
    // the chunk — the registers the chunk leaves free)
    constexpr int NAE = NAF < 8 ? NAF : 8;
    const float4* wq = a.wd + (size_t)cb * NAF * 64 + lane;
    {
#pragma unroll
        for (int q = 0; q < NAE; ++q) afr[q] = wq[q * 64];
#pragma unroll
        for (int pp = 0; pp < EB_P2; ++pp) {
            const bool ok = oy[pp] < H && ox < W;
            const float* src = xs + (ok ? pix_off(a.layx, STR * oy[pp], STR * ox) : 0);
#pragma unroll
            for (int j = 0; j < NXQ; ++j) {
                const int quad = STR == 1 ? 2 * j + h2 : 4 * (j / 2) + 2 * h2 + j % 2;
                xq[pp][j] = *reinterpret_cast<const float4*>(src + (long)quad * 4 * SPX);
            }
        }
    }
    conv2_chunk(EB_NCH - 1, std::integral_constant<int, 1>{});
#pragma unroll
    for (int q = NAE; q < NAF; ++q) afr[q] = wq[q * 64];

    // ---- shortcut, then both epilogues and the add.  Stride 1: the fp32 MFMA in conv1x1_stream_kernel's k order (channel pairs
    // 0 .. C / 2 - 1 in order).  Stride 2: conv_split's 1x1 stride-2 launch — x split with the SHORTCUT's activation scale (its
    // calibrated range is that of the positions it reads, not conv1's), chunks in order, small products first, its own oscale.
    const float* taild = a.shiftd + C;
    const float oscaled = STR == 1 ? 1.f : taild[SPLIT_TAIL_OSCALE], xscaled = STR == 1 ? 1.f : taild[SPLIT_TAIL_XSCALE];
    float scd[16], shd[16], sc2[16], sh2[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int co = cb * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h2;
        scd[reg] = a.scaled[co];
        shd[reg] = a.shiftd[co];
        sc2[reg] = a.scale2[co];
        sh2[reg] = a.shift2[co];
    }
#pragma unroll
    for (int pp = 0; pp < EB_P2; ++pp) {
        f32x16 accs;
#pragma unroll
        for (int i = 0; i < 16; ++i) accs[i] = 0.f;
        if constexpr (STR == 2) {
#pragma unroll
            for (int K = 0; K < NCH1; ++K) {
                const float4 lo = xq[pp][2 * K], hi = xq[pp][2 * K + 1];
                const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                uint4 pieces[NS], aw[NS];
                split_pieces<NS>(v, pieces, xscaled);
#pragma unroll
                for (int s = 0; s < NS; ++s) aw[s] = __builtin_bit_cast(uint4, afr[K * NS + s]);
                split_mfma_step<NS>(aw, pieces, accs);
            }
        } else {
        float bv[4 * NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const float4 q4 = xq[pp][j];
            const auto s01 = __builtin_amdgcn_permlane32_swap(__float_as_uint(q4.x), __float_as_uint(q4.y), false, false);
            const auto s23 = __builtin_amdgcn_permlane32_swap(__float_as_uint(q4.z), __float_as_uint(q4.w), false, false);
            bv[4 * j + 0] = __uint_as_float(s01[0]);
            bv[4 * j + 1] = __uint_as_float(s23[0]);
            bv[4 * j + 2] = __uint_as_float(s01[1]);
            bv[4 * j + 3] = __uint_as_float(s23[1]);
        }
#pragma unroll
        for (int kp = 0; kp < 4 * NQ; ++kp) {
            const float4 av = afr[kp / 4];
            const float a_s = (kp % 4 == 0) ? av.x : (kp % 4 == 1) ? av.y : (kp % 4 == 2) ? av.z : av.w;
            accs = __builtin_amdgcn_mfma_f32_32x32x2f32(a_s, bv[kp], accs, 0, 0, 0);
        }
        }
        const bool ok = oy[pp] < H && ox < W;
        float* o = a.out + b * a.bs + (ok ? pix_off(a.lay, oy[pp], ox) : 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int co0 = cb * 32 + 8 * q + 4 * h2;
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int reg = 4 * q + i;
                const float ac = acc2[pp][reg] * oscale2;
                float y2 = relu_nan(fmaf(ac, sc2[reg], sh2[reg]));
                const float sc = fmaf(STR == 1 ? accs[reg] : accs[reg] * oscaled, scd[reg], shd[reg]);
                y2 = sc + y2;
                v[i] = relu_nan(y2);
            }
            if (ok) *reinterpret_cast<float4*>(o + (long)co0 * SP) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

template <int NS, class S>
int launch_enc_block(const EncBlockArgs& a, dim3 grid, hipStream_t stream) {
    auto kern = enc_block_kernel<NS, S>;
    constexpr size_t lds = S::lds_bytes(NS);
    if (lds > 64 * 1024) {
        static std::atomic<unsigned> raised{0};
        if (int rc = raise_lds_limit(reinterpret_cast<const void*>(kern), raised, (int)lds)) return rc;
    }
    hipLaunchKernelGGL(kern, grid, dim3(S::NTHR), lds, stream, a);
    return NND_OK;
}

template <class S>
int enc_block_run(const ConvLayer& c1, const float* blob1, const ConvLayer& c2, const float* blob2, const ConvLayer& ds, const float* blobd,
                  const float* x, float* out, int N, int Hx, int Wx, hipStream_t stream) {
    const int H = cdiv(Hx, S::STR), W = cdiv(Wx, S::STR);
    EncBlockArgs a{};
    a.x = x; a.out = out;
    a.layx = make_lay(Hx, Wx, true, true); a.lay = make_lay(H, W, true, true);
    a.bsx = S::CIN * a.layx.plane; a.bs = S::C * a.lay.plane;
    a.w1 = reinterpret_cast<const uint4*>(blob1 + c1.w_off); a.shift1 = blob1 + c1.b_off; a.scale1 = blob1 + c1.s_off;
    a.w2 = reinterpret_cast<const uint4*>(blob2 + c2.w_off); a.shift2 = blob2 + c2.b_off; a.scale2 = blob2 + c2.s_off;
    a.wd = reinterpret_cast<const float4*>(blobd + ds.w_off); a.shiftd = blobd + ds.b_off; a.scaled = blobd + ds.s_off;
    a.Hx = Hx; a.Wx = Wx; a.H = H; a.W = W; a.tiles_x = cdiv(W, S::TW);
    const dim3 grid(a.tiles_x * cdiv(H, S::TH), 1, N);
    if (switches().conv_verbose)  // (the tests count the tags: layer1's blocks and layer2's print different ones)
        fprintf(stderr, "[nnd] %s %d -> %d stride %d pieces=%d: grid %ux1x%d, lds %zu B\n", S::C == 64 ? "enc_block" : "enc_stage2_block", S::CIN,
                S::C, S::STR, c1.arith, grid.x, N, S::lds_bytes(c1.arith));
    int rc = c1.arith == 2 ? launch_enc_block<2, S>(a, grid, stream) : launch_enc_block<1, S>(a, grid, stream);
    if (rc != NND_OK) return rc;
    NND_LAUNCH_CHECK();
    return NND_OK;
}
}  // namespace

// conv1: 3x3 Cin -> C, conv2: 3x3 C -> C stride 1, in the same range-scaled fp16 arithmetic (fp16x2 or fp16), folded-norm slots
// packed.  Stride 1 (C = 64: layer1's blocks, C = 96: layer2.1): Cin = C, ds = the 1x1 shortcut on the exact fp32 MFMA in 32-channel
// chunks (what conv1x1_stream_kernel reads).  Stride 2 (layer2.0, 64 -> 96): conv1 and ds = the 1x1 shortcut have stride 2, ds in the
// split arithmetic of the 3x3 convs.  The K order the block reproduces is conv_split's without split K: the caller asks the picker
// (conv_split_no_split_k) for the shape at hand.
bool enc_block_supported(const ConvLayer& c1, const ConvLayer& c2, const ConvLayer& ds) {
    const int Cin = c1.Cin, C = c1.Cout, st = c1.stride;
    auto conv = [](const ConvLayer& l, int k, int cin, int cout, int stride) {
        return l.KH == k && l.KW == k && l.Cin == cin && l.Cout == cout && l.stride == stride && l.s_off >= 0;
    };
    if (!conv(c1, 3, Cin, C, st) || !conv(c2, 3, C, C, 1) || !conv(ds, 1, Cin, C, st) || c1.CI_T != 16 || c2.CI_T != 16 || c1.arith != c2.arith ||
        (c1.arith != 2 && c1.arith != 1))
        return false;
    if (st == 1) return Cin == C && (C == 64 || C == 96) && ds.arith == 0 && ds.CI_T == 32;
    return st == 2 && Cin == 64 && C == 96 && ds.arith == c1.arith && ds.CI_T == 16;
}

// x: (N, Cin, Hx, Wx), out: (N, C, ceil(Hx / stride), ceil(Wx / stride)), tile-major with 4 channels interleaved (layout.h), distinct
// buffers; blob1 / blob2 / blobd: the bases the layers' offsets are relative to
int enc_block_launch(const ConvLayer& c1, const float* blob1, const ConvLayer& c2, const float* blob2, const ConvLayer& ds, const float* blobd,
                     const float* x, float* out, int N, int Hx, int Wx, hipStream_t stream) {
    NND_REQUIRE(enc_block_supported(c1, c2, ds), "enc_block: built for the 64 -> 64, 96 -> 96 (stride 1) and 64 -> 96 (stride 2) blocks in fp16x2 / fp16");
    NND_REQUIRE(x && out && x != out && N > 0 && Hx > 0 && Wx > 0, "enc_block: bad argument");
    NND_REQUIRE(c1.Cout * tiled_plane(Hx, Wx) < (1L << 31), "enc_block: plane offsets exceed 32 bits");
    if (c1.stride == 2) return enc_block_run<EbShape<3, 64, 2>>(c1, blob1, c2, blob2, ds, blobd, x, out, N, Hx, Wx, stream);
    if (c1.Cin == 64) return enc_block_run<EbShape<2, 64, 1>>(c1, blob1, c2, blob2, ds, blobd, x, out, N, Hx, Wx, stream);
    return enc_block_run<EbShape<3, 96, 1>>(c1, blob1, c2, blob2, ds, blobd, x, out, N, Hx, Wx, stream);
}

}  // namespace nnd
