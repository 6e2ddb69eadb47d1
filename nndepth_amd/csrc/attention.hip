// Full (softmax) attention of the LoFTR layer, exact fp32, flash style: the (L x S) score matrix never leaves the registers.
//
// Replaces FullAttention.forward  nndepth/blocks/attn_block.py:59-97 (no masks, no dropout), head dimension 32:
//   out[n, 32h+d, l] = sum_s softmax_s( (sum_d q[n,32h+d,l] k[n,32h+d,s]) / sqrt(32) ) v[n,32h+d,s]
// on the channel-major maps (N, nhead*32, L) / (N, nhead*32, S) that the 1x1 convs of loftr.hip produce: no transposes.
//
// One wave owns 32 queries of one head; the workgroup's ATT_WAVES waves share K / V tiles of 32 keys in LDS.
//   scores, swapped:  St[key][query] = sum_d K[d][key] Q[d][query]          16 x mfma_f32_32x32x2f32, k-step s = d pair (2s, 2s+1)
//       A = K[d = 2s + (lane>>5)][key = lane&31]   (LDS, [d][key], 32-float rows: the two halves of a wave read banks 0-31 / 32-63)
//       B = Q[d = 2s + (lane>>5)][query = lane&31] (16 registers, loaded once, pre-multiplied by log2(e) / sqrt(32))
//     accumulator register r of lane (query = lane&31, half = lane>>5) is key crow(r, half) = (r&3) + 8(r>>2) + 4 half:
//     a lane holds 16 of its query's 32 scores, lane^32 the other 16; max and sum are 15 in-lane steps + one exchange.
//   online softmax in the base-2 domain: m = running max, l = running sum, both per query (equal in the two half lanes)
//   P V, same orientation:  Ot[d][query] = sum_key V[d][key] Pt[key][query]  16 x mfma, k-step r = keys crow(r,0), crow(r,1)
//       B = p[r] (the accumulator register itself: no lane movement)
//       A = V[d = lane&31][key = crow(r, lane>>5)]  (LDS, [half][d][r], 17-float rows: 64 distinct banks per read)
//     Ot lands as o[r] = O[d = crow(r, half)][query = lane&31]; exp2(m_old - m_new) rescales it with one per-lane factor, and the
//     store out[d][query] is contiguous along the query index.
// Keys beyond S are -inf before the max (their K and V tile entries are zero), queries beyond L are computed and not stored.
// No atomics and no split over S: one fixed evaluation order, the same bits run to run.
#include "common.h"

#include <cmath>

namespace nnd {

constexpr int ATT_D = 32;      // head dimension
constexpr int ATT_KT = 32;     // keys per tile
// waves (x 32 queries) per workgroup.  Raced at 1, 2 and 4 (profiles/loftr_full_bench.jsonl, "full_attention_waves_race"): 4 is the
// fastest at every shape from 17x30 to 68x120, N = 1 .. 8 (91.6 us against 103.9 and 119.7 at 33x60, N = 1), although it fills
// only half of the CUs there: a wave's share of the tile's loads and LDS writes, which nothing overlaps, shrinks with the width.
constexpr int ATT_WAVES = 4;
constexpr int ATT_THREADS = 64 * ATT_WAVES;
constexpr int ATT_PER = ATT_D * ATT_KT / ATT_THREADS;  // tile floats per thread, for K and for V
constexpr int ATT_VROW = 17, ATT_VHALF = ATT_D * ATT_VROW;  // V tile: [half][d][r], 17-float rows; the halves are 32 banks apart

using att_f16 = __attribute__((ext_vector_type(16))) float;

// The two halves of a wave exchange a value (v_permlane32_swap, no LDS): returns (the low half's x, the high half's x) in every lane
// pair, in that order in both lanes, so that max and sum come out with the same bits on both sides.
__device__ __forceinline__ void half_pair(float x, float& lo, float& hi) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    lo = __uint_as_float(r[0]);
    hi = __uint_as_float(r[1]);
}

// waves_per_eu(2): a budget of 256 registers, far above the ~100 used, under which the compiler keeps the two MFMA accumulators in
// ordinary vector registers; with the whole file on offer it put them in accumulation registers and moved all 32 of them across
// around every tile's rescale and exponentials (96 moves per tile).
__global__ void __launch_bounds__(ATT_THREADS) __attribute__((amdgpu_waves_per_eu(2)))
full_attention_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, float* __restrict__ out,
                      int L, int S, long q_bs, long kv_bs, long out_bs, float qscale) {
    __shared__ float ks[ATT_D * ATT_KT];
    __shared__ float vs[2 * ATT_VHALF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int h = blockIdx.y, n = blockIdx.z;
    const int qi = (blockIdx.x * ATT_WAVES + wave) * 32 + col;
    const bool q_ok = qi < L;

    const float* qb = q + (long)n * q_bs + (long)h * ATT_D * L;
    float qr[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) qr[s] = q_ok ? qb[(long)(2 * s + half) * L + qi] * qscale : 0.f;

    const float* kb = k + (long)n * kv_bs + (long)h * ATT_D * S;
    const float* vb = v + (long)n * kv_bs + (long)h * ATT_D * S;
    float kreg[ATT_PER], vreg[ATT_PER];
    auto fetch = [&](int key0) {
#pragma unroll
        for (int i = 0; i < ATT_PER; ++i) {
            const int e = tid + i * ATT_THREADS, d = e >> 5, key = key0 + (e & 31);
            const bool ok = key < S;
            kreg[i] = ok ? kb[(long)d * S + key] : 0.f;
            vreg[i] = ok ? vb[(long)d * S + key] : 0.f;
        }
    };

    att_f16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    float m = -INFINITY, l = 0.f;

    fetch(0);
    for (int key0 = 0; key0 < S; key0 += ATT_KT) {
        __syncthreads();  // every wave is done with the previous tile
#pragma unroll
        for (int i = 0; i < ATT_PER; ++i) {
            const int e = tid + i * ATT_THREADS, d = e >> 5, kk = e & 31;
            ks[d * ATT_KT + kk] = kreg[i];
            // key kk = crow(r, hf): r = (kk&3) + 4(kk>>3), hf = bit 2 of kk
            vs[((kk >> 2) & 1) * ATT_VHALF + d * ATT_VROW + (kk & 3) + 4 * (kk >> 3)] = vreg[i];
        }
        __syncthreads();
        if (key0 + ATT_KT < S) fetch(key0 + ATT_KT);  // the next tile's loads fly under this tile's arithmetic

        att_f16 sc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s)
            sc = __builtin_amdgcn_mfma_f32_32x32x2f32(ks[(2 * s + half) * ATT_KT + col], qr[s], sc, 0, 0, 0);
        if (key0 + ATT_KT > S) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (key0 + (r & 3) + 8 * (r >> 2) + 4 * half >= S) sc[r] = -INFINITY;
        }
        float mx = sc[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sc[r]);
        float lo, hi;
        half_pair(mx, lo, hi);
        mx = fmaxf(lo, hi);
        const float m_new = fmaxf(m, mx);  // finite: a tile has at least one key below S
        const float alpha = __builtin_amdgcn_exp2f(m - m_new);
        float rs = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            sc[r] = __builtin_amdgcn_exp2f(sc[r] - m_new);
            rs += sc[r];
        }
        half_pair(rs, lo, hi);
        rs = lo + hi;
        l = fmaf(l, alpha, rs);
        m = m_new;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            o = __builtin_amdgcn_mfma_f32_32x32x2f32(vs[half * ATT_VHALF + col * ATT_VROW + r], sc[r], o, 0, 0, 0);
    }

    if (!q_ok) return;
    float* ob = out + (long)n * out_bs + (long)h * ATT_D * L + qi;
#pragma unroll
    for (int r = 0; r < 16; ++r) ob[(long)((r & 3) + 8 * (r >> 2) + 4 * half) * L] = o[r] / l;
}

}  // namespace nnd

using namespace nnd;

extern "C" int nnd_full_attention(const float* q, const float* k, const float* v, float* out, int N, int nhead, int L, int S,
                                  int64_t q_bs, int64_t kv_bs, int64_t out_bs, void* stream) {
    NND_REQUIRE(q && k && v && out, "full_attention: null pointer");
    NND_REQUIRE(N > 0 && nhead > 0 && L > 0 && S > 0, "full_attention: N %d, nhead %d, L %d, S %d must be positive", N, nhead, L, S);
    NND_REQUIRE(N <= 65535 && nhead <= 65535, "full_attention: N %d / nhead %d above the grid's 65535", N, nhead);
    const int64_t C = (int64_t)nhead * ATT_D;
    NND_REQUIRE(C * L < (1ll << 31) && C * S < (1ll << 31), "full_attention: a sample's map above 2^31 floats");
    NND_REQUIRE(q_bs >= C * L && out_bs >= C * L && kv_bs >= C * S,
                "full_attention: batch strides %lld / %lld / %lld below the (nhead*32, L) / (nhead*32, S) maps", (long long)q_bs,
                (long long)kv_bs, (long long)out_bs);
    const float qscale = (float)(1.4426950408889634 / std::sqrt((double)ATT_D));  // log2(e) / sqrt(D): the softmax runs on exp2
    hipLaunchKernelGGL(full_attention_kernel, dim3(cdiv(L, 32 * ATT_WAVES), nhead, N), dim3(ATT_THREADS), 0, (hipStream_t)stream, q, k,
                       v, out, L, S, (long)q_bs, (long)kv_bs, (long)out_bs, qscale);
    NND_LAUNCH_CHECK();
    return NND_OK;
}
