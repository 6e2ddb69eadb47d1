// What the device-side criteria built as chains of masked reductions share (depth_eval.hip, midas_loss.hip): the block sum in a
// fixed tree, the previous launch's per-block partials added in index order, and the exact rank select on an order-preserving
// integer key with LDS histograms (integer atomics only).  Nothing here waits on another workgroup, retries, or adds floating-point
// values atomically: what is built from it gives the same bits run to run.
#pragma once
#include "common.h"

namespace nnd {

constexpr int DE_T = 256;    // threads of the reduction kernels
constexpr int DE_GMAX = 64;  // blocks per sample at most

// sums acc[0..N) over the block in a fixed tree; the totals are in sh[0][*] afterwards
template <int N>
__device__ __forceinline__ void de_block_sum(double (&acc)[N], double (*sh)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) sh[threadIdx.x][i] = acc[i];
    __syncthreads();
    for (int s = DE_T / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
#pragma unroll
            for (int i = 0; i < N; ++i) sh[threadIdx.x][i] += sh[threadIdx.x + s][i];
        __syncthreads();
    }
}

// tot[q] = sum over blk < G of part[blk * N + q], in index order (thread q); visible to the block after the barrier
template <int N>
__device__ __forceinline__ void de_sum_partials(const double* __restrict__ part, int G, double* tot) {
    if ((int)threadIdx.x < N) {
        double s = 0.0;
        for (int k = 0; k < G; ++k) s += part[(long)k * N + threadIdx.x];
        tot[threadIdx.x] = s;
    }
    __syncthreads();
}

// order-preserving key of an fp32 value (-0.0 sorts before +0.0: the same number either way)
__device__ __forceinline__ unsigned de_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float de_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// the same for a double
__device__ __forceinline__ unsigned long long de_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double de_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

template <typename K>
struct RankSelectLds {
    unsigned hist[256];
    K prefix;
    unsigned rank;
};

// The key at position `rank` (0-based) of the ascending order of the keys of those items i < n for which fetch(i, key) answers
// true: radix select, sizeof(K) passes of 8 bits from the top, each an LDS histogram of the items that agree with the digits already
// decided.  Called by all T threads of the workgroup with the same n and rank; rank < the number of such items (the caller returns
// before the call when there is none).  U items per thread and trip, their loads issued together; an item past the end reads item 0
// and is not counted.  The trip counts depend on n alone.
template <typename K, int T, int U, typename Fetch>
__device__ __forceinline__ K rank_select(long n, unsigned rank, Fetch fetch, RankSelectLds<K>& lds) {
    constexpr int BITS = (int)sizeof(K) * 8;
    if (threadIdx.x == 0) {
        lds.prefix = (K)0;
        lds.rank = rank;
    }
    __syncthreads();
    for (int shift = BITS - 8; shift >= 0; shift -= 8) {
        for (int j = threadIdx.x; j < 256; j += T) lds.hist[j] = 0u;
        __syncthreads();
        const K prefix = lds.prefix;
        const K himask = shift + 8 >= BITS ? (K)0 : (K)(~(K)0 << (shift + 8));  // the bits already decided
        for (long base = threadIdx.x; base < n; base += (long)T * U) {
            K key[U];
            bool ok[U];
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const long i = base + (long)j * T;
                const bool in = i < n;
                ok[j] = fetch(in ? i : 0, key[j]) && in;
            }
#pragma unroll
            for (int j = 0; j < U; ++j)
                if (ok[j] && ((key[j] ^ prefix) & himask) == (K)0) atomicAdd(&lds.hist[(unsigned)(key[j] >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned r = lds.rank, cum = 0u, digit = 255u;
            bool found = false;
            for (int j = 0; j < 256; ++j) {
                if (!found && cum + lds.hist[j] > r) {
                    digit = (unsigned)j;
                    r -= cum;
                    found = true;
                }
                cum += lds.hist[j];
            }
            lds.rank = r;
            lds.prefix = prefix | ((K)digit << shift);
        }
        __syncthreads();
    }
    return lds.prefix;
}

}  // namespace nnd
