// A masked k x k median and a guided weighted median of a disparity or depth map: the last step of the classical clean-up chain
// (left-right check, speckle removal, hole filling, median).  Beyond the reference, which has no such step.  The contract is a
// closed form (include/nndepth_amd.h): the op is a SELECTION, every output a copy of input bits, the weights integers, so the result
// is held to equality.  The guide distance is fp32, every step one rounded operation (built with -ffp-contract=off).
//
// nnd_median_filter: ONE launch, no workspace, no atomics.  A workgroup of 256 threads owns a tile of MED_TH x MED_TW outputs:
//   1  the tile plus a halo of `radius` in LDS, as KEYS: key(v) = bits(v) ^ (sign ? 0xFFFFFFFF : 0x80000000) orders as the values do
//      (-0.0 < +0.0), and 0xFFFFFFFF, which no finite value maps to, says "not ok" (masked out, not finite, out of frame).  With a
//      guide its channels lie behind the keys, and the 256 weights (they arrive in the launch's arguments) behind those.  Consecutive
//      lanes load consecutive columns of a halo row.
//   2  after ONE barrier a thread selects for MED_ROWS pixels of its column (its wave owns MED_ROWS rows of the tile; a wave reads 64
//      consecutive words of a row per tap: no bank conflict whatever the pitch):
//        unweighted, radius 1   a 25-exchange sorting network of the 9 keys in registers; the sentinels sort last and the element of
//                               rank (n - 1) / 2 is picked
//        unweighted, radius 2   the same with Batcher's 140-exchange network of the 25 keys
//        everything else        one pass over the window for n, T, the smallest and the largest ok key and, with a guide, the taps'
//                               weights (the guide distance is computed ONCE per tap); then an MSB-first bisection of the key that
//                               starts below the common prefix of the smallest and the largest key (as many rounds as those two
//                               differ in bits: 23 - 25 of 32 on the benchmark's noisy scene, fewer on a smooth map), each round
//                               the sum of the weights of the taps below the pivot
//      Where the window fits the register file (med_in_registers: to radius 4) the window loops are
//      fully unrolled: the compiler keeps the keys in registers across the rounds and the weights lie beside them PACKED two to a
//      word, 2 - 4 VALU operations per tap and round and no LDS traffic.  The larger windows walk the window's rows in a real loop
//      and read the keys from LDS every round; their weights lie in LDS too, 16 bits per tap and thread behind the table
//      (tap-major, so a wave reads 128 consecutive bytes): at radius 7 with 4 guide channels 147 KiB of the CU's 160.
//
// Bounds.  A global index is formed from (b, y, x) with b < B (the grid), 0 <= y < H, 0 <= x < W checked where it is formed, for the
// halo loads and for the stores alike; an LDS index is < (MED_TH + 2 R) (MED_TW + 2 R) (1 + C) words + the 512 bytes of the table
// (+ (2R+1)^2 * 512 bytes of tap weights for the large guided windows), which is what the launch asks for (med_lds_bytes); a weight
// index is 0 .. 255 by construction (s < 255.0f ? (int)s : 255 with s >= 0 or NaN).
#include <cstring>
#include "map_ops.h"  // the contract of map, stride, mask and its polarity, in and out

namespace nnd {

constexpr int MED_TH = 8, MED_TW = 64;   // the output tile of a workgroup
constexpr int MED_BLOCK = 256, MED_ROWS = MED_TH / (MED_BLOCK / 64);  // rows per thread
constexpr int MED_MAX_R = 7;
constexpr int MED_MAX_C = 4;
constexpr unsigned MED_BAD = 0xFFFFFFFFu;

struct MedWeights {
    unsigned w[128];  // 256 uint16, two to a word, as they lie in memory
};

__host__ __device__ __forceinline__ unsigned med_key(unsigned bits) { return bits ^ ((bits & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u); }
__host__ __device__ __forceinline__ unsigned med_unkey(unsigned k) { return k ^ ((k & 0x80000000u) ? 0x80000000u : 0xFFFFFFFFu); }

__host__ __device__ __forceinline__ void med_exchange(unsigned& a, unsigned& b) {
    const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

// unweighted 3 x 3: `win` = the window's top-left key, rows `pitch` words apart.  False: fewer than min_count ok taps.
__host__ __device__ __forceinline__ bool med_select9(const unsigned* win, int pitch, int min_count, unsigned& out) {
    unsigned v[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) v[i] = win[(i / 3) * pitch + i % 3];
    int n = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) n += v[i] != MED_BAD;
#define MED_X(a, b) med_exchange(v[a], v[b])
    MED_X(0, 3); MED_X(1, 7); MED_X(2, 5); MED_X(4, 8);
    MED_X(0, 7); MED_X(2, 4); MED_X(3, 8); MED_X(5, 6);
    MED_X(0, 2); MED_X(1, 3); MED_X(4, 5); MED_X(7, 8);
    MED_X(1, 4); MED_X(3, 6); MED_X(5, 7);
    MED_X(0, 1); MED_X(2, 4); MED_X(3, 5); MED_X(6, 8);
    MED_X(2, 3); MED_X(4, 5); MED_X(6, 7);
    MED_X(1, 2); MED_X(3, 4); MED_X(5, 6);
#undef MED_X
    const int rank = (n - 1) / 2;  // 0 .. 4
    out = rank == 4 ? v[4] : rank == 3 ? v[3] : rank == 2 ? v[2] : rank == 1 ? v[1] : v[0];
    return n >= min_count && n > 0;
}

// unweighted 5 x 5: Batcher's odd-even merge sort of 25 keys, 140 exchanges (the 0-1 principle checked over all 2^25 inputs); only
// the ranks 0 .. 12 can be picked, so the compiler drops the exchanges that feed the upper half alone
__host__ __device__ __forceinline__ bool med_select25(const unsigned* win, int pitch, int min_count, unsigned& out) {
    unsigned v[25];
#pragma unroll
    for (int i = 0; i < 25; ++i) v[i] = win[(i / 5) * pitch + i % 5];
    int n = 0;
#pragma unroll
    for (int i = 0; i < 25; ++i) n += v[i] != MED_BAD;
#define MED_X(a, b) med_exchange(v[a], v[b])
    MED_X(0, 1); MED_X(2, 3); MED_X(4, 5); MED_X(6, 7); MED_X(8, 9); MED_X(10, 11); MED_X(12, 13); MED_X(14, 15);
    MED_X(16, 17); MED_X(18, 19); MED_X(20, 21); MED_X(22, 23); MED_X(0, 2); MED_X(1, 3); MED_X(4, 6); MED_X(5, 7);
    MED_X(8, 10); MED_X(9, 11); MED_X(12, 14); MED_X(13, 15); MED_X(16, 18); MED_X(17, 19); MED_X(20, 22); MED_X(21, 23);
    MED_X(1, 2); MED_X(5, 6); MED_X(9, 10); MED_X(13, 14); MED_X(17, 18); MED_X(21, 22); MED_X(0, 4); MED_X(1, 5);
    MED_X(2, 6); MED_X(3, 7); MED_X(8, 12); MED_X(9, 13); MED_X(10, 14); MED_X(11, 15); MED_X(16, 20); MED_X(17, 21);
    MED_X(18, 22); MED_X(19, 23); MED_X(2, 4); MED_X(3, 5); MED_X(10, 12); MED_X(11, 13); MED_X(18, 20); MED_X(19, 21);
    MED_X(1, 2); MED_X(3, 4); MED_X(5, 6); MED_X(9, 10); MED_X(11, 12); MED_X(13, 14); MED_X(17, 18); MED_X(19, 20);
    MED_X(21, 22); MED_X(0, 8); MED_X(1, 9); MED_X(2, 10); MED_X(3, 11); MED_X(4, 12); MED_X(5, 13); MED_X(6, 14);
    MED_X(7, 15); MED_X(16, 24); MED_X(4, 8); MED_X(5, 9); MED_X(6, 10); MED_X(7, 11); MED_X(20, 24); MED_X(2, 4);
    MED_X(3, 5); MED_X(6, 8); MED_X(7, 9); MED_X(10, 12); MED_X(11, 13); MED_X(18, 20); MED_X(19, 21); MED_X(22, 24);
    MED_X(1, 2); MED_X(3, 4); MED_X(5, 6); MED_X(7, 8); MED_X(9, 10); MED_X(11, 12); MED_X(13, 14); MED_X(17, 18);
    MED_X(19, 20); MED_X(21, 22); MED_X(23, 24); MED_X(0, 16); MED_X(1, 17); MED_X(2, 18); MED_X(3, 19); MED_X(4, 20);
    MED_X(5, 21); MED_X(6, 22); MED_X(7, 23); MED_X(8, 24); MED_X(8, 16); MED_X(9, 17); MED_X(10, 18); MED_X(11, 19);
    MED_X(12, 20); MED_X(13, 21); MED_X(14, 22); MED_X(15, 23); MED_X(4, 8); MED_X(5, 9); MED_X(6, 10); MED_X(7, 11);
    MED_X(12, 16); MED_X(13, 17); MED_X(14, 18); MED_X(15, 19); MED_X(20, 24); MED_X(2, 4); MED_X(3, 5); MED_X(6, 8);
    MED_X(7, 9); MED_X(10, 12); MED_X(11, 13); MED_X(14, 16); MED_X(15, 17); MED_X(18, 20); MED_X(19, 21); MED_X(22, 24);
    MED_X(1, 2); MED_X(3, 4); MED_X(5, 6); MED_X(7, 8); MED_X(9, 10); MED_X(11, 12); MED_X(13, 14); MED_X(15, 16);
    MED_X(17, 18); MED_X(19, 20); MED_X(21, 22); MED_X(23, 24);
#undef MED_X
    const int rank = (n - 1) / 2;  // 0 .. 12
    unsigned r = v[0];
#pragma unroll
    for (int i = 1; i <= 12; ++i) r = rank == i ? v[i] : r;
    out = r;
    return n >= min_count && n > 0;
}

// The weighted lower median of a (2R+1)^2 window: `win` = its top-left key, `gwin` the same position in guide channel 0 (channels
// `gplane` floats apart), `wtab` the 256 weights.  False: n < min_count or T == 0 (`out` is not written).
template <int R, bool GUIDED>
__host__ __device__ __forceinline__ bool med_select(const unsigned* win, int pitch, const float* gwin, int gplane, int C, float inv_step,
                                                    const unsigned short* wtab, int min_count, unsigned& out) {
    constexpr int K = 2 * R + 1, NT = K * K;
    unsigned wp[GUIDED ? (NT + 1) / 2 : 1];  // the taps' weights, two to a word
    float gc[MED_MAX_C];
    if (GUIDED) {
#pragma unroll
        for (int c = 0; c < MED_MAX_C; ++c) gc[c] = c < C ? gwin[c * gplane + R * pitch + R] : 0.f;
    }
    int n = 0;
    unsigned T = 0, kmin = MED_BAD, kmax1 = 0;  // kmax1: the largest ok key + 1
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int off = (i / K) * pitch + i % K;
        const unsigned k = win[off], k1 = k + 1u;  // k1: 0 for the sentinel, else above 0: plain minima and maxima, no masks to keep
        const unsigned ok = k1 < 1u ? k1 : 1u;
        n += (int)ok;
        kmin = k < kmin ? k : kmin;
        kmax1 = k1 > kmax1 ? k1 : kmax1;
        if (GUIDED) {
            float dist = fabsf(gc[0] - gwin[off]);
#pragma unroll
            for (int c = 1; c < MED_MAX_C; ++c)
                if (c < C) dist = dist + fabsf(gc[c] - gwin[c * gplane + off]);
            const float s = dist * inv_step;
            const int b = (s < 255.0f) ? (int)s : 255;  // a NaN: 255
            const unsigned w = ok * (unsigned)wtab[b];
            T += w;
            if (i & 1) wp[i / 2] |= w << 16;
            else wp[i / 2] = w;
        }
    }
    if (!GUIDED) T = (unsigned)n;
    if (n < min_count || T == 0) return false;
    const unsigned kmax = kmax1 - 1u;  // n > 0 here
    unsigned a = kmin;
    if (kmin != kmax) {
        const int top = 31 - __builtin_clz(kmin ^ kmax);  // the highest bit in which two ok keys differ
        a = kmin & ~((2u << top) - 1u);                   // their common prefix (top == 31: 2u << 31 == 0, so a == 0)
        for (int bit = top; bit >= 0; --bit) {
            const unsigned pivot = a | (1u << bit);
            unsigned below = 0;  // the weight of the taps with key < pivot; a sentinel is below nothing
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const unsigned k = win[(i / K) * pitch + i % K];
                const unsigned w = !GUIDED ? 1u : (i & 1) ? wp[i / 2] >> 16 : wp[i / 2] & 0xFFFFu;
                below += k < pivot ? w : 0u;
            }
            if (2u * below < T) a = pivot;  // 2 T <= 2 * 225 * 65535 < 2^32
        }
    }
    out = a;
    return true;
}

// The same for the windows that do not fit the register file: the rows of the window in a real loop, the keys read from LDS every
// round, the taps' weights in `wts` (tap t at wts[t * wstride]: the caller's own 16 bits per tap).
template <int R, bool GUIDED>
__host__ __device__ __forceinline__ bool med_select_rows(const unsigned* win, int pitch, const float* gwin, int gplane, int C, float inv_step,
                                                         const unsigned short* wtab, unsigned short* wts, int wstride, int min_count,
                                                         unsigned& out) {
    constexpr int K = 2 * R + 1;
    float gc[MED_MAX_C];
    if (GUIDED) {
#pragma unroll
        for (int c = 0; c < MED_MAX_C; ++c) gc[c] = c < C ? gwin[c * gplane + R * pitch + R] : 0.f;
    }
    int n = 0;
    unsigned T = 0, kmin = MED_BAD, kmax1 = 0;
#pragma unroll 1
    for (int dy = 0; dy < K; ++dy) {
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
            const int off = dy * pitch + dx;
            const unsigned k = win[off], k1 = k + 1u;
            const unsigned ok = k1 < 1u ? k1 : 1u;
            n += (int)ok;
            kmin = k < kmin ? k : kmin;
            kmax1 = k1 > kmax1 ? k1 : kmax1;
            if (GUIDED) {
                float dist = fabsf(gc[0] - gwin[off]);
#pragma unroll
                for (int c = 1; c < MED_MAX_C; ++c)
                    if (c < C) dist = dist + fabsf(gc[c] - gwin[c * gplane + off]);
                const float s = dist * inv_step;
                const int b = (s < 255.0f) ? (int)s : 255;
                const unsigned w = ok * (unsigned)wtab[b];
                T += w;
                wts[(dy * K + dx) * wstride] = (unsigned short)w;
            }
        }
    }
    if (!GUIDED) T = (unsigned)n;
    if (n < min_count || T == 0) return false;
    const unsigned kmax = kmax1 - 1u;
    unsigned a = kmin;
    if (kmin != kmax) {
        const int top = 31 - __builtin_clz(kmin ^ kmax);
        a = kmin & ~((2u << top) - 1u);
        for (int bit = top; bit >= 0; --bit) {
            const unsigned pivot = a | (1u << bit);
            unsigned below = 0;
#pragma unroll 1
            for (int dy = 0; dy < K; ++dy) {
#pragma unroll
                for (int dx = 0; dx < K; ++dx) {
                    const unsigned k = win[dy * pitch + dx];
                    const unsigned w = GUIDED ? (unsigned)wts[(dy * K + dx) * wstride] : 1u;
                    below += k < pivot ? w : 0u;
                }
            }
            if (2u * below < T) a = pivot;
        }
    }
    out = a;
    return true;
}

// which windows are selected in registers (at radius 4 the guided kernel takes 254 registers, the unweighted 172; beyond, the
// compiler spills); the others by rows
constexpr bool med_in_registers(int R, bool guided) { return R <= 4; }
// dynamic LDS of a launch: the keys, C guide planes, the table, and for the guided windows selected by rows 16 bits per tap and thread
constexpr size_t med_lds_bytes(int R, bool guided, int C) {
    return (size_t)(MED_TW + 2 * R) * (MED_TH + 2 * R) * 4 * (guided ? 1 + C : 1) + (guided ? 512 : 0) +
           (guided && !med_in_registers(R, guided) ? (size_t)(2 * R + 1) * (2 * R + 1) * MED_BLOCK * 2 : 0);
}
static_assert(med_lds_bytes(MED_MAX_R, true, MED_MAX_C) <= 160 * 1024, "the largest guided window must fit the CU's LDS");

// grid (tiles_x * tiles_y, B); dynamic LDS: the keys, C guide planes, the table
template <int R, bool GUIDED>
__global__ void __launch_bounds__(MED_BLOCK, 2) median_kernel(const float* __restrict__ map, long mbs, const unsigned char* __restrict__ mask,
                                                           int valid_is_one, int min_count, int fill_invalid, float fill,
                                                           const float* __restrict__ guide, int C, float inv_step, MedWeights wt,
                                                           float* __restrict__ filtered, unsigned char* __restrict__ mask_out,
                                                           unsigned char* __restrict__ changed, int H, int W, int tiles_x) {
    constexpr int PW = MED_TW + 2 * R, PH = MED_TH + 2 * R, PA = PW * PH;
    extern __shared__ unsigned med_lds[];
    unsigned* keys = med_lds;
    float* gl = (float*)(med_lds + PA);
    unsigned short* wtab = (unsigned short*)(med_lds + PA * (GUIDED ? 1 + C : 1));
    unsigned short* wts = wtab + 256 + threadIdx.x;  // guided windows selected by rows: tap t of this thread at wts[t * MED_BLOCK]
    const int tid = threadIdx.x, b = blockIdx.y;
    const int y0 = ((int)blockIdx.x / tiles_x) * MED_TH, x0 = ((int)blockIdx.x % tiles_x) * MED_TW;
    const long per = (long)H * W;
    const float* mp = map + (long)b * mbs;

    for (int i = tid; i < PA; i += MED_BLOCK) {
        const int gy = y0 - R + i / PW, gx = x0 - R + i % PW;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        unsigned k = MED_BAD;
        if (in) {
            const long p = (long)gy * W + gx;
            const float v = mp[p];
            if (map_ok(v, mask, (long)b * per + p, valid_is_one)) k = med_key(__float_as_uint(v));
            if (GUIDED)
                for (int c = 0; c < C; ++c) gl[c * PA + i] = guide[((long)b * C + c) * per + p];
        } else if (GUIDED) {
            for (int c = 0; c < C; ++c) gl[c * PA + i] = 0.f;  // a tap out of frame is not ok: its weight is never looked up
        }
        keys[i] = k;
    }
    if (GUIDED && tid < 128) med_lds[PA * (1 + C) + tid] = wt.w[tid];
    __syncthreads();

    const int lx = tid & 63, x = x0 + lx;
#pragma unroll 1
    for (int j = 0; j < MED_ROWS; ++j) {
        const int ly = (tid >> 6) * MED_ROWS + j, y = y0 + ly;
        if (y >= H || x >= W) continue;
        const unsigned* win = keys + ly * PW + lx;  // the window's top-left: the halo's R cancels the window's -R
        const unsigned centre = win[R * PW + R];
        const bool ok = centre != MED_BAD;
        unsigned sel = 0;
        bool produced = false;
        if (ok || fill_invalid) {
            if (R == 1 && !GUIDED) produced = med_select9(win, PW, min_count, sel);
            else if (R == 2 && !GUIDED) produced = med_select25(win, PW, min_count, sel);
            else if (med_in_registers(R, GUIDED)) produced = med_select<R, GUIDED>(win, PW, gl + ly * PW + lx, PA, C, inv_step, wtab, min_count, sel);
            else produced = med_select_rows<R, GUIDED>(win, PW, gl + ly * PW + lx, PA, C, inv_step, wtab, wts, MED_BLOCK, min_count, sel);
        }
        const unsigned out = produced ? med_unkey(sel) : ok ? med_unkey(centre) : __float_as_uint(fill);
        const long o = (long)b * per + (long)y * W + x;
        filtered[o] = __uint_as_float(out);
        if (mask_out) mask_out[o] = mask_byte(ok || produced, valid_is_one);
        if (changed) {
            const unsigned was = ok ? med_unkey(centre) : __float_as_uint(mp[(long)y * W + x]);
            changed[o] = (out != was || (!ok && produced)) ? 1 : 0;
        }
    }
}

template <int R, bool GUIDED>
static int med_launch(const float* map, long mbs, const unsigned char* mask, int pol, int min_count, int fill_invalid, float fill,
                      const float* guide, int C, float inv_step, const MedWeights& wt, float* filtered, unsigned char* mask_out,
                      unsigned char* changed, int B, int H, int W, hipStream_t s) {
    const int tx = cdiv(W, MED_TW), ty = cdiv(H, MED_TH);
    const size_t lds = med_lds_bytes(R, GUIDED, C);
    if (med_lds_bytes(R, GUIDED, MED_MAX_C) > 64 * 1024) {
        static std::atomic<unsigned> raised{0};
        int rc;
        NND_TRY(raise_lds_limit((const void*)median_kernel<R, GUIDED>, raised));
    }
    hipLaunchKernelGGL((median_kernel<R, GUIDED>), dim3((unsigned)(tx * ty), B), dim3(MED_BLOCK), lds, s, map, mbs, mask, pol, min_count,
                       fill_invalid, fill, guide, C, inv_step, wt, filtered, mask_out, changed, H, W, tx);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

}  // namespace nnd

using namespace nnd;

extern "C" {

int nnd_median_filter_limit(int which) {
    return which == 0 ? MED_MAX_R : which == 1 ? MED_TH : which == 2 ? MED_TW : (int)NND_ERR_INVALID;
}

int nnd_median_filter(const float* map, int64_t map_bstride, const unsigned char* mask, int mask_valid_is_one, int radius, int min_count,
                      int fill_invalid, float fill, const float* guide, int C, float inv_step, const uint16_t* weights, float* filtered,
                      unsigned char* mask_out, unsigned char* changed, int B, int H, int W, void* stream) {
    const char* what = "median_filter";
    NND_REQUIRE(map && filtered, "%s: null pointer: no map or no filtered map", what);
    NND_REQUIRE(filtered != map, "%s: the filtered map must not be the input map", what);
    int rc;
    NND_TRY(check_map(what, B, H, W, map_bstride));
    NND_REQUIRE((int64_t)H * W <= 0x7fffffff && (int64_t)B * H <= (1 << 25), "%s: bad shape (%d,1,%d,%d) (H*W < 2^31, B*H <= 2^25)", what,
                B, H, W);  // the grid's x holds the tiles of a sample: < 2^31; B*H as for the operations by rows (warp.hip)
    NND_REQUIRE(radius >= 1 && radius <= MED_MAX_R, "%s: radius %d is outside 1 .. %d (nnd_median_filter_limit)", what, radius, MED_MAX_R);
    const int taps = (2 * radius + 1) * (2 * radius + 1);
    NND_REQUIRE(min_count >= 1 && min_count <= taps, "%s: min_count %d is outside 1 .. %d = (2 radius + 1)^2", what, min_count, taps);
    const bool guided = guide != nullptr;
    NND_REQUIRE(guided == (C != 0) && guided == (weights != nullptr), "%s: null pointer: guide, weights and C = %d do not go together", what,
                C);
    MedWeights wt;
    std::memset(&wt, 0, sizeof(wt));
    if (guided) {
        NND_REQUIRE(C >= 1 && C <= MED_MAX_C, "%s: bad guide channels %d (1 <= C <= %d)", what, C, MED_MAX_C);
        NND_REQUIRE(inv_step > 0.f && inv_step <= 3.402823466e+38f, "%s: inv_step is not finite or not above 0", what);  // false for a NaN
        NND_REQUIRE(weights[0] != 0, "%s: weights[0] is 0: the centre tap must count", what);
        std::memcpy(wt.w, weights, sizeof(wt.w));
    }
    const hipStream_t s = (hipStream_t)stream;
#define MED_CASE(R)                                                                                                                      \
    case R:                                                                                                                              \
        return guided ? med_launch<R, true>(map, (long)map_bstride, mask, mask_valid_is_one != 0, min_count, fill_invalid != 0, fill,    \
                                            guide, C, inv_step, wt, filtered, mask_out, changed, B, H, W, s)                             \
                      : med_launch<R, false>(map, (long)map_bstride, mask, mask_valid_is_one != 0, min_count, fill_invalid != 0, fill,   \
                                             nullptr, 0, 1.f, wt, filtered, mask_out, changed, B, H, W, s);
    switch (radius) {
        MED_CASE(1)
        MED_CASE(2)
        MED_CASE(3)
        MED_CASE(4)
        MED_CASE(5)
        MED_CASE(6)
        MED_CASE(7)
    }
#undef MED_CASE
    return NND_ERR_INVALID;  // not reached: the radius was checked
}

}  // extern "C"
