// A disparity map seen from the other view, the occlusion that warp reveals, and hole filling: what a caller does after ONE forward
// where geometry.hip's left-right check needs two.  Beyond the reference, which has neither step.  The contracts are closed forms
// (include/nndepth_amd.h); every float step is one rounded fp32 operation (built with -ffp-contract=off like geometry.hip) and every
// result is an integer or a copy of input bits.
//
// nnd_warp_disparity: ONE launch, no workspace.  One workgroup per (sample, row): a row's targets depend on that row alone.
//   1  keys[t] = 0 for the W columns of the row in LDS (8 bytes per column)
//   2  every source x that lands on column t: atomicMax(keys[t], bits(m) << 32 | (W - x)) in LDS.  m >= 0 is finite, so its bits
//      order as the values do; W - x is 1 .. W, so the larger key among equal m is the smaller x and a key is never 0.  An integer
//      maximum does not depend on the order of arrival: the same bytes on every run.
//   3  after a barrier: column x as a TARGET reads keys[x] (winner or hole) and stores the other view's outputs; column x as a SOURCE
//      recomputes its own m and t (a handful of VALU operations, cheaper than keeping them) and compares with the winner of keys[t].
// The workgroup walks the row WARP_BLOCK columns per pass.  W <= WARP_MAX_W keeps the keys within the 64 KiB of dynamic LDS a
// kernel gets without raising its limit.
//
// nnd_fill_holes: THREE launches whatever the data, one wave per row in the first two.
//   1  fill_next_kernel   walks the row's chunks of 64 columns from the right: next[row][c] = the first ok column >= 64 c, or -1
//                         (a ballot per chunk, carried in a register).  next[row][0] < 0 says that the row is empty.
//   2  fill_row_kernel    walks the chunks from the left, the last ok column so far carried in a register: a ballot gives every lane
//                         its nearest ok column on either side inside the chunk, the carry and next[row][c + 1] those outside.  A wave
//                         whose row is empty looks for the nearest non-empty rows above and below instead, 64 rows per ballot.
//   3  fill_col_kernel    the pixels of the empty rows, from the row-pass results of those two rows.
// A phase boundary is a kernel boundary: nothing is read in the launch that wrote it, except by the lane that wrote it.
//
// Bounds.  Every global index is formed from (b, y, x) with b < B, y < H, x < W checked where it is formed; a column index read
// from the keys, from `next` or from a ballot is the index of a pixel of the row that was found ok, or is not followed (-1 / 0).
#include "map_ops.h"  // the contract of map, stride, mask and its polarity, in and out

namespace nnd {

constexpr int WARP_BLOCK = 256;    // columns per pass of a workgroup
constexpr int WARP_MAX_W = 8192;   // 8 bytes of LDS per column: 64 KiB
constexpr int FILL_CHUNK = 64;     // columns per step of a wave
constexpr int FILL_BLOCK = 256, FILL_WAVES = FILL_BLOCK / 64;
enum : int { RULE_MIN_ABS = 0, RULE_MAX_ABS = 1, RULE_NEAREST = 2 };

struct WarpSrc {
    float m;     // the magnitude, +0.0 for -0.0
    int t;       // the target column if `lands`
    bool lands;
};

__device__ __forceinline__ WarpSrc warp_source(const float* __restrict__ row, const unsigned char* __restrict__ mrow, int valid_is_one,
                                               int negative, int to_right, int x, int W) {
    WarpSrc s;
    const float d = row[x];
    s.m = (negative ? -d : d) + 0.0f;
    const bool src_ok = mask_valid(mrow, x, valid_is_one) && isfinite(s.m) && s.m >= 0.f;
    const float xr = to_right ? (float)x - s.m : (float)x + s.m;
    const float t = rintf(xr);  // ties to even
    s.lands = src_ok && t >= 0.0f && t <= (float)(W - 1);
    s.t = s.lands ? (int)t : 0;
    return s;
}

// grid (H, B); dynamic LDS: W keys
__global__ void __launch_bounds__(WARP_BLOCK) warp_row_kernel(const float* __restrict__ disp, long dbs, const unsigned char* __restrict__ mask,
                                                              int valid_is_one, int negative, int to_right, float threshold, float fill,
                                                              const float* __restrict__ features, int C, float* __restrict__ disp_other,
                                                              unsigned char* __restrict__ valid_other, unsigned char* __restrict__ occluded,
                                                              int* __restrict__ source, float* __restrict__ features_other, int H, int W) {
    extern __shared__ unsigned long long keys[];
    const int y = blockIdx.x, b = blockIdx.y;
    const long per = (long)H * W, o = (long)b * per + (long)y * W;
    const float* row = disp + (long)b * dbs + (long)y * W;
    const unsigned char* mrow = mask ? mask + o : nullptr;

    for (int x = threadIdx.x; x < W; x += WARP_BLOCK) keys[x] = 0ull;
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += WARP_BLOCK) {
        const WarpSrc s = warp_source(row, mrow, valid_is_one, negative, to_right, x, W);
        if (s.lands) atomicMax(&keys[s.t], ((unsigned long long)__float_as_uint(s.m) << 32) | (unsigned)(W - x));
    }
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += WARP_BLOCK) {
        // column x as a target
        const unsigned long long k = keys[x];
        const bool won = k != 0ull;
        const int xs = won ? W - (int)(unsigned)(k & 0xffffffffull) : -1;
        if (disp_other) {
            const float mw = __uint_as_float((unsigned)(k >> 32));
            disp_other[o + x] = won ? (negative ? -mw : mw) : fill;
        }
        if (valid_other) valid_other[o + x] = mask_byte(won, valid_is_one);
        if (source) source[o + x] = xs;
        if (features_other) {
            const long fo = (long)b * C * per + (long)y * W;
            for (int c = 0; c < C; ++c) features_other[fo + c * per + x] = won ? features[fo + c * per + xs] : 0.f;
        }
        // column x as a source
        if (occluded) {
            const WarpSrc s = warp_source(row, mrow, valid_is_one, negative, to_right, x, W);
            bool vis = false;
            if (s.lands) {
                const float mw = __uint_as_float((unsigned)(keys[s.t] >> 32));
                vis = (mw - s.m) <= threshold;
            }
            occluded[o + x] = vis ? 0 : 1;
        }
    }
}

// ---- fill
__device__ __forceinline__ bool fill_ok(const float* __restrict__ row, const unsigned char* __restrict__ mrow, int valid_is_one, int x, int W,
                                        float& v) {
    v = 0.f;
    if (x >= W) return false;
    v = row[x];
    return map_ok(v, mrow, x, valid_is_one);
}

// launch 1.  One wave per row, from the right.
__global__ void __launch_bounds__(FILL_BLOCK) fill_next_kernel(const float* __restrict__ map, long mbs, const unsigned char* __restrict__ mask,
                                                               int valid_is_one, int* __restrict__ next, int B, int H, int W, int nch) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * FILL_WAVES + (threadIdx.x >> 6);  // wave-uniform
    if (r >= (long)B * H) return;
    const int b = (int)(r / H), y = (int)(r - (long)b * H);
    const float* row = map + (long)b * mbs + (long)y * W;
    const unsigned char* mrow = mask ? mask + r * W : nullptr;
    int carry = -1;
    for (int c = nch - 1; c >= 0; --c) {
        float v;
        const unsigned long long bal = __ballot(fill_ok(row, mrow, valid_is_one, c * FILL_CHUNK + lane, W, v));
        if (bal) carry = c * FILL_CHUNK + __builtin_ctzll(bal);
        if (lane == 0) next[r * nch + c] = carry;
    }
}

// which of the two neighbours (a: left / up, at distance da; b: right / down, at distance db) a hole takes; ties go to a
__device__ __forceinline__ bool fill_takes_first(int rule, float va, float vb, int da, int db) {
    return rule == RULE_MIN_ABS ? fabsf(va) <= fabsf(vb) : rule == RULE_MAX_ABS ? fabsf(va) >= fabsf(vb) : da <= db;
}

__device__ __forceinline__ void fill_store(float* __restrict__ filled, unsigned char* __restrict__ was_filled, unsigned char* __restrict__ mask_out,
                                           int valid_is_one, long p, float v, bool copied, bool valid) {
    filled[p] = v;
    if (was_filled) was_filled[p] = copied ? 1 : 0;
    if (mask_out) mask_out[p] = mask_byte(valid, valid_is_one);
}

// launch 2.  One wave per row, from the left.  ud[row] = {nearest non-empty row above, below} (-1: none) for an empty row.
__global__ void __launch_bounds__(FILL_BLOCK) fill_row_kernel(const float* __restrict__ map, long mbs, const unsigned char* __restrict__ mask,
                                                              int valid_is_one, int rule, int vertical, const int* __restrict__ next,
                                                              int* __restrict__ ud, float* __restrict__ filled,
                                                              unsigned char* __restrict__ was_filled, unsigned char* __restrict__ mask_out, int B,
                                                              int H, int W, int nch) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * FILL_WAVES + (threadIdx.x >> 6);  // wave-uniform
    if (r >= (long)B * H) return;
    const int b = (int)(r / H), y = (int)(r - (long)b * H);
    if (next[r * nch] < 0) {  // an empty row
        int up = -1, down = -1;
        if (vertical) {
            const long r0 = (long)b * H;
            for (int base = y - 1; base >= 0; base -= 64) {
                const int q = base - lane;
                const unsigned long long bal = __ballot(q >= 0 && next[(r0 + q) * nch] >= 0);
                if (bal) {
                    up = base - __builtin_ctzll(bal);
                    break;
                }
            }
            for (int base = y + 1; base < H; base += 64) {
                const int q = base + lane;
                const unsigned long long bal = __ballot(q < H && next[(r0 + q) * nch] >= 0);
                if (bal) {
                    down = base + __builtin_ctzll(bal);
                    break;
                }
            }
        }
        if (lane == 0) {
            ud[2 * r] = up;
            ud[2 * r + 1] = down;
        }
        return;
    }
    const float* row = map + (long)b * mbs + (long)y * W;
    const unsigned char* mrow = mask ? mask + r * W : nullptr;
    int carry = -1;
    for (int c = 0; c < nch; ++c) {
        const int x = c * FILL_CHUNK + lane;
        float v;
        const bool ok = fill_ok(row, mrow, valid_is_one, x, W, v);
        const unsigned long long bal = __ballot(ok);
        const unsigned long long at_or_below = bal & ((2ull << lane) - 1ull), at_or_above = bal & ~((1ull << lane) - 1ull);
        const int L = at_or_below ? c * FILL_CHUNK + 63 - __builtin_clzll(at_or_below) : carry;
        const int R = at_or_above ? c * FILL_CHUNK + __builtin_ctzll(at_or_above) : (c + 1 < nch ? next[r * nch + c + 1] : -1);
        if (bal) carry = c * FILL_CHUNK + 63 - __builtin_clzll(bal);
        if (x >= W) continue;
        bool copied = false;
        if (!ok) {  // the row is not empty: L or R exists
            copied = true;
            if (L < 0) v = row[R];
            else if (R < 0) v = row[L];
            else {
                const float vl = row[L], vr = row[R];
                v = fill_takes_first(rule, vl, vr, x - L, R - x) ? vl : vr;
            }
        }
        fill_store(filled, was_filled, mask_out, valid_is_one, r * W + x, v, copied, true);
    }
}

// launch 3.  One thread per pixel; only the pixels of empty rows have work.
__global__ void __launch_bounds__(FILL_BLOCK) fill_col_kernel(int valid_is_one, int rule, float fill, const int* __restrict__ next,
                                                              const int* __restrict__ ud, float* __restrict__ filled,
                                                              unsigned char* __restrict__ was_filled, unsigned char* __restrict__ mask_out, int H,
                                                              int W, int nch, long per) {
    const long i = (long)blockIdx.x * FILL_BLOCK + threadIdx.x;
    if (i >= per) return;
    const int y = (int)(i / W), x = (int)(i - (long)y * W);
    const long r = (long)blockIdx.y * H + y, base = (long)blockIdx.y * per;
    if (next[r * nch] >= 0) return;
    const int up = ud[2 * r], down = ud[2 * r + 1];
    float v = fill;
    const bool copied = up >= 0 || down >= 0;
    if (up >= 0 && down >= 0) {
        const float vu = filled[base + (long)up * W + x], vd = filled[base + (long)down * W + x];
        v = fill_takes_first(rule, vu, vd, y - up, down - y) ? vu : vd;
    } else if (up >= 0) {
        v = filled[base + (long)up * W + x];
    } else if (down >= 0) {
        v = filled[base + (long)down * W + x];
    }
    fill_store(filled, was_filled, mask_out, valid_is_one, base + i, v, copied, copied);
}

// beyond check_map: a pixel index of a sample is an int, and a launch of one wave (or one workgroup) per row stays below 2^32 threads
static bool rows_ok(int B, int H, int W) { return (int64_t)H * W <= 0x7fffffff && (int64_t)B * H <= (1 << 25); }

static int64_t fill_workspace_bytes(int B, int H, int W) {  // next: a word per row and chunk; ud: two words per row
    const int64_t words = (int64_t)B * H * (cdiv(W, FILL_CHUNK) + 2);
    return (4 * words + 15) / 16 * 16;
}

}  // namespace nnd

using namespace nnd;

extern "C" {

int nnd_warp_disparity_limit(int which) { return which == 0 ? WARP_MAX_W : which == 1 ? WARP_BLOCK : (int)NND_ERR_INVALID; }

int nnd_warp_disparity(const float* disp, int64_t disp_bstride, const unsigned char* mask, int mask_valid_is_one, int negative,
                       int to_right, float threshold, float fill, const float* features, int C, float* disp_other,
                       unsigned char* valid_other, unsigned char* occluded, int32_t* source, float* features_other, int B, int H, int W,
                       void* stream) {
    const char* what = "warp_disparity";
    int rc;
    NND_REQUIRE(disp, "%s: null pointer: no map", what);
    NND_TRY(check_map(what, B, H, W, disp_bstride));
    NND_REQUIRE(rows_ok(B, H, W), "%s: bad shape (%d,1,%d,%d) (H*W < 2^31, B*H <= 2^25)", what, B, H, W);
    NND_REQUIRE(W <= WARP_MAX_W, "%s: a width of %d is above the maximum width %d (nnd_warp_disparity_limit)", what, W, WARP_MAX_W);
    NND_REQUIRE(threshold >= 0.f, "%s: threshold is negative or NaN", what);  // false for a NaN
    NND_REQUIRE(disp_other || valid_other || occluded || source || features_other, "%s: null pointer: no output is asked for", what);
    NND_REQUIRE(C >= 0 && (int64_t)C * H * W <= 0x7fffffff, "%s: bad feature channels %d (0 <= C, C*H*W < 2^31)", what, C);
    NND_REQUIRE((C > 0) == (features != nullptr) && (C > 0) == (features_other != nullptr),
                "%s: null pointer: features, features_other and C = %d do not go together", what, C);
    hipLaunchKernelGGL(warp_row_kernel, dim3(H, B), dim3(WARP_BLOCK), (size_t)W * 8, (hipStream_t)stream, disp, (long)disp_bstride, mask,
                       mask_valid_is_one != 0, negative != 0, to_right != 0, threshold, fill, features, C, disp_other, valid_other, occluded,
                       source, features_other, H, W);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

int nnd_fill_holes_chunk(void) { return FILL_CHUNK; }

int64_t nnd_fill_holes_workspace_bytes(int B, int H, int W) {
    if (!map_shape_ok(B, H, W) || !rows_ok(B, H, W)) return (int64_t)NND_ERR_INVALID;
    return fill_workspace_bytes(B, H, W);
}

int nnd_fill_holes(const float* map, int64_t map_bstride, const unsigned char* mask, int mask_valid_is_one, int rule, int vertical,
                   float fill, float* filled, unsigned char* was_filled, unsigned char* mask_out, void* workspace,
                   int64_t workspace_bytes, int B, int H, int W, void* stream) {
    const char* what = "fill_holes";
    NND_REQUIRE(map && workspace, "%s: null pointer: no map or no workspace", what);
    NND_REQUIRE(filled, "%s: null pointer: no filled map (the column pass reads it)", what);
    int rc;
    NND_TRY(check_map(what, B, H, W, map_bstride));
    NND_REQUIRE(rows_ok(B, H, W), "%s: bad shape (%d,1,%d,%d) (H*W < 2^31, B*H <= 2^25)", what, B, H, W);
    NND_REQUIRE(rule == RULE_MIN_ABS || rule == RULE_MAX_ABS || rule == RULE_NEAREST, "%s: unknown rule %d (0 min_abs, 1 max_abs, 2 nearest)",
                what, rule);
    NND_TRY(check_workspace(what, workspace, workspace_bytes, fill_workspace_bytes(B, H, W), 4));
    NND_REQUIRE(filled != map, "%s: the filled map must not be the input map", what);
    const hipStream_t s = (hipStream_t)stream;
    const int nch = cdiv(W, FILL_CHUNK);
    const long per = (long)H * W, rows = (long)B * H;
    int* next = (int*)workspace;
    int* ud = next + rows * nch;
    const dim3 by_row((unsigned)cdiv64(rows, FILL_WAVES));
    hipLaunchKernelGGL(fill_next_kernel, by_row, dim3(FILL_BLOCK), 0, s, map, (long)map_bstride, mask, mask_valid_is_one != 0, next, B, H, W, nch);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(fill_row_kernel, by_row, dim3(FILL_BLOCK), 0, s, map, (long)map_bstride, mask, mask_valid_is_one != 0, rule,
                       vertical != 0, (const int*)next, ud, filled, was_filled, mask_out, B, H, W, nch);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(fill_col_kernel, dim3((unsigned)cdiv64(per, FILL_BLOCK), B), dim3(FILL_BLOCK), 0, s, mask_valid_is_one != 0, rule, fill,
                       (const int*)next, (const int*)ud, filled, was_filled, mask_out, H, W, nch, per);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

}  // extern "C"
