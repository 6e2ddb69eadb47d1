// Connected regions of a disparity / depth map on the device, and the speckle filter built on them: what a caller does after the
// left-right check (geometry.hip), without the map going back to the host for a labelling pass.  Beyond the reference, which has
// no such step.  The contract is a closed form (include/nndepth_amd.h): two neighbouring pixels are joined iff both are valid and
// fabsf(d[p] - d[q]) <= max_diff, one rounded fp32 subtraction; a region is a connected component of that graph; its label is the
// smallest row-major index in it.  Built with -ffp-contract=off like geometry.hip; all results are integers or copied bits.
//
// Four launches, whatever the data (no host synchronisation, no flag that the host polls: the call can be captured into a graph):
//   1 cc_tile_kernel   one workgroup per 32 x 64 tile.  The float comparison is evaluated HERE and nowhere else: a byte per
//                      pixel (right, down, down-right, down-left, valid) goes to the workspace and every later step reads it.
//                      Rows are labelled by runs (one wave = one tile row: a ballot gives every lane the start of its run), the
//                      runs are joined by a union-find in LDS (atomicMin on the roots), and the pixels of every tile-local root
//                      are counted in LDS.  Out: parent[p] = the tile-local root as an index of the sample (-1: invalid),
//                      total[p] = that count at a tile-local root and 0 elsewhere.
//   2 cc_merge_kernel  the edges whose two pixels lie in different tiles, the diagonals across a tile corner among them: lock-free
//                      unions over `parent` with atomicMin.  Labels that another workgroup may change are read with relaxed
//                      agent-scope atomic loads: a plain load may be served from this CU's L1 or from another XCD's stale copy.
//   3 cc_count_kernel  `parent` is final and read-only from here on (a phase boundary is a kernel boundary).  Every tile-local
//                      root that is not the root of its region adds its count onto the region's root: ONE integer atomicAdd per
//                      tile-local root.
//   4 cc_apply_kernel  the flatten pass: per pixel label = find(parent), size = total[label]; the speckle test, the filtered map
//                      and the masks.
// Only integer atomics (min, add): their results do not depend on the order of arrival, so the bytes are the same on every run.
//
// Termination.  parent[x] <= x holds when launch 1 has written it (a tile-local root is the smallest index of its part) and every
// later write is an atomicMin with a smaller value: labels only decrease.  So a `find` walks a strictly decreasing chain and ends
// after at most H*W steps.  A `union` that loses its atomicMin (another thread lowered the root first) goes on with the value it
// read back, which is smaller than the root it tried: the larger of its two indices strictly decreases from one attempt to the
// next, at most H*W attempts.  No thread ever waits for another workgroup: every iteration does work of its own.  The loops carry
// those bounds as hard caps all the same and leave when one is hit: on a shared machine a wrong answer that a test catches is
// preferred to a hang.
//
// Bounds.  A tile kernel thread touches global memory only at (y, x) with y < H and 0 <= x < W, checked where the index is formed.
// An edge bit is only ever set between two pixels inside the image (a pixel outside it is staged as "invalid"), so the neighbour
// index a set bit leads to needs no second check.  Labels are indices of valid pixels of the sample, or -1, which is never followed.
#include "map_ops.h"  // the contract of map, stride, mask and its polarity, in and out

namespace nnd {

constexpr int CC_TH = 32, CC_TW = 64;            // the tile: one wave (64 lanes) per row
constexpr int CC_BLOCK = 256, CC_WAVES = CC_BLOCK / 64;
constexpr int CC_ROWS = CC_TH / CC_WAVES;        // tile rows per wave
constexpr int CC_PIX = CC_TH * CC_TW;
constexpr int CC_VW = CC_TW + 2, CC_VH = CC_TH + 1;  // the staged values: one column left and right, one row below
static_assert(CC_TW == 64, "a tile row is one wave: the run labelling is a 64-bit ballot");

enum : unsigned { E_RIGHT = 1, E_DOWN = 2, E_DR = 4, E_DL = 8, E_VALID = 16, E_ROOT = 32 };

// ---- union-find in LDS (launch 1).  Other waves of the workgroup lower labels meanwhile: relaxed atomic loads, workgroup scope.
// The map of these loops is the tile: their cap is its pixel count.
__device__ __forceinline__ int lds_find(const int* lab, int x) {
    for (int n = 0; n < CC_PIX; ++n) {
        const int q = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (q == x) break;
        x = q;
    }
    return x;
}

__device__ __forceinline__ void lds_union(int* lab, int a, int b) {
    for (int n = 0; n < CC_PIX; ++n) {
        a = lds_find(lab, a);
        b = lds_find(lab, b);
        if (a == b) return;
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        const int old = __hip_atomic_fetch_min(lab + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) return;  // a was still a root: it now points to b
        a = old;               // someone lowered it first: whatever it pointed to must end up joined with b as well
    }
}

// ---- union-find over `parent` in global memory (launch 2): another workgroup may lower any label at any time
__device__ __forceinline__ int live_find(const int* parent, int x, long cap) {
    for (long n = 0; n < cap; ++n) {
        const int q = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (q == x) break;
        x = q;
    }
    return x;
}

__device__ __forceinline__ void live_union(int* parent, int a, int b, long cap) {
    for (long n = 0; n < cap; ++n) {
        a = live_find(parent, a, cap);
        b = live_find(parent, b, cap);
        if (a == b) return;
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}

// `parent` no longer changes (launches 3 and 4): plain loads
__device__ __forceinline__ int frozen_find(const int* __restrict__ parent, int x, long cap) {
    for (long n = 0; n < cap; ++n) {
        const int q = parent[x];
        if (q == x) break;
        x = q;
    }
    return x;
}

// launch 1.  grid (tiles in x, tiles in y, B)
__global__ void __launch_bounds__(CC_BLOCK) cc_tile_kernel(const float* __restrict__ map, long mbs, const unsigned char* __restrict__ mask,
                                                           int valid_is_one, float max_diff, int eight, int* __restrict__ parent,
                                                           int* __restrict__ total, unsigned char* __restrict__ edges, int H, int W) {
    __shared__ float val[CC_VH * CC_VW];  // the value of a valid pixel of the image, NaN for everything else
    __shared__ int lab[CC_PIX];
    __shared__ int cnt[CC_PIX];
    __shared__ unsigned char edg[CC_PIX];
    __shared__ unsigned long long row_right[CC_TH], row_down[CC_TH];  // per tile row: the lanes with a right / a down edge
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int x0 = blockIdx.x * CC_TW, y0 = blockIdx.y * CC_TH;
    const long per = (long)H * W, base = (long)blockIdx.z * per;
    const float* m = map + (long)blockIdx.z * mbs;

    for (int i = t; i < CC_VH * CC_VW; i += CC_BLOCK) {
        const int vy = i / CC_VW, vx = i - vy * CC_VW;
        const int y = y0 + vy, x = x0 + vx - 1;
        float v = NAN;
        if (x >= 0 && x < W && y < H) {
            const long p = (long)y * W + x;
            const float d = m[p];
            if (map_ok(d, mask, base + p, valid_is_one)) v = d;
        }
        val[i] = v;
    }
    for (int i = t; i < CC_PIX; i += CC_BLOCK) cnt[i] = 0;
    __syncthreads();

    // the edge bits, once; and the run of every pixel along its row.  A comparison with a NaN is false: no edge to an invalid pixel.
    for (int k = 0; k < CC_ROWS; ++k) {
        const int ly = k * CC_WAVES + wave, i = ly * CC_TW + lane;
        const float* c = val + ly * CC_VW + lane + 1;
        const float a = c[0];
        const bool ok = a == a;
        unsigned e = 0;
        if (ok) {
            e = E_VALID;
            if (fabsf(a - c[1]) <= max_diff) e |= E_RIGHT;
            if (fabsf(a - c[CC_VW]) <= max_diff) e |= E_DOWN;
            if (eight) {
                if (fabsf(a - c[CC_VW + 1]) <= max_diff) e |= E_DR;
                if (fabsf(a - c[CC_VW - 1]) <= max_diff) e |= E_DL;
            }
        }
        edg[i] = (unsigned char)e;
        const unsigned long long rb = __ballot((e & E_RIGHT) != 0), db = __ballot((e & E_DOWN) != 0);
        if (lane == 0) {
            row_right[ly] = rb;
            row_down[ly] = db;
        }
        // lane l continues a run iff lane l-1 has a right edge; lane 63's right edge leaves the tile and is shifted out
        const unsigned long long starts = ~(rb << 1);
        const unsigned long long at_or_below = starts & ((2ull << lane) - 1ull);  // never 0: lane 0 is a start
        lab[i] = ok ? ly * CC_TW + (63 - __builtin_clzll(at_or_below)) : -1;
    }
    __syncthreads();

    // the edges to the row below, inside the tile.  One that closes a square or a triangle of edges already taken is skipped:
    //   down(x)        is implied by  left(x), down(x-1) and the right edge of (x-1, y+1)
    //   down-right(x)  by down(x) and the right edge of (x, y+1), or by right(x) and down(x+1)
    //   down-left(x)   by down(x) and the right edge of (x-1, y+1), or by left(x) and down(x-1)
    // (a skipped down edge leans on the down edge one lane to its left, so the chain ends at a lane that does take its own).
    const unsigned long long in_tile = ~(1ull << 63);
    for (int k = 0; k < CC_ROWS; ++k) {
        const int ly = k * CC_WAVES + wave, i = ly * CC_TW + lane;
        if (ly == CC_TH - 1) continue;
        const unsigned e = edg[i];
        const unsigned long long rb = row_right[ly] & in_tile, db = row_down[ly], rbb = row_right[ly + 1] & in_tile;
        const bool down = (e & E_DOWN) != 0;
        const bool left = lane > 0 && ((rb >> (lane - 1)) & 1), left_down = lane > 0 && ((db >> (lane - 1)) & 1);
        const bool below_left_right = lane > 0 && ((rbb >> (lane - 1)) & 1);
        if (down && !(left && left_down && below_left_right)) lds_union(lab, i, i + CC_TW);
        if ((e & E_DR) && lane < 63) {
            const bool implied = (down && ((rbb >> lane) & 1)) || (((rb >> lane) & 1) && ((db >> (lane + 1)) & 1));
            if (!implied) lds_union(lab, i, i + CC_TW + 1);
        }
        if ((e & E_DL) && lane > 0) {
            const bool implied = (down && below_left_right) || (left && left_down);
            if (!implied) lds_union(lab, i, i + CC_TW - 1);
        }
    }
    __syncthreads();

    // flatten; the first lane of every run adds the run's length to its tile-local root
    int root[CC_ROWS];
    for (int k = 0; k < CC_ROWS; ++k) {
        const int ly = k * CC_WAVES + wave, i = ly * CC_TW + lane;
        const int l = lab[i];
        root[k] = l < 0 ? -1 : lds_find(lab, l);
        const unsigned long long starts = ~((row_right[ly] & in_tile) << 1);
        if (l >= 0 && ((starts >> lane) & 1)) {
            const unsigned long long above = starts & ~((2ull << lane) - 1ull);
            const int end = above ? __builtin_ctzll(above) : 64;
            atomicAdd(&cnt[root[k]], end - lane);
        }
    }
    __syncthreads();

    for (int k = 0; k < CC_ROWS; ++k) {
        const int ly = k * CC_WAVES + wave, i = ly * CC_TW + lane;
        const int y = y0 + ly, x = x0 + lane;
        if (x >= W || y >= H) continue;
        const long p = base + (long)y * W + x;
        const int r = root[k];
        const bool is_root = r == i;
        parent[p] = r < 0 ? -1 : (y0 + r / CC_TW) * W + x0 + r % CC_TW;
        total[p] = is_root ? cnt[i] : 0;
        edges[p] = (unsigned char)(edg[i] | (is_root ? E_ROOT : 0u));
    }
}

// launch 2.  One thread per pixel; only a pixel in the first or last column or the last row of its tile has an edge that leaves it.
__global__ void __launch_bounds__(CC_BLOCK) cc_merge_kernel(int* __restrict__ parent_all, const unsigned char* __restrict__ edges, int W,
                                                            long per) {
    const long i = (long)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (i >= per) return;
    const int y = (int)(i / W), x = (int)(i - (long)y * W);
    const int lx = x % CC_TW, ly = y % CC_TH;
    const bool first_col = lx == 0, last_col = lx == CC_TW - 1, last_row = ly == CC_TH - 1;
    if (!(first_col || last_col || last_row)) return;
    const long base = (long)blockIdx.y * per;
    const unsigned char* ed = edges + base + i;  // the bits of this pixel; a set bit says that the neighbour it names is in the image
    const unsigned e = ed[0];
    int* parent = parent_all + base;
    const int p = (int)i;
    // An edge that closes a square or a triangle of edges which are taken anyway is left out, as in launch 1 (on a flat border
    // one union per tile side remains).  A skipped right edge leans on the right edge one row up and on two down edges inside
    // the two tiles (ly > 0); a skipped down edge on the down edge one column to the left and on two right edges inside the two
    // tiles (lx > 0): each chain ends at the first row / column of the tile, which never skips, and no right edge leans on a down
    // edge of a border or the other way round.  A skipped diagonal leans on right and down edges only.
    if ((e & E_RIGHT) && last_col) {
        const bool implied = ly > 0 && (ed[-W] & E_RIGHT) && (ed[-W] & E_DOWN) && (ed[-W + 1] & E_DOWN);
        if (!implied) live_union(parent, p, p + 1, per);
    }
    if ((e & E_DOWN) && last_row) {
        const bool implied = lx > 0 && (ed[-1] & E_DOWN) && (ed[-1] & E_RIGHT) && (ed[W - 1] & E_RIGHT);
        if (!implied) live_union(parent, p, p + W, per);
    }
    if ((e & E_DR) && (last_col || last_row)) {
        const bool implied = ((e & E_DOWN) && (ed[W] & E_RIGHT)) || ((e & E_RIGHT) && (ed[1] & E_DOWN));
        if (!implied) live_union(parent, p, p + W + 1, per);
    }
    if ((e & E_DL) && (first_col || last_row)) {
        const bool implied = ((e & E_DOWN) && (ed[W - 1] & E_RIGHT)) || ((ed[-1] & E_RIGHT) && (ed[-1] & E_DOWN));
        if (!implied) live_union(parent, p, p + W - 1, per);
    }
}

// launch 3.  One integer add per tile-local root onto the root of its region.  total[] of a region's root is only added to, total[]
// of every other tile-local root is only read (by its own thread): the root itself takes no part.
__global__ void __launch_bounds__(CC_BLOCK) cc_count_kernel(const int* __restrict__ parent_all, int* __restrict__ total_all,
                                                            const unsigned char* __restrict__ edges, long per) {
    const long i = (long)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (i >= per) return;
    const long base = (long)blockIdx.y * per;
    if (!(edges[base + i] & E_ROOT)) return;
    const int r = frozen_find(parent_all + base, (int)i, per);
    if (r != (int)i) atomicAdd(total_all + base + r, total_all[base + i]);
}

// launch 4.  Every output is optional.
__global__ void __launch_bounds__(CC_BLOCK) cc_apply_kernel(const float* __restrict__ map, long mbs, const int* __restrict__ parent_all,
                                                            const int* __restrict__ total_all, const unsigned char* __restrict__ edges,
                                                            int valid_is_one, int max_size, float fill, int* __restrict__ labels,
                                                            int* __restrict__ sizes, float* __restrict__ filtered,
                                                            unsigned char* __restrict__ mask_out, unsigned char* __restrict__ speckle_out,
                                                            long per) {
    const long i = (long)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (i >= per) return;
    const long base = (long)blockIdx.y * per, p = base + i;
    const bool valid = (edges[p] & E_VALID) != 0;
    int label = -1, size = 0;
    if (valid) {
        label = frozen_find(parent_all + base, parent_all[p], per);
        size = total_all[base + label];
    }
    const bool speckle = valid && size <= max_size;
    if (labels) labels[p] = label;
    if (sizes) sizes[p] = size;
    if (filtered) {
        const float d = map[(long)blockIdx.y * mbs + i];
        filtered[p] = speckle ? fill : d;
    }
    if (speckle_out) speckle_out[p] = speckle ? 1 : 0;
    if (mask_out) {
        const bool keep = valid && !speckle;
        mask_out[p] = mask_byte(keep, valid_is_one);
    }
}

static int64_t cc_workspace_bytes(int64_t n) { return 8 * n + (n + 15) / 16 * 16; }  // parent, total: int32; the edge bytes

static int cc_check(const char* what, const float* map, int64_t bstride, float max_diff, int connectivity, const void* workspace,
                    int64_t workspace_bytes, int B, int H, int W) {
    int rc;
    NND_REQUIRE(map && workspace, "%s: null pointer", what);
    NND_TRY(check_map(what, B, H, W, bstride));
    NND_REQUIRE((int64_t)H * W <= 0x7fffffff, "%s: bad shape (%d,1,%d,%d): labels are int32, H*W < 2^31", what, B, H, W);
    NND_REQUIRE(cdiv(H, CC_TH) <= 65535, "%s: bad shape (%d,1,%d,%d): 65535 tile rows, H <= %d", what, B, H, W, 65535 * CC_TH);
    NND_REQUIRE(max_diff >= 0.f, "%s: max_diff is negative or NaN", what);  // false for a NaN
    NND_REQUIRE(connectivity == 4 || connectivity == 8, "%s: connectivity %d is neither 4 nor 8", what, connectivity);
    return check_workspace(what, workspace, workspace_bytes, cc_workspace_bytes((int64_t)B * H * W), 8);
}

static int cc_run(const float* map, int64_t bstride, const unsigned char* mask, int valid_is_one, float max_diff, int connectivity,
                  int max_size, float fill, int* labels, int* sizes, float* filtered, unsigned char* mask_out,
                  unsigned char* speckle_out, void* workspace, int B, int H, int W, hipStream_t s) {
    const long per = (long)H * W, n = (long)B * per;
    int* parent = (int*)workspace;
    int* total = parent + n;
    unsigned char* edges = (unsigned char*)(total + n);
    const dim3 flat((unsigned)cdiv64(per, CC_BLOCK), B);
    hipLaunchKernelGGL(cc_tile_kernel, dim3(cdiv(W, CC_TW), cdiv(H, CC_TH), B), dim3(CC_BLOCK), 0, s, map, (long)bstride, mask,
                       valid_is_one, max_diff, connectivity == 8, parent, total, edges, H, W);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_merge_kernel, flat, dim3(CC_BLOCK), 0, s, parent, (const unsigned char*)edges, W, per);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_count_kernel, flat, dim3(CC_BLOCK), 0, s, (const int*)parent, total, (const unsigned char*)edges, per);
    NND_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_apply_kernel, flat, dim3(CC_BLOCK), 0, s, map, (long)bstride, (const int*)parent, (const int*)total,
                       (const unsigned char*)edges, valid_is_one, max_size, fill, labels, sizes, filtered, mask_out, speckle_out, per);
    NND_LAUNCH_CHECK();
    return NND_OK;
}

}  // namespace nnd

using namespace nnd;

extern "C" {

int nnd_connected_regions_tile(int which) { return which == 0 ? CC_TH : which == 1 ? CC_TW : (int)NND_ERR_INVALID; }

int64_t nnd_connected_regions_workspace_bytes(int B, int H, int W) {
    if (!map_shape_ok(B, H, W) || (int64_t)H * W > 0x7fffffff) return (int64_t)NND_ERR_INVALID;
    return cc_workspace_bytes((int64_t)B * H * W);
}

int nnd_connected_regions(const float* map, int64_t map_bstride, const unsigned char* mask, int mask_valid_is_one, float max_diff,
                          int connectivity, int32_t* labels, int32_t* sizes, void* workspace, int64_t workspace_bytes, int B, int H,
                          int W, void* stream) {
    int rc;
    NND_TRY(cc_check("connected_regions", map, map_bstride, max_diff, connectivity, workspace, workspace_bytes, B, H, W));
    NND_REQUIRE(labels || sizes, "connected_regions: null pointer: neither labels nor sizes are asked for");
    return cc_run(map, map_bstride, mask, mask_valid_is_one != 0, max_diff, connectivity, 0, 0.f, labels, sizes, nullptr, nullptr,
                  nullptr, workspace, B, H, W, (hipStream_t)stream);
}

int nnd_speckle_filter(const float* map, int64_t map_bstride, const unsigned char* mask, int mask_valid_is_one, float max_diff,
                       int connectivity, int max_size, float fill, float* filtered, unsigned char* mask_out,
                       unsigned char* speckle_out, int32_t* sizes, void* workspace, int64_t workspace_bytes, int B, int H, int W,
                       void* stream) {
    int rc;
    NND_TRY(cc_check("speckle_filter", map, map_bstride, max_diff, connectivity, workspace, workspace_bytes, B, H, W));
    NND_REQUIRE(max_size >= 0, "speckle_filter: max_size %d is negative", max_size);
    NND_REQUIRE(filtered || mask_out || speckle_out, "speckle_filter: null pointer: no filtered map and no mask is asked for");
    return cc_run(map, map_bstride, mask, mask_valid_is_one != 0, max_diff, connectivity, max_size, fill, nullptr, sizes, filtered,
                  mask_out, speckle_out, workspace, B, H, W, (hipStream_t)stream);
}

}  // extern "C"
