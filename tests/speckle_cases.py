"""Connected regions and the speckle filter (csrc/speckle.hip): a plain-numpy oracle of the closed form in include/nndepth_amd.h,
and the input patterns of tests/test_speckle_cpu.py, tests/test_gpu_speckle.py and scripts/make_golden_speckle.py.

The oracle is hook-and-compress on the edge list: every round lowers the label of each root to the smallest label across its
edges (np.minimum.at: every update is min(old, new), so labels only decrease), then jumps pointers until every pixel points to a
root.  It stops when both ends of every edge carry one label; that label is the smallest index of the component because a label
is always the index of a pixel of the same component and never exceeds the pixel's own.  test_speckle_cpu.py checks it against
scipy.sparse.csgraph.connected_components.

Random inputs come from numpy's PCG64, seeded per case."""
import functools

import numpy as np

F32 = np.float32
GOLDEN_TILE = (32, 64)  # the tile the patterns of tests/golden/speckle.npz were laid out for (nnd_connected_regions_tile)
GOLDEN_SHAPE = (70, 200)
SHAPES = [(1, 1, 1, 1), (2, 1, 1, 9), (2, 1, 9, 1), (2, 1, 5, 7), (1, 1, 33, 130), (3, 1, 70, 200)]  # + 2 * tile + 3, from the library


def rng(seed: int) -> np.random.Generator:
    return np.random.Generator(np.random.PCG64(seed))


def bits(a) -> np.ndarray:
    """The bit patterns of fp32 values: what "bit for bit" compares (warp_cases and median_cases use it under their own names)."""
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ the oracle
def valid_of(d: np.ndarray, mask=None, mask_is_valid: bool = True) -> np.ndarray:
    ok = np.isfinite(d)
    if mask is not None:
        m = np.asarray(mask).reshape(d.shape) != 0
        ok &= m if mask_is_valid else ~m
    return ok


def edges_of(d: np.ndarray, valid: np.ndarray, max_diff: float, connectivity: int = 4):
    """(p, q): the flat indices of the joined pairs of ONE (H,W) fp32 map; |d[p] - d[q]| is one fp32 subtraction."""
    assert d.dtype == F32 and d.ndim == 2 and connectivity in (4, 8)
    H, W = d.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    md = F32(max_diff)
    ps, qs = [], []

    def pairs(a, b):  # two views of the same shape: a = the pixel, b = its neighbour
        with np.errstate(all="ignore"):
            join = valid[a] & valid[b] & (np.abs(d[a] - d[b]) <= md)
        ps.append(idx[a][join])
        qs.append(idx[b][join])

    s = slice(None)
    pairs((s, slice(0, W - 1)), (s, slice(1, W)))  # right
    pairs((slice(0, H - 1), s), (slice(1, H), s))  # down
    if connectivity == 8:
        pairs((slice(0, H - 1), slice(0, W - 1)), (slice(1, H), slice(1, W)))  # down-right
        pairs((slice(0, H - 1), slice(1, W)), (slice(1, H), slice(0, W - 1)))  # down-left
    return np.concatenate(ps), np.concatenate(qs)


def components(n: int, p: np.ndarray, q: np.ndarray) -> np.ndarray:
    """label[i] = the smallest index of i's component in the graph of n nodes with edges (p, q)."""
    L = np.arange(n, dtype=np.int64)
    while True:
        a, b = L[p], L[q]
        if np.array_equal(a, b):
            return L
        m = np.minimum(a, b)
        np.minimum.at(L, a, m)  # min(old, new): monotone
        np.minimum.at(L, b, m)
        while True:
            L2 = L[L]
            if np.array_equal(L2, L):
                break
            L = L2


def regions(d, max_diff, mask=None, mask_is_valid=True, connectivity=4):
    """(labels, sizes) int32 of d's shape (B,1,H,W)."""
    d = np.asarray(d)
    assert d.dtype == F32 and d.ndim == 4 and d.shape[1] == 1
    B, _, H, W = d.shape
    ok = valid_of(d, mask, mask_is_valid)
    labels = np.full(d.shape, -1, np.int32)
    sizes = np.zeros(d.shape, np.int32)
    for b in range(B):
        v = ok[b, 0]
        p, q = edges_of(d[b, 0], v, max_diff, connectivity)
        L = components(H * W, p, q).reshape(H, W)
        count = np.bincount(L[v], minlength=H * W)
        labels[b, 0][v] = L[v]
        sizes[b, 0][v] = count[L[v]]
    return labels, sizes


def speckle_filter(d, max_size, max_diff, mask=None, mask_is_valid=True, connectivity=4, fill=0.0):
    """(filtered, mask_out uint8 in the polarity of the input mask, speckle uint8, sizes)."""
    _, sizes = regions(d, max_diff, mask, mask_is_valid, connectivity)
    ok = valid_of(d, mask, mask_is_valid)
    speckle = ok & (sizes <= max_size)
    filtered = d.copy()
    filtered[speckle] = F32(fill)
    keep = ok & ~speckle
    return filtered, (keep if mask_is_valid else ~keep).astype(np.uint8), speckle.astype(np.uint8), sizes


def regions_scipy(d, max_diff, mask=None, mask_is_valid=True, connectivity=4):
    """The same through scipy's connected_components (its labels are renamed to the smallest index of each component)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    B, _, H, W = d.shape
    ok = valid_of(d, mask, mask_is_valid)
    labels = np.full(d.shape, -1, np.int32)
    sizes = np.zeros(d.shape, np.int32)
    for b in range(B):
        p, q = edges_of(d[b, 0], ok[b, 0], max_diff, connectivity)
        graph = coo_matrix((np.ones(p.size, np.int8), (p, q)), shape=(H * W, H * W))
        n, comp = connected_components(graph, directed=False)
        first = np.full(n, H * W, np.int64)
        np.minimum.at(first, comp, np.arange(H * W))
        count = np.bincount(comp, minlength=n)
        v = ok[b, 0].reshape(-1)
        labels[b, 0].reshape(-1)[v] = first[comp][v]
        sizes[b, 0].reshape(-1)[v] = count[comp][v]
    return labels, sizes


# ---------------------------------------------------------------------------------------------------------------- the patterns
# A pattern is (d (B,1,H,W) fp32, mask (B,1,H,W) bool with True = valid, or None, max_diff).
BG = F32(100.0)  # a value no pattern's foreground joins


def quantised(shape, seed):
    """0.5 * U{0..5}, 80 % valid, max_diff 0.5: many small regions."""
    g = rng(seed)
    d = (g.integers(0, 6, shape) * 0.5).astype(F32)
    return d, g.random(shape) < 0.8, 0.5


def _dilate(m):
    out = m.copy()
    out[..., 1:, :] |= m[..., :-1, :]
    out[..., :-1, :] |= m[..., 1:, :]
    out[..., :, 1:] |= out[..., :, :-1].copy()
    out[..., :, :-1] |= out[..., :, 1:].copy()
    return out


def scene(shape, seed, max_diff=0.5):
    """Two slanted planes (a background and a foreground box 10 above it), 6 % salt noise, 3x3 blobs 5 above their plane, 10 % holes."""
    g = rng(seed)
    B, _, H, W = shape
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    back = 4.0 + 0.02 * x + 0.01 * y
    d = np.broadcast_to(back, shape).copy()
    box = (slice(None), slice(None), slice(H // 4, H // 4 + H // 2), slice(W // 3, W // 3 + W // 3))
    d[box] += 10.0 + 0.03 * y[box[2:]]
    blobs = _dilate(g.random(shape) < 0.003)
    d[blobs] += 5.0
    salt = g.random(shape) < 0.06
    d[salt] += g.uniform(3.0, 20.0, int(salt.sum()))
    return d.astype(F32), g.random(shape) >= 0.10, max_diff


def serpentine(H, W, lo, hi, vertical=False):
    """One path of 1.0 on BG: every second row between columns lo..hi, joined alternately at hi and at lo (transposed: columns)."""
    if vertical:
        d, _, md = serpentine(W, H, lo, hi)
        return np.ascontiguousarray(d.transpose(0, 1, 3, 2)), None, md
    d = np.full((1, 1, H, W), BG, F32)
    d[0, 0, 0::2, lo:hi + 1] = 1.0
    turn = hi
    for r in range(1, H - 1, 2):
        d[0, 0, r, turn] = 1.0
        turn = lo if turn == hi else hi
    return d, None, 0.5


def spiral(H, W):
    """A square spiral of 1.0 on BG, one pixel of BG between its arms."""
    on = np.zeros((H, W), bool)
    y = x = 0
    dy, dx = 0, 1
    on[0, 0] = True

    def free(yy, xx):
        return not (0 <= yy < H and 0 <= xx < W) or not on[yy, xx]

    while True:
        for _ in range(2):
            ny, nx = y + dy, x + dx
            if 0 <= ny < H and 0 <= nx < W and not on[ny, nx] and free(ny + dy, nx + dx):
                y, x = ny, nx
                on[y, x] = True
                break
            dy, dx = dx, -dy
        else:
            break
    d = np.where(on, F32(1.0), BG).astype(F32)
    return d[None, None], None, 0.5


def checkerboard(shape):
    """Valid where (x + y) is even: every pixel alone with 4 neighbours, one region with 8."""
    _, _, H, W = shape
    y, x = np.mgrid[0:H, 0:W]
    return np.ones(shape, F32), np.broadcast_to((x + y) % 2 == 0, shape).copy(), 0.5


def corner_rings(H, W, th, tw):
    """Sample 0: a square ring of 1.0 on BG around the tile corner (th, tw).  Sample 1: a diamond |dy| + |dx| == 3 around the same
    corner on an invalid background: joined by diagonals only, two of which cross the corner's tiles."""
    d = np.full((2, 1, H, W), BG, F32)
    mask = np.ones((2, 1, H, W), bool)
    cy, cx = min(th, H - 4), min(tw, W - 4)
    d[0, 0, cy - 2:cy + 2, cx - 2:cx + 2] = 1.0
    d[0, 0, cy - 1:cy + 1, cx - 1:cx + 1] = BG
    y, x = np.mgrid[0:H, 0:W]
    mask[1, 0] = np.abs(y - cy) + np.abs(x - cx) == 3
    return d, mask, 0.5


def lines(H, W, th, tw):
    """A row on a tile's last row, a column on a tile's first column, both diagonals; each its own value on an invalid background."""
    d = np.zeros((1, 1, H, W), F32)
    mask = np.zeros((1, 1, H, W), bool)
    y, x = np.mgrid[0:H, 0:W]
    for value, on in ((1.0, y == min(th, H) - 1), (3.0, x == min(tw, W - 1)), (5.0, y == x), (7.0, y + x == min(H, W) - 1)):
        d[0, 0][on] = value
        mask[0, 0] |= on
    return d, mask, 0.5


def constant(shape):
    return np.full(shape, 2.5, F32), None, 0.0


def ramp(shape, exact=True):
    """Rows 1000 apart, columns 0.5 apart: a difference of exactly max_diff joins (one region per row); with max_diff one ulp
    below the step, nothing does."""
    _, _, H, W = shape
    y, x = np.mgrid[0:H, 0:W]
    d = np.broadcast_to((1000.0 * y + 0.5 * x).astype(F32), shape).copy()
    return d, None, 0.5 if exact else float(np.nextafter(F32(0.5), F32(0)))


def sized_bars(H, W, tw, n):
    """Bars of n and of n + 1 pixels (one of each across a tile's vertical border where the map is wide enough), BG between."""
    d = np.full((1, 1, H, W), BG, F32)
    x0 = max(0, min(tw - n // 2, W - n - 1))
    d[0, 0, 1, x0:x0 + n] = 1.0
    d[0, 0, 3, x0:x0 + n + 1] = 1.0
    d[0, 0, 5:5 + n, 2] = 1.0
    d[0, 0, 5:5 + n + 1, 4] = 1.0
    return d, None, 0.5


def special(max_diff):
    """(1,1,4,12): NaN and +-inf between finite values, +-3e38 pairs (their difference overflows), -0.0 beside 0.0, and 1.0 beside
    1.5 (a difference of exactly 0.5) and beside the next float above 1.5."""
    big = F32(3e38)
    up = np.nextafter(F32(1.5), F32(2))
    rows = [[1.0, np.nan, 1.0, np.inf, 1.0, -np.inf, 1.0, 1.0, BG, -0.0, 0.0, BG],
            [big, -big, BG, big, big, BG, -big, -big, BG, np.inf, np.inf, BG],
            [1.0, 1.5, BG, 1.0, up, BG, 1.5, 1.0, BG, up, 1.0, BG],
            [np.nan, np.nan, 0.0, -0.0, -0.0, 0.0, BG, -BG, BG, -BG, np.nan, 0.0]]
    return np.array(rows, F32)[None, None], None, max_diff


def all_invalid(shape):
    d = np.full(shape, np.nan, F32)
    d[0, 0, 0, 0] = 1.0
    mask = np.ones(shape, bool)
    mask[0, 0, 0, 0] = False
    return d, mask, 0.5


def slow_patterns(th, tw, H=GOLDEN_SHAPE[0], W=GOLDEN_SHAPE[1]):
    """The long-path patterns whose expected results tests/golden/speckle.npz holds (for GOLDEN_TILE and GOLDEN_SHAPE)."""
    return {
        "serp_h_full": serpentine(H, W, 0, W - 1),
        "serp_h_border": serpentine(H, W, tw - 1, min(2 * tw, W - 1)),  # turns in the last column of one tile and the first of another
        "serp_h_inner": serpentine(H, W, tw, min(2 * tw - 1, W - 1)),   # ... in the first and the last column of ONE tile
        "serp_v_full": serpentine(H, W, 0, H - 1, vertical=True),
        "serp_v_border": serpentine(H, W, th - 1, min(2 * th, H - 1), vertical=True),
        "spiral": spiral(H, W),
        "scene": scene((1, 1, H, W), 77),
    }


@functools.lru_cache(maxsize=None)
def oracle_regions(key, connectivity):
    """Shared, computed once per (pattern key, connectivity): key = (name, th, tw) of `slow_patterns`."""
    name, th, tw = key
    d, mask, md = slow_patterns(th, tw)[name]
    return regions(d, md, mask, True, connectivity)
