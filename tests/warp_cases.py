"""The view warp and hole filling (csrc/warp.hip): vectorised numpy oracles of the two closed forms in include/nndepth_amd.h, and the
inputs of tests/test_warp_cpu.py, tests/test_gpu_warp.py and scripts/make_golden_warp.py.

Everything is float32: `np.rint` rounds ties to even as rintf does, `+ np.float32(0)` turns -0.0 into +0.0, every operation on
float32 arrays is one rounded fp32 operation.  The warp oracle picks a target's winner with a lexicographic sort (m descending,
then x ascending) and takes the first of every target; the loops of scripts/make_golden_warp.py say the same with a running
maximum, and test_warp_cpu.py holds the two against each other.

Random inputs come from numpy's PCG64, seeded per case (speckle_cases.rng)."""
import numpy as np

import speckle_cases as S

F32 = np.float32
bits = S.bits
SHAPES = S.SHAPES  # + (2, 1, 9, 2 * chunk + 3) for each chunk the library reports
RULES = ("min_abs", "max_abs", "nearest")
GOLDEN_SHAPE = (2, 1, 9, 40)


def valid_of(shape, mask=None, mask_is_valid=True) -> np.ndarray:
    if mask is None:
        return np.ones(shape, bool)
    m = np.asarray(mask).reshape(shape) != 0
    return m if mask_is_valid else ~m


# ------------------------------------------------------------------------------------------------------------------ the oracles
def warp_sources(d, disp_sign="negative", to_view="right", mask=None, mask_is_valid=True):
    """(m, t as int64 (0 where it does not land), lands) of every source pixel."""
    d = np.asarray(d)
    assert d.dtype == F32 and d.ndim == 4 and d.shape[1] == 1
    W = d.shape[3]
    with np.errstate(all="ignore"):
        m = (-d if disp_sign == "negative" else d) + F32(0)
        src_ok = valid_of(d.shape, mask, mask_is_valid) & np.isfinite(m) & (m >= 0)
        x = np.arange(W, dtype=F32)
        xr = x - m if to_view == "right" else x + m
        assert xr.dtype == F32
        t = np.rint(xr)
        lands = src_ok & (t >= F32(0)) & (t <= F32(W - 1))
    return m, np.where(lands, t, 0).astype(np.int64), lands


def warp(d, disp_sign="negative", to_view="right", threshold=1.0, mask=None, features=None, fill=0.0, mask_is_valid=True):
    """(disp_other fp32, valid_other uint8 in the polarity of the mask, occluded uint8, source int32, features_other or None)."""
    m, t, lands = warp_sources(d, disp_sign, to_view, mask, mask_is_valid)
    B, _, H, W = d.shape
    rows = np.broadcast_to(np.arange(B * H).reshape(B, 1, H, 1), d.shape)
    xs = np.broadcast_to(np.arange(W), d.shape)
    target = (rows * W + t)[lands]
    ml, xl = m[lands], xs[lands]
    order = np.lexsort((xl, -ml.astype(np.float64), target))  # by target, then m descending, then x ascending
    target, ml, xl = target[order], ml[order], xl[order]
    first = np.ones(target.size, bool)
    first[1:] = target[1:] != target[:-1]
    m_win = np.zeros(B * H * W, F32)
    source = np.full(B * H * W, -1, np.int32)
    m_win[target[first]] = ml[first]
    source[target[first]] = xl[first]
    won = source >= 0
    disp_other = np.where(won, -m_win if disp_sign == "negative" else m_win, F32(fill)).astype(F32).reshape(d.shape)
    with np.errstate(all="ignore"):
        gap = m_win[(rows * W + t).reshape(-1)].reshape(d.shape) - m
        occluded = ~(lands & (gap <= F32(threshold)))
    won, source = won.reshape(d.shape), source.reshape(d.shape)
    feats = None
    if features is not None:
        assert features.dtype == F32 and features.shape[0] == B and features.shape[2:] == (H, W)
        gather = np.broadcast_to(np.maximum(source, 0), features.shape).astype(np.int64)
        feats = np.where(np.broadcast_to(won, features.shape), np.take_along_axis(features, gather, axis=3), F32(0)).astype(F32)
    return disp_other, (won == bool(mask_is_valid)).astype(np.uint8), occluded.astype(np.uint8), source, feats


def _nearest_ok(ok, axis):
    """(index of the nearest set element at or before, at or after) along `axis`; -1 where there is none."""
    n = ok.shape[axis]
    shape = [1] * ok.ndim
    shape[axis] = n
    idx = np.arange(n).reshape(shape)
    before = np.maximum.accumulate(np.where(ok, idx, -1), axis=axis)
    after = np.flip(np.minimum.accumulate(np.flip(np.where(ok, idx, n), axis), axis=axis), axis)
    return before, np.where(after == n, -1, after)


def _choose(rule, va, vb, da, db, a, b):
    """True where the first neighbour (index a, value va, distance da) is taken; both may be missing (-1)."""
    with np.errstate(all="ignore"):
        first = {"min_abs": np.abs(va) <= np.abs(vb), "max_abs": np.abs(va) >= np.abs(vb), "nearest": da <= db}[rule]
    return np.where(b < 0, True, np.where(a < 0, False, first))


def fill_holes(d, mask=None, mask_is_valid=True, rule="min_abs", vertical=True, fill=0.0):
    """(filled fp32, was_filled uint8, mask_out uint8 in the polarity of the mask)."""
    d = np.asarray(d)
    assert d.dtype == F32 and d.ndim == 4 and d.shape[1] == 1 and rule in RULES
    B, _, H, W = d.shape
    ok = valid_of(d.shape, mask, mask_is_valid) & np.isfinite(d)
    x = np.broadcast_to(np.arange(W), d.shape)
    L, R = _nearest_ok(ok, 3)
    vL, vR = np.take_along_axis(d, np.maximum(L, 0), 3), np.take_along_axis(d, np.maximum(R, 0), 3)
    row = np.where(_choose(rule, vL, vR, x - L, R - x, L, R), vL, vR)
    nonempty = np.broadcast_to(ok.any(axis=3, keepdims=True), d.shape)
    out = np.where(nonempty, row, F32(fill)).astype(F32)
    has = nonempty.copy()
    if vertical:
        y = np.broadcast_to(np.arange(H).reshape(1, 1, H, 1), d.shape)
        U, D = _nearest_ok(nonempty, 2)
        vU, vD = np.take_along_axis(out, np.maximum(U, 0), 2), np.take_along_axis(out, np.maximum(D, 0), 2)
        col = np.where(_choose(rule, vU, vD, y - U, D - y, U, D), vU, vD)
        reach = ~nonempty & ((U >= 0) | (D >= 0))
        out = np.where(reach, col, out).astype(F32)
        has |= reach
    out = np.where(ok, d, out)  # ok pixels bit for bit (np.where on float32 copies bits)
    return out, (has & ~ok).astype(np.uint8), (has == bool(mask_is_valid)).astype(np.uint8)


def collisions(d, disp_sign="negative", to_view="right", mask=None, threshold=1.0):
    """Shares: targets with >= 2 sources, with >= 3, landed sources that are occluded, targets that are holes."""
    _, t, lands = warp_sources(d, disp_sign, to_view, mask)
    B, _, H, W = d.shape
    rows = np.broadcast_to(np.arange(B * H).reshape(B, 1, H, 1), d.shape)
    count = np.bincount((rows * W + t)[lands], minlength=d.size)
    occ = warp(d, disp_sign, to_view, threshold, mask)[2] != 0
    return {"two": float((count >= 2).mean()), "three": float((count >= 3).mean()),
            "occluded_of_landed": float(occ[lands].mean()) if lands.any() else 0.0, "holes": float((count == 0).mean())}


# ----------------------------------------------------------------------------------------------------------------- the inputs
def scene(shape, seed, disp_sign="negative"):
    """(d, valid mask): speckle_cases.scene (two slanted planes, a foreground box, salt, blobs; 10 % masked out) as magnitudes."""
    d, mask, _ = S.scene(shape, seed)
    return (-d if disp_sign == "negative" else d), mask


def half_integer(shape, k=0.5):
    """A constant magnitude k + integer: every x -+ m is a tie; (positive sign)"""
    return np.full(shape, k, F32)


def special(W=24):
    """(1,1,3,W) in the positive sign: -0.0, NaN, +-inf and negative (wrong-sign) values among finite ones."""
    d = np.full((1, 1, 3, W), 2.0, F32)
    d[0, 0, 0, ::4] = [-0.0, np.nan, np.inf, -np.inf, -1.0, 0.0][:len(d[0, 0, 0, ::4])]
    d[0, 0, 1] = 0.0
    d[0, 0, 1, 1::3] = -0.0
    d[0, 0, 2, 5:9] = np.nan
    d[0, 0, 2, 12] = -3.0
    return d


BAR_THRESHOLD = 3.0


def bar(threshold=BAR_THRESHOLD, ulp=False, shape=(1, 1, 3, 40)):
    """A background of magnitude 4 and a foreground bar exactly `threshold` nearer (ulp: the next float above that), positive sign:
    going right, the bar takes the targets of the `threshold` background pixels to its left, which are exactly within the
    threshold, or one ulp beyond it."""
    d = np.full(shape, 4.0, F32)
    near = F32(4.0) + F32(threshold)
    d[..., 20:25] = np.nextafter(near, F32(np.inf)) if ulp else near
    return d


def holes(shape, seed, share=0.2):
    """(d, valid mask): signed values, `share` holes in runs, NaNs among the valid ones, and (H >= 5) some rows without a valid pixel."""
    g = S.rng(seed)
    B, _, H, W = shape
    d = g.uniform(-20.0, 20.0, shape).astype(F32)
    run = g.random(shape) < share / 3
    mask = ~(run | np.roll(run, 1, 3) | np.roll(run, 2, 3) | (g.random(shape) < share / 4))
    d[g.random(shape) < 0.01] = np.nan
    if H >= 5:
        mask[:, :, g.integers(0, H, max(1, H // 6))] = False
    return d, mask


def fill_pattern(chunk, seed=3):
    """(2,1,12,2*chunk+3): sample 0 row by row: 0 empty (top); 1 a hole run at the row's start; 2 at its end; 3 across the chunk
    border; 4 one ok pixel; 5, 6 empty between filled rows; 7 equal |v| of opposite signs around the holes; 8 NaN / inf as holes;
    9 random; 10, 11 empty (bottom).  Sample 1 has nothing valid."""
    g = S.rng(seed)
    W = 2 * chunk + 3
    d = g.uniform(-9.0, 9.0, (2, 1, 12, W)).astype(F32)
    mask = np.ones(d.shape, bool)
    mask[0, 0, [0, 5, 6, 10, 11]] = False
    mask[0, 0, 1, :5] = False
    mask[0, 0, 2, W - 4:] = False
    mask[0, 0, 3, chunk - 3:chunk + 2] = False
    mask[0, 0, 3, 2 * chunk - 1:2 * chunk + 1] = False
    mask[0, 0, 4] = False
    mask[0, 0, 4, chunk + 1] = True
    d[0, 0, 7] = np.where(np.arange(W) % 8 < 4, 2.5, -2.5)
    mask[0, 0, 7, 3::8] = False
    mask[0, 0, 7, 4::8] = False
    d[0, 0, 8, 2:6] = np.nan
    d[0, 0, 8, chunk] = np.inf
    d[0, 0, 8, W - 1] = -np.inf
    mask[0, 0, 9] = g.random(W) < 0.5
    mask[1] = False
    d[1, 0, 3, 3] = np.nan
    return d, mask
