"""CPU: the view warp and hole filling (csrc/warp.hip, nndepth_amd/geometry.py, the scene methods) without a GPU: the header, the
exports, the ctypes table and the Makefile rule agree; every entry point validates its arguments before any HIP call; Python
refuses by name what the kernels do not compute; the vectorised numpy oracle of tests/warp_cases.py equals the pixel loops of
scripts/make_golden_warp.py and reproduces tests/golden/warp_fill.npz, which those loops wrote."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import warp_cases as Wc
from cabi_checks import header_exports_ctypes_table_and_makefile_rule_agree, refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nnd_warp_disparity_limit", "nnd_warp_disparity", "nnd_fill_holes_chunk", "nnd_fill_holes_workspace_bytes", "nnd_fill_holes")


def _loops():
    spec = importlib.util.spec_from_file_location("make_golden_warp", os.path.join(ROOT, "scripts", "make_golden_warp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and (np.array_equal(Wc.bits(a), Wc.bits(b)) if a.dtype == np.float32 else np.array_equal(a, b))


def test_header_exports_ctypes_table_and_makefile_rule_agree():
    from nndepth_amd._lib import lib
    header_exports_ctypes_table_and_makefile_rule_agree(NAMES, "warp")
    assert lib.nnd_version() == 105


def test_limits_chunks_and_workspace_size():
    from nndepth_amd import geometry
    from nndepth_amd._lib import lib
    wmax, wchunk, fchunk = lib.nnd_warp_disparity_limit(0), lib.nnd_warp_disparity_limit(1), lib.nnd_fill_holes_chunk()
    assert wmax >= 8192 and 0 < wchunk <= wmax and fchunk > 0 and lib.nnd_warp_disparity_limit(2) < 0
    assert (geometry.warp_max_width(), geometry.warp_chunk(), geometry.fill_chunk()) == (wmax, wchunk, fchunk)
    words = lambda B, H, W: B * H * (-(-W // fchunk) + 2)  # noqa: E731  a word per row and chunk, two per row
    assert lib.nnd_fill_holes_workspace_bytes(2, 5, 7) == -(-4 * words(2, 5, 7) // 16) * 16
    assert geometry.fill_workspace_bytes(3, 70, 2 * fchunk + 3) == -(-4 * words(3, 70, 2 * fchunk + 3) // 16) * 16
    for bad in ((0, 5, 7), (2, 0, 7), (2, 5, -1), (70000, 5, 7), (1, 1 << 16, 1 << 16)):
        assert lib.nnd_fill_holes_workspace_bytes(*bad) < 0, bad


def test_entry_points_validate_before_any_device_call():
    from nndepth_amd._lib import lib
    one, big = C.c_void_p(16), C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first
    inf, nan = float("inf"), float("nan")
    wmax = lib.nnd_warp_disparity_limit(0)

    def warp(disp=one, bstride=35, mask=None, pol=1, neg=1, right=1, thr=1.0, fill=0.0, features=None, Cf=0, other=one, valid=one,
             occ=one, source=None, feats=None, B=1, H=5, W=7):
        return lib.nnd_warp_disparity(disp, bstride, mask, pol, neg, right, thr, fill, features, Cf, other, valid, occ, source, feats,
                                      B, H, W, None)

    def fill(map=one, bstride=35, mask=None, pol=1, rule=0, vertical=1, value=0.0, filled=big, was=None, mask_out=None, ws=big,
             ws_bytes=1 << 20, B=1, H=5, W=7):
        return lib.nnd_fill_holes(map, bstride, mask, pol, rule, vertical, value, filled, was, mask_out, ws, ws_bytes, B, H, W, None)

    refused(warp(disp=None), b"null")
    refused(fill(map=None), b"null")
    for f in (warp, fill):
        refused(f(B=0), b"shape")
        refused(f(B=70000), b"shape")
        refused(f(H=0), b"shape")
        refused(f(H=-1), b"shape")
        refused(f(W=0), b"shape")
        refused(f(W=-3), b"shape")
        refused(f(B=2, bstride=34), b"stride")
    refused(warp(H=1 << 16, W=1 << 16, bstride=1 << 32), b"shape")
    refused(fill(H=1 << 16, W=1 << 16, bstride=1 << 32, ws_bytes=1 << 40), b"shape")
    refused(warp(W=wmax + 1, bstride=5 * (wmax + 1)), b"maximum width")
    refused(warp(thr=nan), b"threshold")
    refused(warp(thr=-0.5), b"threshold")
    refused(warp(thr=-inf), b"threshold")
    refused(warp(other=None, valid=None, occ=None), b"null")
    refused(warp(features=one, Cf=3), b"null")  # no features_other
    refused(warp(feats=one, Cf=3), b"null")     # no features
    refused(warp(features=one, feats=one, Cf=0), b"null")
    refused(warp(Cf=-1), b"channels")
    for rule in (-1, 3, 99):
        refused(fill(rule=rule), b"rule")
    refused(fill(ws=None), b"null")
    refused(fill(filled=None), b"null")
    refused(fill(map=big), b"must not be the input")
    refused(fill(ws_bytes=lib.nnd_fill_holes_workspace_bytes(1, 5, 7) - 1), b"workspace")
    refused(fill(ws=C.c_void_p((1 << 20) + 2)), b"aligned")


def test_python_refusals_by_name():
    from nndepth_amd import geometry, scene
    from nndepth_amd._lib import NndError
    x = torch.rand(3, 1, 6, 9)
    disp, depth = scene.Disparity(x), scene.Depth(x)
    fwd = lambda a, b: [{"up_disp": x}]  # noqa: E731
    for call in (lambda: geometry.warp_disparity(x), lambda: geometry.fill_holes(x), lambda: disp.to_other_view(),
                 lambda: disp.warp_occlusion(), lambda: disp.fill_holes(), lambda: depth.fill_holes(),
                 lambda: geometry.occlusion_from_warp(fwd, x, x)):
        with pytest.raises(NndError, match="HIP device"):  # CPU tensors: no fallback
            call()
    with pytest.raises(NndError, match="float64"):
        geometry.warp_disparity(x.double())
    with pytest.raises(NndError, match="float16"):
        scene.Disparity(x.half()).fill_holes()
    with pytest.raises(NndError, match="masks are torch.bool or torch.uint8; got torch.float32"):
        geometry.warp_disparity(x, valid_mask=torch.ones(3, 1, 6, 9))
    with pytest.raises(NndError, match="masks are torch.bool or torch.uint8; got torch.int64"):
        geometry.fill_holes(x, torch.ones(3, 1, 6, 9, dtype=torch.int64))
    with pytest.raises(NndError, match="tensor on the HIP device; got ndarray"):
        geometry.fill_holes(x.numpy())
    with pytest.raises(NndError, match=r"a map is \(B,1,H,W\)"):
        geometry.warp_disparity(torch.rand(3, 2, 6, 9))
    with pytest.raises(NndError, match=r"a map is \(B,1,H,W\)"):
        geometry.fill_holes(torch.rand(6, 9))
    with pytest.raises(NndError, match="disp_sign must be either"):
        geometry.warp_disparity(x, "up")
    for view in ("up", None, 1):
        with pytest.raises(NndError, match="to_view must be 'right' or 'left'"):
            geometry.warp_disparity(x, to_view=view)
        with pytest.raises(NndError, match="to_view must be 'right' or 'left'"):
            disp.to_other_view(view)
    for thr in (-1.0, float("nan")):
        with pytest.raises(NndError, match="threshold must be >= 0"):
            geometry.warp_disparity(x, threshold=thr)
        with pytest.raises(NndError, match="threshold must be >= 0"):
            disp.warp_occlusion(thr)
    for rule in ("background", "mean", None):
        with pytest.raises(NndError, match="rule must be one of"):
            geometry.fill_holes(x, rule=rule)
    for rule in ("min_abs", "linear"):
        with pytest.raises(NndError, match="rule must be one of"):
            disp.fill_holes(rule)
        with pytest.raises(NndError, match="rule must be one of"):
            depth.fill_holes(rule)


def test_new_functions_have_the_signatures_of_the_issue():
    import inspect
    from nndepth_amd import geometry, scene
    p = inspect.signature(geometry.warp_disparity).parameters
    assert list(p) == ["disp", "disp_sign", "to_view", "threshold", "valid_mask", "features", "fill", "return_source"]
    assert [p[k].default for k in list(p)[1:]] == ["negative", "right", 1.0, None, None, 0.0, False]
    p = inspect.signature(geometry.fill_holes).parameters
    assert list(p) == ["map", "mask", "mask_is_valid", "rule", "vertical", "fill", "workspace"]
    assert [p[k].default for k in list(p)[1:]] == [None, True, "min_abs", True, 0.0, None]
    p = inspect.signature(geometry.occlusion_from_warp).parameters
    assert list(p) == ["forward", "left", "right", "threshold"] and p["threshold"].default == 1.0
    p = inspect.signature(scene.Disparity.to_other_view).parameters
    assert list(p) == ["self", "to", "threshold", "features"] and [p[k].default for k in list(p)[1:]] == ["right", 1.0, None]
    p = inspect.signature(scene.Disparity.warp_occlusion).parameters
    assert list(p) == ["self", "threshold"] and p["threshold"].default == 1.0
    for cls in (scene.Disparity, scene.Depth):
        p = inspect.signature(cls.fill_holes).parameters
        assert list(p)[:2] == ["self", "rule"] and p["rule"].default == "background"
    assert inspect.signature(scene.Disparity.fill_holes).parameters["vertical"].default is True


def test_oracle_equals_the_pixel_loops_and_reproduces_the_golden_file(gold):
    G = _loops()
    g = gold("warp_fill.npz")
    cases = G.cases()
    seen = set()
    for name, (kind, kw) in cases.items():
        loops = G.warp_loops(**kw) if kind == "warp" else G.fill_loops(**kw)
        oracle = Wc.warp(**kw) if kind == "warp" else Wc.fill_holes(**kw)
        for key, a, b in zip(G.WARP_KEYS if kind == "warp" else G.FILL_KEYS, loops, oracle):
            assert _same(a, b), (name, key)
            if b is not None:
                assert _same(b, g[f"{kind}_{name}_{key}"]), (name, key)
                seen.add(f"{kind}_{name}_{key}")
    assert seen == set(g) - {"numpy"}


def test_oracle_equals_the_pixel_loops_on_random_small_maps():
    G = _loops()
    for seed in range(12):
        g = Wc.S.rng(100 + seed)
        shape = (2, 1, int(g.integers(1, 6)), int(g.integers(1, 14)))
        d = (g.integers(-3, 13, shape) * 0.5).astype(np.float32)  # many ties, some wrong-sign values
        d[g.random(shape) < 0.05] = np.nan
        mask = g.random(shape) < 0.8
        feats = g.random((2, 2) + shape[2:]).astype(np.float32)
        for sign in ("negative", "positive"):
            for view in ("right", "left"):
                for thr in (0.0, 1.0, float("inf")):
                    kw = dict(d=d, disp_sign=sign, to_view=view, threshold=thr, mask=mask, features=feats, fill=-2.0)
                    assert all(_same(a, b) for a, b in zip(G.warp_loops(**kw), Wc.warp(**kw))), (seed, sign, view, thr)
        for rule in Wc.RULES:
            for vertical in (True, False):
                for pol, m in ((True, mask), (False, ~mask), (True, None)):
                    kw = dict(d=d, mask=m, mask_is_valid=pol, rule=rule, vertical=vertical, fill=-2.0)
                    assert all(_same(a, b) for a, b in zip(G.fill_loops(**kw), Wc.fill_holes(**kw))), (seed, rule, vertical, pol)


def test_oracle_on_the_closed_form_edge_cases():
    # ties to even: x - 0.5 and x + 0.5 round to the even column; columns 1 and 2 at m = 0.5 both land on 2 going left: x = 1 wins
    d = Wc.half_integer((1, 1, 1, 9))
    other, valid, occ, src, _ = Wc.warp(d, "positive", "left")
    assert src[0, 0, 0].tolist() == [0, -1, 1, -1, 3, -1, 5, -1, 7] and not occ.any()  # 8.5 -> 8: in frame
    other, valid, occ, src, _ = Wc.warp(d, "positive", "right")
    assert src[0, 0, 0].tolist() == [0, -1, 2, -1, 4, -1, 6, -1, 8] and not occ.any()  # -0.5 lands on column 0
    assert valid[0, 0, 0].tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1] and (other[0, 0, 0, 1::2] == 0).all()
    # magnitudes larger than W: everything leaves the frame
    other, valid, occ, src, _ = Wc.warp(np.full((2, 1, 3, 7), -9.0, np.float32), fill=5.0)
    assert occ.all() and not valid.any() and (src == -1).all() and (other == 5.0).all()
    # the bar exactly `threshold` nearer hides nothing; one ulp nearer hides the three background pixels whose targets it takes
    thr = Wc.BAR_THRESHOLD
    assert Wc.warp(Wc.bar(), "positive", threshold=thr)[2].sum() == 12
    occ = Wc.warp(Wc.bar(ulp=True), "positive", threshold=thr)[2]
    assert occ.sum() == 12 + 3 * 3 and occ[0, 0, :, 17:20].all()
    assert Wc.warp(Wc.bar(ulp=True), "positive", threshold=float("inf"))[2].sum() == 12  # 4 columns of 3 rows leave the frame
    # -0.0 is +0.0: it lands on its own column and the other view holds +0.0 (negated: -0.0); NaN, inf and wrong signs are occluded
    d = Wc.special()
    other, valid, occ, src, _ = Wc.warp(d, "positive", threshold=float("inf"))
    assert occ[0, 0, 0, [4, 8, 12, 16]].all() and not occ[0, 0, 0, [0, 20]].any() and not occ[0, 0, 1].any()
    assert (Wc.bits(other[0, 0, 1]) == 0).all() and (src[0, 0, 1] == np.arange(24)).all()
    assert (Wc.bits(Wc.warp(-d, "negative")[0][0, 0, 1]) == 0x80000000).all()
    # the sign flips the map and nothing else; an occlusion mask is a valid mask said the other way round
    d, mask = Wc.scene((2, 1, 9, 40), 5, "negative")
    a, b = Wc.warp(d, "negative", mask=mask), Wc.warp(-d, "positive", mask=~mask, mask_is_valid=False)
    assert np.array_equal(a[0], -b[0]) and _same(a[1], 1 - b[1]) and _same(a[2], b[2]) and _same(a[3], b[3])


def test_oracle_properties_of_the_fill():
    for seed, shape in ((1, (2, 1, 9, 40)), (2, (3, 1, 33, 130)), (3, (2, 1, 1, 9)), (4, (2, 1, 9, 1))):
        d, mask = Wc.holes(shape, seed)
        ok = mask & np.isfinite(d)
        for rule in Wc.RULES:
            for vertical in (True, False):
                filled, was, mask_out = Wc.fill_holes(d, mask, True, rule, vertical, fill=-1.0)
                assert np.array_equal(Wc.bits(filled)[ok], Wc.bits(d)[ok]) and not was[ok].any()  # ok pixels untouched
                assert np.array_equal(mask_out != 0, ok | (was != 0))
                again = Wc.fill_holes(filled, mask_out, True, rule, vertical, fill=-1.0)  # idempotent
                assert _same(again[0], filled) and not again[1].any() and _same(again[2], mask_out)
                if vertical and ok.reshape(shape[0], -1).any(axis=1).all():
                    assert mask_out.all()
        # min_abs never exceeds both neighbours; max_abs is never below both (rows with an ok pixel on both sides of the hole)
        lo, hi = Wc.fill_holes(d, mask, True, "min_abs", False)[0], Wc.fill_holes(d, mask, True, "max_abs", False)[0]
        L, R = Wc._nearest_ok(ok, 3)
        both = ~ok & (L >= 0) & (R >= 0)
        vL, vR = np.take_along_axis(d, np.maximum(L, 0), 3), np.take_along_axis(d, np.maximum(R, 0), 3)
        assert (np.abs(lo[both]) == np.minimum(np.abs(vL), np.abs(vR))[both]).all()
        assert (np.abs(hi[both]) == np.maximum(np.abs(vL), np.abs(vR))[both]).all()
    # equal magnitudes of opposite signs: the tie goes left; rows-only leaves the empty rows at `fill`
    d, mask = Wc.fill_pattern(8)
    for rule in ("min_abs", "max_abs"):
        filled, was, mask_out = Wc.fill_holes(d, mask, True, rule, False, fill=-1.0)
        assert (filled[0, 0, 7, 3::8] == 2.5).all() and (filled[0, 0, 7, 4::8] == 2.5).all() and was[0, 0, 7, 3::8].all()
        assert (filled[0, 0, [0, 5, 6, 10, 11]] == -1.0).all() and (filled[1] == -1.0).all() and not mask_out[1].any()
    filled, was, mask_out = Wc.fill_holes(d, mask, True, "nearest", True, fill=-1.0)
    assert (filled[0, 0, 7, 3::8] == 2.5).all() and (filled[0, 0, 7, 4::8] == -2.5).all()
    assert _same(filled[0, 0, 0], filled[0, 0, 1]) and _same(filled[0, 0, 5], filled[0, 0, 4]) and _same(filled[0, 0, 6], filled[0, 0, 7])
    assert _same(filled[0, 0, 11], filled[0, 0, 9]) and mask_out[0].all() and (filled[1] == -1.0).all() and not was[1].any()
    assert (filled[0, 0, 4] == d[0, 0, 4, 9]).all()  # the single ok pixel of its row
