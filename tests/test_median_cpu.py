"""CPU: the masked median and the guided weighted median (csrc/median.hip, nndepth_amd/geometry.py, the scene methods) without a
GPU: the header, the exports, the ctypes table and the Makefile rule agree; the entry point validates its arguments before any HIP
call; Python refuses by name what the kernel does not compute; the vectorised numpy oracle of tests/median_cases.py equals the
pixel loops of scripts/make_golden_median.py on every input builder and reproduces tests/golden/median.npz, which those loops
wrote."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import median_cases as Mc
from cabi_checks import header_exports_ctypes_table_and_makefile_rule_agree, refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nnd_median_filter_limit", "nnd_median_filter")


def _loops():
    spec = importlib.util.spec_from_file_location("make_golden_median", os.path.join(ROOT, "scripts", "make_golden_median.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and (np.array_equal(Mc.bits(a), Mc.bits(b)) if a.dtype == np.float32 else np.array_equal(a, b))


def test_header_exports_ctypes_table_and_makefile_rule_agree():
    from nndepth_amd._lib import lib
    header_exports_ctypes_table_and_makefile_rule_agree(NAMES, "median")
    assert lib.nnd_version() == 105


def test_limits_and_their_python_mirrors():
    from nndepth_amd import geometry
    from nndepth_amd._lib import lib
    rmax, th, tw = (lib.nnd_median_filter_limit(i) for i in range(3))
    assert rmax >= 7 and th > 0 and tw > 0
    for which in (3, -1, 99):
        assert lib.nnd_median_filter_limit(which) < 0
    assert geometry.median_max_radius() == rmax and geometry.median_tile() == (th, tw)


def test_entry_point_validates_before_any_device_call():
    from nndepth_amd._lib import lib
    one, two = C.c_void_p(16), C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first
    table = np.full(256, 7, np.uint16)  # host memory: weights[0] is read by the validation
    zero0 = table.copy()
    zero0[0] = 0
    inf, nan = float("inf"), float("nan")
    rmax = lib.nnd_median_filter_limit(0)

    def med(map=one, bstride=35, mask=None, pol=1, radius=1, min_count=1, fill_invalid=0, fill=0.0, guide=None, Cg=0, inv_step=1.0,
            weights=None, filtered=two, mask_out=None, changed=None, B=1, H=5, W=7):
        w = None if weights is None else weights.ctypes.data
        return lib.nnd_median_filter(map, bstride, mask, pol, radius, min_count, fill_invalid, fill, guide, Cg, inv_step, w, filtered,
                                     mask_out, changed, B, H, W, None)

    refused(med(map=None), b"null")
    refused(med(filtered=None), b"null")
    refused(med(filtered=one), b"must not be the input")
    for kw in (dict(B=0), dict(B=70000), dict(H=0), dict(H=-1), dict(W=0), dict(W=-3), dict(H=1 << 16, W=1 << 16, bstride=1 << 32)):
        refused(med(**kw), b"shape")
    refused(med(B=2, bstride=34), b"stride")
    for r in (0, -1, rmax + 1, 1000):
        refused(med(radius=r), b"radius")
    for r, mc in ((1, 0), (1, 10), (1, -1), (2, 26), (rmax, (2 * rmax + 1) ** 2 + 1)):
        refused(med(radius=r, min_count=mc), b"min_count")
    refused(med(guide=one), b"do not go together")
    refused(med(guide=one, Cg=3), b"do not go together")
    refused(med(guide=one, weights=table), b"do not go together")
    refused(med(Cg=3, weights=table), b"do not go together")
    refused(med(Cg=1), b"do not go together")
    refused(med(weights=table), b"do not go together")
    for Cg in (5, -1, 100):
        refused(med(guide=one, Cg=Cg, weights=table), b"channels")
    for step in (0.0, -1.0, inf, -inf, nan):
        refused(med(guide=one, Cg=3, weights=table, inv_step=step), b"inv_step")
    refused(med(guide=one, Cg=3, weights=zero0), b"weights[0]")


def test_python_refusals_by_name():
    from nndepth_amd import geometry, scene
    from nndepth_amd._lib import NndError
    x = torch.rand(3, 1, 6, 9)
    for call in (lambda: geometry.median_filter(x), lambda: scene.Disparity(x).median_filter(), lambda: scene.Depth(x).median_filter(2),
                 lambda: geometry.median_filter(x, guide=torch.rand(3, 3, 6, 9))):
        with pytest.raises(NndError, match="HIP device"):  # CPU tensors: no fallback
            call()
    with pytest.raises(NndError, match="float64"):
        geometry.median_filter(x.double())
    with pytest.raises(NndError, match="float16"):
        scene.Depth(x.half()).median_filter()
    with pytest.raises(NndError, match="masks are torch.bool or torch.uint8; got torch.float32"):
        geometry.median_filter(x, valid_mask=torch.ones(3, 1, 6, 9))
    with pytest.raises(NndError, match="tensor on the HIP device; got ndarray"):
        geometry.median_filter(x.numpy())
    for bad in (torch.rand(3, 2, 6, 9), torch.rand(6, 9)):
        with pytest.raises(NndError, match=r"a map is \(B,1,H,W\)"):
            geometry.median_filter(bad)
    for g in (torch.rand(3, 3, 6, 8), torch.rand(2, 3, 6, 9), torch.rand(3, 5, 6, 9), torch.rand(3, 6, 9), torch.rand(3, 0, 6, 9)):
        with pytest.raises(NndError, match=r"the guide is \(B,C,H,W\) = \(3,1..4,6,9\)"):  # a guide of the wrong size
            geometry.median_filter(x, guide=g)
        with pytest.raises(NndError, match=r"the guide is \(B,C,H,W\)"):
            scene.Disparity(x).median_filter(2, guide=scene.Frame(g))
    with pytest.raises(NndError, match="the guide is torch.float32; got torch.float16"):
        geometry.median_filter(x, guide=torch.rand(3, 3, 6, 9).half())
    with pytest.raises(NndError, match="the guide is torch.float32; got ndarray"):
        geometry.median_filter(x, guide=np.zeros((3, 3, 6, 9), np.float32))
    for kind in ("linear", None):
        with pytest.raises(NndError, match="kind must be one of"):
            geometry.range_weights(0.2, kind=kind)
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(NndError, match="sigma must be finite and > 0"):
            geometry.range_weights(sigma)
    for step in (0.0, -0.1, float("inf")):
        with pytest.raises(NndError, match="step must be finite and > 0"):
            geometry.range_weights(0.2, step)


def test_signatures_of_the_issue():
    import inspect
    from nndepth_amd import geometry, scene
    p = inspect.signature(geometry.median_filter).parameters
    assert list(p) == ["map", "radius", "valid_mask", "mask_is_valid", "guide", "sigma", "step", "kind", "weights", "min_count", "fill_invalid",
                       "fill", "return_changed"]
    assert [p[k].default for k in list(p)[1:]] == [1, None, True, None, 0.2, None, "exp", None, 1, False, 0.0, False]
    p = inspect.signature(geometry.range_weights).parameters
    assert list(p) == ["sigma", "step", "kind"] and [p[k].default for k in ("step", "kind")] == [None, "exp"]
    for cls in (scene.Disparity, scene.Depth):
        p = inspect.signature(cls.median_filter).parameters
        assert list(p) == ["self", "radius", "guide", "sigma", "fill_invalid", "min_count", "weights_kw"]
        assert [p[k].default for k in list(p)[1:6]] == [1, None, 0.2, False, 1]
    assert "median_filter" in geometry.__doc__


def test_range_weights_values():
    from nndepth_amd import geometry
    for kind in ("exp", "gauss", "box"):
        for sigma, step in ((0.2, None), (0.05, 0.01), (3.0, 0.5)):
            w, inv = geometry.range_weights(sigma, step, kind)
            ww, winv = Mc.range_weights(sigma, step, kind)
            assert w.dtype == np.uint16 and w.shape == (256,) and np.array_equal(w, ww) and isinstance(inv, float) and inv == float(winv)
            assert w[0] == 65535 and (np.diff(w.astype(np.int64)) <= 0).all()
    w, inv = geometry.range_weights(0.2)
    assert inv == float(np.float32(160.0)) and w[32] == int(np.floor(65535 * np.exp(-1.0) + 0.5)) == 24109 and w[255] == 23
    w, _ = geometry.range_weights(0.2, kind="gauss")
    assert w[32] == int(np.floor(65535 * np.exp(-0.5) + 0.5)) and w[255] == 0
    w, _ = geometry.range_weights(0.2, kind="box")
    assert (w[:33] == 65535).all() and (w[33:] == 0).all()  # 32 * (0.2 / 32) <= 0.2 in float64
    w, inv = geometry.range_weights(1.0, 0.25, "box")
    assert inv == 4.0 and (w[:5] == 65535).all() and (w[5:] == 0).all()


def test_oracle_equals_the_pixel_loops_and_reproduces_the_golden_file(gold):
    G = _loops()
    g = gold("median.npz")
    seen = set()
    for name, kw in G.cases().items():
        for key, a, b in zip(G.KEYS, G.median_loops(**kw), Mc.median_filter(**kw)):
            assert _same(a, b), (name, key)
            assert _same(b, g[f"{name}_{key}"]), (name, key)
            seen.add(f"{name}_{key}")
    assert seen == set(g) - {"numpy"}
    kw = G.cases()["r1"]
    assert kw["d"].shape == Mc.GOLDEN_SHAPE and G.cases()["r3_guided_edge_nan"]["guide"].shape[1] == 3


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 1, 1, 2), (2, 1, 3, 5), Mc.SMALL], ids=str)
def test_oracle_equals_the_pixel_loops_on_every_builder(shape):
    G = _loops()
    for name, kw in Mc.builders(shape).items():
        for radius, min_count in ((1, 1), (2, 7), (7, 1)):
            for a, b in zip(G.median_loops(radius=radius, min_count=min_count, **kw), Mc.median_filter(radius=radius, min_count=min_count, **kw)):
                assert _same(a, b), (name, radius, min_count)


def test_oracle_properties():
    shape = (2, 1, 9, 40)
    B = Mc.builders(shape)
    # a constant table gives the unweighted result
    kw = B["constant_table"]
    plain = {k: v for k, v in kw.items() if k not in ("guide", "weights", "inv_step")}
    for r in (1, 2, 5):
        assert all(_same(a, b) for a, b in zip(Mc.median_filter(radius=r, **kw), Mc.median_filter(radius=r, **plain)))
    # unit weights: the element of rank (n - 1) / 2 of the sorted ok taps; every output is one of the window's ok values or the centre
    for name in ("scene", "few_values", "special", "checkerboard"):
        kw = B[name]
        d = kw["d"]
        ok = Mc.valid_of(d.shape, kw.get("mask"), kw.get("mask_is_valid", True)) & np.isfinite(d)
        for r in (1, 3):
            out, mask_out, changed = Mc.median_filter(radius=r, **kw)
            key = np.where(ok, Mc.keys_of(d), Mc.BAD)[:, 0]
            taps = np.sort(Mc._taps(key, r, Mc.BAD), axis=-1)
            n = (taps != Mc.BAD).sum(-1)
            want = np.take_along_axis(taps, np.maximum((n - 1) // 2, 0)[..., None], -1)[..., 0]
            produced = ((ok[:, 0] | bool(kw.get("fill_invalid", False))) & (n >= 1))
            assert np.array_equal(Mc.keys_of(out)[:, 0][produced], want[produced]), (name, r)
            assert np.array_equal(mask_out[:, 0] != 0, ok[:, 0] | produced)
            assert not changed[ok & (Mc.bits(out) == Mc.bits(d))].any()
    # -0.0 sorts below +0.0: of {-0.0, +0.0, +0.0} the median is +0.0, of {-0.0, -0.0, +0.0} it is -0.0
    for vals, want in (([-0.0, 0.0, 0.0], 0x00000000), ([-0.0, -0.0, 0.0], 0x80000000), ([0.0, -0.0], 0x80000000)):
        d = np.array(vals, np.float32).reshape(1, 1, 1, -1)
        assert Mc.bits(Mc.median_filter(d, radius=2)[0])[0, 0, 0, 0] == want
    # all invalid: nothing is produced, everything is `fill`; a single ok pixel spreads to its window under fill_invalid
    out, mask_out, changed = Mc.median_filter(radius=2, **B["all_invalid"])
    assert (out == 5.0).all() and not mask_out.any()
    kw = B["single"]
    out, mask_out, _ = Mc.median_filter(radius=2, **kw)
    assert mask_out.sum() == 25 and (out[mask_out != 0] == kw["d"][kw["mask"]]).all()
    # the guided median puts the disparity edge on the guide's edge, one column to the right of the map's
    d, m, g = Mc.edge_guide((1, 1, 9, 40), 3, 0)
    w, inv = Mc.range_weights(0.05)
    out = Mc.median_filter(d, 3, None, True, g, inv, w)[0]
    assert (d[0, 0, :, 20] > 20).all() and (out[0, 0, 3:6, 20] < 20).all() and (out[0, 0, 3:6, 21] > 20).all()
    assert (Mc.median_filter(d, 3)[0][0, 0, 3:6, 20] > 20).all()  # the plain median leaves it where it was
