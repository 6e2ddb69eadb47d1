"""CPU: connected regions and the speckle filter (csrc/speckle.hip, nndepth_amd/geometry.py, the scene methods) without a GPU:
the header, the exports, the ctypes table and the Makefile rule agree; every entry point validates its arguments before any HIP
call; Python refuses by name what the kernels do not compute; the numpy oracle of tests/speckle_cases.py equals scipy's
connected_components and reproduces tests/golden/speckle.npz (scripts/make_golden_speckle.py, built from scipy)."""
import ctypes as C

import numpy as np
import pytest
import torch

import speckle_cases as S
from cabi_checks import header_exports_ctypes_table_and_makefile_rule_agree, refused

NAMES = ("nnd_connected_regions_workspace_bytes", "nnd_connected_regions_tile", "nnd_connected_regions", "nnd_speckle_filter")


def test_header_exports_ctypes_table_and_makefile_rule_agree():
    header_exports_ctypes_table_and_makefile_rule_agree(NAMES, "speckle")


def test_tile_and_workspace_size():
    from nndepth_amd import geometry
    from nndepth_amd._lib import lib
    th, tw = lib.nnd_connected_regions_tile(0), lib.nnd_connected_regions_tile(1)
    assert th > 0 and tw > 0 and lib.nnd_connected_regions_tile(2) < 0
    assert geometry.regions_tile() == (th, tw)
    assert lib.nnd_connected_regions_workspace_bytes(2, 5, 7) == 8 * 70 + 80  # two int32 planes and the edge bytes, rounded to 16
    assert geometry.regions_workspace_bytes(1, 4, 4) == 8 * 16 + 16
    for bad in ((0, 5, 7), (2, 0, 7), (2, 5, -1), (70000, 5, 7), (1, 1 << 16, 1 << 16)):
        assert lib.nnd_connected_regions_workspace_bytes(*bad) < 0, bad


def test_entry_points_validate_before_any_device_call():
    from nndepth_amd._lib import lib
    one, big = C.c_void_p(16), C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first
    inf, nan = float("inf"), float("nan")

    def regions(map=one, bstride=35, mask=None, pol=1, max_diff=0.5, conn=4, labels=one, sizes=one, ws=big, ws_bytes=1 << 20, B=1,
                H=5, W=7):
        return lib.nnd_connected_regions(map, bstride, mask, pol, max_diff, conn, labels, sizes, ws, ws_bytes, B, H, W, None)

    def speckle(map=one, bstride=35, mask=None, pol=0, max_diff=0.5, conn=4, max_size=4, fill=0.0, filtered=one, mask_out=one,
                speckle_out=None, sizes=None, ws=big, ws_bytes=1 << 20, B=1, H=5, W=7):
        return lib.nnd_speckle_filter(map, bstride, mask, pol, max_diff, conn, max_size, fill, filtered, mask_out, speckle_out, sizes,
                                      ws, ws_bytes, B, H, W, None)

    for f in (regions, speckle):
        refused(f(map=None), b"null")
        refused(f(ws=None), b"null")
        refused(f(B=0), b"shape")
        refused(f(B=70000), b"shape")
        refused(f(H=0), b"shape")
        refused(f(W=-3), b"shape")
        refused(f(H=1 << 16, W=1 << 16, bstride=1 << 32, ws_bytes=1 << 40), b"shape")
        refused(f(B=2, bstride=34), b"stride")
        refused(f(max_diff=nan), b"max_diff")
        refused(f(max_diff=-0.5), b"max_diff")
        refused(f(max_diff=-inf), b"max_diff")
        refused(f(conn=6), b"connectivity")
        refused(f(conn=0), b"connectivity")
        refused(f(ws_bytes=lib.nnd_connected_regions_workspace_bytes(1, 5, 7) - 1), b"workspace")
        refused(f(ws=C.c_void_p((1 << 20) + 4)), b"aligned")
    refused(regions(labels=None, sizes=None), b"null")
    refused(speckle(filtered=None, mask_out=None, speckle_out=None), b"null")
    refused(speckle(max_size=-1), b"max_size")


def test_python_refusals_by_name():
    from nndepth_amd import geometry, scene
    from nndepth_amd._lib import NndError
    x = torch.rand(3, 1, 6, 9)
    disp, depth = scene.Disparity(x), scene.Depth(x)
    for call in (lambda: geometry.connected_regions(x, 0.5), lambda: geometry.speckle_mask(x, 4), lambda: geometry.speckle_filter(x, 4),
                 lambda: disp.remove_speckles(4), lambda: depth.remove_speckles(4)):
        with pytest.raises(NndError, match="HIP device"):  # CPU tensors: no fallback
            call()
    with pytest.raises(NndError, match="float64"):
        geometry.connected_regions(x.double(), 0.5)
    with pytest.raises(NndError, match="float16"):
        scene.Disparity(x.half()).remove_speckles(4)
    with pytest.raises(NndError, match="masks are torch.bool or torch.uint8; got torch.float32"):
        geometry.connected_regions(x, 0.5, valid_mask=torch.ones(3, 1, 6, 9))
    with pytest.raises(NndError, match="masks are torch.bool or torch.uint8; got torch.int64"):
        scene.Depth(x, valid_mask=torch.ones(3, 1, 6, 9, dtype=torch.int64)).remove_speckles(4)
    with pytest.raises(NndError, match="tensor on the HIP device; got ndarray"):
        geometry.speckle_mask(x.numpy(), 4)
    for conn in (6, 0, "4", None):
        with pytest.raises(NndError, match="connectivity must be 4 or 8"):
            geometry.connected_regions(x, 0.5, connectivity=conn)
    with pytest.raises(NndError, match="connectivity must be 4 or 8"):
        disp.remove_speckles(4, connectivity=5)
    for md in (-1.0, float("nan")):
        with pytest.raises(NndError, match="max_diff must be >= 0"):
            geometry.connected_regions(x, md)
        with pytest.raises(NndError, match="max_diff must be >= 0"):
            depth.remove_speckles(4, max_diff=md)
    for size in (-1, 2.5, True, None):
        with pytest.raises(NndError, match="max_size must be an integer >= 0"):
            geometry.speckle_mask(x, size)


def test_new_methods_have_the_signatures_of_the_issue():
    import inspect
    from nndepth_amd import geometry, scene
    for cls in (scene.Disparity, scene.Depth):
        p = inspect.signature(cls.remove_speckles).parameters
        assert list(p) == ["self", "max_size", "max_diff", "connectivity", "fill"]
        assert (p["max_diff"].default, p["connectivity"].default, p["fill"].default) == (1.0, 4, 0.0)
    p = inspect.signature(geometry.connected_regions).parameters
    assert list(p) == ["map", "max_diff", "valid_mask", "connectivity", "workspace"]
    assert (p["valid_mask"].default, p["connectivity"].default, p["workspace"].default) == (None, 4, None)
    p = inspect.signature(geometry.speckle_mask).parameters
    assert list(p) == ["map", "max_size", "max_diff", "valid_mask", "connectivity", "return_sizes"]
    assert (p["max_diff"].default, p["valid_mask"].default, p["connectivity"].default, p["return_sizes"].default) == (1.0, None, 4, False)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_oracle_equals_scipy_on_random_maps(connectivity):
    pytest.importorskip("scipy")
    for shape, seeds in (((2, 1, 6, 9), range(40)), ((1, 1, 33, 130), range(4))):
        for seed in seeds:
            d, mask, md = S.quantised(shape, seed)
            for m, pol in ((mask, True), (mask, False), (None, True)):
                got, want = S.regions(d, md, m, pol, connectivity), S.regions_scipy(d, md, m, pol, connectivity)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (shape, seed, pol)
    d, mask, md = S.scene((2, 1, 33, 130), 3)
    got, want = S.regions(d, md, mask, True, connectivity), S.regions_scipy(d, md, mask, True, connectivity)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("connectivity", [4, 8])
def test_oracle_reproduces_the_golden_file(gold, connectivity):
    g = gold("speckle.npz")
    assert tuple(g["tile"]) == S.GOLDEN_TILE and tuple(g["shape"]) == S.GOLDEN_SHAPE
    patterns = S.slow_patterns(*S.GOLDEN_TILE)
    assert {k.split("_c")[0] for k in g if k.endswith("_labels")} == set(patterns)
    for name, (d, mask, md) in patterns.items():
        labels, sizes = S.oracle_regions((name, *S.GOLDEN_TILE), connectivity)
        assert np.array_equal(labels[0, 0], g[f"{name}_c{connectivity}_labels"]), name
        assert np.array_equal(sizes[0, 0], g[f"{name}_c{connectivity}_sizes"]), name
    d, mask, md = patterns["scene"]
    for k in (1, 8, 64):
        assert np.array_equal(S.speckle_filter(d, k, md, mask, True, connectivity)[2][0, 0], g[f"scene_c{connectivity}_s{k}_speckle"])
    # the long paths are long: one region holds the whole serpentine / spiral
    assert g["serp_h_full_c4_sizes"].max() == 35 * 200 + 34 and g["spiral_c4_sizes"].max() >= 7000


def test_oracle_on_the_closed_form_edge_cases():
    # a difference equal to max_diff joins; with max_diff one ulp below the step nothing does
    d, _, md = S.ramp((1, 1, 3, 9))
    labels, sizes = S.regions(d, md)
    assert (sizes == 9).all() and np.array_equal(labels[0, 0], np.repeat(np.arange(3) * 9, 9).reshape(3, 9))
    d, _, md = S.ramp((1, 1, 3, 9), exact=False)
    assert md < 0.5 and (S.regions(d, md)[1] == 1).all()
    # the special values: row 0 NaN / inf split the 1.0s; row 1 +-3e38; row 2 exactly 0.5 apart and one ulp more; -0.0 joins 0.0
    d, _, _ = S.special(0.5)
    labels, sizes = S.regions(d, 0.5)
    assert labels[0, 0, 0].tolist() == [0, -1, 2, -1, 4, -1, 6, 6, 8, 9, 9, 11]
    assert labels[0, 0, 1, :2].tolist() == [12, 13] and labels[0, 0, 1, 3:5].tolist() == [15, 15] and labels[0, 0, 1, 9:11].tolist() == [-1, -1]
    assert labels[0, 0, 2, :2].tolist() == [24, 24] and labels[0, 0, 2, 3:5].tolist() == [27, 28]
    assert labels[0, 0, 2, 6:8].tolist() == [30, 30] and labels[0, 0, 2, 9:11].tolist() == [33, 34]
    assert labels[0, 0, 3, 2:6].tolist() == [38] * 4 and labels[0, 0, 3, :2].tolist() == [-1, -1]
    inf_labels, inf_sizes = S.regions(d, float("inf"))  # every valid pixel joins its valid neighbours, 3e38 - -3e38 = inf included
    assert inf_labels[0, 0, 1, :2].tolist() == [0, 0] and inf_labels[0, 0, 0, 1] == -1 and inf_labels[0, 0, 3, 6:10].tolist() == [0] * 4
    # a checkerboard: alone with 4 neighbours, one region with 8; sizes of exactly n and n + 1
    d, mask, md = S.checkerboard((1, 1, 5, 7))
    assert S.regions(d, md, mask)[1].max() == 1 and S.regions(d, md, mask, connectivity=8)[1].max() == 18
    d, _, md = S.sized_bars(16, 20, 8, 6)
    sp = S.speckle_filter(d, 6, md)[2][0, 0]
    assert sp[1].sum() == 6 and sp[3].sum() == 0 and sp[:, 2].sum() == 6 and sp[:, 4].sum() == 0
    d, mask, md = S.all_invalid((2, 1, 5, 7))
    labels, sizes = S.regions(d, md, mask)
    assert (labels == -1).all() and (sizes == 0).all()
