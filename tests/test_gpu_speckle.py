"""GPU: connected regions and the speckle filter through the HIP path (csrc/speckle.hip) against the numpy oracle of
tests/speckle_cases.py and the scipy-built fixture tests/golden/speckle.npz (scripts/make_golden_speckle.py).  Every comparison
is an equality: labels, sizes, masks, and the bits of the filtered map.  The patterns are laid out for the tile the library
reports (nnd_connected_regions_tile): turns, rings and lines sit on its borders and corners."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import speckle_cases as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(x):
    return x.cpu().numpy()


def _bits(x) -> np.ndarray:
    x = _np(x) if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _tile():
    from nndepth_amd import geometry
    return geometry.regions_tile()


def _tile_shape():
    th, tw = _tile()
    return (2, 1, 2 * th + 3, 2 * tw + 3)


def _shapes():
    return S.SHAPES + ["tile"]


def _shape(s):
    return _tile_shape() if s == "tile" else s


def _check_regions(d, mask, md, conn, what, want=None):
    """labels and sizes of the device against the oracle (or `want`); returns the oracle's pair"""
    from nndepth_amd import geometry
    want = want or S.regions(d, md, mask, True, conn)
    labels, sizes = geometry.connected_regions(_t(d), md, None if mask is None else _t(mask), conn)
    assert labels.dtype == torch.int32 and sizes.dtype == torch.int32 and labels.shape == d.shape and sizes.shape == d.shape
    nl, ns = int((_np(labels) != want[0]).sum()), int((_np(sizes) != want[1]).sum())
    print(f"[speckle] {what} c{conn}: {nl} labels and {ns} sizes of {d.size} differ; largest region {int(want[1].max())}")
    assert nl == 0 and ns == 0, what
    return want


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", _shapes(), ids=str)
def test_quantised_random(shape, conn):
    from nndepth_amd import geometry
    shape = _shape(shape)
    d, mask, md = S.quantised(shape, 1000 + shape[2] * shape[3])
    _, sizes = _check_regions(d, mask, md, conn, f"quantised {shape}")
    if shape == (3, 1, 70, 200) and conn == 4:  # a condition on the input: mostly small regions
        valid = S.valid_of(d, mask)
        assert (sizes[valid] <= 8).mean() > 0.3 and sizes.max() < 2000
    # the mask as uint8 (B,H,W); no mask at all
    labels, _ = geometry.connected_regions(_t(d), md, _t(mask[:, 0].astype(np.uint8)), conn)
    assert np.array_equal(_np(labels), S.regions(d, md, mask, True, conn)[0])
    _check_regions(d, None, md, conn, f"quantised {shape} without a mask")
    want = S.speckle_filter(d, 8, md, mask, True, conn)
    sp, sz = geometry.speckle_mask(_t(d), 8, md, _t(mask), conn, return_sizes=True)
    assert sp.dtype == torch.uint8 and np.array_equal(_np(sp), want[2]) and np.array_equal(_np(sz), want[3])
    assert torch.equal(geometry.speckle_mask(_t(d), 8, md, _t(mask), conn), sp)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("md", [0.5, 1.0])
def test_scene_remove_speckles(conn, md):
    from nndepth_amd.scene import Depth, Disparity
    shape = (3, 1, 70, 200)
    d, mask, _ = S.scene(shape, 77, md)
    dd, occ_bool, valid_u8 = _t(d), _t(~mask), _t(mask[:, 0].astype(np.uint8))
    _check_regions(d, mask, md, conn, f"scene max_diff {md}")
    for max_size in (1, 8, 64):
        filt, mask_valid, speckle, sizes = S.speckle_filter(d, max_size, md, mask, True, conn, fill=-1.0)
        share = float(speckle.mean())
        print(f"[speckle] scene c{conn} max_diff {md} max_size {max_size}: {100 * share:.2f} % removed, largest region {int(sizes.max())}")
        assert 0.02 < share < 0.2 and sizes.max() > max_size  # conditions on the oracle alone
        # Disparity: occlusion as bool (B,1,H,W), 1 = invalid
        got = Disparity(dd, "positive", occlusion=occ_bool, baseline=0.3).remove_speckles(max_size, md, conn, fill=-1.0)
        assert isinstance(got, Disparity) and got.disp_sign == "positive" and got.baseline == 0.3 and got.occlusion.dtype == torch.bool
        assert np.array_equal(_bits(got.data), _bits(filt))
        assert np.array_equal(_np(got.occlusion), mask_valid == 0)
        assert np.array_equal(_bits(got.data)[speckle == 0], _bits(d)[speckle == 0])  # untouched pixels: the input's bits
        # Depth: valid_mask as uint8 (B,H,W), 1 = valid
        got = Depth(dd, valid_mask=valid_u8).remove_speckles(max_size, md, conn, fill=-1.0)
        assert isinstance(got, Depth) and got.valid_mask.dtype == torch.uint8 and got.valid_mask.shape == shape
        assert np.array_equal(_bits(got.data), _bits(filt)) and np.array_equal(_np(got.valid_mask), mask_valid)


@pytest.mark.parametrize("name", ["serp_h_full", "serp_h_border", "serp_h_inner", "serp_v_full", "serp_v_border", "spiral", "scene"])
def test_long_paths(name, gold):
    """One region winds through every tile: the serpentines turn on tile borders and corners, the spiral's background is a second
    spiral.  Against the oracle for the library's tile, and against the scipy-built fixture when that tile is the fixture's."""
    th, tw = _tile()
    d, mask, md = S.slow_patterns(th, tw)[name]
    g = gold("speckle.npz")
    for conn in (4, 8):
        want = S.oracle_regions((name, th, tw), conn)
        if (th, tw) == tuple(g["tile"]):
            assert np.array_equal(want[0][0, 0], g[f"{name}_c{conn}_labels"]) and np.array_equal(want[1][0, 0], g[f"{name}_c{conn}_sizes"])
        _check_regions(d, mask, md, conn, name, want)
        if name != "scene":
            assert want[1].max() >= 7000  # the path is one region


def _small_patterns():
    th, tw = _tile()
    B, _, H, W = _tile_shape()
    return {
        "checkerboard": S.checkerboard((2, 1, H, W)),
        "corner_rings": S.corner_rings(H, W, th, tw),
        "lines": S.lines(H, W, th, tw),
        "lines_wide": S.lines(2 * th + 3, 3 * tw + 5, th, tw),  # the row crosses four tiles
        "constant": S.constant((2, 1, H, W)),
        "constant_70x200": S.constant((3, 1, 70, 200)),
        "ramp": S.ramp((1, 1, H, W)),
        "ramp_ulp": S.ramp((1, 1, H, W), exact=False),
        "bars": S.sized_bars(H, W, tw, 8),
        "special": S.special(0.5),
        "special_inf": S.special(float("inf")),
        "special_zero": S.special(0.0),
        "all_invalid": S.all_invalid((2, 1, H, W)),
        "all_invalid_1x1": (np.full((1, 1, 1, 1), np.inf, np.float32), None, 0.5),
    }


@pytest.mark.parametrize("name", ["checkerboard", "corner_rings", "lines", "lines_wide", "constant", "constant_70x200", "ramp", "ramp_ulp",
                                  "bars", "special", "special_inf", "special_zero", "all_invalid", "all_invalid_1x1"])
def test_patterns(name):
    from nndepth_amd import geometry
    d, mask, md = _small_patterns()[name]
    H, W = d.shape[2:]
    for conn in (4, 8):
        labels, sizes = _check_regions(d, mask, md, conn, name)
        valid = S.valid_of(d, mask)
        if name == "checkerboard":  # alone with 4 neighbours, one region with 8
            assert (sizes[valid] == (1 if conn == 4 else (H * W + 1) // 2)).all()
        elif name.startswith("constant"):
            assert (sizes == H * W).all() and (labels == 0).all()
        elif name == "ramp":
            assert (sizes == W).all()
        elif name == "ramp_ulp":
            assert (sizes == 1).all()
        elif name == "corner_rings":
            assert sizes[0, 0, d[0, 0] == 1.0].tolist() == [12] * 12 and (sizes[1][valid[1]] == (1 if conn == 4 else 12)).all()
        elif name.startswith("all_invalid"):
            assert (labels == -1).all() and (sizes == 0).all()
        elif name == "bars":  # regions of exactly max_size pixels go, of max_size + 1 stay
            sp = _np(geometry.speckle_mask(_t(d), 8, md, None, conn))
            assert np.array_equal(sp, S.speckle_filter(d, 8, md, None, True, conn)[2])
            assert sp[0, 0, 1].sum() == 8 and sp[0, 0, 3].sum() == 0 and sp[0, 0, :, 2].sum() == 8 and sp[0, 0, :, 4].sum() == 0
        if name.startswith("special"):  # NaN / inf stay as they are in the filtered map; the masks flag them
            for pol in (True, False):
                want = S.speckle_filter(d, 1, md, None, pol, conn, fill=-5.0)
                got = geometry.speckle_filter(_t(d), 1, md, None, pol, conn, fill=-5.0, return_sizes=True)
                assert np.array_equal(_bits(got[0]), _bits(want[0])) and all(np.array_equal(_np(a), b) for a, b in zip(got[1:], want[1:]))


def test_mask_polarities_shapes_and_a_channel_slice_read_in_place():
    from nndepth_amd import geometry
    g = S.rng(9)
    two = (g.integers(0, 4, (2, 2, 37, 70)) * 0.5).astype(np.float32)
    mask = g.random((2, 1, 37, 70)) < 0.85
    dev = _t(two)
    for c in (0, 1):
        view, d = dev[:, c:c + 1], np.ascontiguousarray(two[:, c:c + 1])
        assert not view.is_contiguous() and view.stride(0) == 2 * 37 * 70
        for conn in (4, 8):
            want = S.regions(d, 0.5, mask, True, conn)
            for m in (_t(mask), _t(mask[:, 0]), _t(mask.astype(np.uint8)), _t(mask[:, 0].astype(np.uint8) * 7)):  # non-zero = set
                labels, sizes = geometry.connected_regions(view, 0.5, m, conn)
                assert np.array_equal(_np(labels), want[0]) and np.array_equal(_np(sizes), want[1])
            for pol, m in ((True, mask), (False, ~mask)):  # the same pixels valid, said both ways
                want_f = S.speckle_filter(d, 3, 0.5, m, pol, conn, fill=9.0)
                got = geometry.speckle_filter(view, 3, 0.5, _t(m[:, 0]), pol, conn, fill=9.0, return_sizes=True)
                assert np.array_equal(_bits(got[0]), _bits(want_f[0]))
                assert all(np.array_equal(_np(a), b) for a, b in zip(got[1:], want_f[1:]))
                assert np.array_equal(want_f[1] != 0, (S.speckle_filter(d, 3, 0.5, mask, True, conn)[1] != 0) == pol)
    assert torch.equal(dev, _t(two))  # the input is not written


def _raw(d_dev, mask_dev, pol, md, conn, max_size, fill, fillers):
    """Both entry points through ctypes on buffers of our own, every output and the workspace pre-filled by `fillers`."""
    from nndepth_amd._lib import check, lib
    from nndepth_amd.ops import _p, _stream
    B, _, H, W = d_dev.shape
    n = lib.nnd_connected_regions_workspace_bytes(B, H, W)
    mk = lambda dtype, fill_: fill_(torch.empty((B, 1, H, W), dtype=dtype, device=DEV))  # noqa: E731
    f_i32, f_u8, f_f32, f_ws = fillers
    ws = f_ws(torch.empty(n // 8 + 1, dtype=torch.int64, device=DEV))
    labels, sizes, sizes2 = mk(torch.int32, f_i32), mk(torch.int32, f_i32), mk(torch.int32, f_i32)
    filt, mask_out, speckle = mk(torch.float32, f_f32), mk(torch.uint8, f_u8), mk(torch.uint8, f_u8)
    check(lib.nnd_connected_regions(_p(d_dev), H * W, _p(mask_dev), pol, md, conn, _p(labels), _p(sizes), _p(ws), ws.numel() * 8, B, H, W,
                                    _stream(d_dev.device)), "connected_regions")
    ws = f_ws(ws)
    check(lib.nnd_speckle_filter(_p(d_dev), H * W, _p(mask_dev), pol, md, conn, max_size, fill, _p(filt), _p(mask_out), _p(speckle),
                                 _p(sizes2), _p(ws), ws.numel() * 8, B, H, W, _stream(d_dev.device)), "speckle_filter")
    return labels, sizes, sizes2, filt, mask_out, speckle


def test_same_bytes_on_every_run_and_whatever_the_buffers_held():
    shape = _tile_shape()
    d, mask, md = S.scene(shape, 5)
    dd, mm = _t(d), _t(mask.view(np.uint8))
    zero = lambda t: t.zero_()  # noqa: E731
    ones = lambda t: t.view(torch.uint8).fill_(0xFF).view(t.dtype).view(t.shape) if t.dtype != torch.uint8 else t.fill_(0xFF)  # noqa: E731
    small = lambda t: t.fill_(3)  # noqa: E731  small positive labels / counts: what a stale workspace looks like

    for conn in (4, 8):
        want_l, want_s = S.regions(d, md, mask, True, conn)
        want_f = S.speckle_filter(d, 8, md, mask, True, conn, fill=-2.0)
        runs = [_raw(dd, mm, 1, md, conn, 8, -2.0, f) for f in ((zero,) * 4, (zero,) * 4, (ones,) * 4, (small, small, small, small))]
        torch.cuda.synchronize()
        for labels, sizes, sizes2, filt, mask_out, speckle in runs:
            assert np.array_equal(_np(labels), want_l) and np.array_equal(_np(sizes), want_s) and np.array_equal(_np(sizes2), want_s)
            assert np.array_equal(_bits(filt), _bits(want_f[0])) and np.array_equal(_np(mask_out), want_f[1])
            assert np.array_equal(_np(speckle), want_f[2])
        for other in runs[1:]:  # byte for byte
            assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(runs[0], other))


def test_one_graph_capture_replayed_on_new_input():
    from nndepth_amd import geometry
    shape = (3, 1, 70, 200)
    inputs = [S.scene(shape, 21), S.quantised(shape, 22), (S.constant(shape)[0], np.ones(shape, bool), 0.5)]
    buf_d, buf_m = torch.zeros(shape, dtype=torch.float32, device=DEV), torch.ones(shape, dtype=torch.bool, device=DEV)
    ws = torch.empty(geometry.regions_workspace_bytes(3, 70, 200) // 8 + 1, dtype=torch.int64, device=DEV)

    def run():
        labels, sizes = geometry.connected_regions(buf_d, 0.5, buf_m, 8, workspace=ws)
        return (labels, sizes) + geometry.speckle_filter(buf_d, 8, 0.5, buf_m, True, 8, fill=-1.0, workspace=ws)

    for _ in range(2):
        run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = run()
    torch.cuda.current_stream(DEV).wait_stream(side)
    for d, mask, _ in inputs:
        buf_d.copy_(_t(d))
        buf_m.copy_(_t(mask))
        graph.replay()
        torch.cuda.synchronize()
        want_l, want_s = S.regions(d, 0.5, mask, True, 8)
        want_f = S.speckle_filter(d, 8, 0.5, mask, True, 8, fill=-1.0)
        assert np.array_equal(_np(out[0]), want_l) and np.array_equal(_np(out[1]), want_s)
        assert np.array_equal(_bits(out[2]), _bits(want_f[0])) and np.array_equal(_np(out[3]), want_f[1])
        assert np.array_equal(_np(out[4]), want_f[2])


def test_a_workspace_that_is_too_small_is_refused_by_name():
    from nndepth_amd import geometry
    from nndepth_amd._lib import NndError
    d = torch.zeros((1, 1, 5, 7), device=DEV)
    with pytest.raises(NndError, match="workspace of 8 bytes"):
        geometry.connected_regions(d, 0.5, workspace=torch.empty(1, dtype=torch.int64, device=DEV))
    with pytest.raises(NndError, match="workspace must be a contiguous tensor"):
        geometry.connected_regions(d, 0.5, workspace=torch.empty(1000, dtype=torch.int64))
