"""GPU: the masked median and the guided weighted median through the HIP path (csrc/median.hip) against the numpy oracle of
tests/median_cases.py, which tests/test_median_cpu.py holds against the pixel loops of scripts/make_golden_median.py.  Every
comparison is an equality: the bits of the maps, the masks as integers.  The shapes straddle the tile the library reports
(nnd_median_filter_limit), the radii every selection path (the 3 x 3 and 5 x 5 networks, the windows selected in registers, the windows
selected by rows, at the largest radius with their weights in LDS).  The counts of differing elements per case (all 0) are printed
and written to tests/golden/REPORT_median.txt."""
import functools
import os

import numpy as np
import pytest
import torch

import median_cases as Mc
import speckle_cases as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPORT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "REPORT_median.txt")
HEADER = ("Masked median and guided weighted median (tests/test_gpu_median.py): elements of the HIP result (filtered, mask_out, changed)\n"
          "that differ from the numpy oracle of tests/median_cases.py, summed over the shapes and parameter sets of a case (every count must be\n"
          "0), and the share of pixels the filter changed.\n")
_lines, _sums = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if not _lines:
        return
    text = HEADER + "".join(_lines[k] for k in sorted(_lines))
    print(text)
    try:
        with open(REPORT, "w") as f:
            f.write(text)
    except OSError:
        pass  # a read-only checkout: the figures were printed


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(x):
    return x.cpu().numpy()


def _diff(got, want) -> int:
    got = _np(got) if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return int((Mc.bits(got) != Mc.bits(want)).sum()) if want.dtype == np.float32 else int((got != want).sum())


@functools.lru_cache(maxsize=None)
def _limits():
    from nndepth_amd import geometry
    return geometry.median_max_radius(), geometry.median_tile()


def _shape(s):
    th, tw = _limits()[1]
    return (2, 1, th + 3, 2 * tw + 3) if s == "tile" else s


def _radius(r):
    return _limits()[0] if r == "max" else r


@functools.lru_cache(maxsize=None)
def _builders(shape):
    """The inputs of one shape, built once and left unchanged."""
    return Mc.builders(shape)


def _step(inv_step):
    step = 1.0 / float(inv_step)
    assert np.float32(1.0 / step) == np.float32(inv_step)  # geometry.median_filter forms inv_step = float32(1 / step)
    return step


def _check(what, radius, d, mask=None, mask_is_valid=True, guide=None, inv_step=None, weights=None, min_count=1, fill_invalid=False, fill=0.0,
           mask_dev=None, dev=None, guide_dev=None):
    """The three outputs of the device against the oracle; returns the oracle's."""
    from nndepth_amd import geometry
    want = Mc.median_filter(d, radius, mask, mask_is_valid, guide, inv_step, weights, min_count, fill_invalid, fill)
    if mask is not None and mask_dev is None:
        mask_dev = _t(mask)
    if guide is not None and guide_dev is None:
        guide_dev = _t(guide)
    got = geometry.median_filter(_t(d) if dev is None else dev, radius, mask_dev, mask_is_valid, guide_dev,
                                 step=None if guide is None else _step(inv_step), weights=weights, min_count=min_count,
                                 fill_invalid=fill_invalid, fill=fill, return_changed=True)
    assert [g.dtype for g in got] == [torch.float32, torch.uint8, torch.uint8] and all(g.shape == d.shape for g in got)
    counts = [_diff(g, w) for g, w in zip(got, want)]
    key = f"{what}, radius {radius}{'' if guide is None else f', guide of {guide.shape[1]}'}"
    calls, elements, differ, moved = _sums.get(key, (0, 0, [0, 0, 0], 0))
    _sums[key] = (calls + 1, elements + d.size, [a + b for a, b in zip(differ, counts)], moved + int(want[2].sum()))
    calls, elements, differ, moved = _sums[key]
    _lines[key] = f"{key}: {calls} calls, {differ} of {elements} differ; {100 * moved / elements:.1f} % changed\n"
    assert counts == [0, 0, 0], (_lines[key], d.shape, min_count, fill_invalid)
    two = geometry.median_filter(_t(d) if dev is None else dev, radius, mask_dev, mask_is_valid, guide_dev,
                                 step=None if guide is None else _step(inv_step), weights=weights, min_count=min_count,
                                 fill_invalid=fill_invalid, fill=fill)
    assert len(two) == 2 and _diff(two[0], want[0]) == 0 and _diff(two[1], want[1]) == 0  # without `changed`
    return want


SHAPES = list(Mc.SHAPES) + ["tile", Mc.SMALL]


# ------------------------------------------------------------------------------------------------------------------ unweighted
@pytest.mark.parametrize("radius", [1, 2, 3, "max"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_unweighted_scene(shape, radius):
    shape, r = _shape(shape), _radius(radius)
    B = _builders(shape)
    full = (2 * r + 1) ** 2
    d, mask = B["scene"]["d"], B["scene"]["mask"]
    _check("scene bool mask", r, d, mask, fill=-7.0)
    _check("scene bool mask", r, d, mask, min_count=full // 2, fill_invalid=True, fill=-7.0)
    _check("scene bool mask", r, d, mask, min_count=full, fill_invalid=True, fill=3.5)
    kw = B["scene_negative_occlusion"]  # an occlusion mask, (B,H,W) uint8 with non-zero = set, on the negated map
    _check("negative, occlusion (B,H,W) uint8", r, kw["d"], kw["mask"], False, min_count=min(3, full), fill_invalid=True, fill=-2.0,
           mask_dev=_t(kw["mask"][:, 0].astype(np.uint8) * 5))
    _check("negative, occlusion (B,H,W) uint8", r, kw["d"], kw["mask"], False, fill=-2.0, mask_dev=_t(kw["mask"][:, 0].astype(np.uint8) * 5))
    _check("scene no mask", r, d)


@pytest.mark.parametrize("radius", [1, 2, 3, "max"])
@pytest.mark.parametrize("name", ["few_values", "special", "all_invalid", "checkerboard", "single"])
def test_unweighted_patterns(name, radius):
    r = _radius(radius)
    for shape in ((2, 1, 9, 40), Mc.SMALL):
        kw = dict(_builders(shape)[name])
        d = kw.pop("d")
        out, mask_out, changed = _check(name, r, d, **kw)
        _check(name + ", not fill_invalid", r, d, **{**kw, "fill_invalid": False, "min_count": min(4, (2 * r + 1) ** 2)})
        if name == "all_invalid":
            assert (out == 5.0).all() and not mask_out.any()
        elif name == "single" and r == 2 and shape == (2, 1, 9, 40):
            assert mask_out.sum() == 25


# ---------------------------------------------------------------------------------------------------------------------- guided
@pytest.mark.parametrize("radius", [1, 3, "max"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_guided(shape, radius):
    shape, r = _shape(shape), _radius(radius)
    B = _builders(shape)
    full = (2 * r + 1) ** 2
    for name, extra in (("edge_c1", {}), ("edge_c3", {}), ("edge_c3", dict(fill_invalid=False, min_count=full // 2, fill=-4.0)),
                        ("guide_nan", dict(min_count=min(5, full))), ("zeros_after_5", {}), ("zeros_after_5", dict(min_count=full)),
                        ("constant_table", dict(fill_invalid=True)), ("box_c4", {})):
        kw = {**B[name], **extra}
        d = kw.pop("d")
        want = _check(name, r, d, **kw)
        if name == "constant_table":  # a constant table gives the unweighted result
            plain = {k: v for k, v in kw.items() if k not in ("guide", "weights", "inv_step")}
            assert all(_diff(a, b) == 0 for a, b in zip(Mc.median_filter(d, r, **plain), want))
    kw = dict(B["edge_c3"])
    d, mask = kw.pop("d"), kw.pop("mask")
    _check("edge_c3 occlusion mask", r, -d, ~mask, False, **kw)
    _check("edge_c3 no mask", r, d, None, **kw)


def test_guided_median_moves_the_edge_onto_the_guides():
    from nndepth_amd import geometry
    d, _, g = Mc.edge_guide((1, 1, 9, 40), 3, 0)
    w, inv = Mc.range_weights(0.05)
    out, _ = geometry.median_filter(_t(d), 3, guide=_t(g), sigma=0.05)  # the default table: range_weights(sigma)
    assert _diff(out, Mc.median_filter(d, 3, None, True, g, inv, w)[0]) == 0
    out = _np(out)
    assert (d[0, 0, :, 20] > 20).all() and (out[0, 0, 3:6, 20] < 20).all() and (out[0, 0, 3:6, 21] > 20).all()
    for kind in ("gauss", "box"):
        w, inv = Mc.range_weights(0.1, 0.01, kind)
        out, _ = geometry.median_filter(_t(d), 2, guide=_t(g), sigma=0.1, step=0.01, kind=kind)
        assert _diff(out, Mc.median_filter(d, 2, None, True, g, inv, w)[0]) == 0


# --------------------------------------------------------------------------------------------------- strides, buffers, graphs
def test_reads_a_channel_slice_and_half_a_batch_where_they_lie():
    g = S.rng(9)
    two = g.uniform(-30.0, 3.0, (2, 2, 19, 70)).astype(np.float32)
    two[g.random(two.shape) < 0.05] = np.nan
    mask = g.random((2, 1, 19, 70)) < 0.85
    guide = g.random((2, 3, 19, 70)).astype(np.float32)
    w, inv = Mc.range_weights(0.2)
    dev = _t(two)
    for c in (0, 1):
        view = dev[:, c:c + 1]
        assert not view.is_contiguous() and view.stride(0) == 2 * 19 * 70
        _check(f"channel {c} of (2,2,19,70)", 2, np.ascontiguousarray(two[:, c:c + 1]), mask, dev=view, fill_invalid=True)
        _check(f"channel {c} of (2,2,19,70) guided", 3, np.ascontiguousarray(two[:, c:c + 1]), mask, True, guide, inv, w, dev=view)
    stacked = _t(np.concatenate([two[:, :1], two[:, 1:]], axis=0))  # (4,1,H,W): the halves of a stacked batch
    for h in (0, 1):
        half = stacked[2 * h:2 * h + 2]
        _check(f"half {h} of a stacked batch", 1, np.ascontiguousarray(two[:, h:h + 1]), mask, dev=half)
        _check(f"half {h} of a stacked batch guided", 7, np.ascontiguousarray(two[:, h:h + 1]), mask, True, guide, inv, w, dev=half)
    assert torch.equal(dev.view(torch.int32), _t(two).view(torch.int32))  # the input is not written


def _raw(d_dev, mask_dev, guide_dev, radius, table, inv_step, fillers):
    """The entry point through ctypes on buffers of our own, every output pre-filled by `fillers`."""
    from nndepth_amd._lib import check, lib
    from nndepth_amd.ops import _p, _stream
    B, _, H, W = d_dev.shape
    f_u8, f_f32 = fillers
    filtered = f_f32(torch.empty((B, 1, H, W), dtype=torch.float32, device=DEV))
    mask_out, changed = (f_u8(torch.empty((B, 1, H, W), dtype=torch.uint8, device=DEV)) for _ in range(2))
    C = 0 if guide_dev is None else guide_dev.shape[1]
    check(lib.nnd_median_filter(_p(d_dev), H * W, _p(mask_dev), 1, radius, 2, 1, -2.0, _p(guide_dev), C, float(inv_step),
                                None if guide_dev is None else table.ctypes.data, _p(filtered), _p(mask_out), _p(changed), B, H, W,
                                _stream(d_dev.device)), "median_filter")
    return filtered, mask_out, changed


@pytest.mark.parametrize("radius,guided", [(1, False), (3, False), (3, True), ("max", False), ("max", True)])
def test_same_bytes_on_every_run_and_whatever_the_outputs_held(radius, guided):
    r = _radius(radius)
    shape = _shape("tile")
    kw = _builders(shape)["edge_c3"]
    d, mask, guide = kw["d"], kw["mask"], kw["guide"] if guided else None
    table, inv = kw["weights"], kw["inv_step"]
    dd, mm, gg = _t(d), _t(mask.view(np.uint8)), None if guide is None else _t(guide)
    zero = lambda t: t.zero_()  # noqa: E731
    ones = lambda t: t.view(torch.uint8).fill_(0xFF).view(t.dtype).view(t.shape) if t.dtype != torch.uint8 else t.fill_(0xFF)  # noqa: E731
    nans = lambda t: t.fill_(float("nan")) if t.dtype == torch.float32 else t.fill_(0x7F)  # noqa: E731
    want = Mc.median_filter(d, r, mask, True, guide, inv, table, 2, True, -2.0)
    runs = [_raw(dd, mm, gg, r, table, inv, f) for f in ((zero, zero), (zero, zero), (ones, ones), (nans, nans))]
    torch.cuda.synchronize()
    for i, run in enumerate(runs):
        counts = [_diff(g, w) for g, w in zip(run, want)]
        _lines[f"zz buffers r{r} guided {int(guided)} run {i}"] = f"pre-filled outputs, r{r}{' guided' if guided else ''}, run {i}: {counts} differ\n"
        assert counts == [0, 0, 0]
    for other in runs[1:]:  # byte for byte
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(runs[0], other))


def test_one_graph_capture_replayed_on_new_input():
    from nndepth_amd import geometry
    shape = _shape("tile")
    rmax = _limits()[0]
    inputs = [_builders(shape)["edge_c3"], _builders(shape)["guide_nan"]]
    table, inv = Mc.range_weights(0.2)
    buf_d, buf_m = torch.zeros(shape, dtype=torch.float32, device=DEV), torch.ones(shape, dtype=torch.bool, device=DEV)
    buf_g = torch.zeros((shape[0], 3) + shape[2:], dtype=torch.float32, device=DEV)

    def run():
        return (geometry.median_filter(buf_d, 1, buf_m, fill_invalid=True, fill=-1.0, return_changed=True)
                + geometry.median_filter(buf_d, 2, buf_m, guide=buf_g, sigma=0.2, return_changed=True)
                + geometry.median_filter(buf_d, rmax, buf_m, guide=buf_g, sigma=0.2, min_count=9, return_changed=True))

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
    for kw in inputs:
        d, mask, g = kw["d"], kw["mask"], kw["guide"]
        buf_d.copy_(_t(d))
        buf_m.copy_(_t(mask))
        buf_g.copy_(_t(g))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [o.clone() for o in out]
        direct = run()
        torch.cuda.synchronize()
        want = (Mc.median_filter(d, 1, mask, fill_invalid=True, fill=-1.0) + Mc.median_filter(d, 2, mask, True, g, inv, table)
                + Mc.median_filter(d, rmax, mask, True, g, inv, table, 9))
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(replayed, direct))
        assert [_diff(a, w) for a, w in zip(replayed, want)] == [0] * 9


# ----------------------------------------------------------------------------------------------------------- the scene methods
def test_scene_methods():
    from nndepth_amd.scene import Depth, Disparity, Frame
    shape = (2, 1, 19, 70)
    d, mask = Mc.scene(shape, 77, "negative")
    guide = S.rng(2).random((2, 3, 19, 70)).astype(np.float32)
    w, inv = Mc.range_weights(0.2)
    w2, inv2 = Mc.range_weights(0.1, 0.01, "gauss")
    dd, gg = _t(d), _t(guide)
    for occ_dev, dtype in ((_t(~mask), torch.bool), (None, torch.uint8)):
        m = None if occ_dev is None else ~mask
        disp = Disparity(dd, "negative", occlusion=occ_dev, baseline=0.3)
        for got, want in ((disp.median_filter(), Mc.median_filter(d, 1, m, False)),
                          (disp.median_filter(2, fill_invalid=True, min_count=4), Mc.median_filter(d, 2, m, False, min_count=4, fill_invalid=True)),
                          (disp.median_filter(2, guide=Frame(gg)), Mc.median_filter(d, 2, m, False, guide, inv, w)),
                          (disp.median_filter(3, gg, 0.1, step=0.01, kind="gauss"), Mc.median_filter(d, 3, m, False, guide, inv2, w2))):
            assert isinstance(got, Disparity) and got.disp_sign == "negative" and got.baseline == 0.3 and got.occlusion.dtype == dtype
            assert got.occlusion.shape == shape and _diff(got.data, want[0]) == 0 and np.array_equal(_np(got.occlusion) != 0, want[1] != 0)
    # a (C,H,W) picture in a Frame guides a batch of one
    one = Disparity(dd[:1], "negative").median_filter(2, guide=Frame(gg[0]))
    assert _diff(one.data, Mc.median_filter(d[:1], 2, None, True, guide[:1], inv, w)[0]) == 0
    z = np.abs(d) + np.float32(1)
    zz = _t(z)
    for valid_dev, dtype in ((_t(mask), torch.bool), (_t(mask[:, 0].astype(np.uint8)), torch.uint8), (None, torch.uint8)):
        m = None if valid_dev is None else mask
        for inverse in (False, True):
            depth = Depth(zz, valid_mask=valid_dev, is_inverse=inverse)
            for got, want in ((depth.median_filter(2, fill_invalid=True), Mc.median_filter(z, 2, m, True, fill_invalid=True)),
                              (depth.median_filter(1, Frame(gg), min_count=3), Mc.median_filter(z, 1, m, True, guide, inv, w, 3))):
                assert isinstance(got, Depth) and got.is_inverse == inverse and got.valid_mask.dtype == dtype
                assert _diff(got.data, want[0]) == 0 and np.array_equal(_np(got.valid_mask) != 0, want[1] != 0)


def test_the_chain_remove_speckles_fill_holes_median_filter():
    import warp_cases as Wc
    from nndepth_amd.scene import Disparity, Frame
    shape = (2, 1, 33, 130)
    d, mask = Mc.scene(shape, 21, "negative")
    guide = S.rng(3).random((2, 3, 33, 130)).astype(np.float32)
    w, inv = Mc.range_weights(0.2)
    left = Frame(_t(guide))
    got = Disparity(_t(d), "negative", occlusion=_t(~mask)).remove_speckles(8, 0.5, 8).fill_holes("background").median_filter(2, guide=left)
    filt, occ, _, _ = S.speckle_filter(d, 8, 0.5, ~mask, False, 8)
    filled, _, occ2 = Wc.fill_holes(filt, occ, False, "min_abs", True)
    want = Mc.median_filter(filled, 2, occ2, False, guide, inv, w)
    counts = [_diff(got.data, want[0]), int((_np(got.occlusion) != (want[1] != 0)).sum())]
    _lines["zz chain"] = f"remove_speckles(8, 0.5, 8).fill_holes('background').median_filter(2, guide=left) {shape}: {counts} differ\n"
    assert counts == [0, 0] and got.occlusion.dtype == torch.bool


def test_refusals_on_the_device_by_name():
    from nndepth_amd import geometry
    from nndepth_amd._lib import NndError
    d = torch.zeros((2, 1, 5, 7), device=DEV)
    rmax = _limits()[0]
    for r in (0, rmax + 1):
        with pytest.raises(NndError, match="radius"):
            geometry.median_filter(d, r)
    for r, mc in ((1, 0), (1, 10), (2, 26)):
        with pytest.raises(NndError, match="min_count"):
            geometry.median_filter(d, r, min_count=mc)
    with pytest.raises(NndError, match=r"the mask is \(2, 5, 6\)"):
        geometry.median_filter(d, valid_mask=torch.ones((2, 5, 6), dtype=torch.bool, device=DEV))
    with pytest.raises(NndError, match="the guide is on cpu"):
        geometry.median_filter(d, guide=torch.zeros((2, 3, 5, 7)))
    with pytest.raises(NndError, match=r"the guide is \(B,C,H,W\)"):
        geometry.median_filter(d, guide=torch.zeros((2, 5, 5, 7), device=DEV))
    g = torch.zeros((2, 3, 5, 7), device=DEV)
    with pytest.raises(NndError, match="weights are 256 uint16"):
        geometry.median_filter(d, guide=g, weights=np.ones(255, np.uint16))
    with pytest.raises(NndError, match=r"weights\[0\] is 0"):
        geometry.median_filter(d, guide=g, weights=np.zeros(256, np.uint16))
    with pytest.raises(NndError, match="weights without a guide"):
        geometry.median_filter(d, weights=np.ones(256, np.uint16))
