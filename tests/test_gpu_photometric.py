"""GPU: view synthesis and the photometric error through the HIP path (csrc/photometric.hip) against the numpy oracle of
tests/photometric_cases.py, which tests/test_photometric_cpu.py holds against the pixel loops of
scripts/make_golden_photometric.py and against the Monodepth composition.  Every comparison of a map, a mask or a count is an
equality: the bits of the maps, the masks and counts as integers.  The sums of `stats` are held to N * 2^-52 relative of
math.fsum over the oracle's valid values, the bound for adding N non-negative doubles in any order.  The shapes straddle the
tile the library reports (nnd_photometric_limit).  The counts of differing elements per case (all 0) are printed and written to
tests/golden/REPORT_photometric.txt."""
import functools
import os

import numpy as np
import pytest
import torch

import photometric_cases as Pc
import speckle_cases as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPORT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "REPORT_photometric.txt")
CPU_MARK = "-- the contract against the Monodepth composition (tests/test_photometric_cpu.py) --\n"
HEADER = ("View synthesis and photometric error (tests/test_gpu_photometric.py): elements of the HIP result (recon, in, error, valid, l1,\n"
          "dssim) that differ from the numpy oracle of tests/photometric_cases.py, summed over the shapes and parameter sets of a case\n"
          "(every count must be 0), the share of valid pixels, and the largest relative deviation of a sum of `stats` from math.fsum in\n"
          "units of N * 2^-52 (must be <= 1).\n")
_lines, _sums = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if not _lines:
        return
    text = HEADER + "".join(_lines[k] for k in sorted(_lines))
    print(text)
    try:
        old = open(REPORT).read() if os.path.exists(REPORT) else ""
        tail = CPU_MARK + old.split(CPU_MARK)[1] if CPU_MARK in old else ""
        with open(REPORT, "w") as f:
            f.write(text + tail)
    except OSError:
        pass  # a read-only checkout: the figures were printed


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(x):
    return x.cpu().numpy()


def _diff(got, want) -> int:
    got = _np(got) if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return int((Pc.bits(got) != Pc.bits(want)).sum()) if want.dtype == np.float32 else int((got != want).sum())


@functools.lru_cache(maxsize=None)
def _tile():
    from nndepth_amd import geometry
    return geometry.photometric_tile()


def _shapes():
    th, tw = _tile()
    return Pc.SMALL_SHAPES + [(1, 3, th, tw), (2, 3, th + 3, 2 * tw + 3), (1, 4, 2 * th + 1, tw - 1), (2, 3, 19, 131)]


@functools.lru_cache(maxsize=None)
def _builders(shape):
    """The inputs of one shape, built once and left unchanged."""
    return Pc.builders(shape)


def _stats_close(got, want):
    """count equal; every sum within N * 2^-52 relative of math.fsum; returns the largest deviation in units of that bound."""
    assert got.shape == want.shape and got.dtype == np.float64 and np.isfinite(got).all()
    assert np.array_equal(got[:, 0], want[:, 0])
    worst = 0.0
    for b in range(got.shape[0]):
        bound = max(got[b, 0], 1.0) * 2.0 ** -52
        for k in (1, 2, 3):
            dev = abs(got[b, k] - want[b, k])
            assert dev <= bound * abs(want[b, k]), (b, k, got[b, k], want[b, k])
            if want[b, k] != 0:
                worst = max(worst, dev / (bound * abs(want[b, k])))
    return worst


def _check(what, target, other, d, mask=None, mask_is_valid=True, disp_sign="negative", target_view="left", ssim_weight=0.85,
           data_range=2.0, fill=0.0, mask_dev=None, disp_dev=None):
    """Every output of the two device calls against the oracle; returns the oracle's (error, valid, l1, dssim, ok)."""
    from nndepth_amd import geometry
    want = Pc.photometric_error(target, other, d, mask, mask_is_valid, disp_sign, target_view, ssim_weight, data_range, fill)
    wrecon, win = Pc.synthesize_view(other, d, mask, mask_is_valid, disp_sign, target_view, fill)
    if mask is not None and mask_dev is None:
        mask_dev = _t(mask)
    tt, oo, dd = _t(target), _t(other), _t(d) if disp_dev is None else disp_dev
    recon, inn = geometry.synthesize_view(oo, dd, disp_sign, target_view, mask_dev, mask_is_valid, fill)
    error, valid, stats, l1, dssim = geometry.photometric_error(tt, oo, dd, disp_sign, target_view, mask_dev, mask_is_valid, ssim_weight,
                                                                data_range, fill, return_parts=True)
    assert [g.dtype for g in (recon, inn, error, valid, l1, dssim, stats)] == [torch.float32, torch.uint8] * 2 + [torch.float32] * 2 + [torch.float64]
    counts = [_diff(g, w) for g, w in zip((recon, inn, error, valid, l1, dssim), (wrecon, win) + want[:4])]
    wstats = Pc.stats_of(want[0], want[2], want[3], want[4], ssim_weight)
    dev = _stats_close(_np(stats), wstats)
    calls, elements, differ, nvalid, worst = _sums.get(what, (0, 0, [0] * 6, 0, 0.0))
    _sums[what] = (calls + 1, elements + d.size, [a + b for a, b in zip(differ, counts)], nvalid + int(want[4].sum()), max(worst, dev))
    calls, elements, differ, nvalid, worst = _sums[what]
    _lines[what] = f"{what}: {calls} calls, {differ} of {elements} pixels differ; {100 * nvalid / elements:.0f} % valid; stats {worst:.3f}\n"
    assert counts == [0] * 6, (_lines[what], target.shape, ssim_weight)
    three = geometry.photometric_error(tt, oo, dd, disp_sign, target_view, mask_dev, mask_is_valid, ssim_weight, data_range, fill, stats=False)
    assert len(three) == 3 and three[2] is None and _diff(three[0], want[0]) == 0 and _diff(three[1], want[1]) == 0  # maps alone
    return want


def _run(name, kw, **extra):
    kw = {**kw, **extra}
    return _check(name, kw.pop("target"), kw.pop("other"), kw.pop("d"), **kw)


# ------------------------------------------------------------------------------------------------------------ shapes and builders
@pytest.mark.parametrize("index", range(7))
def test_every_builder_at_every_shape(index):
    shape = _shapes()[index]
    for name, kw in _builders(shape).items():
        _run(name, kw)
        _run(name, kw, ssim_weight=0.0, fill=-7.0)
        _run(name, kw, ssim_weight=1.0, fill=-7.0, data_range=1.0)


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_channel_counts(C):
    th, tw = _tile()
    for shape in ((2, C, 2, 2), (2, C, 11, tw + 5)):
        B = _builders(shape)
        for name in ("small_m", "scene", "scene_right", "scene_positive_occlusion", "special_pictures"):
            _run(f"C = {C}", B[name])
            _run(f"C = {C}", B[name], ssim_weight=0.0)


def test_non_finite_pictures_invalidate_their_windows_and_stats_stay_finite():
    from nndepth_amd import geometry
    shape = (2, 3, 19, 131)
    kw = _builders(shape)["special_pictures"]
    want = _run("special_pictures", kw)
    ok = want[4][:, 0]
    bad = ~np.isfinite(kw["target"]).all(1)
    p = np.pad(bad, ((0, 0), (1, 1), (1, 1)))
    grown = np.any([p[:, dy:dy + 19, dx:dx + 131] for dy in range(3) for dx in range(3)], axis=0)
    assert bad.any() and grown.sum() > bad.sum() and not ok[grown].any() and ok.mean() >= 0.25
    stats = geometry.photometric_error(_t(kw["target"]), _t(kw["other"]), _t(kw["d"]), valid_mask=_t(kw["mask"]))[2]
    assert torch.isfinite(stats).all() and (stats[:, 0] > 0).all()


def test_mask_dtypes_and_polarities():
    shape = (2, 3, 19, 131)
    kw = _builders(shape)["scene"]
    t, o, d, m = kw["target"], kw["other"], kw["d"], kw["mask"]
    a = _check("masks", t, o, d, m, True, fill=-7.0)                                                    # bool, (B,1,H,W)
    b = _check("masks", t, o, d, m, True, fill=-7.0, mask_dev=_t(m[:, 0].astype(np.uint8) * 5))       # uint8, (B,H,W), non-zero = set
    c = _check("masks", t, o, d, ~m, False, fill=-7.0)                                                  # an occlusion mask, bool
    e = _check("masks", t, o, d, ~m, False, fill=-7.0, mask_dev=_t((~m).astype(np.uint8) * 255))
    for other in (b, c, e):
        assert _diff(other[0], a[0]) == 0 and np.array_equal(other[4], a[4])
    assert np.array_equal(c[1], 1 - a[1]) and np.array_equal(a[1] != 0, a[4])  # the mask comes back in the polarity it was read in


def test_both_signs_and_both_views():
    shape = (2, 3, 19, 131)
    kw = _builders(shape)["scene"]
    t, o, d, m = kw["target"], kw["other"], kw["d"], kw["mask"]
    a = _check("signs", t, o, d, m)
    b = _check("signs", t, o, -d, m, disp_sign="positive")
    assert _diff(a[0], b[0]) == 0
    kw = _builders(shape)["scene_right"]
    c = _check("views", kw["target"], kw["other"], kw["d"], kw["mask"], target_view="right")
    assert c[4].mean() >= 0.25


def test_reads_a_channel_slice_and_half_a_batch_where_they_lie():
    shape = (2, 3, 19, 131)
    kw = _builders(shape)["scene"]
    t, o, d, m = kw["target"], kw["other"], kw["d"], kw["mask"]
    g = S.rng(9)
    two = np.concatenate([d, g.uniform(-30.0, 3.0, d.shape).astype(np.float32)], axis=1)  # (2,2,H,W): the map is channel 0
    view = _t(two)[:, :1]
    assert not view.is_contiguous() and view.stride(0) == 2 * 19 * 131
    _check("channel 0 of a 2-channel tensor", t, o, d, m, disp_dev=view)
    stacked = _t(np.concatenate([two[:, 1:], d], axis=0))  # (4,1,H,W): the map is the second half of a stacked batch
    _check("half of a stacked batch", t, o, d, m, disp_dev=stacked[2:])
    _check("half of a stacked batch", t, o, np.ascontiguousarray(two[:, 1:]), m, disp_dev=stacked[:2])


def test_a_consistent_pair_scores_exactly_zero():
    th, tw = _tile()
    for shape, k in (((2, 3, 9, 40), 0), ((2, 3, 9, 40), 3), ((1, 4, th + 3, tw + 9), 5), ((2, 1, 5, 7), 1)):
        t, o, d = Pc.consistent(shape, k, 5 + k)
        for w in (0.85, 1.0, 0.0):
            error, _, _, _, ok = _check("consistent", t, o, d, ssim_weight=w, fill=-7.0)
            assert ok.sum() > 0 and (Pc.bits(error[ok]) == 0).all()  # rec == t: n == dn bit for bit


def test_synthesize_view_gives_the_bits_of_the_reconstruction_inside_the_fused_call():
    """Device against device: with one channel, a zero target, data_range 1 and ssim_weight 0 the fused call's error is
    fabsf(0 - rec) * 1.0f * 1.0f, the bits of rec for a picture that is nowhere negative."""
    from nndepth_amd import geometry
    th, tw = _tile()
    for shape in ((2, 3, 19, 131), (1, 4, 2 * th + 1, tw - 1)):
        for name, view, sign in (("scene", "left", "negative"), ("scene_right", "right", "negative"), ("integer_half", "left", "negative")):
            kw = _builders(shape)[name]
            dd, mm = _t(kw["d"]), None if kw.get("mask") is None else _t(kw["mask"])
            other = _t(np.abs(kw["other"]))
            recon, inn = geometry.synthesize_view(other, dd, sign, view, mm, fill=-7.0)
            for c in range(shape[1]):
                one = other[:, c:c + 1].contiguous()
                error, valid, _ = geometry.photometric_error(torch.zeros_like(one), one, dd, sign, view, mm, ssim_weight=0.0, data_range=1.0,
                                                             fill=-7.0, stats=False)
                assert torch.equal(valid, inn) and (valid != 0).float().mean() >= 0.25
                assert torch.equal(error.view(torch.int32), recon[:, c:c + 1].view(torch.int32)), (shape, name, c)


# ----------------------------------------------------------------------------------------------- buffers, history, graphs, stats
def _raw(tt, oo, dd, mm, fillers, w=0.85):
    """The entry point through ctypes on buffers of our own, every output and the workspace pre-filled by `fillers`."""
    from nndepth_amd import geometry
    from nndepth_amd._lib import check, lib
    from nndepth_amd.ops import _p, _stream
    B, C, H, W = tt.shape
    f_u8, f_f32, f_f64 = fillers
    error, l1, dssim = (f_f32(torch.empty((B, 1, H, W), dtype=torch.float32, device=DEV)) for _ in range(3))
    valid = f_u8(torch.empty((B, 1, H, W), dtype=torch.uint8, device=DEV))
    stats = f_f64(torch.empty((B, 4), dtype=torch.float64, device=DEV))
    ws = f_f64(torch.empty(geometry.photometric_workspace_bytes(B, H, W) // 8, dtype=torch.float64, device=DEV))
    c1, c2, inv = (float(v) for v in Pc.constants(2.0))
    check(lib.nnd_photometric_error(_p(tt), _p(oo), _p(dd), H * W, _p(mm), 1, 1, 1, w, c1, c2, inv, -2.0, _p(error), _p(l1), _p(dssim),
                                    _p(valid), _p(stats), _p(ws), ws.numel() * 8, B, C, H, W, _stream(tt.device)), "photometric_error")
    return error, valid, l1, dssim, stats


@pytest.mark.parametrize("w", [0.85, 0.0])
def test_same_bytes_on_every_run_and_whatever_outputs_and_workspace_held(w):
    th, tw = _tile()
    shape = (2, 3, th + 3, 2 * tw + 3)
    kw = _builders(shape)["scene"]
    tt, oo, dd, mm = _t(kw["target"]), _t(kw["other"]), _t(kw["d"]), _t(kw["mask"].view(np.uint8))
    zero = lambda t: t.zero_()  # noqa: E731
    ones = lambda t: t.view(torch.uint8).fill_(0xFF).view(t.dtype).view(t.shape) if t.dtype != torch.uint8 else t.fill_(0xFF)  # noqa: E731
    want = Pc.photometric_error(kw["target"], kw["other"], kw["d"], kw["mask"], ssim_weight=w, fill=-2.0)
    wstats = Pc.stats_of(want[0], want[2], want[3], want[4], w)
    runs = [_raw(tt, oo, dd, mm, f, w) for f in ((ones,) * 3, (ones,) * 3, (zero,) * 3)]
    torch.cuda.synchronize()
    for i, run in enumerate(runs):
        counts = [_diff(g, x) for g, x in zip(run[:4], want[:4])]
        _lines[f"zz buffers w{w} run {i}"] = f"pre-filled outputs and workspace, ssim_weight {w}, run {i}: {counts} differ\n"
        assert counts == [0, 0, 0, 0]
        _stats_close(_np(run[4]), wstats)
    for other in runs[1:]:  # byte for byte, the statistics included
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(runs[0], other))


def test_one_graph_capture_with_a_passed_workspace():
    from nndepth_amd import geometry
    th, tw = _tile()
    shape = (2, 3, th + 3, 2 * tw + 3)
    B = _builders(shape)
    bt, bo = (torch.zeros(shape, dtype=torch.float32, device=DEV) for _ in range(2))
    bd = torch.zeros((shape[0], 1) + shape[2:], dtype=torch.float32, device=DEV)
    bm = torch.ones(bd.shape, dtype=torch.bool, device=DEV)
    ws = torch.empty(geometry.photometric_workspace_bytes(shape[0], shape[2], shape[3]) // 8, dtype=torch.float64, device=DEV)

    def run():
        return (geometry.photometric_error(bt, bo, bd, valid_mask=bm, return_parts=True, workspace=ws, fill=-1.0)
                + geometry.synthesize_view(bo, bd, valid_mask=bm))

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
    for name in ("scene", "special_disp"):
        kw = B[name]
        for buf, a in ((bt, kw["target"]), (bo, kw["other"]), (bd, kw["d"]), (bm, kw["mask"])):
            buf.copy_(_t(a))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [o.clone() for o in out]
        direct = run()
        torch.cuda.synchronize()
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(replayed, direct))
        want = Pc.photometric_error(kw["target"], kw["other"], kw["d"], kw["mask"], fill=-1.0)
        assert [_diff(replayed[i], want[j]) for i, j in ((0, 0), (1, 1), (3, 2), (4, 3))] == [0] * 4
        assert _diff(replayed[5], Pc.synthesize_view(kw["other"], kw["d"], kw["mask"])[0]) == 0


# ------------------------------------------------------------------------------------------------ the score and the scene methods
def test_photometric_score_equals_the_two_steps():
    from nndepth_amd import geometry
    from nndepth_amd.scene import Disparity
    shape = (2, 3, 19, 131)
    kw = _builders(shape)["scene_no_mask"]
    left, right = _t(kw["target"]), _t(kw["other"])
    up = _t(np.concatenate([kw["d"], np.zeros_like(kw["d"])], axis=1))  # a 2-channel output whose channel 0 is the map
    calls = []

    def forward(a, b):
        calls.append((a, b))
        return [{"up_disp": up}]

    disp, error, stats = geometry.photometric_score(forward, left, right, threshold=0.5, ssim_weight=0.5, fill=-7.0)
    assert len(calls) == 1 and calls[0][0] is left and calls[0][1] is right and isinstance(disp, Disparity)
    two = geometry.occlusion_from_warp(forward, left, right, 0.5)
    e2, _, s2 = geometry.photometric_error(left, right, two.data, valid_mask=two.occlusion, mask_is_valid=False, ssim_weight=0.5, fill=-7.0)
    assert torch.equal(disp.occlusion, two.occlusion) and torch.equal(error.view(torch.int32), e2.view(torch.int32))
    assert torch.equal(stats.view(torch.int64), s2.view(torch.int64))
    occ = _np(disp.occlusion) != 0
    want = Pc.photometric_error(kw["target"], kw["other"], kw["d"], occ, False, ssim_weight=0.5, fill=-7.0)
    assert _diff(error, want[0]) == 0 and 0.25 <= want[4].mean() < 1.0 and occ.any()


def test_scene_methods():
    from nndepth_amd.scene import Disparity, Frame
    shape = (2, 3, 19, 131)
    kw = _builders(shape)["scene"]
    t, o, d, mask = kw["target"], kw["other"], kw["d"], kw["mask"]
    tt, oo, dd = _t(t), _t(o), _t(d)
    for occ_dev, dtype in ((_t(~mask), torch.bool), (_t((~mask).astype(np.uint8)), torch.uint8), (None, torch.uint8)):
        m = None if occ_dev is None else ~mask
        disp = Disparity(dd, "negative", occlusion=occ_dev, baseline=0.3)
        recon, inv = disp.synthesize(Frame(oo))
        wrecon, winv = Pc.synthesize_view(o, d, m, False)
        assert inv.dtype == dtype and _diff(recon, wrecon) == 0 and np.array_equal(_np(inv) != 0, winv != 0)
        want = Pc.photometric_error(t, o, d, m, False, fill=-7.0)
        for frame, other in ((Frame(tt), Frame(oo)), (tt, oo)):
            got = disp.photometric_error(frame, other, fill=-7.0, return_parts=True)
            assert len(got) == 5 and got[1].dtype == dtype and got[2].shape == (2, 4)
            assert [_diff(got[i], want[j]) for i, j in ((0, 0), (3, 2), (4, 3))] == [0, 0, 0]
            assert np.array_equal(_np(got[1]) != 0, ~want[4])  # the polarity of the occlusion: 1 = no trusted error here
            assert np.array_equal(_np(got[2])[:, 0], want[4].reshape(2, -1).sum(1).astype(np.float64))
    # a right-view map, positive sign; a (C,H,W) picture in a Frame beside a batch of one
    kw = _builders(shape)["scene_right"]
    right = Disparity(_t(-kw["d"]), "positive", occlusion=_t(~kw["mask"]))
    got = right.photometric_error(_t(kw["target"]), _t(kw["other"]), view="right", ssim_weight=1.0)
    assert len(got) == 3 and _diff(got[0], Pc.photometric_error(kw["target"], kw["other"], -kw["d"], ~kw["mask"], False, "positive", "right", 1.0)[0]) == 0
    one = Disparity(dd[:1], "negative").synthesize(Frame(oo[0]))[0]
    assert _diff(one, Pc.synthesize_view(o[:1], d[:1])[0]) == 0


def test_refusals_on_the_device_by_name():
    from nndepth_amd import geometry
    from nndepth_amd._lib import NndError
    d = torch.zeros((2, 1, 5, 7), device=DEV)
    p = torch.zeros((2, 3, 5, 7), device=DEV)
    with pytest.raises(NndError, match=r"the mask is \(2, 5, 6\)"):
        geometry.photometric_error(p, p, d, valid_mask=torch.ones((2, 5, 6), dtype=torch.bool, device=DEV))
    with pytest.raises(NndError, match="the other picture is on cpu"):
        geometry.photometric_error(p, p.cpu(), d)
    with pytest.raises(NndError, match="the other picture is on cpu"):
        geometry.synthesize_view(p.cpu(), d)
    with pytest.raises(NndError, match="H and W must be at least 2"):
        geometry.synthesize_view(torch.zeros((2, 3, 1, 7), device=DEV), torch.zeros((2, 1, 1, 7), device=DEV))
    with pytest.raises(NndError, match="a workspace of 8 bytes"):
        geometry.photometric_error(p, p, d, workspace=torch.zeros(1, dtype=torch.float64, device=DEV))
    with pytest.raises(NndError, match="must not be an input"):  # the entry point itself: an output that aliases an input
        from nndepth_amd._lib import check, lib
        from nndepth_amd.ops import _p, _stream
        check(lib.nnd_synthesize_view(_p(p), _p(d), 35, None, 1, 1, 1, 0.0, _p(p), None, 2, 3, 5, 7, _stream(p.device)), "synthesize_view")
