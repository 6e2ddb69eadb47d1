"""GPU: the view warp, its occlusion and hole filling through the HIP path (csrc/warp.hip) against the numpy oracles of
tests/warp_cases.py, which tests/test_warp_cpu.py holds against the pixel loops of scripts/make_golden_warp.py.  Every comparison
is an equality: the bits of maps and features, masks and sources as integers.  The widths straddle the chunks the library reports
(nnd_warp_disparity_limit(1), nnd_fill_holes_chunk).  The counts of differing elements per case (all 0) and the collision
statistics of every warp input are printed and written to tests/golden/REPORT_warp_fill.txt."""
import functools
import os

import numpy as np
import pytest
import torch

import speckle_cases as S
import warp_cases as Wc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPORT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "REPORT_warp_fill.txt")
HEADER = ("View warp and hole filling (tests/test_gpu_warp.py): elements of the HIP result that differ from the numpy oracle of\n"
          "tests/warp_cases.py, per output (every count must be 0), and for a warp the shares of its input: targets with >= 2 and >= 3\n"
          "sources, landed sources that are occluded, targets that are holes.\n")
_lines = {}


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
    return int((Wc.bits(got) != Wc.bits(want)).sum()) if want.dtype == np.float32 else int((got != want).sum())


@functools.lru_cache(maxsize=None)
def _chunks():
    from nndepth_amd import geometry
    return geometry.warp_chunk(), geometry.fill_chunk()


def _shapes():
    return list(Wc.SHAPES) + ["warp_chunk", "fill_chunk"]


def _shape(s):
    return (2, 1, 9, 2 * _chunks()[0 if s == "warp_chunk" else 1] + 3) if isinstance(s, str) else s


def _check_warp(what, d, sign, view, thr, mask=None, mask_dev=None, features=None, fill=0.0, dev=None):
    """The five outputs of the device against the oracle; returns the oracle's."""
    from nndepth_amd import geometry
    want = Wc.warp(d, sign, view, thr, mask, features, fill)
    if mask is not None and mask_dev is None:
        mask_dev = _t(mask)
    got = geometry.warp_disparity(_t(d) if dev is None else dev, sign, view, thr, mask_dev, None if features is None else _t(features),
                                  fill, return_source=True)
    assert len(got) == (4 if features is None else 5)
    assert [g.dtype for g in got[:4]] == [torch.float32, torch.uint8, torch.uint8, torch.int32] and all(g.shape == d.shape for g in got[:4])
    counts = [_diff(g, w) for g, w in zip(got, want)]
    c = Wc.collisions(d, sign, view, mask, thr)
    what = f"{what} {sign} {view} {thr}"
    _lines[what] = (f"warp {what} {d.shape} {sign} to {view}, threshold {thr}: {counts} of {d.size} differ; two {100 * c['two']:.2f} % "
                    f"three {100 * c['three']:.2f} % occluded {100 * c['occluded_of_landed']:.2f} % holes {100 * c['holes']:.2f} %\n")
    assert counts == [0] * len(counts), _lines[what]
    return want


def _check_fill(what, d, mask, pol, rule, vertical, fill=0.0, mask_dev=None, dev=None):
    from nndepth_amd import geometry
    want = Wc.fill_holes(d, mask, pol, rule, vertical, fill)
    if mask is not None and mask_dev is None:
        mask_dev = _t(mask)
    got = geometry.fill_holes(_t(d) if dev is None else dev, mask_dev, pol, rule, vertical, fill)
    assert [g.dtype for g in got] == [torch.float32, torch.uint8, torch.uint8] and all(g.shape == d.shape for g in got)
    counts = [_diff(g, w) for g, w in zip(got, want)]
    label, what = what, f"{what} {rule} {vertical} {pol}"
    _lines[what] = (f"fill {label} {d.shape} {rule}{'' if vertical else ', rows only'}{'' if pol else ', occlusion mask'}: {counts} of {d.size} differ; "
                    f"{int(want[1].sum())} filled\n")
    assert counts == [0] * 3, _lines[what]
    return want


# ------------------------------------------------------------------------------------------------------------------------ warp
@pytest.mark.parametrize("sign,view", [("negative", "right"), ("positive", "right"), ("negative", "left"), ("positive", "left")])
@pytest.mark.parametrize("shape", _shapes(), ids=str)
def test_warp_scene(shape, sign, view):
    shape = _shape(shape)
    B, _, H, W = shape
    d, mask = Wc.scene(shape, 77, sign)
    g = S.rng(shape[2] * shape[3])
    f3, f1 = g.random((B, 3, H, W)).astype(np.float32), g.random((B, 1, H, W)).astype(np.float32)
    f3[0, 0, 0, 0] = -0.0  # copied bit for bit
    key = f"scene {shape} {sign} {view}"
    _check_warp(key + " bool mask", d, sign, view, 1.0, mask, None, f3, fill=-7.0)
    _check_warp(key + " uint8 (B,H,W) mask", d, sign, view, 0.25, mask, _t(mask[:, 0].astype(np.uint8) * 5))  # non-zero = set
    _check_warp(key + " no mask", d, sign, view, 1.0, None, None, f1)
    if shape == (3, 1, 70, 200):  # conditions on the input alone
        c = Wc.collisions(d, sign, view, mask)
        assert c["two"] >= 0.05 and c["three"] > 0.002 and c["occluded_of_landed"] > 0.05 and c["holes"] > 0.1, c


def _patterns():
    inf = float("inf")
    return {  # name: (d, sign, view, threshold)
        "ties_left": (Wc.half_integer((2, 1, 3, 9)), "positive", "left", 1.0),
        "ties_right": (Wc.half_integer((2, 1, 3, 9)), "positive", "right", 1.0),
        "ties_left_negative": (-Wc.half_integer((1, 1, 2, 12), 2.5), "negative", "left", 0.0),
        "ties_right_wide": (Wc.half_integer((1, 1, 2, 2 * _chunks()[0] + 3), 1.5), "positive", "right", 1.0),
        "out_of_frame_right": (np.full((2, 1, 5, 7), -9.0, np.float32), "negative", "right", 1.0),
        "out_of_frame_left": (np.full((2, 1, 5, 7), 7.5, np.float32), "positive", "left", inf),
        "special": (Wc.special(), "positive", "right", 1.0),
        "special_inf": (Wc.special(), "positive", "left", inf),
        "special_negative": (-Wc.special(), "negative", "right", 0.0),
        "bar": (Wc.bar(), "positive", "right", Wc.BAR_THRESHOLD),
        "bar_ulp": (Wc.bar(ulp=True), "positive", "right", Wc.BAR_THRESHOLD),
        "bar_ulp_inf": (Wc.bar(ulp=True), "positive", "right", inf),
        "zero_threshold": (Wc.scene((2, 1, 9, 40), 3, "positive")[0], "positive", "right", 0.0),
    }


@pytest.mark.parametrize("name", ["ties_left", "ties_right", "ties_left_negative", "ties_right_wide", "out_of_frame_right", "out_of_frame_left",
                                  "special", "special_inf", "special_negative", "bar", "bar_ulp", "bar_ulp_inf", "zero_threshold"])
def test_warp_patterns(name):
    d, sign, view, thr = _patterns()[name]
    other, valid, occ, src, _ = _check_warp(name, d, sign, view, thr, fill=-3.0)
    if name == "ties_left":  # columns 1 and 2 both land on 2: the smaller x wins
        assert src[0, 0, 0].tolist() == [0, -1, 1, -1, 3, -1, 5, -1, 7] and not occ.any()
    elif name == "ties_right":  # -0.5 lands on column 0
        assert src[0, 0, 0].tolist() == [0, -1, 2, -1, 4, -1, 6, -1, 8] and not occ.any()
    elif name.startswith("out_of_frame"):
        assert occ.all() and not valid.any() and (src == -1).all() and (other == -3.0).all()
    elif name == "bar":  # exactly the threshold nearer: hides nothing (12 pixels leave the frame)
        assert occ.sum() == 12
    elif name == "bar_ulp":  # one ulp nearer: the three background pixels it covers
        assert occ.sum() == 12 + 9 and occ[0, 0, :, 17:20].all()
    elif name == "bar_ulp_inf":
        assert occ.sum() == 12


def test_warp_reads_a_channel_slice_where_it_lies_and_does_not_write_its_input():
    g = S.rng(9)
    two = g.uniform(-30.0, 3.0, (2, 2, 37, 70)).astype(np.float32)
    mask = g.random((2, 1, 37, 70)) < 0.85
    dev = _t(two)
    for c in (0, 1):
        view = dev[:, c:c + 1]
        assert not view.is_contiguous() and view.stride(0) == 2 * 37 * 70
        _check_warp(f"channel {c} of (2,2,37,70)", np.ascontiguousarray(two[:, c:c + 1]), "negative", "right", 1.0, mask, dev=view)
        _check_fill(f"channel {c} of (2,2,37,70)", np.ascontiguousarray(two[:, c:c + 1]), mask, True, "min_abs", True, dev=view)
    assert torch.equal(dev, _t(two))


def test_warp_at_the_largest_width():
    from nndepth_amd import geometry
    from nndepth_amd._lib import NndError
    W = geometry.warp_max_width()
    g = S.rng(4)
    d = (g.integers(0, 2 * W, (1, 1, 2, W)) * 0.25).astype(np.float32)  # half of them leave the frame, many ties
    _check_warp("largest width", d, "positive", "left", 1.0)
    _check_warp("largest width", d, "positive", "right", 1.0)
    with pytest.raises(NndError, match="maximum width"):
        geometry.warp_disparity(torch.zeros((1, 1, 1, W + 1), device=DEV))


# ------------------------------------------------------------------------------------------------------------------------ fill
@pytest.mark.parametrize("rule", Wc.RULES)
@pytest.mark.parametrize("shape", _shapes(), ids=str)
def test_fill_random_holes(shape, rule):
    shape = _shape(shape)
    d, mask = Wc.holes(shape, 31 + shape[2] * shape[3])
    key = f"holes {shape}"
    _check_fill(key + " valid mask", d, mask, True, rule, True, fill=-1.0)
    _check_fill(key + " occlusion mask (B,H,W) uint8", d, ~mask, False, rule, True, fill=-1.0, mask_dev=_t((~mask)[:, 0].astype(np.uint8) * 3))
    _check_fill(key + " rows only", d, mask, True, rule, False, fill=-1.0)
    filled, was, mask_out = _check_fill(key + " no mask", d, None, True, rule, True)  # the NaNs alone are holes
    again = _check_fill(key + " again", filled, mask_out, True, rule, True)  # filling a filled map changes nothing
    assert _diff(again[0], filled) == 0 and not again[1].any()


@pytest.mark.parametrize("rule", Wc.RULES)
def test_fill_patterns(rule):
    chunk = _chunks()[1]
    d, mask = Wc.fill_pattern(chunk)
    filled, was, mask_out = _check_fill("pattern", d, mask, True, rule, True, fill=-1.0)
    assert mask_out[0].all() and not mask_out[1].any() and (filled[1] == -1.0).all()  # nothing valid beside a normal sample
    assert (filled[0, 0, 7, 3::8] == 2.5).all()  # |v_L| == |v_R| with opposite signs: the tie goes left
    filled, was, mask_out = _check_fill("pattern", d, ~mask, False, rule, False, fill=4.0)
    assert (filled[0, 0, [0, 5, 6, 10, 11]] == 4.0).all() and mask_out[0, 0, [0, 5, 6, 10, 11]].all() and not mask_out[0, 0, 1].any()
    for W in (chunk - 1, chunk, chunk + 1, 3 * chunk):  # one ok pixel per row, at either end and on the chunk borders
        for x in sorted({0, W - 1, min(chunk - 1, W - 1), min(chunk, W - 1)}):
            d1 = S.rng(W + x).uniform(-5.0, 5.0, (1, 1, 2, W)).astype(np.float32)
            m1 = np.zeros(d1.shape, bool)
            m1[0, 0, 1, x] = True
            filled, _, _ = _check_fill(f"single pixel W {W} x {x}", d1, m1, True, rule, True)
            assert (filled == d1[0, 0, 1, x]).all()


@pytest.mark.parametrize("rule", Wc.RULES)
def test_fill_scene_masked_by_its_warp_occlusion(rule):
    shape = (3, 1, 70, 200)
    d, mask = Wc.scene(shape, 77, "negative")
    occ = Wc.warp(d, "negative", "right", 1.0, mask)[2]
    assert 0.15 < occ.mean() < 0.5
    _check_fill("scene masked by its warp occlusion", d, occ, False, rule, True)


def _raw(d_dev, mask_dev, feats_dev, fillers):
    """Both entry points through ctypes on buffers of our own, every output and the workspace pre-filled by `fillers`."""
    from nndepth_amd._lib import check, lib
    from nndepth_amd.ops import _p, _stream
    B, _, H, W = d_dev.shape
    f_i32, f_u8, f_f32 = fillers
    mk = lambda dtype, f, C=1: f(torch.empty((B, C, H, W), dtype=dtype, device=DEV))  # noqa: E731
    other, valid, occ, src = mk(torch.float32, f_f32), mk(torch.uint8, f_u8), mk(torch.uint8, f_u8), mk(torch.int32, f_i32)
    feats = mk(torch.float32, f_f32, feats_dev.shape[1])
    check(lib.nnd_warp_disparity(_p(d_dev), H * W, _p(mask_dev), 1, 1, 1, 1.0, -2.0, _p(feats_dev), feats_dev.shape[1], _p(other), _p(valid),
                                 _p(occ), _p(src), _p(feats), B, H, W, _stream(d_dev.device)), "warp_disparity")
    n = lib.nnd_fill_holes_workspace_bytes(B, H, W)
    ws = f_i32(torch.empty(n // 4, dtype=torch.int32, device=DEV))
    filled, was, mask_out = mk(torch.float32, f_f32), mk(torch.uint8, f_u8), mk(torch.uint8, f_u8)
    check(lib.nnd_fill_holes(_p(d_dev), H * W, _p(mask_dev), 1, 0, 1, -2.0, _p(filled), _p(was), _p(mask_out), _p(ws), n, B, H, W,
                             _stream(d_dev.device)), "fill_holes")
    return other, valid, occ, src, feats, filled, was, mask_out


def test_same_bytes_on_every_run_and_whatever_the_buffers_held():
    shape = (2, 1, 12, 2 * _chunks()[0] + 3)
    d, mask = Wc.scene(shape, 5, "negative")
    mask[0, 0, [0, 5, 6, 11]] = False
    mask[1] = False
    feats = S.rng(6).random((2, 2, 12, shape[3])).astype(np.float32)
    dd, mm, ff = _t(d), _t(mask.view(np.uint8)), _t(feats)
    zero = lambda t: t.zero_()  # noqa: E731
    ones = lambda t: t.view(torch.uint8).fill_(0xFF).view(t.dtype).view(t.shape) if t.dtype != torch.uint8 else t.fill_(0xFF)  # noqa: E731
    small = lambda t: t.fill_(3)  # noqa: E731  small positive indices: what a stale workspace looks like
    want = Wc.warp(d, "negative", "right", 1.0, mask, feats, -2.0) + Wc.fill_holes(d, mask, True, "min_abs", True, -2.0)
    runs = [_raw(dd, mm, ff, f) for f in ((zero,) * 3, (zero,) * 3, (ones,) * 3, (small,) * 3)]
    torch.cuda.synchronize()
    for i, run in enumerate(runs):
        counts = [_diff(g, w) for g, w in zip(run, want)]
        _lines[f"zz buffers {i}"] = f"warp + fill on pre-filled buffers, run {i}: {counts} differ\n"
        assert counts == [0] * 8
    for other in runs[1:]:  # byte for byte
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(runs[0], other))


# ----------------------------------------------------------------------------------------------------------- the scene methods
def test_scene_methods():
    from nndepth_amd.scene import Depth, Disparity
    shape = (3, 1, 70, 200)
    d, mask = Wc.scene(shape, 77, "negative")
    feats = S.rng(2).random((3, 3, 70, 200)).astype(np.float32)
    dd = _t(d)
    for occ_dev, dtype in ((_t(~mask), torch.bool), (_t((~mask)[:, 0].astype(np.uint8)), torch.uint8), (None, torch.uint8)):
        m = None if occ_dev is None else ~mask
        disp = Disparity(dd, "negative", occlusion=occ_dev, baseline=0.3)
        # to_other_view: an existing occlusion makes its pixels invalid sources; the new occlusion is 1 in the holes
        want = Wc.warp(d, "negative", "right", 0.5, m, feats, 0.0, mask_is_valid=False)
        got, gf = disp.to_other_view("right", 0.5, _t(feats))
        assert isinstance(got, Disparity) and got.disp_sign == "negative" and got.baseline == 0.3 and got.occlusion.dtype == dtype
        assert got.occlusion.shape == shape and _diff(got.data, want[0]) == 0 and _diff(gf, want[4]) == 0
        assert np.array_equal(_np(got.occlusion) != 0, want[3] < 0)
        alone = disp.to_other_view()
        assert isinstance(alone, Disparity) and _diff(alone.data, Wc.warp(d, "negative", "right", 1.0, m, mask_is_valid=False)[0]) == 0
        # warp_occlusion: the old occlusion plus the warp-occluded pixels
        want = Wc.warp(d, "negative", "right", 2.0, m, mask_is_valid=False)[2]
        got = disp.warp_occlusion(2.0)
        assert got.occlusion.dtype == dtype and got.data is dd and got.baseline == 0.3
        assert np.array_equal(_np(got.occlusion) != 0, want != 0)
        if m is not None:
            assert want[m].all() and want.sum() > m.sum()
        # fill_holes
        for name, rule in (("background", "min_abs"), ("foreground", "max_abs"), ("nearest", "nearest")):
            want = Wc.fill_holes(d, m, False, rule, True)
            got = disp.fill_holes(name)
            assert got.occlusion.dtype == dtype and got.disp_sign == "negative" and got.baseline == 0.3
            assert _diff(got.data, want[0]) == 0 and np.array_equal(_np(got.occlusion) != 0, want[2] != 0)
        want = Wc.fill_holes(d, m, False, "min_abs", False)
        assert _diff(disp.fill_holes(vertical=False).data, want[0]) == 0
    # a right-view map (positive sign) into the left view
    got = Disparity(_t(-d), "positive").to_other_view("left")
    assert got.disp_sign == "positive" and _diff(got.data, Wc.warp(-d, "positive", "left")[0]) == 0
    # Depth: the background is the LARGER depth, the smaller value of an inverse depth
    z = np.abs(d) + np.float32(1)
    zz = _t(z)
    for valid_dev, dtype in ((_t(mask), torch.bool), (_t(mask[:, 0].astype(np.uint8)), torch.uint8), (None, torch.uint8)):
        m = None if valid_dev is None else mask
        for inverse in (False, True):
            for name, rule in (("background", "min_abs" if inverse else "max_abs"), ("foreground", "max_abs" if inverse else "min_abs"),
                               ("nearest", "nearest")):
                want = Wc.fill_holes(z, m, True, rule, True)
                got = Depth(zz, valid_mask=valid_dev, is_inverse=inverse).fill_holes(name)
                assert isinstance(got, Depth) and got.is_inverse == inverse and got.valid_mask.dtype == dtype
                assert _diff(got.data, want[0]) == 0 and np.array_equal(_np(got.valid_mask) != 0, want[2] != 0)


def test_the_chain_warp_occlusion_remove_speckles_fill_holes():
    from nndepth_amd.scene import Disparity
    shape = (3, 1, 70, 200)
    d, mask = Wc.scene(shape, 21, "negative")
    got = Disparity(_t(d), "negative", occlusion=_t(~mask)).warp_occlusion(1.0).remove_speckles(8, 0.5, 8).fill_holes()
    occ = Wc.warp(d, "negative", "right", 1.0, ~mask, mask_is_valid=False)[2]
    filt, occ2, speckle, _ = S.speckle_filter(d, 8, 0.5, occ, False, 8)
    assert speckle.mean() > 0.02
    filled, was, occ3 = Wc.fill_holes(filt, occ2, False, "min_abs", True)
    counts = [_diff(got.data, filled), int((_np(got.occlusion) != (occ3 != 0)).sum())]
    _lines["zz chain"] = f"warp_occlusion().remove_speckles(8, 0.5, 8).fill_holes() {shape}: {counts} differ; {int(was.sum())} filled\n"
    assert counts == [0, 0] and got.occlusion.dtype == torch.bool and not occ3.any()


def test_occlusion_from_warp_runs_one_forward_at_batch_b():
    from nndepth_amd import geometry
    from nndepth_amd._lib import NndError
    from nndepth_amd.scene import Disparity
    shape = (2, 1, 33, 130)
    d, _ = Wc.scene(shape, 8, "negative")
    up = _t(np.concatenate([d, np.zeros_like(d)], axis=1))  # a 2-channel map: channel 0 is read where it lies
    left, right = torch.zeros((2, 3, 33, 130), device=DEV), torch.ones((2, 3, 33, 130), device=DEV)
    calls = []

    def forward(a, b):
        calls.append((a, b))
        return [{"up_disp": None}, {"up_disp": up}]

    got = geometry.occlusion_from_warp(forward, left, right, threshold=0.5)
    assert len(calls) == 1 and calls[0][0] is left and calls[0][1] is right and calls[0][0].shape[0] == 2
    assert isinstance(got, Disparity) and got.disp_sign == "negative" and got.data.data_ptr() == up.data_ptr() and got.data.shape == shape
    assert got.occlusion.dtype == torch.uint8 and _diff(got.occlusion, Wc.warp(d, "negative", "right", 0.5)[2]) == 0
    with pytest.raises(NndError, match="for a batch of 2"):
        geometry.occlusion_from_warp(lambda a, b: [{"up_disp": up[:1]}], left, right)


def test_one_graph_capture_replayed_on_new_input():
    from nndepth_amd import geometry
    shape = (3, 1, 70, 200)
    inputs = [Wc.scene(shape, 21, "negative"), Wc.holes(shape, 22)]
    feats = [S.rng(s).random((3, 3, 70, 200)).astype(np.float32) for s in (1, 2)]
    buf_d, buf_m = torch.zeros(shape, dtype=torch.float32, device=DEV), torch.ones(shape, dtype=torch.bool, device=DEV)
    buf_f = torch.zeros((3, 3, 70, 200), dtype=torch.float32, device=DEV)
    ws = torch.empty(geometry.fill_workspace_bytes(3, 70, 200) // 4, dtype=torch.int32, device=DEV)

    def run():
        return (geometry.warp_disparity(buf_d, "negative", "right", 1.0, buf_m, buf_f, -1.0, return_source=True)
                + geometry.fill_holes(buf_d, buf_m, True, "nearest", True, -1.0, workspace=ws))

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
    for (d, mask), f in zip(inputs, feats):
        buf_d.copy_(_t(d))
        buf_m.copy_(_t(mask))
        buf_f.copy_(_t(f))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [o.clone() for o in out]
        direct = run()
        torch.cuda.synchronize()
        want = Wc.warp(d, "negative", "right", 1.0, mask, f, -1.0) + Wc.fill_holes(d, mask, True, "nearest", True, -1.0)
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(replayed, direct))
        assert [_diff(a, w) for a, w in zip(replayed, want)] == [0] * 8


def test_refusals_on_the_device_by_name():
    from nndepth_amd import geometry
    from nndepth_amd._lib import NndError
    d = torch.zeros((2, 1, 5, 7), device=DEV)
    with pytest.raises(NndError, match="workspace of 8 bytes"):
        geometry.fill_holes(d, workspace=torch.empty(1, dtype=torch.int64, device=DEV))
    with pytest.raises(NndError, match="workspace must be a contiguous tensor"):
        geometry.fill_holes(d, workspace=torch.empty(1000, dtype=torch.int64))
    for call in (lambda m: geometry.warp_disparity(d, valid_mask=m), lambda m: geometry.fill_holes(d, m)):
        with pytest.raises(NndError, match=r"the mask is \(2, 5, 6\)"):
            call(torch.ones((2, 5, 6), dtype=torch.bool, device=DEV))
        with pytest.raises(NndError, match="the mask is on cpu"):
            call(torch.ones((2, 5, 7), dtype=torch.bool))
    for f in (torch.zeros((2, 3, 5, 6), device=DEV), torch.zeros((1, 3, 5, 7), device=DEV), torch.zeros((2, 5, 7), device=DEV)):
        with pytest.raises(NndError, match=r"features are \(B,C,H,W\)"):
            geometry.warp_disparity(d, features=f)
    with pytest.raises(NndError, match="features are torch.float32"):
        geometry.warp_disparity(d, features=torch.zeros((2, 3, 5, 7), device=DEV, dtype=torch.float16))
    with pytest.raises(NndError, match="the features are on cpu"):
        geometry.warp_disparity(d, features=torch.zeros((2, 3, 5, 7)))
