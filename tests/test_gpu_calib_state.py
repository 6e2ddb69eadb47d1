"""GPU: fp16x2 activation ranges as data, on top of the contract of tests/test_gpu_calib.py (records accumulate and do not stick,
overflow is visible as non-finite output, a calibrated model does not silently recalibrate).
  a. nnd_scales_write / nnd_scales_read on one layer against integers computed here; nnd_nonfinite_flag
  b. a state taken from one model and loaded into another: bit-identical outputs, no calibration asked for, also after a repack
  c. calibrate(widen=True) is the exact per-layer minimum
  d. overflow is reported (watch_range, range_report) and repaired by widening
  e. a loaded state reaches a captured graph in place
  f. a Conv3d layer is one entry: the state reaches the formulation another depth picks
The models, inputs and bars are those of tests/test_gpu_calib.py.  NaN and inf are data values here; no test provokes a fault."""
import json
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_calib as TC  # noqa: E402  (its small models and its _EngineWatch; nothing of it is collected from here)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPORT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "REPORT_calib_state.txt")


# ------------------------------------------------------------------------------------------------- a. the C-ABI on one layer
def test_scales_write_set_and_widen_on_one_layer():
    """mode 0 sets xs, mode 1 keeps the smaller one, both clamp to |xs| <= 60; XSCALE == 2^xs and OSCALE == WSINV * 2^-xs exactly
    (powers of two); the record and every other float of the blob keep their bits."""
    from nndepth_amd import ops
    conv = TC._layer()
    conv.packed = conv.packed.to(DEV)
    (name, off), = conv._slots()
    assert name == "" and off == conv.packed.numel() - 4
    assert conv.read_scales().tolist() == [2] and not conv.calibrated
    x = torch.randn(2, 32, 5, 9, generator=torch.Generator().manual_seed(1))
    conv.calibrate(x.to(DEV))
    m = x.abs().max().item()
    assert conv.read_scales().tolist() == [11 - (math.frexp(m)[1])]  # calib.hip: xs = 11 - e, max = f * 2^e with f in [0.5, 1)
    conv.packed[off + 2] = 1.5  # a pending record, as a calibrating forward leaves one
    before = conv.packed.clone()
    wsinv = float(before[off + 3])
    ptr = conv.packed.data_ptr()

    def check(xs):
        tail = conv.packed[off:off + 4].cpu()
        assert conv.read_scales().tolist() == [xs]
        assert float(tail[1]) == 2.0 ** xs and float(tail[0]) == wsinv * 2.0 ** -xs, (xs, tail)
        assert float(tail[2]) == 1.5 and float(tail[3]) == wsinv
        rest = torch.ones_like(before, dtype=torch.bool)
        rest[off:off + 2] = False
        assert torch.equal(conv.packed.view(torch.int32)[rest], before.view(torch.int32)[rest]) and conv.packed.data_ptr() == ptr
        assert conv.activation_range() == 65504.0 / 2.0 ** xs

    cur = None
    for xs, widen in [(7, False), (9, True), (7, True), (3, True), (5, True), (-12, False), (0, True), (-13, True), (60, False),
                      (61, False), (1000, False), (-60, False), (-61, True), (-2 ** 31, False), (4, False)]:
        conv.write_scales([xs], widen=widen)
        cur = max(-60, min(60, min(cur, xs) if widen else xs))
        check(cur)
    assert conv.calibrated
    conv.write_scales(torch.tensor([6], dtype=torch.int64, device=DEV))  # a device tensor of another integer type is taken as well
    check(6)
    with pytest.raises(ops.NndError, match="2 exponents for 1 layers"):
        conv.write_scales([1, 2])
    # the record: read, read and cleared, gone
    assert conv.read_records(clear=False).tolist() == [1.5] and conv.read_records(clear=True).tolist() == [1.5]
    assert conv.read_records().tolist() == [0.0] and conv.read_scales().tolist() == [6]
    # and the layer computes with what was written: at xs = 6 values up to 65504 / 64 are finite, beyond they are not
    y = conv(torch.full((1, 32, 5, 9), 1000.0, device=DEV))
    assert torch.isfinite(y).all() and not torch.isfinite(conv(torch.full((1, 32, 5, 9), 1100.0, device=DEV))).all()


@pytest.mark.parametrize("n", [1, 63, 257, 2048 * 256 + 3])
def test_nonfinite_flag(n):
    """Every position class of the grid-stride loop: first, last, one past a full pass; inf of either sign and NaN; OR, never clear."""
    from nndepth_amd import ops
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    x = torch.randn(n, device=DEV) * 1e30
    x[n // 2] = 3.4028234e38  # the largest finite float is finite
    ops.nonfinite_flag(x, word)
    assert word.item() == 0
    for pos, bad in [(0, float("inf")), (n - 1, float("nan")), (n // 2, float("-inf")), (min(n - 1, 2048 * 256), float("nan"))]:
        w = torch.zeros(1, dtype=torch.int32, device=DEV)
        y = x.clone()
        y[pos] = bad
        ops.nonfinite_flag(y, w)
        assert w.item() == 1, (n, pos, bad)
        ops.nonfinite_flag(x, w)  # a finite tensor afterwards does not clear it
        assert w.item() == 1
    word.fill_(6)
    ops.nonfinite_flag(x[:1] * float("inf"), word)
    assert word.item() == 7  # ORed into the word


# ------------------------------------------------------------------------------------------------- b. round trip
def _outs(model, f1, f2):
    return [o["up_disp"].clone() for o in model(f1, f2)]


class _SharedEncoderSide:
    """The Coarse2Fine double's encoder side is a PyTorch-ROCm conv pyramid (tests/c2f_double.py; not this project's code), and
    those convs are not bit-reproducible from call to call: two forwards of ONE model on ONE pair differ by 4e-9 .. 6e-8 in the
    feature maps and up to 3e-6 in the outputs (measured on the MI355X while the packed blobs of the two models were bit-identical).
    A bit-for-bit comparison of two models therefore feeds both the features computed ONCE per pair: everything behind them — the
    three-stage HIP cascade, which is what holds the activation ranges — stays compared bit for bit."""

    def __init__(self, model):
        self.compute, self.seen = model.forward_features, {}

    def __call__(self, f1, f2):
        key = (f1.data_ptr(), f2.data_ptr())
        if key not in self.seen:
            self.seen[key] = self.compute(f1, f2)
        return self.seen[key]


@pytest.mark.parametrize("model", list(TC.MODELS))
def test_state_round_trip_gives_bit_identical_outputs(gold, monkeypatch, model):
    from nndepth_amd import weightgen
    a, (f1, f2), refs, bar, _ = TC.MODELS[model](gold)
    B, H, W = f1.shape[0], f1.shape[-2], f1.shape[-1]
    P = (f1.to(DEV), f2.to(DEV))
    Q = tuple(x.to(DEV) for x in weightgen.synthetic_frames(41, B, H, W))  # held out
    a.calibrate(*P)
    state = json.loads(json.dumps(a.calibration_state()))
    assert state["arithmetic"] == "fp16x2" and len(state["layers"]) >= 11 and all(isinstance(v, int) for v in state["layers"].values())
    assert any(v != 2 for v in state["layers"].values())
    b = TC.MODELS[model](gold)[0]  # a fresh model with the same weights
    if model == "c2f":
        a.forward_features = b.forward_features = _SharedEncoderSide(a)
    want_p, want_q = _outs(a, *P), _outs(a, *Q)
    assert len(want_p) == len(refs)
    watch = TC._EngineWatch(monkeypatch)
    b.load_calibration_state(state)  # nothing is packed yet: pending
    for got, want in ((_outs(b, *P), want_p), (_outs(b, *Q), want_q)):
        assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))
    assert watch.calls == 0, "a model with a loaded state must not ask for calibration"
    assert b.calibration_state() == state
    b.clear_calibration_state()
    assert b.calibration_state() == state  # read back from the engines: what was loaded is what they hold
    b.load_calibration_state(state)
    # a repack: an in-place edit that keeps the values (every parameter, so every engine of the model packs again)
    blob = b.update_block.engine.packed
    with torch.no_grad():
        for p in b.parameters():
            p.mul_(1.0)
    got = _outs(b, *Q)
    assert b.update_block.engine.packed is not blob, "the edit did not repack"
    assert all(torch.equal(g, w) for g, w in zip(got, want_q)) and all(torch.equal(g, w) for g, w in zip(_outs(b, *P), want_p))
    assert watch.calls == 0
    # unpinned, the next repack is a fresh blob and the model calibrates on its own input again (today's behaviour)
    b.clear_calibration_state()
    with torch.no_grad():
        next(b.update_block.parameters()).mul_(1.0)
    b(*P)
    assert watch.calls > 0


# ------------------------------------------------------------------------------------------------- c. widening
def _pairs():
    from nndepth_amd import weightgen
    A = tuple((x / 16.0).to(DEV) for x in weightgen.synthetic_frames(45, 1, 96, 160))
    B = tuple(x.to(DEV) for x in weightgen.synthetic_frames(0, 1, 96, 160))
    return A, B


def test_widening_is_the_exact_minimum_and_meets_the_bar_on_the_small_pair():
    """calibrate(A); calibrate(B, widen=True) == per-layer min(calibrate(A), calibrate(B)) == the other order.  The widened model
    on A (1/16 contrast) against the oracle at the bar of test_raft_calibrated_then_a_sixteenth_of_the_contrast, whose situation
    this is: every layer holds B's scale (that test's) or A's own."""
    from nndepth_amd import weightgen
    from oracle import torch_ref as R
    A, B = _pairs()
    xa = TC._raft().calibrate(*A).calibration_state()["layers"]
    xb = TC._raft().calibrate(*B).calibration_state()["layers"]
    want = {k: min(xa[k], xb[k]) for k in xa}
    assert list(xa) == list(xb) and want != xa, "the case does not tell: widening B's ranges by A's would be replacing them"
    ab = TC._raft().calibrate(*A).calibrate(*B, widen=True)
    ba = TC._raft().calibrate(*B).calibrate(*A, widen=True)
    for k in want:
        print(f"{k:44s} A {xa[k]:4d}  B {xb[k]:4d}  A then B {ab.calibration_state()['layers'][k]:4d}")
    assert ab.calibration_state()["layers"] == want
    assert ba.calibration_state()["layers"] == want
    # widen=False (default) replaces: B's ranges alone
    assert TC._raft().calibrate(*A).calibrate(*B).calibration_state()["layers"] == xb
    sd = weightgen.fill_state_dict(R.raft_stereo_spec())
    ref = R.raft_stereo_forward(sd, A[0].cpu(), A[1].cpu(), 6)
    errs = [(o["up_disp"].cpu() - r).abs().max().item() for o, r in zip(ab(*A), ref)]
    print("widened (A then B) on A vs oracle:", " ".join(f"{e:.2e}" for e in errs))
    assert len(errs) == 6 and max(errs) <= 1e-4


# ------------------------------------------------------------------------------------------------- d. overflow
def test_overflow_is_reported_and_repaired(gold):
    m, (f1, f2), refs, bar, _ = TC._model_raft(gold)
    f1, f2 = f1.to(DEV), f2.to(DEV)
    big = (f1 * 4096.0, f2 * 4096.0)
    m.calibrate(f1, f2)
    blobs = [s.engine().packed.clone() for s in m._calibration_sites().values()]
    # the precondition (tests/test_gpu_calib.py::test_model_overflow_is_visible): this input is beyond the calibrated range
    assert torch.isfinite(m(f1, f2)[-1]["up_disp"]).all() and not torch.isfinite(m(*big)[-1]["up_disp"]).all()
    assert m.range_status() == {"overflow": False, "forwards": 0}  # not watched so far
    m.watch_range = True
    m(f1, f2)
    assert m.range_status() == {"overflow": False, "forwards": 1}
    m(*big)
    assert m.range_status() == {"overflow": True, "forwards": 2}
    m(f1, f2)  # sticky until reset
    assert m.range_status() == {"overflow": True, "forwards": 3}
    m.reset_range_status()
    assert m.range_status() == {"overflow": False, "forwards": 0}
    m(f1, f2)
    assert m.range_status() == {"overflow": False, "forwards": 1}
    # which layer: the report changes no scale and leaves no record behind
    rep = m.range_report(*big)
    assert set(rep) == set(m.calibration_state()["layers"])
    over = [k for k, v in rep.items() if not v["seen"] <= v["limit"]]
    print("exceeded on the pair x 4096:", ", ".join(over))
    assert any(k.startswith("fnet/") and rep[k]["seen"] > rep[k]["limit"] for k in over)
    first = rep["fnet/layer1.0.conv1"]  # the first scaled layer stages the exact stem's output: finite, and beyond what it was calibrated for
    assert first["limit"] < first["seen"] < float("inf")
    small = m.range_report(f1, f2)
    assert all(v["seen"] <= v["limit"] / 16.0 for k, v in small.items() if v["seen"] > 0), "calibrated: a factor 32 of headroom, 16 at least"
    assert small["fnet/layer1.0.conv1"]["seen"] < first["seen"]
    assert all(torch.equal(s.engine().packed.view(torch.int32), b.view(torch.int32)) for s, b in zip(m._calibration_sites().values(), blobs))
    # repaired
    before = m.calibration_state()["layers"]
    m.calibrate(*big, widen=True, max_passes=8)  # (a pass per layer of products: the correlation squares the factor)
    after = m.calibration_state()["layers"]
    # ranges only grow; the first layer's by the 12 octaves of the input, give or take one (the stem's folded shift does not scale)
    assert all(after[k] <= before[k] for k in before) and 11 <= before["fnet/layer1.0.conv1"] - after["fnet/layer1.0.conv1"] <= 13
    m.reset_range_status()
    outs, outs_big = m(f1, f2), m(*big)
    assert all(torch.isfinite(o["up_disp"]).all() for o in outs) and all(torch.isfinite(o["up_disp"]).all() for o in outs_big)
    assert m.range_status() == {"overflow": False, "forwards": 2}
    errs = [(o["up_disp"].cpu() - torch.from_numpy(r)).abs().max().item() for o, r in zip(outs, refs)]
    lines = ["RAFT-Stereo small (96x160, 6 iterations), fp16x2, calibrated on its golden pair, then widened by calibrate(pair * 4096, widen=True):\n",
             "max-abs error of the ORIGINAL pair against the golden, per output (not gated; the bar of a model calibrated on its own\n",
             f"input is {bar:g}): " + " ".join(f"{e:.2e}" for e in errs) + "\n",
             "exponents lowered by: " + " ".join(str(before[k] - after[k]) for k in before) + "\n"]
    print("".join(lines))
    try:
        with open(REPORT, "w") as f:
            f.write("Cost of widening fp16x2 activation ranges (tests/test_gpu_calib_state.py::test_overflow_is_reported_and_repaired).\n" + "".join(lines))
    except OSError:
        pass  # a read-only checkout: the figures were printed


# ------------------------------------------------------------------------------------------------- e. under a graph
def test_loaded_state_reaches_a_captured_graph_in_place(gold):
    from nndepth_amd.graph import GraphedForward
    m, (f1, f2), _, _, _ = TC._model_raft(gold)
    f1, f2 = f1.to(DEV), f2.to(DEV)
    m.calibrate(f1, f2)
    fwd = GraphedForward(m)
    first = [o["up_disp"].clone() for o in fwd(f1, f2)]
    assert all(torch.equal(a, b["up_disp"]) for a, b in zip(first, m(f1, f2)))
    engines = [s.engine() for s in m._calibration_sites().values()]
    ptrs = [e.packed.data_ptr() for e in engines]
    graph = fwd._graphs[next(iter(fwd._graphs))][0]
    state = m.calibration_state()
    wide = {**state, "layers": {k: v - 2 for k, v in state["layers"].items()}}
    m.load_calibration_state(wide)
    replay = [o["up_disp"].clone() for o in fwd(f1, f2)]
    assert len(fwd._graphs) == 1 and fwd._graphs[next(iter(fwd._graphs))][0] is graph, "recaptured"
    assert [e.packed.data_ptr() for e in engines] == ptrs, "a blob was reallocated"
    for e, site in zip(engines, m._calibration_sites()):
        assert e.read_scales().tolist() == [wide["layers"][k] for k in wide["layers"] if k.startswith(site + "/")]
    direct = m(f1, f2)
    assert len(replay) == len(direct) == 6 and all(torch.equal(a, b["up_disp"]) for a, b in zip(replay, direct))
    # 16376 x the old limit would be needed to tell the two states apart by overflow; the scales themselves tell: the replay ran
    # a forward whose first scaled layer accepts 4 x more
    rep = m.range_report(f1, f2)
    assert rep["fnet/layer1.0.conv1"]["limit"] == 65504.0 / 2.0 ** wide["layers"]["fnet/layer1.0.conv1"]


# ------------------------------------------------------------------------------------------------- f. Conv3d: one entry
def test_conv3d_state_reaches_the_formulation_another_depth_picks():
    """16 <- 48 channels, stride 1: the J = 2 grouped layer where the depth is even, the plain one where it is odd (conv3d.hip).  A range
    taken at depth 6 is loaded and run at depth 7: the plain formulation holds it, and computes what a layer calibrated at depth 7 on
    the same maximum computes, bit for bit."""
    from nndepth_amd import ops
    g = torch.Generator().manual_seed(9)
    Cout, Cin = 16, 48
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) * (2.0 / (Cin * 27)) ** 0.5
    bn = (torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1, torch.randn(Cout, generator=g) * 0.1, torch.rand(Cout, generator=g) + 0.5)
    x6 = 37.0 * torch.randn(1, Cin, 6, 9, 14, generator=g)
    x7 = torch.cat([x6, 0.5 * x6[:, :, :1]], dim=2)  # one more slice, the same maximum
    base = ops.Conv3dNorm(w, None, 1, bn, 1e-5, 0.01, 0, DEV, arithmetic="fp16x2")
    assert [n for n, _ in base.formulations()] == ["plain", "grouped"] and base.scale_names() == [""]

    def layer():
        import copy
        e = copy.copy(base)
        e.packed = base.packed.clone()
        return e

    def run(conv, x):
        return conv(ops.volume_to_depth_major(x.to(DEV)))

    xs = 11 - math.frexp(x6.abs().max().item())[1]
    a = layer()
    with ops.calibration():
        run(a, x6)
    assert a.read_scales(per_formulation=True).tolist() == [2, xs]  # the grouped formulation ran; the plain one is at its default
    assert a.read_scales().tolist() == [xs]  # ... and the layer's range is the one that ran
    b = layer()
    b.write_scales(a.read_scales())
    assert b.read_scales(per_formulation=True).tolist() == [xs, xs] and b.calibrated
    c = layer()
    with ops.calibration():
        run(c, x7)
    assert c.read_scales(per_formulation=True).tolist() == [xs, 2] and c.read_scales().tolist() == [xs]
    y = run(b, x7)
    assert torch.isfinite(y).all() and torch.equal(y, run(c, x7))
    assert torch.equal(run(b, x6), run(a, x6))
    # widening a Conv3d layer: every formulation ends at the minimum, whichever ran
    with ops.calibration():
        run(a, x7 * 8.0)  # depth 7: the plain formulation records, 3 octaves up
    a.widen_scales(torch.tensor([xs], dtype=torch.int32, device=DEV))
    assert a.read_scales(per_formulation=True).tolist() == [xs - 3, xs - 3]
