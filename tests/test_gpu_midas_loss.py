"""GPU: MiDasLoss / MiDasLossMean on the device (csrc/midas_loss.hip) against the fixture tests/golden/midas_loss.npz: r = the
reference's own fp32 results, f = the contract in float64 (scripts/make_golden_midas_loss.py; the cases' inputs regenerate from
their names, tests/midas_loss_cases.py).

Accuracy bar, per case and value with a finite f:  |d - f| <= max(|r - f|, 2^-24 * max(1, |f|))  — the device result d is at
least as close to float64 as the reference's fp32 result is, down to the resolution of the fp32 value the reference returns."""
import json
import math

import numpy as np
import pytest
import torch

import depth_eval_cases as dc
import midas_loss_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fx(gold):
    g = gold("midas_loss.npz")
    names = json.loads(str(g["names"]))
    assert tuple(names) == mc.NAMES
    return {n: dict(r=g["r"][i], f=g["f"][i], n=int(g["n"][i]), kept=int(g["kept"][i])) for i, n in enumerate(names)}


@pytest.fixture(scope="module")
def inputs():
    """name -> (pred, target, mask) on the device; not modified by any test."""
    return {name: tuple(t.to(DEV) for t in mc.make_case(name)) for name in mc.NAMES}


@pytest.fixture(scope="module")
def device_results(inputs):
    """name -> the six doubles of values_tensor, computed once."""
    from nndepth_amd.prepost import MiDasLoss
    crit = MiDasLoss(*mc.COEFS)
    return {name: crit.values_tensor(*inputs[name]).cpu().numpy() for name in mc.NAMES}


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


@pytest.mark.parametrize("name", mc.NAMES)
def test_at_least_as_close_to_float64_as_the_reference(fx, device_results, name):
    d, r, f = device_results[name], fx[name]["r"], fx[name]["f"]
    for i, k in enumerate(mc.VALUES):
        bound = max(abs(r[i] - f[i]), 2.0 ** -24 * max(1.0, abs(f[i]))) if math.isfinite(f[i]) else None
        print(f"{name} {k}: d = {float(d[i])!r}, f = {float(f[i])!r}, r = {float(r[i])!r}, bound on |d - f| = {bound!r}")
    for i, k in enumerate(mc.VALUES):
        if math.isfinite(f[i]):
            assert abs(d[i] - f[i]) <= max(abs(r[i] - f[i]), 2.0 ** -24 * max(1.0, abs(f[i]))), (name, k, d[i], f[i], r[i])
        assert math.isnan(d[i]) == math.isnan(f[i]), (name, k, d[i])  # NaN exactly where f is NaN
    assert d[4] == fx[name]["n"] and d[5] == fx[name]["kept"], (name, d[4:], fx[name])


def test_dict_has_the_references_keys_and_loss_is_the_first_value(inputs, device_results):
    from nndepth_amd.prepost import MiDasLoss
    loss, res = MiDasLoss(*mc.COEFS)(*inputs["B"])
    assert list(res.keys()) == list(mc.VALUES) and all(type(v) is float for v in res.values())
    assert _same(list(res.values()), device_results["B"][:4])
    assert torch.is_tensor(loss) and loss.dim() == 0 and loss.dtype == torch.float64 and loss.device == torch.device(DEV)
    assert _same(loss.cpu().numpy(), device_results["B"][0])


def test_the_coefficients_weigh_the_two_terms(inputs, device_results):
    from nndepth_amd.prepost import MiDasLoss
    d = MiDasLoss(0.25, 3.0).values_tensor(*inputs["D"]).cpu().numpy()
    assert _same(d[1:], device_results["D"][1:])
    assert d[0] == d[1] * 0.25 + d[2] * 3.0


@pytest.mark.parametrize("name", ["B", "D", "H"])
def test_same_bits_run_to_run(inputs, device_results, name):
    from nndepth_amd.prepost import MiDasLoss
    crit = MiDasLoss(*mc.COEFS)
    for _ in range(2):
        assert _same(crit.values_tensor(*inputs[name]).cpu().numpy(), device_results[name])


@pytest.mark.parametrize("fill", ["nan", "ff"])
def test_result_does_not_depend_on_what_workspace_and_output_held(inputs, device_results, monkeypatch, fill):
    """The cached workspace is replaced by exactly the bytes the library asks for, filled with NaN or with 0xFF bytes (a set mask
    byte, an all-ones key), and the output the wrapper allocates comes filled the same way."""
    from nndepth_amd import prepost
    from nndepth_amd._lib import lib

    def poison(t):
        return t.fill_(float("nan")) if fill == "nan" else t.view(torch.uint8).fill_(0xFF).view(t.dtype)

    real_empty = torch.empty
    filled = []

    def empty(*a, **k):
        t = poison(real_empty(*a, **k))
        filled.append(t.numel())
        return t
    try:
        for name in ("C", "B", "D"):  # C first: its third sample writes no e at all
            B, H, W = next(s for n, s, _ in mc.CASES if n == name)
            nbytes = int(lib.nnd_midas_loss_workspace_bytes(B, H, W))
            ws = prepost._MIDAS_LOSS_WS[DEV] = poison(real_empty(nbytes // 8, dtype=torch.float64, device=DEV))
            monkeypatch.setattr(torch, "empty", empty)
            got = prepost.MiDasLoss(*mc.COEFS).values_tensor(*inputs[name])
            monkeypatch.setattr(torch, "empty", real_empty)
            assert prepost._MIDAS_LOSS_WS[DEV].data_ptr() == ws.data_ptr() and filled == [6], filled
            filled.clear()
            assert _same(got.cpu().numpy(), device_results[name]), (name, got, device_results[name])
    finally:
        monkeypatch.setattr(torch, "empty", real_empty)
        prepost._MIDAS_LOSS_WS.pop(DEV, None)


def test_uint8_mask_equals_bool_mask(inputs, device_results):
    from nndepth_amd.prepost import MiDasLoss
    crit = MiDasLoss(*mc.COEFS)
    for name in ("B", "T"):
        pred, target, mask = inputs[name]
        assert _same(crit.values_tensor(pred, target, mask.to(torch.uint8)).cpu().numpy(), device_results[name])
    pred, target, mask = inputs["Z"]
    assert _same(crit.values_tensor(pred, target, mask.to(torch.uint8) * 255).cpu().numpy(), device_results["Z"])  # any non-zero byte


def test_non_contiguous_prediction(inputs, device_results):
    from nndepth_amd.prepost import MiDasLoss
    pred, target, mask = inputs["C"]
    big = torch.full((3, 2, 33 + 4, 47 + 6), 7.0, device=DEV)
    big[:, 1:2, 3:-1, 2:-4] = pred
    view = big[:, 1:2, 3:-1, 2:-4]
    assert not view.is_contiguous() and view.stride(3) == 1
    assert _same(MiDasLoss(*mc.COEFS).values_tensor(view, target, mask).cpu().numpy(), device_results["C"])
    wide = torch.zeros((3, 1, 33, 2 * 47), device=DEV)
    wide[..., ::2] = pred
    assert wide[..., ::2].stride(3) == 2  # no unit stride along a row: the wrapper makes the copy
    assert _same(MiDasLoss(*mc.COEFS).values_tensor(wide[..., ::2], target, mask).cpu().numpy(), device_results["C"])


def test_inputs_are_left_untouched(inputs):
    """The reference zeroes the invalid pixels of a private copy of the normalised target; ours writes to no input."""
    from nndepth_amd.prepost import MiDasLoss
    before = [t.clone() for t in inputs["B"]]
    MiDasLoss(*mc.COEFS)(*inputs["B"])
    torch.cuda.synchronize()
    for a, b in zip(before, inputs["B"]):
        assert torch.equal(a.view(torch.uint8) if a.dtype == torch.bool else a.view(torch.int32),
                           b.view(torch.uint8) if b.dtype == torch.bool else b.view(torch.int32))


def test_values_tensor_replays_from_a_hip_graph(inputs, device_results):
    """Captured once on fixed buffers (A's shape), replayed after the buffers took case Z's maps and mask, then case A's: the replay
    equals the direct call bit for bit."""
    from nndepth_amd.prepost import MiDasLoss
    crit = MiDasLoss(*mc.COEFS)
    pa, ta, ma = inputs["A"]
    bufs = [torch.zeros_like(pa), torch.ones_like(ta), torch.ones_like(ma)]
    for _ in range(2):
        crit.values_tensor(*bufs)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = crit.values_tensor(*bufs)
    torch.cuda.current_stream(DEV).wait_stream(side)
    for name in ("Z", "A"):
        for b, t in zip(bufs, inputs[name]):
            b.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(out.cpu().numpy(), device_results[name]), name
        assert _same(out.cpu().numpy(), crit.values_tensor(*inputs[name]).cpu().numpy())


def test_validation_mean_is_the_plain_mean_and_nan_propagates(inputs):
    """trainer.py:341-350 over the batches A, C, D: np.mean of the per-batch dicts, bit for bit; with E in the list every mean is NaN."""
    from nndepth_amd.prepost import MiDasLoss, MiDasLossMean
    crit, mean = MiDasLoss(*mc.COEFS), MiDasLossMean(*mc.COEFS)
    dicts = []
    for name in ("A", "C", "D"):
        mean.update(*inputs[name])
        dicts.append(crit(*inputs[name])[1])
    want = {f"val/{k}": float(np.mean([m[k] for m in dicts])) for k in mc.VALUES}
    got = mean.result()
    assert list(got.keys()) == list(want.keys()) and all(type(v) is float for v in got.values())
    assert _same(list(got.values()), list(want.values())), (got, want)
    mean.update(*inputs["E"])
    got = mean.result()
    assert list(got.keys()) == list(want.keys()) and all(math.isnan(v) for v in got.values()), got


def test_depth_eval_is_unchanged_by_the_shared_select(gold):
    """DepthEvalCriterion's median now runs on the select of csrc/eval_chain.h: cases B (a sample without a pixel), G (negative
    scale: the rank counted from the other end) and F (ties, even counts) still meet tests/golden/depth_eval.npz under that file's bar."""
    from nndepth_amd.prepost import DepthEvalCriterion
    g = gold("depth_eval.npz")
    names = json.loads(str(g["names"]))
    crit = DepthEvalCriterion(max_depth=dc.MAX_DEPTH)
    for name in ("B", "G", "F"):
        i = names.index(name)
        pred, gt, mask = dc.make_case(name)
        d = crit.metrics_tensor(pred.to(DEV), gt.to(DEV), None if mask is None else mask.to(DEV)).cpu().numpy()
        r, f = g["r"][i], g["f"][i]
        for j, k in enumerate(dc.METRICS):
            if math.isfinite(f[j]):
                assert abs(d[j] - f[j]) <= max(abs(r[j] - f[j]), 2.0 ** -24 * max(1.0, abs(f[j]))), (name, k, d[j], f[j], r[j])
            assert math.isnan(d[j]) == math.isnan(f[j]), (name, k, d[j])
        assert _same(d[4:7], f[4:7]) and d[9] == int(g["count"][i]), name


def test_bad_inputs_are_refused_by_name(inputs):
    from nndepth_amd._lib import NndError
    from nndepth_amd.prepost import MiDasLoss
    crit = MiDasLoss()
    pred, target, mask = inputs["B"]
    with pytest.raises(NndError, match="fp32"):
        crit(pred.double(), target, mask)
    with pytest.raises(NndError, match="fp32"):
        crit(pred, target.half(), mask)
    with pytest.raises(NndError, match="valid_mask is torch.bool"):
        crit(pred, target, mask.float())
    with pytest.raises(NndError, match="valid_mask is required"):
        crit(pred, target, None)
    with pytest.raises(NndError, match=r"\(B,1,H,W\)"):
        crit(pred.expand(-1, 2, -1, -1), target.expand(-1, 2, -1, -1), mask.expand(-1, 2, -1, -1))
    with pytest.raises(NndError, match=r"\(B,1,H,W\)"):
        crit(pred[:, 0], target[:, 0], mask[:, 0])
    with pytest.raises(NndError, match="one shape"):
        crit(pred, target[:, :, :-1], mask)
    with pytest.raises(NndError, match="one shape"):
        crit(pred, target, mask[:1])
    with pytest.raises(NndError, match="HIP device"):
        crit(pred.cpu(), target, mask)
    with pytest.raises(NndError, match="HIP device"):
        crit(pred, target.cpu(), mask)
    with pytest.raises(NndError, match="no CPU fallback"):
        crit(pred, target, mask.cpu())
    with pytest.raises(NndError, match="at least 16"):
        crit(pred[:, :, :15], target[:, :, :15], mask[:, :, :15])
    with pytest.raises(NndError, match="at least 16"):
        crit(pred[..., :15], target[..., :15], mask[..., :15])
    with pytest.raises(NndError, match="no backward"):
        crit(pred.clone().requires_grad_(True), target, mask)
    with torch.no_grad():  # the validation loop's way: a value
        loss, _ = crit(pred.clone().requires_grad_(True), target, mask)
    assert not loss.requires_grad
