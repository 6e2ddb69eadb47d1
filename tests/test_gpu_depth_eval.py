"""GPU: DepthEvalCriterion / DepthEvalMean on the device (csrc/depth_eval.hip) against the fixture tests/golden/depth_eval.npz:
r = the reference's own fp32 results, f = the contract in float64 (scripts/make_golden_depth_eval.py; the cases' inputs
regenerate from their names, tests/depth_eval_cases.py).

Accuracy bar, per case and metric with a finite f:  |d - f| <= max(|r - f|, 2^-24 * max(1, |f|))  — the device result d is at
least as close to float64 as the reference's fp32 result is, down to the resolution of the fp32 value the reference returns."""
import json
import math

import numpy as np
import pytest
import torch

import depth_eval_cases as dc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fx(gold):
    g = gold("depth_eval.npz")
    names = json.loads(str(g["names"]))
    assert tuple(names) == dc.NAMES
    return {n: dict(r=g["r"][i], f=g["f"][i], count=int(g["count"][i])) for i, n in enumerate(names)}


@pytest.fixture(scope="module")
def inputs():
    """name -> (pred, gt, mask or None) on the device; not modified by any test."""
    out = {}
    for name in dc.NAMES:
        pred, gt, mask = dc.make_case(name)
        out[name] = (pred.to(DEV), gt.to(DEV), None if mask is None else mask.to(DEV))
    return out


@pytest.fixture(scope="module")
def device_results(inputs):
    """name -> the ten doubles of metrics_tensor, computed once."""
    from nndepth_amd.prepost import DepthEvalCriterion
    crit = DepthEvalCriterion(max_depth=dc.MAX_DEPTH)
    return {name: crit.metrics_tensor(*inputs[name]).cpu().numpy() for name in dc.NAMES}


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


@pytest.mark.parametrize("name", dc.NAMES)
def test_at_least_as_close_to_float64_as_the_reference(fx, device_results, name):
    d, r, f = device_results[name], fx[name]["r"], fx[name]["f"]
    for i, k in enumerate(dc.METRICS):
        bound = max(abs(r[i] - f[i]), 2.0 ** -24 * max(1.0, abs(f[i]))) if math.isfinite(f[i]) else None
        print(f"{name} {k}: d = {float(d[i])!r}, f = {float(f[i])!r}, r = {float(r[i])!r}, bound on |d - f| = {bound!r}")
    for i, k in enumerate(dc.METRICS):
        if math.isfinite(f[i]):
            assert abs(d[i] - f[i]) <= max(abs(r[i] - f[i]), 2.0 ** -24 * max(1.0, abs(f[i]))), (name, k, d[i], f[i], r[i])
        elif math.isnan(f[i]):
            assert math.isnan(d[i]), (name, k, d[i])
        else:
            assert d[i] == f[i], (name, k, d[i])
        assert math.isnan(d[i]) == math.isnan(f[i]), (name, k, d[i])  # NaN exactly where f is NaN
    assert d[9] == fx[name]["count"]


@pytest.mark.parametrize("name", dc.NAMES)
def test_delta_metrics_are_the_exact_counts(fx, device_results, name):
    assert _same(device_results[name][4:7], fx[name]["f"][4:7]), (device_results[name][4:7], fx[name]["f"][4:7])


def test_no_valid_pixel_gives_the_empty_metrics(inputs, device_results):
    from nndepth_amd.prepost import DepthEvalCriterion
    assert _same(device_results["E"][:9], dc.empty_metrics()) and device_results["E"][9] == 0
    res = DepthEvalCriterion(max_depth=dc.MAX_DEPTH)(*inputs["E"])
    assert list(res.keys()) == list(dc.METRICS) and list(res.values()) == dc.empty_metrics().tolist()


def test_dict_has_the_references_keys_and_the_tensors_values(inputs, device_results):
    from nndepth_amd.prepost import DepthEvalCriterion
    res = DepthEvalCriterion(max_depth=dc.MAX_DEPTH)(*inputs["B"])
    assert list(res.keys()) == list(dc.METRICS) and all(type(v) is float for v in res.values())
    assert _same(list(res.values()), device_results["B"][:9])


@pytest.mark.parametrize("name", ["B", "G", "H"])
def test_same_bits_run_to_run(inputs, device_results, name):
    from nndepth_amd.prepost import DepthEvalCriterion
    crit = DepthEvalCriterion(max_depth=dc.MAX_DEPTH)
    for _ in range(2):
        assert _same(crit.metrics_tensor(*inputs[name]).cpu().numpy(), device_results[name])


def test_metrics_tensor_replays_from_a_hip_graph(inputs, device_results):
    """Captured once on fixed buffers (D's shape), replayed after the buffers took case G's maps and mask, then D's maps under the
    same mask: the replay equals the direct call bit for bit."""
    from nndepth_amd.prepost import DepthEvalCriterion
    crit = DepthEvalCriterion(max_depth=dc.MAX_DEPTH)
    pg, gg, mg = inputs["G"]
    pd, gd, _ = inputs["D"]
    bufs = [torch.zeros_like(pg), torch.ones_like(gg), torch.ones_like(mg)]
    for _ in range(2):
        crit.metrics_tensor(*bufs)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = crit.metrics_tensor(*bufs)
    torch.cuda.current_stream(DEV).wait_stream(side)
    for new in ((pg, gg, mg), (pd, gd, mg)):
        for b, t in zip(bufs, new):
            b.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(out.cpu().numpy(), crit.metrics_tensor(*new).cpu().numpy())
    assert _same(crit.metrics_tensor(pg, gg, mg).cpu().numpy(), device_results["G"])


def test_dataset_mean_follows_the_references_rule(inputs):
    """evaluate.py:300-312 over the batches A, D, E: D's NaN is left out of rmse_log alone, E's infinities everywhere."""
    from nndepth_amd.prepost import DepthEvalCriterion, DepthEvalMean
    crit, mean = DepthEvalCriterion(max_depth=dc.MAX_DEPTH), DepthEvalMean(max_depth=dc.MAX_DEPTH)
    dicts = []
    for name in ("A", "D", "E"):
        mean.update(*inputs[name])
        dicts.append(crit(*inputs[name]))
    want = {}
    for k in dc.METRICS:
        vals = [m[k] for m in dicts if not (np.isnan(m[k]) or np.isinf(m[k]))]
        want[k] = np.mean(vals) if len(vals) > 0 else (float("inf") if k not in ["delta1", "delta2", "delta3"] else 0.0)
    got = mean.result()
    assert list(got.keys()) == list(dc.METRICS)
    assert _same(list(got.values()), list(want.values())), (got, want)
    assert got["rmse_log"] == dicts[0]["rmse_log"] and got["rmse"] == (dicts[0]["rmse"] + dicts[1]["rmse"]) / 2
    only_e = DepthEvalMean(max_depth=dc.MAX_DEPTH)
    only_e.update(*inputs["E"])
    assert list(only_e.result().values()) == dc.empty_metrics().tolist()


def test_uint8_mask_equals_bool_mask(inputs, device_results):
    from nndepth_amd.prepost import DepthEvalCriterion
    crit = DepthEvalCriterion(max_depth=dc.MAX_DEPTH)
    for name in ("B", "F"):
        pred, gt, mask = inputs[name]
        assert _same(crit.metrics_tensor(pred, gt, mask.to(torch.uint8)).cpu().numpy(), device_results[name])
    pred, gt, _ = inputs["A"]
    assert _same(crit.metrics_tensor(pred, gt, torch.ones_like(gt, dtype=torch.bool)).cpu().numpy(), device_results["A"])


def test_bad_inputs_are_refused_by_name(inputs):
    from nndepth_amd._lib import NndError
    from nndepth_amd.prepost import DepthEvalCriterion
    crit = DepthEvalCriterion()
    pred, gt, mask = inputs["B"]
    with pytest.raises(NndError, match="valid_mask"):
        crit(pred, gt, mask.float())
    with pytest.raises(NndError, match=r"\(B,1,H,W\)"):
        crit(pred.expand(-1, 2, -1, -1), gt.expand(-1, 2, -1, -1))
    with pytest.raises(NndError, match="one shape"):
        crit(pred, gt[:, :, :-1])
    with pytest.raises(NndError, match="one shape"):
        crit(pred, gt, mask[:2])
    with pytest.raises(NndError, match="HIP device"):
        crit(pred.cpu(), gt)
    with pytest.raises(NndError, match="no CPU fallback"):
        crit(pred, gt, mask.cpu())


def test_non_contiguous_prediction(inputs, device_results):
    from nndepth_amd.prepost import DepthEvalCriterion
    pred, gt, mask = inputs["B"]
    big = torch.full((3, 2, 33 + 4, 47 + 6), 7.0, device=DEV)
    big[:, 1:2, 3:-1, 2:-4] = pred
    view = big[:, 1:2, 3:-1, 2:-4]
    assert not view.is_contiguous()
    assert _same(DepthEvalCriterion(max_depth=dc.MAX_DEPTH).metrics_tensor(view, gt, mask).cpu().numpy(), device_results["B"])
