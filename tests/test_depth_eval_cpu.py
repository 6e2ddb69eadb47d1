"""CPU: the fixture of the monocular evaluation criterion (tests/golden/depth_eval.npz, scripts/make_golden_depth_eval.py) is
consistent — the cases regenerate from their names, the tests' float64 statement of the contract (depth_eval_cases.contract64,
torch) reproduces the script's (numpy), the reference's fp32 results lie within the script's cap — and the entry points'
host-side checks answer with a status and a message, without a device."""
import ctypes as C
import json
import math

import numpy as np
import pytest

import depth_eval_cases as dc

CAP = 1e-5  # scripts/make_golden_depth_eval.py refuses a case above it


@pytest.fixture(scope="module")
def fx(gold):
    g = gold("depth_eval.npz")
    names = json.loads(str(g["names"]))
    assert tuple(names) == dc.NAMES
    assert [tuple(s) for s in g["shapes"].tolist()] == [c[1] for c in dc.CASES]
    return {n: dict(r=g["r"][i], f=g["f"][i], count=int(g["count"][i])) for i, n in enumerate(names)}


@pytest.fixture(scope="module")
def restated():
    out = {}
    for name in dc.NAMES:
        pred, gt, mask = dc.make_case(name)
        out[name] = dc.contract64(pred, gt, mask)
    return out


@pytest.mark.parametrize("name", dc.NAMES)
def test_float64_restatement_reproduces_the_fixture(fx, restated, name):
    f, n = restated[name]
    want = fx[name]["f"]
    assert n == fx[name]["count"]
    for k, a, b in zip(dc.METRICS, f, want):
        if math.isfinite(b):
            assert abs(a - b) <= 1e-12 * max(1.0, abs(b)), (name, k, a, b)
        else:
            assert (math.isnan(a) and math.isnan(b)) or a == b, (name, k, a, b)


@pytest.mark.parametrize("name", dc.NAMES)
def test_reference_results_lie_within_the_cap(fx, name):
    r, f = fx[name]["r"], fx[name]["f"]
    for k, a, b in zip(dc.METRICS, r, f):
        if math.isfinite(b):
            assert math.isfinite(a) and abs(a - b) <= CAP * max(1.0, abs(b)), (name, k, a, b)
            assert a == float(np.float32(a))  # an fp32 result, held exactly
        else:
            assert (math.isnan(a) and math.isnan(b)) or a == b, (name, k, a, b)


def test_cases_cover_what_they_are_there_for(fx, restated):
    assert np.array_equal(fx["E"]["f"], dc.empty_metrics()) and fx["E"]["count"] == 0
    for name in ("D", "G"):  # negative aligned values: rmse_log alone is NaN
        assert [math.isnan(v) for v in fx[name]["f"]] == [k == "rmse_log" for k in dc.METRICS]
    _, _, m = dc.make_case("C2")
    assert m.flatten(1).sum(1).tolist() == [100, 101]
    _, _, m = dc.make_case("B")
    assert int(m[2].sum()) == 0 and int(m[:2].sum()) > 200
    _, _, m = dc.make_case("F")
    assert m.flatten(1).sum(1).tolist() == [320, 64]
    pred, _, _ = dc.make_case("R")
    assert bool((pred == 3.0).all())


def test_workspace_bytes_is_positive_and_non_decreasing():
    from nndepth_amd._lib import lib
    sizes = [lib.nnd_depth_eval_workspace_bytes(B) for B in (1, 2, 3, 8, 64, 1000)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert lib.nnd_depth_eval_workspace_bytes(0) < 0 and b"batch" in lib.nnd_last_error()
    assert lib.nnd_depth_eval_workspace_bytes(-3) < 0


def test_bad_arguments_come_back_as_status_and_message():
    from nndepth_amd._lib import lib
    n = lib.nnd_depth_eval_workspace_bytes(2)
    buf = (C.c_double * (n // 8))()
    one = C.cast(buf, C.c_void_p)  # a host buffer: every check below answers before anything is launched
    args = lambda **k: [k.get("pred", one), k.get("gt", one), None, k.get("B", 2), k.get("H", 4), k.get("W", 4), 80.0,
                        k.get("ws", one), k.get("n", n), k.get("out", one), None]
    for k in ("pred", "gt", "ws", "out"):
        assert lib.nnd_depth_eval(*args(**{k: None})) == -1 and b"null" in lib.nnd_last_error(), k
    for k in (dict(B=0), dict(H=0), dict(W=-1), dict(B=70000)):
        assert lib.nnd_depth_eval(*args(**k)) == -1 and b"shape" in lib.nnd_last_error(), k
    assert lib.nnd_depth_eval(*args(B=2, H=32768, W=32768)) == -1 and b"2^31" in lib.nnd_last_error()
    assert lib.nnd_depth_eval(*args(n=n - 1)) == -1 and b"workspace" in lib.nnd_last_error()
    assert lib.nnd_depth_eval(*args(n=0)) == -1 and b"workspace" in lib.nnd_last_error()
    assert lib.nnd_depth_eval_accumulate(None, one, one, None) == -1 and b"null" in lib.nnd_last_error()
    assert lib.nnd_depth_eval_accumulate(one, one, None, None) == -1


def test_python_seam_refuses_before_the_device():
    import torch
    from nndepth_amd._lib import NndError
    from nndepth_amd.prepost import DEPTH_METRICS, DepthEvalCriterion, DepthEvalMean
    assert DEPTH_METRICS == dc.METRICS
    crit = DepthEvalCriterion()
    x = torch.ones(1, 1, 4, 4)
    with pytest.raises(NndError, match="HIP device"):
        crit(x, x)
    with pytest.raises(NndError, match="valid_mask"):
        crit(x, x, torch.ones(1, 1, 4, 4))
    with pytest.raises(NndError, match=r"\(B,1,H,W\)"):
        crit(torch.ones(1, 2, 4, 4), torch.ones(1, 2, 4, 4))
    with pytest.raises(NndError, match="one shape"):
        crit(x, torch.ones(1, 1, 4, 5))
    assert DepthEvalMean().result() == dict(zip(dc.METRICS, dc.empty_metrics().tolist()))
