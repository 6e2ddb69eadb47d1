"""CPU: the fixture of the stereo evaluation criterion (tests/golden/stereo_eval.npz, scripts/make_golden_stereo_eval.py) is
consistent — the cases regenerate from their names, the tests' float64 statement of the contract (stereo_eval_cases.contract64,
torch) reproduces the script's (numpy), the reference's fp32 results lie within the script's cap, the cases cover what they are
there for — and the entry points' host-side checks answer with a status and a message, without a device."""
import ctypes as C
import json
import math

import numpy as np
import pytest

import stereo_eval_cases as sc

CAP = 1e-5  # scripts/make_golden_stereo_eval.py refuses a case above it


@pytest.fixture(scope="module")
def fx(gold):
    g = gold("stereo_eval.npz")
    assert tuple(json.loads(str(g["names"]))) == sc.NAMES
    assert tuple(json.loads(str(g["columns"]))) == sc.COLUMNS
    return {n: {k: g[f"{n}/{k}"] for k in ("r", "has_r", "f", "counts", "loss")} for n in sc.NAMES}


@pytest.fixture(scope="module")
def restated():
    return {name: sc.contract64(sc.make_case(name)) for name in sc.NAMES}


def _close(a, b, tol):
    return abs(a - b) <= tol * max(1.0, abs(b)) if math.isfinite(b) else (math.isnan(a) and math.isnan(b))


@pytest.mark.parametrize("name", sc.NAMES)
def test_float64_restatement_reproduces_the_fixture(fx, restated, name):
    f, loss, counts = restated[name]
    want = fx[name]
    assert f.shape == want["f"].shape == (len(sc.make_case(name).outputs), sc.K)
    assert np.array_equal(counts, want["counts"])
    for i in range(f.shape[0]):
        for k, col in enumerate(sc.COLUMNS):
            assert _close(f[i, k], want["f"][i, k], 1e-12), (name, i, col, f[i, k], want["f"][i, k])
    assert _close(loss, want["loss"][0], 1e-12)


@pytest.mark.parametrize("name", sc.NAMES)
def test_reference_results_lie_within_the_cap(fx, name):
    r, has, f = fx[name]["r"], fx[name]["has_r"], fx[name]["f"]
    assert has[:, 0].all() and has[:, 3:3 + len(sc.ABOVE)].all() and not has[:, 1:3].any()
    for i, k in zip(*np.nonzero(has)):
        assert _close(r[i, k], f[i, k], CAP), (name, i, sc.COLUMNS[k], r[i, k], f[i, k])
        assert math.isnan(r[i, k]) or r[i, k] == float(np.float32(r[i, k]))  # an fp32 result, held exactly
    loss_f, loss_r, loss_has = fx[name]["loss"]
    assert bool(loss_has) == (sc.make_case(name).mask is None)
    if loss_has:
        assert _close(loss_r, loss_f, CAP)
        assert has[-1, 3 + len(sc.ABOVE):].all()  # RAFTLoss's metrics of the last output


def test_cases_cover_what_they_are_there_for(fx):
    # T: pred - gt is exactly T_DELTAS[i % 5]; strict comparisons on both sides, counts in closed form
    t = sc.make_case("T")
    assert np.array_equal((t.outputs[0] - t.gt).numpy().reshape(-1), np.array(sc.T_DELTAS, np.float32)[np.arange(320) % 5])
    assert fx["T"]["counts"][0].tolist() == [320, 128, 64, 64, 128, 192, 256]  # valid, > 1, > 3, < 0.5, < 1, < 3, < 5
    assert fx["T"]["f"][0, 0] == pytest.approx(2.15, abs=1e-12) and fx["T"]["f"][0, 2] == fx["T"]["f"][0, 0]
    # E: nothing valid
    e = fx["E"]["f"][0]
    assert e[1] == 0 and e[2] == 0 and np.isnan(e[[0] + list(range(3, sc.K))]).all() and not fx["E"]["counts"].any()
    # B: sample 2 fully masked, the others partly
    b = sc.make_case("B")
    assert int(b.mask[2].sum()) == 0 and 0 < int(b.mask[:2].sum()) < b.mask[:2].numel()
    # M: the magnitude test cuts part of the ground truth off
    m = sc.make_case("M")
    assert 0 < fx["M"]["counts"][0, 0] < m.gt.numel() and float(m.gt.abs().max()) > m.max_flow
    # every threshold splits the pixels of the general cases
    for name in ("A", "B", "C", "D", "M", "G2", "G3", "G4", "V"):
        c = fx[name]["counts"][0]
        assert all(0 < v < c[0] for v in c[1:]), (name, c)
    # the pooled sizes: equal to the output (G2, with a dropped row), resampled rows (G3), resampled columns (G4)
    sizes = {n: (g, o[0][1:]) for n, g, o in sc.CASES}
    assert sc.pooled_size(*sizes["G2"]) == (37, 62) == sizes["G2"][1] and 37 * 2 < 75
    assert sc.pooled_size(*sizes["G3"]) == (25, 41) and sizes["G3"][1] == (24, 41)
    assert sc.pooled_size(*sizes["G4"]) == (25, 43) and sizes["G4"][1] == (25, 42)
    # S: three size groups under a 1-channel ground truth; R: views of one stacked tensor; V: a strided view
    s = sc.make_case("S")
    assert s.gt.shape[1] == 1 and len({tuple(o.shape) for o in s.outputs}) == 3 and all(o.shape[1] == 2 for o in s.outputs)
    r = sc.make_case("R")
    assert len(r.outputs) == 8 and len({o.untyped_storage().data_ptr() for o in r.outputs}) == 1 and r.mask is not None
    v = sc.make_case("V").outputs[0]
    assert not v.is_contiguous() and v.stride() == (44 * 60, 44 * 60, 60, 1) and v.storage_offset() == 3 * 60 + 2


def test_workspace_bytes_is_positive_and_non_decreasing():
    from nndepth_amd._lib import lib
    sizes = [lib.nnd_stereo_eval_workspace_bytes(n) for n in (1, 2, 3, 8, 32, 64)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:]))
    for n in (0, -3, 65):
        assert lib.nnd_stereo_eval_workspace_bytes(n) < 0 and b"outputs" in lib.nnd_last_error(), n


def _desc(one, **k):
    from nndepth_amd._lib import StereoEvalDesc
    d = StereoEvalDesc()
    d.gt, d.B, d.Cg, d.H, d.W = k.get("gt", one.value), k.get("B", 2), k.get("Cg", 1), k.get("H", 8), k.get("W", 12)
    d.mask, d.mask_h, d.mask_w = k.get("mask", None), k.get("mask_h", 0), k.get("mask_w", 0)
    d.gamma, d.max_flow = 0.8, 1000.0
    d.n_above, d.n_below = k.get("n_above", 2), k.get("n_below", 4)
    d.num_outputs = k.get("num_outputs", 2)
    for i in range(max(0, min(64, d.num_outputs))):
        o = d.outputs[i]
        o.data, o.C, o.h, o.w = one.value, 1, 8, 12
        o.stride_b, o.stride_c, o.stride_row = 96, 96, 12
    for key, v in k.get("out0", {}).items():
        setattr(d.outputs[0], key, v)
    return d


def test_bad_arguments_come_back_as_status_and_message():
    from nndepth_amd._lib import lib
    n = lib.nnd_stereo_eval_workspace_bytes(2)
    buf = (C.c_double * (n // 8))()
    one = C.cast(buf, C.c_void_p)  # a host buffer: every check below answers before anything is launched

    def call(ws=one, nbytes=n, out=one, **k):
        return lib.nnd_stereo_eval(C.byref(_desc(one, **k)), ws, nbytes, out, None), lib.nnd_last_error()

    assert lib.nnd_stereo_eval(None, one, n, one, None) == -1 and b"null" in lib.nnd_last_error()
    bad = _desc(one)
    bad.struct_size = 16
    assert lib.nnd_stereo_eval(C.byref(bad), one, n, one, None) == -1 and b"struct_size" in lib.nnd_last_error()
    bad = _desc(one)
    bad.flags = 4
    assert lib.nnd_stereo_eval(C.byref(bad), one, n, one, None) == -1 and b"flags" in lib.nnd_last_error()
    for k in (dict(gt=None), dict(ws=None), dict(out=None), dict(out0=dict(data=None))):
        rc, msg = call(**k)
        assert rc == -1 and b"null" in msg, k
    for k in (dict(B=0), dict(Cg=0), dict(H=-1), dict(W=0), dict(out0=dict(C=0)), dict(out0=dict(h=0)), dict(out0=dict(w=-2)),
              dict(B=4, H=32768, W=32768)):
        rc, msg = call(**k)
        assert rc == -1 and b"shape" in msg, k
    for k in (dict(num_outputs=0), dict(num_outputs=65), dict(num_outputs=-1)):
        rc, msg = call(**k)
        assert rc == -1 and b"outputs" in msg, k
    for k in (dict(n_above=9), dict(n_below=9), dict(n_above=-1)):
        rc, msg = call(**k)
        assert rc == -1 and b"thresholds" in msg, k
    for k in (dict(nbytes=n - 1), dict(nbytes=0)):
        rc, msg = call(**k)
        assert rc == -1 and b"workspace" in msg, k
    rc, msg = call(ws=C.c_void_p(one.value + 4))
    assert rc == -1 and b"aligned" in msg
    rc, msg = call(Cg=3)  # neither 1 nor the output's channel count
    assert rc == -1 and b"channels" in msg
    rc, msg = call(Cg=2, out0=dict(C=2))  # output 1 still has one channel
    assert rc == -1 and b"output 1" in msg and b"channels" in msg
    rc, msg = call(out0=dict(stride_row=-12))
    assert rc == -1 and b"stride" in msg
    rc, msg = call(out0=dict(w=13))  # wider than the ground truth: scale = 12 // 13 = 0
    assert rc == -1 and b"wider" in msg
    rc, msg = call(H=2, W=12, out0=dict(h=1, w=3))  # scale 4 leaves no row of a 2-row ground truth
    assert rc == -1 and b"no row" in msg
    rc, msg = call(mask=one.value, mask_h=8, mask_w=12, out0=dict(h=4, w=6))
    assert rc == -1 and b"valid_mask" in msg
    rc, msg = call(mask=one.value, mask_h=0, mask_w=12)
    assert rc == -1 and b"valid_mask" in msg

    assert lib.nnd_stereo_eval_accumulate(None, 4, one, None) == -1 and b"null" in lib.nnd_last_error()
    assert lib.nnd_stereo_eval_accumulate(one, 4, None, None) == -1 and b"null" in lib.nnd_last_error()
    assert lib.nnd_stereo_eval_accumulate(one, 0, one, None) == -1 and b"length" in lib.nnd_last_error()
    pool = lambda **k: lib.nnd_min_pool_nearest(k.get("gt", one), k.get("dst", one), k.get("B", 1), 1, k.get("H", 8), k.get("W", 12),
                                                k.get("h", 4), k.get("w", 6), None)
    assert pool(gt=None) == -1 and b"null" in lib.nnd_last_error()
    assert pool(dst=None) == -1 and b"null" in lib.nnd_last_error()
    assert pool(B=0) == -1 and b"shape" in lib.nnd_last_error()
    assert pool(h=0) == -1 and b"shape" in lib.nnd_last_error()
    assert pool(w=13) == -1 and b"wider" in lib.nnd_last_error()
    assert pool(H=1, h=1, w=3) == -1 and b"no row" in lib.nnd_last_error()


def test_python_seam_refuses_before_the_device():
    import torch
    from nndepth_amd._lib import NndError
    from nndepth_amd.prepost import EvalCriterion, StereoEvalCriterion, StereoEvalMean, downsample_gt
    crit = StereoEvalCriterion(sc.ABOVE, sc.BELOW)
    assert crit.columns == sc.COLUMNS
    assert StereoEvalCriterion().columns == ("epe", "count", "l1")
    x = torch.ones(1, 1, 4, 4)
    with pytest.raises(NndError, match="HIP device"):
        crit(x, x)
    with pytest.raises(NndError, match="HIP device"):
        crit(x, [{"up_disp": x}, {"up_disp": x}])
    with pytest.raises(NndError, match="HIP device"):
        downsample_gt(torch.ones(1, 1, 8, 8), (4, 4))
    with pytest.raises(NndError, match="HIP device"):
        EvalCriterion()(torch.ones(1, 1, 8, 8), torch.ones(1, 1, 4, 4))
    with pytest.raises(NndError, match="thresholds"):
        EvalCriterion({f"d{i}": float(i) for i in range(9)})(x, x)
    with pytest.raises(NndError, match="HIP device"):
        EvalCriterion({"count": 1.0})(x, x)  # the caller's keys are not column names
    with pytest.raises(NndError, match="outputs"):
        crit(x, [x] * 65)
    with pytest.raises(NndError, match="outputs"):
        crit(x, [])
    with pytest.raises(NndError, match="thresholds"):
        StereoEvalCriterion({f"d{i}": float(i) for i in range(9)})
    with pytest.raises(NndError, match="thresholds"):
        StereoEvalMean(below={f"b{i}": float(i) for i in range(9)})
    with pytest.raises(NndError, match="distinct"):
        StereoEvalCriterion({"1px": 1.0}, {"1px": 1.0})
    with pytest.raises(NndError, match=r"\(B,C,h,w\)"):
        crit(x, [torch.ones(4, 4)])
    mean = StereoEvalMean(sc.ABOVE)
    assert mean.curve() == [] and list(mean.result()) == ["epe", "d1", "d3"] and all(math.isnan(v) for v in mean.result().values())
    with pytest.raises(NndError, match="HIP device"):
        mean.update(x, [x])
    # the shapes are judged before the device
    with pytest.raises(NndError, match="channels"):
        crit(torch.ones(1, 3, 4, 4), [torch.ones(1, 2, 4, 4)])
    with pytest.raises(NndError, match="batch size"):
        crit(torch.ones(2, 1, 4, 4), [x])
    with pytest.raises(NndError, match="valid_mask"):
        crit(x, [x, torch.ones(1, 1, 2, 2)], torch.ones(1, 1, 4, 4, dtype=torch.bool))
    with pytest.raises(NndError, match="valid_mask"):
        crit(x, [x], torch.ones(1, 1, 4, 4))
    with pytest.raises(NndError, match="valid_mask"):
        crit(x, [x], torch.ones(2, 4, 4, dtype=torch.bool))
    with pytest.raises(NndError, match="fp32"):
        crit(x.double(), [x.double()])
