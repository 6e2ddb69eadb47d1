"""CPU: the fixture of the monocular loss value (tests/golden/midas_loss.npz, scripts/make_golden_midas_loss.py) is consistent —
the cases regenerate from their names, the tests' float64 statement of the contract (midas_loss_cases.contract64, torch) reproduces
the script's (numpy), the reference's fp32 results lie within the script's cap — and the entry points' host-side checks answer
with a status and a message, without a device."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import midas_loss_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1e-5  # scripts/make_golden_midas_loss.py refuses a case above it
SYMBOLS = ("nnd_midas_loss_workspace_bytes", "nnd_midas_loss", "nnd_midas_loss_accumulate")


@pytest.fixture(scope="module")
def fx(gold):
    g = gold("midas_loss.npz")
    names = json.loads(str(g["names"]))
    assert tuple(names) == mc.NAMES
    assert [tuple(s) for s in g["shapes"].tolist()] == [c[1] for c in mc.CASES]
    return {n: dict(r=g["r"][i], f=g["f"][i], n=int(g["n"][i]), kept=int(g["kept"][i])) for i, n in enumerate(names)}


@pytest.fixture(scope="module")
def restated():
    return {name: mc.contract64(*mc.make_case(name)) for name in mc.NAMES}


@pytest.mark.parametrize("name", mc.NAMES)
def test_float64_restatement_reproduces_the_fixture(fx, restated, name):
    f, n, kept = restated[name]
    assert n == fx[name]["n"] and kept == fx[name]["kept"]
    for k, a, b in zip(mc.VALUES, f, fx[name]["f"]):
        if math.isfinite(b):
            assert abs(a - b) <= 1e-12 * max(1.0, abs(b)), (name, k, a, b)
        else:
            assert mc.same_or_both_nan(a, b), (name, k, a, b)


@pytest.mark.parametrize("name", mc.NAMES)
def test_reference_results_lie_within_the_cap(fx, name):
    for k, a, b in zip(mc.VALUES, fx[name]["r"], fx[name]["f"]):
        if math.isfinite(b):
            assert math.isfinite(a) and abs(a - b) <= CAP * max(1.0, abs(b)), (name, k, a, b)
            assert a == float(np.float32(a))  # an fp32 result, held exactly
        else:
            assert mc.same_or_both_nan(a, b), (name, k, a, b)


def test_cases_cover_what_they_are_there_for(fx):
    per_sample = lambda name: mc.make_case(name)[2].flatten(1).sum(1).tolist()
    assert per_sample("A") == [256, 256]
    b = per_sample("B")
    assert b[1] == 6 and 100 < b[0] < 17 * 19 - 100 and fx["B"]["n"] == sum(b) and fx["B"]["kept"] == b[0] - int(b[0] * 0.1)
    c = per_sample("C")
    assert c[2] == 0 and min(c[:2]) > 900 and all(math.isfinite(v) for v in fx["C"]["f"])
    assert per_sample("T") == [320, 310] and (310 - 31) % 2 == 1
    pred, t, m = mc.make_case("T")
    half = 16 * 20 // 2
    for x in (pred, t, m):  # sample 1: every valid (pred, target) pair twice
        flat = x[1, 0].flatten()
        assert torch.equal(flat[:half], flat[half:])
    assert bool((pred * 2 == (pred * 2).round()).all()) and bool((t * 2 == (t * 2).round()).all())
    assert bool((mc.make_case("K")[0] == 3.0).all()) and fx["K"]["f"][3] == 1.0  # sp = 0, mean |st| = 1 by construction
    assert per_sample("N9") == [9] and fx["N9"]["kept"] == 0 and per_sample("N10") == [10] and fx["N10"]["kept"] == 9
    assert [math.isnan(v) for v in fx["N9"]["f"]] == [True, True, False, False]
    assert per_sample("E") == [0, 0] and all(math.isnan(v) for v in fx["E"]["f"]) and fx["E"]["n"] == 0 and fx["E"]["kept"] == 0
    assert fx["H"]["n"] > 384 * 384 * 0.69


def test_case_z_is_decided_by_the_first_maximum():
    """Both windows hold four equal T (the batch's minimum normalises to exactly 0, invalid pixels are set to 0): the pooled mask bit
    is the FIRST pixel's: set in sample 0 (the valid minimum leads), cleared in sample 1 (an invalid pixel leads).  Another rule
    (the last maximum, or a valid pixel preferred) flips one of the two."""
    _, t, m = mc.make_case("Z")
    tv = t[m]
    assert float(tv.min()) == 0.25 and int((tv == tv.min()).sum()) == 2
    tn = torch.where(m, (t.double() - 0.25) / (float(tv.max()) - 0.25 + 1e-6), torch.zeros((), dtype=torch.float64))
    pooled, idx = F.max_pool2d(tn, 2, stride=2, return_indices=True)
    pm = m.flatten(2).gather(2, idx.flatten(2)).view_as(idx)
    (b0, y0, x0), (b1, y1, x1) = mc.Z_MIN
    assert (y0 % 2, x0 % 2) == (0, 0) and (y1 % 2, x1 % 2) == (1, 1) and bool(m[b0, 0, y0, x0]) and bool(m[b1, 0, y1, x1])
    for b, y, x in mc.Z_MIN:
        assert float(tn[b, 0, y, x]) == 0.0 and float(pooled[b, 0, y // 2, x // 2]) == 0.0
        assert int(m[b, 0, y // 2 * 2:y // 2 * 2 + 2, x // 2 * 2:x // 2 * 2 + 2].sum()) == 1
    assert bool(pm[b0, 0, y0 // 2, x0 // 2]) and not bool(pm[b1, 0, y1 // 2, x1 // 2])
    assert int(pm.sum()) == 2 * 64 - 1


def test_symbols_are_declared_in_the_header_and_the_ctypes_table():
    from nndepth_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nndepth_amd.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, src), f"{s} is not declared in include/nndepth_amd.h"
        assert s in _lib.SIGNATURES and hasattr(raw, s), s


def test_workspace_bytes_is_positive_and_grows_with_the_shape():
    from nndepth_amd._lib import lib
    sizes = [lib.nnd_midas_loss_workspace_bytes(*s) for s in ((1, 16, 16), (1, 17, 19), (2, 17, 19), (2, 40, 72), (8, 384, 384))]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 8 == 0 for s in sizes)
    assert sizes[0] >= 8 * 16 * 16 + 2 * 8 * (64 + 16 + 4) + (64 + 16 + 4)  # e, the pooled T and P in doubles, the pooled mask
    for bad in ((0, 16, 16), (-1, 16, 16), (70000, 16, 16)):
        assert lib.nnd_midas_loss_workspace_bytes(*bad) < 0 and b"shape" in lib.nnd_last_error(), bad
    for bad in ((1, 15, 16), (1, 16, 15), (2, 8, 384)):
        assert lib.nnd_midas_loss_workspace_bytes(*bad) < 0 and b"at least 16" in lib.nnd_last_error(), bad


def test_bad_arguments_come_back_as_status_and_message():
    from nndepth_amd._lib import lib
    n = lib.nnd_midas_loss_workspace_bytes(2, 16, 16)
    buf = (C.c_double * (n // 8))()
    one = C.cast(buf, C.c_void_p)  # a host buffer: every check below answers before anything is launched
    args = lambda **k: [k.get("pred", one), k.get("target", one), k.get("mask", one), k.get("B", 2), k.get("H", 16), k.get("W", 16),
                        k.get("sb", 256), k.get("sy", 16), 1.0, 0.1, k.get("ws", one), k.get("n", n), k.get("out", one), None]
    for k in ("pred", "target", "mask", "ws", "out"):
        assert lib.nnd_midas_loss(*args(**{k: None})) == -1 and b"null" in lib.nnd_last_error(), k
    for k in (dict(B=0), dict(H=0), dict(W=-1), dict(B=70000)):
        assert lib.nnd_midas_loss(*args(**k)) == -1 and b"shape" in lib.nnd_last_error(), k
    for k in (dict(H=15), dict(W=15), dict(H=8, W=8)):  # the host refusal of a map too small for four levels, before any launch
        assert lib.nnd_midas_loss(*args(**k)) == -1 and b"at least 16" in lib.nnd_last_error(), k
    assert lib.nnd_midas_loss(*args(B=2, H=32768, W=32768, sy=32768)) == -1 and b"2^31" in lib.nnd_last_error()
    assert lib.nnd_midas_loss(*args(sy=15)) == -1 and b"strides" in lib.nnd_last_error()
    assert lib.nnd_midas_loss(*args(n=n - 1)) == -1 and b"workspace" in lib.nnd_last_error()
    assert lib.nnd_midas_loss(*args(n=0)) == -1 and b"workspace" in lib.nnd_last_error()
    assert lib.nnd_midas_loss_accumulate(None, one, one, None) == -1 and b"null" in lib.nnd_last_error()
    assert lib.nnd_midas_loss_accumulate(one, one, None, None) == -1


def test_python_seam_refuses_before_the_device():
    from nndepth_amd._lib import NndError
    from nndepth_amd.prepost import MIDAS_LOSS_METRICS, MiDasLoss, MiDasLossMean
    assert MIDAS_LOSS_METRICS == mc.VALUES
    crit = MiDasLoss()
    assert (crit.trimmed_loss_coef, crit.gradient_reg_coef) == mc.COEFS
    x, m = torch.ones(1, 1, 16, 16), torch.ones(1, 1, 16, 16, dtype=torch.bool)
    small, msmall = torch.ones(1, 1, 15, 16), torch.ones(1, 1, 15, 16, dtype=torch.bool)
    with pytest.raises(NndError, match="at least 16"):  # CPU tensors: the size is judged before the device is asked for
        crit(small, small, msmall)
    with pytest.raises(NndError, match="at least 16"):
        crit(small.transpose(2, 3), small.transpose(2, 3), msmall.transpose(2, 3))
    with pytest.raises(NndError, match="HIP device"):
        crit(x, x, m)
    with pytest.raises(NndError, match="valid_mask is required"):
        crit(x, x, None)
    with pytest.raises(NndError, match="valid_mask is torch.bool"):
        crit(x, x, m.float())
    with pytest.raises(NndError, match="fp32"):
        crit(x.double(), x, m)
    with pytest.raises(NndError, match=r"\(B,1,H,W\)"):
        crit(x.expand(1, 2, 16, 16), x.expand(1, 2, 16, 16), m.expand(1, 2, 16, 16))
    with pytest.raises(NndError, match="one shape"):
        crit(x, torch.ones(1, 1, 16, 17), m)
    res = MiDasLossMean().result()
    assert list(res.keys()) == [f"val/{k}" for k in mc.VALUES] and all(math.isnan(v) for v in res.values())
