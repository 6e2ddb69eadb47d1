"""GPU: the LoFTR full (softmax) attention in HIP (csrc/attention.hip) from the kernel to the model: an exact gather that pins the
MFMA lane maps, tails and strides bit for bit; the attention and the whole layer against the float64 contract within a bar derived
from the reference's own fp32 error (tests/golden/loftr_full.npz; cases, contract and bar in tests/loftr_full_cases.py); history
independence; and CREStereoBase(attention="full") against the same model on the package's PyTorch token path.

With NND_LOFTR_FULL_REPORT=<path> the measured errors are written there, in the form of the "GPU:" section of
tests/golden/REPORT_loftr_full.txt."""
import os

import numpy as np
import pytest
import torch

import history_util as hu
import loftr_full_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_measured = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nndepth_amd import ops as o
    return o


def teardown_module(module):
    path = os.environ.get("NND_LOFTR_FULL_REPORT")
    if path and _measured:
        arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
        lines = ["GPU:", f"measured by tests/test_gpu_loftr_full.py on {arch}: max |HIP fp32 - float64 contract|, "
                 "the bar max(4 d_ref, 4 * 2^-23 fmax), error / d_ref (bar at 4; '-' where d_ref is 0: the floor decides)"]
        for name in lc.CASES:
            if name in _measured:
                err, d = _measured[name], lc.fixture()[name]["d_ref"]
                lines.append(f"case {name:36s} err = {err:.3e}  bar = {lc.bar(name):.3e}  d_ref = {d:.3e}  err / d_ref = "
                             + (f"{err / d:.2f}" if d > 0 else "-"))
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def _engine(ops, prefix):
    return ops.LoftrEngine(lc.D_MODEL, lc.NHEAD, "full").load(lc.state_dict(), prefix, device=DEV)


# ------------------------------------------------------------------------------------------------ 1. exact gather
@pytest.mark.parametrize("N,nhead,L,S", lc.GATHER_SHAPES)
def test_exact_gather(ops, N, nhead, L, S):
    """One-hot softmax by construction (loftr_full_cases.gather_case): out[..., i] is v[..., (7 i + 3) mod S] bit for bit, through
    the C-ABI with its strides.  Catches a swapped row / column of a lane map, a wrong key order in the P V step, a wrong head or
    batch stride and a wrong tail mask; the winners fall in every KV tile, before and after the running maximum changes."""
    q, k, v, pi = lc.gather_case(N, nhead, L, S)
    margin = lc.gather_margin(q, k, nhead, pi)
    print(f"\ngather {N}x{nhead}x{L}x{S}: smallest float64 margin {margin:.0f}")
    assert margin >= 120.0
    got = ops.full_attention(q.to(DEV), k.to(DEV), v.to(DEV), nhead).cpu()
    want = v[:, :, pi]
    assert got.shape == want.shape
    wrong = int((got.view(torch.int32) != want.contiguous().view(torch.int32)).sum())
    assert wrong == 0, f"{wrong} of {want.numel()} outputs are not the gathered value's bits"


# ------------------------------------------------------------------------------------------------ 2. attention vs float64
@pytest.mark.parametrize("name", lc.ATT_CASES)
def test_attention_vs_float64(ops, name):
    q, k, v, nhead = lc.make_case(name)
    got = ops.full_attention(q.to(DEV), k.to(DEV), v.to(DEV), nhead).cpu()
    assert bool(torch.isfinite(got).all()), "NaN or inf in the output"
    err = float(np.abs(got.double().numpy() - lc.contract(name)).max())
    _measured[name] = err
    fx = lc.fixture()[name]
    print(f"\n{name}: err {err:.3e}  d_ref {fx['d_ref']:.3e}  fmax {fx['fmax']:.4g}  bar {lc.bar(name):.3e}")
    assert err <= lc.bar(name)


# ------------------------------------------------------------------------------------------------ 3. layer vs float64
@pytest.mark.parametrize("name", lc.LAYER_CASES)
def test_layer_vs_float64(ops, name):
    """nnd_loftr_full_layer_forward through LoftrEngine against contract64_layer: the bar of the attention test and the project's
    3e-5 * max(1, fmax) of test_gpu_parity.py::test_loftr_layer_vs_oracle."""
    prefix, x, source = lc.make_case(name)
    got = _engine(ops, prefix).forward(x.to(DEV), source.to(DEV)).cpu()
    assert bool(torch.isfinite(got).all()), "NaN or inf in the output"
    err = float(np.abs(got.double().numpy() - lc.contract(name)).max())
    _measured[name] = err
    fx = lc.fixture()[name]
    print(f"\n{name}: err {err:.3e}  d_ref {fx['d_ref']:.3e}  fmax {fx['fmax']:.4g}  bar {lc.bar(name):.3e}  err / d_ref {err / fx['d_ref']:.2f}")
    assert err <= lc.bar(name)
    assert err <= 3e-5 * max(1.0, fx["fmax"])


# ------------------------------------------------------------------------------------------------ 4. history independence
def _call_layer(eng, name):
    _, x, source = lc.make_case(name)
    return eng.forward(x.to(DEV), source.to(DEV))


def test_history_independence(ops, monkeypatch):
    """Equal bits from two calls; with the workspace and every allocated output pre-filled with NaN; and after a larger shape."""
    from nndepth_amd._lib import lib
    small, big = "layer/2x5x8/cross/g4", "layer/2x9x15/cross/g1"
    eng = _engine(ops, "cross_att_fn.layers.0.")
    base = hu.snapshot(_call_layer(eng, small))
    assert not hu.differences(base, hu.snapshot(_call_layer(eng, small)))
    need = int(lib.nnd_loftr_full_workspace_floats(lc.D_MODEL, lc.NHEAD, 2, 5, 8))
    ws = eng._ws = hu.aligned_buffer(need, "nan", DEV, 1)
    with hu.poisoned_allocators(monkeypatch, "nan", 1) as filled:
        res = hu.snapshot(_call_layer(eng, small))
    torch.cuda.synchronize()
    assert filled and eng._ws.data_ptr() == ws.data_ptr()  # ran on the NaN-filled workspace of exactly the documented size
    assert not hu.differences(base, res)
    used = _engine(ops, "cross_att_fn.layers.0.")
    _call_layer(used, big)
    ws_big = used._ws
    res = hu.snapshot(_call_layer(used, small))
    assert used._ws is ws_big
    assert not hu.differences(base, res)
    # the attention alone: same bits twice, and into a NaN-filled output
    q, k, v, nhead = (t.to(DEV) if torch.is_tensor(t) else t for t in lc.make_case("att/2x8x40x97/g4"))
    a = ops.full_attention(q, k, v, nhead)
    with hu.poisoned_allocators(monkeypatch, "nan", 2) as filled:
        b = ops.full_attention(q, k, v, nhead)
    assert filled and not hu.differences([a], [b])


# ------------------------------------------------------------------------------------------------ 5. the model
def test_model_full_attention_vs_token_path(monkeypatch):
    """CREStereoBase(attention="full") on 2 x 3 x 160 x 224 (5 x 7 = 35 tokens at 1/32: more than one 32-query block): the HIP
    attention against the same model with LocalFeatureTransformer.hip_ready patched to False (the package's PyTorch token path);
    every other kernel is shared, every output within the project's 1e-4.  A checkpoint of attention="linear" loads strictly."""
    from nndepth_amd import weightgen
    from nndepth_amd.cre_stereo import CREStereoBase, LocalFeatureTransformer
    linear = CREStereoBase(iters=2, arithmetic="fp32")
    linear.load_state_dict(lc.state_dict(), strict=True)
    model = CREStereoBase(iters=2, attention="full", arithmetic="fp32")
    model.load_state_dict(linear.state_dict(), strict=True)
    model = model.eval().to(DEV)
    f1, f2 = (t.to(DEV) for t in weightgen.synthetic_frames(11, 2, 160, 224))
    calls = []
    real = LocalFeatureTransformer.forward_maps
    monkeypatch.setattr(LocalFeatureTransformer, "forward_maps", lambda self, a, b: (calls.append(self.hip_ready(a)), real(self, a, b))[1])
    hip = [o["up_disp"].clone() for o in model(f1, f2)]
    assert calls and all(calls), "the HIP attention did not run"
    n_hip = len(calls)
    monkeypatch.setattr(LocalFeatureTransformer, "hip_ready", lambda self, t: False)
    tok = [o["up_disp"].clone() for o in model(f1, f2)]
    assert len(calls) == 2 * n_hip and not any(calls[n_hip:])
    assert len(hip) == len(tok) == 4 and [o.shape for o in hip] == [o.shape for o in tok] and tuple(hip[-1].shape) == (2, 2, 160, 224)
    errs = [float((a - b).abs().max()) for a, b in zip(hip, tok)]
    print(f"\nCREStereoBase full attention, HIP vs token path: max-abs per output {' '.join(f'{e:.1e}' for e in errs)} "
          f"(|flow| max {float(tok[-1].abs().max()):.1f})")
    assert all(bool(torch.isfinite(o).all()) for o in hip)
    assert max(errs) <= 1e-4, errs
    # and full attention is not the linear one: the switch reaches the kernels
    lin = [o["up_disp"] for o in linear.eval().to(DEV)(f1, f2)]
    assert float((lin[-1] - tok[-1]).abs().max()) > 1e-4
