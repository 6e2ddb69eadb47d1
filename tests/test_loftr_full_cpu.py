"""CPU: the LoFTR full (softmax) attention's host side: argument checks of its three C-ABI entry points, the Python seams'
`attention` switch, the token-level PyTorch path against the fixture and the float64 contract, and the fixture itself
(tests/golden/loftr_full.npz, scripts/make_golden_loftr_full.py; cases and contract in tests/loftr_full_cases.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import loftr_full_cases as lc


def _tok(t):
    n, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(n, h * w, c)


def test_argument_checks():
    """Every argument error is a negative status before any HIP call (this host has no device)."""
    from nndepth_amd._lib import lib
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    att = lambda q=p, k=p, v=p, o=p, N=1, nhead=2, L=3, S=5, qbs=192, kvbs=320, obs=192: lib.nnd_full_attention(
        q, k, v, o, N, nhead, L, S, qbs, kvbs, obs, None)
    for kw in ({"q": None}, {"k": None}, {"v": None}, {"o": None}, {"N": 0}, {"N": -1}, {"nhead": 0}, {"L": 0}, {"L": -3}, {"S": 0},
               {"S": -5}, {"qbs": 191}, {"kvbs": 319}, {"obs": 191}):  # strides below nhead * 32 * L / S: nhead * 32 != C
        assert att(**kw) < 0, kw
    ws = lib.nnd_loftr_full_workspace_floats
    assert ws(256, 8, 2, 33, 60) == 6 * 2 * 256 * 33 * 60  # q, k, v, message and the 2C-wide hidden map
    assert ws(256, 8, 2, 33, 60) < lib.nnd_loftr_workspace_floats(256, 8, 2, 33, 60)
    for bad in ((256, 4, 1, 8, 8), (250, 8, 1, 8, 8), (256, 0, 1, 8, 8), (256, 8, 0, 8, 8), (256, 8, 1, 0, 8), (256, 8, 1, 8, -1)):
        assert ws(*bad) < 0, bad
    fwd = lambda d=256, nh=8, pk=p, x=p, s=p, o=p, w=p, N=1, H=2, W=2: lib.nnd_loftr_full_layer_forward(d, nh, pk, x, s, o, w, N, H, W, None)
    for kw in ({"pk": None}, {"x": None}, {"s": None}, {"o": None}, {"w": None}, {"N": 0}, {"H": 0}, {"W": 0}, {"H": -2}, {"nh": 4},
               {"d": 250}):
        assert fwd(**kw) < 0, kw


def test_attention_switch_keeps_the_parameters():
    from nndepth_amd import ops
    from nndepth_amd._lib import NndError
    from nndepth_amd.cre_stereo import LocalFeatureTransformer, LoFTREncoderLayer
    full, linear = LocalFeatureTransformer(256, 8, ["self"], "full"), LocalFeatureTransformer(256, 8, ["self"], "linear")
    assert list(full.state_dict().keys()) == list(linear.state_dict().keys())
    assert [tuple(t.shape) for t in full.state_dict().values()] == [tuple(t.shape) for t in linear.state_dict().values()]
    assert LocalFeatureTransformer(256, 8, ["cross"]).attention == "linear" and LoFTREncoderLayer(256, 8).attention == "linear"
    for cls, args in ((LocalFeatureTransformer, (256, 8, ["self"], "softmax")), (LoFTREncoderLayer, (256, 8, "softmax"))):
        with pytest.raises(ValueError):
            cls(*args)
    sd = lc.state_dict()
    a = ops.LoftrEngine(256, 8, "full").load(sd, "self_att_fn.layers.0.", device="cpu")
    b = ops.LoftrEngine(256, 8, "linear").load(sd, "self_att_fn.layers.0.", device="cpu")
    assert ops.LoftrEngine(256, 8).attention == "linear"
    assert torch.equal(a.packed, b.packed) and a.packed_floats == b.packed_floats
    with pytest.raises(NndError):
        ops.LoftrEngine(256, 8, "softmax")
    with pytest.raises(NndError):
        ops.LoftrEngine(256, 4)
    with pytest.raises(NndError):
        ops.LoftrEngine(256, 4, "full")


def test_model_keyword_and_checkpoint():
    from nndepth_amd.cre_stereo import CREStereoBase
    full, linear = CREStereoBase(iters=2, attention="full"), CREStereoBase(iters=2)
    assert full.self_att_fn.attention == full.cross_att_fn.attention == "full" and linear.self_att_fn.attention == "linear"
    assert list(full.state_dict().keys()) == list(linear.state_dict().keys())
    full.load_state_dict(linear.state_dict(), strict=True)
    with pytest.raises(ValueError):
        CREStereoBase(iters=2, attention="softmax")


def _token_layer(name):
    from nndepth_amd.cre_stereo import LoFTREncoderLayer
    prefix, x, source = lc.make_case(name)
    layer = LoFTREncoderLayer(lc.D_MODEL, lc.NHEAD, "full").eval()
    layer.load_state_dict({k[len(prefix):]: t for k, t in lc.state_dict().items() if k.startswith(prefix)}, strict=True)
    n, c, h, w = x.shape
    with torch.no_grad():
        return layer(_tok(x), _tok(source)).reshape(n, h, w, c).permute(0, 3, 1, 2)


@pytest.mark.parametrize("name", lc.STORED)
def test_token_path_vs_stored_reference(name):
    """The package's token-level layer against the reference's stored fp32 output: within the reference's own distance from the
    float64 contract."""
    fx = lc.fixture()[name]
    err = float((_token_layer(name).double().numpy() - fx["ref_out"].astype(np.float64)).__abs__().max())
    print(f"{name}: |token path - reference| = {err:.3e}, d_ref = {fx['d_ref']:.3e}")
    assert fx["ref_out"].shape == tuple(lc.make_case(name)[1].shape)
    assert err <= fx["d_ref"]


@pytest.mark.parametrize("name", lc.LAYER_CASES)
def test_token_path_vs_contract(name):
    got = _token_layer(name)
    assert bool(torch.isfinite(got).all())
    err = float(np.abs(got.double().numpy() - lc.contract(name)).max())
    print(f"{name}: |token path - contract| = {err:.3e}, bar = {lc.bar(name):.3e}")
    assert err <= lc.bar(name)


def test_token_attention_is_the_contract():
    """LoFTREncoderLayer._attend("full") on (N, L, H, D) tokens against contract64_attention on the channel-major maps, L != S."""
    from nndepth_amd.cre_stereo import LoFTREncoderLayer
    name = "att/2x8x40x97/g4"
    q, k, v, nhead = lc.make_case(name)
    tok = lambda t: t.reshape(t.shape[0], nhead, lc.HEAD, t.shape[2]).permute(0, 3, 1, 2)
    got = LoFTREncoderLayer(lc.D_MODEL, nhead, "full")._attend(tok(q), tok(k), tok(v)).permute(0, 2, 3, 1).reshape(q.shape)
    assert float(np.abs(got.double().numpy() - lc.contract(name)).max()) <= lc.bar(name)


def test_fixture_integrity():
    fx = lc.fixture()
    assert set(fx) == set(lc.CASES) and not set(lc.REFUSED) & set(fx)
    for name in lc.CASES:
        d, f = fx[name]["d_ref"], fx[name]["fmax"]
        assert 0.0 <= d <= lc.CAP * max(1.0, f), name
        # the committed contract reproduces fmax (float64; the inputs are fp32 roundings of float64 Box-Muller values)
        assert abs(float(np.abs(lc.contract(name)).max()) - f) <= 1e-6 * f, name
    for name in lc.STORED:
        ref = fx[name]["ref_out"]
        assert ref.dtype == np.float32 and abs(float(np.abs(ref.astype(np.float64) - lc.contract(name)).max()) - fx[name]["d_ref"]) <= 1e-6 * fx[name]["fmax"]


def test_gather_construction():
    """The exact-gather inputs of the GPU test: the float64 margin, and fp32 PyTorch gathers exactly."""
    for n, nhead, l, s in lc.GATHER_SHAPES:
        q, k, v, pi = lc.gather_case(n, nhead, l, s)
        assert lc.gather_margin(q, k, nhead, pi) >= 120.0
        assert len({tuple(col) for col in k[0, :lc.HEAD].t().tolist()}) == s  # distinct keys
        tok = lambda t: t.reshape(n, nhead, lc.HEAD, t.shape[2]).permute(0, 3, 1, 2)
        a = torch.softmax(torch.einsum("nlhd,nshd->nlsh", tok(q), tok(k)) / lc.HEAD ** 0.5, dim=2)
        out = torch.einsum("nlsh,nshd->nlhd", a, tok(v)).permute(0, 2, 3, 1).reshape(q.shape)
        assert torch.equal(out, v[:, :, pi])
