"""GPU: the frame-size stage outputs of the Coarse2Fine cascade in HIP (nnd_resize_nearest_scaled, csrc/cascade.hip;
nndepth_amd.raft_stereo.frame_size_outputs) against the expression they replace, F.interpolate(u, size=frame) * rate
(raft_stereo/model.py:309-314), bit for bit — NaN payloads and signed zeros included, so the comparison is on the bit patterns."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("n,h,w,ry,rx,mul", [(12, 8, 15, 16, 16, 16.0), (12, 32, 60, 4, 4, 4.0), (3, 5, 7, 3, 3, 3.0), (2, 4, 6, 2, 4, 4.0),
                                             (1, 1, 1, 8, 8, 8.0), (2, 3, 5, 1, 1, 1.0)])
def test_resize_nearest_scaled_is_interpolate_times_rate(n, h, w, ry, rx, mul):
    from nndepth_amd import ops
    g = torch.Generator().manual_seed(100 * h + w)
    u = (torch.randn((n, 1, h, w), generator=g) * 50).to(DEV)
    flat = u.view(-1)
    flat[0] = float("nan")
    if flat.numel() > 3:
        flat[1], flat[2], flat[3] = 0.0, -0.0, -7.25
    H, W = h * ry, w * rx
    exp = torch.nn.functional.interpolate(u, size=(H, W)) * mul
    got = ops.resize_nearest_scaled(u, (H, W), mul)
    assert torch.isnan(got).sum() == ry * rx and _same_bits(got, exp)
    # the fused loop's layout: a stack (iterations, B, 1, h, w) in one launch
    got5 = ops.resize_nearest_scaled(u.reshape(n, 1, 1, h, w), (H, W), mul)
    assert tuple(got5.shape) == (n, 1, 1, H, W) and _same_bits(got5.reshape(n, 1, H, W), exp)


def test_a_non_integer_ratio_is_refused():
    from nndepth_amd import ops
    from nndepth_amd._lib import NndError
    u = torch.zeros((1, 1, 4, 6), device=DEV)
    with pytest.raises(NndError, match="integer ratio"):
        ops.resize_nearest_scaled(u, (8, 9), 1.5)
    with pytest.raises(NndError, match="integer ratio"):
        ops.resize_nearest_scaled(u, (6, 12), 2.0)


@pytest.fixture(scope="module")
def c2f():
    """The Coarse2Fine double on a seeded 384x512 pair.  Its encoder side is PyTorch convolutions, which on this backend are not
    run-to-run identical (tests/test_gpu_fp16_models.py); the cascade starts behind them, so the features of the pair are computed
    once and every forward of this file refines the same tensors."""
    from c2f_double import make_c2f
    from nndepth_amd.raft_stereo import Coarse2FineRAFTStereoBase
    cpu, dev = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    torch.manual_seed(3)
    m = make_c2f(Coarse2FineRAFTStereoBase, corr_levels=1, iters=2)
    torch.set_rng_state(cpu)  # the constructors drew from the global generators: later tests see the state they would see without this
    torch.cuda.set_rng_state(dev, DEV)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(4)
    left, right = torch.rand((1, 3, 384, 512), generator=g).to(DEV), torch.rand((1, 3, 384, 512), generator=g).to(DEV)
    memo, real = {}, m.forward_features
    m.forward_features = lambda f1, f2: memo.setdefault("features", real(f1, f2))
    return m, left, right


@pytest.mark.parametrize("outputs", ["all", "last"])
def test_cascade_outputs_do_not_depend_on_who_resizes(c2f, outputs, monkeypatch):
    m, left, right = c2f
    m.outputs = outputs
    try:
        hip = [o["up_disp"].clone() for o in m(left, right)]
        monkeypatch.setenv("NND_C2F_TORCH_RESIZE", "1")
        ref = [o["up_disp"].clone() for o in m(left, right)]
        monkeypatch.delenv("NND_C2F_TORCH_RESIZE")
    finally:
        m.outputs = "all"
    assert len(hip) == len(ref) == (6 if outputs == "all" else 1)
    assert all(tuple(u.shape) == (1, 1, 384, 512) and torch.isfinite(u).all() for u in hip)
    assert all(_same_bits(a, b) for a, b in zip(hip, ref))


def test_default_cascade_never_calls_interpolate(c2f, monkeypatch):
    """Behind the encoder side no call reaches torch.nn.functional.interpolate; with NND_C2F_TORCH_RESIZE=1 it does (the patch bites)."""
    m, left, right = c2f
    feats, cnets = m.forward_features(left, right)

    def refuse(*a, **k):
        raise AssertionError("torch.nn.functional.interpolate called inside refine_stages")

    monkeypatch.setattr(torch.nn.functional, "interpolate", refuse)
    with torch.no_grad():
        outs = m.refine_stages(feats, cnets, (384, 512))
        assert len(outs) == 6 and all(tuple(o["up_disp"].shape) == (1, 1, 384, 512) for o in outs)
        monkeypatch.setenv("NND_C2F_TORCH_RESIZE", "1")
        with pytest.raises(AssertionError, match="interpolate called"):
            m.refine_stages(feats, cnets, (384, 512))
