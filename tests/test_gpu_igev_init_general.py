"""GPU: cv_squeezer + soft-argmin beyond 8 groups / 512 candidates (nnd_igev_init_disparity_dev, igev_squeeze_general_kernel in
csrc/corr1d.hip: the candidate axis walked in chunks, the logits parked in LDS, the squeezer's parameters read from device memory).

Op level: every shape against the reference's ops on the CPU in fp32 (`exp32`: Conv3d on the permuted view, softmax, expectation —
oracle.torch_ref.igev_init_disparity) and in float64 (`exp64`).  Gates:
  (i)  |got - exp32|max <= 2e-5 * D, the bar of tests/test_gpu_parity.py::test_igev_squeezer_init_vs_oracle;
  (ii) |got - exp64|max <= 2 * |exp32 - exp64|max: at most twice the reference's own fp32 distance from the float64 formula.
The chunk length C of the seam cases is the library's own (nnd_igev_init_disparity_chunk() = SQG_C of csrc/corr1d.hip); the seam
cases have 8 groups and at most 2C + 1 candidates, a shape ops.igev_init_disparity hands to the older kernels, so they call the
chunked kernel through ops.igev_init_disparity_general.  Model level: IGEVStereoBase with cv_groups = 16 (and, 8 groups, a
2112-px-wide pair with 528 candidates) runs without the warned PyTorch Conv3d.  The figures of a run go to
tests/golden/REPORT_igev_init.txt."""
import functools
import os
import warnings

import pytest
import torch

from conftest import GOLD

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPORT = os.path.join(GOLD, "REPORT_igev_init.txt")
HEADER = ("cv_squeezer + soft-argmin beyond 8 groups / 512 candidates (tests/test_gpu_igev_init_general.py): max-abs distances of the\n"
          "HIP result from the reference's CPU ops in fp32 (gate 2e-5 * D) and in float64 (gate: 2 x the reference's own fp32-to-float64\n"
          "distance), that distance, the ratio of the two, and the kernel taken.  Shape = (B, G, H, W, D, amplitude of the volume).\n")
_lines = {}

MORE_GROUPS = [(2, 9, 3, 11, 21, 1.0), (1, 16, 4, 9, 40, 1.0), (1, 12, 2, 10, 300, 0.5), (1, 64, 2, 9, 16, 1.0)]
MORE_CANDIDATES = [(1, 8, 3, 9, 513, 1.0), (1, 8, 2, 10, 777, 1.0), (1, 3, 2, 17, 1024, 2.0), (1, 8, 1, 9, 2050, 1.0),
                   (1, 2, 2, 8, 4096, 1.0), (1, 8, 2, 9, 4096, 4.0)]
BOTH = [(1, 16, 3, 9, 600, 1.0)]
# W no multiple of the 8 pixels of a workgroup (13, 10, 5, 3), one image row, more rows than the 8 XCD bands, two samples, a last
# chunk of 4 candidates (516) and of 2 with D % 4 != 0 (130: the scalar staging)
RAGGED = [(1, 9, 1, 13, 40, 1.0), (1, 10, 17, 10, 24, 1.0), (2, 8, 2, 5, 516, 1.0), (1, 9, 3, 3, 130, 1.0)]
SHAPES = MORE_GROUPS + MORE_CANDIDATES + BOTH + RAGGED


def _id(s):
    return "B{}_G{}_{}x{}_D{}_a{}".format(*s)


def _chunk():
    from nndepth_amd._lib import lib
    return int(lib.nnd_igev_init_disparity_chunk())


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if not _lines:
        return
    try:
        with open(REPORT, "w") as f:
            f.write(HEADER + "".join(_lines[k] for k in sorted(_lines)))
    except OSError:
        pass  # a read-only checkout: the figures were printed


@functools.lru_cache(maxsize=None)
def _case(shape, peaks=False):
    """Seeded volume and squeezer with the two CPU references; made once per shape, never modified."""
    from oracle import torch_ref as R
    B, G, H, W, D, amp = shape
    g = torch.Generator().manual_seed(1000 + 7 * G + D + H + (50000 if peaks else 0))
    geo = torch.randn((B, G, H, W, D), generator=g) * amp
    weight = (torch.rand((1, G, 3, 3, 3), generator=g) * 2 - 1) / (27 * G) ** 0.5  # Conv3d's default initial range
    bias = (torch.rand((1,), generator=g) * 2 - 1) / (27 * G) ** 0.5
    if peaks:  # a near-delta softmax at candidate 0 (left columns) / D - 1 (right columns): +30 in every group, no negative weight
        # (the taps beside the centre weigh a quarter of it along the candidate axis and a tenth in the image plane, and the centre
        # taps of the groups add up to 0.65: the peak's logit stands about 20 above the rest — its own place within 1e-4 of the end
        # of the axis — while some 1e-7 of the mass stays on the candidate beside it, so the sums still have small terms to lose)
        weight = weight.abs() * torch.tensor([0.25, 1.0, 0.25]).reshape(1, 1, 3, 1, 1)
        weight = weight * torch.tensor([[0.1, 0.1, 0.1], [0.1, 1.0, 0.1], [0.1, 0.1, 0.1]]).reshape(1, 1, 1, 3, 3)
        weight = weight * (0.65 / weight[0, :, 1, 1, 1].sum())
        geo[:, :, :, :W // 2, 0] += 30.0
        geo[:, :, :, W // 2:, D - 1] += 30.0
    vol = geo.permute(0, 1, 4, 2, 3)
    exp32 = R.igev_init_disparity(torch.nn.functional.conv3d(vol, weight, bias, padding=1).squeeze(1))
    exp64 = R.igev_init_disparity(torch.nn.functional.conv3d(vol.double(), weight.double(), bias.double(), padding=1).squeeze(1))
    return geo, weight, bias, exp32, exp64


def _check(shape, got, kernel, tag, order):
    B, G, H, W, D, amp = shape
    _, _, _, exp32, exp64 = _case(shape, tag == "peaks")
    got = got.cpu()
    assert got.shape == exp32.shape and torch.isfinite(got).all()
    e32 = (got - exp32).abs().max().item()
    e64 = (got.double() - exp64).abs().max().item()
    own = (exp32.double() - exp64).abs().max().item()
    line = (f"{str(shape):<28} {tag:<6} vs fp32 {e32:.2e} (gate {2e-5 * D:.2e})   vs float64 {e64:.2e}   reference's own {own:.2e}   "
            f"ratio {e64 / own if own else float('inf'):.2f} (gate 2)   |out| max {exp64.abs().max().item():.4g}   {kernel}\n")
    print("\n" + line, end="")
    _lines[(order, _id(shape), tag)] = line
    assert e32 <= 2e-5 * D, line
    assert e64 <= 2 * own, line


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_shapes_the_older_kernels_refuse(shape):
    from nndepth_amd import ops
    B, G, H, W, D, _ = shape
    geo, weight, bias, _, _ = _case(shape)
    assert G > 8 or D > 512
    kernel = ops.igev_init_disparity_kernel(B, G, H, W, D)
    assert kernel == "igev_squeeze_general_kernel"
    got = ops.igev_init_disparity(geo.to(DEV), weight.to(DEV), bias.to(DEV), B, G, H, W, D)
    _check(shape, got, kernel, "", SHAPES.index(shape))


@pytest.mark.parametrize("which", ["C-1", "C", "C+1", "2C+1"])
def test_chunk_seams(which):
    """D around the chunk length C (the library's nnd_igev_init_disparity_chunk(), SQG_C in csrc/corr1d.hip) at G = 8, H = 2,
    W = 9, through the chunked kernel's own wrapper (ops.igev_init_disparity hands these shapes to the older kernels)."""
    from nndepth_amd import ops
    C = _chunk()
    assert C >= 16
    D = {"C-1": C - 1, "C": C, "C+1": C + 1, "2C+1": 2 * C + 1}[which]
    shape = (1, 8, 2, 9, D, 1.0)
    geo, weight, bias, _, _ = _case(shape)
    got = ops.igev_init_disparity_general(geo.to(DEV), weight.to(DEV), bias.to(DEV), 1, 8, 2, 9, D)
    _check(shape, got, "igev_squeeze_general_kernel", "seam", 100)


@pytest.mark.parametrize("D", [600, 2050])
def test_peaks_at_the_ends_of_the_candidate_axis(D):
    """A near-delta softmax at candidate 0 or D - 1: a zero pad or halo put at a chunk seam instead of the ends of the axis moves it."""
    from nndepth_amd import ops
    shape = (1, 8, 2, 9, D, 1.0)
    geo, weight, bias, exp32, _ = _case(shape, True)
    got = ops.igev_init_disparity(geo.to(DEV), weight.to(DEV), bias.to(DEV), 1, 8, 2, 9, D)
    _check(shape, got, "igev_squeeze_general_kernel", "peaks", 200)
    got, left = got.cpu()[0, 0], 9 // 2
    assert got[:, :left].abs().max() <= 1.0 and (got[:, left:] + (D - 1)).abs().max() <= 1.0, got
    assert exp32[0, 0][:, :left].abs().max() <= 1.0 and (exp32[0, 0][:, left:] + (D - 1)).abs().max() <= 1.0  # the fixture does what it says


def test_unchanged_shapes_keep_their_kernels(monkeypatch, capfd):
    """(1, 8, 5, 13, 300) and (1, 8, 19, 61, 256) still run the older kernels.  NND_DEBUG_SYNC names the update block's launches only,
    so the record is the library's own dispatch query, which nnd_igev_init_disparity's branch shares (squeeze_takes_walk)."""
    from nndepth_amd import ops
    from nndepth_amd._lib import lib
    monkeypatch.setenv("NND_DEBUG_SYNC", "1")
    for (B, G, H, W, D), want in (((1, 8, 5, 13, 300), "igev_squeeze_softargmin_kernel"), ((1, 8, 19, 61, 256), "igev_squeeze_softargmin_kernel")):
        geo, weight, bias, exp32, _ = _case((B, G, H, W, D, 1.0))
        got = ops.igev_init_disparity(geo.to(DEV), weight, bias, B, G, H, W, D).cpu()
        assert (got - exp32).abs().max() <= 2e-5 * D
        assert ops.igev_init_disparity_kernel(B, G, H, W, D) == want
        assert ops.igev_init_disparity_host_params(G, D)
    torch.cuda.synchronize()
    assert "general" not in capfd.readouterr().err
    monkeypatch.delenv("NND_DEBUG_SYNC")
    monkeypatch.setenv("NND_IGEV_SQUEEZE_WALK", "1")
    assert ops.igev_init_disparity_kernel(1, 8, 19, 61, 256) == "igev_squeeze_walk_kernel"
    assert ops.igev_init_disparity_kernel(1, 8, 5, 13, 300) == "igev_squeeze_softargmin_kernel"  # D > 256: never the walking kernel
    monkeypatch.delenv("NND_IGEV_SQUEEZE_WALK")
    assert ops.igev_init_disparity_kernel(1, 8, 136, 240, 240) == "igev_squeeze_walk_kernel"  # the size that fills the chip
    for (G, D), want in (((8, 512), True), ((9, 21), True), ((64, 4096), True), ((65, 16), False), ((8, 4097), False)):
        assert ops.igev_init_disparity_supported(G, D) is want
        assert bool(lib.nnd_igev_init_disparity_supported(G, D)) is want


def test_two_runs_are_bit_identical():
    from nndepth_amd import ops
    shape = (1, 16, 3, 9, 600, 1.0)
    geo, weight, bias, _, _ = _case(shape)
    geo, weight, bias = geo.to(DEV), weight.to(DEV), bias.to(DEV)
    a = ops.igev_init_disparity(geo, weight, bias, 1, 16, 3, 9, 600)
    junk = torch.full((1 << 20,), float("nan"), device=DEV)  # whatever the allocator hands out next held something else
    del junk
    b = ops.igev_init_disparity(geo, weight, bias, 1, 16, 3, 9, 600)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ model level
def _model(cv_groups, hw, seed):
    from igev_double import make_igev
    from nndepth_amd.igev_stereo import CostVolumeFilterNetwork, IGEVStereoBase
    cpu, dev = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    torch.manual_seed(seed)
    # 2 levels at 8 groups and 1 level at 16: 288 correlation planes either way, inside the range tests/desc_sweep_cases.py sweeps
    m = make_igev(IGEVStereoBase, CostVolumeFilterNetwork, cv_groups=cv_groups, hidden_dim=64, context_dim=64,
                  corr_levels=2 if cv_groups <= 8 else 1, iters=2)
    if cv_groups * cv_groups > 2 * 64:
        # the volume correlates the first cv_groups chunks of cv_groups feature channels: the double's 2 * hidden_dim = 128 channels
        # are too few for 16 groups, so its feature projection (tied to hidden_dim by nothing downstream) gets cv_groups^2 = 256
        m.fnet_proj = torch.nn.Sequential(torch.nn.Conv2d(24, cv_groups * cv_groups, 3, 1, 1), torch.nn.ReLU(False))
    torch.set_rng_state(cpu)  # the constructors drew from the global generators: later tests see the state they would see without this
    torch.cuda.set_rng_state(dev, DEV)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(seed + 1)
    left, right = torch.rand((1, 3) + hw, generator=g).to(DEV), torch.rand((1, 3) + hw, generator=g).to(DEV)
    # the double's backbone is PyTorch convolutions, which on this backend are not run-to-run identical (tests/test_gpu_fp16_models.py);
    # the code under test starts behind them: the features of the pair are computed once and every forward refines the same tensors
    memo, real = {}, m.forward_fnet
    m.forward_fnet = lambda f1, f2: memo.setdefault("features", real(f1, f2))
    return m, left, right


def _ups(outs):
    return [o["up_disp"].clone() for o in outs]


def _model_checks(cv_groups, hw, seed, monkeypatch):
    from nndepth_amd import ops
    from nndepth_amd.graph import GraphedForward
    m, left, right = _model(cv_groups, hw, seed)
    calls = []
    hook = m.cv_squeezer.register_forward_hook(lambda *a: calls.append(1))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        first = _ups(m(left, right))
        second = _ups(m(left, right))
    assert not [w for w in caught if issubclass(w.category, RuntimeWarning)], [str(w.message) for w in caught]
    assert calls == [], "the squeezer's PyTorch Conv3d ran"
    assert len(first) == 2 and all(torch.isfinite(u).all() for u in first)
    assert all(torch.equal(a, b) for a, b in zip(first, second)), "two forwards"
    replay = _ups(GraphedForward(m)(left, right))
    assert all(torch.equal(a, b) for a, b in zip(first, replay)), "graph replay"
    assert calls == []
    # today's path, to prove that the switch switches: the library's answer replaced by "unsupported"
    monkeypatch.setattr(ops, "igev_init_disparity_supported", lambda G, D: False)
    with pytest.warns(RuntimeWarning, match="squeezer Conv3d runs on PyTorch-ROCm"):
        fallback = _ups(m(left, right))
    assert calls == [1]
    hook.remove()
    d = max((a - b).abs().max().item() for a, b in zip(first, fallback))
    print(f"\n[cv_groups {cv_groups}, {hw[0]}x{hw[1]}] fused init vs PyTorch-ROCm Conv3d + soft-argmin, final maps: max-abs {d:.2e}", end="")
    assert all(torch.isfinite(u).all() for u in fallback)


def test_model_with_sixteen_groups_stays_on_hip(monkeypatch):
    """IGEVStereoBase(cv_groups=16) on a 96x128 pair (24x32 at 1/4, 32 candidates): no warning, no call of cv_squeezer, finite,
    repeatable, graph-capturable; with the support query forced to False the warned PyTorch Conv3d runs once.
    16, not 9, groups: nine cannot reach the squeezer in this project or in the reference — 128 feature channels do not divide by 9
    (the volume's assertion, igev_stereo/cost_volume.py:82-84 of the reference), and with 144 channels the HIP regulariser refuses
    its 36-channel concat layer ("(J+2)*Cin0 % 16 == 0", csrc/conv3d.hip).  16 is the smallest group count above 8 that the volume
    and the regulariser both build; the op-level cases above cover 9, 10, 12 and 64 groups."""
    _model_checks(16, (96, 128), 31, monkeypatch)


def test_model_on_a_2112_px_wide_pair_stays_on_hip(monkeypatch):
    """8 groups, 64x2112 (16x528 at 1/4: 528 candidates, a 143 MB volume) — a width the older kernels refuse."""
    _model_checks(8, (64, 2112), 33, monkeypatch)
