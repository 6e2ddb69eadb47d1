"""GPU: the model classes in the one-piece fp16 arithmetic ("fp16", csrc/split_arith.h).

1. BaseRAFTStereo against the reference itself (tests/golden/fp16_raft*.npz, scripts/make_golden_fp16.py: the TartanAir pair at
   64x128 / 12 iterations and 96x160 / 8 iterations, the imported reference's fp32 up_disp per iteration and its CPU bf16-autocast
   up_disp — the arithmetic its trainers validate with): on every iteration the HIP model's mean-abs deviation from the reference's
   fp32 map is at most 0.5 x the recorded fp32-to-autocast deviation (the float64 emulation of the contract gives a ratio of 0.03).
2. The four model classes on the smallest shapes of tests/test_gpu_models_smoke.py: outputs="last" is the last of "all" bit for bit,
   GraphedForward equals the direct launches, two forwards are bit-identical, the outputs are finite, activation_ranges() is
   populated by the first forward (auto-calibration), and the model's "fp16x2" result does not change by "fp16" having run in the
   process."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLD, t
from fp16_report import report_section

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARK = "== models (tests/test_gpu_fp16_models.py)\n"
_lines = {}


@pytest.fixture(autouse=True)
def _keep_global_rng():
    """The module constructors draw their initial parameters from torch's global generators; tests that run later in the same process
    and draw from them (tests/test_gpu_last_only.py) must see the state they would see without this file."""
    cpu, dev = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    yield
    torch.set_rng_state(cpu)
    torch.cuda.set_rng_state(dev, DEV)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _lines:
        report_section(MARK, [_lines[k] for k in sorted(_lines)])


@pytest.mark.parametrize("key,npz", [("64x128", "fp16_raft.npz"), ("96x160", "fp16_raft_96x160.npz")])
def test_raft_stereo_within_half_the_autocast_deviation(raft_sd, key, npz):
    from nndepth_amd.raft_stereo import BaseRAFTStereo
    g = dict(np.load(os.path.join(GOLD, npz)))
    frames, ref, dev = t(g["frames_" + key]), t(g["fp32_" + key]), g["dev_" + key]
    iters = ref.shape[0]
    assert np.allclose(dev, (t(g["bf16_" + key]) - ref).abs().mean(dim=(1, 2)).numpy(), rtol=1e-5)  # the fixture is consistent
    f1, f2 = frames[:1].to(DEV), frames[1:].to(DEV)
    got = {}
    for arith in ("fp16", "fp16x2"):
        m = BaseRAFTStereo(iters=iters, context_dim=64, arithmetic=arith)
        m.load_state_dict(raft_sd, strict=True)
        m = m.to(DEV).eval()
        outs = m(f1, f2)  # the first forward calibrates on this pair
        assert len(outs) == iters and m.activation_ranges()
        ups = torch.stack([o["up_disp"][0, 0] for o in outs]).cpu()
        assert torch.isfinite(ups).all()
        got[arith] = (ups - ref).abs().mean(dim=(1, 2)).numpy()
    ratio = got["fp16"] / dev
    txt = (f"BaseRAFTStereo {key}, {iters} iterations, mean-abs deviation from the reference's fp32 up_disp per iteration\n"
           f"    reference under bf16 autocast  " + " ".join(f"{d:.2e}" for d in dev) + "\n"
           f"    HIP fp16                       " + " ".join(f"{d:.2e}" for d in got["fp16"]) + "\n"
           f"    ratio (gate 0.5)               " + " ".join(f"{d:8.3f}" for d in ratio) + "\n"
           f"    HIP fp16x2 (for comparison)    " + " ".join(f"{d:.2e}" for d in got["fp16x2"]) + "\n")
    print("\n" + txt, end="")
    _lines[(0, key)] = txt
    assert (ratio <= 0.5).all(), txt


def _raft(arith):
    from nndepth_amd.raft_stereo import BaseRAFTStereo
    return BaseRAFTStereo(iters=4, arithmetic=arith), (480, 640)


def _cre(arith):
    from nndepth_amd.cre_stereo import CREStereoBase
    return CREStereoBase(iters=2, arithmetic=arith), (480, 640)


def _igev(arith):
    from igev_double import make_igev
    from nndepth_amd.igev_stereo import CostVolumeFilterNetwork, IGEVStereoBase
    return make_igev(IGEVStereoBase, CostVolumeFilterNetwork, iters=4, arithmetic=arith), (480, 640)


def _c2f(arith):
    from c2f_double import make_c2f
    from nndepth_amd.raft_stereo import Coarse2FineRAFTStereoBase
    return make_c2f(Coarse2FineRAFTStereoBase, corr_levels=1, iters=2, arithmetic=arith), (384, 512)


MAKERS = {"raft": _raft, "cre": _cre, "igev": _igev, "c2f": _c2f}


def _ups(outs):
    return [o["up_disp"].clone() for o in outs]


@pytest.mark.parametrize("family", list(MAKERS))
def test_model_class_in_one_piece(family):
    from nndepth_amd.graph import GraphedForward
    make = MAKERS[family]
    torch.manual_seed(0)
    proto, hw = make("fp16x2")
    sd = {k: v.clone() for k, v in proto.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    left, right = torch.rand((1, 3) + hw, generator=g).to(DEV), torch.rand((1, 3) + hw, generator=g).to(DEV)

    memo = {}

    def build(arith):
        m, _ = make(arith)
        m.load_state_dict(sd, strict=True)
        m = m.to(DEV).eval()
        if family == "c2f":
            # the double's encoder side is PyTorch convolutions, and on this backend those are not run-to-run identical (measured: the
            # feature maps differ between two calls in every arithmetic, fp32 included); the HIP path starts behind them, so the
            # features of this pair are computed once and every model of the test refines the same tensors
            real = m.forward_features
            m.forward_features = lambda f1, f2: memo.setdefault("features", real(f1, f2))
        return m

    before = _ups(build("fp16x2")(left, right))  # fp16x2 before anything ran in one piece
    m = build("fp16")
    assert m.activation_ranges() == {} or set(m.activation_ranges().values()) == {65504.0 / 4}  # not packed yet, or the default scales
    full = _ups(m(left, right))
    ranges = m.activation_ranges()
    assert ranges and len(set(ranges.values())) > 1 and m.update_block.engine.calibrated, ranges  # populated by the first forward
    assert all(torch.isfinite(u).all() for u in full)
    again = _ups(m(left, right))
    assert len(again) == len(full) and all(torch.equal(a, b) for a, b in zip(full, again)), "two forwards"
    replay = GraphedForward(m)(left, right)
    assert len(replay) == len(full) and all(torch.equal(a, b["up_disp"]) for a, b in zip(full, replay)), "graph replay"
    m.outputs = "last"
    last = m(left, right)
    assert len(last) == 1 and torch.equal(last[0]["up_disp"], full[-1]), "outputs='last'"
    after = _ups(build("fp16x2")(left, right))
    assert len(after) == len(before) and all(torch.equal(a, b) for a, b in zip(before, after)), "fp16x2 after fp16 ran"
    d = max((a - b).abs().max().item() for a, b in zip(full, before))
    line = f"{family}: {len(full)} maps {tuple(full[-1].shape)}, |up| max {full[-1].abs().max().item():.3g}, max |fp16 - fp16x2| over the maps {d:.2e}\n"
    print("\n" + line, end="")
    _lines[(1, family)] = line
