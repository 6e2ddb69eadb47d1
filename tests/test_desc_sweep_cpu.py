"""CPU: the descriptor sweep's case table and float64 composition (tests/desc_sweep_cases.py) — the restated lookups return the
oracle's bits in float32, the fp32 oracle itself stays within 5e-5 of the float64 composition on every case and run (so the 1e-4
assertions of tests/test_gpu_desc_sweep.py measure the kernels, not the reference), and the table reaches what it claims."""
import os

import pytest
import torch

import desc_sweep_cases as S
from conftest import GOLD

REPORT = os.path.join(GOLD, "REPORT_desc_sweep.txt")
IDS = [c["name"] for c in S.CASES]


@pytest.fixture(scope="module")
def fp32_runs():
    with torch.no_grad():
        return {(c["name"], run): S.compose(c, torch.float32, run) for c in S.CASES + S.LARGE_HIDDEN for run in S.RUNS}


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_restated_lookups_equal_the_oracles_bit_for_bit(fp32_runs, case):
    x = S.inputs(case)
    pyr = S.build_pyramids(case, x)
    for run in S.RUNS:
        states = fp32_runs[(case["name"], run)]["states"]
        assert len(states) == S.ITERS
        for it, state in enumerate(states):
            got, exp = S.lookup(case, pyr, x, state, it), S.oracle_lookup(case, pyr, x, state, it)
            assert got.dtype == exp.dtype == torch.float32 and got.shape == (S.B, S.cor_planes(case), S.H, S.W)
            assert torch.equal(got, exp), (run, it)
        if run == "wide" and case["loop"] != "cre":  # every level samples beyond both borders
            c0 = states[0]
            assert c0.min() < -case["radius"] and c0.max() > S.W - 1 + case["radius"]


def test_fp32_oracle_drift_from_float64(fp32_runs):
    """The reference alone: |fp32 composition - float64 composition| on the upsampled maps (all iterations), the final low-resolution
    state and the hidden state, per case and run; written to the report, each map figure below 5e-5."""
    lines, worst = [], {}
    for c in S.CASES + S.LARGE_HIDDEN:
        for run in S.RUNS:
            a, r = fp32_runs[(c["name"], run)], S.reference(c, run)
            e_up = max((u.double() - v).abs().max().item() for u, v in zip(a["ups"], r["ups"]))
            e_low = (a["low"].double() - r["low"]).abs().max().item()
            e_net = (a["net"].double() - r["net"]).abs().max().item()
            up_max = max(v.abs().max().item() for v in r["ups"])
            worst[(c["name"], run)] = e_up
            lines.append(f"{c['name']:<11} {run:<5} {e_up:.2e}   low {e_low:.2e}   net {e_net:.2e}   |up| max {up_max:7.2f}   |low| max "
                         f"{r['low'].abs().max().item():6.2f}\n")
    old = open(REPORT).read() if os.path.exists(REPORT) else ""
    try:  # this block of the report; the GPU block behind it stays
        with open(REPORT, "w") as f:
            f.write(S.report_join("".join(lines), S.report_split(old)[1]))
    except OSError:
        pass  # a read-only checkout: the figures are printed
    print("\n" + "".join(lines))
    assert S.oracle_drift("".join(lines)) == {k: float(f"{v:.2e}") for k, v in worst.items()}  # the GPU test reads these back
    bad = {k: v for k, v in worst.items() if not v < 5e-5}
    assert not bad, bad


def test_wide_run_reaches_large_values():
    for c in S.CASES:
        r = S.reference(c, "wide")
        assert max(u.abs().max().item() for u in r["ups"]) > 0.8 * c["rate"] * S.W / 2, c["name"]
        assert all(torch.isfinite(u).all() for u in r["ups"])
    for c in S.CASES:  # generated weights keep the update small: from zero the state stays near its start
        if c["loop"] != "igev":
            assert S.reference(c, "zero")["low"].abs().max().item() < 1.5, c["name"]


def test_table_reaches_what_it_claims():
    names = [c["name"] for c in S.CASES]
    assert len(set(names)) == len(names) >= 15
    planes = {S.cor_planes(c) for c in S.CASES}
    assert {27, 14, 5, 44, 21, 28, 36, 162, 288, 336, 56} <= planes
    assert any(p % 2 == 1 for p in planes) and any(p < 32 for p in planes) and any(p > 64 for p in planes)
    assert any(p % 16 != 0 and p > 64 for p in planes)  # a partial last chunk behind whole ones
    assert {c["hid"] for c in S.CASES} >= {32, 64, 96, 128, 160}
    assert {(c["gru"], c["rate"]) for c in S.CASES} >= {(g, r) for g in ("sep_conv", "conv_gru") for r in (4, 8)}
    assert 232 in {S.gru_cin(c) for c in S.CASES}
    assert {c["fc"] for c in S.CASES} == {1, 2} and {c["loop"] for c in S.CASES} == {"raft", "cre", "igev", "group"}
    assert {c["fc"] for c in S.CASES if c["hid"] == 64 and c["rate"] == 8} == {1, 2}  # launch_mu<8,128> with either flow
    for c in S.CASES:
        assert c["hid"] % 32 == 0 and c["ctx"] % 8 == 0
        assert (c["up"] == "fused") == (2 * c["hid"] in (128, 256) and c["rate"] in (4, 8)), c["name"]
        if c["loop"] == "cre":
            assert c["fc"] == 2 and c["C"] % 4 == 0
        if c["loop"] == "group":
            assert c["groups"] ** 2 <= c["C"]
        if c["loop"] in ("raft", "igev", "group"):
            assert S.W >> (c["levels"] - 1) >= 2  # the coarsest level read still has two entries
    # Cout of encoder.conv (hid - fc) ragged against the 32-channel blocks: 31, 95, 159 and, with two flow channels, 62 / 126
    assert {c["hid"] - c["fc"] for c in S.CASES} >= {31, 95, 159, 62, 126}


def test_block_kwargs_build_the_drop_in_module_and_take_the_generated_weights():
    from nndepth_amd.blocks import BasicUpdateBlock
    for c in S.CASES:
        ub = BasicUpdateBlock(**S.block_kwargs(c))
        ub.load_state_dict(S.state_dict(c, strip=True), strict=True)
        assert ub.engine.desc.cor_planes == S.cor_planes(c) and ub.engine.desc.mask_channels == 9 * c["rate"] ** 2


def test_hidden_dim_beyond_flow_head_conv2_is_refused_when_the_engine_is_built():
    """flow_head.conv2 stages all hidden channels of a tile's halo in LDS (64 KB): a descriptor beyond that is refused by the plan, by
    name — not by that launch after half an iteration was enqueued.  192 with one flow channel is the largest that fits."""
    from nndepth_amd._lib import NndError
    from nndepth_amd.blocks import BasicUpdateBlock
    for hid, fc, ok in ((192, 1, True), (160, 2, True), (224, 1, False), (256, 1, False), (192, 2, False)):
        kw = dict(hidden_dim=hid, cor_planes=36, context_dim=64, flow_channel=fc, spatial_scale=8)
        if ok:
            BasicUpdateBlock(**kw)
        else:
            with pytest.raises(NndError, match="hidden_dim"):
                BasicUpdateBlock(**kw)
