"""GPU: the four refinement loops in the one-piece fp16 arithmetic ("fp16", csrc/split_arith.h) over the descriptor sweep's table
(tests/desc_sweep_cases.py: 15 cases, both runs, 3 iterations), after calibration on the very input.

The mode is not an fp32-parity arithmetic; what it promises is to stay well inside the arithmetic the reference's checkpoints are
validated with (torch.amp.autocast(dtype=bfloat16): an 8-bit significand on both operands of every convolution).  So the yardstick
is that arithmetic, emulated: `compose(c, float64, run)` with oracle.torch_ref._conv rounding both operands to bfloat16; its
mean-abs deviation from the float64 composition, per upsampled map, is d_bf16.  Gate: each kernel map's mean-abs deviation from the
float64 composition is at most 0.5 * d_bf16 of the same map.  Why 0.5: three more significand bits predict 1/8; the float64
emulation of this contract (both operands of every conv rounded to one fp16 piece of a power-of-two-scaled value) gives 0.06 to
0.36 on these 30 runs, so the contract alone stays inside the cap with 1.4 x to spare, and passing still proves the mode strictly
better than what the reference validates with.  Max-abs ratios are printed to tests/golden/REPORT_fp16.txt, not gated."""
import functools
import re

import pytest
import torch

import desc_sweep_cases as S
from fp16_report import report_section
from test_gpu_fp16_conv import _bf16_conv, split_lines

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARK = "== loops (tests/test_gpu_fp16_loops.py)\n"
IDS = [c["name"] for c in S.CASES]
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
        head = ("case        run    per iteration: mean-abs deviation of the fp16 maps from float64 / of the bf16-emulated maps (ratio; gate 0.5) "
                "| max-abs ratio (not gated)\n")
        report_section(MARK, [head] + [_lines[k] for k in sorted(_lines)])


@functools.lru_cache(maxsize=None)
def _bf16_emulation(name, run):
    """The case's loop in float64 with the operands of every convolution rounded to bfloat16; computed once, not modified."""
    from oracle import torch_ref as R
    real = R._conv
    R._conv = _bf16_conv
    try:
        with torch.no_grad():
            return S.compose(S.BY_NAME[name], torch.float64, run)
    finally:
        R._conv = real


def _make_block(case, arith="fp16"):
    from nndepth_amd.blocks import BasicUpdateBlock
    ub = BasicUpdateBlock(**S.block_kwargs(case), arithmetic=arith)
    ub.load_state_dict(S.state_dict(case, strip=True), strict=True)
    return ub.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _dev_inputs(name):
    from nndepth_amd import ops
    c = S.BY_NAME[name]
    x = {k: v.to(DEV) for k, v in S.inputs(c).items()}
    L, G = c["levels"], c["groups"]
    if c["loop"] == "raft":
        x["pyr"] = ops.corr1d_build(x["f1"], x["f2"], L)
    elif c["loop"] == "group":
        x["pyr"] = ops.raft_group_corr_build(x["f1"], x["f2"], G, L)
    elif c["loop"] == "igev":
        rows = S.B * G * S.H * S.W
        x["fp"] = ops.pyramid_from_level0(x["feat"].reshape(rows, S.W), S.B * G, S.H, S.W, L)
        x["gp"] = ops.pyramid_from_level0(x["geo"].permute(0, 1, 3, 4, 2).reshape(rows, S.W), S.B * G, S.H, S.W, L)
        x["il"] = ops.igev_interleave_pyramids(x["fp"], x["gp"], S.B, G, S.H, S.W, L)
    return x


def _refine(eng, case, run, iters=S.ITERS, **kw):
    x = _dev_inputs(case["name"])
    init = S.init_of(case, run, x)
    L, r, G, rate = case["levels"], case["radius"], case["groups"], case["rate"]
    if case["loop"] == "raft":
        return eng.refine(x["pyr"], L, r, x["net"], x["inp"], rate, iters, disp_init=init, **kw)
    if case["loop"] == "group":
        return eng.refine_group(x["pyr"], G, L, r, x["net"], x["inp"], rate, iters, disp_init=init, **kw)
    if case["loop"] == "igev":
        return eng.refine_igev(x["fp"], x["gp"], G, L, r, x["net"], x["inp"], rate, iters, disp_init=init, interleaved=x["il"], **kw)
    return eng.refine_cre(x["f1"], x["f2"], x["net"], x["inp"], rate, iters, flow_init=init, **kw)


def _engine(case, run):
    from nndepth_amd.raft_stereo import calibration_passes
    eng = _make_block(case).sync_engine(DEV)
    calibration_passes(lambda: _refine(eng, case, run), 4, f"{case['name']}: activations still overflow fp16 after 4 passes")
    assert eng.calibrated
    return eng


@pytest.mark.parametrize("run", S.RUNS)
@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_fused_loop_within_half_the_bf16_deviation(case, run):
    ref, emu = S.reference(case, run), _bf16_emulation(case["name"], run)
    eng = _engine(case, run)
    up, low, net = (t.clone() for t in _refine(eng, case, run))
    assert up.shape[0] == S.ITERS and torch.isfinite(up).all() and torch.isfinite(low).all() and torch.isfinite(net).all()
    up2 = _refine(eng, case, run)[0]
    assert torch.equal(up, up2), "run to run"
    last = _refine(eng, case, run, last_only=True)[0]
    assert last.shape[0] == 1 and torch.equal(last[0], up[-1]), "last_only is the last map of the all-outputs call, bit for bit"
    upd = up.cpu().double()
    fields, ok = [], True
    for i in range(S.ITERS):
        d16, dbf = (upd[i] - ref["ups"][i]).abs(), (emu["ups"][i] - ref["ups"][i]).abs()
        ratio, mratio = d16.mean().item() / dbf.mean().item(), d16.max().item() / dbf.max().item()
        fields.append(f"{d16.mean().item():.2e} / {dbf.mean().item():.2e} ({ratio:.3f}) | {mratio:.3f}")
        ok = ok and ratio <= 0.5
    line = f"{case['name']:<11} {run:<5}  " + "   ".join(fields) + "\n"
    print("\n" + line, end="")
    _lines[(IDS.index(case["name"]), S.RUNS.index(run))] = line
    assert ok, line


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_the_one_piece_launches_claimed_are_the_ones_run(case, monkeypatch, capfd):
    """From NND_DEBUG_SYNC's trace and the NND_CONV_VERBOSE plan lines: every conv_split launch of the loop carries one piece, and the
    fused launches are those of the range-scaled fp16 arithmetics — the flow branch in one launch (merged with lookup + convc1 on a
    RAFT-Stereo pyramid), mask.2 inside the upsample kernel with the folded flow head where 2 * hid is 128 or 256, else mask.2 as
    a one-piece conv in front of the convex upsample."""
    from test_gpu_desc_sweep import _expected_launches
    iters = 2
    eng = _engine(case, "zero")
    torch.cuda.synchronize()
    capfd.readouterr()
    monkeypatch.setenv("NND_DEBUG_SYNC", "1")
    monkeypatch.setenv("NND_CONV_VERBOSE", "1")
    _refine(eng, case, "zero", iters)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    names = re.findall(r"\[nnd\] (.*?) \.\.\. ok", err)
    want, never = _expected_launches(case, "fp16x2")  # the launch structure of fp16x2: the two arithmetics share every predicate
    for name, per_iter in want.items():
        assert names.count(name) == per_iter * iters, (name, names)
    for name in never:
        assert names.count(name) == 0, (name, names)
    lines = split_lines(err)
    assert lines and all(L["pieces"] == 1 for L in lines), lines
    shapes = {(L["KH"], L["KW"], L["Cin"], L["Cout"]) for L in lines}
    assert (3, 3, 256, 192) in shapes and (3, 3, case["hid"], 3 * case["hid"]) in shapes, shapes  # convc2, flow_head.conv1 + mask.0
    if case["up"] == "unfused":
        assert (1, 1, 2 * case["hid"], 9 * case["rate"] ** 2) in shapes, shapes  # mask.2 as a one-piece conv
    ranges = eng.activation_ranges()
    assert "encoder.convf2" in ranges and "mask.2" in ranges and all(0 < v < float("inf") for v in ranges.values()), ranges


@pytest.mark.parametrize("name", ["h64_r8", "h128_f2_c8", "ig_l2", "grp_g8", "h96"])
def test_calibration_does_not_depend_on_last_only(name):
    """A call with NND_FLAG_CALIBRATE runs the all-outputs schedule whatever NND_FLAG_LAST_UPSAMPLE_ONLY says (the mask head records
    its range in every iteration): the scales it leaves are the same."""
    from nndepth_amd import ops
    case = S.BY_NAME[name]
    got = []
    for last_only in (False, True):
        eng = _make_block(case).sync_engine(DEV)
        with ops.calibration() as c:
            _refine(eng, case, "wide", last_only=last_only)
        assert not (c.status & 1) and eng.calibrated  # (bit 1: a layer of the blob is not on this loop's path — the single-call GRU convs)
        got.append((eng.activation_ranges(), eng.packed.clone()))
    assert got[0][0] == got[1][0] and torch.equal(got[0][1], got[1][1])
    assert len(set(got[0][0].values())) > 1  # calibrated: not the default scale everywhere
