"""GPU: the update-block descriptor sweep (tests/desc_sweep_cases.py) — every case of the table in the three arithmetics against
the float64 composition of its loop: one application of the block, the fused loop from zero and from a large initial state, the
launches the case claims to reach (read from NND_DEBUG_SYNC's trace), each fused launch against its NND_NO_* switch, the
descriptors that must be refused when the engine is built, and BaseRAFTStereo with non-default dimensions through the HIP encoder.
The fp32 oracle's own drift from float64 (tests/golden/REPORT_desc_sweep.txt, written by tests/test_desc_sweep_cpu.py) is printed
beside every figure."""
import functools
import os
import re

import pytest
import torch

import desc_sweep_cases as S
from conftest import GOLD

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPORT = os.path.join(GOLD, "REPORT_desc_sweep.txt")
IDS = [c["name"] for c in S.CASES]
_figures = {}  # (case, arith, run) -> report line


def _make_block(case, arith):
    from nndepth_amd.blocks import BasicUpdateBlock
    ub = BasicUpdateBlock(**S.block_kwargs(case), arithmetic=arith)
    ub.load_state_dict(S.state_dict(case, strip=True), strict=True)
    return ub.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _dev_inputs(name):
    """The case's inputs on the device and its pyramid(s) built there; made once, never modified."""
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
        x["il"] = ops.igev_interleave_pyramids(x["fp"], x["gp"], S.B, G, S.H, S.W, L)  # as IGEVStereoBase hands it over
    return x


def _refine(eng, case, run, iters=S.ITERS):
    """The case's fused loop through the engine's own entry point -> (up (iters, B, fc, rate*H, rate*W), low, net)."""
    x = _dev_inputs(case["name"])
    init = S.init_of(case, run, x)
    L, r, G, rate = case["levels"], case["radius"], case["groups"], case["rate"]
    if case["loop"] == "raft":
        return eng.refine(x["pyr"], L, r, x["net"], x["inp"], rate, iters, disp_init=init)
    if case["loop"] == "group":
        return eng.refine_group(x["pyr"], G, L, r, x["net"], x["inp"], rate, iters, disp_init=init)
    if case["loop"] == "igev":
        return eng.refine_igev(x["fp"], x["gp"], G, L, r, x["net"], x["inp"], rate, iters, disp_init=init, interleaved=x["il"])
    return eng.refine_cre(x["f1"], x["f2"], x["net"], x["inp"], rate, iters, flow_init=init)


def _calibrate(arith, run_once, what):
    """fp16x2: the activation scales from this very input, as the model classes do on their first forward."""
    if arith == "fp16x2":
        from nndepth_amd.raft_stereo import calibration_passes
        calibration_passes(run_once, 4, f"{what}: activations still overflow fp16 after 4 passes")


def _engine(case, arith, run="wide"):
    eng = _make_block(case, arith).sync_engine(DEV)
    _calibrate(arith, lambda: _refine(eng, case, run), case["name"])
    return eng


def _drift():
    return S.oracle_drift(S.report_split(open(REPORT).read())[0]) if os.path.exists(REPORT) else {}


@pytest.fixture(scope="module", autouse=True)
def _gpu_report():
    """The GPU figures of this run appended to the report (behind the CPU block, replacing an earlier GPU block)."""
    yield
    if not _figures:
        return
    lines = "".join(_figures[k] for k in sorted(_figures, key=lambda k: (IDS.index(k[0]) if k[0] in IDS else 99, S.ARITHS.index(k[1]), k[2])))
    try:
        cpu = S.report_split(open(REPORT).read())[0] if os.path.exists(REPORT) else ""
        with open(REPORT, "w") as f:
            f.write(S.report_join(cpu, lines))
    except OSError:
        pass  # a read-only checkout: the figures were printed


def _check_loop(case, arith, run, got):
    """Every iteration's map and the final low-resolution state within 1e-4 (the project's parity bar), the hidden state within
    5e-5 (test_update_block_conv_gru_vs_oracle's), against float64."""
    up, low, net = (t.cpu().double() for t in got)
    ref = S.reference(case, run)
    assert up.shape[0] == len(ref["ups"]) == S.ITERS and torch.isfinite(up).all()
    e_ups = [(up[i] - ref["ups"][i]).abs().max().item() for i in range(S.ITERS)]
    e_low = (low - ref["low"]).abs().max().item()
    e_net = (net - ref["net"]).abs().max().item()
    drift = _drift().get((case["name"], run))
    line = (f"{case['name']:<11} {arith:<7} {run:<5} up {max(e_ups):.2e}   low {e_low:.2e}   net {e_net:.2e}   "
            f"(fp32 oracle's own drift on the maps: {'n/a' if drift is None else format(drift, '.2e')})\n")
    print("\n" + line, end="")
    _figures[(case["name"], arith, run)] = line
    assert max(e_ups) <= 1e-4, (e_ups, line)
    assert e_low <= 1e-4 and e_net <= 5e-5, line


@pytest.mark.parametrize("arith", S.ARITHS)
@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_block_once_vs_float64(case, arith):
    """BasicUpdateBlock.forward on features from the float64 lookup: net, mask and delta within 2e-5 * max(1, |ref| max), the bar of
    test_update_block_golden / test_update_block_fullsize_vs_oracle.  (The single-call path runs the full GRU convs: Cin 232 for
    h96, which the split blobs keep in exact fp32.)"""
    ins, truth = S.block_once(case)
    ub = _make_block(case, arith)
    dev_ins = [t.to(DEV) for t in ins]
    _calibrate(arith, lambda: ub(*dev_ins), case["name"])
    outs = [o.cpu().double() for o in ub(*dev_ins)]
    for got, exp, key in zip(outs, truth, ("net", "mask", "delta")):
        err, sc = (got - exp).abs().max().item(), exp.abs().max().item()
        print(f"\n[{case['name']} {arith}] {key}: max-abs {err:.2e} (|ref| max {sc:.3g})", end="")
        assert got.shape == exp.shape and err <= 2e-5 * max(1.0, sc), (key, err, sc)
    if arith == "fp16x2":
        ranges = ub.engine.activation_ranges()  # the layers that kept the split arithmetic
        for name in ("gru.convz1+convr1", "gru.convq1", "gru.convz1+convr1[inp]"):
            cin = S.gru_cin(case) if "[" not in name else case["ctx"]
            assert (name in ranges) == (cin % 16 == 0), (name, cin, sorted(ranges))
        assert "gru.convz1+convr1[h,motion]" in ranges and "encoder.convc2" in ranges
        assert ("encoder.convc1" in ranges) == (S.cor_planes(case) % 16 == 0)


@pytest.mark.parametrize("run", S.RUNS)
@pytest.mark.parametrize("arith", S.ARITHS)
@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_fused_loop_vs_float64(case, arith, run):
    eng = _engine(case, arith, run)
    _check_loop(case, arith, run, _refine(eng, case, run))


def _expected_launches(case, arith):
    """{launch name: count per iteration} the case must show in NND_DEBUG_SYNC's trace, and the names it must not show."""
    loop, split = case["loop"], arith != "fp32"
    planes = S.cor_planes(case)
    want, never = {}, []
    # mask head + upsample
    if case["up"] == "fused":
        folded = arith == "fp16x2" and loop != "cre"  # flow_head.conv2 inside the launch: one flow channel, at most 256 tiles
        want["flow_head.conv2 + mask.2 + upsample" if folded else "mask.2 + upsample"] = 1
        never += ["mask.2", "convex upsample", "mask.2 + upsample" if folded else "flow_head.conv2 + mask.2 + upsample"]
        want["flow_head.conv2"] = 0 if folded else 1
    else:
        want.update({"mask.2": 1, "convex upsample": 1, "flow_head.conv2": 1})
        never += ["mask.2 + upsample", "flow_head.conv2 + mask.2 + upsample"]
    # lookup + convc1
    il = loop == "igev" and case["groups"] == 8 and case["radius"] == 4
    if loop == "raft" and arith == "fp16x2":
        want["encoder.convf1+convf2 | lookup+convc1"] = 1
        never += ["lookup+convc1", "lookup", "encoder.convc1", "encoder.convf1+convf2"]
    elif il:
        want["lookup+convc1 (interleaved)"] = 1
        never += ["lookup+convc1", "lookup", "encoder.convc1"]
    elif loop == "raft" or (loop == "igev" and not (split and planes % 16 == 0)):
        want["lookup+convc1"] = 1  # the sampled features never reach HBM: convc1 in exact fp32 inside lookup_convc1_kernel
        never += ["lookup", "encoder.convc1", "lookup+convc1 (interleaved)"]
    else:  # cre, group; igev with a split convc1 and no interleaved kernel for its groups / radius
        want.update({"lookup": 1, "encoder.convc1": 1})
        never += ["lookup+convc1", "lookup+convc1 (interleaved)"]
    # the motion encoder's flow branch: one launch in a split arithmetic
    if not (loop == "raft" and arith == "fp16x2"):
        if split:
            want["encoder.convf1+convf2"] = 1
            never += ["encoder.convf1", "encoder.convf2"]
        else:
            want.update({"encoder.convf1": 1, "encoder.convf2": 1})
    gru = {"gru.convz1+convr1[h,motion]": 1, "gru.convq1[rh,motion]": 1}
    gru.update({"gru.convz2+convr2[h,motion]": 1, "gru.convq2[rh,motion]": 1} if case["gru"] == "sep_conv" else {})
    want.update(gru)
    want.update({"encoder.convc2": 1, "encoder.conv": 1, "flow_head.conv1+mask.0": 1})
    return want, never


@pytest.mark.parametrize("arith", S.ARITHS)
@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_the_path_claimed_is_the_path_run(case, arith, monkeypatch, capfd):
    iters = 2
    eng = _engine(case, arith, "zero")
    torch.cuda.synchronize()
    capfd.readouterr()
    monkeypatch.setenv("NND_DEBUG_SYNC", "1")
    _refine(eng, case, "zero", iters)
    torch.cuda.synchronize()
    names = re.findall(r"\[nnd\] (.*?) \.\.\. ok", capfd.readouterr().err)
    want, never = _expected_launches(case, arith)
    for name, per_iter in want.items():
        assert names.count(name) == per_iter * iters, (name, names)
    for name in never:
        assert names.count(name) == 0, (name, names)
    ctx_terms = [n for n in names if n.endswith("[inp]")]  # once per pair, in front of the loop
    assert len(ctx_terms) == (4 if case["gru"] == "sep_conv" else 2), names


@pytest.mark.parametrize("arith", S.ARITHS)
@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_fused_launches_against_their_switches(case, arith, monkeypatch):
    """Every fused launch the case took, against the launches it replaces.  NND_NO_FOLDED_FLOW_HEAD and NND_NO_MERGED_FB_LOOKUP: every
    output bit for bit (test_folded_flow_head_is_bit_identical_to_its_own_launch,
    test_merged_flow_branch_lookup_launch_is_bit_identical_to_two_launches).  NND_NO_FUSED_UPSAMPLE: the recurrence bit for bit, the maps to
    rounding, 2e-5 relative (test_fused_mask_upsample_split_matches_unfused).  NND_NO_FUSED_LOOKUP: another K split of convc1, so
    everything to rounding (test_fused_lookup_convc1_matches_unfused)."""
    want, _ = _expected_launches(case, arith)
    eng = _engine(case, arith, "wide")
    base = [t.clone() for t in _refine(eng, case, "wide")]
    assert all(torch.isfinite(t).all() for t in base)

    def close(a, b):
        return (a - b).abs().max().item() <= 2e-5 * max(1.0, b.abs().max().item())

    ran = []
    if want.get("flow_head.conv2 + mask.2 + upsample"):
        monkeypatch.setenv("NND_NO_FOLDED_FLOW_HEAD", "1")
        other = _refine(eng, case, "wide")
        monkeypatch.delenv("NND_NO_FOLDED_FLOW_HEAD")
        assert all(torch.equal(a, b) for a, b in zip(base, other)), "folded flow head"
        ran.append("fold")
    if want.get("encoder.convf1+convf2 | lookup+convc1"):  # the same device code as its two launches: bit for bit
        monkeypatch.setenv("NND_NO_MERGED_FB_LOOKUP", "1")
        other = _refine(eng, case, "wide")
        monkeypatch.delenv("NND_NO_MERGED_FB_LOOKUP")
        assert all(torch.equal(a, b) for a, b in zip(base, other)), "merged flow branch + lookup"
        ran.append("merged")
    if case["up"] == "fused":
        monkeypatch.setenv("NND_NO_FUSED_UPSAMPLE", "1")
        up, low, net = _refine(eng, case, "wide")
        monkeypatch.delenv("NND_NO_FUSED_UPSAMPLE")
        assert torch.equal(low, base[1]) and torch.equal(net, base[2]), "the recurrence does not depend on how the mask head is launched"
        assert close(up, base[0])
        ran.append("upsample")
    if any(k in want for k in ("lookup+convc1", "lookup+convc1 (interleaved)", "encoder.convf1+convf2 | lookup+convc1")):
        monkeypatch.setenv("NND_NO_FUSED_LOOKUP", "1")
        other = _refine(eng, case, "wide")
        monkeypatch.delenv("NND_NO_FUSED_LOOKUP")
        assert all(close(a, b) for a, b in zip(other, base)), "fused lookup"
        ran.append("lookup")
    assert ran or case["up"] == "unfused"


# ---------------------------------------------------------------- descriptors outside the table
@pytest.mark.parametrize("case", S.LARGE_HIDDEN, ids=[c["name"] for c in S.LARGE_HIDDEN])
def test_large_hidden_dim_runs_or_is_refused_when_the_engine_is_built(case):
    """hidden_dim 192 / 256: held to the table's bars, or refused by name before anything is enqueued — never accepted by pack and
    then refused by a launch in the middle of refine."""
    from nndepth_amd._lib import NndError
    for arith in S.ARITHS:
        try:
            eng = _make_block(case, arith).sync_engine(DEV)
        except NndError as e:
            assert "hidden_dim" in str(e), str(e)
            continue
        ins, truth = S.block_once(case)
        ub = _make_block(case, arith)
        dev_ins = [t.to(DEV) for t in ins]
        _calibrate(arith, lambda: ub(*dev_ins), case["name"])
        for got, exp in zip(ub(*dev_ins), truth):
            assert (got.cpu().double() - exp).abs().max().item() <= 2e-5 * max(1.0, exp.abs().max().item())
        for run in S.RUNS:
            _calibrate(arith, lambda: _refine(eng, case, run), case["name"])
            _check_loop(case, arith, run, _refine(eng, case, run))


@pytest.mark.parametrize("kw,word", [(dict(hidden_dim=48, context_dim=64), "hidden_dim"), (dict(hidden_dim=64, context_dim=12), "context_dim"),
                                     (dict(hidden_dim=256, context_dim=64, flow_channel=2), "hidden_dim")])
def test_unsupported_descriptors_are_refused_when_the_engine_is_built(kw, word):
    from nndepth_amd._lib import NndError
    from nndepth_amd.blocks import BasicUpdateBlock
    kw = dict(dict(cor_planes=36, flow_channel=1, spatial_scale=8), **kw)
    for arith in S.ARITHS:
        with pytest.raises(NndError, match=word):
            BasicUpdateBlock(arithmetic=arith, **kw).to(DEV).sync_engine(DEV)


# ---------------------------------------------------------------- model level
MODELS = {"f128_h96_c40_l3r4": dict(fnet_dim=128, hidden_dim=96, context_dim=40, corr_levels=3, corr_radius=4),
          "f64_h64_c64_l2r3": dict(fnet_dim=64, hidden_dim=64, context_dim=64, corr_levels=2, corr_radius=3)}


@functools.lru_cache(maxsize=None)
def _model_reference(name):
    from nndepth_amd import weightgen
    from oracle import torch_ref as R
    kw = MODELS[name]
    sd = weightgen.fill_state_dict(R.raft_stereo_spec(**kw))
    f1, f2 = weightgen.synthetic_frames(4, 2, 104, 176)
    with torch.no_grad():
        ref = R.raft_stereo_forward(sd, f1, f2, 3, **{k: v for k, v in kw.items() if k != "fnet_dim"})
    return sd, f1, f2, ref


@pytest.mark.parametrize("arith", ["fp32", "fp16x2"])
@pytest.mark.parametrize("name", list(MODELS))
def test_raft_stereo_with_non_default_dimensions_vs_oracle(name, arith):
    """BaseRAFTStereo forwards fnet_dim / hidden_dim / context_dim / corr_levels / corr_radius to the HIP encoder, the pyramid build
    and the loop: 2 x 104 x 176 frames (13 x 22 at 1/8), 3 iterations, every map within 1e-4 of the oracle's forward with the same
    keywords (test_forward_kitti_shape_batch2_vs_oracle's bar); fp16x2 through the model's own first-forward calibration;
    outputs="last" returns the last map of outputs="all" bit for bit."""
    from nndepth_amd.raft_stereo import BaseRAFTStereo
    sd, f1, f2, ref = _model_reference(name)
    m = BaseRAFTStereo(iters=3, arithmetic=arith, **MODELS[name])
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    assert m.hip_encoder
    a, b = f1.to(DEV), f2.to(DEV)
    outs = m(a, b)
    errs = [(o["up_disp"].cpu() - r).abs().max().item() for o, r in zip(outs, ref)]
    print(f"\n[{name} {arith}] max-abs per iteration vs oracle:", " ".join(f"{e:.2e}" for e in errs), end="")
    assert len(outs) == len(ref) == 3 and max(errs) <= 1e-4, errs
    full = [o["up_disp"].clone() for o in m(a, b)]
    m.outputs = "last"
    last = m(a, b)
    assert len(last) == 1 and torch.equal(last[0]["up_disp"], full[-1])
