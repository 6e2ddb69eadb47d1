"""GPU: the one-piece fp16 arithmetic ("fp16", csrc/split_arith.h) layer by layer.

Contract: y_c = oscale * sum x^ w^ (+ bias, epilogue) in float64 with x^ = fp16_rne(x * 2^xs), w^ = fp16_rne(w * 2^s) rounded on the host by
torch.half from the scales read back from the blob.  Gate: the exact fp32 kernel fed the pre-rounded operands x^ / 2^xs, w^ / 2^s
computes the same sum (every product of two fp16 values is exact in fp32) with fp32 accumulation; the one-piece kernel's max-abs and
rms error against y_c must be at most 2 x those of that run — the factor covers the other summation order (16-deep MFMA, split-K
exchange).  Both errors of every case go into tests/golden/REPORT_fp16.txt.

1. ops.Conv2d (one NCHW source, stride 1): every stride-1 layer shape of the loops on the ragged 2x13x22 map, every (ny, ks, P, nu,
   fast) the picker accepts for NS = 1 — enumerated from the NND_CONV_VERBOSE plan line, forced with NND_SPLIT_CFG —, inputs of
   magnitude log-uniform in [2^-6, 1] * M, M in 2^-8 / 1 / 2^8; subnormal pieces against the analytic bound; out of range; NaN;
   poisoned outputs; run to run.
2. What only the engines launch — two sources in the c4 layout with the GRU epilogues, stride 2 with the folded-norm and residual
   epilogues — is held to the same contract gate launch by launch in tests/test_gpu_fp16_layers.py.  Here the update block's whole
   forward and the whole encoder run once more in place: against the gate of tests/test_gpu_fp16_loops.py (at most half the
   deviation that operands rounded to bfloat16 give, against float64), bit-identical run to run and with NaN-filled workspaces, and
   a frame past the encoder's calibrated range gives non-finite feature maps."""
import re

import pytest
import torch

import desc_sweep_cases as S
import history_util as HU
from fp16_report import report_section

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARK = "== per layer (tests/test_gpu_fp16_conv.py)\n"
B, H, W = 2, 13, 22
_lines = {}


@pytest.fixture(autouse=True)
def _keep_global_rng():
    """The module constructors draw their initial parameters from torch's global generators; tests that run later in the same process
    and draw from them (tests/test_gpu_last_only.py) must see the state they would see without this file."""
    cpu, dev = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    yield
    torch.set_rng_state(cpu)
    torch.cuda.set_rng_state(dev, DEV)

SPLIT_RE = re.compile(r"\[nnd\] conv_split (\d)x(\d) Cin=(\d+) Cout=(\d+) pieces=(\d): ny=(\d+), wco=(\d+), ks=(\d+), P=(\d+), nu=(\d+)"
                      r"(, fast)?, grid [^\n]*?(, stride 2)?$", re.M)


def split_lines(err):
    return [dict(KH=int(m[1]), KW=int(m[2]), Cin=int(m[3]), Cout=int(m[4]), pieces=int(m[5]), ny=int(m[6]), wco=int(m[7]), ks=int(m[8]),
                 P=int(m[9]), nu=int(m[10]), fast=bool(m[11]), stride=2 if m[12] else 1) for m in SPLIT_RE.finditer(err)]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _lines:
        report_section(MARK, [_lines[k] for k in sorted(_lines)])


# (KH, KW, Cin, Cout): the stride-1 shapes the loops send to the split kernels — 3x3 at Cin 64 / 128 / 256 / 320 (hid + ctx + hid of
# the default block; the loops split it into its two sources) / 384, ragged Cout, the separable GRU's 1x5 / 5x1, 1x1 (mask.2, IGEV's convc1)
CLASSES = [(3, 3, 64, 192), (3, 3, 128, 64), (3, 3, 128, 384), (3, 3, 256, 192), (3, 3, 256, 127), (3, 3, 320, 128), (3, 3, 384, 256),
           (1, 5, 256, 256), (5, 1, 256, 128), (1, 5, 64, 128), (5, 1, 320, 256), (1, 1, 256, 576), (1, 1, 576, 256)]
M_SWEEP = {(3, 3, 128, 64), (1, 5, 256, 256), (1, 1, 256, 576)}  # these also at M = 2^-8 and 2^8
CASES = [(k, m) for k in CLASSES for m in ((-8, 0, 8) if k in M_SWEEP else (0,))]


def _log_uniform(shape, lo, hi, g):
    mag = torch.exp2(lo + (hi - lo) * torch.rand(shape, generator=g, dtype=torch.float64))
    sign = torch.randint(0, 2, shape, generator=g, dtype=torch.int64) * 2 - 1
    return (mag * sign).float()


_DATA = {}


def data(k, m, lo=-6.0):
    """(w, b, x) of a case: magnitudes log-uniform in [2^lo, 1] * 2^m with random sign, computed once."""
    if (k, m, lo) not in _DATA:
        kh, kw, cin, cout = k
        g = torch.Generator().manual_seed(kh * 1000003 + kw * 10007 + cin * 31 + cout + 7 * (m + 8))
        w = _log_uniform((cout, cin, kh, kw), lo + m, float(m), g)
        x = _log_uniform((B, cin, H, W), lo + m, float(m), g)
        b = _log_uniform((cout,), lo + 2 * m, 2.0 * m, g)
        _DATA[(k, m, lo)] = (w, b, x)
    return _DATA[(k, m, lo)]


def scales(conv):
    """(xscale = 2^xs, wsinv = 2^-s, oscale) of an ops.Conv2d in a range-scaled arithmetic: the 4-float tail behind the bias."""
    tail = conv.packed[-4:].cpu()
    return tail[1].item(), tail[3].item(), tail[0].item()


def contract(conv, w, b, x, relu=False):
    """-> (y_c float64, x^ / 2^xs, w^ / 2^s as float32 tensors: exact, powers of two)"""
    xscale, wsinv, oscale = scales(conv)
    assert oscale == wsinv / xscale
    xh, wh = (x * xscale).half(), (w / wsinv).half()
    assert torch.isfinite(xh).all() and torch.isfinite(wh).all()
    kh, kw = w.shape[2:]
    y = torch.nn.functional.conv2d(xh.double(), wh.double(), None, padding=(kh // 2, kw // 2)) * oscale + b.double().view(1, -1, 1, 1)
    return (y.clamp_min(0) if relu else y), xh.float() / xscale, wh.float() * wsinv, (xh, wh)


def errs(y, truth):
    d = y.double() - truth
    return d.abs().max().item(), d.pow(2).mean().sqrt().item()


def _run(capfd, fn):
    from nndepth_amd._lib import NndError
    torch.cuda.synchronize()
    capfd.readouterr()
    try:
        out = fn()
        torch.cuda.synchronize()
    except NndError as e:
        out = e
    return out, capfd.readouterr().err


def _divisors(n):
    return [d for d in range(1, n + 1) if n % d == 0]


def case_id(c):
    (kh, kw, cin, cout), m = c
    return f"{kh}x{kw}-{cin}to{cout}-M2^{m}"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_conv2d_every_configuration_vs_contract(monkeypatch, capfd, case):
    from nndepth_amd import ops
    k, m = case
    kh, kw, cin, cout = k
    w, b, x = data(k, m)
    xd = x.to(DEV)
    conv = ops.Conv2d(w, b, arithmetic="fp16")
    conv.calibrate(xd)
    y_c, xr, wr, (xh, wh) = contract(conv, w, b, x)
    # calibrated on these inputs every scaled operand is a normal fp16 number: the largest in [2^10, 2^11) / [2^13, 2^14)
    xscale, wsinv, _ = scales(conv)
    assert 2 ** 10 <= x.abs().max().item() * xscale < 2 ** 11 and 2 ** 13 <= w.abs().max().item() / wsinv < 2 ** 14
    assert xh.float().abs().min() >= 2.0 ** -14 and wh.float().abs().min() >= 2.0 ** -14
    y_relu = y_c.clamp_min(0)
    exact = ops.Conv2d(wr, b)  # the exact fp32 kernel on the pre-rounded operands
    e32 = errs(exact(xr.to(DEV)).cpu(), y_c)
    ncb = (cout + 31) // 32
    cfgs = [(f"{ny},{ks},2", ny, ks) for ks in (1, 2, 4) for ny in _divisors(ncb)] + [(None, 0, 0), ("nofast", 0, 0)]
    rows, refused, groups = [], [], {}
    for cfg, ny, ks in cfgs:
        monkeypatch.delenv("NND_SPLIT_CFG", raising=False)
        monkeypatch.delenv("NND_SPLIT_NO_FAST", raising=False)
        monkeypatch.setenv("NND_CONV_VERBOSE", "1")
        if cfg == "nofast":
            monkeypatch.setenv("NND_SPLIT_NO_FAST", "1")
        elif cfg is not None:
            monkeypatch.setenv("NND_SPLIT_CFG", cfg)
        y, err = _run(capfd, lambda: conv(xd))
        lines = split_lines(err)
        if isinstance(y, Exception):
            assert cfg not in (None, "nofast"), f"the picker found no configuration: {y}"
            assert "no configuration" in str(y) and f"ny={ny} ks={ks} P=2" in str(y), str(y)
            assert not lines, f"refused configuration {cfg} launched: {lines}"
            refused.append(cfg)
            continue
        assert len(lines) == 1, err
        L = lines[0]
        assert (L["KH"], L["KW"], L["Cin"], L["Cout"], L["pieces"], L["stride"]) == (kh, kw, cin, cout, 1, 1), L
        if ny:
            assert (L["ny"], L["ks"], L["P"], L["wco"]) == (ny, ks, 2, ncb // ny), (cfg, L)
        if cfg == "nofast":
            assert not L["fast"], L
        y2, yr = conv(xd).cpu(), conv(xd, relu=True).cpu()
        y = y.cpu()
        assert torch.equal(y, y2), (cfg, "run to run")
        rows.append((cfg or "picker", L, errs(y, y_c), errs(yr, y_relu)))
        groups.setdefault((L["ks"], L["P"], L["fast"]), []).append((cfg or "picker", y))
    monkeypatch.delenv("NND_SPLIT_CFG", raising=False)
    monkeypatch.delenv("NND_SPLIT_NO_FAST", raising=False)
    txt = (f"{case_id(case):<22} |y| max {y_c.abs().max().item():.3g}: exact fp32 kernel on the rounded operands max-abs {e32[0]:.2e} rms {e32[1]:.2e}; "
           f"{len(rows)} configurations accepted, {len(refused)} refused\n")
    for cfg, L, e, er in rows:
        txt += (f"    {cfg:>8} ny={L['ny']} wco={L['wco']} ks={L['ks']} P={L['P']} nu={L['nu']} {'fast' if L['fast'] else 'generic':<7} "
                f"max-abs {e[0]:.2e} rms {e[1]:.2e}   relu max-abs {er[0]:.2e}\n")
    print("\n" + txt, end="")
    _lines[(CASES.index(case), 0)] = txt
    for cfg, L, e, er in rows:
        assert e[0] <= 2 * e32[0] and e[1] <= 2 * e32[1], (cfg, L, e, e32)
        assert er[0] <= 2 * e32[0] and er[1] <= 2 * e32[1], (cfg, L, er, e32)
    for key, outs in groups.items():  # ny only groups output-channel blocks into workgroups
        for cfg, y in outs[1:]:
            assert torch.equal(y, outs[0][1]), (key, outs[0][0], cfg)
    nchunks = cin // 16
    assert {L["ks"] for _, L, *_ in rows} >= {ks for ks in (1, 2, 4) if ks <= nchunks and any(
        ncb // ny * ks <= 12 for ny in _divisors(ncb))}, rows


def test_plans_use_the_one_piece_geometry(monkeypatch, capfd):
    """pick_split plans from split_patch(..., NS = 1): half the piece bytes per staged position (48 B against 80), so the LDS a
    configuration asks for is below the fp16x2 plan's of the same shape, and both staging variants (nu 2 / 4) and both regimes run."""
    from nndepth_amd import ops
    seen = set()
    for k, cfg in [((3, 3, 256, 192), "1,2,2"), ((3, 3, 256, 192), "6,1,2"), ((1, 1, 256, 576), "3,2,2"), ((1, 5, 256, 256), "2,1,2")]:
        w, b, x = data(k, 0)
        lds = {}
        for arith in ("fp16", "fp16x2"):
            conv = ops.Conv2d(w, b, arithmetic=arith)
            conv.calibrate(x.to(DEV))
            monkeypatch.setenv("NND_CONV_VERBOSE", "1")
            monkeypatch.setenv("NND_SPLIT_CFG", cfg)
            y, err = _run(capfd, lambda: conv(x.to(DEV)))
            assert not isinstance(y, Exception), y
            (L,) = split_lines(err)
            assert L["pieces"] == (1 if arith == "fp16" else 2)
            lds[arith] = int(re.search(r"lds (\d+) B", err)[1])
            if arith == "fp16":
                seen.add((L["nu"], L["fast"]))
        ks = int(cfg.split(",")[1])
        if ks == 1:  # no split-K exchange buffer: the patch alone, 2 buffers x P x SUBB
            assert lds["fp16"] < lds["fp16x2"], (k, cfg, lds)
        else:
            assert lds["fp16"] <= lds["fp16x2"], (k, cfg, lds)
    monkeypatch.setenv("NND_SPLIT_NO_FAST", "1")
    monkeypatch.delenv("NND_SPLIT_CFG")
    w, b, x = data((3, 3, 128, 64), 0)
    conv = ops.Conv2d(w, b, arithmetic="fp16")
    y, err = _run(capfd, lambda: conv(x.to(DEV)))
    (L,) = split_lines(err)
    seen.add((L["nu"], L["fast"]))
    print(f"\n(nu, fast) variants run: {sorted(seen)}")
    assert {nu for nu, _ in seen} == {2, 4} and {f for _, f in seen} == {True, False}, seen


def test_subnormal_pieces_within_the_analytic_bound():
    """Elements down to M * 2^-30: below 2^-14 in scaled units a piece is an fp16 subnormal (absolute error <= 2^-25).  |y - y_true| <= (2^-10 + K * 2^-24) * sum |x||w| + 2^-25 * 2^-xs * sum |w| with y_true the float64 convolution of the
    unrounded operands: 2^-11 relative for each operand (and their product), fp32 accumulation of K products, and the absolute
    error of the subnormal pieces."""
    from nndepth_amd import ops
    k = (3, 3, 128, 64)
    kh, kw, cin, cout = k
    w, b, _ = data(k, 0)
    _, _, x = data(k, 0, lo=-30.0)
    xd = x.to(DEV)
    conv = ops.Conv2d(w, b, arithmetic="fp16")
    conv.calibrate(xd)
    xscale, wsinv, _ = scales(conv)
    xh = (x * xscale).half().float()
    nsub, nzero = int(((xh.abs() < 2.0 ** -14) & (xh != 0)).sum()), int((xh == 0).sum())
    assert nsub > 1000, (nsub, nzero)  # (M * 2^-30 scaled by 2^10 is 2^-20: above half the smallest subnormal, no piece is zero)
    conv2 = torch.nn.functional.conv2d
    truth = conv2(x.double(), w.double(), b.double(), padding=1)
    K = cin * kh * kw
    bound = (2.0 ** -10 + K * 2.0 ** -24) * conv2(x.double().abs(), w.double().abs(), padding=1) \
        + 2.0 ** -25 / xscale * conv2(torch.ones_like(x, dtype=torch.float64), w.double().abs(), padding=1)
    y = conv(xd).cpu().double()
    ratio = ((y - truth).abs() / bound).max().item()
    line = f"subnormal pieces 3x3-128to64, |x| in [2^-30, 1]: {nsub} subnormal pieces; max |y - y_true| / bound = {ratio:.3f}\n"
    print("\n" + line, end="")
    _lines[(900, 0)] = line
    assert ratio <= 1.0


@pytest.mark.parametrize("k", [(3, 3, 128, 64), (1, 5, 256, 256), (1, 1, 256, 576)], ids=lambda k: "x".join(map(str, k)))
def test_out_of_range_and_nan_are_visible(k):
    """An activation of 64 x the calibrated maximum (the range ends at 32 x) gives inf or NaN in every output whose window holds it,
    and no other output changes; NaN in gives NaN out in the same outputs."""
    from nndepth_amd import ops
    kh, kw, cin, cout = k
    w, b, x = data(k, 0)
    conv = ops.Conv2d(w, b, arithmetic="fp16")
    conv.calibrate(x.to(DEV))
    assert conv.activation_range() >= 32 * x.abs().max().item() * 0.999 and conv.activation_range() < 64 * x.abs().max().item()
    base = conv(x.to(DEV)).cpu()
    assert torch.isfinite(base).all()
    bi, ci, yi, xi = 1, 37, 6, 10
    reach = torch.zeros(B, 1, H, W, dtype=torch.bool)
    reach[bi, 0, max(0, yi - kh // 2):yi + kh // 2 + 1, max(0, xi - kw // 2):xi + kw // 2 + 1] = True
    reach = reach.expand(B, cout, H, W)
    for bad, name in ((64.0 * x.abs().max().item(), "64 x max"), (-64.0 * x.abs().max().item(), "-64 x max"), (float("nan"), "nan")):
        x2 = x.clone()
        x2[bi, ci, yi, xi] = bad
        y = conv(x2.to(DEV)).cpu()
        assert not torch.isfinite(y[reach]).any(), (name, int(torch.isfinite(y[reach]).sum()))
        if name == "nan":
            assert torch.isnan(y[reach]).all()
        assert torch.equal(y[~reach], base[~reach]), name
    yr = conv(x2.to(DEV), relu=True).cpu()  # NaN passes the ReLU (common.h relu_nan)
    assert torch.isnan(yr[reach]).all() and torch.equal(yr[~reach], base[~reach].clamp_min(0))


def test_poisoned_outputs_do_not_change_results(monkeypatch):
    from nndepth_amd import ops
    for k in [(3, 3, 256, 127), (1, 1, 576, 256), (5, 1, 320, 256)]:
        w, b, x = data(k, 0)
        conv = ops.Conv2d(w, b, arithmetic="fp16")
        conv.calibrate(x.to(DEV))
        base = HU.snapshot(conv(x.to(DEV)))
        for kind in ("nan", "garbage"):
            with HU.poisoned_allocators(monkeypatch, kind) as filled:
                got = HU.snapshot(conv(x.to(DEV)))
            assert filled and not HU.differences(base, got), (k, kind, HU.differences(base, got))


# ------------------------------------------------------------------------------------------------ item 2: inside the engines
def _bf16_conv(sd, name, x, stride=1, padding=0):
    """oracle.torch_ref._conv with both operands rounded to bfloat16: the reference's validation arithmetic (autocast), emulated."""
    r = lambda t: t.to(torch.bfloat16).to(t.dtype)  # noqa: E731
    bias = sd.get(name + ".bias")
    return torch.nn.functional.conv2d(r(x), r(sd[name + ".weight"]), bias, stride=stride, padding=padding)


BLOCK_CASES = ["h64_r8", "h128_f2_c8", "h64_cg", "h128_r4", "ig_l2", "h96"]


@pytest.mark.parametrize("name", BLOCK_CASES)
def test_update_block_forward_two_sources_and_gru_epilogues(monkeypatch, name):
    """The update block's single call (two-source c4 launches, GRU z/r and q epilogues, ReLU, the flow branch, mask.2 as a conv):
    net, mask and delta deviate from the float64 block by at most half of what operands rounded to bfloat16 give (mean-abs, per
    output; the gate of the loops test, where it is derived); two calls are bit-identical, poisoned workspaces change nothing."""
    from oracle import torch_ref as R
    from nndepth_amd.blocks import BasicUpdateBlock
    from nndepth_amd.raft_stereo import calibration_passes
    case = S.BY_NAME[name]
    ins, truth = S.block_once(case)
    with torch.no_grad(), monkeypatch.context() as mp:
        mp.setattr(R, "_conv", _bf16_conv)
        emu = R.update_block(S.state_dict(case, torch.float64), S.prefix(case), *(t.double() for t in ins), gru=case["gru"])
    ub = BasicUpdateBlock(**S.block_kwargs(case), arithmetic="fp16")
    ub.load_state_dict(S.state_dict(case, strip=True), strict=True)
    ub = ub.to(DEV).eval()
    dev_ins = [t.to(DEV) for t in ins]
    calibration_passes(lambda: ub(*dev_ins), 4, name)
    outs = HU.snapshot(ub(*dev_ins))
    assert not HU.differences(outs, HU.snapshot(ub(*dev_ins)))
    ub.engine._ws = None  # a fresh workspace, poisoned
    with HU.poisoned_allocators(monkeypatch, "nan") as filled:
        again = HU.snapshot(ub(*dev_ins))
    assert filled and not HU.differences(outs, again), HU.differences(outs, again)
    txt = f"update block forward {name}:"
    ok = True
    for got, exp, e, key in zip(outs, truth, emu, ("net", "mask", "delta")):
        d16, dbf = (got.cpu().double() - exp).abs().mean().item(), (e - exp).abs().mean().item()
        txt += f"  {key} fp16 {d16:.2e} bf16-emulated {dbf:.2e} ratio {d16 / dbf:.3f}"
        ok = ok and torch.isfinite(got).all().item() and d16 <= 0.5 * dbf
    print("\n" + txt, end="")
    _lines[(910, BLOCK_CASES.index(name))] = txt + "\n"
    assert ok, txt


@pytest.mark.parametrize("Bn,Hf,Wf", [(2, 104, 176), (1, 99, 161)])
def test_encoder_stride2_norm_and_residual_epilogues(monkeypatch, capfd, raft_sd, Bn, Hf, Wf):
    """The encoder in one piece: stride-2 3x3 and 1x1 launches (2x26x44 maps at layer3's input for 104x176 frames; odd sizes for
    99x161), folded-norm + ReLU and residual epilogues, the context projection.  fmap and cnet deviate from the float64 oracle by at
    most half of the oracle's deviation with conv operands rounded to bfloat16 (mean-abs); the plan lines say pieces=1, stride-2
    launches included; two runs are bit-identical; NaN-filled workspaces change nothing; a frame beyond the calibrated range gives
    non-finite feature maps, never finite wrong ones."""
    from oracle import torch_ref as R
    from nndepth_amd import ops, weightgen
    fr1, fr2 = weightgen.synthetic_frames(7, Bn, Hf, Wf)
    frames = torch.cat([fr1, fr2], 0)
    enc_sd = {kk[len("fnet."):]: v for kk, v in raft_sd.items() if kk.startswith("fnet.")}
    cnet_sd = {kk[len("cnet_proj."):]: v for kk, v in raft_sd.items() if kk.startswith("cnet_proj.")}
    sd64 = {kk: v.double() for kk, v in raft_sd.items()}

    def oracle():
        fm = R.basic_encoder(sd64, "fnet", frames.double())
        return fm, torch.relu(R._conv(sd64, "cnet_proj.0", fm[:Bn], padding=1))
    with torch.no_grad():
        exp = oracle()
        with monkeypatch.context() as mp:
            mp.setattr(R, "_conv", _bf16_conv)
            emu = oracle()
    eng = ops.EncoderEngine(256, "batch", 192, arithmetic="fp16").load(enc_sd, cnet_sd, device=DEV)
    fd = frames.to(DEV)
    with ops.calibration() as c:
        eng.forward(fd, n_cnet=Bn)
    assert c.status == 0
    monkeypatch.setenv("NND_CONV_VERBOSE", "1")
    out, err = _run(capfd, lambda: HU.snapshot(eng.forward(fd, n_cnet=Bn)))
    monkeypatch.delenv("NND_CONV_VERBOSE")
    assert not isinstance(out, Exception), out
    lines = split_lines(err)
    s2 = [L for L in lines if L["stride"] == 2]
    assert lines and all(L["pieces"] == 1 for L in lines), lines
    assert {(L["KH"], L["Cin"], L["Cout"]) for L in s2} == {(3, 64, 96), (1, 64, 96), (3, 96, 128), (1, 96, 128)} and all(L["fast"] for L in s2), s2
    assert not HU.differences(out, HU.snapshot(eng.forward(fd, n_cnet=Bn)))
    with HU.poisoned_allocators(monkeypatch, "nan") as filled:
        again = HU.snapshot(eng.forward(fd, n_cnet=Bn))
    assert filled and not HU.differences(out, again), HU.differences(out, again)
    txt = f"encoder {Bn}x{Hf}x{Wf}:"
    ok = True
    for got, e, m, key in zip(out, exp, emu, ("fmap", "cnet")):
        d16, dbf = (got.cpu().double() - e).abs().mean().item(), (m - e).abs().mean().item()
        txt += f"  {key} fp16 {d16:.2e} bf16-emulated {dbf:.2e} ratio {d16 / dbf:.3f}"
        ok = ok and torch.isfinite(got).all().item() and d16 <= 0.5 * dbf
    print("\n" + txt, end="")
    _lines[(920, Bn)] = txt + "\n"
    assert ok, txt
    big = eng.forward(fd * 4096.0, n_cnet=Bn)[0]  # far beyond 32 x the calibrated maxima of the deeper layers
    assert not torch.isfinite(big).all()
