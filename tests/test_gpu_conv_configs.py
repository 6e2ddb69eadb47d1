"""GPU: every tile configuration the conv pickers can choose, against float64.

The two convolution kernels take a tile configuration from a host-side plan on every call, and the choice depends on the image
size and batch: conv_split.hip plan_split (pick_split, then restrict_split) -> (ny, ks, P), hence nu and FAST / generic;
conv_mfma.hip plan_tile (pick_tile) -> (wco, ks), hence NE and the LDS size; each prints its plan as one NND_CONV_VERBOSE line
(print_split_plan, print_tile_plan).  The forcing switches (NND_SPLIT_CFG=ny,ks[,P], NND_CONV_CFG=p,ks,wco) reach every configuration; one that
does not exist is refused by the picker before any launch (NndError, no verbose line).  This file sweeps them:

1. split kernel, stride 1, ops.Conv2d: every NND_SPLIT_CFG=ny,ks,2 (ny | ncb, ks in 1 / 2 / 4), the picker's own choice and
   NND_SPLIT_NO_FAST, on every layer class of LAYERS with a split arithmetic; bars of test_split_conv_vs_float64, ReLU epilogue,
   run-to-run torch.equal, and bit-identical outputs over ny for fixed (ks, P, fast);
2. split kernel, stride 2 (the encoder) and two sources in the c4 tile-major layout (the update block), under each forced ks;
3. exact kernel: every NND_CONV_CFG=1,ks,wco on every fp32 class of LAYERS (ops.Conv2d at stride 1, ops.ConvNorm at stride 2),
   against 1.25x the error of the same sums in fp32 chains of the kernel's length; both NE instantiations;
4. the streaming 1x1 kernel of conv_mfma.hip (tile-major sources, Cin 64 / 96 / 128);
5. a coverage guard: every layer the refinement loops launch, at every workload's loop resolution, picks a configuration that
   items 1 and 3 verify.

The float64 truth of a shape is computed once on the CPU and cached for the module."""
import re

import numpy as np
import pytest
import torch

from conftest import t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPLIT_ARITHS = ("bf16x3", "fp16x2")
PIECES = {"bf16x3": 3, "fp16x2": 2}

SPLIT_RE = re.compile(r"\[nnd\] conv_split (\d)x(\d) Cin=(\d+) Cout=(\d+) pieces=(\d): ny=(\d+), wco=(\d+), ks=(\d+), P=(\d+), nu=(\d+)"
                      r"(, fast)?, grid [^\n]*?(, stride 2)?$", re.M)
CONV_RE = re.compile(r"\[nnd\] conv (\d)x(\d) Cin=(\d+) Cout=(\d+) CI_T=(\d+): P=(\d+), wco=(\d+), ks=(\d+), ne=(\d+), grid [^\n]*?(, stride 2)?$",
                     re.M)
STREAM_RE = re.compile(r"\[nnd\] conv1x1_stream Cin=(\d+) Cout=(\d+)")


def split_lines(err):
    """verbose conv_split lines -> [dict(KH, KW, Cin, Cout, pieces, ny, wco, ks, P, nu, fast, stride)]"""
    return [dict(KH=int(m[1]), KW=int(m[2]), Cin=int(m[3]), Cout=int(m[4]), pieces=int(m[5]), ny=int(m[6]), wco=int(m[7]), ks=int(m[8]),
                 P=int(m[9]), nu=int(m[10]), fast=bool(m[11]), stride=2 if m[12] else 1) for m in SPLIT_RE.finditer(err)]


def conv_lines(err):
    """verbose conv_mfma lines -> [dict(KH, KW, Cin, Cout, CI_T, P, wco, ks, ne, stride)]"""
    return [dict(KH=int(m[1]), KW=int(m[2]), Cin=int(m[3]), Cout=int(m[4]), CI_T=int(m[5]), P=int(m[6]), wco=int(m[7]), ks=int(m[8]),
                 ne=int(m[9]), stride=2 if m[10] else 1) for m in CONV_RE.finditer(err)]


# ------------------------------------------------------------------------------------------------ the layer-class table
# (KH, KW, stride, Cin, Cout, arith) -> (B, H, W) of the input the sweeps use.  Items 1 and 3 sweep every class exhaustively; item 5
# requires every layer of the refinement loops to be one of them.  The spatial shapes are the places where tiling goes wrong: an odd
# number of 4x8 sub-tiles (the last P = 2 workgroup has an empty sub-tile), ragged rows and columns, a single sub-tile, W < 8, H < 4,
# batch 3, and one map large enough for the picker's "many columns" rule (136x240 at batch 1: 510 workgroup columns).
ODD = (1, 9, 35)      # 3 x 5 = 15 sub-tiles, both edges cut
RAGGED = (2, 13, 22)  # 4 x 3 sub-tiles, batch 2
TINY = (3, 5, 9)      # 2 x 2 sub-tiles, batch 3
ONE = (1, 4, 8)       # a single sub-tile
SMALL = (2, 3, 6)     # H < 4 and W < 8
MANY = (1, 136, 240)  # 510 columns: the "many columns" rule fires unforced


def _classes(rows, ariths):
    return {(kh, kw, st, cin, cout, a): shape for (kh, kw, st, cin, cout, shape) in rows for a in ariths}


# stride-1 layers of the refinement loops (item 5 checks this list against what the loops launch) and edge classes
_LOOP_SPLIT = [
    (3, 3, 1, 256, 192, ODD), (3, 3, 1, 256, 127, RAGGED), (3, 3, 1, 256, 126, ODD), (3, 3, 1, 256, 63, TINY),
    (1, 5, 1, 256, 256, ODD), (1, 5, 1, 256, 128, RAGGED), (5, 1, 1, 256, 256, RAGGED), (5, 1, 1, 256, 128, ODD),
    (1, 5, 1, 64, 256, ODD), (1, 5, 1, 64, 128, TINY), (5, 1, 1, 64, 256, RAGGED), (5, 1, 1, 64, 128, ODD),
    (1, 5, 1, 128, 256, TINY), (1, 5, 1, 128, 128, ODD), (5, 1, 1, 128, 256, ODD), (5, 1, 1, 128, 128, RAGGED),
    (1, 5, 1, 64, 64, ODD), (5, 1, 1, 64, 64, TINY),
    (3, 3, 1, 256, 256, ODD), (3, 3, 1, 128, 256, RAGGED), (3, 3, 1, 128, 128, TINY),
    (3, 3, 1, 128, 384, ODD), (3, 3, 1, 64, 192, RAGGED), (1, 1, 1, 576, 256, ODD), (3, 3, 1, 128, 64, ODD),
    (1, 5, 1, 128, 64, RAGGED), (5, 1, 1, 128, 64, ODD), (3, 3, 1, 256, 128, RAGGED),
]
_EDGE_SPLIT = [
    (3, 3, 1, 16, 33, TINY),      # one 16-channel chunk: ks > 1 refused; ragged Cout
    (5, 1, 1, 48, 64, RAGGED),    # nchunks % 2 != 0: ks = 2 runs the generic kernel
    (3, 3, 1, 64, 160, ODD),      # the short-K rule; a prime number of channel blocks
    (1, 5, 1, 320, 96, SMALL),    # 20 chunks
    (3, 3, 1, 128, 33, ONE),
    (1, 1, 1, 128, 127, ODD),
    (3, 3, 1, 128, 96, MANY),
]
_EXACT = [
    (3, 3, 1, 256, 192, ODD), (3, 3, 1, 256, 127, RAGGED), (3, 3, 1, 128, 64, TINY), (3, 3, 1, 128, 384, ODD),
    (1, 5, 1, 256, 256, RAGGED), (5, 1, 1, 256, 128, ODD), (1, 5, 1, 64, 256, ODD), (5, 1, 1, 64, 128, TINY),
    (1, 1, 1, 36, 256, ODD), (1, 1, 1, 256, 576, ONE), (1, 1, 1, 200, 96, RAGGED),  # 200: not a multiple of the 128-channel chunk
    (3, 3, 1, 80, 33, SMALL), (3, 3, 1, 64, 160, ODD), (1, 5, 1, 48, 64, RAGGED),   # 80 / 48: not a multiple of the 32-channel chunk
    (3, 3, 1, 256, 256, ODD), (3, 3, 1, 128, 256, RAGGED), (3, 3, 1, 128, 128, TINY), (3, 3, 1, 64, 192, RAGGED),
    (1, 5, 1, 128, 128, ODD), (5, 1, 1, 128, 256, RAGGED), (1, 5, 1, 256, 128, ODD), (5, 1, 1, 256, 256, ODD),
    (1, 5, 1, 128, 256, TINY), (5, 1, 1, 128, 128, RAGGED), (1, 5, 1, 64, 128, ODD), (5, 1, 1, 64, 256, RAGGED),
    (3, 3, 1, 256, 126, ODD), (3, 3, 1, 256, 63, TINY), (1, 5, 1, 64, 64, ODD), (5, 1, 1, 64, 64, TINY),
    (1, 1, 1, 128, 144, ODD), (1, 1, 1, 576, 256, RAGGED), (1, 5, 1, 128, 64, RAGGED), (5, 1, 1, 128, 64, ODD),
    (3, 3, 1, 256, 128, RAGGED),
    (3, 3, 1, 128, 96, MANY),
    # stride 2 (ops.ConvNorm; the shape is the input's): the encoder's downsampling 3x3 and 1x1 layers, odd input sizes
    (3, 3, 2, 64, 96, (2, 19, 37)), (1, 1, 2, 64, 96, (1, 17, 33)), (3, 3, 2, 96, 128, (1, 21, 35)), (1, 1, 2, 96, 128, (2, 9, 15)),
]
LAYERS = {**_classes(_LOOP_SPLIT + _EDGE_SPLIT, SPLIT_ARITHS), **_classes(_EXACT, ("fp32",))}
SPLIT_CLASSES = [k for k in LAYERS if k[5] != "fp32"]
EXACT_CLASSES = [k for k in LAYERS if k[5] == "fp32"]


def cls_id(k):
    kh, kw, st, cin, cout, a = k
    return f"{kh}x{kw}s{st}-{cin}to{cout}-{a}"


# ------------------------------------------------------------------------------------------------ float64 truth, once per class
_DATA = {}


def data(k):
    """(w, b, x, truth float64, |truth| max) of layer class k, computed once."""
    if k not in _DATA:
        kh, kw, st, cin, cout, _ = k
        B, H, W = LAYERS[k]
        g = torch.Generator().manual_seed(kh * 1000003 + kw * 10007 + st * 101 + cin * 31 + cout)
        w = torch.randn(cout, cin, kh, kw, generator=g) / (cin * kh * kw) ** 0.5
        b = torch.randn(cout, generator=g)
        x = torch.randn(B, cin, H, W, generator=g) * 3.0
        truth = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), stride=st, padding=(kh // 2, kw // 2))
        _DATA[k] = (w, b, x, truth, truth.abs().max().item())
    return _DATA[k]


_SEQ = {}


def chain_fp32_error(k, ks, cit):
    """max-abs error vs float64 of the same convolution summed in fp32 the way the exact kernel sums it: each output's products in
    ks sequential chains (chain kj takes the CI_T-channel chunks kj, kj + ks, ...), the chains added at the end, then the bias.  (Its
    order inside a chunk differs from the kernel's; the chain length, which sets the rounding error, is the same.)"""
    if (k, ks, cit) not in _SEQ:
        kh, kw, st, cin, cout, _ = k
        w, b, x, truth, _ = data(k)
        xp = torch.nn.functional.pad(x, (kw // 2, kw // 2, kh // 2, kh // 2))
        Ho, Wo = truth.shape[2:]
        parts = [torch.zeros(truth.shape, dtype=torch.float32) for _ in range(ks)]
        for ci in range(cin):
            acc = parts[(ci // cit) % ks]
            for dy in range(kh):
                for dx in range(kw):
                    xs = xp[:, ci:ci + 1, dy:dy + st * (Ho - 1) + 1:st, dx:dx + st * (Wo - 1) + 1:st]
                    acc += w[:, ci, dy, dx].view(1, -1, 1, 1) * xs
        y = parts[0]
        for p_ in parts[1:]:
            y = y + p_
        _SEQ[(k, ks, cit)] = errs(y + b.view(1, -1, 1, 1), truth)[0]
    return _SEQ[(k, ks, cit)]


def errs(y, truth):
    d = y.double() - truth
    return d.abs().max().item(), d.pow(2).mean().sqrt().item()


def _run(capfd, fn):
    """fn() with the verbose lines it prints -> (result or the NndError, stderr)"""
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


# ------------------------------------------------------------------------------------------------ item 1: split kernel, stride 1
@pytest.mark.parametrize("k", SPLIT_CLASSES, ids=cls_id)
def test_split_every_configuration_vs_float64(monkeypatch, capfd, k):
    """Every NND_SPLIT_CFG=ny,ks,2 with ny | ncb and ks in 1 / 2 / 4, the picker's own choice and NND_SPLIT_NO_FAST, against float64
    with the bars of test_split_conv_vs_float64; the ReLU epilogue; two runs torch.equal; for fixed (ks, P, fast) every ny gives the same bits (ny only groups output-channel blocks into
    workgroups: the K order of a wave and the sum of the ks partial tiles do not depend on it).
    The yardstick is the exact fp32 kernel at the same split-K (NND_CONV_CFG=1,min(ks,2): it has no ks = 4): both kernels sum an
    output's K products in ks fp32 chains, and the chain length, not the configuration, sets the rounding error — measured on
    3x3 256 -> 192 with bf16x3, ks = 1 / 2 / 4 give 1.85e-5 / 1.19e-5 / 7.1e-6 max-abs, the exact kernel 2.46e-5 (ks = 1) and
    1.61e-5 (ks = 2)."""
    from nndepth_amd import ops
    kh, kw, st, cin, cout, arith = k
    w, b, x, truth, scale = data(k)
    xd = x.to(DEV)
    exact, ref32 = ops.Conv2d(w, b), {}
    for ks in (1, 2):
        monkeypatch.setenv("NND_CONV_CFG", f"1,{ks}")
        y32, _ = _run(capfd, lambda: exact(xd))
        ref32[ks] = errs(y32.cpu(), truth) if not isinstance(y32, Exception) else ref32[1]  # one chunk: no split-K
    monkeypatch.delenv("NND_CONV_CFG")
    conv = ops.Conv2d(w, b, arithmetic=arith)
    if arith == "fp16x2":
        conv.calibrate(xd)  # the scale lives in the blob: one calibration serves every configuration
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
            assert not lines, f"refused configuration {cfg} launched: {lines}"  # refused before any launch
            refused.append(cfg)
            continue
        assert len(lines) == 1, err
        L = lines[0]
        assert (L["KH"], L["KW"], L["Cin"], L["Cout"], L["pieces"], L["stride"]) == (kh, kw, cin, cout, PIECES[arith], 1), L
        if ny:
            assert (L["ny"], L["ks"], L["P"], L["wco"]) == (ny, ks, 2, ncb // ny), (cfg, L)
        if cfg == "nofast":
            assert not L["fast"], L
        y2 = conv(xd)
        yr = conv(xd, relu=True)
        y, y2, yr = y.cpu(), y2.cpu(), yr.cpu()
        assert torch.equal(y, y2), (cfg, "run to run")
        esp, rsp = errs(y, truth)
        erelu = (yr.double() - truth.clamp_min(0)).abs().max().item()
        rows.append((cfg or "picker", L, esp, rsp, erelu))
        groups.setdefault((L["ks"], L["P"], L["fast"]), []).append((cfg or "picker", L["ny"], y))
    print(f"\n[split {cls_id(k)} {LAYERS[k]}] exact fp32 kernel ks=1: max-abs {ref32[1][0]:.2e} rms {ref32[1][1]:.2e}, ks=2: "
          f"max-abs {ref32[2][0]:.2e} rms {ref32[2][1]:.2e}   |y| max {scale:.1f}")
    for cfg, L, esp, rsp, erelu in rows:
        print(f"  {cfg:>8}  ({kh},{kw},{arith},ny={L['ny']},wco={L['wco']},ks={L['ks']},P={L['P']},nu={L['nu']},"
              f"{'fast' if L['fast'] else 'generic'})  max-abs {esp:.2e} rms {rsp:.2e}  relu {erelu:.2e}")
    print(f"  accepted {len(rows)}, refused {len(refused)}: {refused}")
    for cfg, L, esp, rsp, erelu in rows:
        e32, r32 = ref32[min(L["ks"], 2)]
        assert esp <= 2e-5 * max(1.0, scale / 4) and esp <= 1.25 * e32 + 2e-7 * max(1.0, scale), (cfg, L, esp, e32)
        assert rsp <= 1.05 * r32 + 2e-8 * max(1.0, scale), (cfg, L, rsp, r32)
        assert erelu <= 2e-5 * max(1.0, scale / 4), (cfg, L, erelu)
    for key, outs in groups.items():
        for cfg, ny, y in outs[1:]:
            assert torch.equal(y, outs[0][2]), (key, outs[0][:2], (cfg, ny), float((y - outs[0][2]).abs().max()))
    # every ks the layer has chunks for is reachable with at least one ny
    nchunks = cin // 16
    assert {L["ks"] for _, L, *_ in rows} >= {ks for ks in (1, 2, 4) if ks <= nchunks and any(
        ncb // ny * ks <= 12 for ny in _divisors(ncb))}, rows


def test_split_p3_p4_are_refused(monkeypatch, capfd):
    """P = 3 / 4 are not instantiated (conv_split_kernel.h launch_split_shape): forcing them is refused before any launch."""
    from nndepth_amd import ops
    k = (3, 3, 1, 256, 192, "bf16x3")
    w, b, x, _, _ = data(k)
    conv = ops.Conv2d(w, b, arithmetic="bf16x3")
    monkeypatch.setenv("NND_CONV_VERBOSE", "1")
    for cfg in ("0,0,3", "0,0,4", "2,1,3", "1,2,4"):
        monkeypatch.setenv("NND_SPLIT_CFG", cfg)
        y, err = _run(capfd, lambda: conv(x.to(DEV)))
        assert isinstance(y, Exception) and "no configuration" in str(y), (cfg, y)
        assert not split_lines(err), (cfg, err)


# ------------------------------------------------------------------------------------------------ item 2: stride 2, two sources
@pytest.mark.parametrize("B,H,W", [(1, 99, 161), (2, 120, 200)])
@pytest.mark.parametrize("arith", SPLIT_ARITHS)
def test_encoder_split_stride2_every_ks_vs_oracle(monkeypatch, capfd, raft_sd, arith, B, H, W):
    """The stride-2 FAST kernels (the encoder's layer2.0 / layer3.0 conv1 and 1x1 shortcuts) under each forced ks (NND_SPLIT_CFG=0,ks:
    every split layer of the encoder) and the picker, against the oracle's encoder with the bar of test_encoder_small_vs_oracle.  A
    forced ks that a layer cannot take (ks > its chunks, or a stride-2 layer whose chunks ks does not divide: the stride-2 kernels
    exist in the FAST regime only, or LDS) is refused before that layer launches: which ones is asserted."""
    from oracle import torch_ref as R
    from nndepth_amd import ops, weightgen
    fr1, fr2 = weightgen.synthetic_frames(7, B, H, W)
    frames = torch.cat([fr1, fr2], 0)
    enc_sd = {kk[len("fnet."):]: v for kk, v in raft_sd.items() if kk.startswith("fnet.")}
    cnet_sd = {kk[len("cnet_proj."):]: v for kk, v in raft_sd.items() if kk.startswith("cnet_proj.")}
    with torch.no_grad():
        exp = R.basic_encoder(raft_sd, "fnet", frames)
        exp_c = torch.relu(torch.nn.functional.conv2d(exp[:B], raft_sd["cnet_proj.0.weight"], raft_sd["cnet_proj.0.bias"], padding=1))
    accepted, refused = [], []
    for ks in (0, 1, 2, 4):
        if ks:
            monkeypatch.setenv("NND_SPLIT_CFG", f"0,{ks}")
        else:
            monkeypatch.delenv("NND_SPLIT_CFG", raising=False)
        monkeypatch.setenv("NND_CONV_VERBOSE", "1")
        eng = ops.EncoderEngine(256, "batch", 192, arithmetic=arith).load(enc_sd, cnet_sd, device=DEV)

        def fwd():
            if arith == "fp16x2":
                with ops.calibration():
                    eng.forward(frames.to(DEV), n_cnet=B)
            return eng.forward(frames.to(DEV), n_cnet=B)
        out, err = _run(capfd, fwd)
        lines = split_lines(err)
        s2 = [L for L in lines if L["stride"] == 2]
        if isinstance(out, Exception):
            assert ks, f"the picker found no configuration: {out}"
            assert "no configuration" in str(out), str(out)
            refused.append((ks, str(out).splitlines()[0]))
            continue
        assert s2 and all(L["fast"] for L in s2), lines
        if ks:
            assert all(L["ks"] == ks for L in lines), lines
        fm, cnet = out
        e1, e2 = (fm.cpu() - exp).abs().max().item(), (cnet.cpu() - exp_c).abs().max().item()
        cfgs = sorted({(L["KH"], L["Cin"], L["Cout"], L["ny"], L["wco"], L["ks"], L["nu"]) for L in s2})
        print(f"\n[encoder {arith} {B}x{H}x{W} ks={ks or 'picker'}] fmap max-abs {e1:.2e}, cnet {e2:.2e}; stride-2 (K, Cin, Cout, ny, wco, ks, nu): {cfgs}")
        accepted.append(ks)
        assert e1 <= 5e-5 and e2 <= 5e-5, (ks, e1, e2)
    print(f"  accepted ks {accepted}, refused {refused}")
    # stride-2 64 -> 96 (layer2.0) refuses ks = 4, and ks = 2 in bf16x3 (its 3-piece patch needs more than 160 KiB of LDS)
    assert accepted == ([0, 1, 2] if arith == "fp16x2" else [0, 1]), (accepted, refused)
    assert all("3x3 Cin=64 (64+0) Cout=96 stride 2" in m for _, m in refused), refused


UB_CASES = {"raft_h128_c64": (128, 64, 36, 1, 8, "sep_conv", "update_block.npz"),
            "raft_h128_c128": (128, 128, 36, 1, 8, "sep_conv", "update_block.npz"),
            "cre_h128_c128_f2": (128, 128, 36, 2, 8, "sep_conv", "update_block.npz"),
            "igev_h64_c64_cp576": (64, 64, 576, 1, 4, "sep_conv", "update_block.npz"),
            "convgru_h128_c128": (128, 128, 36, 1, 8, "conv_gru", "update_block_conv_gru.npz"),
            "convgru_h64_c64_f2": (64, 64, 36, 2, 4, "conv_gru", "update_block_conv_gru.npz")}
UB_MODES = ["ks1", "ks2", "ks4", "nofast", "noc4"]


@pytest.mark.parametrize("mode", UB_MODES)
@pytest.mark.parametrize("name", list(UB_CASES))
@pytest.mark.parametrize("arith", SPLIT_ARITHS)
def test_update_block_two_source_configs_golden(monkeypatch, capfd, gold, arith, name, mode):
    """The two-source, c4 tile-major launches of the update block under NND_SPLIT_CFG=0,ks (ks 1 / 2 / 4: including the picker's
    c0 % (ks*16) condition on the first source), NND_SPLIT_NO_FAST and NND_NO_C4, against the reference's goldens with the bar of
    test_update_block_golden_split."""
    from oracle import torch_ref as R
    from nndepth_amd import weightgen
    from nndepth_amd.blocks import BasicUpdateBlock
    hid, ctx, cp, fc, sps, gru, npz = UB_CASES[name]
    g = gold(npz)
    pre = "ub." + name
    sd = weightgen.fill_state_dict(R.update_block_spec(pre, hid, cp, ctx, fc, sps, gru=gru))
    monkeypatch.setenv("NND_CONV_VERBOSE", "1")
    if mode.startswith("ks"):
        monkeypatch.setenv("NND_SPLIT_CFG", f"0,{mode[2:]}")
    elif mode == "nofast":
        monkeypatch.setenv("NND_SPLIT_NO_FAST", "1")
    else:
        monkeypatch.setenv("NND_NO_C4", "1")
    ub = BasicUpdateBlock(hidden_dim=hid, cor_planes=cp, context_dim=ctx, flow_channel=fc, spatial_scale=sps, gru=gru, arithmetic=arith)
    ub.load_state_dict({kk[len(pre) + 1:]: v for kk, v in sd.items()})
    ub = ub.to(DEV)
    ins = [t(g[f"{name}_{kk}"]).to(DEV) for kk in ("net", "inp", "corr", "flow")]
    out, err = _run(capfd, lambda: [o.clone() for o in ub(*ins)])
    lines = split_lines(err)
    assert not isinstance(out, Exception), f"{mode} refused: {out}"  # every forced ks exists for every layer of these blocks
    assert lines, err
    if mode.startswith("ks"):
        assert all(L["ks"] == int(mode[2:]) for L in lines), lines
    if mode == "nofast":
        assert not any(L["fast"] for L in lines), lines
    out2 = [o.clone() for o in ub(*ins)]
    cfgs = sorted({(L["KH"], L["KW"], L["Cin"], L["Cout"], L["ny"], L["wco"], L["ks"], L["nu"], L["fast"]) for L in lines})
    print(f"\n[update block {name} {arith} {mode}] (KH, KW, Cin, Cout, ny, wco, ks, nu, fast): {cfgs}")
    for got, again, key in zip(out, out2, ("net_out", "mask_out", "delta_out")):
        exp = g[f"{name}_{key}"]
        e = np.abs(got.cpu().numpy() - exp).max()
        print(f"  {key}: max-abs {e:.2e} (|exp| max {np.abs(exp).max():.2f})")
        assert torch.equal(got, again), key
        assert e <= 2e-5 * max(1.0, np.abs(exp).max()), (key, e)


# ------------------------------------------------------------------------------------------------ item 3: exact kernel
@pytest.mark.parametrize("k", EXACT_CLASSES, ids=cls_id)
def test_exact_every_configuration_vs_float64(monkeypatch, capfd, k):
    """Every NND_CONV_CFG=1,ks,wco (ks 1 / 2, wco 8 / 6 / 4 / 3 / 2 / 1) and the picker's own choice, ops.Conv2d at stride 1 and
    ops.ConvNorm at stride 2: max-abs vs float64 within 1.25x that of the same sums in fp32 chains of the kernel's length
    (chain_fp32_error) plus 1e-7 |y|max; two runs torch.equal.  PyTorch's own fp32 CPU convolution error is printed beside it: it
    blocks its sums, and is 3-7x below any sequential fp32 chain of 600-2300 products (measured: 3x3 256 -> 192, PyTorch 3.5e-6,
    the exact kernel 2.5e-5 with ks = 1 and 1.6e-5 with ks = 2 for every wco), so it cannot be the bar of an fp32 fmaf chain."""
    from nndepth_amd import ops
    kh, kw, st, cin, cout, _ = k
    w, b, x, truth, scale = data(k)
    xd = x.to(DEV)
    ecpu = (torch.nn.functional.conv2d(x, w, b, stride=st, padding=(kh // 2, kw // 2)).double() - truth).abs().max().item()
    conv = ops.Conv2d(w, b) if st == 1 else ops.ConvNorm(w, b, stride=st, device=DEV)
    rows, refused = [], []
    for cfg in [None] + [f"1,{ks},{wco}" for ks in (1, 2) for wco in (8, 6, 4, 3, 2, 1)]:
        monkeypatch.setenv("NND_CONV_VERBOSE", "1")
        if cfg is None:
            monkeypatch.delenv("NND_CONV_CFG", raising=False)
        else:
            monkeypatch.setenv("NND_CONV_CFG", cfg)
        y, err = _run(capfd, lambda: conv(xd))
        lines = conv_lines(err)
        if isinstance(y, Exception):
            assert cfg is not None, f"the picker found no configuration: {y}"
            assert "no tile configuration" in str(y) and "p=1 ks=%s wco=%s" % tuple(cfg.split(",")[1:]) in str(y), str(y)
            assert not lines and not STREAM_RE.search(err), (cfg, err)
            refused.append(cfg)
            continue
        assert len(lines) == 1, err
        L = lines[0]
        assert (L["KH"], L["KW"], L["Cin"], L["Cout"], L["stride"]) == (kh, kw, cin, cout, st), L
        if cfg is not None:
            assert (L["P"], L["ks"], L["wco"]) == tuple(int(v) for v in cfg.split(",")), (cfg, L)
        y, y2 = y.cpu(), conv(xd).cpu()
        assert torch.equal(y, y2), (cfg, "run to run")
        rows.append((cfg or "picker", L, errs(y, truth)[0], chain_fp32_error(k, L["ks"], L["CI_T"])))
    print(f"\n[exact {cls_id(k)} {LAYERS[k]}] PyTorch fp32 CPU max-abs {ecpu:.2e}   |y| max {scale:.1f}")
    for cfg, L, e, eseq in rows:
        print(f"  {cfg:>8}  (P={L['P']},wco={L['wco']},ks={L['ks']},ne={L['ne']},CI_T={L['CI_T']})  max-abs {e:.2e}  fp32 chains {eseq:.2e}")
    print(f"  accepted {len(rows)}, refused {len(refused)}: {refused}")
    assert len(rows) >= 2, rows
    for cfg, L, e, eseq in rows:
        assert e <= 1.25 * eseq + 1e-7 * scale, (cfg, L, e, eseq, ecpu)


def test_exact_kernel_runs_both_ne_instantiations(monkeypatch, capfd):
    """NE (patch elements per staging thread: the NE = 8 or NE = 16 instantiation) follows from wco, ks and the kernel size: among the
    configurations the sweep above accepts, both instantiations run."""
    from nndepth_amd import ops
    ne = set()
    for k in [(3, 3, 1, 256, 192, "fp32"), (1, 1, 1, 200, 96, "fp32"), (1, 5, 1, 48, 64, "fp32")]:
        w, b, x, _, _ = data(k)
        conv = ops.Conv2d(w, b)
        monkeypatch.setenv("NND_CONV_VERBOSE", "1")
        for cfg in [f"1,{ks},{wco}" for ks in (1, 2) for wco in (8, 6, 4, 3, 2, 1)]:
            monkeypatch.setenv("NND_CONV_CFG", cfg)
            y, err = _run(capfd, lambda: conv(x.to(DEV)))
            ne |= {L["ne"] for L in conv_lines(err)}
    print(f"\nne values run: {sorted(ne)}")
    assert any(v <= 8 for v in ne) and any(8 < v <= 16 for v in ne), ne


# ------------------------------------------------------------------------------------------------ item 4: the 1x1 stream kernel
@pytest.mark.parametrize("B,H,W", [(1, 24, 40), (2, 13, 22)])
def test_conv1x1_stream_encoder_output_conv(monkeypatch, capfd, raft_sd, B, H, W):
    """conv_mfma.hip's streaming 1x1 kernel (launch_conv1x1_stream: stride 1, one tile-major source, Cin 64 / 96 / 128).  The
    production layers that take it, from NND_CONV_VERBOSE runs of the four model families in fp32 (RAFT-Stereo, CREStereo, IGEV,
    Coarse2Fine; their update blocks' module forward): the BasicEncoder's stride-1 1x1 convs 64 -> 64, 96 -> 96, 128 -> 128 and its
    output conv 128 -> 256 (RAFT-Stereo, CREStereo), and mask.2 of a 64-channel hidden state, 128 -> 144, in the update block's
    module forward (IGEV; the refinement loops run mask.2 inside the fused upsample kernel).  Through the encoder: against the oracle (the bar of test_encoder_small_vs_oracle) and against NND_NO_CONV1X1_STREAM=1 (the same layer on the
    tiled kernel: same products, another summation order)."""
    from oracle import torch_ref as R
    from nndepth_amd import ops, weightgen
    fr1, fr2 = weightgen.synthetic_frames(11, B, 8 * H, 8 * W)
    frames = torch.cat([fr1, fr2], 0)
    enc_sd = {kk[len("fnet."):]: v for kk, v in raft_sd.items() if kk.startswith("fnet.")}
    with torch.no_grad():
        exp = R.basic_encoder(raft_sd, "fnet", frames)
    outs = {}
    for mode in ("stream", "tiled"):
        monkeypatch.setenv("NND_CONV_VERBOSE", "1")
        if mode == "tiled":
            monkeypatch.setenv("NND_NO_CONV1X1_STREAM", "1")
        eng = ops.EncoderEngine(256, "batch", 0).load(enc_sd, device=DEV)
        out, err = _run(capfd, lambda: eng.forward(frames.to(DEV))[0].clone())
        assert not isinstance(out, Exception), out
        streams = [(int(m[1]), int(m[2])) for m in STREAM_RE.finditer(err)]
        assert sorted(set(streams)) == ([(64, 64), (96, 96), (128, 128), (128, 256)] if mode == "stream" else []), (mode, streams)
        outs[mode] = out.cpu()
    e_s, e_t = ((outs[m] - exp).abs().max().item() for m in ("stream", "tiled"))
    print(f"\n[conv1x1 stream, encoder {B}x{8 * H}x{8 * W}] max-abs vs oracle: stream {e_s:.2e}, tiled kernel {e_t:.2e}")
    assert e_s <= 5e-5 and e_t <= 5e-5
    assert (outs["stream"] - outs["tiled"]).abs().max().item() <= 2e-5 * max(1.0, exp.abs().max().item())


# ------------------------------------------------------------------------------------------------ item 5: coverage guard
# the refinement loops of the four model families: (hidden, cor_planes, context, flow channels, gru) and the loop resolutions
# (B, H, W) of their workloads
FAMILIES = {
    "raft": ((128, 36, 64, 1, "sep_conv"), {"raft 544x960": (1, 68, 120), "raft kitti batch 8": (8, 48, 156)}),
    "cre": ((128, 36, 128, 2, "sep_conv"), {"cre 1080x1920 stage 1/8": (1, 135, 240), "cre stage 1/16": (1, 67, 120),
                                            "cre stage 1/32": (1, 33, 60)}),
    "igev": ((64, 576, 64, 1, "sep_conv"), {"igev 136x240": (1, 136, 240), "igev 136x240 batch 8": (8, 136, 240)}),
    "c2f": ((128, 36, 128, 1, "conv_gru"), {"c2f 512x960 stage 0": (1, 8, 15), "c2f stage 1": (1, 32, 60), "c2f stage 2": (1, 128, 240)}),
}
ALL_ARITHS = ("fp32",) + SPLIT_ARITHS


def loop_layers(family, arith, capfd, monkeypatch):
    """Run two iterations of the family's refinement loop on a small map with NND_CONV_VERBOSE: the (KH, KW, Cin, Cout, kernel
    arithmetic) of every launch that goes through a picker (the fused lookup / flow-branch / mask-upsample kernels do not)."""
    from nndepth_amd import ops, weightgen
    from nndepth_amd.blocks import BasicUpdateBlock
    from nndepth_amd.cost_volume import CorrBlock1D
    (hid, cp, ctx, fc, gru), _ = FAMILIES[family]
    sps = {"raft": 8, "cre": 8, "igev": 4, "c2f": (4, 4)}[family]
    ub = BasicUpdateBlock(hidden_dim=hid, cor_planes=cp, context_dim=ctx, flow_channel=fc, spatial_scale=sps, gru=gru, arithmetic=arith)
    weightgen.fill_module_(ub, "cov.update_block.")
    eng = ub.to(DEV).eval().sync_engine(DEV)
    torch.manual_seed(61)
    B, H, W = 1, 12, 24
    net, inp = torch.tanh(torch.randn(B, hid, H, W)).to(DEV), torch.relu(torch.randn(B, ctx, H, W)).to(DEV)
    monkeypatch.setenv("NND_CONV_VERBOSE", "1")

    def run():
        if family == "raft":
            f1, f2 = torch.randn(B, 256, H, W, device=DEV), torch.randn(B, 256, H, W, device=DEV)
            return eng.refine(CorrBlock1D(f1, f2, 4, 4)._pyr, 4, 4, net, inp, 8, 2)
        if family == "cre":
            f1, f2 = torch.randn(B, 256, H, W, device=DEV), torch.randn(B, 256, H, W, device=DEV)
            return eng.refine_cre(f1, f2, net, inp, 8, 2)
        if family == "igev":
            G = 8
            fp_ = ops.group_corr_build(torch.randn(B, 64, H, W, device=DEV), torch.randn(B, 64, H, W, device=DEV), G, 8, 4)
            gp_ = ops.group_corr_build(torch.randn(B, 64, H, W, device=DEV), torch.randn(B, 64, H, W, device=DEV), G, 8, 4)
            return eng.refine_igev(fp_, gp_, G, 4, 4, net, inp, 4, 2, disp_init=torch.rand(B, 1, H, W, device=DEV) * 3)
        gpyr = ops.raft_group_corr_build(torch.randn(B, 64, H, W, device=DEV), torch.randn(B, 64, H, W, device=DEV), 4, 1)
        return eng.refine_group(gpyr, 4, 1, 4, net, inp, 4, 2)
    out, err = _run(capfd, run)
    monkeypatch.delenv("NND_CONV_VERBOSE")
    assert not isinstance(out, Exception), out
    names = {"2": "fp16x2", "3": "bf16x3"}
    layers = {(L["KH"], L["KW"], L["Cin"], L["Cout"], names[str(L["pieces"])]) for L in split_lines(err)}
    layers |= {(L["KH"], L["KW"], L["Cin"], L["Cout"], "fp32") for L in conv_lines(err)}
    return sorted(layers)


@pytest.mark.parametrize("arith", ALL_ARITHS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_loop_layer_picks_a_verified_configuration(monkeypatch, capfd, family, arith):
    """For every layer the family's refinement loop launches through a picker (found by running the loop with NND_CONV_VERBOSE, so a
    change of the models' shapes shows up here) and every workload's loop resolution: one ops.Conv2d call with NND_CONV_VERBOSE
    records the configuration the picker chooses there, and
      - the layer's class (KH, KW, stride 1, Cin, Cout, kernel arithmetic) is in LAYERS, which items 1 and 3 sweep exhaustively;
      - that configuration, forced on the class' sweep shape, is accepted and gives the same tile shape (split: ny, wco, ks, P, nu,
        FAST; exact: P, wco, ks, ne): a configuration items 1 / 3 compare against float64.
    A one-source NCHW call (ops.Conv2d) can pick differently from the loop's own two-source c4 tile-major call of the same layer (the
    picker's c0 % (ks*16) condition; the FAST regime per source): those calls are what test_update_block_two_source_configs_golden
    covers under every forced ks.  Layers of the encoders and of the Conv3d volumes are not loop layers and are not checked here."""
    from nndepth_amd import ops
    layers = loop_layers(family, arith, capfd, monkeypatch)
    assert layers, f"{family} {arith}: the loop launched no picked conv"
    _, workloads = FAMILIES[family]
    missing, unverified, seen = [], [], {}
    for (kh, kw, cin, cout, ka) in layers:
        k = (kh, kw, 1, cin, cout, ka)
        if k not in LAYERS:
            missing.append(f"{cls_id(k)} (launched by the {family} loop in {arith}; workloads {', '.join(workloads)})")
            continue
        torch.manual_seed(0)
        w, b = torch.randn(cout, cin, kh, kw) * 0.01, torch.zeros(cout)
        conv = ops.Conv2d(w, b, arithmetic=ka)
        for wl, (B, H, W) in workloads.items():
            monkeypatch.delenv("NND_SPLIT_CFG", raising=False)
            monkeypatch.delenv("NND_CONV_CFG", raising=False)
            monkeypatch.setenv("NND_CONV_VERBOSE", "1")
            x = torch.zeros(B, cin, H, W, device=DEV)
            y, err = _run(capfd, lambda: conv(x))
            del x
            assert not isinstance(y, Exception), (wl, k, y)
            if ka == "fp32":
                (L,) = conv_lines(err)
                cfg, env, fields = f"1,{L['ks']},{L['wco']}", "NND_CONV_CFG", ("P", "wco", "ks", "ne")
            else:
                (L,) = split_lines(err)
                cfg, env, fields = f"{L['ny']},{L['ks']},{L['P']}", "NND_SPLIT_CFG", ("ny", "wco", "ks", "P", "nu", "fast")
            picked = tuple(L[f] for f in fields)
            monkeypatch.setenv(env, cfg)
            xs = data(k)[2].to(DEV)
            y2, err2 = _run(capfd, lambda: conv(xs))
            forced = (conv_lines if ka == "fp32" else split_lines)(err2)
            ok = not isinstance(y2, Exception) and len(forced) == 1 and tuple(forced[0][f] for f in fields) == picked
            seen.setdefault((cls_id(k), dict(zip(fields, picked)).__repr__()), []).append(wl)
            if not ok:
                unverified.append(f"{wl}: {cls_id(k)} picks {dict(zip(fields, picked))}, not accepted as such on {LAYERS[k]}: "
                                  f"{y2 if isinstance(y2, Exception) else forced}")
    print(f"\n[coverage {family} {arith}] {len(layers)} loop layers, picked configurations:")
    for (cid, c), wls in sorted(seen.items()):
        print(f"  {cid:>26} {c}  verified  ({', '.join(wls)})")
    assert not missing, "loop layers whose class is not swept by items 1 / 3: " + "; ".join(missing)
    assert not unverified, "picked configurations no sweep verifies: " + "; ".join(unverified)


@pytest.mark.parametrize("hid,cp,ctx,sps", [(128, 64, 64, 8), (128, 96, 64, 8), (64, 128, 64, 4)])
def test_conv1x1_stream_update_block_vs_float64(monkeypatch, capfd, hid, cp, ctx, sps):
    """The streaming 1x1 kernel inside the update block's forward (fp32, tile-major workspace): encoder.convc1 (cor_planes -> 256)
    with Cin 64 / 96 / 128, and mask.2 of a 64-channel hidden state (128 -> 9 * 4 * 4 = 144 channels: a Cout that is not a multiple
    of 32, as in IGEV), against the float64 evaluation of the reference's update block and against NND_NO_CONV1X1_STREAM=1, with
    the bar of test_update_block_golden_split.  Ragged 13x22 map, batch 2."""
    from oracle import torch_ref as R
    from nndepth_amd import weightgen
    from nndepth_amd.blocks import BasicUpdateBlock
    pre = "ub.stream"
    sd = weightgen.fill_state_dict(R.update_block_spec(pre, hid, cp, ctx, 1, sps))
    g = torch.Generator().manual_seed(hid + cp)
    B, H, W = 2, 13, 22
    ins = [torch.tanh(torch.randn(B, hid, H, W, generator=g)), torch.relu(torch.randn(B, ctx, H, W, generator=g)),
           torch.randn(B, cp, H, W, generator=g), torch.randn(B, 1, H, W, generator=g) * 4]
    with torch.no_grad():
        truth = R.update_block({kk: v.double() for kk, v in sd.items()}, pre, *(i.double() for i in ins))
    outs = {}
    for mode in ("stream", "tiled"):
        monkeypatch.setenv("NND_CONV_VERBOSE", "1")
        if mode == "tiled":
            monkeypatch.setenv("NND_NO_CONV1X1_STREAM", "1")
        ub = BasicUpdateBlock(hidden_dim=hid, cor_planes=cp, context_dim=ctx, flow_channel=1, spatial_scale=sps, arithmetic="fp32")
        ub.load_state_dict({kk[len(pre) + 1:]: v for kk, v in sd.items()})
        ub = ub.to(DEV)
        out, err = _run(capfd, lambda: [o.clone() for o in ub(*(i.to(DEV) for i in ins))])
        assert not isinstance(out, Exception), out
        streams = sorted((int(m[1]), int(m[2])) for m in STREAM_RE.finditer(err))
        want = sorted([(cp, 256)] + ([(2 * hid, 9 * sps * sps)] if 2 * hid in (64, 96, 128) else []))
        assert streams == (want if mode == "stream" else []), (mode, streams, want)
        outs[mode] = [o.cpu().double() for o in out]
    for j, key in enumerate(("net_out", "mask_out", "delta_out")):
        sc = max(1.0, truth[j].abs().max().item())
        e_s, e_t = ((outs[m][j] - truth[j]).abs().max().item() for m in ("stream", "tiled"))
        d = (outs["stream"][j] - outs["tiled"][j]).abs().max().item()
        print(f"\n[conv1x1 stream, update block hid {hid} cp {cp}] {key}: max-abs vs float64 stream {e_s:.2e}, tiled {e_t:.2e}, "
              f"stream - tiled {d:.2e}")
        assert e_s <= 2e-5 * sc and e_t <= 2e-5 * sc and d <= 2e-5 * sc, (key, e_s, e_t, d)
