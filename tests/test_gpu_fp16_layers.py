"""GPU: the one-piece fp16 arithmetic on the layers only the engines launch, ONE LAUNCH AT A TIME, against the contract.

tests/test_gpu_fp16_conv.py holds ops.Conv2d (one planar source, stride 1) to the contract gate.  This file does the same for
  - the update block's own launches (nnd_update_block_layer_forward): 4-channel-interleaved tile-major sources, two sources (the GRU's
    q conv: r*h | inp, motion, flow), the GRU z / r and q epilogues, the context bias maps of the loop's GRU convs, ReLU, mask.2's
    0.25 scale, Cin 64 / 128 / 192 / 256 / 320;
  - the encoder's layers (nnd_conv_forward_ex): 3x3 at stride 1 and 2, the stride-2 1x1 shortcut (Cout >= 96), folded BatchNorm + ReLU,
    residual add + ReLU, planar and in the encoder's 4-channel-interleaved layout; 2x26x44 inputs for stride 2;
under the picker's choice, every forced split-K (NND_SPLIT_CFG=0,ks), NND_SPLIT_NO_FAST and (block) NND_NO_C4.

Contract: y_c = epilogue(oscale * sum x^ w^ ...) in float64, x^ = fp16_rne(x * 2^xs), w^ = fp16_rne(w * 2^s) rounded on the host with the
scales read back from the blob.  Gate: the same launch in exact fp32 on the pre-rounded operands (x^ / 2^xs, w^ / 2^s) computes the
same sums with fp32 accumulation; the one-piece launch's max-abs and rms error against the contract are at most 2 x that launch's.
Every plan line says pieces=1, two runs are bit-identical, an activation of 64 x the calibrated maximum or a NaN gives non-finite
values in every output that reads it and changes no other."""
import ctypes as C

import pytest
import torch

from fp16_report import report_section
from test_gpu_fp16_conv import _log_uniform, _run, errs, split_lines

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARK = "== single launches of the engines (tests/test_gpu_fp16_layers.py)\n"
B, H, W = 2, 13, 22
_lines = {}
F = torch.nn.functional


@pytest.fixture(autouse=True)
def _keep_global_rng():
    cpu, dev = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    yield
    torch.set_rng_state(cpu)
    torch.cuda.set_rng_state(dev, DEV)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _lines:
        report_section(MARK, [_lines[k] for k in sorted(_lines)])


def _p(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def _half(x, scale):
    """x^ / scale: the value the kernel multiplies, as float64"""
    return (x.float() * scale).half().double() / scale


# ------------------------------------------------------------------------------------------------ the update block's launches
NAMES = ["C1", "CF", "HX", "Z", "RH", "FM", "CTXB", "MASK"]
IDS = {"convc2": 1, "conv": 3, "zr1x": 4, "q1x": 5, "zr2x": 6, "q2x": 7, "fhm": 8, "mask2": 9, "zr1": 10, "q1": 11, "zr2": 12, "q2": 13,
       "zr1c": 14, "q1c": 15}
BLOCKS = {"h128_c64": dict(hid=128, ctx=64, gru="sep_conv", rate=8), "h64_cg": dict(hid=64, ctx=64, gru="conv_gru", rate=4)}
LAYERS = [("h128_c64", k) for k in ("convc2", "conv", "fhm", "mask2", "zr1", "q1", "zr2", "q2", "zr1x", "q1x", "zr1c")] + \
         [("h64_cg", k) for k in ("conv", "fhm", "mask2", "zr1", "q1", "q1x")]


def _block(name, arith, sd=None, flags=0):
    from nndepth_amd import ops, weightgen
    from oracle import torch_ref as R
    c = BLOCKS[name]
    if sd is None:
        sd = weightgen.fill_state_dict(R.update_block_spec("lay." + name, c["hid"], 36, c["ctx"], 1, c["rate"], gru=c["gru"]))
        sd = {k[len("lay." + name) + 1:]: v for k, v in sd.items()}
    eng = ops.UpdateBlockEngine(c["hid"], c["ctx"], 36, 1, 9 * c["rate"] ** 2, c["gru"], arith)
    eng.load(sd, "", device=DEV)
    return eng, sd


def _tensors(name):
    """The workspace tensors of a block as the launches find them: activations of their kinds, magnitudes over several octaves."""
    c = BLOCKS[name]
    hid, ctx = c["hid"], c["ctx"]
    g = torch.Generator().manual_seed(hid * 7 + ctx)
    t = {"C1": _log_uniform((B, 256, H, W), -6, 1, g).abs(), "CF": _log_uniform((B, 256, H, W), -6, 1, g).abs(),
         "HX": torch.cat([torch.tanh(torch.randn(B, hid, H, W, generator=g)), _log_uniform((B, ctx, H, W), -6, 1, g).abs(),
                          _log_uniform((B, hid - 1, H, W), -6, 1, g).abs(), torch.randn(B, 1, H, W, generator=g) * 4], 1),
         "Z": torch.sigmoid(torch.randn(B, hid, H, W, generator=g)), "RH": torch.tanh(torch.randn(B, hid, H, W, generator=g)) * 0.7,
         "FM": _log_uniform((B, 3 * hid, H, W), -6, 1, g).abs(), "CTXB": torch.randn(B, 6 * hid, H, W, generator=g)}
    return t


def _weights(name, layer, sd):
    """(weight, bias or None) of the launch, in its own input-channel order"""
    c = BLOCKS[name]
    hid, ctx = c["hid"], c["ctx"]
    cat = torch.cat
    p = "1" if layer[-2 if layer[-1] in "xc" else -1] == "1" else "2"
    if layer == "convc2":
        return sd["encoder.convc2.weight"], sd["encoder.convc2.bias"]
    if layer == "conv":
        return sd["encoder.conv.weight"], sd["encoder.conv.bias"]
    if layer == "fhm":
        return cat([sd["flow_head.conv1.weight"], sd["mask.0.weight"]]), cat([sd["flow_head.conv1.bias"], sd["mask.0.bias"]])
    if layer == "mask2":
        return sd["mask.2.weight"], sd["mask.2.bias"]
    wz, wr, wq = (sd[f"gru.conv{k}{p}.weight"] for k in "zrq")
    bz, br, bq = (sd[f"gru.conv{k}{p}.bias"] for k in "zrq")
    hm = list(range(hid)) + list(range(hid + ctx, 2 * hid + ctx))  # [h | motion, flow] of [h | inp | motion, flow]
    inp = list(range(hid, hid + ctx))
    if layer.startswith("zr"):
        w, b = cat([wz, wr]), cat([bz, br])
    else:
        w, b = wq, bq
    if layer.endswith("x"):
        return w[:, hm].contiguous(), None  # the context term and the bias arrive as the bias map
    if layer.endswith("c"):
        return w[:, inp].contiguous(), b
    return w, b


def _contract(name, layer, w, b, t, xs, ws, rnd):
    """float64 outputs {tensor name: value} of the launch on the tensors t; rnd: round the conv's operands to one fp16 piece."""
    c = BLOCKS[name]
    hid, ctx = c["hid"], c["ctx"]
    d = {k: v.double() for k, v in t.items()}
    r = (lambda x: _half(x, xs)) if rnd else (lambda x: x.double())
    w64 = _half(w, ws) if rnd else w.double()
    pad = (w.shape[2] // 2, w.shape[3] // 2)
    conv = lambda x: F.conv2d(r(x), w64, None if b is None else b.double(), padding=pad)  # noqa: E731
    h = d["HX"][:, :hid]
    if layer == "convc2":
        cf = d["CF"].clone()
        cf[:, :192] = conv(t["C1"]).clamp_min(0)
        return {"CF": cf}
    if layer == "conv":
        hx = d["HX"].clone()
        hx[:, hid + ctx:2 * hid + ctx - 1] = conv(t["CF"]).clamp_min(0)
        return {"HX": hx}
    if layer == "fhm":
        return {"FM": conv(t["HX"][:, :hid]).clamp_min(0)}
    if layer == "mask2":
        return {"MASK": 0.25 * conv(t["FM"][:, hid:])}
    if layer in ("zr1", "zr2", "zr1x", "zr2x"):
        if layer.endswith("x"):
            v = conv(torch.cat([t["HX"][:, :hid], t["HX"][:, hid + ctx:]], 1)) + d["CTXB"][:, (0 if layer == "zr1x" else 3 * hid):][:, :2 * hid]
        else:
            v = conv(t["HX"])
        return {"Z": torch.sigmoid(v[:, :hid]), "RH": torch.sigmoid(v[:, hid:]) * h}
    if layer in ("q1", "q2", "q1x", "q2x"):
        if layer.endswith("x"):
            v = conv(torch.cat([t["RH"], t["HX"][:, hid + ctx:]], 1)) + d["CTXB"][:, (2 * hid if layer == "q1x" else 5 * hid):][:, :hid]
        else:
            v = conv(torch.cat([t["RH"], t["HX"][:, hid:]], 1))
        hx = d["HX"].clone()
        hx[:, :hid] = (1 - d["Z"]) * h + d["Z"] * torch.tanh(v)
        return {"HX": hx}
    if layer in ("zr1c", "q1c"):
        cb = d["CTXB"].clone()
        o, n = (0, 2 * hid) if layer == "zr1c" else (2 * hid, hid)
        cb[:, o:o + n] = conv(t["HX"][:, hid:hid + ctx])
        return {"CTXB": cb}
    raise KeyError(layer)


def _sources(name, layer):
    """{tensor name: channel slice} the launch's conv reads"""
    c = BLOCKS[name]
    hid, ctx = c["hid"], c["ctx"]
    return {"convc2": {"C1": slice(None)}, "conv": {"CF": slice(None)}, "fhm": {"HX": slice(0, hid)}, "mask2": {"FM": slice(hid, None)},
            "zr1": {"HX": slice(None)}, "zr2": {"HX": slice(None)}, "q1": {"RH": slice(None), "HX": slice(hid, None)},
            "q2": {"RH": slice(None), "HX": slice(hid, None)}, "zr1x": {"HX": [slice(0, hid), slice(hid + ctx, None)]},
            "q1x": {"RH": slice(None), "HX": slice(hid + ctx, None)}, "zr1c": {"HX": slice(hid, hid + ctx)},
            "q1c": {"HX": slice(hid, hid + ctx)}}[layer]


def _launch(eng, which, t, want, flags=0):
    from nndepth_amd._lib import lib
    from nndepth_amd.ops import _stream, check
    d = type(eng.desc).from_buffer_copy(eng.desc)
    d.flags = flags
    dev = {k: v.to(DEV).contiguous() for k, v in t.items()}
    ins = (C.c_void_p * 8)(*[dev[k].data_ptr() if k in dev else None for k in NAMES])
    c = BLOCKS_OF[id(eng)]
    shapes = {"C1": 256, "CF": 256, "HX": 2 * c["hid"] + c["ctx"], "Z": c["hid"], "RH": c["hid"], "FM": 3 * c["hid"], "CTXB": 6 * c["hid"],
              "MASK": 9 * c["rate"] ** 2}
    outs = {k: torch.empty((B, shapes[k], H, W), dtype=torch.float32, device=DEV) for k in want}
    op = (C.c_void_p * 8)(*[outs[k].data_ptr() if k in outs else None for k in NAMES])
    ws = eng.workspace(B, H, W, DEV)
    check(lib.nnd_update_block_layer_forward(C.byref(d), _p(eng.packed), which, ins, op, _p(ws), B, H, W, _stream(torch.device(DEV))),
          "update_block_layer_forward")
    return outs


BLOCKS_OF = {}


@pytest.mark.parametrize("name,layer", LAYERS, ids=[f"{n}-{k}" for n, k in LAYERS])
def test_update_block_launch_vs_contract(monkeypatch, capfd, name, layer):
    from nndepth_amd._lib import NND_FLAG_CALIBRATE, NndError, lib
    from nndepth_amd.ops import _stream, check
    which = IDS[layer]
    t = _tensors(name)
    eng, sd = _block(name, "fp16")
    BLOCKS_OF[id(eng)] = BLOCKS[name]
    w, b = _weights(name, layer, sd)
    want = list(_contract(name, layer, w, b, t, 1.0, 1.0, False))
    _launch(eng, which, t, want, NND_FLAG_CALIBRATE)
    check(lib.nnd_update_block_calibration_finish(C.byref(eng.desc), _p(eng.packed), None, _stream(torch.device(DEV))), "finish")
    n = int(lib.nnd_update_block_scale_slots(C.byref(eng.desc), None, 0))
    offs = (C.c_int64 * n)()
    lib.nnd_update_block_scale_slots(C.byref(eng.desc), offs, n)
    assert offs[which] >= 0, "the layer is not in one piece"
    tail = eng.packed[offs[which]:offs[which] + 4].cpu()
    xs, ws = tail[1].item(), 1.0 / tail[3].item()
    assert tail[0].item() == tail[3].item() / xs and xs != 4.0
    y_c = _contract(name, layer, w, b, t, xs, ws, True)
    # the same launch in exact fp32 on the pre-rounded operands: weights w^ / 2^s in the state dict, sources x^ / 2^xs in the tensors
    t32 = {k: v.clone() for k, v in t.items()}
    for k, sl in _sources(name, layer).items():
        for s_ in (sl if isinstance(sl, list) else [sl]):
            t32[k][:, s_] = _half(t[k][:, s_], xs).float()
    w32 = _half(w, ws).float()
    y_c32 = _contract(name, layer, w32, b, t32, 1.0, 1.0, False)
    sd32 = dict(sd)
    _put_back(name, layer, sd32, w32)
    exact, _ = _block(name, "fp32", sd32)
    BLOCKS_OF[id(exact)] = BLOCKS[name]
    o32 = _launch(exact, which, t32, want)
    e32 = {k: errs(o32[k].cpu(), y_c32[k]) for k in want}
    rows, refused = [], []
    for cfg in (None, "0,1", "0,2", "0,4", "nofast", "noc4"):
        for v in ("NND_SPLIT_CFG", "NND_SPLIT_NO_FAST", "NND_NO_C4"):
            monkeypatch.delenv(v, raising=False)
        monkeypatch.setenv("NND_CONV_VERBOSE", "1")
        if cfg == "nofast":
            monkeypatch.setenv("NND_SPLIT_NO_FAST", "1")
        elif cfg == "noc4":
            monkeypatch.setenv("NND_NO_C4", "1")
        elif cfg:
            monkeypatch.setenv("NND_SPLIT_CFG", cfg)
        out, err = _run(capfd, lambda: _launch(eng, which, t, want))
        if isinstance(out, NndError):
            assert cfg and cfg[0] == "0" and "no configuration" in str(out), (cfg, out)
            refused.append(cfg)
            continue
        (L,) = split_lines(err)
        assert L["pieces"] == 1 and (cfg is None or cfg[0] != "0" or L["ks"] == int(cfg[2])) and (cfg != "nofast" or not L["fast"]), (cfg, L)
        again = _launch(eng, which, t, want)
        assert all(torch.equal(out[k], again[k]) for k in want), (cfg, "run to run")
        rows.append((cfg or "picker", L, {k: errs(out[k].cpu(), y_c[k]) for k in want}))
    for v in ("NND_SPLIT_CFG", "NND_SPLIT_NO_FAST", "NND_NO_C4"):
        monkeypatch.delenv(v, raising=False)
    txt = f"{name} {layer}: exact fp32 launch on the rounded operands " + " ".join(f"{k} max-abs {e[0]:.2e} rms {e[1]:.2e}" for k, e in e32.items()) + f"; refused {refused}\n"
    for cfg, L, e in rows:
        txt += (f"    {cfg:>7} {L['KH']}x{L['KW']} {L['Cin']}->{L['Cout']} ny={L['ny']} wco={L['wco']} ks={L['ks']} nu={L['nu']} {'fast' if L['fast'] else 'generic'}  "
                + " ".join(f"{k} max-abs {v[0]:.2e} rms {v[1]:.2e}" for k, v in e.items()) + "\n")
    print("\n" + txt, end="")
    _lines[(0, LAYERS.index((name, layer)))] = txt
    assert len(rows) >= 3
    for cfg, L, e in rows:
        for k in want:
            assert e[k][0] <= 2 * e32[k][0] and e[k][1] <= 2 * e32[k][1], (cfg, k, e[k], e32[k])


def _put_back(name, layer, sd, w):
    """The state dict with the launch's weights replaced by w (in the launch's channel order)."""
    c = BLOCKS[name]
    hid, ctx = c["hid"], c["ctx"]
    if layer in ("convc2", "conv"):
        sd["encoder." + layer + ".weight"] = w
    elif layer == "fhm":
        sd["flow_head.conv1.weight"], sd["mask.0.weight"] = w[:hid].contiguous(), w[hid:].contiguous()
    elif layer == "mask2":
        sd["mask.2.weight"] = w
    else:
        p = "1" if "1" in layer else "2"
        keys = ["z", "r"] if layer.startswith("zr") else ["q"]
        cols = {"x": list(range(hid)) + list(range(hid + ctx, 2 * hid + ctx)), "c": list(range(hid, hid + ctx))}.get(layer[-1])
        for i, k in enumerate(keys):
            full = sd[f"gru.conv{k}{p}.weight"].clone()
            part = w[i * hid:(i + 1) * hid]
            if cols is None:
                full = part.contiguous()
            else:
                full[:, cols] = part
            sd[f"gru.conv{k}{p}.weight"] = full


@pytest.mark.parametrize("name,layer", [("h128_c64", "q1"), ("h64_cg", "fhm")])
def test_update_block_launch_out_of_range_and_nan(name, layer):
    from nndepth_amd._lib import NND_FLAG_CALIBRATE, lib
    from nndepth_amd.ops import _stream, check
    which = IDS[layer]
    t = _tensors(name)
    eng, sd = _block(name, "fp16")
    BLOCKS_OF[id(eng)] = BLOCKS[name]
    w, b = _weights(name, layer, sd)
    want = list(_contract(name, layer, w, b, t, 1.0, 1.0, False))
    _launch(eng, which, t, want, NND_FLAG_CALIBRATE)
    check(lib.nnd_update_block_calibration_finish(C.byref(eng.desc), _p(eng.packed), None, _stream(torch.device(DEV))), "finish")
    base = {k: v.clone() for k, v in _launch(eng, which, t, want).items()}
    assert all(torch.isfinite(v).all() for v in base.values())
    src, sl = next(iter(_sources(name, layer).items()))
    amax = max(t[k][:, s_].abs().max().item() for k, ss in _sources(name, layer).items() for s_ in (ss if isinstance(ss, list) else [ss]))
    kh, kw = w.shape[2:]
    bi, ci, yi, xi = 1, 5, 6, 10
    hid = BLOCKS[name]["hid"]
    for bad in (64.0 * amax, float("nan")):
        t2 = {k: v.clone() for k, v in t.items()}
        t2[src][bi, ci, yi, xi] = bad
        out = _launch(eng, which, t2, want)
        for k in want:
            reach = torch.zeros(B, 1, H, W, dtype=torch.bool)
            reach[bi, 0, max(0, yi - kh // 2):yi + kh // 2 + 1, max(0, xi - kw // 2):xi + kw // 2 + 1] = True
            o, ref = out[k].cpu(), base[k].cpu()
            chans = slice(0, hid) if (k == "HX" and layer.startswith("q")) else slice(None)  # the q conv writes the new h only
            r = reach.expand(B, o[:, chans].shape[1], H, W)
            assert not torch.isfinite(o[:, chans][r]).any(), (k, bad)
            keep = torch.ones_like(o, dtype=torch.bool)
            keep[:, chans][r] = False
            if src == k:
                keep[bi, ci, yi, xi] = False  # the planted value itself, where the tensor is also an input
            assert torch.equal(o[keep], ref[keep]), (k, bad)


# ------------------------------------------------------------------------------------------------ the encoder's layers
ENC = [(3, 1, 64, 64), (3, 2, 64, 96), (1, 2, 64, 96), (3, 1, 96, 96), (3, 2, 96, 128), (1, 2, 96, 128), (3, 1, 128, 128), (3, 1, 256, 192)]


class _ConvNormEx:
    def __init__(self, w, bias, bn, stride, arith):
        from nndepth_amd._lib import ConvDesc, lib
        from nndepth_amd.ops import check
        co, ci, kh, kw = w.shape
        self.desc, self.arith = ConvDesc(co, ci, kh, kw, stride), arith
        n = int(lib.nnd_conv_packed_floats_ex(C.byref(self.desc), arith))
        assert n > 0
        blob = torch.zeros(n)
        check(lib.nnd_conv_pack_ex(C.byref(self.desc), arith, _p(w.contiguous()), _p(bias), *[_p(v.contiguous()) for v in bn], 1e-5, _p(blob)), "pack")
        self.packed = blob.to(DEV)
        ncb, nch = (co + 31) // 32, ci // 16
        self.tail = ncb * nch * kh * kw * 256 + ncb * 32

    def __call__(self, x, res, c4, flags=0):
        from nndepth_amd._lib import lib
        from nndepth_amd.ops import _stream, check
        Bn, _, Hin, Win = x.shape
        st = self.desc.stride
        y = torch.empty((Bn, self.desc.Cout, (Hin + st - 1) // st, (Win + st - 1) // st), dtype=torch.float32, device=DEV)
        ws = torch.empty(int(lib.nnd_conv_workspace_floats_ex(C.byref(self.desc), Bn, Hin, Win)), dtype=torch.float32, device=DEV) if c4 else None
        check(lib.nnd_conv_forward_ex(C.byref(self.desc), self.arith, flags, _p(self.packed), _p(x), _p(res), _p(y), _p(ws), None, Bn, Hin, Win,
                                      1, 1 if res is not None else 0, _stream(torch.device(DEV))), "conv_forward_ex")
        return y


@pytest.mark.parametrize("k,st,cin,cout", ENC, ids=[f"{k}x{k}s{st}-{ci}to{co}" for k, st, ci, co in ENC])
def test_encoder_layer_vs_contract(monkeypatch, capfd, k, st, cin, cout):
    """conv -> folded BatchNorm -> ReLU -> + residual -> ReLU (a residual block's second half; its first half and the shortcut without the
    residual), planar NCHW and the encoder's c4 tile-major layout."""
    from nndepth_amd._lib import NND_FLAG_CALIBRATE, NndError
    g = torch.Generator().manual_seed(k * 1000 + st * 100 + cin + cout)
    w = _log_uniform((cout, cin, k, k), -6, 0, g) / (cin * k * k) ** 0.5
    bias = _log_uniform((cout,), -6, 0, g)
    bn = [torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1, torch.randn(cout, generator=g) * 0.1, torch.rand(cout, generator=g) + 0.5]
    Hin, Win = (26, 44) if st == 2 else (13, 22)
    x = _log_uniform((B, cin, Hin, Win), -6, 1, g)
    res = torch.randn(B, cout, 13, 22, generator=g)
    conv = _ConvNormEx(w, bias, bn, st, 1)
    xd, rd = x.to(DEV), res.to(DEV)
    conv(xd, None, False, NND_FLAG_CALIBRATE)
    tail = conv.packed[conv.tail:conv.tail + 4].cpu()
    xs, ws = tail[1].item(), 1.0 / tail[3].item()
    assert tail[0].item() == tail[3].item() / xs and 2 ** 10 <= x.abs().max().item() * xs < 2 ** 11
    sc = bn[0].double() / torch.sqrt(bn[3].double() + 1e-5)
    sh = (bias.double() - bn[2].double()) * sc + bn[1].double()

    def contract(xx, ww, r):
        y = F.conv2d(xx, ww, None, stride=st, padding=k // 2) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
        y = y.clamp_min(0)
        return y if r is None else (y + r.double()).clamp_min(0)
    xr, wr = _half(x, xs), _half(w, ws)
    exact = _ConvNormEx(wr.float(), bias, bn, st, 0)
    rows, refused = [], []
    for r_, rdev in ((None, None), (res, rd)):
        y_c = contract(xr, wr, r_)
        for c4 in (False, True):
            # (the exact kernel reads 4-channel-interleaved sources at stride 1 only: at stride 2 its planar launch is the yardstick)
            e32 = errs(exact(xr.float().to(DEV), rdev, c4 and st == 1).cpu(), y_c)
            for cfg in (None, "0,1", "0,2", "0,4", "nofast"):
                monkeypatch.delenv("NND_SPLIT_CFG", raising=False)
                monkeypatch.delenv("NND_SPLIT_NO_FAST", raising=False)
                monkeypatch.setenv("NND_CONV_VERBOSE", "1")
                if cfg == "nofast":
                    monkeypatch.setenv("NND_SPLIT_NO_FAST", "1")
                elif cfg:
                    monkeypatch.setenv("NND_SPLIT_CFG", cfg)
                y, err = _run(capfd, lambda: conv(xd, rdev, c4))
                if isinstance(y, NndError):
                    assert cfg and cfg[0] == "0" and "no configuration" in str(y), (cfg, y)
                    refused.append(cfg)
                    continue
                (L,) = split_lines(err)
                assert L["pieces"] == 1 and L["stride"] == st and (cfg is None or cfg[0] != "0" or L["ks"] == int(cfg[2])), (cfg, L)
                assert torch.equal(y, conv(xd, rdev, c4)), (cfg, "run to run")
                e = errs(y.cpu(), y_c)
                rows.append((f"{'res' if r_ is not None else 'relu'} {'c4' if c4 else 'nchw'} {cfg or 'picker'}", L, e, e32))
    monkeypatch.delenv("NND_SPLIT_CFG", raising=False)
    monkeypatch.delenv("NND_SPLIT_NO_FAST", raising=False)
    txt = f"encoder layer {k}x{k} stride {st} {cin}->{cout}: refused {sorted(set(refused))}\n"
    for what, L, e, e32 in rows:
        txt += (f"    {what:<20} ny={L['ny']} wco={L['wco']} ks={L['ks']} nu={L['nu']} {'fast' if L['fast'] else 'generic'}  max-abs {e[0]:.2e} rms {e[1]:.2e}"
                f"   (exact fp32 launch {e32[0]:.2e} {e32[1]:.2e})\n")
    print("\n" + txt, end="")
    _lines[(1, ENC.index((k, st, cin, cout)))] = txt
    assert len(rows) >= 8
    for what, L, e, e32 in rows:
        assert e[0] <= 2 * e32[0] and e[1] <= 2 * e32[1], (what, L, e, e32)
    # out of range / NaN in the c4 layout
    base = conv(xd, rd, True).cpu()
    bi, ci, yi, xi = 1, 7, 6 * st, 10 * st
    reach = torch.zeros(B, 1, 13, 22, dtype=torch.bool)
    reach[bi, 0, max(0, 6 - (k // 2)):6 + k // 2 + 1, max(0, 10 - (k // 2)):10 + k // 2 + 1] = True
    if st == 2 and k == 3:  # input (2r + dy - 1, 2c + dx - 1): the even position (12, 20) is read by outputs (6, 10) only ... and its neighbours' taps
        reach[:] = False
        reach[bi, 0, 6:8, 10:12] = True
        yi, xi = 13, 21  # an odd position: read by outputs r in {6, 7}, c in {10, 11}
    elif st == 2:
        reach[:] = False
        reach[bi, 0, 6, 10] = True
    reach = reach.expand(B, cout, 13, 22)
    for bad in (64.0 * x.abs().max().item(), float("nan")):
        x2 = x.clone()
        x2[bi, ci, yi, xi] = bad
        y = conv(x2.to(DEV), rd, True).cpu()
        assert not torch.isfinite(y[reach]).any(), bad
        assert torch.equal(y[~reach], base[~reach]), bad
