"""GPU: the fp16x2 range contract (include/nndepth_amd.h "fp16x2 activation range", csrc/calib.hip, csrc/split_arith.h).
  a. nnd_*_calibration_finish: the scale a recorded maximum gives, exactly, over 40 octaves; zero and non-finite records
  b. what each layer of the update block records, against the float64 walk of tests/calib_cases.py
  c. how records accumulate: over the batch, over the iterations of a loop, over the calls of one calibration block — and that
     they are cleared by the finish
  d. calibrating on one input and evaluating on another, at model level, against the reference's golden outputs
  e. beyond 32 x the calibrated maximum the output is inf / NaN — through every epilogue, never a finite wrong value
NaN and inf are data values here; no test provokes a fault."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calib_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------- a. finish arithmetic
def _layer(cin=32, cout=48, seed=5):
    from nndepth_amd import ops
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    return ops.Conv2d(w, torch.zeros(cout), arithmetic="fp16x2")


@pytest.mark.parametrize("kind", ["gauss", "single_1.0", "single_1.37", "single_below_2"])
@pytest.mark.parametrize("shape", [(3, 5, 9), (2, 17, 9)], ids=lambda s: "x".join(map(str, s)))
def test_finish_sets_the_scale_of_the_recorded_maximum(shape, kind):
    """calibrate(x * 2^k).activation_range() == expected_range(max|x| * 2^k) for k = -20 .. 20: the scaling by 2^k is exact, so
    the equality is.  `single_*`: the maximum is ONE element, in the last sample's last channel's last pixel (a record over part
    of the batch or of the image misses it); 1.0 and the float below 2 are the two ends of one octave."""
    B, H, W = shape
    conv = _layer()
    g = torch.Generator().manual_seed(B * 100 + H)
    if kind == "gauss":
        x = torch.randn(B, 32, H, W, generator=g)
    else:
        x = 0.25 * torch.rand(B, 32, H, W, generator=g)
        x[-1, -1, -1, -1] = -{"single_1.0": 1.0, "single_1.37": 1.37, "single_below_2": float(np.nextafter(np.float32(2), np.float32(0)))}[kind]
    m = x.abs().max().item()
    assert conv.activation_range() == CC.DEFAULT_RANGE
    for k in range(-20, 21):
        got = conv.calibrate((x * 2.0 ** k).to(DEV)).activation_range()
        assert got == CC.expected_range(m * 2.0 ** k), (k, got, m)


def test_finish_keeps_the_scale_on_zeros_and_widens_it_on_inf():
    conv = _layer()
    z = torch.zeros(2, 32, 5, 9, device=DEV)
    assert conv.calibrate(z).activation_range() == CC.DEFAULT_RANGE  # nothing recorded: the default stays
    x = torch.randn(2, 32, 5, 9)
    r = conv.calibrate(x.to(DEV)).activation_range()
    assert r == CC.expected_range(x.abs().max().item()) and conv.calibrate(z).activation_range() == r  # ... and so does a calibrated one
    x[1, 7, 2, 3] = float("inf")
    assert conv.calibrate(x.to(DEV)).activation_range() == r * 4096.0
    x[1, 7, 2, 3] = float("nan")
    assert conv.calibrate(x.to(DEV)).activation_range() == r * 4096.0 ** 2
    x[1, 7, 2, 3] = 0.0  # the non-finite record did not stick either
    assert conv.calibrate(x.to(DEV)).activation_range() == CC.expected_range(x.abs().max().item())


# ------------------------------------------------------------------------------------------- b. what each layer records
def _block(name, arithmetic="fp16x2"):
    from nndepth_amd.blocks import BasicUpdateBlock
    kw, gru, sd, prefix, ins = CC.make_case(name)
    ub = BasicUpdateBlock(gru=gru, arithmetic=arithmetic, **kw)
    ub.load_state_dict({k[len(prefix) + 1:]: v for k, v in sd.items()}, strict=True)
    return ub.to(DEV), kw, gru, sd, prefix, ins


_walks = {}


def _walk(name):
    """The float64 walk of a case, computed once and shared (read-only)."""
    if name not in _walks:
        kw, gru, sd, prefix, ins = CC.make_case(name)
        _walks[name] = CC.staged_maxima(sd, prefix, *ins, gru=gru)
    return _walks[name]


@pytest.mark.parametrize("switch", [None, "NND_NO_C4", "NND_NO_FUSED_FLOW_BRANCH"])
@pytest.mark.parametrize("name", CC.NAMES)
def test_update_block_records_what_each_layer_stages(monkeypatch, name, switch):
    """One calibrating call of nnd_update_block_forward: every fp16x2 layer on its path has the scale of the float64 maximum of the
    tensor it stages — in the default layout, with planar workspaces (NND_NO_C4) and with convf1 / convf2 as two launches
    (NND_NO_FUSED_FLOW_BRANCH: other launchers, other calib_amax_* call sites).
    Off the path BY DESIGN: the loop's packings of the GRU convs, `...[h,motion]`, `...[rh,motion]` and `...[inp]`
    (update_block.hip: run_update launches C_ZR1 / C_Q1 / C_ZR2 / C_Q2, lines 552-556; enqueue_refine the C_*X and C_*C layers,
    lines 840-841 and 915-919).  They keep the default scale and are what sets status bit 1; bit 0 is clear."""
    from nndepth_amd import ops
    if switch:
        monkeypatch.setenv(switch, "1")
    ub, kw, gru, sd, prefix, ins = _block(name)
    _, M = _walk(name)
    with ops.calibration() as c:
        ub(*(x.to(DEV) for x in ins))
    got = ub.engine.activation_ranges()
    ref = {k: v for k, v in M.items() if CC.is_fp16x2(k, kw)}
    assert set(got) == set(ref), (sorted(set(got) - set(ref)), sorted(set(ref) - set(got)))
    for k in sorted(ref):
        want = CC.DEFAULT_RANGE if CC.is_loop_only(k) else CC.expected_range(ref[k])
        print(f"{name:20s} {k:32s} M_ref {ref[k]:9.5f}  range {got[k]:9.1f}  expected {want:9.1f}")
        assert got[k] == want, (name, switch, k, got[k], want, ref[k])
    assert c.status == 2


@pytest.mark.parametrize("name", ["raft_h128_c64", "convgru_h128_c128"])
def test_one_loop_iteration_records_what_the_loop_layers_stage(name):
    """The other entry point: refine(iters=1) from a given disparity runs the walk's network on corr = the lookup at that disparity, so
    the loop's own packings (`[h,motion]`, `[rh,motion]`, `[inp]`) record the walk's maxima; the single-call GRU layers are off ITS
    path (see above) and keep the default.  corr comes from the oracle's lookup; the GPU's differs by rounding only."""
    from nndepth_amd import ops
    from oracle import torch_ref as R
    ub, kw, gru, sd, prefix, (net, inp, _, flow) = _block(name)
    g = torch.Generator().manual_seed(70)  # (the margins asserted below hold for this seed)
    f1, f2 = torch.randn(CC.B, 64, CC.H, CC.W, generator=g), torch.randn(CC.B, 64, CC.H, CC.W, generator=g)
    org = torch.arange(CC.W).float()[None, None, None].repeat(CC.B, 1, CC.H, 1)
    corr = R.corr1d_lookup(R.corr1d_build(f1, f2, 4), org + flow, 4, 4)
    _, M = CC.staged_maxima(sd, prefix, net, inp, corr, flow, gru=gru)
    eng = ub.sync_engine(DEV)
    with ops.calibration() as c:
        eng.refine(ops.corr1d_build(f1.to(DEV), f2.to(DEV), 4), 4, 4, net.to(DEV), inp.to(DEV), 8, 1, disp_init=flow.to(DEV))
    got = eng.activation_ranges()
    for k in sorted(got):
        want = CC.DEFAULT_RANGE if CC.is_single_only(k) else CC.expected_range(M[k])
        print(f"{name:20s} {k:32s} M_ref {M[k]:9.5f} (margin {CC.power_of_two_margin(M[k]):.3f})  range {got[k]:9.1f}  expected {want:9.1f}")
        assert CC.is_single_only(k) or CC.power_of_two_margin(M[k]) >= 0.01, (name, k, M[k])
        assert got[k] == want, (name, k, got[k], want, M[k])
    assert c.status == 2


# ---------------------------------------------------------------------------------------------------- c. accumulation
class _Loop:
    """One refinement entry point on one sample-independent input generator: make(seed, B, scale) -> inputs, run(eng, inputs, iters,
    init, net) -> (up, low, net_out), cat(a, b) -> the batch of both."""
    H, W = 13, 22

    def __init__(self, kind):
        self.kind = kind
        self.case = {"refine": "raft_h128_c64", "refine_group": "convgru_h128_c128", "refine_igev": "igev_h64_c64_cp576",
                     "refine_igev_il": "igev_h64_c64_cp576", "refine_cre": "cre_h128_c128_f2"}[kind]
        self.kw, self.gru, self.sd, self.prefix, _ = CC.make_case(self.case)
        self.rate = self.kw["spatial_scale"]
        self.fc = self.kw["flow_channel"]

    def engine(self):
        from nndepth_amd import ops
        kw = self.kw
        eng = ops.UpdateBlockEngine(kw["hidden_dim"], kw["context_dim"], kw["cor_planes"], self.fc, 9 * self.rate ** 2, self.gru, "fp16x2")
        return eng.load(self.sd, self.prefix + ".", device=DEV)

    def make(self, seed, B=1, scale=1.0):
        g = torch.Generator().manual_seed(seed)
        C = 128 if self.kind.startswith("refine_igev") else 64
        d = {"f1": torch.randn(B, C, self.H, self.W, generator=g), "f2": torch.randn(B, C, self.H, self.W, generator=g),
             "g1": torch.randn(B, C, self.H, self.W, generator=g) * 1.5, "g2": torch.randn(B, C, self.H, self.W, generator=g) * 1.5,
             "net": torch.tanh(torch.randn(B, self.kw["hidden_dim"], self.H, self.W, generator=g)),
             "inp": torch.relu(torch.randn(B, self.kw["context_dim"], self.H, self.W, generator=g)),
             "init": -3.0 * torch.rand(B, self.fc, self.H, self.W, generator=g)}
        return {k: (v * (scale if k != "init" else 1.0)).to(DEV) for k, v in d.items()}

    @staticmethod
    def cat(a, b):
        return {k: torch.cat([a[k], b[k]], 0) for k in a}

    def run(self, eng, d, iters, init=None, net=None):
        from nndepth_amd import ops
        init = d["init"] if init is None else init
        net = d["net"] if net is None else net
        B = net.shape[0]
        if self.kind == "refine":
            return eng.refine(ops.corr1d_build(d["f1"], d["f2"], 4), 4, 4, net, d["inp"], self.rate, iters, disp_init=init)
        if self.kind == "refine_group":
            return eng.refine_group(ops.raft_group_corr_build(d["f1"], d["f2"], 4, 1), 4, 1, 4, net, d["inp"], self.rate, iters, disp_init=init)
        if self.kind == "refine_cre":
            return eng.refine_cre(d["f1"], d["f2"], net, d["inp"], self.rate, iters, flow_init=init)
        fp, gp = ops.group_corr_build(d["f1"], d["f2"], 8, 16, 4), ops.group_corr_build(d["g1"], d["g2"], 8, 16, 4)
        il = ops.igev_interleave_pyramids(fp, gp, B, 8, self.H, self.W, 4) if self.kind == "refine_igev_il" else None
        self.last_pyramids = (fp, gp)
        return eng.refine_igev(fp, gp, 8, 4, 4, net, d["inp"], self.rate, iters, disp_init=init, interleaved=il)


LOOPS = ["refine", "refine_group", "refine_igev", "refine_igev_il", "refine_cre"]


def _on_loop_path(eng):
    return {k: v for k, v in eng.activation_ranges().items() if not CC.is_single_only(k)}


@pytest.mark.parametrize("kind", LOOPS)
def test_loop_records_accumulate_over_batch_calls_and_iterations(kind):
    from nndepth_amd import ops
    L = _Loop(kind)
    A, Bq = L.make(1), L.make(2, scale=8.0)  # B's activations are larger: a record of the first sample / call only would be A's
    # -- over the batch == over the calls of one block
    e_cat, e_seq, e_A = L.engine(), L.engine(), L.engine()
    with ops.calibration() as c1:
        L.run(e_cat, L.cat(A, Bq), 2)
    with ops.calibration() as c2:
        L.run(e_seq, A, 2)
        L.run(e_seq, Bq, 2)
    with ops.calibration() as c3:
        L.run(e_A, A, 2)
    assert torch.equal(e_cat.packed, e_seq.packed), "batch cat(A, B) and the calls A, B of one block must leave the same scales"
    assert not torch.equal(e_cat.packed, e_A.packed), "the case does not tell: B adds nothing to A's records"
    # -- every layer on the loop's path has recorded (status bit 1 is set all the same: the single-call GRU convs C_ZR1 / C_Q1 /
    #    C_ZR2 / C_Q2 of update_block.hip:552-556 are not launched by enqueue_refine, :915-919, by design), none saw inf / NaN
    for c in (c1, c2, c3):
        assert c.status & 1 == 0
    rg = e_A.activation_ranges()  # (inputs at O(1): no maximum anywhere near the default's octave [256, 512))
    print(kind, {k: v for k, v in rg.items()})
    for k, v in rg.items():
        assert (v == CC.DEFAULT_RANGE) == CC.is_single_only(k), (kind, k, v)
    # -- over the iterations: 3 iterations in one call == 3 chained one-iteration calls in one block
    e3, e111 = L.engine(), L.engine()
    with ops.calibration():
        up3, low3, net3 = L.run(e3, A, 3)
    if kind == "refine_cre":
        # a stage alternates its search window with the iteration's parity (update_block.hip:831-833, `it & 1`): three first iterations
        # are another computation than iterations 0, 1, 2, so neither outputs nor records are comparable for this entry point
        return
    org = torch.arange(L.W, device=DEV).float()[None, None, None].repeat(1, 1, L.H, 1)
    with ops.calibration():
        init, net, ups = None, None, []
        for _ in range(3):
            up, low, net = L.run(e111, A, 1, init, net)
            # the loop hands its state over as the low-resolution map: IGEV's is the coordinate itself (update_block.hip:333,
            # `absolute`), and a call starts from x + disp_init (init_coords_kernel)
            init = low - org if kind.startswith("refine_igev") else low
            ups.append(up[0])
    # NOT bit for bit: the state crosses the call as c - x and comes back as x + (c - x), one rounding of the coordinate
    # (measured: up to 6e-6 on the upsampled map after 3 iterations); the records — powers of two — do not see it
    d_up = max((a - b).abs().max().item() for a, b in zip(ups, up3))
    d_low, d_net = (low - low3).abs().max().item(), (net - net3).abs().max().item()
    print(f"{kind}: chained one-iteration calls vs 3 iterations: up {d_up:.3e}  low {d_low:.3e}  net {d_net:.3e}")
    assert d_up <= 1e-4 and d_low <= 1e-4 and d_net <= 1e-4
    assert torch.equal(e3.packed, e111.packed)
    # ... and a record of the first iteration alone would be another one: from a zero disparity the flow branch stages relu(convf1(0)),
    # its bias, in iteration 1 and the real flow from iteration 2 on (RAFT's relative flow; IGEV's is the coordinate itself)
    z = torch.zeros_like(A["init"])
    e3z, e1z = L.engine(), L.engine()
    with ops.calibration():
        L.run(e3z, A, 3, init=z)
    with ops.calibration():
        L.run(e1z, A, 1, init=z)
    r3, r1 = e3z.activation_ranges()["encoder.convf2"], e1z.activation_ranges()["encoder.convf2"]
    print(f"{kind}: encoder.convf2 range after 3 iterations {r3}, after the first alone {r1}")
    if not kind.startswith("refine_igev"):
        assert r3 > r1, "the case does not tell: iterations 2 and 3 add nothing to the first one's record"


@pytest.mark.parametrize("kind", LOOPS)
def test_loop_records_do_not_stick(kind):
    """A, then in a NEW block a much smaller B: the scales of a fresh engine calibrated on B alone."""
    from nndepth_amd import ops
    L = _Loop(kind)
    A, Bq = L.make(3, scale=16.0), L.make(4, scale=1.0 / 16)
    e, fresh = L.engine(), L.engine()
    with ops.calibration():
        L.run(e, A, 2)
    after_a = e.packed.clone()
    with ops.calibration():
        L.run(e, Bq, 2)
    with ops.calibration():
        L.run(fresh, Bq, 2)
    # (the single-call layers are at the default in both)
    assert torch.equal(e.packed, fresh.packed) and not torch.equal(e.packed, after_a)


def test_igev_interleaved_lookup_records_the_bound_of_both_pyramids():
    """refine_igev over the interleaved copy: convc1's operands are interpolated inside the kernel, so its record is the bound taken in
    update_block.hip:880-883 — the largest entry of either pyramid, which are inputs of the call: exact."""
    from nndepth_amd import ops
    L = _Loop("refine_igev_il")
    d = L.make(5, B=2)
    eng = L.engine()
    with ops.calibration():
        L.run(eng, d, 2)
    fp, gp = L.last_pyramids
    m = max(fp.abs().max().item(), gp.abs().max().item())
    assert eng.activation_ranges()["encoder.convc1"] == CC.expected_range(m), (m, eng.activation_ranges()["encoder.convc1"])


def _encoder(norm, raft_sd):
    from nndepth_amd import ops
    enc_sd = {k[len("fnet."):]: v for k, v in raft_sd.items() if k.startswith("fnet.")}
    cnet_sd = {k[len("cnet_proj."):]: v for k, v in raft_sd.items() if k.startswith("cnet_proj.")}
    return ops.EncoderEngine(256, norm, 192, "fp16x2").load(enc_sd, cnet_sd, device=DEV)


@pytest.mark.parametrize("norm", ["batch", "instance"])
def test_encoder_records_accumulate_and_do_not_stick(raft_sd, norm):
    from nndepth_amd import ops, weightgen
    a = weightgen.synthetic_frames(1, 1, 72, 104)[0].to(DEV)
    b = (weightgen.synthetic_frames(2, 1, 72, 104)[0] * (8.0 if norm == "batch" else 1.0)).to(DEV)
    e_cat, e_seq, e_a, e_b = (_encoder(norm, raft_sd) for _ in range(4))
    with ops.calibration() as c:
        e_cat.forward(torch.cat([a, b]), n_cnet=2)
    with ops.calibration():
        e_seq.forward(a, n_cnet=1)
        e_seq.forward(b, n_cnet=1)
    assert c.status == 0  # every fp16x2 layer of the encoder is on the path of a forward with its cnet conv
    assert torch.equal(e_cat.packed, e_seq.packed)
    with ops.calibration():
        e_a.forward(a, n_cnet=1)
    with ops.calibration():
        e_b.forward(b, n_cnet=1)
    if norm == "batch":  # (an instance-norm encoder normalises every sample: b's records equal a's up to the image content)
        assert not torch.equal(e_cat.packed, e_a.packed)
    with ops.calibration():
        e_a.forward(b, n_cnet=1)  # a, then in a new block b: b's scales alone
    assert torch.equal(e_a.packed, e_b.packed)


@pytest.mark.parametrize("Cout,Cin,split,stride", [(8, 16, 0, 1), (16, 32, 16, 1), (16, 8, 0, 2), (32, 16, 0, 2)])
def test_conv3d_records_accumulate_and_do_not_stick(Cout, Cin, split, stride):
    from nndepth_amd import ops
    g = torch.Generator().manual_seed(Cout + Cin)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) * (2.0 / (Cin * 27)) ** 0.5
    bn = (torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1, torch.randn(Cout, generator=g) * 0.1, torch.rand(Cout, generator=g) + 0.5)
    a, b = torch.randn(1, Cin, 6, 9, 14, generator=g), 8.0 * torch.randn(1, Cin, 6, 9, 14, generator=g)
    if split:  # the second operand of the concat carries the maximum
        b[:, :split] /= 64.0

    base = ops.Conv3dNorm(w, None, stride, bn, 1e-5, 0.01, split, DEV, arithmetic="fp16x2")

    def layer():  # copies of ONE packed blob: the parts of it that no formulation of this shape uses are never written
        import copy
        e = copy.copy(base)
        e.packed = base.packed.clone()
        return e

    def same(a, b):
        return torch.equal(a.packed.view(torch.int32), b.packed.view(torch.int32))

    def run(conv, x):
        x = x.to(DEV)
        if split:
            return conv(ops.volume_to_depth_major(x[:, :split]), ops.volume_to_depth_major(x[:, split:]))
        return conv(ops.volume_to_depth_major(x))

    e_cat, e_seq, e_a, e_b = layer(), layer(), layer(), layer()
    with ops.calibration() as c:
        run(e_cat, torch.cat([a, b]))
    with ops.calibration():
        run(e_seq, a)
        run(e_seq, b)
    # a stride-1 layer packs three formulations of itself, each with its own slot (conv3d.hip:72-75, 335-338: tail1, tailJ, the
    # depth-marching kernel's); the one that runs records, so bit 1 is set there by design.  A stride-2 layer has one.
    assert c.status & 1 == 0 and bool(c.status & 2) == (stride == 1)
    assert same(e_cat, e_seq)
    with ops.calibration():
        run(e_a, a)
    assert not same(e_a, e_cat)
    with ops.calibration():
        run(e_a, b / 1024.0)
    with ops.calibration():
        run(e_b, b / 1024.0)
    assert same(e_a, e_b)


# ----------------------------------------------------------------------------------- d. held-out inputs, model level
def _raft(arithmetic="fp16x2"):
    from nndepth_amd import weightgen
    from nndepth_amd.raft_stereo import BaseRAFTStereo
    from oracle import torch_ref as R
    m = BaseRAFTStereo(iters=6, context_dim=64, arithmetic=arithmetic)
    m.load_state_dict(weightgen.fill_state_dict(R.raft_stereo_spec()), strict=True)
    return m.to(DEV).eval()


def _model_raft(gold):
    from nndepth_amd import weightgen
    g = gold("forward_small.npz")
    return _raft(), weightgen.synthetic_frames(0, 1, 96, 160), [g["up_disp"][i] for i in range(6)], 1e-4, (128, 160)


def _model_cre(gold):
    from nndepth_amd import weightgen
    from nndepth_amd.cre_stereo import CREStereoBase
    from oracle import cre_ref
    g = gold("cre_forward.npz")
    m = CREStereoBase(iters=4, arithmetic="fp16x2")
    m.load_state_dict(weightgen.fill_state_dict(cre_ref.cre_stereo_spec()), strict=True)
    return m.to(DEV).eval(), weightgen.synthetic_frames(3, 1, 128, 192), [g[f"up_disp_{i}"] for i in range(8)], 1e-4, (160, 224)


def _model_igev(gold):
    from igev_double import make_igev
    from nndepth_amd import weightgen
    from nndepth_amd.igev_stereo import IGEVStereoBase, CostVolumeFilterNetwork
    g = gold("igev_forward.npz")
    m = make_igev(IGEVStereoBase, CostVolumeFilterNetwork, iters=4, hidden_dim=64, context_dim=64, arithmetic="fp16x2")
    weightgen.fill_module_(m, "igev.")
    return m.to(DEV).eval(), weightgen.synthetic_frames(6, 1, 128, 192), [g["up_disp"][i] for i in range(4)], 1e-4, (160, 224)


def _model_c2f(gold):
    from c2f_double import make_c2f
    from nndepth_amd import weightgen
    from nndepth_amd.raft_stereo import Coarse2FineRAFTStereoBase
    g = gold("c2f.npz")
    name = "c2f_b1_64x128_it3"
    B, Hf, Wf, iters, seed = (int(v) for v in g[name + "_cfg"])
    m = make_c2f(Coarse2FineRAFTStereoBase, iters=iters, corr_levels=1, arithmetic="fp16x2")
    weightgen.fill_module_(m, "c2f.")
    ref = g[name + "_ups"]
    return m.to(DEV).eval(), weightgen.synthetic_frames(seed, B, Hf, Wf), [ref[i] for i in range(3 * iters)], 1.5e-5, (128, 192)


MODELS = {"raft": _model_raft, "cre": _model_cre, "igev": _model_igev, "c2f": _model_c2f}


class _EngineWatch:
    """Every engine that takes part in a calibration, and how often one was asked (ops._Calibration.flags is the one door)."""

    def __init__(self, monkeypatch):
        from nndepth_amd import ops
        self.engines, self.calls = [], 0
        orig = ops._Calibration.flags

        def flags(cal, engine):
            self.calls += 1
            if all(e is not engine for e in self.engines):
                self.engines.append(engine)
            return orig(cal, engine)

        monkeypatch.setattr(ops._Calibration, "flags", flags)


@pytest.mark.parametrize("variant", ["other_seed", "other_seed_other_shape", "batch_of_two_other_seeds", "half_contrast"])
@pytest.mark.parametrize("model", list(MODELS))
def test_model_calibrated_on_one_input_meets_the_golden_on_another(gold, monkeypatch, model, variant):
    """The existing golden tests' bar, with the activation scales taken from ANOTHER input: a record over the wrong tensor, part of
    the batch or the first iteration only suits the input it was taken on and shows here.  Half contrast: the largest activation
    of the golden pair is at most about 4 x the calibrated one (the correlation is the only product of two activations), an
    eighth of the factor-32 headroom."""
    from nndepth_amd import weightgen
    m, (f1, f2), refs, bar, other_hw = MODELS[model](gold)
    H, W = f1.shape[-2:]
    if variant == "other_seed":
        c1, c2 = weightgen.synthetic_frames(41, 1, H, W)
    elif variant == "other_seed_other_shape":
        c1, c2 = weightgen.synthetic_frames(42, 1, *other_hw)
    elif variant == "batch_of_two_other_seeds":
        (a1, a2), (b1, b2) = weightgen.synthetic_frames(43, 1, H, W), weightgen.synthetic_frames(44, 1, H, W)
        c1, c2 = torch.cat([a1, b1]), torch.cat([a2, b2])
    else:
        c1, c2 = 0.5 * f1, 0.5 * f2
    watch = _EngineWatch(monkeypatch)
    m.calibrate(c1.to(DEV), c2.to(DEV))
    assert watch.engines and all(e.calibrated for e in watch.engines)
    blobs = [e.packed.clone() for e in watch.engines]
    calls = watch.calls
    outs = m(f1.to(DEV), f2.to(DEV))
    errs = [np.abs(o["up_disp"].cpu().numpy() - r).max() for o, r in zip(outs, refs)]
    print(f"{model} calibrated on {variant}: max-abs vs golden per output:", " ".join(f"{e:.2e}" for e in errs))
    assert len(outs) == len(refs) and max(errs) <= bar, (model, variant, errs)
    # no silent recalibration: nobody asked for calibration flags, and every packed blob is bit for bit what the calibration left
    # (compared as bit patterns: a blob may hold padding that was never written)
    assert watch.calls == calls and all(torch.equal(e.packed.view(torch.int32), b.view(torch.int32)) for e, b in zip(watch.engines, blobs))


def test_raft_calibrated_then_a_sixteenth_of_the_contrast():
    """The lower side of the window: scales from the seed-0 pair, evaluation on another pair at 1/16 contrast (activations 4 to 8
    octaves below the calibrated maxima, inside the 13 octaves that keep all 22 bits)."""
    from nndepth_amd import weightgen
    from oracle import torch_ref as R
    sd = weightgen.fill_state_dict(R.raft_stereo_spec())
    f1, f2 = (x / 16.0 for x in weightgen.synthetic_frames(45, 1, 96, 160))
    ref = R.raft_stereo_forward(sd, f1, f2, 6)
    e32 = [(o["up_disp"].cpu() - r).abs().max().item() for o, r in zip(_raft("fp32")(f1.to(DEV), f2.to(DEV)), ref)]
    print("fp32 arithmetic vs oracle at 1/16 contrast:", " ".join(f"{e:.2e}" for e in e32))
    assert max(e32) <= 1e-4, "the pair itself is outside the bar: change the pair"
    m = _raft()
    c1, c2 = weightgen.synthetic_frames(0, 1, 96, 160)
    m.calibrate(c1.to(DEV), c2.to(DEV))
    errs = [(o["up_disp"].cpu() - r).abs().max().item() for o, r in zip(m(f1.to(DEV), f2.to(DEV)), ref)]
    print("fp16x2 calibrated on the seed-0 pair, same input:", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= 1e-4


def test_calibrate_refuses_a_frame_with_nan():
    from nndepth_amd import weightgen
    from nndepth_amd._lib import NndError
    f1, f2 = weightgen.synthetic_frames(0, 1, 96, 160)
    f1[0, 1, 40, 70] = float("nan")
    with pytest.raises(NndError):
        _raft().calibrate(f1.to(DEV), f2.to(DEV))


# -------------------------------------------------------------------------------------------- e. overflow is visible
def _touched(shape, y, x, r):
    m = torch.zeros(shape, dtype=torch.bool)
    m[..., max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = True
    return m


@pytest.mark.parametrize("calibrated", [False, True], ids=["default_scale", "calibrated_x64"])
def test_layer_overflow_is_visible_through_relu_and_sigmoid(calibrated):
    """One activation beyond the layer's range (20000 at the default scale; 64 x the calibrated maximum): every output that reads
    it is non-finite through the ReLU epilogue, and through the sigmoid epilogue of a following exact conv (ops.conv2d_offset
    takes fp32 packings only, so it is applied to the fp16x2 layer's result); every other output is right."""
    from nndepth_amd import ops
    torch.manual_seed(3)
    w = torch.randn(64, 128, 3, 3) / (128 * 9) ** 0.5
    x = torch.randn(1, 128, 12, 20)
    x[0, 5, 6, 7] = 20000.0
    conv = ops.Conv2d(w, torch.zeros(64), arithmetic="fp16x2")
    if calibrated:
        conv.calibrate(x.to(DEV))
        assert torch.isfinite(conv((x * 16).to(DEV), relu=True)).all()
        x = x * 64
    ref = torch.relu(torch.nn.functional.conv2d(x.double(), w.double(), None, padding=1))
    y = conv(x.to(DEV), relu=True).cpu()
    near = _touched(ref.shape, 6, 7, 1)
    assert not torch.isfinite(y[near]).any(), "ReLU must not turn the NaN of an overflow into 0"
    assert (y[~near].double() - ref[~near]).abs().max() <= 2e-5 * max(1.0, ref[~near].abs().max().item())
    w2 = torch.randn(18, 64, 3, 3) / (64 * 9) ** 0.5
    b2 = torch.randn(18) * 0.1
    z = ops.conv2d_offset(ops.Conv2d(w2, b2), y.to(DEV), 4.0).cpu()
    near2 = _touched(z.shape, 6, 7, 2)
    clean = torch.nan_to_num(y, nan=0.0, posinf=0.0, neginf=0.0).double()
    ref2 = 4.0 * (torch.sigmoid(torch.nn.functional.conv2d(clean, w2.double(), b2.double(), padding=1)) - 0.5) * 2.0
    assert not torch.isfinite(z[near2]).any(), "the sigmoid epilogue must not saturate a NaN"
    assert (z[~near2].double() - ref2[~near2]).abs().max() <= 2e-5 * max(1.0, clean.abs().max().item())


@pytest.mark.parametrize("name,where", [("raft_h128_c64", "inp"), ("raft_h128_c64", "net"), ("convgru_h128_c128", "inp"),
                                        ("convgru_h128_c128", "net"), ("cre_h128_c128_f2", "inp"), ("igev_h64_c64_cp576", "inp"),
                                        ("igev_h64_c64_cp576", "net"), ("igev_h64_c64_cp576", "corr")])
def test_update_block_overflow_is_visible(name, where):
    """nnd_update_block_forward, calibrated on the case's inputs, then one 20000 in `where` (far beyond 32 x any calibrated maximum):
    net_out, mask and delta are non-finite at that pixel of that sample through the ReLU, sigmoid and tanh epilogues of the block;
    more than 8 pixels away (the block's reach: 8 from corr, 6 from net / inp) and in the other sample they are finite and meet the
    bar of test_update_block_over_input_scales against the float64 walk."""
    from nndepth_amd import ops
    ub, kw, gru, sd, prefix, ins = _block(name)
    ub32 = _block(name, "fp32")[0]
    with ops.calibration() as c:
        ub(*(x.to(DEV) for x in ins))
    assert c.status & 1 == 0
    b, ch, y, x = 1, 3, 2, 3
    ins = [v.clone() for v in ins]
    ins[("net", "inp", "corr").index(where)][b, ch, y, x] = 20000.0
    truth, _ = CC.staged_maxima(sd, prefix, *ins, gru=gru)
    got = [o.cpu().double() for o in ub(*(v.to(DEV) for v in ins))]
    exact = [o.cpu().double() for o in ub32(*(v.to(DEV) for v in ins))]
    yy, xx = torch.meshgrid(torch.arange(CC.H), torch.arange(CC.W), indexing="ij")
    far = ((yy - y).abs().maximum((xx - x).abs()) > 8)[None, None].expand(CC.B, 1, CC.H, CC.W).clone()
    far[1 - b] = True
    assert far[b].any() and not far[b].all()
    for o, o32, tr, key in zip(got, exact, truth, ("net_out", "mask", "delta")):
        assert not torch.isfinite(o[b, :, y, x]).any(), (name, where, key, "finite at the overflowing pixel")
        sel = far.expand_as(o)
        assert torch.isfinite(o[sel]).all(), (name, where, key, "non-finite far from the pixel")
        sc = tr[sel].abs().max().item()
        e32, esp = (o32[sel] - tr[sel]).abs().max().item(), (o[sel] - tr[sel]).abs().max().item()
        print(f"{name} 20000 in {where}: {key} away from it: |y| max {sc:.3g}  exact fp32 {e32 / sc:.2e}  fp16x2 {esp / sc:.2e}")
        assert esp <= 1.5 * e32 + 1e-6 * sc, (name, where, key, esp, e32, sc)


def test_encoder_overflow_is_visible(raft_sd):
    """Calibrated on a frame, run on it x 2^12.  Batch norm (folded into the convs): the activations grow with the frame, 128 x past the
    headroom — the feature map is not all finite.  Instance norm: the stem is exact fp32 and every conv's input is normalised per sample
    (encoder.hip:626-651), so the fp16x2 layers stage what they staged before; the map must then be finite AND right (against the
    exact arithmetic on the same frame): the one thing it may not be is finite and wrong."""
    from nndepth_amd import ops, weightgen
    f = weightgen.synthetic_frames(0, 1, 72, 104)[0].to(DEV)
    for norm in ("batch", "instance"):
        eng = _encoder(norm, raft_sd)
        with ops.calibration() as c:
            eng.forward(f, n_cnet=1)
        assert c.status == 0
        fmap, cnet = eng.forward(f * 4096.0, n_cnet=1)
        if norm == "batch":
            assert not torch.isfinite(fmap).all() and not torch.isfinite(cnet).all()
        else:
            enc_sd = {k[len("fnet."):]: v for k, v in raft_sd.items() if k.startswith("fnet.")}
            cnet_sd = {k[len("cnet_proj."):]: v for k, v in raft_sd.items() if k.startswith("cnet_proj.")}
            ref, _ = ops.EncoderEngine(256, norm, 192, "fp32").load(enc_sd, cnet_sd, device=DEV).forward(f * 4096.0, n_cnet=1)
            err = (fmap - ref).abs().max().item()
            print(f"instance-norm encoder on the frame x 2^12: fp16x2 vs exact {err:.2e} (|fmap| max {ref.abs().max().item():.2f})")
            assert torch.isfinite(fmap).all() and err <= 5e-5 * max(1.0, ref.abs().max().item())


def test_model_overflow_is_visible():
    """RAFT-Stereo small, calibrated on its pair, then the frames x 2^12: the NaN of the encoder's overflow survives the context split, the
    correlation, the loop and the convex upsample."""
    from nndepth_amd import weightgen
    m = _raft()
    f1, f2 = (x.to(DEV) for x in weightgen.synthetic_frames(0, 1, 96, 160))
    m.calibrate(f1, f2)
    assert torch.isfinite(m(f1, f2)[-1]["up_disp"]).all()
    assert not torch.isfinite(m(f1 * 4096.0, f2 * 4096.0)[-1]["up_disp"]).all()
