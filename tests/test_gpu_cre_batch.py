"""GPU: CREStereo with more than one pair per call.  Every other CREStereo test runs B = 1, so a wrong batch stride in the
per-sample machinery (instance-norm statistics, the LoFTR sums, the AGCL kernels and their channels-last scratch, the zero
initial flow, the per-iteration output buffers, the flow hand-over between the cascade stages) would give a finite, plausible
flow for sample 1 beside a correct sample 0 and no test would fail.  Here: the stages with N = 2 against an independent reference,
the whole cascade at B = 2 / B = 3 against the batched oracle (tests/cre_batch_cases.py; tests/test_cre_batch_cpu.py pins that
reference and shows that the samples are more than 0.5 px apart), and the entry points (flow_init, two-stage, last-only, graph
replay, one model over changing batch sizes) at B > 1."""
import pytest
import torch

import cre_batch_cases as cb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ARITHMETICS = ["fp32", "bf16x3", "fp16x2"]


@pytest.fixture(scope="module")
def CR():
    from oracle import cre_ref
    return cre_ref


def _model(cre_sd, iters, **kw):
    from nndepth_amd.cre_stereo import CREStereoBase
    m = CREStereoBase(iters=iters, **kw)
    m.load_state_dict(cre_sd, strict=True)
    return m.to(DEV).eval()


def _maps(outs):
    """Every returned map, cloned (a later call must not be able to change what is compared)."""
    return [o["up_disp"].clone() for o in outs]


def _fmt(errs):
    return " ".join(f"{e:.1e}" for e in errs)


def _errors_by_sample(got, exp):
    """[output][sample] max-abs of device maps against CPU references."""
    return [cb.per_sample_errors(g.cpu(), e) for g, e in zip(got, exp)]


def _report(title, errs):
    B = len(errs[0])
    print(f"\n{title}: max-abs per output" + "".join(f"\n  sample {i}: {_fmt([e[i] for e in errs])}" for i in range(B)))


def _worst(errs):
    """(error, output index, sample index) of the largest entry: a failure names the sample."""
    return max((e, o, i) for o, per in enumerate(errs) for i, e in enumerate(per))


# ------------------------------------------------------------ stages, N = 2, another sample at each index
@pytest.mark.parametrize("H,W", [(13, 21), (8, 12)])  # W % 4 != 0: the scalar window kernel | W % 4 == 0: 4 pixels per lane
def test_agcl_two_samples_vs_oracle(CR, H, W):
    """The AGCL class in both modes and with both window shapes, N = 2 and C = 256 (channels-last offset kernel), against the
    oracle on the same seeded inputs; bounds of test_cre_agcl_class_fullsize_vs_oracle (2e-6 iter mode, 2e-5 offset mode behind
    the attention callable).  Then the channels-last offset kernel against the planar one (<= 1e-6, as in
    test_cre_agcl_offset_channels_last)."""
    from nndepth_amd import ops
    from nndepth_amd.cost_volume import AGCL
    torch.manual_seed(100 * H + W)
    N, C = 2, 256
    f1, f2 = torch.randn(N, C, H, W), torch.randn(N, C, H, W)
    flow = torch.randn(N, 2, H, W) * 3
    off = torch.rand(N, 18, H, W) * 2 - 1
    lin = torch.nn.Linear(C, C, bias=False)

    def att(a, b):
        with torch.no_grad():
            return a + 0.1 * lin.to(a.device)(b), b + 0.1 * lin.to(a.device)(a)

    d1, d2, dflow, doff = (x.to(DEV) for x in (f1, f2, flow, off))
    for sp in (False, True):
        exp = CR.agcl_corr_iter(f1, f2, flow, sp)
        got = AGCL(d1, d2)(dflow, None, small_patch=sp, iter_mode=True)
        e_it = cb.per_sample_errors(got.cpu(), exp)
        exp = CR.agcl_corr_att_offset(f1, f2, flow, off, sp, att=att)
        got = AGCL(d1, d2, att=att)(dflow, doff, small_patch=sp)
        e_of = cb.per_sample_errors(got.cpu(), exp)
        print(f"\nagcl N=2 {H}x{W} small_patch={sp}: per sample, iter {_fmt(e_it)} | att + offset {_fmt(e_of)}")
        assert tuple(got.shape) == (N, 36, H, W)
        assert max(e_it) <= 2e-6, (sp, e_it)
        assert max(e_of) <= 2e-5, (sp, e_of)
    wide = doff * 2  # offsets in [-2, 2]
    a, b = ops.nchw_to_nhwc(d1), ops.nchw_to_nhwc(d2)
    assert torch.equal(a, d1.permute(0, 2, 3, 1).contiguous())
    for sp in (False, True):
        got = ops.agcl_corr_offset(a, b, dflow, wide, sp, channels_last=True)
        ref = ops.agcl_corr_offset(d1, d2, dflow, wide, sp)
        e_cl = cb.per_sample_errors(got, ref)
        print(f"agcl N=2 {H}x{W} small_patch={sp}: channels-last vs planar per sample {_fmt(e_cl)}")
        assert max(e_cl) <= 1e-6, (sp, e_cl)


def test_instance_norm_encoder_two_pointers_two_pairs(cre_sd, CR):
    """The instance-norm encoder at B = 2, 104x168 (13x21 at 1/8): the two-pointer entry that CREStereoBase.forward_fnet uses gives
    the concatenated batch's result bit for bit (tested with BatchNorm only so far), and all four frames are within 5e-5 of the
    oracle (the bound of test_instance_norm_encoder_vs_oracle): statistics per sample, left frames first."""
    from nndepth_amd import ops
    f1, f2 = cb.frames("b2_104x168_it4")
    enc_sd = {k[len("fnet."):]: v for k, v in cre_sd.items() if k.startswith("fnet.")}
    eng = ops.EncoderEngine(256, "instance", 0).load(enc_sd, None, device=DEV)
    two, _ = eng.forward(f1.to(DEV), frames_b=f2.to(DEV))
    cat, _ = eng.forward(torch.cat([f1, f2]).to(DEV))
    exp = CR.basic_encoder_in(cre_sd, "fnet", torch.cat([f1, f2]))
    assert tuple(two.shape) == tuple(exp.shape) == (4, 256, 13, 21)
    errs = cb.per_sample_errors(two.cpu(), exp)
    print(f"\ninstance-norm encoder 2 x 104x168: max-abs per frame (left 0, left 1, right 0, right 1) {_fmt(errs)} "
          f"(|fmap| max {exp.abs().max():.2f})")
    assert torch.equal(two, cat)
    assert max(errs) <= 5e-5, errs


def test_conv2d_offset_two_samples_vs_torch():
    """range * (sigmoid(conv3x3(x)) - 0.5) * 2 in the conv epilogue with N = 2 at the 1/16 map of the 104x168 case (6x10);
    test_cascade_glue_ops_vs_torch has N = 1, its bound 2e-6."""
    from nndepth_amd import ops
    torch.manual_seed(32)
    conv = torch.nn.Conv2d(256, 18, 3, padding=1)
    x = torch.randn(2, 256, 6, 10)
    with torch.no_grad():
        exp = 1.0 * (torch.sigmoid(conv(x)) - 0.5) * 2.0
    got = ops.conv2d_offset(ops.Conv2d(conv.weight, conv.bias), x.to(DEV), 1.0).cpu()
    errs = cb.per_sample_errors(got, exp)
    print(f"\nconv2d_offset N=2 6x10: max-abs per sample {_fmt(errs)}")
    assert max(errs) <= 2e-6, errs


# ------------------------------------------------------------ the whole cascade
@pytest.mark.parametrize("arithmetic", ARITHMETICS)
@pytest.mark.parametrize("name", list(cb.CASES))
def test_cascade_batched_vs_oracle(cre_sd, name, arithmetic):
    """Every output of every sample against the batched oracle, <= 1e-4 (the project's bar and the bound of the B = 1 cascade
    tests), in the three arithmetics; a fresh model per case, so that fp16x2 calibrates on the batch it is given."""
    B, H, W, iters = cb.CASES[name]
    f1, f2 = (x.to(DEV) for x in cb.frames(name))
    exp = cb.oracle(cre_sd, name)
    outs = _maps(_model(cre_sd, iters, arithmetic=arithmetic)(f1, f2))
    assert [tuple(o.shape) for o in outs] == cb.output_shapes(name)
    errs = _errors_by_sample(outs, exp)
    _report(f"cre {name} {arithmetic} vs batched oracle (|flow| max {exp[-1].abs().max():.1f})", errs)
    err, o, i = _worst(errs)
    assert err <= 1e-4, f"output {o}, sample {i}: {err:.3e}"


@pytest.mark.parametrize("arithmetic", ARITHMETICS)
def test_sample_order_does_not_matter(cre_sd, arithmetic):
    """m([a, b]) and m([b, a]) are the same tensors with the samples swapped, and m([a, a]) holds the same sample twice, bit for
    bit.  From the code: every workgroup works on one sample (blockIdx.z, or a tile index inside one sample), every summation order
    is fixed, and the fp16x2 calibration (done by the first call, on [a, b]) is a maximum over the batch."""
    B, H, W, iters = cb.CASES["b2_104x168_it4"]
    f1, f2 = (x.to(DEV) for x in cb.frames("b2_104x168_it4"))
    m = _model(cre_sd, iters, arithmetic=arithmetic)
    ab = _maps(m(f1, f2))
    ba = _maps(m(f1.flip(0).contiguous(), f2.flip(0).contiguous()))
    aa = _maps(m(f1[:1].repeat(2, 1, 1, 1), f2[:1].repeat(2, 1, 1, 1)))
    assert len(ab) == len(ba) == len(aa) == 2 * iters
    for o, (x, y, z) in enumerate(zip(ab, ba, aa)):
        assert not torch.equal(x[0], x[1]), o  # two different samples went in
        assert torch.equal(x, y.flip(0)), f"output {o}: swapped batch, max-abs per sample {cb.per_sample_errors(x, y.flip(0))}"
        assert torch.equal(z[0], z[1]), f"output {o}: the same sample twice, max-abs {(z[0] - z[1]).abs().max().item():.3e}"
        assert torch.equal(z[0], x[0]), f"output {o}: sample a beside itself vs beside b, max-abs {(z[0] - x[0]).abs().max().item():.3e}"


def test_fused_stage_matches_seam_by_seam_two_pairs(cre_sd):
    """nnd_cre_stereo_refine against the seam-by-seam loop over the same kernels at B = 2, 104x168: all 8 outputs <= 5e-5, as
    test_cre_fused_stage_matches_seam_by_seam at B = 1.  With test_cascade_batched_vs_oracle this places an error inside or
    outside the fused call."""
    f1, f2 = (x.to(DEV) for x in cb.frames("b2_104x168_it4"))
    m = _model(cre_sd, 4)
    fused = _maps(m(f1, f2))
    m.fused_loop = False
    seam = _maps(m(f1, f2))
    assert len(fused) == len(seam) == 8
    errs = [cb.per_sample_errors(a, b) for a, b in zip(fused, seam)]
    _report("cre 2 x 104x168 fused vs seam-by-seam", errs)
    err, o, i = _worst(errs)
    assert err <= 5e-5, f"output {o}, sample {i}: {err:.3e}"


# ------------------------------------------------------------ entry points at B = 2, 128x192
def test_flow_init_and_two_stage_two_pairs(cre_sd, CR):
    """The flow_init entry (one stage of `iters` iterations at 1/8, seeded with the oracle's batched final flow) and the two-stage
    harness, each against the oracle's statement of it, <= 1e-4."""
    from nndepth_amd.cre_stereo import two_stage_forward
    f1, f2 = cb.frames("b2_128x192_it4")
    init = cb.oracle(cre_sd, "b2_128x192_it4")[-1]
    m = _model(cre_sd, 4)
    m.iters = 2
    outs = _maps(m(f1.to(DEV), f2.to(DEV), flow_init=init.to(DEV)))
    exp = CR.cre_stereo_forward(cre_sd, f1, f2, 2, flow_init=init)
    assert [tuple(o.shape) for o in outs] == [(2, 2, 128, 192)] * 2 and len(exp) == 2
    errs = _errors_by_sample(outs, exp)
    _report("cre 2 x 128x192 flow_init, 2 iterations", errs)
    err, o, i = _worst(errs)
    assert err <= 1e-4, f"flow_init: output {o}, sample {i}: {err:.3e}"
    outs = _maps(two_stage_forward(_model(cre_sd, 4), f1.to(DEV), f2.to(DEV)))
    exp = CR.cre_two_stage_forward(cre_sd, f1, f2, 4)
    assert [tuple(o.shape) for o in outs] == [(2, 2, 128, 192)] * 4 and len(exp) == 4
    errs = _errors_by_sample(outs, exp)
    _report("cre 2 x 128x192 two-stage", errs)
    err, o, i = _worst(errs)
    assert err <= 1e-4, f"two-stage: output {o}, sample {i}: {err:.3e}"


def test_last_and_test_mode_equal_all_two_pairs(cre_sd):
    f1, f2 = (x.to(DEV) for x in cb.frames("b2_128x192_it4"))
    m = _model(cre_sd, 4)
    full = _maps(m(f1, f2))
    m.outputs = "last"
    last = _maps(m(f1, f2))
    m.outputs = "all"
    assert len(full) == 8 and len(last) == 1
    assert not torch.equal(full[-1][0], full[-1][1])
    assert torch.equal(last[0], full[-1])
    m.test_mode = True
    assert torch.equal(m(f1, f2), full[-1])


def test_graphed_forward_equals_direct_two_pairs(cre_sd):
    """The captured forward replays bit-identically for two different batches of one shape (the second goes through the replay
    only)."""
    from nndepth_amd.graph import GraphedForward
    m = _model(cre_sd, 4)
    fwd = GraphedForward(m)
    finals = []
    for seeds in ((40, 41), (42, 43)):
        f1, f2 = (x.to(DEV) for x in cb.frames_of(seeds, 128, 192))
        direct = _maps(m(f1, f2))
        replay = fwd(f1, f2)
        assert len(replay) == len(direct) == 8
        for a, b in zip(direct, replay):
            assert torch.equal(a, b["up_disp"])
        finals.append(direct[-1])
    assert len(fwd._graphs) == 1 and not torch.equal(finals[0], finals[1])


def test_one_model_over_changing_batch_sizes(cre_sd):
    """One fp32 model (no calibration state) called with B = 3, then B = 1, then B = 2 at 72x104: the smaller batches equal, bit
    for bit, a fresh model called with that batch alone.  The update-block workspace, the encoder workspace and the ParamCache
    objects live across the calls; nothing in them may remember the batch stride of the B = 3 call."""
    f1, f2 = (x.to(DEV) for x in cb.frames("b3_72x104_it2"))
    m = _model(cre_sd, 2, arithmetic="fp32")
    first = _maps(m(f1, f2))
    assert len(first) == 4
    for sl in (slice(0, 1), slice(1, 3)):  # B = 1: sample 0; B = 2: samples 1 and 2, now at indices 0 and 1
        a, b = f1[sl].contiguous(), f2[sl].contiguous()
        used = _maps(m(a, b))
        fresh = _maps(_model(cre_sd, 2, arithmetic="fp32")(a, b))
        assert len(used) == len(fresh) == 4
        for o, (x, y) in enumerate(zip(used, fresh)):
            assert torch.equal(x, y), f"B={a.shape[0]} output {o}: max-abs per sample {cb.per_sample_errors(x, y)}"
