"""GPU: StereoEvalCriterion / StereoEvalMean / downsample_gt on the device (csrc/stereo_eval.hip) against the fixture
tests/golden/stereo_eval.npz: r = the reference's own fp32 results, f = the contract in float64
(scripts/make_golden_stereo_eval.py; the cases' inputs regenerate from their names, tests/stereo_eval_cases.py).

Accuracy bar, per case, output and column with a finite f:  |d - f| <= max(|r - f|, 2^-24 * max(1, |f|))  — the device result d is
at least as close to float64 as the reference's fp32 result is, down to the resolution of the fp32 value the reference returns;
2^-24 * max(1, |f|) alone where the reference has no counterpart (count, l1, and the `below` fractions and the loss of a case
with a mask).  A double sum of at most 2e4 non-negative terms in any order is within n * 2^-53 relative: orders of magnitude
inside the bar."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import stereo_eval_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NA, NB = len(sc.ABOVE), len(sc.BELOW)


@pytest.fixture(scope="module")
def fx(gold):
    g = gold("stereo_eval.npz")
    assert tuple(json.loads(str(g["names"]))) == sc.NAMES and tuple(json.loads(str(g["columns"]))) == sc.COLUMNS
    return {n: {k: g[f"{n}/{k}"] for k in ("r", "has_r", "f", "counts", "loss")} for n in sc.NAMES}


def _to_dev(case: sc.Case) -> sc.Case:
    """The case on the device with the layout it has on the CPU (R: slices of one stacked tensor; V: a cropped view)."""
    outs = case.outputs
    base = outs[0]._base if outs[0]._base is not None else None
    if base is None:
        dev_outs = [o.to(DEV) for o in outs]
    else:
        b = base.to(DEV)
        dev_outs = [b.as_strided(o.size(), o.stride(), o.storage_offset()) for o in outs]
    return sc.Case(case.gt.to(DEV), dev_outs, None if case.mask is None else case.mask.to(DEV), case.max_flow)


@pytest.fixture(scope="module")
def inputs():
    """name -> Case on the device; not modified by any test."""
    return {name: _to_dev(sc.make_case(name)) for name in sc.NAMES}


def _crit(max_flow=sc.MAX_FLOW):
    from nndepth_amd.prepost import StereoEvalCriterion
    return StereoEvalCriterion(sc.ABOVE, sc.BELOW, max_flow=max_flow, gamma=sc.GAMMA)


def _run(gt, outputs, mask=None, max_flow=sc.MAX_FLOW):
    """((N,K) metrics, loss) of one call as numpy / float."""
    m, loss = _crit(max_flow).metrics_tensor(gt, outputs, mask)
    return m.cpu().numpy(), float(loss.cpu())


@pytest.fixture(scope="module")
def device_results(inputs):
    """name -> ((N,K) float64, loss), computed once."""
    return {name: _run(c.gt, c.outputs, c.mask, c.max_flow) for name, c in inputs.items()}


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


def _bar(f, r=None):
    floor = 2.0 ** -24 * max(1.0, abs(f))
    return floor if r is None else max(abs(r - f), floor)


def test_the_case_layouts_survive_the_upload(inputs):
    r, v = inputs["R"].outputs, inputs["V"].outputs[0]
    assert len({o.untyped_storage().data_ptr() for o in r}) == 1 and r[1].data_ptr() - r[0].data_ptr() == 40 * 56 * 4
    assert not v.is_contiguous() and v.stride() == (44 * 60, 44 * 60, 60, 1)


@pytest.mark.parametrize("name,size", [("G2", (37, 62)), ("G3", (24, 41)), ("G4", (25, 42)), ("C", (18, 26)), ("C", (11, 17)),
                                       ("A", (37, 53)), ("A", (37, 50))])
def test_min_pool_nearest_is_the_references_three_lines(inputs, name, size):
    """Bit-equal to -max_pool2d(-gt, s) / s and F.interpolate run by torch on the CPU (C: the 2-channel ground truth, pooled
    12x17 read at 11x17; A: the equal size, and scale 1 with resampled columns)."""
    from nndepth_amd.prepost import downsample_gt
    gt = inputs[name].gt
    want = sc.gt_at(gt.cpu(), size)
    got = downsample_gt(gt, size)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(got.cpu().view(torch.int32), want.contiguous().view(torch.int32))


def test_eval_criterion_on_a_coarse_output_equals_the_parent_expression(inputs):
    """EvalCriterion's size-mismatch branch: the dict the PyTorch expression it replaces gives, fed back as an equal-size map."""
    from nndepth_amd.prepost import EvalCriterion
    c = inputs["G2"]
    pred = c.outputs[0]
    gt_cpu = c.gt.cpu()
    scale = gt_cpu.shape[-1] // pred.shape[-1]
    g = -torch.nn.functional.max_pool2d(-gt_cpu, kernel_size=scale) / scale
    g = torch.nn.functional.interpolate(g, size=pred.shape[-2:])
    crit = EvalCriterion(dict(sc.ABOVE))
    got, want = crit(c.gt, pred), crit(g.to(DEV), pred)
    assert list(got) == ["epe"] + list(sc.ABOVE) and got == want


def _same32(got: dict, cols) -> bool:
    """The dict's values are Python floats with the bits of the float64 columns `cols` rounded to fp32."""
    want = [float(np.float32(x)) for x in cols]
    return all(type(v) is float for v in got.values()) and _same(list(got.values()), want)


@pytest.mark.parametrize("name", ["A", "B", "T", "C", "D", "M", "E", "G2", "G3", "G4", "V"])
def test_eval_criterion_is_the_fp32_rounding_of_the_single_output_row(inputs, device_results, name):
    """EvalCriterion is StereoEvalCriterion with one output: epe and the `above` columns of row 0 rounded to fp32, NaN where they
    are NaN (E).  D: the 1-channel ground truth under a 2-channel map; G2, G3, G4: ragged pooling; V: a cropped view read where it
    lies; B, E: a mask and the empty mask; M: a binding max_flow."""
    from nndepth_amd.prepost import EvalCriterion
    c = inputs[name]
    assert len(c.outputs) == 1
    got = EvalCriterion(dict(sc.ABOVE), max_flow=c.max_flow)(c.gt, c.outputs[0], c.mask)
    row = device_results[name][0][0]
    assert list(got) == ["epe"] + list(sc.ABOVE)
    assert _same32(got, [row[0]] + list(row[3:3 + NA])), (name, got, row)
    assert [math.isnan(v) for v in got.values()] == [bool(np.isnan(x)) for x in [row[0]] + list(row[3:3 + NA])]


def test_eval_criterion_takes_a_mask_of_any_dtype_and_shape(inputs):
    from nndepth_amd.prepost import EvalCriterion
    c = inputs["B"]
    crit = EvalCriterion(dict(sc.ABOVE), max_flow=c.max_flow)
    assert c.mask.dtype == torch.bool and c.mask.dim() == 4 and c.mask.shape[1] == 1
    want = crit(c.gt, c.outputs[0], c.mask)
    for mask in (c.mask.float(), c.mask.reshape(-1)):
        got = crit(c.gt, c.outputs[0], mask)
        assert list(got) == list(want) and _same(list(got.values()), list(want.values()))


def test_eval_criterion_keeps_a_threshold_key_that_is_a_column_name(inputs, device_results):
    from nndepth_amd.prepost import EvalCriterion
    c = inputs["A"]
    thr = list(sc.ABOVE.values())[0]
    got = EvalCriterion({"count": thr}, max_flow=c.max_flow)(c.gt, c.outputs[0], c.mask)
    row = device_results["A"][0][0]
    assert list(got) == ["epe", "count"] and _same32(got, [row[0], row[3]])


@pytest.mark.parametrize("name", sc.NAMES)
def test_at_least_as_close_to_float64_as_the_reference(fx, device_results, name):
    (d, dloss), w = device_results[name], fx[name]
    f, r, has = w["f"], w["r"], w["has_r"]
    assert d.shape == f.shape
    for i in range(f.shape[0]):
        for k, col in enumerate(sc.COLUMNS):
            bound = _bar(f[i, k], r[i, k] if has[i, k] else None) if math.isfinite(f[i, k]) else None
            print(f"{name} output {i} {col}: d = {float(d[i, k])!r}, f = {float(f[i, k])!r}, r = {float(r[i, k])!r}, bound on |d - f| = {bound!r}")
    loss_f, loss_r, loss_has = w["loss"]
    loss_bound = _bar(loss_f, loss_r if loss_has else None)
    print(f"{name} loss: d = {dloss!r}, f = {float(loss_f)!r}, r = {float(loss_r)!r}, bound on |d - f| = {loss_bound!r}")
    for i in range(f.shape[0]):
        for k, col in enumerate(sc.COLUMNS):
            if math.isfinite(f[i, k]):
                assert abs(d[i, k] - f[i, k]) <= _bar(f[i, k], r[i, k] if has[i, k] else None), (name, i, col, d[i, k], f[i, k], r[i, k])
            assert math.isnan(d[i, k]) == math.isnan(f[i, k]), (name, i, col, d[i, k])  # NaN exactly where f is NaN
    assert abs(dloss - loss_f) <= loss_bound, (name, dloss, loss_f, loss_r)


@pytest.mark.parametrize("name", sc.NAMES)
def test_counts_are_the_fixtures_integers_and_fractions_their_quotients(fx, device_results, name):
    d, counts = device_results[name][0], fx[name]["counts"]
    for i in range(d.shape[0]):
        n = int(counts[i, 0])
        assert d[i, 1] == n, (name, i, d[i, 1], n)
        if n == 0:
            assert np.isnan(d[i, 3:]).all() and np.isnan(d[i, 0]) and d[i, 2] == 0.0
            continue
        want = [float(c) / float(n) for c in counts[i, 1:]]
        assert _same(d[i, 3:], want), (name, i, d[i, 3:], want)  # bit-equal to count_k / count in double


def test_closed_form_counts_of_the_strict_comparisons(device_results):
    d = device_results["T"][0][0]
    assert d[1] == 320 and np.rint(d[3:] * 320).tolist() == [128, 64, 64, 128, 192, 256]
    assert abs(d[0] - 2.15) <= 2.0 ** -24 * 2.15 and _same(d[0], d[2])  # one channel, every pixel valid: l1 is the epe


@pytest.mark.parametrize("name", ["R", "S"])
def test_rows_of_a_sequence_equal_the_single_output_calls(inputs, device_results, name):
    c = inputs[name]
    d, dloss = device_results[name]
    N = len(c.outputs)
    for i, o in enumerate(c.outputs):
        one, one_loss = _run(c.gt, o, c.mask, c.max_flow)
        assert one.shape == (1, sc.K) and _same(one[0], d[i]), (name, i, one[0], d[i])
        assert _same(one_loss, d[i, 2])  # a single output: gamma^0 * l1
    loss = 0.0
    for i in range(N):
        loss += sc.GAMMA ** (N - 1 - i) * d[i, 2]
    assert _same(dloss, loss), (dloss, loss)
    if name == "S":  # the order of the outputs inside a call does not change a row
        rev, _ = _run(c.gt, c.outputs[::-1], c.mask, c.max_flow)
        assert _same(rev[::-1], d)


def test_strided_view_equals_its_contiguous_copy(inputs, device_results):
    c = inputs["V"]
    m, loss = _run(c.gt, [c.outputs[0].contiguous()])
    assert _same(m, device_results["V"][0]) and _same(loss, device_results["V"][1])


def _shifted(t: torch.Tensor) -> torch.Tensor:
    """The same values one element off 16-byte alignment."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = flat[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 != 0
    return out


def test_vector_and_scalar_loads_give_the_same_bits(inputs, device_results):
    """R (40x56, aligned slices, a mask) and a coarse 2-channel pair under a 1-channel 32x48 ground truth take the 16-byte path;
    the same values one element off alignment take the scalar one."""
    c = inputs["R"]
    assert all(o.data_ptr() % 16 == 0 and o.shape[-1] % 4 == 0 for o in c.outputs)
    m, loss = _run(c.gt, [_shifted(o) for o in c.outputs], c.mask)
    assert _same(m, device_results["R"][0]) and _same(loss, device_results["R"][1])
    m, _ = _run(c.gt, c.outputs, _shifted(c.mask.view(torch.uint8)))
    assert _same(m, device_results["R"][0])
    m, _ = _run(c.gt, c.outputs, c.mask[:, 0])  # (B,h,w)
    assert _same(m, device_results["R"][0])
    gt = ((2.0 * sc._u("stereo_eval/gpu/coarse/gt", (1, 1, 32, 48)) - 1.0) * 60.0).astype(np.float32)
    gt = torch.from_numpy(gt)
    outs = []
    for i, (h, w) in enumerate(((8, 12), (16, 24), (32, 48))):
        noise = torch.from_numpy((2.0 * sc._u(f"stereo_eval/gpu/coarse/noise{i}", (1, 2, h, w)) - 1.0) * np.float32(4.0))
        outs.append((sc.gt_at(gt, (h, w)).expand(1, 2, h, w) + noise).contiguous())
    f, loss_f, counts = sc.contract64(sc.Case(gt, outs, None, sc.MAX_FLOW))
    dev = [o.to(DEV) for o in outs]
    assert all(o.data_ptr() % 16 == 0 for o in dev)
    a, la = _run(gt.to(DEV), dev)
    b, lb = _run(_shifted(gt.to(DEV)), [_shifted(o) for o in dev])
    assert _same(a, b) and _same(la, lb)
    assert np.array_equal(a[:, 1], counts[:, 0]) and _same(a[:, 3:], counts[:, 1:] / counts[:, :1].astype(np.float64))
    assert (np.abs(a - f) <= 2.0 ** -24 * np.maximum(1.0, np.abs(f))).all() and abs(la - loss_f) <= 2.0 ** -24 * max(1.0, loss_f)


@pytest.mark.parametrize("name", ["B", "S", "R"])
def test_same_bits_run_to_run_and_whatever_the_buffers_held(inputs, device_results, name):
    from nndepth_amd._lib import check, lib
    from nndepth_amd.ops import _p, _stream
    c = inputs[name]
    for _ in range(2):
        m, loss = _run(c.gt, c.outputs, c.mask, c.max_flow)
        assert _same(m, device_results[name][0]) and _same(loss, device_results[name][1])
    desc, d, keep = _crit(c.max_flow).describe(c.gt, c.outputs, c.mask)
    n = desc.num_outputs
    nbytes = int(lib.nnd_stereo_eval_workspace_bytes(n))
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full(((n * sc.K + 1) * 8,), 0xFF, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(d):
        check(lib.nnd_stereo_eval(C.byref(desc), _p(ws), nbytes, _p(out), _stream(d)), "stereo_eval")
    got = out.view(torch.float64).cpu().numpy()
    assert _same(got[:-1].reshape(n, sc.K), device_results[name][0]) and _same(got[-1], device_results[name][1])


def test_call_returns_one_dict_per_output(inputs, device_results):
    c = inputs["S"]
    res = _crit()(c.gt, [{"up_disp": o} for o in c.outputs])
    assert len(res) == 5 and all(list(r) == list(sc.COLUMNS) and all(type(v) is float for v in r.values()) for r in res)
    assert _same([list(r.values()) for r in res], device_results["S"][0])
    e = inputs["E"]
    res = _crit()(e.gt, e.outputs[0], e.mask)
    assert res[0]["count"] == 0.0 and res[0]["l1"] == 0.0 and all(math.isnan(res[0][k]) for k in sc.COLUMNS if k not in ("count", "l1"))


def test_dataset_mean_is_np_mean_of_the_per_pair_values(inputs):
    """evaluate.py:141-169 over three pairs of 16x16 crops (cropped views: read where they lie), then with case E among them:
    the columns that are NaN for E become NaN, count and l1 do not."""
    from nndepth_amd._lib import NndError
    from nndepth_amd.prepost import StereoEvalMean
    crit = _crit()
    crop = lambda n: (inputs[n].gt[..., :16, :16], [inputs[n].outputs[0][..., :16, :16], inputs[n].outputs[0][..., 4:20, 8:24]], None)
    pairs = [crop("A"), crop("V"), crop("M")]
    e = inputs["E"]
    with_e = pairs[:2] + [(e.gt, [e.outputs[0], e.outputs[0]], e.mask)]
    for batch, nan_cols in ((pairs, ()), (with_e, ("epe",) + tuple(sc.ABOVE) + tuple(sc.BELOW))):
        mean = StereoEvalMean(sc.ABOVE, sc.BELOW, gamma=sc.GAMMA)
        dicts = []
        for gt, outs, mask in batch:
            mean.update(gt, outs, mask)
            dicts.append(crit(gt, outs, mask))
        curve = mean.curve()
        assert len(curve) == 2
        for i in range(2):
            assert list(curve[i]) == list(sc.COLUMNS)
            for k in sc.COLUMNS:
                want = float(np.mean([d[i][k] for d in dicts]))
                assert math.isnan(want) == (k in nan_cols) == math.isnan(curve[i][k]), (i, k, want, curve[i][k])
                if not math.isnan(want):
                    assert abs(curve[i][k] - want) <= 2.0 ** -52 * abs(want), (i, k, curve[i][k], want)
        res = mean.result()
        assert list(res) == ["epe"] + list(sc.ABOVE) + list(sc.BELOW)
        assert all(_same(res[k], curve[-1][k]) for k in res)
    with pytest.raises(NndError, match="outputs"):
        mean.update(pairs[0][0], pairs[0][1][:1])
    with pytest.raises(NndError, match="sizes"):
        mean.update(inputs["A"].gt, [inputs["A"].outputs[0]] * 2)


def test_bad_inputs_are_refused_by_name(inputs):
    from nndepth_amd._lib import NndError
    c = inputs["B"]
    crit = _crit()
    with pytest.raises(NndError, match="valid_mask"):
        crit(c.gt, c.outputs, c.mask.float())
    with pytest.raises(NndError, match="valid_mask"):
        crit(c.gt, [c.outputs[0], c.outputs[0][..., :16, :23]], c.mask)
    with pytest.raises(NndError, match="no CPU fallback"):
        crit(c.gt, c.outputs, c.mask.cpu())
    with pytest.raises(NndError, match="HIP device"):
        crit(c.gt, [c.outputs[0].cpu()])
    with pytest.raises(NndError, match="batch size"):
        crit(c.gt, [c.outputs[0][:2]])
    with pytest.raises(NndError, match="channels"):
        crit(c.gt.expand(-1, 3, -1, -1), [c.outputs[0].expand(-1, 2, -1, -1)])
    with pytest.raises(NndError, match="wider"):
        crit(c.gt[..., :40], c.outputs)


def _forward_maps(model, sd, frames):
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    with torch.no_grad():
        return model(*(x.to(DEV) for x in frames))


def _synthetic_gt(tag, shape):
    return torch.from_numpy(((2.0 * sc._u(tag, shape) - 1.0) * 8.0).astype(np.float32)).to(DEV)


def test_a_raft_forwards_list_goes_straight_in(raft_sd):
    """64x128: the narrowest frame whose fourth correlation level (width / 64) still has the two columns the lookup needs."""
    from nndepth_amd import weightgen
    from nndepth_amd.raft_stereo import BaseRAFTStereo
    outs = _forward_maps(BaseRAFTStereo(iters=4, context_dim=64), raft_sd, weightgen.synthetic_frames(0, 1, 64, 128))
    assert len(outs) == 4 and all(tuple(o["up_disp"].shape) == (1, 1, 64, 128) for o in outs)
    gt = _synthetic_gt("stereo_eval/gpu/raft/gt", (1, 1, 64, 128))
    m, loss = _run(gt, outs)
    assert m.shape == (4, sc.K) and np.isfinite(m).all() and (m[:, 1] == 64 * 128).all()
    for i, o in enumerate(outs):
        assert _same(_run(gt, o["up_disp"])[0][0], m[i])
    want = 0.0
    for i in range(4):
        want += sc.GAMMA ** (3 - i) * m[i, 2]
    assert _same(loss, want)


def test_a_cre_forwards_list_goes_straight_in(cre_sd):
    from nndepth_amd import weightgen
    from nndepth_amd.cre_stereo import CREStereoBase
    outs = _forward_maps(CREStereoBase(iters=2), cre_sd, weightgen.synthetic_frames(3, 1, 128, 192))
    shapes = [tuple(o["up_disp"].shape) for o in outs]
    assert len(outs) == 4 and len(set(shapes)) == 3 and all(s[1] == 2 for s in shapes), shapes
    gt = _synthetic_gt("stereo_eval/gpu/cre/gt", (1, 1, 128, 192))  # one channel under 2-channel outputs, as the script has it
    m, loss = _run(gt, outs)
    assert m.shape == (4, sc.K) and np.isfinite(m).all()
    for i, o in enumerate(outs):
        one = _run(gt, o["up_disp"])[0][0]
        assert _same(one, m[i]) and one[1] == shapes[i][2] * shapes[i][3]
    f, loss_f, counts = sc.contract64(sc.Case(gt.cpu(), [o["up_disp"].cpu() for o in outs], None, sc.MAX_FLOW))
    assert np.array_equal(m[:, 1], counts[:, 0]) and _same(m[:, 3:], counts[:, 1:] / counts[:, :1].astype(np.float64))
    assert (np.abs(m - f) <= 2.0 ** -24 * np.maximum(1.0, np.abs(f))).all() and abs(loss - loss_f) <= 2.0 ** -24 * max(1.0, abs(loss_f))


@pytest.mark.parametrize("Cg", [1, 3])
def test_three_channel_outputs_take_the_general_kernel(Cg):
    """Channel counts other than 1 and 2 run the instance whose channel loop has a runtime bound: a same-size and a coarse
    3-channel output, ragged rows, against the float64 contract stated in the test."""
    gt = torch.from_numpy(((2.0 * sc._u(f"stereo_eval/gpu/c3/{Cg}/gt", (2, Cg, 30, 45)) - 1.0) * 60.0).astype(np.float32))
    outs = []
    for i, (h, w) in enumerate(((30, 45), (15, 22))):
        noise = torch.from_numpy((2.0 * sc._u(f"stereo_eval/gpu/c3/{Cg}/noise{i}", (2, 3, h, w)) - 1.0) * np.float32(4.0))
        outs.append((sc.gt_at(gt, (h, w)).expand(2, 3, h, w) + noise).contiguous())
    f, loss_f, counts = sc.contract64(sc.Case(gt, outs, None, sc.MAX_FLOW))
    m, loss = _run(gt.to(DEV), [o.to(DEV) for o in outs])
    assert np.array_equal(m[:, 1], counts[:, 0]) and _same(m[:, 3:], counts[:, 1:] / counts[:, :1].astype(np.float64))
    assert (np.abs(m - f) <= 2.0 ** -24 * np.maximum(1.0, np.abs(f))).all() and abs(loss - loss_f) <= 2.0 ** -24 * max(1.0, abs(loss_f))
