"""GPU: stereo geometry through the HIP path (csrc/geometry.hip) against the closed-form oracles of tests/geometry_cases.py and
the fixture tests/golden/geometry.npz (scripts/make_golden_geometry.py).  Every comparison is an equality: depth, disparity and
point bits, masks, offsets, the finite err values of the left-right check; the model outputs of `both_views` against one
forward of the batch built with torch ops."""
import numpy as np
import pytest
import torch

import geometry_cases as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(x) -> np.ndarray:
    x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _same_bits(got, want, what):
    a, b = _bits(got), _bits(want)
    assert a.shape == b.shape, what
    n = int((a != b).sum())
    print(f"[geometry] {what}: {n} of {a.size} values differ in their bits")
    assert n == 0, what


def _K(B, H, W):
    """(B,3,3) intrinsics, a different camera per sample, principal point off the pixel grid."""
    K = np.zeros((B, 3, 3), np.float32)
    for b in range(B):
        K[b] = [[320.5 + 7 * b, 0, W / 2 - 0.3 + b], [0, 318.25 - 3 * b, H / 2 + 0.1 * b], [0, 0, 1]]
    return K


@pytest.mark.parametrize("shape", [(2, 1, 5, 7), (1, 1, 33, 130)])
@pytest.mark.parametrize("sign", ["negative", "positive"])
def test_to_depth_bits_and_mask(shape, sign):
    from nndepth_amd.scene import Camera, Disparity
    B, _, H, W = shape
    d, _ = G.special_disparity(B, H, W, seed=B * 100 + W, sign=sign)
    K = _K(B, H, W)
    fx = K[:, 0, 0]
    g = np.random.default_rng(5)
    mask = g.random((B, 1, H, W)) < 0.8
    cam = Camera(_t(K))
    for kw, baseline in ((dict(), 0.25), (dict(min_disp=0.5), 0.25), (dict(max_depth=20.0), 0.25),
                         (dict(min_disp=0.5, max_depth=60.0, valid_mask=mask), 0.54)):
        okw = {("mask" if k == "valid_mask" else k): v for k, v in kw.items()}
        want_z, want_ok = G.to_depth(d, fx, baseline, sign, **okw)
        if "valid_mask" in kw:
            kw = dict(kw, valid_mask=_t(mask) if B == 2 else _t(mask[:, 0].astype(np.uint8)))  # bool (B,1,H,W) / uint8 (B,H,W)
        got = Disparity(_t(d), sign, baseline=baseline).to_depth(cam, **kw)
        assert got.data.shape == (B, 1, H, W) and got.valid_mask.dtype == torch.uint8 and got.valid_mask.shape == (B, 1, H, W)
        assert np.array_equal(got.valid_mask.cpu().numpy(), want_ok), (shape, sign, kw)
        _same_bits(got.data, want_z, f"to_depth {shape} {sign} {sorted(okw)}")
    # one fx for the whole batch, as a number and as a host (3,3) intrinsic; the baseline given to the call wins
    want_z, want_ok = G.to_depth(d, [320.0], 0.25, sign)
    for c in (320.0, torch.tensor([[320.0, 0, 1], [0, 320.0, 1], [0, 0, 1]]), Camera(torch.tensor([[[320.0, 0, 1], [0, 300.0, 1], [0, 0, 1]]]))):
        got = Disparity(_t(d), sign, baseline=9.0).to_depth(c, baseline=0.25)
        assert np.array_equal(got.valid_mask.cpu().numpy(), want_ok)
        _same_bits(got.data, want_z, f"to_depth {shape} {sign} fx = 320")


def test_to_depth_max_depth_on_a_representable_boundary():
    """fx * baseline = 80: disparity 4 gives exactly z = 20 = max_depth (valid), one ulp less disparity gives z > 20 (invalid)."""
    from nndepth_amd.scene import Disparity
    d, idx = G.special_disparity(2, 5, 7, seed=1)
    got = Disparity(_t(d), baseline=0.25).to_depth(320.0, max_depth=20.0)
    z, ok = got.data[0, 0].flatten().cpu().numpy(), got.valid_mask[0, 0].flatten().cpu().numpy()
    assert ok[idx].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0]
    assert z[idx[9]] == 20.0 and z[idx[10]] == 0.0 and 0.0 < z[idx[11]] < 20.0


def test_to_depth_reads_a_channel_slice_where_it_lies():
    from nndepth_amd.scene import Disparity
    g = np.random.default_rng(3)
    two = -(g.random((2, 2, 5, 7)) * 40 + 0.5).astype(np.float32)
    dev = _t(two)
    for c in (0, 1):
        view = dev[:, c:c + 1]
        assert not view.is_contiguous() and view.stride(0) == 70
        want_z, want_ok = G.to_depth(two[:, c:c + 1], [311.0], 0.3)
        got = Disparity(view, baseline=0.3).to_depth(311.0)
        assert np.array_equal(got.valid_mask.cpu().numpy(), want_ok)
        _same_bits(got.data, want_z, f"to_depth channel {c} of (2,2,5,7)")
    half = dev.reshape(4, 1, 5, 7)[2:]  # half of a stacked batch
    _same_bits(Disparity(half, baseline=0.3).to_depth(311.0).data, G.to_depth(two.reshape(4, 1, 5, 7)[2:], [311.0], 0.3)[0], "half batch")


def test_to_disparity_equals_the_reference_expression_on_the_golden_crop(gold):
    from nndepth_amd.scene import Depth
    g = gold("geometry.npz")
    z = _t(g["ta_depth"][None])
    fx, baseline = float(g["ta_fx"]), float(g["ta_baseline"])
    disp = Depth(z).to_disparity(fx, baseline)
    assert disp.disp_sign == "negative" and disp.baseline == baseline and disp.data.shape == (1, 1, 48, 64)
    _same_bits(disp.data[0], g["ta_disp"], "to_disparity vs -BASELINE * FX / (depth + 1e-8)")
    pos = Depth(z).to_disparity(fx, baseline, disp_sign="positive")
    assert pos.disp_sign == "positive"
    _same_bits(pos.data[0], -g["ta_disp"], "to_disparity positive")
    # per-sample fx, another eps, zeros in the map (c / eps)
    zz = np.concatenate([g["ta_depth"][None], g["ta_depth"][None] * 2])
    zz[1, 0, 0, :5] = 0.0
    K = _K(2, 48, 64)
    got = Depth(_t(zz)).to_disparity(_t(K), 0.54, eps=1e-3)
    _same_bits(got.data, G.to_disparity(zz, K[:, 0, 0], 0.54, eps=1e-3), "to_disparity per-sample fx")
    # the round trip is close, not exact (two roundings): the back-converted depth equals the oracle's, not the input
    back = disp.to_depth(fx)
    _same_bits(back.data, g["ta_back_depth"], "to_depth(to_disparity(z))")
    assert np.array_equal(back.valid_mask.cpu().numpy(), g["ta_back_valid"])
    _same_bits(back.to_points_map(_t(g["ta_K"])), g["ta_points"], "points of the golden crop")


def _point_masks(B, H, W):
    g = np.random.default_rng(11)
    last = np.zeros((B, 1, H, W), bool)
    last[-1, 0, -1, -1] = True
    return {"all": np.ones((B, 1, H, W), bool), "none": np.zeros((B, 1, H, W), bool), "last": last,
            "random70": g.random((B, 1, H, W)) < 0.7}


# 2x1x40x70: 11 workgroups of 256 pixels per sample, the last ragged; 1x1x520x510: 1036 workgroup counts, more than the 1024 threads
# of the scan, so that a thread scans a chunk of two
@pytest.mark.parametrize("shape", [(3, 1, 9, 13), (2, 1, 40, 70), (1, 1, 520, 510)])
def test_points_dense_and_compacted(shape):
    from nndepth_amd.scene import Camera, Depth
    B, _, H, W = shape
    g = np.random.default_rng(B * H)
    z = (g.random(shape) * 30 + 0.2).astype(np.float32)
    feats = g.standard_normal((B, 3, H, W)).astype(np.float32)
    K = _K(B, H, W)
    cam_np, cam = G.cam_of(K, B), Camera(_t(K))
    zd, fd = _t(z), _t(feats)
    for name, mask in _point_masks(B, H, W).items():
        what = f"points {shape} mask {name}"
        for md in (_t(mask), _t(mask[:, 0].astype(np.uint8))):
            depth = Depth(zd, md)
            _same_bits(depth.to_points_map(cam), G.points_map(z, cam_np, mask), what + " dense")
        want_p, want_f, want_off = G.compact(z, cam_np, mask, feats)
        pts, fo, off = depth.points_tensor(cam, fd)
        assert pts.shape == (B * H * W, 3) and fo.shape == (B * H * W, 3) and off.dtype == torch.int64 and off.shape == (B + 1,)
        assert off.cpu().numpy().tolist() == want_off.tolist(), what
        n = int(want_off[-1])
        if name == "random70":
            assert all(int(c) % 64 for c in np.diff(want_off))  # no sample's count is a multiple of the wave size
        _same_bits(pts[:n], want_p, what + " rows")  # rows past offsets[B] are unspecified and not read
        _same_bits(fo[:n], want_f, what + " features")
        pts2, fo2, off2 = depth.points_tensor(cam, fd)  # the same bytes on a second run
        assert torch.equal(off, off2) and torch.equal(pts[:n], pts2[:n]) and torch.equal(fo[:n], fo2[:n])
        p3, none, off3 = depth.points_tensor(cam)
        assert none is None and torch.equal(off3, off) and torch.equal(p3[:n], pts[:n])
        per = depth.to_points(cam, fd)
        assert len(per) == B
        for b, (pb, fb) in enumerate(per):
            lo, hi = int(want_off[b]), int(want_off[b + 1])
            assert pb.shape == (hi - lo, 3) and fb.shape == (hi - lo, 3)
            assert np.array_equal(_bits(pb), _bits(want_p[lo:hi])) and np.array_equal(_bits(fb), _bits(want_f[lo:hi]))
        assert [tuple(p.shape) for p in depth.to_points(cam)] == [(int(c), 3) for c in np.diff(want_off)]
    # no mask: every pixel, and a single (3,3) camera for the whole batch
    pts, _, off = Depth(zd).points_tensor(_t(K[0]))
    assert off.cpu().tolist() == [b * H * W for b in range(B + 1)]
    _same_bits(pts, G.compact(z, G.cam_of(K[0], B))[0], f"points {shape} without a mask")


@pytest.mark.parametrize("name", ["12x40", "7x33", "3x5", "2x9x70"])
def test_lr_consistency_on_dyadic_scenes(name, gold):
    from nndepth_amd import geometry
    mL, mR = G.lr_cases()[name]
    g = gold("geometry.npz")
    thr = G.LR_THRESHOLD
    for sl, sr, flip in (("negative", "negative", False), ("negative", "negative", True), ("positive", "negative", True),
                         ("negative", "positive", False)):
        dl, dr = G.stored(mL, sl), G.stored(mR, sr)
        dr = np.ascontiguousarray(dr[..., ::-1]) if flip else dr  # the same data, stored mirrored
        occ64, err64 = G.lr(dl, dr, thr, sl, sr, flip, dtype=np.float64)
        fin = np.isfinite(err64)
        assert np.abs(err64[fin] - thr).min() >= 2.0 ** -10  # a condition on the inputs; no pixel is excluded
        assert np.array_equal(occ64, g[f"lr_{name}_occ"])
        occ, err = geometry.lr_consistency(_t(dl), _t(dr), thr, sl, sr, right_flipped=flip, return_error=True)
        assert occ.dtype == torch.uint8 and occ.shape == dl.shape and err.shape == dl.shape
        got_err = err.cpu().numpy()
        nd = int((occ.cpu().numpy() != occ64).sum())
        print(f"[geometry] lr_consistency {name} {sl}/{sr} flipped={flip}: {nd} mask pixels differ, {100 * occ64.mean():.1f} % occluded")
        assert nd == 0
        assert np.array_equal(np.isfinite(got_err), fin) and np.array_equal(np.isnan(got_err), np.isnan(err64))
        assert np.array_equal(got_err[fin].astype(np.float64), err64[fin])
        assert np.all(np.isposinf(got_err[~fin & ~np.isnan(err64)]))
        only = geometry.lr_consistency(_t(dl), _t(dr), thr, sl, sr, right_flipped=flip)
        assert torch.equal(only, occ)
    # the decided-early pixels of the batch case: NaN, inf, wrong sign, out of frame on the left; -0 is a disparity of 0
    if name == "2x9x70":
        occ = g["lr_2x9x70_occ"]
        assert occ[1, 0, 0, 3] == 1 and occ[1, 0, 0, 9] == 1 and occ[1, 0, 1, 2] == 1 and occ[1, 0, 2, 5] == 1 and occ[1, 0, 0, 69] == 0
        assert occ[1, 0, 4, 20] == 1 and np.isnan(g["lr_2x9x70_err"][1, 0, 4, 20])  # a NaN on the right: occluded


def test_lr_consistency_reads_strided_maps_in_place():
    from nndepth_amd import geometry
    mL, mR = G.lr_cases()["2x9x70"]
    two = _t(np.concatenate([-mL, -mR[..., ::-1]], 1))  # (2,2,9,70): channel 0 = left, channel 1 = right, mirrored
    occ = geometry.lr_consistency(two[:, :1], two[:, 1:], G.LR_THRESHOLD, right_flipped=True)
    assert np.array_equal(occ.cpu().numpy(), G.lr(-mL, -mR, G.LR_THRESHOLD)[0])


def _both_views_checks(model, fwd, left, right):
    from nndepth_amd import geometry, scene
    B = left.shape[0]
    f1 = torch.cat([left, right.flip(-1)])
    f2 = torch.cat([right, left.flip(-1)])
    g1, g2 = geometry.pair_both_views(left, right)
    assert torch.equal(g1, f1) and torch.equal(g2, f2)
    want = model(f1, f2)[-1]["up_disp"].clone()
    dl, dr = geometry.both_views(fwd, left, right)
    assert dl.shape == dr.shape == (B, 1, *left.shape[-2:])
    assert torch.equal(dl, want[:B, :1]) and torch.equal(dr, want[B:, :1])
    mask = geometry.lr_consistency(dl, dr, 1.0, right_flipped=True).clone()
    out = geometry.occlusion(fwd, left, right, threshold=1.0)
    assert isinstance(out, scene.Disparity) and out.disp_sign == "negative" and out.baseline is None
    assert torch.equal(out.data, want[:B, :1]) and out.occlusion.dtype == torch.uint8 and torch.equal(out.occlusion, mask)
    return out


def test_both_views_and_occlusion_raft(raft_sd):
    """64x128, not 64x96: the four-level correlation pyramid of BaseRAFTStereo needs W / 8 >= 16 (at 64x96 the library refuses the
    forward itself, "lookup: level 3 has width 1 < 2"), so 128 is the smallest width this model runs at."""
    from nndepth_amd import weightgen
    from nndepth_amd.graph import GraphedForward
    from nndepth_amd.raft_stereo import BaseRAFTStereo
    m = BaseRAFTStereo(iters=2, context_dim=64)
    m.load_state_dict(raft_sd, strict=True)
    m = m.to(DEV).eval()
    left, right = (x.to(DEV) for x in weightgen.synthetic_frames(5, 1, 64, 128))
    _both_views_checks(m, m, left, right)
    fwd = GraphedForward(m)
    for seed in (5, 6):  # the second pair goes through the replay only
        left, right = (x.to(DEV) for x in weightgen.synthetic_frames(seed, 1, 64, 128))
        out = _both_views_checks(m, fwd, left, right)
    # the chain of the serving loop stays on the device: depth and compacted points of the pixels the check trusts
    depth = out.to_depth(320.0, baseline=0.25, valid_mask=out.occlusion == 0)
    pts, _, off = depth.points_tensor(torch.tensor([[320.0, 0, 64], [0, 320.0, 32], [0, 0, 1]]))
    assert int(off[-1]) == int(depth.valid_mask.sum()) and pts.shape == (64 * 128, 3)


def test_both_views_uses_channel_0_of_cre_stereo(cre_sd):
    from nndepth_amd import weightgen
    from nndepth_amd.cre_stereo import CREStereoBase
    m = CREStereoBase(iters=2)
    m.load_state_dict(cre_sd, strict=True)
    m = m.to(DEV).eval()
    left, right = (x.to(DEV) for x in weightgen.synthetic_frames(7, 1, 128, 192))
    assert m(left, right)[-1]["up_disp"].shape[1] == 2
    _both_views_checks(m, m, left, right)
