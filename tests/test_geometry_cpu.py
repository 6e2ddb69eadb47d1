"""CPU: the stereo-geometry unit (csrc/geometry.hip, nndepth_amd/geometry.py, the new scene methods) without a GPU: the header,
the exports and the ctypes table agree on its names; every entry point validates its arguments before any HIP call; Python
refuses by name what the kernels do not compute; and the oracles of tests/geometry_cases.py reproduce tests/golden/geometry.npz
(scripts/make_golden_geometry.py), whose to_disparity part is the reference's own TartanAir expression."""
import ctypes as C

import numpy as np
import pytest
import torch

import geometry_cases as G
from cabi_checks import header_exports_ctypes_table_and_makefile_rule_agree, refused

NAMES = ("nnd_disparity_to_depth", "nnd_depth_to_disparity", "nnd_depth_to_points", "nnd_points_compact_workspace_bytes",
         "nnd_points_compact", "nnd_lr_consistency", "nnd_pair_both_views")


def test_header_exports_and_ctypes_table_agree_on_the_new_names():
    header_exports_ctypes_table_and_makefile_rule_agree(NAMES, "geometry")


def test_entry_points_validate_before_any_device_call():
    from nndepth_amd._lib import lib
    one = C.c_void_p(16)  # never dereferenced: every call below is refused first

    refused(lib.nnd_disparity_to_depth(None, 35, None, one, 0, 0.25, 1, 0.0, 0, 0.0, None, None, 1, 5, 7, None), b"null")
    refused(lib.nnd_disparity_to_depth(one, 35, None, None, 0, 0.25, 1, 0.0, 0, 0.0, one, one, 1, 5, 7, None), b"camera")
    refused(lib.nnd_disparity_to_depth(one, 35, None, one, 3, 0.25, 1, 0.0, 0, 0.0, one, one, 1, 5, 7, None), b"cam_stride")
    refused(lib.nnd_disparity_to_depth(one, 35, None, one, 0, 0.25, 1, 0.0, 0, 0.0, one, one, 0, 5, 7, None), b"shape")
    refused(lib.nnd_disparity_to_depth(one, 34, None, one, 0, 0.25, 1, 0.0, 0, 0.0, one, one, 2, 5, 7, None), b"stride")
    refused(lib.nnd_disparity_to_depth(one, 35, None, one, 0, float("nan"), 1, 0.0, 0, 0.0, one, one, 1, 5, 7, None), b"NaN")
    refused(lib.nnd_depth_to_disparity(None, 35, one, 0, 0.25, 1, 1e-8, None, 1, 5, 7, None), b"null")
    refused(lib.nnd_depth_to_disparity(one, 35, one, 0, 0.25, 1, 1e-8, one, 1, 5, 0, None), b"shape")
    refused(lib.nnd_depth_to_disparity(one, 35, one, 0, 0.25, 1, 1e-8, one, 70000, 5, 7, None), b"shape")
    refused(lib.nnd_depth_to_points(one, 35, None, one, 0, None, 1, 5, 7, None), b"null")
    refused(lib.nnd_depth_to_points(one, 35, None, None, 0, one, 1, 5, 7, None), b"camera")
    refused(lib.nnd_depth_to_points(one, 35, None, one, 0, one, 1, -5, 7, None), b"shape")
    assert lib.nnd_points_compact_workspace_bytes(0, 5, 7) < 0 and lib.nnd_points_compact_workspace_bytes(2, 5, 0) < 0
    assert lib.nnd_points_compact_workspace_bytes(2, 40, 70) == 2 * 11 * 12  # 11 workgroups of 256 pixels per sample
    big = C.c_void_p(1 << 20)
    refused(lib.nnd_points_compact(one, 35, None, one, 0, None, 0, one, None, None, big, 1 << 20, 1, 5, 7, None), b"null")
    refused(lib.nnd_points_compact(one, 35, None, one, 0, one, 3, one, None, one, big, 1 << 20, 1, 5, 7, None), b"together")
    refused(lib.nnd_points_compact(one, 35, None, one, 0, one, 0, one, one, one, big, 1 << 20, 1, 5, 7, None), b"channels")
    refused(lib.nnd_points_compact(one, 35, None, one, 0, None, 0, one, None, one, big, 8, 1, 5, 7, None), b"workspace")
    refused(lib.nnd_points_compact(one, 35, None, one, 0, None, 0, one, None, one, C.c_void_p(20), 1 << 20, 1, 5, 7, None), b"aligned")
    refused(lib.nnd_lr_consistency(one, 35, None, 35, 1, 1, 0, 1.0, one, None, 1, 5, 7, None), b"null")
    refused(lib.nnd_lr_consistency(one, 35, one, 10, 1, 1, 0, 1.0, one, None, 2, 5, 7, None), b"stride")
    refused(lib.nnd_lr_consistency(one, 35, one, 35, 1, 1, 0, float("nan"), one, None, 1, 5, 7, None), b"threshold")
    refused(lib.nnd_pair_both_views(one, None, one, one, 1, 3, 8, 8, None), b"null")
    refused(lib.nnd_pair_both_views(one, one, one, one, 1, 0, 8, 8, None), b"shape")


def test_python_refusals_by_name():
    from nndepth_amd import geometry, scene
    from nndepth_amd._lib import NndError
    x = torch.rand(3, 1, 6, 9)
    cam = scene.Camera(torch.tensor([[320.0, 0, 4.5], [0, 320.0, 3.0], [0, 0, 1]]))
    disp, depth = scene.Disparity(x, baseline=0.25), scene.Depth(x)
    # CPU tensors: no fallback
    for call in (lambda: disp.to_depth(cam), lambda: disp.to_depth(320.0), lambda: depth.to_disparity(cam, 0.25),
                 lambda: depth.to_points_map(cam), lambda: depth.points_tensor(cam), lambda: depth.to_points(cam),
                 lambda: geometry.lr_consistency(x, x), lambda: geometry.both_views(lambda a, b: None, x, x),
                 lambda: geometry.occlusion(lambda a, b: None, x, x), lambda: geometry.depth_to_points(x, cam),
                 lambda: geometry.points_compact(x, cam), lambda: geometry.disparity_to_depth(x, 320.0, 0.25)):
        with pytest.raises(NndError, match="HIP device"):
            call()
    # dtypes
    with pytest.raises(NndError, match="float64"):
        scene.Disparity(x.double(), baseline=0.25).to_depth(cam)
    with pytest.raises(NndError, match="float16"):
        scene.Depth(x.half()).points_tensor(cam)
    with pytest.raises(NndError, match="float16"):
        geometry.lr_consistency(x.half(), x.half())
    with pytest.raises(NndError, match="int32"):
        geometry.both_views(lambda a, b: None, x.int(), x.int())
    with pytest.raises(NndError, match="masks are torch.bool or torch.uint8; got torch.float32"):
        disp.to_depth(cam, valid_mask=torch.ones(3, 1, 6, 9))
    with pytest.raises(NndError, match="masks are torch.bool or torch.uint8; got torch.int64"):
        scene.Depth(x, valid_mask=torch.ones(3, 1, 6, 9, dtype=torch.int64)).to_points_map(cam)
    # values
    with pytest.raises(NndError, match="no baseline"):
        scene.Disparity(x).to_depth(cam)
    with pytest.raises(NndError, match="no baseline"):
        geometry.disparity_to_depth(x, 320.0, None)
    with pytest.raises(NndError, match=r"\(3,3\) or \(B,3,3\) with B = 3; got \(2, 3, 3\)"):
        geometry.camera_params(scene.Camera(torch.eye(3).repeat(2, 1, 1)), 3, torch.device("cpu"))
    with pytest.raises(NndError, match="got \\(3, 4\\)"):
        geometry.camera_params(torch.zeros(3, 4), 3, torch.device("cpu"))
    with pytest.raises(NndError, match="no intrinsic"):
        geometry.camera_params(scene.Camera(), 3, torch.device("cpu"))
    with pytest.raises(NndError, match="fx alone"):
        geometry.camera_params(320.0, 3, torch.device("cpu"), fx_only=False)
    with pytest.raises(NndError, match="'sideways'"):
        geometry.lr_consistency(x, x, left_sign="sideways")
    with pytest.raises(NndError, match="'sideways'"):
        geometry.depth_to_disparity(x, 320.0, 0.25, disp_sign="sideways")
    # the host side of camera_params: {fx, fy, cx, cy} per camera, one camera -> stride 0, kept on the Camera
    K = torch.tensor([[[300.0, 0, 4.5], [0, 310.0, 3.0], [0, 0, 1]], [[301.0, 0, 4.25], [0, 311.0, 3.5], [0, 0, 1]],
                      [[302.0, 0, 4.0], [0, 312.0, 2.5], [0, 0, 1]]])
    par, stride = geometry.camera_params(scene.Camera(K), 3, torch.device("cpu"))
    assert stride == 4 and torch.equal(par, torch.tensor([[300.0, 310.0, 4.5, 3.0], [301.0, 311.0, 4.25, 3.5], [302.0, 312.0, 4.0, 2.5]]))
    assert np.array_equal(par.numpy().astype(np.float64), G.cam_of(K.numpy(), 3))
    par1, stride1 = geometry.camera_params(cam, 3, torch.device("cpu"))
    assert stride1 == 0 and par1.tolist() == [[320.0, 320.0, 4.5, 3.0]]
    assert geometry.camera_params(cam, 3, torch.device("cpu"))[0] is par1  # the copy is made once
    cam.intrinsic[0, 0] = 321.0  # ... until the intrinsic is edited
    assert geometry.camera_params(cam, 3, torch.device("cpu"))[0].tolist() == [[321.0, 320.0, 4.5, 3.0]]
    fx_par, fx_stride = geometry.camera_params(320.0, 3, torch.device("cpu"))
    assert fx_stride == 0 and fx_par[0, 0].item() == 320.0


def test_new_scene_methods_leave_the_reference_signatures_alone():
    import inspect
    from nndepth_amd import scene
    p = inspect.signature(scene.Disparity.to_depth).parameters
    assert list(p) == ["self", "camera_or_fx", "baseline", "min_disp", "max_depth", "valid_mask"]
    assert (p["baseline"].default, p["min_disp"].default, p["max_depth"].default, p["valid_mask"].default) == (None, 0.0, None, None)
    p = inspect.signature(scene.Depth.to_disparity).parameters
    assert list(p) == ["self", "camera_or_fx", "baseline", "disp_sign", "eps"]
    assert (p["disp_sign"].default, p["eps"].default) == ("negative", 1e-8)
    for name, args in (("to_points_map", ["self", "camera"]), ("points_tensor", ["self", "camera", "features"]),
                       ("to_points", ["self", "camera", "features"])):
        assert list(inspect.signature(getattr(scene.Depth, name)).parameters) == args


def test_oracles_reproduce_the_golden_file(gold):
    g = gold("geometry.npz")
    fx, baseline = float(g["ta_fx"]), float(g["ta_baseline"])
    assert (fx, baseline) == (G.TARTANAIR_FX, G.TARTANAIR_BASELINE) and g["ta_depth"].shape == (1, 48, 64)
    # the reference's own expression, bit for bit
    disp = G.to_disparity(g["ta_depth"][None], [fx], baseline)
    assert disp.dtype == np.float32 and np.array_equal(disp[0].view(np.uint32), g["ta_disp"].view(np.uint32))
    assert np.array_equal(G.to_disparity(g["ta_depth"][None], [fx], baseline, "positive"), -disp)
    depth, valid = G.to_depth(g["ta_disp"][None], [fx], baseline)
    assert np.array_equal(depth.view(np.uint32), g["ta_back_depth"].view(np.uint32)) and np.array_equal(valid, g["ta_back_valid"])
    assert valid.all() and np.abs(depth[0].astype(np.float64) - g["ta_depth"]).max() <= 2.0 ** -22  # close, not exact
    pts = G.points_map(depth, G.cam_of(g["ta_K"], 1), valid)
    assert np.array_equal(pts.view(np.uint32), g["ta_points"].view(np.uint32))
    rows, _, offsets = G.compact(depth, G.cam_of(g["ta_K"], 1), valid)
    assert offsets.tolist() == [0, 48 * 64] and np.array_equal(rows, pts[0].reshape(3, -1).T)
    cases = G.lr_cases()
    assert set(cases) == {"12x40", "7x33", "3x5", "2x9x70"}
    for name, (mL, mR) in cases.items():
        assert np.array_equal(mL * 8, np.round(mL * 8), equal_nan=True) and np.array_equal(mR * 8, np.round(mR * 8), equal_nan=True)
        for sl, sr, flip in (("negative", "negative", False), ("positive", "negative", True), ("negative", "positive", False)):
            dr = G.stored(mR, sr)
            dr = np.ascontiguousarray(dr[..., ::-1]) if flip else dr
            occ64, err64 = G.lr(G.stored(mL, sl), dr, G.LR_THRESHOLD, sl, sr, flip, dtype=np.float64)
            occ32, err32 = G.lr(G.stored(mL, sl), dr, G.LR_THRESHOLD, sl, sr, flip, dtype=np.float32)
            assert np.array_equal(occ64, g[f"lr_{name}_occ"]) and np.array_equal(occ32, occ64)
            assert np.array_equal(err64.astype(np.float32), g[f"lr_{name}_err"], equal_nan=True)
            assert np.array_equal(err32, g[f"lr_{name}_err"], equal_nan=True)
        assert 0.05 < g[f"lr_{name}_occ"].mean() < 0.5


def test_to_depth_oracle_on_the_special_values():
    d, idx = G.special_disparity(2, 5, 7, 1)
    z, ok = G.to_depth(d, [320.0, 300.5], 0.25, max_depth=20.0)
    flat_z, flat_ok = z[0, 0].reshape(-1), ok[0, 0].reshape(-1)
    # 0, -0, +-subnormal, wrong sign x2, +-inf, NaN, 4, just below 4, just above 4, 0.5, just below 0.5
    assert flat_ok[idx].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0]  # z of 0.5 (160) and of the subnormal exceed max_depth
    assert flat_z[idx[9]] == 20.0 and flat_z[idx[10]] == 0.0  # z == max_depth is valid; one ulp less disparity is not
    z2, ok2 = G.to_depth(d, [320.0, 300.5], 0.25, min_disp=0.5)
    assert ok2[0, 0].reshape(-1)[idx].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0]  # m > min_disp is strict
    z3, ok3 = G.to_depth(d, [320.0, 300.5], 0.25)
    assert ok3[0, 0].reshape(-1)[idx[2]] == 1 and np.isinf(z3[0, 0].reshape(-1)[idx[2]])  # 80 / 1e-41 overflows fp32: +inf, valid
