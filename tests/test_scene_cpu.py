"""CPU: the scene types (nndepth_amd/scene.py, csrc/scene.hip) mirror the reference's signatures, refuse by name what they do
not compute, and the closed form of the coloured view that the HIP kernel implements reproduces the reference's pictures of
tests/golden/scene.npz (scripts/make_golden_scene.py) byte for byte when evaluated in numpy float64."""
import inspect
import json

import numpy as np
import pytest
import torch

CMAPS = ("RdYlGn", "magma", "nipy_spectral", "red2green")


def view_closed_form(data: np.ndarray, mask, kind: str, table: np.ndarray, vmin=None, vmax=None, reverse=False) -> np.ndarray:
    """The closed form of Disparity.get_view / Depth.get_view for one batch element (C,H,W) -> (H,W,3) uint8 (float64)."""
    v = data.astype(np.float32)
    if kind == "disp":
        v = np.abs(v)
        if mask is not None:
            v = np.where(mask.astype(np.float32) == 1, np.float32(0), v)
    elif mask is not None:
        ok = mask.astype(np.float32) == 1
        v = np.where(ok, v, v[ok].min())
    lo = float(v.min()) if vmin is None else float(vmin)
    hi = float(v.max()) if vmax is None else float(vmax)
    N = table.shape[0]
    x = np.clip(v.astype(np.float64), lo, hi)
    n = np.zeros_like(x) if lo == hi else (x - lo) / (hi - lo)
    if reverse:
        n = 1.0 - n
    t = n * N
    idx = np.where(t == N, N - 1, t.astype(np.int64))
    return table[np.clip(idx, 0, N - 1)[0]]


def views_closed_form(data, mask, kind, table, vmin=None, vmax=None, reverse=False):
    """3-dim map -> (H,W,3); 4-dim map -> (B,H,W,3), each batch element with its own range."""
    if data.ndim == 3:
        return view_closed_form(data, mask, kind, table, vmin, vmax, reverse)
    return np.stack([view_closed_form(data[b], None if mask is None else mask[b], kind, table, vmin, vmax, reverse)
                     for b in range(data.shape[0])])


def _signature(fn):
    return [[p.name, p.kind.name, repr(p.default) if p.default is not inspect.Parameter.empty else None]
            for p in inspect.signature(fn).parameters.values()]


def test_signatures_and_defaults_equal_the_reference(gold):
    from nndepth_amd import scene
    ref = json.loads(str(gold("scene.npz")["signatures"]))
    assert len(ref) == 11
    for name, sig in ref.items():
        cls, meth = name.split(".")
        assert _signature(getattr(getattr(scene, cls), meth)) == sig, name
    for cls in ("Disparity", "Depth"):  # the device-side addition takes get_view's arguments
        assert _signature(getattr(scene, cls).get_view_tensor) == ref[f"{cls}.get_view"]
    d = scene.Disparity(torch.zeros(1, 2, 2))
    assert (d.disp_sign, d.occlusion, d.baseline) == ("negative", None, None)
    z = scene.Depth(torch.zeros(1, 2, 2))
    assert (z.valid_mask, z.is_inverse) == (None, False)
    f = scene.Frame(torch.zeros(3, 2, 2))
    assert (f.disparity, f.depth, f.camera, f.camera_id, f.pose) == (None,) * 5


def test_closed_form_reproduces_the_reference_views_byte_for_byte(gold):
    """Pins the closed form itself: matplotlib's Normalize(clip=True) + Colormap + (rgb * 255).astype(uint8), as the reference
    ran them, equal the float64 restatement above on every view of the fixture — zero differing bytes."""
    g = gold("scene.npz")
    cases = json.loads(str(g["view_cases"]))
    assert len(cases) >= 30 and {c["cmap"] for c in cases} == set(CMAPS)
    for i, c in enumerate(cases):
        got = views_closed_form(g[f"v{i}_data"], g.get(f"v{i}_mask"), c["cls"], g[f"table_{c['cmap']}"], c["min"], c["max"], c["reverse"])
        ref = g[f"v{i}_out"]
        assert got.shape == ref.shape and got.dtype == np.uint8
        assert np.array_equal(got, ref), f"view case {i} {c}: {(got != ref).any(-1).sum()} pixels differ"


def test_table_builder_equals_the_committed_tables(gold):
    pytest.importorskip("matplotlib")
    import matplotlib
    from nndepth_amd import scene
    g = gold("scene.npz")
    for name in CMAPS:
        tab = scene.colormap_table(name)
        assert tab.dtype == torch.uint8 and tab.device.type == "cpu"
        assert np.array_equal(tab.numpy(), g[f"table_{name}"]), name
    assert np.array_equal(scene.colormap_table(matplotlib.colormaps["magma"]).numpy(), g["table_magma"])
    with pytest.raises(ValueError, match="not a colormap"):
        scene.colormap_table("no_such_colormap")


def test_tables_given_as_arrays(gold):
    from nndepth_amd import scene
    from nndepth_amd._lib import NndError
    tab = gold("scene.npz")["table_magma"]
    assert np.array_equal(scene.colormap_table(tab).numpy(), tab)
    rgba = np.concatenate([tab, np.full((len(tab), 1), 255, np.uint8)], 1)
    assert np.array_equal(scene.colormap_table(torch.from_numpy(rgba)).numpy(), tab)
    f = np.linspace(0, 1, 12).reshape(4, 3)
    assert np.array_equal(scene.colormap_table(f).numpy(), (f * 255).astype(np.uint8))
    for n in (1, 4097):
        with pytest.raises(NndError, match=rf"N = {n}"):
            scene.colormap_table(np.zeros((n, 3), np.uint8))
    with pytest.raises(NndError, match=r"\(N,3\) or \(N,4\)"):
        scene.colormap_table(np.zeros((8, 2), np.uint8))
    with pytest.raises(NndError, match="int32"):
        scene.colormap_table(np.zeros((8, 3), np.int32))
    with pytest.raises(NndError, match=r"\[0,1\]"):
        scene.colormap_table(np.full((8, 3), 1.5))
    with pytest.raises(NndError, match="a name, a matplotlib Colormap"):
        scene.colormap_table(3)


def test_a_name_without_matplotlib_asks_for_a_table(monkeypatch):
    import sys
    from nndepth_amd import scene
    from nndepth_amd._lib import NndError
    monkeypatch.setitem(sys.modules, "matplotlib", None)  # import matplotlib -> ImportError
    monkeypatch.setattr(scene, "_TABLES_HOST", {})
    with pytest.raises(NndError, match="pass an .* table"):
        scene.colormap_table("magma")


def test_python_refusals_by_name(gold):
    from nndepth_amd import scene
    from nndepth_amd._lib import NndError
    tab = gold("scene.npz")["table_magma"]
    x = torch.rand(1, 8, 12)
    # CPU tensors: no fallback
    for call in (lambda: scene.Disparity(x).get_view(cmap=tab), lambda: scene.Disparity(x).get_view_tensor(cmap=tab),
                 lambda: scene.Depth(x).get_view(cmap=tab), lambda: scene.Disparity(x).resize((4, 6)),
                 lambda: scene.Disparity(x).resize((4, 6), "maxpool"), lambda: scene.Depth(x).resize((4, 6), "minpool"),
                 lambda: scene.Depth(x).resize((4, 6)), lambda: scene.Depth(x).inverse(), lambda: scene.Frame(x).resize((4, 6))):
        with pytest.raises(NndError, match="HIP device"):
            call()
    # dtypes
    with pytest.raises(NndError, match="float64"):
        scene.Disparity(x.double()).get_view(cmap=tab)
    with pytest.raises(NndError, match="float16"):
        scene.Depth(x.half()).resize((4, 6))
    with pytest.raises(NndError, match="float32"):
        scene.Disparity(x, occlusion=torch.zeros(1, 8, 12)).get_view(cmap=tab)  # a float mask
    with pytest.raises(NndError, match="int64"):
        scene.Depth(x, valid_mask=torch.ones(1, 8, 12, dtype=torch.int64)).resize((4, 6))
    with pytest.raises(NndError, match="uint8"):
        scene.Frame(torch.zeros(3, 8, 12, dtype=torch.uint8)).resize((4, 6))
    # values
    with pytest.raises(ValueError, match="less than or equal"):
        scene.Disparity(x).get_view(min=3.0, max=1.0, cmap=tab)
    with pytest.raises(NndError, match="less than or equal"):
        scene.Depth(x).get_view_tensor(min=3.0, max=1.0, cmap=tab)
    with pytest.raises(NndError, match="N = 1 "):
        scene.Disparity(x).get_view(cmap=tab[:1])
    with pytest.raises(NndError, match="3 or 4 dimensions"):
        scene.Disparity(x[0]).get_view(cmap=tab)
    occ = torch.zeros(1, 8, 12, dtype=torch.bool)
    with pytest.raises(NndError, match="bilinear step after the pool"):
        scene.Disparity(x, occlusion=occ).resize((3, 5), "maxpool")  # window 2x2 -> 4x6, then bilinear
    with pytest.raises(NndError, match="only shrink"):
        scene.Disparity(x).resize((16, 24), "maxpool")
    with pytest.raises(NndError, match="antialias"):
        scene.Depth(x).resize((4, 6), antialias=True)
    with pytest.raises(AssertionError, match="method must be in"):
        scene.Disparity(x).resize((4, 6), "nearest")


def test_cabi_argument_checks_run_before_any_device_call():
    import ctypes as C
    from nndepth_amd._lib import lib
    one = C.c_void_p(16)  # never dereferenced: every call below is refused first
    assert lib.nnd_view_range_workspace_bytes(0) < 0 and lib.nnd_view_range_workspace_bytes(3) == 3 * 128 * 2 * 4
    assert lib.nnd_view_range(None, None, 0, 1, 1, 4, 4, None, None, None) == -1 and b"null" in lib.nnd_last_error()
    assert lib.nnd_view_range(one, None, 2, 1, 1, 4, 4, one, one, None) == -1 and b"kind" in lib.nnd_last_error()
    assert lib.nnd_view_range(one, None, 0, 1, 1, 0, 4, one, one, None) == -1 and b"shape" in lib.nnd_last_error()
    assert lib.nnd_colorize(None, None, 0, 1, 1, 4, 4, None, 0, 0.0, 0, 0.0, 0, None, 256, None, None) == -1
    for n in (1, 4097):
        assert lib.nnd_colorize(one, None, 0, 1, 1, 4, 4, one, 0, 0.0, 0, 0.0, 0, one, n, one, None) == -1
        assert b"colours" in lib.nnd_last_error()
    assert lib.nnd_colorize(one, None, 0, 1, 1, 4, 4, one, 1, 3.0, 1, 1.0, 0, one, 256, one, None) == -1
    assert b"less than or equal" in lib.nnd_last_error()
    assert lib.nnd_colorize(one, None, 0, 1, 1, 4, 4, None, 1, 0.0, 0, 0.0, 0, one, 256, one, None) == -1  # a bound is missing
    assert b"range" in lib.nnd_last_error()
    assert lib.nnd_colorize(one, one, 1, 1, 1, 4, 4, None, 1, 0.0, 1, 1.0, 0, one, 256, one, None) == -1  # depth mask: fill value
    assert lib.nnd_pool_abs(None, None, None, None, None, None, 1, 1, 4, 4, 2, 2, 0, 0, 0, 1.0, 1.0, None) == -1
    assert lib.nnd_pool_abs(one, one, None, None, None, None, 1, 1, 4, 4, 0, 2, 0, 0, 0, 1.0, 1.0, None) == -1
    assert b"window" in lib.nnd_last_error()
    assert lib.nnd_pool_abs(one, one, None, None, None, None, 1, 1, 4, 4, 5, 2, 0, 0, 0, 1.0, 1.0, None) == -1
    assert lib.nnd_pool_abs(one, one, None, one, None, None, 1, 1, 4, 4, 2, 2, 0, 0, 0, 1.0, 1.0, None) == -1
    assert b"together" in lib.nnd_last_error()
    assert lib.nnd_pool_abs(one, one, None, None, None, None, 1, 1, 4, 4, 2, 2, 0, 0, 1, 2.0, 0.0, None) == -1
    assert lib.nnd_resize_bilinear(None, 0, None, None, 0, None, 1, 4, 4, 8, 8, 0, 0, 1.0, 1.0, None) == -1
    assert lib.nnd_resize_bilinear(one, 0, None, None, 0, None, 1, 4, 4, 8, 8, 0, 0, 1.0, 1.0, None) == -1  # no output at all
    assert lib.nnd_resize_bilinear(one, 0, one, None, 0, None, 1, 4, 0, 8, 8, 0, 0, 1.0, 1.0, None) == -1
    assert b"shape" in lib.nnd_last_error()
    assert lib.nnd_resize_bilinear(one, 1, None, one, 3, None, 1, 4, 4, 8, 8, 0, 0, 1.0, 1.0, None) == -1
    assert b"u8_mode" in lib.nnd_last_error()
    assert lib.nnd_resize_bilinear(one, 0, one, None, 0, None, 70000, 4, 4, 8, 8, 0, 0, 1.0, 1.0, None) == -1
    assert lib.nnd_depth_inverse(None, None, 4, 1e-6, 0, 0.0, 0, 0.0, None) == -1
    assert lib.nnd_depth_inverse(one, one, 0, 1e-6, 0, 0.0, 0, 0.0, None) == -1


def test_camera_resize_equals_the_fixture(gold):
    from nndepth_amd.scene import Camera
    g = gold("scene.npz")
    K = torch.from_numpy(g["frame_K"])
    cam = Camera(K.clone(), extrinsic=torch.eye(4))
    new = cam.resize((12, 18))
    assert torch.equal(new.intrinsic, torch.from_numpy(g["frame_out_K"])) and torch.equal(cam.intrinsic, K)
    assert new.extrinsic is cam.extrinsic
    batched = Camera(K.repeat(2, 1, 1)).resize((12, 18))
    assert torch.equal(batched.intrinsic, torch.from_numpy(g["frame_out_K"]).repeat(2, 1, 1))
    empty = Camera()
    assert empty.resize((12, 18)) is empty
