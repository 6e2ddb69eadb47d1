"""CPU: view synthesis and the photometric error (csrc/photometric.hip, nndepth_amd/geometry.py, the scene methods) without a
GPU: the header, the exports, the ctypes table and the Makefile rule agree; the entry points validate their arguments before any
HIP call; Python refuses by name what the kernel does not compute; the vectorised numpy oracle of tests/photometric_cases.py
equals the pixel loops of scripts/make_golden_photometric.py on every input builder and reproduces tests/golden/photometric.npz,
which those loops wrote; and the contract IS the Monodepth formula: the oracle run in float64 against an independent float64
composition of grid_sample, reflection padding and avg_pool2d, and the float32 oracle no further from float64 than twice what
that composition is when it runs in float32."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import photometric_cases as Pc
from cabi_checks import header_exports_ctypes_table_and_makefile_rule_agree, refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nnd_photometric_limit", "nnd_photometric_workspace_bytes", "nnd_synthesize_view", "nnd_photometric_error")
REPORT = os.path.join(ROOT, "tests", "golden", "REPORT_photometric.txt")
CPU_MARK = "-- the contract against the Monodepth composition (tests/test_photometric_cpu.py) --\n"


def _loops():
    spec = importlib.util.spec_from_file_location("make_golden_photometric", os.path.join(ROOT, "scripts", "make_golden_photometric.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and (np.array_equal(Pc.bits(a), Pc.bits(b)) if a.dtype == np.float32 else np.array_equal(a, b))


def _oracle(**kw):
    """The oracle's outputs in the order of the loops' KEYS."""
    syn = {k: v for k, v in kw.items() if k in ("other", "d", "mask", "mask_is_valid", "disp_sign", "target_view", "fill")}
    recon, inn = Pc.synthesize_view(**syn)
    error, valid, l1, dssim, _ = Pc.photometric_error(**kw)
    return recon, inn, error, valid, l1, dssim


def test_header_exports_ctypes_table_and_makefile_rule_agree():
    from nndepth_amd._lib import lib
    header_exports_ctypes_table_and_makefile_rule_agree(NAMES, "photometric")
    assert lib.nnd_version() == 105


def test_limits_and_their_python_mirrors():
    from nndepth_amd import geometry
    from nndepth_amd._lib import NndError, lib
    cmax, th, tw = (lib.nnd_photometric_limit(i) for i in range(3))
    assert cmax >= 4 and th > 0 and tw > 0
    for which in (3, -1, 99):
        assert lib.nnd_photometric_limit(which) < 0
    assert geometry.photometric_max_channels() == cmax and geometry.photometric_tile() == (th, tw)
    tiles = lambda H, W: -(-H // th) * -(-W // tw)  # noqa: E731
    for B, H, W in ((1, 2, 2), (2, 19, 131), (3, th + 3, 2 * tw + 3), (8, 384, 1248)):
        assert lib.nnd_photometric_workspace_bytes(B, H, W) == geometry.photometric_workspace_bytes(B, H, W) == B * tiles(H, W) * 32
    for B, H, W in ((0, 5, 5), (70000, 5, 5), (1, 1, 5), (1, 5, 1), (1, 0, 5), (1, -2, 5), (1, 1 << 16, 1 << 16)):
        assert lib.nnd_photometric_workspace_bytes(B, H, W) < 0
        with pytest.raises(NndError):
            geometry.photometric_workspace_bytes(B, H, W)


def test_entry_points_validate_before_any_device_call():
    from nndepth_amd._lib import lib
    one, two, three, four = C.c_void_p(16), C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20)  # never dereferenced
    inf, nan = float("inf"), float("nan")
    cmax = lib.nnd_photometric_limit(0)
    need = lib.nnd_photometric_workspace_bytes(1, 5, 7)

    def syn(other=one, disp=two, bstride=35, mask=None, pol=1, neg=1, left=1, fill=0.0, recon=three, valid=None, B=1, Cc=3, H=5, W=7):
        return lib.nnd_synthesize_view(other, disp, bstride, mask, pol, neg, left, fill, recon, valid, B, Cc, H, W, None)

    def pho(target=four, other=one, disp=two, bstride=35, mask=None, pol=1, neg=1, left=1, w=0.85, c1=4e-4, c2=3.6e-3, inv_range=0.5,
            fill=0.0, error=three, l1=None, dssim=None, valid=None, stats=None, ws=None, ws_bytes=0, B=1, Cc=3, H=5, W=7):
        return lib.nnd_photometric_error(target, other, disp, bstride, mask, pol, neg, left, w, c1, c2, inv_range, fill, error, l1, dssim,
                                         valid, stats, ws, ws_bytes, B, Cc, H, W, None)

    for call in (syn, pho):
        refused(call(other=None), b"null")
        refused(call(disp=None), b"null")
        for kw in (dict(B=0), dict(B=70000), dict(H=0), dict(H=-1), dict(W=0), dict(W=-3), dict(H=1), dict(W=1, bstride=5),
                   dict(H=1 << 16, W=1 << 16, bstride=1 << 32)):
            refused(call(**kw), b"shape")
        refused(call(B=2, bstride=34), b"stride")
        for Cc in (0, -1, cmax + 1, 100):
            refused(call(Cc=Cc), b"channels")
    refused(syn(recon=None), b"null")
    refused(syn(recon=one), b"must not be an input")
    refused(syn(recon=two), b"must not be an input")
    refused(pho(target=None), b"null")
    refused(pho(error=None), b"null")
    for alias in (one, two, four):
        refused(pho(error=alias), b"must not be an input")
    for w in (-0.01, 1.01, inf, -inf, nan):
        refused(pho(w=w), b"ssim_weight")
    for bad in (0.0, -1.0, inf, -inf, nan):
        refused(pho(c1=bad), b"c1")
        refused(pho(c2=bad), b"c2")
        refused(pho(inv_range=bad), b"inv_range")
    refused(pho(stats=one), b"workspace")
    refused(pho(stats=one, ws=C.c_void_p(4 << 20), ws_bytes=need - 1), b"workspace")
    refused(pho(stats=one, ws=C.c_void_p((4 << 20) + 4), ws_bytes=need), b"aligned")


def test_python_refusals_by_name():
    from nndepth_amd import geometry, scene
    from nndepth_amd._lib import NndError
    d, p = torch.rand(3, 1, 6, 9), torch.rand(3, 3, 6, 9)
    for call in (lambda: geometry.synthesize_view(p, d), lambda: geometry.photometric_error(p, p, d),
                 lambda: scene.Disparity(d).synthesize(scene.Frame(p)), lambda: scene.Disparity(d).photometric_error(p, scene.Frame(p))):
        with pytest.raises(NndError, match="HIP device"):  # CPU tensors: no fallback
            call()
    with pytest.raises(NndError, match="float64"):
        geometry.photometric_error(p, p, d.double())
    with pytest.raises(NndError, match="the target picture is torch.float32; got torch.float16"):
        geometry.photometric_error(p.half(), p, d)
    with pytest.raises(NndError, match="the other picture is torch.float32; got torch.float64"):
        geometry.photometric_error(p, p.double(), d)
    with pytest.raises(NndError, match="the other picture is torch.float32; got ndarray"):
        geometry.synthesize_view(p.numpy(), d)
    with pytest.raises(NndError, match="masks are torch.bool or torch.uint8; got torch.float32"):
        geometry.photometric_error(p, p, d, valid_mask=torch.ones(3, 1, 6, 9))
    with pytest.raises(NndError, match="tensor on the HIP device; got ndarray"):
        geometry.synthesize_view(p, d.numpy())
    for bad in (torch.rand(3, 2, 6, 9), torch.rand(6, 9)):
        with pytest.raises(NndError, match=r"a map is \(B,1,H,W\)"):
            geometry.photometric_error(p, p, bad)
    cmax = geometry.photometric_max_channels()
    for q in (torch.rand(3, 3, 6, 8), torch.rand(2, 3, 6, 9), torch.rand(3, cmax + 1, 6, 9), torch.rand(3, 6, 9), torch.rand(3, 0, 6, 9)):
        with pytest.raises(NndError, match=rf"the other picture is \(B,C,H,W\) = \(3,1..{cmax},6,9\)"):  # a mismatched shape, C above the limit
            geometry.photometric_error(p, q, d)
        with pytest.raises(NndError, match=r"the other picture is \(B,C,H,W\)"):
            geometry.synthesize_view(q, d)
        with pytest.raises(NndError, match=r"the target picture is \(B,C,H,W\)"):
            scene.Disparity(d).photometric_error(scene.Frame(q), p)
    with pytest.raises(NndError, match="the pictures have 3 and 1 channels"):
        geometry.photometric_error(p, p[:, :1], d)
    with pytest.raises(NndError, match="disp_sign must be"):
        geometry.photometric_error(p, p, d, disp_sign="plus")
    with pytest.raises(NndError, match="target_view must be one of"):
        geometry.synthesize_view(p, d, target_view="top")
    for w in (-0.1, 1.5, float("nan")):
        with pytest.raises(NndError, match="ssim_weight must be in"):
            geometry.photometric_error(p, p, d, ssim_weight=w)
    for r in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(NndError, match="data_range must be finite and > 0"):
            geometry.photometric_error(p, p, d, data_range=r)


def test_signatures_of_the_issue():
    import inspect
    from nndepth_amd import geometry, scene
    p = inspect.signature(geometry.synthesize_view).parameters
    assert list(p) == ["other", "disp", "disp_sign", "target_view", "valid_mask", "mask_is_valid", "fill"]
    assert [p[k].default for k in list(p)[2:]] == ["negative", "left", None, True, 0.0]
    p = inspect.signature(geometry.photometric_error).parameters
    assert list(p) == ["target", "other", "disp", "disp_sign", "target_view", "valid_mask", "mask_is_valid", "ssim_weight", "data_range", "fill",
                       "return_parts", "stats", "workspace"]
    assert [p[k].default for k in list(p)[3:]] == ["negative", "left", None, True, 0.85, 2.0, 0.0, False, True, None]
    p = inspect.signature(geometry.photometric_score).parameters
    assert list(p) == ["forward", "left", "right", "threshold", "kw"] and p["threshold"].default == 1.0
    assert list(inspect.signature(scene.Disparity.synthesize).parameters) == ["self", "other", "view"]
    assert list(inspect.signature(scene.Disparity.photometric_error).parameters) == ["self", "frame", "other", "view", "kw"]
    assert "photometric_error" in geometry.__doc__ and "synthesize_view" in geometry.__doc__
    c1, c2, inv = Pc.constants(2.0)
    assert (c1, c2, inv) == (np.float32(0.0004), np.float32(0.0036), np.float32(0.5))


def test_oracle_equals_the_pixel_loops_and_reproduces_the_golden_file(gold):
    G = _loops()
    g = gold("photometric.npz")
    seen = set()
    for name, kw in G.cases().items():
        for key, a, b in zip(G.KEYS, G.photometric_loops(**kw), _oracle(**kw)):
            assert _same(a, b), (name, key)
            if key in G.stored(name):
                assert _same(b, g[f"{name}_{key}"]), (name, key)
                seen.add(f"{name}_{key}")
    assert seen == set(g) - {"numpy"}
    assert G.cases()["scene"]["d"].shape == (2, 1) + Pc.GOLDEN_SHAPE[2:] and G.cases()["scene"]["target"].shape == Pc.GOLDEN_SHAPE


@pytest.mark.parametrize("shape", Pc.SMALL_SHAPES + [(2, 1, 2, 2), (1, 4, 6, 21)], ids=str)
def test_oracle_equals_the_pixel_loops_on_every_builder(shape):
    G = _loops()
    for name, kw in Pc.builders(shape).items():
        for extra in (dict(), dict(ssim_weight=0.0, fill=-7.0), dict(ssim_weight=1.0, data_range=1.0)):
            for key, a, b in zip(G.KEYS, G.photometric_loops(**kw, **extra), _oracle(**kw, **extra)):
                assert _same(a, b), (name, extra, key)


@pytest.mark.parametrize("shape", Pc.SCENE_SHAPES + [Pc.GOLDEN_SHAPE, (2, 3, 2, 2), (1, 1, 3, 5), (2, 3, 5, 7)], ids=str)
def test_the_builders_leave_enough_valid_pixels(shape):
    """A test on inputs that are mostly invalid would compare `fill` with `fill`: outside the builders whose purpose is what is not
    valid, at least a quarter of the pixels carry an error.  Frames narrower than MIN_SHARE_WIDTH are held to that by `small_m`
    alone: there the margin x < m, which the other picture does not cover, takes the frame."""
    for name, kw in Pc.builders(shape).items():
        if name in Pc.INVALIDITY or (shape[3] < Pc.MIN_SHARE_WIDTH and name != "small_m"):
            continue
        for w in (0.85, 0.0):
            ok = Pc.photometric_error(**kw, ssim_weight=w)[4]
            assert ok.mean() >= Pc.MIN_VALID_SHARE, (name, w, float(ok.mean()))


def test_oracle_properties():
    B = Pc.builders((2, 3, 9, 40))
    # synthesize_view alone is the reconstruction inside the fused call; a zero weight gives the L1 term, fill where not valid
    for name, kw in B.items():
        error, valid, l1, dssim, ok = Pc.photometric_error(**kw, ssim_weight=0.0, fill=-7.0)
        assert _same(error, l1) and (dssim == -7.0).all() and ((error == -7.0) | ok).all()
        recon, inn = Pc.synthesize_view(kw["other"], kw["d"], kw.get("mask"), kw.get("mask_is_valid", True), kw.get("disp_sign", "negative"),
                                        kw.get("target_view", "left"))
        inside = inn[:, 0] == int(kw.get("mask_is_valid", True))
        want = np.abs(kw["target"] - recon).astype(np.float32)
        if name != "special_pictures":
            assert np.array_equal(ok[:, 0], inside)
        assert np.allclose(l1[:, 0][ok[:, 0]], (want.mean(1) * 0.5)[ok[:, 0]], rtol=1e-5, atol=1e-7)
    # a non-finite picture value: its pixel is not valid, nor is any pixel whose window holds it or a sample of it
    kw = B["special_pictures"]
    ok = Pc.photometric_error(**kw)[4][:, 0]
    bad_t = ~np.isfinite(kw["target"]).all(1)
    assert bad_t.any() and not ok[bad_t].any()
    p = np.pad(bad_t, ((0, 0), (1, 1), (1, 1)))
    grown = np.any([p[:, dy:dy + 9, dx:dx + 40] for dy in range(3) for dx in range(3)], axis=0)
    assert grown.sum() > bad_t.sum() and not ok[grown].any()
    # a consistent pair scores exactly zero
    for k in (0, 1, 3):
        t, o, d = Pc.consistent((2, 3, 9, 40), k, 5 + k)
        error, _, _, _, ok = Pc.photometric_error(t, o, d)
        assert ok.sum() == 2 * 9 * (40 - k - (1 if k else 0)) and (Pc.bits(error[ok]) == 0).all()
    # xr exactly 0 and exactly W-1 are in; half a pixel further is not
    for name, sign, view in (("edges", "negative", "left"), ("edges_right", "positive", "right")):
        kw = B[name]
        inn = Pc.sample(kw["other"], kw["d"], None, True, sign, view)[1]
        assert inn[:, :5].all() and not inn[:, 5:].any()
        assert Pc.photometric_error(**kw)[4][:, 0, :4].all()  # and their windows carry an error


# ------------------------------------------------------------------------------- the contract is the Monodepth formula
def _monodepth(target, other, d, mask, mask_is_valid, disp_sign, target_view, ssim_weight, data_range, dtype):
    """The photometric error as the Monodepth family composes it from framework operations, in `dtype`: grid_sample along the
    row (bilinear, border padding, align_corners), ReflectionPad2d(1) + AvgPool2d(3, 1) for the five means, the clamped SSIM
    quotient, the channel means and the weighted sum."""
    t, o = torch.from_numpy(target).to(dtype), torch.from_numpy(other).to(dtype)
    dd = torch.from_numpy(d).to(dtype)
    B, Cc, H, W = t.shape
    m = -dd if disp_sign == "negative" else dd
    x = torch.arange(W, dtype=dtype).view(1, 1, 1, W)
    xr = (x - m if target_view == "left" else x + m)[:, 0]
    xr = torch.where(torch.isfinite(xr), xr, torch.zeros_like(xr))
    gx = 2.0 * xr / (W - 1) - 1.0
    gy = (2.0 * torch.arange(H, dtype=dtype) / (H - 1) - 1.0).view(1, H, 1).expand(B, H, W)
    rec = Fn.grid_sample(o, torch.stack([gx, gy], dim=-1), mode="bilinear", padding_mode="border", align_corners=True)
    pool = lambda v: Fn.avg_pool2d(Fn.pad(v, (1, 1, 1, 1), mode="reflect"), 3, 1)  # noqa: E731
    c1, c2, inv_range = (float(v) for v in Pc.constants(data_range))  # the float32 constants of the contract, in either precision
    ssim_weight = float(np.float32(ssim_weight))
    mx, my = pool(t), pool(rec)
    sx, sy, sxy = pool(t * t) - mx * mx, pool(rec * rec) - my * my, pool(t * rec) - mx * my
    n = (2 * mx * my + c1) * (2 * sxy + c2)
    dn = (mx * mx + my * my + c1) * (sx + sy + c2)
    ds = torch.clamp((1 - n / dn) / 2, 0, 1).mean(1, keepdim=True)
    l1 = ((t - rec).abs() * inv_range).mean(1, keepdim=True)
    return (ssim_weight * ds + (1 - ssim_weight) * l1).numpy()


def test_the_contract_is_the_monodepth_formula():
    lines = [CPU_MARK, "max |difference| of the error on the oracle's valid pixels; the float32 oracle's deviation from float64 must stay within\n"
             "2 x the deviation of the same composition of framework operations run in float32 on the same inputs\n"]
    for shape in Pc.SCENE_SHAPES:
        for name in ("scene", "scene_right", "scene_positive_occlusion"):
            kw = Pc.builders(shape)[name]
            args = (kw["target"], kw["other"], kw["d"], kw.get("mask"), kw.get("mask_is_valid", True), kw.get("disp_sign", "negative"),
                    kw.get("target_view", "left"))
            for w in (0.85, 1.0):
                e32, _, _, _, ok = Pc.photometric_error(*args, ssim_weight=w)
                e64, _, _, _, ok64 = Pc.photometric_error(*args, ssim_weight=w, dtype=np.float64)
                assert e64.dtype == np.float64 and np.array_equal(ok, ok64) and ok.mean() >= Pc.MIN_VALID_SHARE
                m64 = _monodepth(*args, w, 2.0, torch.float64)
                m32 = _monodepth(*args, w, 2.0, torch.float32)
                formula = float(np.abs(e64 - m64)[ok].max())
                ours = float(np.abs(e32.astype(np.float64) - e64)[ok].max())
                eager = float(np.abs(m32.astype(np.float64) - m64)[ok].max())
                lines.append(f"{shape} {name} ssim_weight {w}: oracle64 vs composition64 {formula:.1e}; oracle32 vs 64 {ours:.2e}, "
                             f"composition32 vs 64 {eager:.2e}, ratio {ours / eager:.2f}; valid {100 * ok.mean():.0f} %\n")
                print(lines[-1], end="")
                assert formula <= 1e-10, lines[-1]
                assert ours <= 2.0 * eager, lines[-1]
    try:
        old = open(REPORT).read() if os.path.exists(REPORT) else ""
        with open(REPORT, "w") as f:
            f.write(old.split(CPU_MARK)[0] + "".join(lines))
    except OSError:
        pass  # a read-only checkout: the figures were printed
