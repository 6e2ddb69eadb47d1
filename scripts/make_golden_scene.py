"""Fixture of the scene types (tests/golden/scene.npz, REPORT_scene.txt): inputs and the reference's own outputs.

Runs only where the reference checkout is importable (like scripts/make_golden_midas.py; it installs the stand-ins of
oracle/make_golden.py and changes nothing under oracle/), on the CPU.  Needs matplotlib: the reference's get_view is
matplotlib's Normalize + Colormap; the colormaps are handed to it as objects (matplotlib.colormaps[name]).  Stored:

  signatures            JSON: for Disparity / Depth / Frame / Camera and their public methods, [name, kind, repr(default)] of
                        every parameter of the reference
  table_<name>          the (N,3) uint8 table of RdYlGn, magma, nipy_spectral, red2green:
                        (c(np.arange(c.N))[:, :3] * 255).astype(np.uint8)
  resize_cases          JSON list; case i has r<i>_data, r<i>_mask (occlusion / valid mask), r<i>_out, r<i>_outmask,
                        r<i>_idx (pooled: the reference's max_pool2d indices) and, where a bilinear step is involved,
                        r<i>_f64 (the interpolation formula evaluated in float64 on the same input) with e_ref = max |out - f64|
                        over the finite entries and maxabs = the largest finite |f64|
  inverse_cases         JSON list; i<i>_data, i<i>_out
  frame_*               one Frame.resize carrying a disparity, a depth and a camera
  view_cases            JSON list; v<i>_data, v<i>_mask, v<i>_out (the uint8 picture; a 4-dim map's list stacked to (B,H,W,3))

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_scene.py [path of the reference checkout; default: oracle's]
"""
import inspect
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
CMAPS = ("RdYlGn", "magma", "nipy_spectral", "red2green")


def bilinear64(x: np.ndarray, size, align_corners: bool) -> np.ndarray:
    """F.interpolate(x (B,C,h,w), size, mode="bilinear") with index, weights and sums in float64."""
    x = x.astype(np.float64)

    def axis(n_in, n_out):
        d = np.arange(n_out, dtype=np.float64)
        if n_in == n_out:
            real = d
        elif align_corners:
            real = d * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
        else:
            real = np.maximum((d + 0.5) * (n_in / n_out) - 0.5, 0.0)
        i0 = np.minimum(np.floor(real).astype(np.int64), n_in - 1)
        l1 = np.clip(real - i0, 0.0, 1.0)
        return i0, np.minimum(i0 + 1, n_in - 1), 1.0 - l1, l1

    y0, y1, ly0, ly1 = axis(x.shape[-2], size[0])
    x0, x1, lx0, lx1 = axis(x.shape[-1], size[1])
    with np.errstate(invalid="ignore"):
        top = x[..., y0, :][..., x0] * lx0 + x[..., y0, :][..., x1] * lx1
        bot = x[..., y1, :][..., x0] * lx0 + x[..., y1, :][..., x1] * lx1
        return top * ly0[:, None] + bot * ly1[:, None]


def signature(fn):
    return [[p.name, p.kind.name, repr(p.default) if p.default is not inspect.Parameter.empty else None]
            for p in inspect.signature(fn).parameters.values()]


def main(ref_path):
    import matplotlib
    import matplotlib.colors
    import oracle.make_golden as mg
    if ref_path:
        mg.REF = ref_path
    mg._install_standins()
    from nndepth.scene import Camera, Depth, Disparity, Frame
    from nndepth.scene.depth import maxpool_depth, minpool_depth
    from nndepth.scene.disparity import maxpool_disp, minpool_disp

    out = {}
    rep = ["scene types: the reference's nndepth.scene on the CPU (scripts/make_golden_scene.py), "
           f"torch {torch.__version__.split('+')[0]}, matplotlib {matplotlib.__version__}, numpy {np.__version__}"]
    g = torch.Generator().manual_seed(20)

    out["signatures"] = np.array(json.dumps({
        f"{c.__name__}.{m}": signature(getattr(c, m))
        for c, ms in ((Disparity, ("__init__", "resize", "get_view")), (Depth, ("__init__", "resize", "inverse", "get_view")),
                      (Frame, ("__init__", "resize")), (Camera, ("__init__", "resize"))) for m in ms}))

    cm = {n: matplotlib.colormaps[n] for n in CMAPS[:3]}
    cm["red2green"] = matplotlib.colors.LinearSegmentedColormap.from_list("rg", ["r", "w", "g"], N=256)
    for n, c in cm.items():
        out[f"table_{n}"] = (c(np.arange(c.N))[:, :3] * 255).astype(np.uint8)

    # ------------------------------------------------------------------ resize
    def smooth(B, C, H, W, scale=40.0):
        yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
        base = torch.stack([torch.stack([torch.sin(3 * xx + b + c) * torch.cos(2 * yy - c) for c in range(C)]) for b in range(B)])
        return (-scale * (0.55 + 0.45 * base) + 0.3 * torch.randn(B, C, H, W, generator=g)).float()

    def ints(B, C, H, W):
        return torch.randint(-4, 5, (B, C, H, W), generator=g).float()

    def rnd_mask(shape, dtype, p=0.3):
        return (torch.rand(shape, generator=g) < p).to(dtype)

    def holes(d):
        d = d.abs() + 0.5
        flat = d.view(-1)
        n = flat.numel()
        idx = torch.randperm(n, generator=g)
        flat[idx[: n // 20]] = float("nan")
        flat[idx[n // 20: n // 12]] = float("inf")
        return d

    rcases = []
    rep.append("resize cases (bilinear: e_ref = the reference's fp32 max-abs deviation from the float64 formula; maxabs = largest finite |f64|):")

    def add_resize(cls, data, mask, size, method, align, sign="negative", squeeze=False):
        i = len(rcases)
        if squeeze:
            data, mask = data[0], (mask[0] if mask is not None else None)
        kw = {} if align is None else {"align_corners": align}
        if cls == "disp":
            obj = Disparity(data.clone(), sign, None if mask is None else mask.clone())
            res = obj.resize(size, method, **kw)
            omask = res.occlusion
        else:
            obj = Depth(data.clone(), None if mask is None else mask.clone())
            res = obj.resize(size, method, **kw)
            omask = res.valid_mask
        meta = dict(cls=cls, sign=sign, size=list(size), method=method, align=align, ndim=data.ndim, bilinear=False,
                    mask_dtype=None if mask is None else str(mask.dtype).replace("torch.", ""))
        d4 = data if data.ndim == 4 else data[None]
        H, W = d4.shape[-2:]
        out[f"r{i}_data"] = data.numpy()
        if mask is not None:
            out[f"r{i}_mask"] = mask.numpy()
            out[f"r{i}_outmask"] = omask.numpy()
        out[f"r{i}_out"] = res.data.numpy()
        pre = d4.numpy()
        if method != "interpolate":
            if cls == "disp":
                pooled, idx = (maxpool_disp if method == "maxpool" else minpool_disp)(d4.clone(), (H // (H // size[0]), W // (W // size[1])), sign)
            else:
                pooled, idx = (maxpool_depth if method == "maxpool" else minpool_depth)(d4.clone(), (H // (H // size[0]), W // (W // size[1])))
            out[f"r{i}_idx"] = idx.numpy()
            pre = pooled.numpy()
            assert tuple(pooled.shape[-2:]) == (H // (H // size[0]), W // (W // size[1]))
            meta["bilinear"] = tuple(pooled.shape[-2:]) != tuple(size)
        else:
            meta["bilinear"] = True
        if meta["bilinear"]:
            f64 = bilinear64(pre, size, bool(align))
            if cls == "disp":
                f64 = f64 * size[1] / W
            f64 = f64 if data.ndim == 4 else f64[0]
            got = res.data.numpy().astype(np.float64)
            fin = np.isfinite(f64) & np.isfinite(got)
            with np.errstate(invalid="ignore"):
                meta["e_ref"] = float(np.abs(got - f64)[fin].max())
            meta["maxabs"] = float(np.abs(f64[fin]).max())
            out[f"r{i}_f64"] = f64
        rcases.append(meta)
        rep.append(f"  r{i:<2d} {cls:5s} {method:11s} {tuple(data.shape)!s:16s} -> {tuple(size)!s:9s} align_corners={align!s:5s} "
                   f"mask={meta['mask_dtype']!s:5s}" + (f" e_ref {meta['e_ref']:.3e}  maxabs {meta['maxabs']:.4f}" if meta["bilinear"] else
                                                        "  exact (pool only)"))

    for method in ("interpolate", "maxpool", "minpool"):
        add_resize("disp", smooth(2, 1, 24, 36), None, (12, 18), method, None)
        add_resize("disp", ints(2, 1, 24, 36), rnd_mask((2, 1, 24, 36), torch.bool), (12, 18), method, None)
        add_resize("disp", ints(2, 1, 25, 37), rnd_mask((2, 1, 25, 37), torch.uint8), (8, 12), method, None, sign="positive")
        add_resize("disp", smooth(1, 1, 24, 36), rnd_mask((1, 1, 24, 36), torch.bool), (12, 18), method, None, squeeze=True)
        add_resize("depth", holes(smooth(2, 1, 24, 36)), rnd_mask((2, 1, 24, 36), torch.bool), (12, 18), method, None)
        add_resize("depth", holes(ints(1, 1, 25, 37)), rnd_mask((1, 1, 25, 37), torch.uint8), (8, 12), method, None, squeeze=True)
        add_resize("depth", smooth(2, 2, 24, 36).abs(), None, (12, 18), method, None)
    for align in (False, True):
        add_resize("disp", smooth(2, 1, 24, 36), rnd_mask((2, 1, 24, 36), torch.bool), (17, 29), "interpolate", align)
        add_resize("disp", smooth(2, 1, 24, 36), None, (40, 50), "interpolate", align, sign="positive")
        add_resize("disp", smooth(2, 1, 24, 36), None, (10, 16), "maxpool", align)       # pool 12x18, then bilinear
        add_resize("disp", ints(2, 1, 24, 36), None, (10, 16), "minpool", align)
        add_resize("depth", holes(smooth(2, 1, 24, 36)), rnd_mask((2, 1, 24, 36), torch.bool), (17, 29), "interpolate", align)
        add_resize("depth", holes(smooth(2, 1, 24, 36)), rnd_mask((2, 1, 24, 36), torch.uint8), (10, 16), "maxpool", align)
        add_resize("depth", smooth(1, 1, 24, 36).abs(), None, (10, 16), "minpool", align, squeeze=True)
    add_resize("disp", smooth(1, 1, 68, 120), None, (34, 60), "interpolate", None)
    out["resize_cases"] = np.array(json.dumps(rcases))

    # ------------------------------------------------------------------ inverse
    icases = []
    for i, (cmax, cmin, eps) in enumerate(((None, None, 1e-6), (5.0, None, 1e-6), (None, 0.05, 1e-6), (2.0, 0.1, 1e-3))):
        d = (torch.rand(2, 1, 13, 21, generator=g) * 30).float()
        d.view(-1)[::17] = 0.0
        d.view(-1)[5::41] = float("nan")
        res = Depth(d.clone(), torch.isfinite(d)).inverse(clip_max=cmax, clip_min=cmin, eps=eps)
        out[f"i{i}_data"], out[f"i{i}_out"] = d.numpy(), res.data.numpy()
        icases.append(dict(clip_max=cmax, clip_min=cmin, eps=eps))
    out["inverse_cases"] = np.array(json.dumps(icases))
    rep.append(f"inverse cases: {len(icases)} (exact)")

    # ------------------------------------------------------------------ Frame.resize
    img = (torch.rand(3, 24, 36, generator=g) * 255).float()
    fdisp, focc = smooth(1, 1, 24, 36)[0], rnd_mask((1, 24, 36), torch.bool)
    fdepth, fvalid = holes(smooth(1, 1, 24, 36))[0], rnd_mask((1, 24, 36), torch.bool)
    K = torch.tensor([[0.8, 0.0, 0.5], [0.0, 1.1, 0.45], [0.0, 0.0, 1.0]])
    fr = Frame(img.clone(), Disparity(fdisp.clone(), "negative", focc.clone()), Depth(fdepth.clone(), fvalid.clone()), Camera(K.clone()))
    res = fr.resize((12, 18), disparity_resize_method="maxpool", depth_resize_method="minpool")
    f64 = bilinear64(img[None].numpy(), (12, 18), True)[0]
    e_ref = float(np.abs(res.data.numpy() - f64).max())
    out.update(frame_data=img.numpy(), frame_disp=fdisp.numpy(), frame_occ=focc.numpy(), frame_depth=fdepth.numpy(),
               frame_valid=fvalid.numpy(), frame_K=K.numpy(), frame_out=res.data.numpy(), frame_f64=f64,
               frame_e_ref=np.float64(e_ref), frame_maxabs=np.float64(np.abs(f64).max()),
               frame_out_disp=res.disparity.data.numpy(), frame_out_occ=res.disparity.occlusion.numpy(),
               frame_out_depth=res.depth.data.numpy(), frame_out_valid=res.depth.valid_mask.numpy(), frame_out_K=res.camera.intrinsic.numpy())
    rep.append(f"Frame.resize (3,24,36) -> (12,18), align_corners=True, disparity maxpool, depth minpool: image e_ref {e_ref:.3e}  "
               f"maxabs {np.abs(f64).max():.4f}")

    # ------------------------------------------------------------------ views
    vcases = []

    def add_view(cls, data, mask, cmap, vmin=None, vmax=None, reverse=False):
        i = len(vcases)
        obj = Disparity(data.clone(), "negative", mask) if cls == "disp" else Depth(data.clone(), mask)
        before = obj.data.clone()
        pic = obj.get_view(min=vmin, max=vmax, cmap=cm[cmap] if cmap != "red2green" else "red2green", reverse=reverse)
        assert torch.equal(torch.nan_to_num(obj.data), torch.nan_to_num(before))
        pic = np.stack(pic) if isinstance(pic, list) else pic
        assert pic.dtype == np.uint8
        out[f"v{i}_data"], out[f"v{i}_out"] = data.numpy(), pic
        if mask is not None:
            out[f"v{i}_mask"] = mask.numpy()
        vcases.append(dict(cls=cls, cmap=cmap, min=vmin, max=vmax, reverse=reverse, ndim=data.ndim,
                           mask_dtype=None if mask is None else str(mask.dtype).replace("torch.", "")))

    H, W = 20, 31
    for cmap in CMAPS:
        add_view("disp", smooth(1, 1, H, W)[0], None, cmap)
        add_view("disp", smooth(1, 1, H, W)[0], None, cmap, vmin=5.0, vmax=33.3, reverse=True)
        add_view("disp", smooth(2, 1, H, W) * torch.tensor([1.0, 7.5]).view(2, 1, 1, 1), rnd_mask((2, 1, H, W), torch.bool), cmap)
        d = holes(smooth(1, 1, H, W))[0]
        add_view("depth", d, torch.isfinite(d) & (torch.rand(d.shape, generator=g) < 0.8), cmap)
        d = holes(smooth(2, 1, H, W) * torch.tensor([0.1, 3.0]).view(2, 1, 1, 1))
        add_view("depth", d, (torch.isfinite(d) & (torch.rand(d.shape, generator=g) < 0.8)).to(torch.uint8), cmap, vmin=1.0, reverse=True)
    add_view("disp", torch.full((1, H, W), -3.25), None, "magma")                       # lo == hi
    add_view("disp", torch.full((1, H, W), -3.25), None, "magma", reverse=True)
    add_view("depth", torch.full((2, 1, H, W), 7.0), None, "RdYlGn")
    add_view("disp", smooth(1, 2, H, W)[0], None, "nipy_spectral")                      # 2 channels: range over both, colour of channel 0
    add_view("disp", smooth(1, 2, H, W)[0], rnd_mask((2, H, W), torch.uint8), "RdYlGn", vmax=30.0)
    add_view("depth", smooth(2, 2, H, W).abs() + 1, rnd_mask((2, 2, H, W), torch.bool, 0.7), "magma", vmin=2.0, vmax=40.0)
    add_view("disp", ints(1, 1, H, W)[0] * 1e-3, None, "RdYlGn")                        # small magnitudes, many ties
    add_view("disp", smooth(1, 1, H, W, scale=4e4)[0], None, "nipy_spectral", vmin=100.0)
    add_view("depth", smooth(1, 1, H, W)[0].abs(), None, "magma", vmax=25.0)
    add_view("disp", smooth(1, 1, 136, 240, scale=60.0)[0], None, "RdYlGn")              # the one larger map
    out["view_cases"] = np.array(json.dumps(vcases))
    rep.append(f"view cases: {len(vcases)} (uint8 pictures of the reference; the tests ask for byte equality)")

    path = os.path.join(GOLD, "scene.npz")
    np.savez_compressed(path, **out)
    rep.append(f"scene.npz: {len(out)} arrays, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1 << 20
    with open(os.path.join(GOLD, "REPORT_scene.txt"), "w") as f:
        f.write("\n".join(rep) + "\n")
    print("\n".join(rep))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
