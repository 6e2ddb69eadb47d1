"""GPU: the scene types through the HIP path (csrc/scene.hip) against the reference's own outputs of tests/golden/scene.npz
(scripts/make_golden_scene.py).  Views: byte equality.  Pooled values, indices, gathered occlusion, valid masks, interpolated
occlusion, inverse: torch.equal.  Bilinear maps: max-abs deviation from the float64 formula at most twice the reference's own
(e_ref), with a floor of two fp32 ulp of the map's largest magnitude."""
import json

import numpy as np
import pytest
import torch

from test_scene_cpu import views_closed_form

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bilinear_bound(e_ref: float, maxabs: float) -> float:
    return max(2.0 * e_ref, 2.0 * float(np.spacing(np.float32(maxabs))))


def _check_bilinear(got: torch.Tensor, f64: np.ndarray, e_ref: float, maxabs: float, what: str):
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == f64.shape, what
    fin = np.isfinite(f64)
    assert np.array_equal(np.isnan(got), np.isnan(f64)) and np.array_equal(np.isinf(got), np.isinf(f64)), what
    err = float(np.abs(got[fin] - f64[fin]).max())
    bound = _bilinear_bound(e_ref, maxabs)
    print(f"[scene] {what}: HIP vs float64 {err:.3e}, reference vs float64 {e_ref:.3e}, bound {bound:.3e}")
    assert err <= bound, what


def test_views_equal_the_reference_byte_for_byte(gold):
    from nndepth_amd.scene import Depth, Disparity
    g = gold("scene.npz")
    cases = json.loads(str(g["view_cases"]))
    for i, c in enumerate(cases):
        data = _t(g[f"v{i}_data"])
        mask = _t(g[f"v{i}_mask"]) if f"v{i}_mask" in g else None
        obj = Disparity(data, "negative", mask) if c["cls"] == "disp" else Depth(data, mask)
        before = data.clone()
        table = _t(g[f"table_{c['cmap']}"])
        pic = obj.get_view(min=c["min"], max=c["max"], cmap=table, reverse=c["reverse"])
        ref = g[f"v{i}_out"]
        if c["ndim"] == 3:
            assert isinstance(pic, np.ndarray) and pic.dtype == np.uint8 and pic.shape == ref.shape
        else:
            assert isinstance(pic, list) and len(pic) == ref.shape[0] and all(p.dtype == np.uint8 for p in pic)
            pic = np.stack(pic)
        assert np.array_equal(pic, ref), f"view case {i} {c}: {(pic != ref).any(-1).sum()} pixels differ"
        assert torch.equal(torch.nan_to_num(obj.data), torch.nan_to_num(before))  # get_view does not modify the map
        dev = obj.get_view_tensor(min=c["min"], max=c["max"], cmap=table, reverse=c["reverse"])
        assert dev.is_cuda and dev.dtype == torch.uint8 and np.array_equal(dev.cpu().numpy().reshape(ref.shape), ref)
    # a table handed over as a host array, and as float RGBA
    c0 = cases[0]
    data = _t(g["v0_data"])
    from nndepth_amd.scene import Disparity as D
    tab = g[f"table_{c0['cmap']}"]
    assert np.array_equal(D(data).get_view(cmap=tab), g["v0_out"])


def test_resize_cases_equal_the_reference(gold):
    from nndepth_amd import ops
    from nndepth_amd.scene import Depth, Disparity
    g = gold("scene.npz")
    cases = json.loads(str(g["resize_cases"]))
    assert len(cases) >= 36
    for i, c in enumerate(cases):
        what = f"resize case {i} {c['cls']} {c['method']} -> {c['size']} align_corners={c['align']}"
        data = _t(g[f"r{i}_data"])
        mask = _t(g[f"r{i}_mask"]) if f"r{i}_mask" in g else None
        kw = {} if c["align"] is None else {"align_corners": c["align"]}
        if c["cls"] == "disp":
            res = Disparity(data, c["sign"], mask).resize(tuple(c["size"]), c["method"], **kw)
            omask = res.occlusion
            assert res.disp_sign == c["sign"]
        else:
            res = Depth(data, mask).resize(tuple(c["size"]), c["method"], **kw)
            omask = res.valid_mask
        ref = torch.from_numpy(g[f"r{i}_out"])
        assert res.data.is_cuda and res.data.ndim == c["ndim"] and tuple(res.data.shape) == tuple(ref.shape), what
        if c["bilinear"]:
            _check_bilinear(res.data, g[f"r{i}_f64"], c["e_ref"], c["maxabs"], what)
        else:
            assert torch.equal(torch.nan_to_num(res.data.cpu(), nan=-7.0), torch.nan_to_num(ref, nan=-7.0)), what
            assert torch.equal(torch.isnan(res.data.cpu()), torch.isnan(ref)), what
        if mask is None:
            assert omask is None
        else:
            rmask = torch.from_numpy(g[f"r{i}_outmask"])
            assert omask.dtype == rmask.dtype == mask.dtype and torch.equal(omask.cpu(), rmask), what
        if c["method"] != "interpolate":  # the pool's own indices (and values before any bilinear step)
            d4 = data if data.ndim == 4 else data[None]
            H, W = d4.shape[-2:]
            kernel = (H // c["size"][0], W // c["size"][1])
            _, idx, _, _ = ops.pool_abs(d4, kernel, c["method"] == "minpool", c["cls"] == "disp" and c["sign"] == "negative", indices=True)
            assert idx.dtype == torch.int64 and torch.equal(idx.cpu(), torch.from_numpy(g[f"r{i}_idx"])), what


def test_pooled_occlusion_is_gathered_from_plane_0(gold):
    """the reference gathers occlusion.flatten()[indices.flatten()] with plane-local indices."""
    from nndepth_amd.scene import Disparity
    g = gold("scene.npz")
    cases = json.loads(str(g["resize_cases"]))
    i = next(k for k, c in enumerate(cases) if c["cls"] == "disp" and c["method"] == "maxpool" and c["mask_dtype"] == "bool" and c["ndim"] == 4)
    data, occ = g[f"r{i}_data"], g[f"r{i}_mask"]
    res = Disparity(_t(data), "negative", _t(occ)).resize(tuple(cases[i]["size"]), "maxpool")
    idx = torch.from_numpy(g[f"r{i}_idx"])
    plane0 = torch.from_numpy(occ).flatten()[idx.flatten()].reshape(idx.shape)
    per_sample = torch.stack([torch.from_numpy(occ[b]).flatten()[idx[b].flatten()].reshape(idx[b].shape) for b in range(idx.shape[0])])
    assert torch.equal(res.occlusion.cpu(), plane0) and not torch.equal(plane0, per_sample)


def test_inverse_equals_the_reference(gold):
    from nndepth_amd.scene import Depth
    g = gold("scene.npz")
    for i, c in enumerate(json.loads(str(g["inverse_cases"]))):
        d = _t(g[f"i{i}_data"])
        valid = torch.isfinite(d)
        res = Depth(d, valid).inverse(clip_max=c["clip_max"], clip_min=c["clip_min"], eps=c["eps"])
        ref = torch.from_numpy(g[f"i{i}_out"])
        assert res.is_inverse and res.valid_mask is not valid and torch.equal(res.valid_mask, valid)
        assert torch.equal(torch.isnan(res.data.cpu()), torch.isnan(ref)), i
        assert torch.equal(torch.nan_to_num(res.data.cpu(), nan=-7.0), torch.nan_to_num(ref, nan=-7.0)), f"inverse case {i} {c}"


def test_frame_resize_equals_the_reference(gold):
    from nndepth_amd.scene import Camera, Depth, Disparity, Frame
    g = gold("scene.npz")
    pose = torch.eye(4)
    fr = Frame(_t(g["frame_data"]), Disparity(_t(g["frame_disp"]), "negative", _t(g["frame_occ"])),
               Depth(_t(g["frame_depth"]), _t(g["frame_valid"])), Camera(torch.from_numpy(g["frame_K"])), camera_id="left", pose=pose)
    res = fr.resize((12, 18), disparity_resize_method="maxpool", depth_resize_method="minpool")
    _check_bilinear(res.data, g["frame_f64"], float(g["frame_e_ref"]), float(g["frame_maxabs"]), "Frame.resize image, align_corners=True")
    assert res.data.ndim == 3 and res.pose is pose and res.camera_id is None
    assert torch.equal(res.disparity.data.cpu(), torch.from_numpy(g["frame_out_disp"]))
    assert torch.equal(res.disparity.occlusion.cpu(), torch.from_numpy(g["frame_out_occ"]))
    rd = torch.from_numpy(g["frame_out_depth"])
    assert torch.equal(torch.nan_to_num(res.depth.data.cpu(), nan=-7.0), torch.nan_to_num(rd, nan=-7.0))
    assert torch.equal(res.depth.valid_mask.cpu(), torch.from_numpy(g["frame_out_valid"]))
    assert torch.equal(res.camera.intrinsic, torch.from_numpy(g["frame_out_K"]))


def _random_table(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 1, 1, 37), (3, 1, 5, 7), (1, 1, 9, 2), (2, 2, 6, 13), (3, 1, 33, 258)])
@pytest.mark.parametrize("N", [2, 256, 4096])
def test_views_of_odd_shapes_and_table_sizes(shape, N):
    """Widths that are not multiples of 4 (byte stores, rows that start off a dword), a 1-row and a 1x1 map, batch 3, the
    smallest and the largest table — against the numpy float64 closed form."""
    from nndepth_amd.scene import Depth, Disparity
    g = torch.Generator().manual_seed(shape[-1] * 7 + N)
    data = (torch.randn(shape, generator=g) * 30).float()
    table = _random_table(N, N)
    for cls, kind in ((Disparity, "disp"), (Depth, "depth")):
        for mask in (None, torch.rand(shape, generator=g) < 0.6):
            if mask is not None and kind == "depth":
                mask.view(shape[0], -1)[:, 0] = True  # at least one valid pixel per batch element
            for kw in ({}, {"min": 3.0, "max": 41.5, "reverse": True}):
                obj = cls(data.to(DEV), "negative", None if mask is None else mask.to(DEV)) if kind == "disp" else \
                    cls(data.to(DEV), None if mask is None else mask.to(DEV))
                got = np.stack(obj.get_view(cmap=table, **kw))
                want = views_closed_form(data.numpy(), None if mask is None else mask.numpy(), kind, table,
                                         kw.get("min"), kw.get("max"), kw.get("reverse", False))
                assert np.array_equal(got, want), (shape, N, kind, mask is not None, kw)


def test_non_finite_values_never_leave_the_table():
    """Outside the contract (the colour is unspecified), but every index stays inside the table: with a table of one repeated
    colour every pixel must come back as that colour."""
    from nndepth_amd.scene import Disparity
    data = torch.tensor([float("nan"), float("inf"), -float("inf"), 1.0, -2.0, 0.0, 3e38, float("nan")]).view(1, 2, 4)
    table = np.full((7, 3), 201, np.uint8)
    for kw in ({}, {"min": 0.0, "max": 1.0}, {"min": -1e300, "max": 1e300, "reverse": True}):
        pic = Disparity(data.to(DEV)).get_view(cmap=table, **kw)
        assert pic.shape == (2, 4, 3) and (pic == 201).all()


def test_get_view_tensor_is_capturable_and_equals_get_view(gold):
    """No host synchronisation and no allocation outside PyTorch: get_view_tensor on a fixed input buffer is captured into a HIP
    graph once (linear graph, default queues) and replayed after the buffer's content changed."""
    from nndepth_amd.scene import Depth, Disparity
    g = gold("scene.npz")
    table = _t(g["table_RdYlGn"])
    maps = [_t(g["v0_data"]), _t(g["v0_data"]) * 0.37 - 1.0]
    valid = torch.rand(maps[0].shape, device=DEV) < 0.7
    for make in (lambda buf: Disparity(buf, "negative"), lambda buf: Depth(buf, valid)):
        buf = maps[0].clone()
        obj = make(buf)
        for _ in range(2):
            obj.get_view_tensor(cmap=table)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                out = obj.get_view_tensor(cmap=table)
        torch.cuda.current_stream(DEV).wait_stream(side)
        for m in maps[::-1]:
            buf.copy_(m)
            graph.replay()
            torch.cuda.synchronize()
            want = make(m.clone()).get_view(cmap=table)
            assert np.array_equal(out.cpu().numpy()[0], want)
            assert np.array_equal(make(m.clone()).get_view_tensor(cmap=table).cpu().numpy()[0], want)


def test_end_to_end_raft_disparity_view(raft_sd, tartanair_frames, gold):
    """The inference script's tail on device tensors: the model's up_disp coloured without leaving the GPU equals the numpy
    float64 closed form applied to up_disp.cpu()."""
    from nndepth_amd.raft_stereo import BaseRAFTStereo
    from nndepth_amd.scene import Disparity
    m = BaseRAFTStereo(iters=12, context_dim=64, outputs="last")
    m.load_state_dict(raft_sd, strict=True)
    m = m.to(DEV).eval()
    up = m(tartanair_frames[0].to(DEV), tartanair_frames[1].to(DEV))[-1]["up_disp"]
    assert tuple(up.shape) == (1, 1, 544, 960)
    table = gold("scene.npz")["table_RdYlGn"]
    pic = Disparity(up, "negative").get_view_tensor(cmap=_t(table))
    want = views_closed_form(up.cpu().numpy(), None, "disp", table)
    assert tuple(pic.shape) == (1, 544, 960, 3) and np.array_equal(pic.cpu().numpy(), want)
    assert np.array_equal(Disparity(up[0], "negative").get_view(cmap=table), want[0])
