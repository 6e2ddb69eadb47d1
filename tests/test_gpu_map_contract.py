"""GPU: the input contract that the map operations share (csrc/map_ops.h), tested once across the four that take a mask of either
polarity: speckle_filter, the view warp, fill_holes and median_filter (at radius 1 and, with a guide, at the largest radius).

Each operation runs twice on the same data: on a contiguous map with a torch.bool VALID mask of shape (B,1,H,W), and on channel 0
of a 2-channel tensor (a real batch stride) with the complementary OCCLUSION mask as uint8 of shape (B,H,W) whose set bytes are 3.
The value outputs of the two calls are equal bit for bit, their mask outputs exact complements, and both equal the numpy oracles
of tests/*_cases.py.  The shape is the smallest that crosses every tile and chunk border the library reports and leaves ragged
edges: B = 2, H = the tallest tile + 3, W = the widest tile or chunk + 5 ((2,1,35,261) with today's tiles).  The refusals tested
are Python's own; nothing here asks a kernel to go wrong."""
import functools

import numpy as np
import pytest
import torch

import median_cases as Mc
import speckle_cases as S
import warp_cases as Wc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAX_SIZE, THRESHOLD, FILL = 6, 1.0, -7.0


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, want) -> bool:
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return np.array_equal(S.bits(got), S.bits(want)) if want.dtype == np.float32 else np.array_equal(got, want)


@functools.lru_cache(maxsize=None)
def _data():
    """The inputs, built once and left unchanged: host arrays, and the device tensors of the two ways to pass them."""
    from nndepth_amd import geometry
    heights = (geometry.regions_tile()[0], geometry.median_tile()[0])
    widths = (geometry.regions_tile()[1], geometry.median_tile()[1], geometry.fill_chunk(), geometry.warp_chunk())
    shape = (2, 1, max(heights) + 3, max(widths) + 5)
    d, valid, max_diff = S.scene(shape, 11)
    g = S.rng(12)
    for value in (np.nan, np.inf, -np.inf):
        d[g.random(shape) < 0.01] = value
    valid[0, 0, 5] = False  # a row without a valid pixel: the column pass of fill_holes
    guide = g.uniform(0.0, 1.0, (2, 3) + shape[2:]).astype(np.float32)
    features = g.uniform(-1.0, 1.0, (2, 2) + shape[2:]).astype(np.float32)
    two = _t(np.concatenate([d, g.uniform(0.0, 9.0, shape).astype(np.float32)], axis=1))
    occlusion = (~valid).astype(np.uint8).reshape(shape[0], *shape[2:]) * 3
    assert two[:, :1].stride(0) == 2 * shape[2] * shape[3] and set(np.unique(occlusion)) == {0, 3}
    host = dict(d=d, valid=valid, occlusion=occlusion, max_diff=max_diff, guide=guide, features=features)
    ways = ((_t(d), _t(valid), True), (two[:, :1], _t(occlusion), False))  # (map, mask, mask_is_valid)
    return host, ways, _t(guide), _t(features)


def _speckle(map, mask, pol, h, guide, features):
    from nndepth_amd import geometry
    return geometry.speckle_filter(map, MAX_SIZE, h["max_diff"], mask, pol, 8, FILL)


def _speckle_oracle(mask, pol, h):
    return S.speckle_filter(h["d"], MAX_SIZE, h["max_diff"], mask, pol, 8, FILL)[:3]


def _warp(map, mask, pol, h, guide, features):
    from nndepth_amd import geometry
    return geometry._warp("map contract", map, "positive", "right", THRESHOLD, mask, pol, features, FILL, True)


def _warp_oracle(mask, pol, h):
    return Wc.warp(h["d"], "positive", "right", THRESHOLD, mask, h["features"], FILL, pol)


def _fill(vertical):
    def run(map, mask, pol, h, guide, features):
        from nndepth_amd import geometry
        return geometry.fill_holes(map, mask, pol, "min_abs", vertical, FILL)

    def oracle(mask, pol, h):
        return Wc.fill_holes(h["d"], mask, pol, "min_abs", vertical, FILL)
    return run, oracle


def _median(radius, guided):
    def r():
        from nndepth_amd import geometry
        return geometry.median_max_radius() if radius == "max" else radius

    def run(map, mask, pol, h, guide, features):
        from nndepth_amd import geometry
        return geometry.median_filter(map, r(), mask, pol, guide if guided else None, sigma=0.2, fill=FILL, return_changed=True)

    def oracle(mask, pol, h):
        table, inv_step = Mc.range_weights(0.2) if guided else (None, None)
        return Mc.median_filter(h["d"], r(), mask, pol, h["guide"] if guided else None, inv_step, table, fill=FILL)
    return run, oracle


# name -> (the call, its oracle, the index of the output that is a mask in the polarity of the input mask)
OPS = {"speckle_filter": (_speckle, _speckle_oracle, 1), "warp": (_warp, _warp_oracle, 1), "fill_holes": (*_fill(True), 2),
       "fill_holes_rows_only": (*_fill(False), 2), "median_r1": (*_median(1, False), 1), "median_max_guided": (*_median("max", True), 1)}


@pytest.mark.parametrize("op", list(OPS))
def test_both_mask_polarities_and_a_batch_stride_give_the_oracles_result(op):
    run, oracle, mask_at = OPS[op]
    host, ways, guide, features = _data()
    (map_a, mask_a, pol_a), (map_b, mask_b, pol_b) = ways
    got_a, got_b = run(map_a, mask_a, pol_a, host, guide, features), run(map_b, mask_b, pol_b, host, guide, features)
    want_a, want_b = oracle(host["valid"], True, host), oracle(host["occlusion"], False, host)
    assert len(got_a) == len(got_b) == len(want_a) == len(want_b)
    for i, (a, b, wa, wb) in enumerate(zip(got_a, got_b, want_a, want_b)):
        assert _same(a, wa) and _same(b, wb), (op, i)  # both calls equal the oracle
        if i == mask_at:
            a, b = a.cpu().numpy(), b.cpu().numpy()
            assert a.dtype == np.uint8 and max(a.max(), b.max()) <= 1 and np.array_equal(a, 1 - b), (op, i)  # exact complements
        else:
            assert _same(a, b.cpu().numpy()), (op, i)  # the values do not depend on how the mask was passed
    assert _same(map_a, host["d"]) and _same(map_b, host["d"]) and _same(mask_a, host["valid"]) and _same(mask_b, host["occlusion"])


@pytest.mark.parametrize("op", ["speckle_filter", "warp", "fill_holes", "median_r1"])
def test_python_refuses_a_mask_or_a_workspace_that_does_not_fit_the_map(op):
    from nndepth_amd import geometry
    from nndepth_amd._lib import NndError
    run = OPS[op][0]
    host, ways, guide, features = _data()
    map, mask, pol = ways[0]
    B, _, H, W = map.shape
    for bad, word in ((mask[:, :, :-1], "the mask is"), (mask[:1], "the mask is"), (mask.reshape(B, H * W), "the mask is"),
                      (mask.cpu(), "the mask is on cpu"), (mask.float(), "masks are torch.bool or torch.uint8"),
                      (host["valid"], "masks are torch.bool or torch.uint8")):
        with pytest.raises(NndError, match=word):
            run(map, bad, pol, host, guide, features)
    with pytest.raises(NndError, match="HIP device"):
        run(map.cpu(), mask.cpu(), pol, host, guide, features)
    small = torch.empty(16, dtype=torch.uint8, device=DEV)
    if op == "speckle_filter":
        with pytest.raises(NndError, match=r"a workspace of 16 bytes, \d+ needed \(regions_workspace_bytes\)"):
            geometry.speckle_filter(map, MAX_SIZE, 0.5, mask, workspace=small)
        with pytest.raises(NndError, match="the workspace must be a contiguous tensor on"):
            geometry.speckle_filter(map, MAX_SIZE, 0.5, mask, workspace=small.cpu())
    if op == "fill_holes":
        with pytest.raises(NndError, match=r"a workspace of 16 bytes, \d+ needed \(fill_workspace_bytes\)"):
            geometry.fill_holes(map, mask, workspace=small)
        with pytest.raises(NndError, match="the workspace must be a contiguous tensor on"):
            geometry.fill_holes(map, mask, workspace=torch.empty(1 << 16, dtype=torch.int32, device=DEV)[::2])
    if op == "warp":
        with pytest.raises(NndError, match=r"features are \(B,C,H,W\)"):
            run(map, mask, pol, host, guide, features[:, :, :-1])
