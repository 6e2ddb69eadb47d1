"""CPU: the float64 reference of the fp16x2 calibration tests (tests/calib_cases.py) is the network of the pinned oracle, and its
cases are usable: no recorded maximum sits so close to a power of two that the GPU's fp32 tensors (about 1e-5 relative from
float64, the per-op bar of the parity tests) could land in the neighbouring octave and legitimately choose another scale."""
import math

import pytest
import torch

import calib_cases as CC
from oracle import torch_ref as R


@pytest.fixture(scope="module", params=CC.NAMES)
def walked(request):
    kw, gru, sd, prefix, ins = CC.make_case(request.param)
    outs, M = CC.staged_maxima(sd, prefix, *ins, gru=gru)
    return request.param, kw, gru, sd, prefix, ins, outs, M


def test_walk_is_the_oracles_update_block(walked):
    name, kw, gru, sd, prefix, ins, outs, M = walked
    ref = R.update_block({k: v.double() for k, v in sd.items()}, prefix, *(x.double() for x in ins), gru=gru)
    for got, exp, what in zip(outs, ref, ("net", "mask", "delta")):
        assert got.shape == exp.shape and got.dtype == torch.float64
        err = (got - exp).abs().max().item()
        assert err <= 1e-12 * exp.abs().max().item(), (name, what, err)


def test_walk_names_every_convolution_once(walked):
    name, kw, gru, sd, prefix, ins, outs, M = walked
    n_pass = 2 if gru == "sep_conv" else 1
    assert len(M) == 4 + 6 * n_pass + 2
    assert sum(CC.is_loop_only(k) for k in M) == 4 * n_pass and sum(CC.is_single_only(k) for k in M) == 2 * n_pass
    assert all(math.isfinite(v) and v > 0 for v in M.values())


def test_recorded_maxima_keep_clear_of_powers_of_two(walked):
    name, kw, gru, sd, prefix, ins, outs, M = walked
    for layer, m in M.items():
        print(f"{name:20s} {layer:32s} M = {m:9.5f}  range {CC.expected_range(m):9.1f}  margin {CC.power_of_two_margin(m):.3f}")
        assert CC.power_of_two_margin(m) >= 0.01, (name, layer, m)


def test_expected_range_arithmetic():
    assert CC.expected_range(1.0) == 65504.0 / 1024  # 1 = 0.5 * 2^1: xs = 10
    assert CC.expected_range(0.999) == 65504.0 / 2048
    assert CC.expected_range(511.0) == CC.DEFAULT_RANGE and CC.expected_range(512.0) == 2 * CC.DEFAULT_RANGE
    assert CC.expected_range(20000.0) == 65504.0 * 16
    assert CC.power_of_two_margin(1.0) == 0.0 and abs(CC.power_of_two_margin(1.01) - 0.01) < 1e-12
