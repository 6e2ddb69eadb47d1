"""CPU: the helper of the prior-contents tests (tests/history_util.py) does what tests/test_gpu_history.py relies on — reproducible
pattern fills with the stated range and sign mix that leave integer and bool tensors alone, buffers of an exact size on a 256-byte
boundary, allocator replacements that fill and undo themselves — and the package's modules take device memory through the three
allocators those replacements cover, so that no buffer escapes the poison unnoticed."""
import glob
import math
import os

import pytest
import torch

import history_util as hu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_patterns_are_reproducible_and_in_range():
    n = 1 << 16
    assert hu.PATTERNS == ("zero", "garbage", "nan")
    z, g, q = (hu.pattern(k, n) for k in hu.PATTERNS)
    assert z.dtype == g.dtype == q.dtype == torch.float32
    assert torch.equal(z, torch.zeros(n)) and bool(torch.isnan(q).all())
    assert torch.equal(g, hu.pattern("garbage", n)) and not torch.equal(g, hu.pattern("garbage", n, seed=1))
    assert bool(torch.isfinite(g).all())
    mag = g.abs().double()
    lo, hi = hu.GARBAGE_LOG2
    assert (lo, hi) == (-8.0, 12.0)
    assert float(mag.min()) >= 2.0 ** lo * (1 - 2.0 ** -23) and float(mag.max()) <= 2.0 ** hi * (1 + 2.0 ** -23)
    # log-uniform: every octave of [2^-8, 2^12] holds its twentieth of the values (+- 6 sigma of the binomial count)
    octave = torch.floor(torch.log2(mag)).clamp(lo, hi - 1)
    sigma = math.sqrt(n * 0.05 * 0.95)
    for o in range(int(lo), int(hi)):
        assert abs(int((octave == o).sum()) - n / 20) <= 6 * sigma, o
    assert abs(int((g > 0).sum()) - n / 2) <= 6 * math.sqrt(n / 4)  # the sign mix
    assert float(mag.max()) * 16 > 65504.0  # moves an fp16x2 maximum: overflows an fp16 piece at a scale of 16 already
    with pytest.raises(ValueError):
        hu.pattern("ones", 4)


def test_fill_touches_floating_point_tensors_only():
    for kind in ("garbage", "nan"):
        for dtype in (torch.float32, torch.float64, torch.float16):
            t = hu.fill_(torch.ones(3, 5, 7, dtype=dtype), kind)
            assert not bool((t == 1).any()), (kind, dtype)
            assert torch.equal(torch.isnan(t), torch.isnan(hu.pattern(kind, 105).reshape(3, 5, 7)))
        for t in (torch.ones(9, dtype=torch.int32), torch.ones(9, dtype=torch.int64), torch.ones(9, dtype=torch.bool),
                  torch.ones(9, dtype=torch.uint8)):
            assert torch.equal(hu.fill_(t.clone(), kind), t), (kind, t.dtype)
    a, b = hu.fill_(torch.empty(1000), "garbage", seed=3, offset=5), hu.fill_(torch.empty(1000), "garbage", seed=3, offset=5)
    assert torch.equal(a, b) and torch.equal(a, hu.pattern("garbage", 1 << 20, seed=3)[5:1005])
    assert not torch.equal(a, hu.fill_(torch.empty(1000), "garbage", seed=3, offset=6))
    view = torch.zeros(6, 8)[:, ::2]  # a strided view is filled where it lies
    assert not view.is_contiguous() and bool(torch.isnan(hu.fill_(view, "nan")).all())
    wrap = hu.fill_(torch.empty((1 << 20) + 10), "garbage", offset=(1 << 20) - 3)  # past the pool's end: read cyclically
    pool = hu.pattern("garbage", 1 << 20)
    assert torch.equal(wrap[:3], pool[-3:]) and torch.equal(wrap[3:13], pool[:10])
    # a byte workspace gets the pattern's bytes on request only
    raw = hu.fill_(torch.zeros(10, dtype=torch.uint8), "nan", raw_bytes=True)
    assert torch.equal(raw, torch.full((3,), float("nan")).view(torch.uint8)[:10])
    assert torch.equal(hu.fill_(torch.zeros(10, dtype=torch.int32), "nan", raw_bytes=True), torch.zeros(10, dtype=torch.int32))


@pytest.mark.parametrize("numel", [1, 63, 1000, 4097])
def test_aligned_buffer_has_the_exact_size_on_a_256_byte_boundary(numel):
    for dtype in (torch.float32, torch.float64):
        buf = hu.aligned_buffer(numel, "garbage", "cpu", dtype=dtype)
        assert buf.numel() == numel and buf.dtype == dtype and buf.is_contiguous() and buf.data_ptr() % 256 == 0
        assert torch.equal(buf, hu.pattern("garbage", 1 << 20)[:numel].to(dtype))  # the seeded pool from its start
    assert bool(torch.isnan(hu.aligned_buffer(numel, "nan", "cpu")).all())


def test_poisoned_allocators_fill_and_restore(monkeypatch):
    real = [torch.empty, torch.empty_like, torch.zeros]
    with hu.poisoned_allocators(monkeypatch, "nan", device_types=("cpu",)) as filled:
        assert torch.empty is not real[0] and torch.zeros is not real[2]
        a = torch.empty((2, 3), dtype=torch.float32)
        b = torch.empty_like(a)
        c = torch.zeros(4, dtype=torch.float64)
        i = torch.zeros(4, dtype=torch.int32)
        u = torch.empty(4, dtype=torch.uint8).fill_(7)
        assert all(bool(torch.isnan(t).all()) for t in (a, b, c))
        assert torch.equal(i, torch.tensor([0] * 4, dtype=torch.int32)) and bool((u == 7).all())
    assert [torch.empty, torch.empty_like, torch.zeros] == real
    assert filled == [("empty", (2, 3)), ("empty_like", (2, 3)), ("zeros", (4,))]
    with hu.poisoned_allocators(monkeypatch, "garbage", device_types=("cpu",)) as f1:
        x = [torch.empty(50), torch.zeros(70)]
    with hu.poisoned_allocators(monkeypatch, "garbage", device_types=("cpu",)) as f2:
        y = [torch.empty(50), torch.zeros(70)]
    assert f1 == f2 and all(torch.equal(p, q) for p, q in zip(x, y)) and not torch.equal(x[0], x[1][:50])  # reproducible, not repeated
    with hu.poisoned_allocators(monkeypatch, "nan"):  # default: device tensors only — host tensors are parameters being packed
        assert torch.equal(torch.zeros(3), torch.tensor([0.0] * 3))
    with hu.poisoned_allocators(monkeypatch, "nan", device_types=("cpu",), raw_bytes=True):
        assert not torch.equal(torch.zeros(8, dtype=torch.uint8), torch.tensor([0] * 8, dtype=torch.uint8))


def test_differences_compares_bits():
    a = [torch.tensor([1.0, float("nan"), 0.0]), torch.arange(3)]
    assert hu.differences(a, hu.snapshot(a)) == []
    assert len(hu.differences(a, [torch.tensor([1.0, float("nan"), -0.0]), torch.arange(3)])) == 1  # -0.0 is not 0.0
    assert len(hu.differences(a, [a[0], torch.arange(3) + 1])) == 1 and len(hu.differences(a, a[:1])) == 1
    assert [tuple(t.shape) for t in hu.flatten(({"a": a[0], "b": None}, [a[1], 2.5]))] == [(3,), (3,), ()]


def test_scan_flags_what_would_escape_the_poison():
    ok = """
    y = torch.empty((B, C), dtype=torch.float32, device=d)
    z = torch.empty_like(x)
    ws = torch.zeros(n, dtype=torch.float32, device=device)
    w = torch.ones(cout, dtype=torch.float64)  # a host tensor
    b = torch.full((3,), 2.0)
    coords = torch.arange(W, device=dev).float()
    """
    assert hu.scan_allocations(ok) == []
    for bad in ("y = x.new_empty((B, C))", "y = x.new_zeros(4)", "y = torch.empty_strided((2, 3), (3, 1), device=d)",
                "ws = torch.full((n,), 0.0, device=d)", "ws = torch.full((n,), 0.0,\n                dtype=torch.float32, device=d)",
                "a = torch.zeros_like(x)", "a = torch.ones((2, 9), device=m.device)", "a = torch.full_like(x, 1.0)"):
        assert len(hu.scan_allocations(bad)) == 1, bad
    assert hu.scan_allocations("# y = x.new_empty(3) in a comment") == []


def test_package_allocates_device_tensors_through_the_three_allocators_only():
    files = sorted(glob.glob(os.path.join(ROOT, "nndepth_amd", "*.py")))
    assert len(files) > 10
    hits = [f"{os.path.basename(f)}:{line}: {why}" for f in files for line, why in hu.scan_allocations(open(f).read())]
    assert hits == [], hits
    assert hu.ALLOCATORS == ("empty", "empty_like", "zeros")
