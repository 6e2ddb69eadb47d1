"""Shared by tests/test_gpu_history.py and tests/test_history_cpu.py (not a test module): what a buffer may hold before a call.

The contract under test (include/nndepth_amd.h, conventions): workspaces, scratch and output buffers may hold anything on entry, NaN
and inf included, and no result depends on it.  This module builds the "anything": three seeded, reproducible prior contents

  zero     the baseline
  garbage  finite values, magnitude log-uniform over [2^-8, 2^12], random sign: large enough to move an fp16x2 activation maximum and
           to overflow an fp16 piece once scaled, small enough that a coordinate built from them stays inside what the samplers clamp
  nan      quiet NaN everywhere: garbage times a zero-padded weight is harmless, NaN / inf times it is not, and a workspace does hold
           inf after an out-of-range fp16x2 frame — "read, then multiplied by zero" counts as a dependence

and the two ways to put them in front of a call: a buffer of an exact size on a 256-byte boundary to hand to an engine
(`aligned_buffer`), and replacements for the three allocators the package takes device memory from (`poisoned_allocators`).  The
source scan of tests/test_history_cpu.py (`scan_allocations`) keeps that list of three complete."""
import contextlib
import re
from typing import Dict, Iterable, List, Tuple

import torch

PATTERNS = ("zero", "garbage", "nan")
GARBAGE_LOG2 = (-8.0, 12.0)
ALLOCATORS = ("empty", "empty_like", "zeros")  # every device allocation of the package goes through torch.<one of these>
ALIGN = 256  # bytes; the encoder checks its workspace's alignment
_POOL = 1 << 20
_real = {name: getattr(torch, name) for name in ALLOCATORS}  # taken at import: the helpers below never see a replacement
_pools: Dict[Tuple[str, int, str], torch.Tensor] = {}


def pattern(kind: str, n: int, seed: int = 0) -> torch.Tensor:
    """n float32 values of the pattern on the CPU, a pure function of (kind, n, seed)."""
    if kind == "zero":
        return _real["zeros"](n, dtype=torch.float32)
    if kind == "nan":
        return torch.full((n,), float("nan"), dtype=torch.float32)
    if kind != "garbage":
        raise ValueError(f"unknown pattern {kind!r}")
    g = torch.Generator().manual_seed(0x5EED + seed)
    lo, hi = GARBAGE_LOG2
    mag = torch.exp2(lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64))
    sign = torch.randint(0, 2, (n,), generator=g, dtype=torch.int64) * 2 - 1
    return (mag * sign).to(torch.float32)


def _pool(kind: str, seed: int, device: torch.device) -> torch.Tensor:
    key = (kind, seed, str(device))
    if key not in _pools:
        _pools[key] = pattern(kind, _POOL, seed).to(device)
    return _pools[key]


def _take(kind: str, n: int, seed: int, offset: int, device: torch.device) -> torch.Tensor:
    """n values of the pattern on `device`: the seeded pool read cyclically from `offset`."""
    pool = _pool(kind, seed, device)
    offset %= _POOL
    if offset + n <= _POOL:
        return pool[offset:offset + n]
    reps = (offset + n + _POOL - 1) // _POOL
    return pool.repeat(reps)[offset:offset + n]


def fill_(t: torch.Tensor, kind: str, seed: int = 0, offset: int = 0, raw_bytes: bool = False) -> torch.Tensor:
    """Overwrite a floating-point tensor with the pattern, in place; integer and bool tensors are left alone (a stale index is not
    what this is about), except that raw_bytes=True also gives a uint8 tensor — a byte workspace — the pattern's bytes."""
    n = t.numel()
    if n == 0:
        return t
    if t.is_floating_point():
        t.copy_(_take(kind, n, seed, offset, t.device).reshape(t.shape))
    elif raw_bytes and t.dtype == torch.uint8:
        t.copy_(_take(kind, (n + 3) // 4, seed, offset, t.device).contiguous().view(torch.uint8)[:n].reshape(t.shape))
    return t


def aligned_buffer(numel: int, kind: str, device, seed: int = 0, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """A contiguous tensor of exactly `numel` elements that starts on a 256-byte boundary and holds the pattern."""
    size = _real["empty"]((), dtype=dtype).element_size()
    raw = _real["empty"](numel + ALIGN // size, dtype=dtype, device=device)
    skip = (-raw.data_ptr()) % ALIGN
    assert skip % size == 0
    buf = raw[skip // size:skip // size + numel]
    assert buf.numel() == numel and buf.data_ptr() % ALIGN == 0 and buf.is_contiguous()
    return fill_(buf, kind, seed)


@contextlib.contextmanager
def poisoned_allocators(monkeypatch, kind: str, seed: int = 0, device_types: Iterable[str] = ("cuda",), raw_bytes: bool = False):
    """Inside the block torch.empty, torch.empty_like and torch.zeros return tensors that hold the pattern (`fill_`: floating-point
    ones; successive allocations read the seeded pool at successive offsets, so the run is reproducible).  Only tensors on a device
    type of `device_types` are filled: host tensors of the package are parameters being folded and packed, not scratch.  Yields the
    list of (allocator, shape) it filled."""
    filled: List[Tuple[str, tuple]] = []
    types = tuple(device_types)
    offset = [0]

    def replacement(name):
        def alloc(*args, **kwargs):
            t = _real[name](*args, **kwargs)
            if t.device.type in types and (t.is_floating_point() or (raw_bytes and t.dtype == torch.uint8)):
                fill_(t, kind, seed, offset[0], raw_bytes)
                offset[0] += t.numel() + 17
                filled.append((name, tuple(t.shape)))
            return t
        return alloc

    with monkeypatch.context() as mp:
        for name in ALLOCATORS:
            mp.setattr(torch, name, replacement(name))
        yield filled


# ------------------------------------------------------------------------------------------------ comparing results bit for bit
def flatten(result) -> List[torch.Tensor]:
    """Every tensor of a nested result (tensors, None, numbers, tuples / lists / dicts of them), in order; numbers as float64."""
    if result is None:
        return []
    if torch.is_tensor(result):
        return [result]
    if isinstance(result, (int, float)):
        return [torch.tensor(float(result), dtype=torch.float64)]
    if isinstance(result, dict):
        return [t for k in result for t in flatten(result[k])]
    if isinstance(result, (tuple, list)):
        return [t for r in result for t in flatten(r)]
    raise TypeError(type(result))


def snapshot(result) -> List[torch.Tensor]:
    """Copies of every tensor of `result` (outputs may be views of a workspace that the next call overwrites)."""
    return [t.detach().clone() for t in flatten(result)]


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    if t.is_floating_point():
        return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def differences(a: List[torch.Tensor], b: List[torch.Tensor]) -> List[str]:
    """One line per tensor of `b` that is not `a`'s bit for bit (NaN equals NaN of the same bits); empty if all are identical."""
    if len(a) != len(b):
        return [f"{len(a)} tensors vs {len(b)}"]
    out = []
    for i, (x, y) in enumerate(zip(a, b)):
        if x.shape != y.shape or x.dtype != y.dtype:
            out.append(f"#{i}: {tuple(x.shape)} {x.dtype} vs {tuple(y.shape)} {y.dtype}")
            continue
        ne = _bits(x) != _bits(y)
        if bool(ne.any()):
            d = (x.double() - y.double()).abs()
            finite = d[torch.isfinite(d)]
            out.append(f"#{i} {tuple(x.shape)}: {int(ne.sum())} of {x.numel()} elements differ, "
                       f"{int((~torch.isfinite(y.double())).sum())} non-finite, "
                       f"largest finite difference {float(finite.max()) if finite.numel() else 0.0:.3e}")
    return out


# ------------------------------------------------------------------------------------------------ source scan
# Allocators that hand out a buffer with no data of its own in it: uninitialised, or one constant everywhere.  (arange, rand, tensor,
# linspace ... make values, not buffers.)
_BUFFER_MAKERS = ("empty", "empty_like", "empty_strided", "empty_permuted", "zeros", "zeros_like", "ones", "ones_like", "full", "full_like")
_CALL = re.compile(r"\btorch\.(" + "|".join(_BUFFER_MAKERS) + r")\(")
_METHOD = re.compile(r"\.new_(empty|empty_strided|zeros|ones|full|tensor)\(")


def _statement(lines: List[str], i: int) -> str:
    """Line i joined with its continuation lines (until the brackets opened on it are closed)."""
    text, depth = "", 0
    for line in lines[i:i + 12]:
        code = line.split("#", 1)[0]
        text += code
        depth += sum(code.count(c) for c in "([{") - sum(code.count(c) for c in ")]}")
        if depth <= 0:
            break
    return text


def scan_allocations(source: str) -> List[Tuple[int, str]]:
    """(line number, reason) of every buffer allocation in `source` that could put a device tensor out of `poisoned_allocators`'
    reach: a `.new_*(` method or a `*_like` other than torch.empty_like (the device comes with the tensor), torch.empty_strided /
    empty_permuted, and any other buffer maker called with a `device`.  It reads single statements as text: a host buffer moved
    afterwards (`torch.full(...).to(dev)`, `.cuda()`) is not seen, and the caller chooses the files (today the package has no
    sub-packages)."""
    lines = source.splitlines()
    hits = []
    for i, line in enumerate(lines):
        code = line.split("#", 1)[0]
        for m in _METHOD.finditer(code):
            hits.append((i + 1, f".new_{m.group(1)}("))
        for m in _CALL.finditer(code):
            name = m.group(1)
            if name in ALLOCATORS:
                continue
            if name.endswith("_like") or name in ("empty_strided", "empty_permuted") or "device" in _statement(lines, i):
                hits.append((i + 1, f"torch.{name}("))
    return hits
