"""CPU: the C-ABI of the squeezer + soft-argmin beyond 8 groups / 512 candidates and of the nearest resize — arguments are checked
before any HIP call (a negative status and a message that names the limit, never a crash on a CPU-only host), the `supported`
query is the one table the Python side reads, and the header, the exported symbols and the ctypes table agree on the new names."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nnd_igev_init_disparity_dev", "nnd_igev_init_disparity_supported", "nnd_igev_init_disparity_chunk",
       "nnd_igev_init_disparity_kernel", "nnd_resize_nearest_scaled")


@pytest.fixture(scope="module")
def lib():
    from nndepth_amd._lib import lib
    return lib


@pytest.fixture(scope="module")
def bufs():
    """Four host buffers: non-null pointers for calls that must be refused before anything is enqueued."""
    keep = [(C.c_float * 64)() for _ in range(4)]
    return keep, [C.cast(b, C.c_void_p) for b in keep]


def _err(lib):
    return lib.nnd_last_error().decode()


def test_init_disparity_dev_refuses_bad_arguments(lib, bufs):
    _, (geo, w, b, out) = bufs
    assert lib.nnd_igev_init_disparity_dev(None, w, b, out, 1, 9, 4, 4, 16, None) < 0 and "null pointer" in _err(lib)
    assert lib.nnd_igev_init_disparity_dev(geo, None, b, out, 1, 9, 4, 4, 16, None) < 0 and "null pointer" in _err(lib)
    assert lib.nnd_igev_init_disparity_dev(geo, w, b, None, 1, 9, 4, 4, 16, None) < 0 and "null pointer" in _err(lib)
    assert lib.nnd_igev_init_disparity_dev(geo, w, b, out, 1, 0, 4, 4, 16, None) < 0 and ">= 1" in _err(lib)
    assert lib.nnd_igev_init_disparity_dev(geo, w, b, out, 1, 9, 4, 4, 0, None) < 0 and ">= 1" in _err(lib)
    assert lib.nnd_igev_init_disparity_dev(geo, w, b, out, 1, 65, 4, 4, 16, None) == -3  # NND_ERR_UNSUPPORTED
    assert "groups 65 (max 64)" in _err(lib)
    assert lib.nnd_igev_init_disparity_dev(geo, w, b, out, 1, 8, 4, 4, 4097, None) == -3
    assert "candidates 4097 (max 4096)" in _err(lib)
    assert lib.nnd_igev_init_disparity_dev(geo, w, b, out, 65536, 9, 4, 4, 16, None) < 0 and "65535" in _err(lib)
    # the host-pointer entry point keeps its limits and its message
    assert lib.nnd_igev_init_disparity(geo, w, b, out, 1, 9, 4, 4, 16, None) == -3 and "max 8" in _err(lib)
    assert lib.nnd_igev_init_disparity(geo, w, b, out, 1, 8, 4, 4, 513, None) == -3 and "max 512" in _err(lib)


@pytest.mark.parametrize("G,D,want", [(8, 512, True), (9, 21, True), (64, 4096, True), (1, 1, True), (65, 16, False), (8, 4097, False),
                                      (0, 16, False), (8, 0, False)])
def test_supported_query_is_the_python_sides_answer(lib, G, D, want):
    from nndepth_amd import ops
    assert bool(lib.nnd_igev_init_disparity_supported(G, D)) is want
    assert ops.igev_init_disparity_supported(G, D) is want


def test_kernel_query_and_chunk(lib):
    from nndepth_amd import ops
    C_ = lib.nnd_igev_init_disparity_chunk()
    src = open(os.path.join(ROOT, "nndepth_amd", "csrc", "corr1d.hip")).read()
    assert C_ == int(re.search(r"constexpr int SQG_C = (\d+)", src).group(1)) and C_ % 4 == 0
    assert ops.igev_init_disparity_kernel(1, 9, 4, 4, 16) == "igev_squeeze_general_kernel"
    assert ops.igev_init_disparity_kernel(1, 8, 4, 4, 513) == "igev_squeeze_general_kernel"
    assert ops.igev_init_disparity_kernel(1, 8, 4, 4, 512) == "igev_squeeze_softargmin_kernel"
    assert ops.igev_init_disparity_kernel(1, 8, 136, 240, 240) == "igev_squeeze_walk_kernel"
    assert ops.igev_init_disparity_kernel(1, 65, 4, 4, 16) is None and ops.igev_init_disparity_kernel(0, 8, 4, 4, 16) is None
    assert ops.igev_init_disparity_host_params(8, 512) and not ops.igev_init_disparity_host_params(9, 21)
    assert not ops.igev_init_disparity_host_params(8, 513) and not ops.igev_init_disparity_host_params(65, 16)


def test_resize_nearest_scaled_refuses_bad_arguments(lib, bufs):
    _, (x, y, _, _) = bufs
    assert lib.nnd_resize_nearest_scaled(None, y, 1, 2, 2, 4, 4, 2.0, None) < 0 and "null pointer" in _err(lib)
    assert lib.nnd_resize_nearest_scaled(x, y, 0, 2, 2, 4, 4, 2.0, None) < 0 and "bad shape" in _err(lib)
    assert lib.nnd_resize_nearest_scaled(x, y, 1, 2, 2, 5, 4, 2.0, None) < 0 and "not an integer ratio" in _err(lib)
    assert lib.nnd_resize_nearest_scaled(x, y, 1, 2, 3, 4, 4, 2.0, None) < 0 and "2x3 -> 4x4" in _err(lib)


def test_header_exports_and_ctypes_table_agree_on_the_new_names():
    from nndepth_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nndepth_amd.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        decl = re.search(r"([\w \*]+?)\b" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl, f"{name} is not declared in include/nndepth_amd.h"
        assert hasattr(raw, name), f"{name} is declared but not exported"
        res, args = _lib.SIGNATURES[name]
        params = [p for p in decl.group(2).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(args), (name, params)
        for p, a in zip(params, args):
            want = C.c_void_p if "*" in p else C.c_float if "float" in p else C.c_int
            assert a is want, (name, p, a)
        assert res is (C.c_char_p if "char" in decl.group(1) else C.c_int), name
