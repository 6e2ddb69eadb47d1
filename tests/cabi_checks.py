"""What the CPU tests of every C-ABI unit check in the same way (a plain module, imported by tests/test_*_cpu.py)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"int64_t": C.c_int64, "int": C.c_int, "double": C.c_double, "float": C.c_float}


def header_exports_ctypes_table_and_makefile_rule_agree(names, unit, flags=("$(NOSLP)", "-ffp-contract=off")):
    """Every name is declared in the header, exported by the built library and listed in _lib.SIGNATURES with the same result
    and, parameter by parameter, the same pointer / integer / floating kind; `unit`.o is in the Makefile's OBJS and its own rule
    carries `flags`."""
    from nndepth_amd import _lib
    header = open(os.path.join(ROOT, "include", "nndepth_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in names:
        proto = re.search(rf"\b(int64_t|int)\s+{name}\s*\(([^;]*)\)\s*;", code)
        assert proto, f"{name} is not declared in include/nndepth_amd.h"
        assert hasattr(raw, name), f"{name} is not exported"
        res, args = _lib.SIGNATURES[name]
        assert res is (C.c_int64 if proto.group(1) == "int64_t" else C.c_int)
        params = [p.strip() for p in proto.group(2).split(",") if p.strip() != "void"]
        assert len(params) == len(args), f"{name}: {len(params)} parameters declared, {len(args)} in the ctypes table"
        for p, a in zip(params, args):
            want = C.c_void_p if "*" in p else KINDS[p.split()[0]]
            assert a is want, f"{name}: `{p}` is {a.__name__} in the ctypes table"
    mk = open(os.path.join(ROOT, "nndepth_amd", "csrc", "Makefile")).read()
    assert re.search(rf"^OBJS\s*=.*\b{unit}\.o\b", mk, re.M)
    rule = re.search(rf"^{unit}\.o:.*\n\t(.*)$", mk, re.M)
    assert rule and all(flag in rule.group(1) for flag in flags)


def refused(rc, word):
    """The call was refused (rc < 0) and the library's error message holds `word` (bytes)."""
    from nndepth_amd._lib import lib
    assert rc < 0 and word in lib.nnd_last_error(), (rc, lib.nnd_last_error())
