"""CPU tier: the feasible-point entry points (include/katana_hip.h) through every layer that runs without a
GPU -- the header, the library's export table, the Python and Julia bindings and the front ends."""
import ctypes
import os
import re

import katana_jl_amd as ktn
from katana_jl_amd import _lib as L
from katana_jl_amd.batch import FusedBatch
from katana_jl_amd.solver import FeasiblePoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "katana_hip.h")).read()
JL = open(os.path.join(ROOT, "katana.jl_amd", "julia", "KatanaHIP.jl")).read()
SYMBOLS = ("ktn_get_feasible_point", "ktn_blocks_get_feasible_points")


def test_header_declares_the_entry_points():
    assert re.search(r"#define\s+KTN_FEAS_INFO_LEN\s+8\b", HEADER)
    assert re.search(r"\bint ktn_get_feasible_point\(ktn_handle h, double\* x_out, int64_t n, double\* info, int64_t cap\);", HEADER)
    assert re.search(r"\bint ktn_blocks_get_feasible_points\(ktn_handle h, double\* x_out, int64_t n,\s*double\* info, int64_t cap, int64_t\* count\);",
                     HEADER)
    assert re.search(r"#define\s+KTN_ABI_VERSION\s+1\b", HEADER)                  # the change only adds entry points
    assert re.search(r"\bint ktn_get_feasible_row_lambdas\(", HEADER)


def test_python_binding_and_library_carry_them():
    assert L.FEAS_INFO_LEN == 8
    lib = L.lib()
    for fn in SYMBOLS + ("ktn_get_feasible_row_lambdas",):
        assert fn in L.PROTOTYPES
        assert getattr(lib, fn) is not None                                       # exported (ctypes raises AttributeError otherwise)
    raw = ctypes.CDLL(L.LIB_PATH)
    for fn in SYMBOLS:
        assert hasattr(raw, fn)
    assert L.PROTOTYPES["ktn_get_feasible_point"][1][1:] == [L.P(L.c_f64), L.c_i64, L.P(L.c_f64), L.c_i64]
    assert L.PROTOTYPES["ktn_blocks_get_feasible_points"][1][1:] == [L.P(L.c_f64), L.c_i64, L.P(L.c_f64), L.c_i64, L.P(L.c_i64)]
    assert lib.ktn_abi_version() == 1


def test_julia_binding_calls_them():
    for fn in SYMBOLS:
        assert re.search(r"ccall\(\(:%s, LIB\), Cint," % fn, JL)
    assert re.search(r"^function feasible_point\(m::KatanaHipModel\)", JL, re.M)
    assert "const KTN_FEAS_INFO_LEN = 8" in JL
    assert re.search(r"export .*\bfeasible_point\b", JL)


def test_front_ends_have_the_methods():
    for name in ("feasible_point", "getfeasiblesolution", "getprimalbound", "getcertifiedgap", "getobjgap", "blocks_feasible_points"):
        assert callable(getattr(ktn.KatanaNonlinearModel, name)), name
        assert callable(getattr(ktn.LinearQuadraticModel, name)), name                # inherited
    assert callable(FusedBatch.feasible_points)
    assert FeasiblePoint._fields == ("found", "x", "lam", "objval", "nl_margin", "lin_viol", "blocking_row", "unconverged", "backoffs")
