"""CPU tier: the entry points of the re-solve from the kept cut pool (include/katana_hip.h) through every layer
that runs without a GPU -- the header, the library's export table, the Python and Julia bindings and the front ends."""
import ctypes
import os
import re

import katana_jl_amd as ktn
from katana_jl_amd import _lib as L
from katana_jl_amd.batch import FusedBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "katana_hip.h")).read()
JL = open(os.path.join(ROOT, "katana.jl_amd", "julia", "KatanaHIP.jl")).read()
SYMBOLS = ("ktn_set_var_bounds", "ktn_set_linear_objective", "ktn_lp_row_activity")


def test_header_declares_the_entry_points():
    assert re.search(r"\bint ktn_set_var_bounds\(ktn_handle h, const double\* l, const double\* u, int64_t n\);", HEADER)
    assert re.search(r"\bint ktn_set_linear_objective\(ktn_handle h, const double\* c, int64_t n, double c0\);", HEADER)
    assert re.search(r"\bint ktn_lp_row_activity\(ktn_handle h, double\* amin, double\* amax, int64_t m\);", HEADER)
    assert re.search(r"#define\s+KTN_ABI_VERSION\s+1\b", HEADER)                  # the change only adds entry points
    for stat in ("screen_runs", "screen_infeasible_rows", "screen_crossed_cols", "screen_first_row", "screen_redundant_rows",
                 "warm_solves", "warm_clamped_cols"):
        assert '"%s"' % stat in HEADER, stat


def test_python_binding_and_library_carry_them():
    lib = L.lib()
    raw = ctypes.CDLL(L.LIB_PATH)
    for fn in SYMBOLS:
        assert fn in L.PROTOTYPES
        assert getattr(lib, fn) is not None and hasattr(raw, fn)                  # exported
    assert L.PROTOTYPES["ktn_set_var_bounds"] == (L.c_i32, [ctypes.c_void_p, L.P(L.c_f64), L.P(L.c_f64), L.c_i64])
    assert L.PROTOTYPES["ktn_set_linear_objective"] == (L.c_i32, [ctypes.c_void_p, L.P(L.c_f64), L.c_i64, L.c_f64])
    assert L.PROTOTYPES["ktn_lp_row_activity"] == (L.c_i32, [ctypes.c_void_p, L.P(L.c_f64), L.P(L.c_f64), L.c_i64])
    assert lib.ktn_abi_version() == 1
    null = ctypes.c_void_p()                                                      # a null handle is refused, not dereferenced
    assert lib.ktn_set_var_bounds(null, None, None, 0) == L.E_INVALID
    assert lib.ktn_set_linear_objective(null, None, 0, 0.0) == L.E_INVALID
    assert lib.ktn_lp_row_activity(null, None, None, 0) == L.E_INVALID


def test_params_and_description_did_not_grow():
    assert ctypes.sizeof(L.KtnParams) == L.lib().ktn_sizeof_params()
    assert ctypes.sizeof(L.KtnNlpDesc) == L.lib().ktn_sizeof_nlp_desc()
    assert "set_var" not in "".join(f for f, _ in L.KtnParams._fields_)


def test_julia_binding_calls_them():
    for fn in SYMBOLS:
        assert re.search(r"ccall\(\(:%s, LIB\), Cint," % fn, JL), fn
    for method in ("setvarLB!", "setvarUB!", "setobj!"):
        assert re.search(r"^(function )?MathProgBase\.%s\(m::KatanaHipModel" % re.escape(method), JL, re.M), method
    assert re.search(r"^export .*\bsetvarbounds!", JL, re.M) and re.search(r"^export .*\blp_row_activity\b", JL, re.M)


def test_front_ends_have_the_methods():
    for name in ("setvarLB", "setvarUB", "setvarbounds", "setobj", "lp_row_activity"):
        assert callable(getattr(ktn.KatanaNonlinearModel, name)), name
        assert callable(getattr(ktn.LinearQuadraticModel, name)), name
    assert ktn.LinearQuadraticModel.setvarbounds is not ktn.KatanaNonlinearModel.setvarbounds      # the 7-argument path keeps its own copy
    assert callable(FusedBatch.set_var_bounds) and callable(FusedBatch.set_costs)


def test_linear_quadratic_model_keeps_changes_made_before_the_load():
    m = ktn.LinearQuadraticModel.__new__(ktn.LinearQuadraticModel)                # no handle: the 7-argument state alone
    m._lq = dict(n=2, collb=[0.0, 0.0], colub=[1.0, 1.0], obj=[1.0, 1.0], dirty=True)
    m.setvarbounds([0.5, 0.5], None)
    m.setobj([2.0, 3.0])
    assert list(m._lq["collb"]) == [0.5, 0.5] and list(m._lq["colub"]) == [1.0, 1.0] and list(m._lq["obj"]) == [2.0, 3.0]
