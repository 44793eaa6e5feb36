"""CPU tier: the entry points of the re-solve after a change of constraint bounds (include/katana_hip.h; DESIGN.md section 14
"Row bounds") through every layer that runs without a GPU -- the header, the library's export table, the Python and Julia
bindings and the front ends."""
import ctypes
import os
import re

import numpy as np

import katana_jl_amd as ktn
from katana_jl_amd import _lib as L
from katana_jl_amd.batch import FusedBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "katana_hip.h")).read()
JL = open(os.path.join(ROOT, "katana.jl_amd", "julia", "KatanaHIP.jl")).read()
SYMBOLS = ("ktn_set_row_bounds", "ktn_lp_get_row_owners")


def test_header_declares_the_entry_points():
    assert re.search(r"\bint ktn_set_row_bounds\(ktn_handle h, const double\* lb, const double\* ub, int64_t m\);", HEADER)
    assert re.search(r"\bint ktn_lp_get_row_owners\(ktn_handle h, int64_t\* owner, int64_t m\);", HEADER)
    assert re.search(r"#define\s+KTN_ABI_VERSION\s+1\b", HEADER)                  # the change only adds entry points
    for stat in ("rebase_rows", "rebase_kernel_s", "screen_crossed_rows"):
        assert '"%s"' % stat in HEADER, stat


def test_python_binding_and_library_carry_them():
    lib = L.lib()
    raw = ctypes.CDLL(L.LIB_PATH)
    for fn in SYMBOLS:
        assert fn in L.PROTOTYPES
        assert getattr(lib, fn) is not None and hasattr(raw, fn)                  # exported
    assert L.PROTOTYPES["ktn_set_row_bounds"] == (L.c_i32, [ctypes.c_void_p, L.P(L.c_f64), L.P(L.c_f64), L.c_i64])
    assert L.PROTOTYPES["ktn_lp_get_row_owners"] == (L.c_i32, [ctypes.c_void_p, L.P(L.c_i64), L.c_i64])
    assert lib.ktn_abi_version() == 1
    null = ctypes.c_void_p()                                                      # a null handle is refused, not dereferenced
    assert lib.ktn_set_row_bounds(null, None, None, 0) == L.E_INVALID
    assert lib.ktn_lp_get_row_owners(null, None, 0) == L.E_INVALID


def test_params_and_description_did_not_grow():
    assert ctypes.sizeof(L.KtnParams) == L.lib().ktn_sizeof_params()
    assert ctypes.sizeof(L.KtnNlpDesc) == L.lib().ktn_sizeof_nlp_desc()
    assert "row_bound" not in "".join(f for f, _ in L.KtnParams._fields_)
    # the sizes of the parent commit: neither struct gained a field
    assert (ctypes.sizeof(L.KtnParams), ctypes.sizeof(L.KtnNlpDesc)) == (264, 256)


def test_julia_binding_calls_them():
    for fn in SYMBOLS:
        assert re.search(r"ccall\(\(:%s, LIB\), Cint," % fn, JL), fn
    for method in ("setconstrLB!", "setconstrUB!"):
        assert re.search(r"^(function )?MathProgBase\.%s\(m::KatanaHipModel" % re.escape(method), JL, re.M), method
    assert re.search(r"^export .*\bsetconstrbounds!", JL, re.M) and re.search(r"^export .*\blp_row_owners\b", JL, re.M)
    assert re.search(r"^function setconstrbounds!\(m::KatanaHipModel, lb, ub\)", JL, re.M)
    assert re.search(r"^function lp_row_owners\(m::KatanaHipModel\)", JL, re.M)


def test_front_ends_have_the_methods():
    for name in ("setconstrLB", "setconstrUB", "setconstrbounds", "lp_row_owners"):
        assert callable(getattr(ktn.KatanaNonlinearModel, name)), name
        assert callable(getattr(ktn.LinearQuadraticModel, name)), name
    assert ktn.LinearQuadraticModel.setconstrbounds is not ktn.KatanaNonlinearModel.setconstrbounds      # the 7-argument path keeps its own copy
    assert callable(FusedBatch.set_row_bounds)


def test_linear_quadratic_model_keeps_changes_made_before_the_load():
    m = ktn.LinearQuadraticModel.__new__(ktn.LinearQuadraticModel)                # no handle: the 7-argument state alone
    m._lq = dict(n=2, lb=[-np.inf, 0.0], ub=[1.0, np.inf], dirty=True)
    m.setconstrbounds(None, [2.0, np.inf])
    assert m._lq["lb"] == [-np.inf, 0.0] and m._lq["ub"] == [2.0, np.inf]
    m.setconstrLB([-1.0, 0.5])
    m.setconstrUB([3.0, 4.0])
    assert m._lq["lb"] == [-1.0, 0.5] and m._lq["ub"] == [3.0, 4.0]
    try:
        m.setconstrbounds([0.0], None)
    except ValueError:
        pass
    else:
        raise AssertionError("a vector of the wrong length must be refused")
    assert m._lq["lb"] == [-1.0, 0.5]


def test_fused_batch_places_the_vectors_at_the_instances_rows():
    """FusedBatch.set_row_bounds without a handle: the fused vectors handed to setconstrbounds (fuse_instances puts the linear
    rows of every instance first, then the nonlinear rows)"""
    insts = [ktn.instances.make_instance(n=12, m_nl=2, k=4, family="explog", seed=s) for s in (1, 2)]
    big, offs = ktn.instances.fuse_instances(insts)

    class Rec:
        def setconstrbounds(self, lb, ub):
            self.got = (np.array(lb), np.array(ub))

    fb = FusedBatch.__new__(FusedBatch)
    fb.instances, fb.big, fb.offs, fb._objinfo, fb._row_bounds, fb.m = insts, big, offs, None, None, Rec()
    ub1 = np.array(insts[1].u_constr, dtype=np.float64) + 0.5
    cur = fb.set_row_bounds(None, [None, ub1])
    idx0, idx1 = [r for r, _ in fb._row_ranges()]
    assert np.array_equal(cur[1][idx1], ub1) and np.array_equal(cur[1][idx0], np.array(big.u_constr)[idx0])
    assert np.array_equal(cur[0], np.array(big.l_constr, dtype=np.float64)) and fb.m.got[1].tobytes() == cur[1].tobytes()
    lb0 = np.array(insts[0].l_constr, dtype=np.float64)
    cur2 = fb.set_row_bounds([lb0, None], None)                                   # the earlier change stays in force
    assert np.array_equal(cur2[1][idx1], ub1)
