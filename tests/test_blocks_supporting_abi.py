"""CPU tier: the surface of supporting-hyperplane cuts inside the device-side batch loop -- the header's flags and entry points,
their ctypes prototypes, which symbol optimize_blocks() resolves to, and the fused layout of per-instance interior points.
Nothing here needs a GPU (the solves are in tests/test_gpu_blocks_supporting.py)."""
import ctypes as C
import math
import os
import re

import numpy as np

import katana_jl_amd as ktn
from katana_jl_amd import batch, nlp
from katana_jl_amd import _lib as L
from katana_jl_amd.solver import KatanaNonlinearModel

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = open(os.path.join(HERE, "..", "include", "katana_hip.h")).read()
NEW = ("ktn_optimize_blocks_ex", "ktn_blocks_get_results", "ktn_blocks_get_cuts")


def test_header_defines_the_flags_and_declares_the_entry_points():
    flags = dict(re.findall(r"#define\s+(KTN_BLOCKS_\w+)\s+(\d+)", HEADER))
    assert flags == {"KTN_BLOCKS_SUPPORTING": "1", "KTN_BLOCKS_NO_FALLBACK": "2"}
    assert re.search(r"int\s+ktn_optimize_blocks_ex\(ktn_handle h, int32_t cut_capacity, int32_t flags\);", HEADER)
    assert re.search(r"int\s+ktn_blocks_get_results\(ktn_handle h, double\* out, int64_t cap, int64_t\* count\);", HEADER)
    assert re.search(r"int\s+ktn_blocks_get_cuts\(ktn_handle h, int64_t block,", HEADER)
    # the slot meanings of the per-instance records are documented where the caller reads them
    doc = HEADER[HEADER.index("KTN_BLOCKS_NO_FALLBACK 2"):HEADER.index("int ktn_blocks_get_results")]
    for word in ("status", "iterations", "objective", "cuts", "PDHG", "violation", "LP rows", "overflow"):
        assert word in doc, word


def test_python_prototypes_and_constants_match_the_header():
    assert (L.BLOCKS_SUPPORTING, L.BLOCKS_NO_FALLBACK) == (1, 2)
    i32, i64, f64, P, vp = C.c_int32, C.c_int64, C.c_double, C.POINTER, C.c_void_p
    assert L.PROTOTYPES["ktn_optimize_blocks_ex"] == (i32, [vp, i32, i32])
    assert L.PROTOTYPES["ktn_blocks_get_results"] == (i32, [vp, P(f64), i64, P(i64)])
    assert L.PROTOTYPES["ktn_blocks_get_cuts"] == (i32, [vp, i64, P(i64), P(i32), P(f64), P(f64), P(f64), P(i64), P(f64), i64, i64, P(i64), P(i64)])
    # the argument count of the C declaration of ktn_blocks_get_cuts
    decl = re.search(r"int ktn_blocks_get_cuts\((.*?)\);", HEADER, re.S).group(1)
    assert len(decl.split(",")) == len(L.PROTOTYPES["ktn_blocks_get_cuts"][1])
    for name in NEW:                                              # the built library exports them
        assert hasattr(L.lib(), name), name


class _Recorder:
    """stands in for the loaded library: records which symbol a call went to"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name,) + tuple(a for a in args[1:]))
            return L.STATUS_OPTIMAL
        return fn


def _model():
    m = object.__new__(KatanaNonlinearModel)                       # no handle: nothing below reaches the engine
    m._lib, m._h = _Recorder(), None
    return m


def test_optimize_blocks_with_default_keywords_is_the_old_symbol():
    m = _model()
    assert m.optimize_blocks() == "Optimal" and m.optimize_blocks(7) == "Optimal"
    assert m._lib.calls == [("ktn_optimize_blocks", 0), ("ktn_optimize_blocks", 7)]
    m = _model()
    m.optimize_blocks(supporting=True)
    m.optimize_blocks(3, fallback=False)
    m.optimize_blocks(supporting=True, fallback=False)
    assert m._lib.calls == [("ktn_optimize_blocks_ex", 0, L.BLOCKS_SUPPORTING), ("ktn_optimize_blocks_ex", 3, L.BLOCKS_NO_FALLBACK),
                            ("ktn_optimize_blocks_ex", 0, L.BLOCKS_SUPPORTING | L.BLOCKS_NO_FALLBACK)]


def _lin_problem(n, seed):
    rng = np.random.default_rng(seed)
    d = ktn.QuadNLP(n, rng.uniform(-1, 1, n), 0.0, None, [(np.arange(n), np.ones(n), np.arange(n), np.arange(n), np.ones(n), 0.0)])
    return ktn.Problem(n, 1, np.full(n, -2.0), np.full(n, 2.0), [-math.inf], [1.0], "Min", d)


def _quad_objective_problem(n, seed):
    rng = np.random.default_rng(seed)
    d = ktn.QuadNLP(n, rng.uniform(-1, 1, n), 0.0, (np.arange(n), np.arange(n), np.ones(n)),
                    [(np.arange(n), np.ones(n), np.arange(n), np.arange(n), np.ones(n), 0.0)])
    return ktn.Problem(n, 1, np.full(n, -2.0), np.full(n, 2.0), [-math.inf], [1.0], "Min", d)


def test_set_interior_points_lays_the_points_out_at_the_fused_offsets():
    probs = [_lin_problem(3, 0), _quad_objective_problem(4, 1), _lin_problem(2, 2)]
    big, offs, objinfo = nlp.fuse_problems(probs, allow_quad=True)
    assert list(np.diff(offs)) == [3, 5, 2]                        # the quadratic objective's epigraph variable is column 4 of instance 1
    pts = [np.array([1.0, 2.0, 3.0]), np.array([4.0, 5.0, 6.0, 7.0]), np.array([8.0, 9.0])]
    want = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 0.0, 8.0, 9.0])

    class _Model:
        def set_interior_point(self, x):
            self.x = None if x is None else np.array(x)
    fb = object.__new__(batch.FusedBatch)                          # a loaded batch without its handle
    fb.m, fb.offs, fb._objinfo, fb._nvar = _Model(), offs, objinfo, [int(p.num_var) for p in probs]
    got = fb.set_interior_points(pts)
    assert np.array_equal(got, want) and np.array_equal(fb.m.x, want) and len(want) == big.num_var
    fb.set_interior_points(None)
    assert fb.m.x is None
    # separable instances: no column is added, every instance fills its range
    assert np.array_equal(batch.fuse_points([[1.0], [2.0, 3.0]], np.array([0, 1, 3])), [1.0, 2.0, 3.0])
    for bad in ([pts[0], pts[1]], [pts[0], pts[1][:3], pts[2]]):
        try:
            batch.fuse_points(bad, offs, fb._nvar)
        except ValueError:
            continue
        raise AssertionError("a wrong number of points or entries must be refused")
