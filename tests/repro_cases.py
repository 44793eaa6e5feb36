"""Cases of tests/test_gpu_reproducible.py: one function per solve path, each returning a FRESH solved handle (or batch) made under
the KTN_* environment of the moment of the call, and `fingerprint`, the tuple of everything a caller can read from it that is
not a time.  The cases are the smallest that still take the path each names; every case asserts through stat() that it did.

A fingerprint is a list of (field name, value); values are numpy arrays, ints, strings, or floats kept as one-element float64
arrays so that NaN compares equal to the same NaN and -0.0 differs from 0.0 (bytes are compared, never values)."""
import os

import numpy as np

import katana_jl_amd as ktn
from helpers import hip_load_instance, pool_arrays
from katana_jl_amd.batch import FusedBatch

L = ktn._lib
make = ktn.instances.make_instance

PURGE = dict(purge_min_rows=1, purge_min_frac=0.0)


class Solved:
    """a solved handle with what the fingerprint needs to know about it"""

    def __init__(self, m, status, inst=None, fb=None):
        self.m, self.status, self.inst, self.fb = m, status, inst, fb


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def purge_mid_instance():
    return make(n=300, m_nl=40, k=8, m_lin=100, family="explog", bound_frac=0.5)


PURGE_MID_KW = dict(PURGE, iter_cap=60)


def purge_mid():
    """the configuration of test_gpu_kkt.test_report_after_a_solve_that_purged, unchanged"""
    inst = purge_mid_instance()
    m = hip_load_instance(ktn, inst, **PURGE_MID_KW)
    st = m.optimize()
    for name in ("purges", "purged_rows", "mid_lp_solves", "lp_stalls"):
        assert m.stat(name) > 0, (name, m.stat(name))
    # an exact solve of this run ends with a row at two positions of its working set (k_mid_final's summed store, the race this
    # suite found): should the trajectory ever change, this says that the path is no longer covered
    assert m.stat("mid_lp_dup_sides") > 0, m.stat("mid_lp_dup_sides")
    return Solved(m, st, inst)


PURGE_PDHG_KW = dict(PURGE, lp_dense_after=0, iter_cap=25)
STEPPED_KW = {"purge_mid": PURGE_MID_KW, "purge_pdhg": PURGE_PDHG_KW}      # the solves that are also driven round by round


def purge_pdhg():
    """the same instance with the first-order LP only"""
    inst = purge_mid_instance()
    m = hip_load_instance(ktn, inst, **PURGE_PDHG_KW)
    st = m.optimize()
    assert m.stat("purges") > 0 and m.stat("mid_lp_solves") == 0 and m.stat("dense_lp_solves") == 0, (m.stat("purges"), m.stat("mid_lp_solves"))
    return Solved(m, st, inst)


def consolidate():
    """(b2) the quad-objective model of tests/tools/lp_bits.py, whose first-order solves consolidate"""
    inst = make(n=3000, m_nl=300, k=16, family="quad", seed=1, objective="quad")
    m = hip_load_instance(ktn, inst)
    st = m.optimize()
    assert m.stat("lp_consolidations") > 0, m.stat("lp_consolidations")
    return Solved(m, st, inst)


def mid_refactor():
    """the exact mid-size LP with warm starts, refactorisations every 40 pivots and purging on (KTN_MID_REFACTOR is read when the
    handle is made and put back at once).  n = 200, m_nl = 30, k = 8, m_lin = 60 and 100 rounds: at n = 120, m_nl = 20, k = 6,
    m_lin = 40 no purge of 60 -- or 200 -- rounds drops a working row (one cold start, the first solve's; measured on an MI355X)"""
    inst = make(n=200, m_nl=30, k=8, m_lin=60, family="explog", bound_frac=0.5)
    old = os.environ.get("KTN_MID_REFACTOR")
    os.environ["KTN_MID_REFACTOR"] = "40"
    try:
        m = hip_load_instance(ktn, inst, lp_dense_after=-1, iter_cap=100, **PURGE)
    finally:
        if old is None:
            del os.environ["KTN_MID_REFACTOR"]
        else:
            os.environ["KTN_MID_REFACTOR"] = old
    st = m.optimize()
    assert m.stat("mid_lp_refactors") > 0 and m.stat("purges") > 0, (m.stat("mid_lp_refactors"), m.stat("purges"))
    assert m.stat("mid_lp_cold_starts") >= 2, m.stat("mid_lp_cold_starts")      # a purge that drops a working row forces a cold start
    return Solved(m, st, inst)


def dense_instance():
    return make(n=24, m_nl=8, k=4, m_lin=8, family="explog")


def dense():
    inst = dense_instance()
    m = hip_load_instance(ktn, inst, lp_dense_after=-1)
    st = m.optimize()
    assert m.stat("dense_lp_solves") > 0
    return Solved(m, st, inst)


def epigraph():
    inst = make(n=300, m_nl=40, k=8, m_lin=100, family="explog", objective="quad")
    m = hip_load_instance(ktn, inst, iter_cap=30)
    st = m.optimize()
    assert m.stat("lp_epi_shifts") > 0
    return Solved(m, st, inst)


def supporting():
    """the smallest separable model of tests/test_gpu_supporting_hyperplanes.py (OFF_SMALL) under supporting-hyperplane cuts, the
    interior point found by the engine"""
    inst = make(n=50, m_nl=5, k=8, family="explog", seed=0, bound_frac=0.5)
    m = hip_load_instance(ktn, inst, cut_algo="supporting_hyperplane", iter_cap=40)
    st = m.optimize()
    assert m.stat("esh_interior_found") == 1 and m.stat("esh_rows") > 0, (m.stat("esh_interior_found"), m.stat("esh_rows"))
    return Solved(m, st, inst)


def _ellipsoid(which):
    import quad_cases as QC
    E = QC.ellipsoid(8)
    p = (QC.ellipsoid_quad if which == "quad" else QC.ellipsoid_tape)(E)
    m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, lp_dense_after=-1))
    m.loadproblem(*p)
    st = m.optimize()
    assert st == "Optimal" and m.stat("dense_lp_solves") + m.stat("mid_lp_solves") > 0
    return Solved(m, st)


def quad():
    return _ellipsoid("quad")


def tape():
    return _ellipsoid("tape")


def _blocks(supporting):
    insts = [make(n=40, m_nl=6, k=4, m_lin=12, seed=s) for s in range(8)]
    kw = dict(cut_algo="supporting_hyperplane") if supporting else {}
    fb = FusedBatch(ktn.KatanaSolver(log_level=0, lp_max_iter=400000, **kw), insts)
    st = fb.m.optimize_blocks(128, supporting=supporting)
    assert fb.m.stat("ecp_blocks_launches") == 1 and fb.m.stat("ecp_blocks_fallbacks") == 0
    if supporting:
        assert fb.m.stat("ecp_blocks_esh_rows") > 0
    return Solved(fb.m, st, fb=fb)


def blocks_kelley():
    return _blocks(False)


def blocks_supporting():
    return _blocks(True)


def resolve():
    """the shape of case `dense` with half of the variables off their bounds (on the vertex family every variable but one sits on a
    bound, and tightening it empties the box); two bounds tightened past the planted optimum, then a warm re-solve from the kept pool"""
    inst = make(n=24, m_nl=8, k=4, m_lin=8, family="explog", bound_frac=0.5)
    m = hip_load_instance(ktn, inst, lp_dense_after=-1)
    assert m.optimize() == "Optimal"
    l, u = np.array(inst.l_var, dtype=np.float64), np.array(inst.u_var, dtype=np.float64)
    x = np.asarray(inst.xhat, dtype=np.float64)[:inst.n]
    j0, j1 = np.argsort(-np.minimum(x - l, u - x), kind="stable")[:2]
    u[j0] = x[j0] - 0.25 * (x[j0] - l[j0])
    l[j1] = x[j1] + 0.25 * (u[j1] - x[j1])
    m.setvarbounds(l, u)
    st = m.optimize()
    assert m.stat("warm_solves") == 1, m.stat("warm_solves")
    return Solved(m, st, inst)


CASES = {"dense": dense, "resolve": resolve, "quad": quad, "tape": tape, "supporting": supporting, "blocks_kelley": blocks_kelley,
         "blocks_supporting": blocks_supporting, "mid_refactor": mid_refactor, "epigraph": epigraph, "purge_pdhg": purge_pdhg,
         "consolidate": consolidate, "purge_mid": purge_mid}


# ---- the fingerprint ------------------------------------------------------------------------------------------------------------
def _f(v):
    return np.array([v], dtype=np.float64)


def _try(fields, name, call):
    """a getter's answer, or the code it is refused with: a refusal is part of what the caller can read"""
    try:
        v = call()
    except L.KatanaHipError as e:
        fields.append((name, "refused %d" % e.code))
        return None
    return v


def state_fields(m):
    """what the loop itself leaves: status, counters, objective, point and the cut pool with its multipliers"""
    rows, duals, nrows, ncuts = pool_arrays(m)
    out = [("status", m.status()), ("numiters", m.numiters()), ("numcuts", ncuts), ("objval", _f(m.getobjval())),
           ("solution", m.getsolution()), ("lp_num_rows", nrows)]
    out += [("lp_rows." + n, a) for n, a in zip(("rowptr", "col", "val", "lo", "hi"), rows)]
    out.append(("lp_duals", duals))
    return out


def report_fields(m):
    """the KKT report and the feasible point with its objective"""
    out = []
    for name, call in (("getconstrduals", m.getconstrduals), ("getreducedcosts", m.getreducedcosts), ("getobjbound", m.getobjbound),
                       ("getobjgap", m.getobjgap)):
        v = _try(out, name, call)
        if v is not None:
            out.append((name, v if isinstance(v, np.ndarray) else _f(v)))
    fp = _try(out, "feasible_point", m.feasible_point)
    if fp is not None:
        out += [("feasible_point.found", fp.found), ("feasible_point.x", fp.x), ("feasible_point.objval", _f(fp.objval)),
                ("feasible_point.rest", np.array([fp.lam, fp.nl_margin, fp.lin_viol, fp.blocking_row, fp.unconverged, fp.backoffs], dtype=np.float64))]
    return out


def batch_fields(fb):
    m = fb.m
    out = [("blocks_results", m.blocks_results())]
    for b in range(len(fb.instances)):
        c = m.blocks_cuts(b)
        out += [("blocks_cuts[%d].%s" % (b, k), c[k]) for k in ("rowptr", "col", "val", "lo", "hi", "slot", "lam")]
        out.append(("blocks_duals[%d]" % b, m.blocks_duals(b)))
    v = _try(out, "blocks_dual_bounds", m.blocks_dual_bounds)
    if v is not None:
        out.append(("blocks_dual_bounds", v))
    v = _try(out, "blocks_feasible_points", m.blocks_feasible_points)
    if v is not None:
        out += [("blocks_feasible_points.x", v[0]), ("blocks_feasible_points.info", v[1])]
    return out


def fingerprint(s, report=True):
    """s: a Solved, or a bare handle (then without the batch fields)"""
    m = s.m if isinstance(s, Solved) else s
    out = []
    if isinstance(s, Solved):
        out.append(("optimize", s.status))
    out += state_fields(m)
    if report:
        out += report_fields(m)
        if isinstance(s, Solved) and s.fb is not None:
            out += batch_fields(s.fb)
    return out


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape
                and a.tobytes() == b.tobytes())
    return type(a) is type(b) and a == b


def first_difference(a, b):
    """None when the two fingerprints are equal; else a description of the first field that differs: its name, and for arrays
    the first differing index with both values"""
    for k in range(max(len(a), len(b))):
        if k >= len(a) or k >= len(b):
            return "field %d: %r against %r (one fingerprint ends)" % (k, a[k][0] if k < len(a) else None, b[k][0] if k < len(b) else None)
        (na, va), (nb, vb) = a[k], b[k]
        if na != nb:
            return "field %d is %r in one and %r in the other" % (k, na, nb)
        if _same(va, vb):
            continue
        if isinstance(va, np.ndarray) and isinstance(vb, np.ndarray) and va.dtype == vb.dtype and va.shape == vb.shape:
            fa, fb_ = va.reshape(-1), vb.reshape(-1)
            ua = np.frombuffer(fa.tobytes(), dtype=np.uint8).reshape(len(fa), -1)
            ub = np.frombuffer(fb_.tobytes(), dtype=np.uint8).reshape(len(fb_), -1)
            bad = np.flatnonzero((ua != ub).any(axis=1))
            i = int(bad[0])
            return "%s: %d of %d elements differ, first at index %d: %r against %r" % (na, len(bad), len(fa), i, fa[i], fb_[i])
        if isinstance(va, np.ndarray) and isinstance(vb, np.ndarray):
            return "%s: %s%r against %s%r" % (na, va.dtype, va.shape, vb.dtype, vb.shape)
        return "%s: %r against %r" % (na, va, vb)
    return None
