"""GPU tier: the two exact LP solvers -- csrc/dense_lp.hpp (<= 32 columns, one kernel) and csrc/mid_lp.hpp (33 .. lp_mid_max_var
columns, 19 kernels) -- against an exact-rational KKT certificate (tests/exact_lp_ref.py) on the case list of
tests/exact_lp_cases.py.  lp_dense_after = -1 sends every LP straight to its exact solver.  Tolerances: those of
test_exact_small_lp_kernel_matches_highs (rows 1e-8, bounds 1e-9, |gap| <= 1e-7 max(1, |pobj|)); objective against HiGHS to 1e-9
relative for the dense kernel and 1e-7 for the mid-size solver, which keeps a 1e-9 cost perturbation."""
import functools

import numpy as np
import pytest

import katana_jl_amd as ktn
from exact_lp_cases import WARM_SEED, dense_cases, highs_solve, max_row_violation, mid_cases, start_vertex, warm_cases, warm_rows
from exact_lp_ref import certify, failures
from helpers import hip_load_instance

pytestmark = pytest.mark.gpu

MID = {c.name: c for c in mid_cases()}
DENSE = {c.name: c for c in dense_cases()}
OBJ_REL = {"mid_lp": 1e-7, "dense_lp": 1e-9}


@functools.lru_cache(maxsize=None)
def _highs(name):
    return highs_solve(MID[name] if name in MID else DENSE[name])


def _load(case, **kw):
    return hip_load_instance(ktn, case.instance(), **dict(dict(lp_dense_after=-1), **kw))


def _certify(case, m, rows=None):
    """the certificate of the handle's current (x, y) against the case's own data, or against `rows` = lp_rows() of the handle"""
    rowptr, col, val, lo, hi = (case.rowptr, case.col, case.val, case.lo, case.hi) if rows is None else rows
    cert = certify((rowptr, col, val), lo, hi, case.l, case.u, case.c, case.sense, m.getsolution(), m.lp_duals())
    print(case.name, cert)
    return cert


def _assert_optimal(case, m, prefix, want_obj, rows=None):
    cert = _certify(case, m, rows)
    print(case.name, "objective", m.getobjval(), "HiGHS", want_obj)
    assert abs(m.getobjval() - want_obj) <= OBJ_REL[prefix] * max(1.0, abs(want_obj)), (m.getobjval(), want_obj)
    assert failures(cert) == [], (failures(cert), cert)
    return cert


def _cold(case, prefix):
    m = _load(case)
    st, pivots = m.lp_solve()
    fallbacks = m.stat(prefix + "_fallbacks")
    print(case.name, st, "pivots", pivots, "solves", m.stat(prefix + "_solves"), "fallbacks", fallbacks, "refactors", m.stat("mid_lp_refactors"))
    if "bigbound" in case.tags and case.status == "Infeasible":
        # either the exact path says so, or it hands over (a counted fall-back) and the first-order path says so; never Optimal
        assert st == "Infeasible" and fallbacks in (0, 1)
        assert fallbacks == m.stat("lp_big_bound_rejects")                      # a hand-over here is the check of the bounds left out
        return m
    assert st == case.status
    assert fallbacks == 0
    if st == "Optimal":
        want = _highs(case.name)
        assert want[0] == "Optimal"
        assert m.stat(prefix + "_solves") == 1
        # pivots > 0 -- unless the bound vertex both solvers start from satisfies every row: it is the optimum then and no side enters
        boxed = bool(np.all(np.isfinite(case.l)) and np.all(np.isfinite(case.u)))
        if "start_optimal" in case.tags:
            assert pivots == 0 and m.getsolution()[1] == 0.0                   # x1 still on its artificial side at 0
        elif boxed and max_row_violation(case, start_vertex(case)) <= 0.0:
            assert pivots == 0 and case.m <= 1
        else:
            assert pivots > 0
        _assert_optimal(case, m, prefix, want[1])
        if "x0" in case.info:
            assert abs(m.getsolution()[0] - case.info["x0"]) <= 1e-9 * case.info["x0"]
    return m


@pytest.mark.parametrize("name", [n for n in MID if n != "mid_free8"])
def test_mid_size_solver_cold(name):
    m = _cold(MID[name], "mid_lp")
    if name == "mid_n33":
        assert m.stat("mid_lp_refactors") == 0                                 # the default cadence (1 500 pivots) is out of reach here


def test_free_column_below_its_artificial_side_is_handed_to_the_first_order_method():
    """mid_free8 (mid_free8_nonneg is its exact-path twin).  A free column starts on an artificial side at 0 that may only LEAVE the
    working set (mid_lp.hpp, by design), so a free column whose optimum lies on the other side of 0 cannot get there: the entering
    row finds no side to leave, the ray has weight on the artificial side, the solve gives up -- one counted fall-back -- and the
    first-order method answers.  Its tolerances are those test_gpu_lp.py asserts on that path after lp_solve(1e-8, 1e-8): rows
    1e-7, box exact (the prox clips), multipliers sign feasible, objective within 1e-6 relative of HiGHS; the same 1e-6 for the gap
    and for the charge of reduced costs on the free columns' missing bounds."""
    case = MID["mid_free8"]
    want = _highs(case.name)
    m = _load(case)
    st, iters = m.lp_solve(row_tol=1e-8, gap_tol=1e-8)
    print(case.name, st, "iterations", iters, "fallbacks", m.stat("mid_lp_fallbacks"), "solves", m.stat("mid_lp_solves"))
    assert st == "Optimal" and want[0] == "Optimal"
    assert m.stat("mid_lp_solves") == 1 and m.stat("mid_lp_fallbacks") == 1 and m.stat("pdhg_iters") > 0
    cert = _certify(case, m)
    scale = max(1.0, abs(want[1]))
    print(case.name, "objective", m.getobjval(), "HiGHS", want[1])
    assert abs(m.getobjval() - want[1]) <= 1e-6 * scale
    assert cert.row_viol <= 1e-7 and cert.bound_viol <= 1e-12 and cert.sign_ok
    assert abs(cert.gap) <= 1e-6 * scale and cert.charge <= 1e-6 * scale


@pytest.mark.parametrize("name", list(DENSE))
def test_dense_kernel_cold(name):
    _cold(DENSE[name], "dense_lp")


# ---- warm re-solve, purge remap, truncate ------------------------------------------------------------------------------------------

def _warm_sequence(solver, case, expect_refactor):
    prefix = solver + "_lp"
    # (purge_min_rows = 1: ktn_lp_purge does nothing below purge_min_rows appended rows, 2 000 by default)
    m = _load(case, purge_age=1, purge_min_frac=0.0, dedupe_eps=0.0, purge_min_rows=1)
    st, p1 = m.lp_solve()
    assert st == "Optimal" and p1 > 0
    x1, obj1 = m.getsolution(), m.getobjval()
    _assert_optimal(case, m, prefix, highs_solve(case)[1])
    # 20 rows slack by >= 1 at x*, then 5 rows that cut x* off
    extra = warm_rows(case, x1, WARM_SEED)
    m.lp_append_rows(*extra)
    st, p2 = m.lp_solve()
    print(case.name, "cold pivots", p1, "warm pivots", p2)
    assert st == "Optimal"
    if solver == "mid":
        assert m.stat("mid_lp_cold_starts") == 1
    # a cold start costs >= n pivots plus those for the cuts: 50 per cut separates warm from cold ...
    assert 0 < p2 <= 50 * 5
    # ... and so does the cold solve of the same grown LP on a fresh handle (the dense kernel has no cold-start counter: this is
    # what tells a reused working set from a silent cold start there; seen: 23 cold pivots at n = 12, 6 warm)
    fresh = _load(case)
    fresh.lp_append_rows(*extra)
    st, p_cold = fresh.lp_solve()
    print(case.name, "cold pivots of the grown LP", p_cold)
    assert st == "Optimal" and p2 < p_cold
    assert abs(fresh.getobjval() - m.getobjval()) <= OBJ_REL[prefix] * max(1.0, abs(m.getobjval()))
    want = highs_solve(case, extra)
    assert want[0] == "Optimal"
    rows = m.lp_rows()
    assert len(rows[3]) == case.m + 25
    _assert_optimal(case, m, prefix, want[1], rows)
    obj2 = m.getobjval()
    if solver == "mid":
        # purge: the slack rows go, the working cuts change index (k_mid_remap and the scatter of y onto the new indices)
        cold = m.stat("mid_lp_cold_starts")
        dropped = m.lp_purge()
        print(case.name, "purged", dropped)
        rows = m.lp_rows()
        assert dropped >= 15 and len(rows[3]) == case.m + 25 - dropped
        assert np.array_equal(rows[4][:case.m], case.hi, equal_nan=True)       # the loaded rows stay
        st, p3 = m.lp_solve()
        assert st == "Optimal" and p3 == 0 and m.stat("mid_lp_cold_starts") == cold
        assert abs(m.getobjval() - obj2) <= 1e-12 * max(1.0, abs(obj2))
        _assert_optimal(case, m, prefix, want[1], rows)
        assert np.count_nonzero(m.lp_duals()[case.m:]) >= 1                    # a cut carries a multiplier, at its NEW index
    # truncate back to the loaded rows: the warm start is void
    m.lp_truncate(case.m)
    cold = m.stat("mid_lp_cold_starts")
    st, p4 = m.lp_solve()
    assert st == "Optimal" and p4 == p1                                    # the cold solve of the loaded LP, pivot for pivot
    if solver == "mid":
        assert m.stat("mid_lp_cold_starts") == cold + 1
    assert abs(m.getobjval() - obj1) <= 1e-12 * max(1.0, abs(obj1)) and np.max(np.abs(m.getsolution() - x1)) <= 1e-9
    _assert_optimal(case, m, prefix, highs_solve(case)[1])
    assert m.stat(prefix + "_fallbacks") == 0
    print(case.name, "refactors", m.stat("mid_lp_refactors"))
    if expect_refactor:
        assert m.stat("mid_lp_refactors") >= 1
    return obj1, obj2


@pytest.mark.parametrize("solver,case", warm_cases(), ids=lambda v: getattr(v, "name", v))
def test_warm_resolve_purge_remap_and_truncate(solver, case, monkeypatch):
    monkeypatch.delenv("KTN_MID_REFACTOR", raising=False)
    _warm_sequence(solver, case, False if solver == "mid" else None)


# ---- refactorisation (k_mid_gj_*): KTN_MID_REFACTOR = 16 brings the 1 500-pivot cadence within reach of small LPs -------------------

@pytest.mark.parametrize("name", ["mid_n33", "mid_n65", "mid_n257", "mid_swap"])
def test_refactorisation_gives_the_same_answer(name, monkeypatch):
    """Gauss-Jordan with row swaps over [B | I].  A row that enters the working set takes the slot of the side that leaves, whatever
    its columns, and k_mid_gj_pivot pivots on the largest magnitude of the column: row swaps are routine in every one of these
    cases (a `k_mid_gj_swap` that swaps the wrong way fails them).  mid_swap adds a column with a single non-zero in B."""
    case = MID[name]
    want = _highs(name)
    res = []
    for every in (None, "16"):
        if every is None:
            monkeypatch.delenv("KTN_MID_REFACTOR", raising=False)
        else:
            monkeypatch.setenv("KTN_MID_REFACTOR", every)                     # (read when the handle is created)
        m = _load(case)
        st, pivots = m.lp_solve()
        print(name, "KTN_MID_REFACTOR", every, st, "pivots", pivots, "refactors", m.stat("mid_lp_refactors"))
        assert st == "Optimal" and m.stat("mid_lp_fallbacks") == 0 and m.stat("mid_lp_cold_starts") == 1
        _assert_optimal(case, m, "mid_lp", want[1])
        res.append((m.getobjval(), m.stat("mid_lp_refactors")))
    # (the default cadence is out of reach below ~1 500 pivots; the 2 900 pivots of n = 257 reach it once)
    assert res[1][1] > res[0][1] and (res[0][1] == 0 or case.n >= 255)
    assert abs(res[0][0] - res[1][0]) <= 1e-9 * max(1.0, abs(res[0][0]))


@pytest.mark.parametrize("solver,case", [w for w in warm_cases() if w[0] == "mid"], ids=lambda v: getattr(v, "name", v))
def test_warm_resolve_with_refactorisations(solver, case, monkeypatch):
    monkeypatch.delenv("KTN_MID_REFACTOR", raising=False)
    a = _warm_sequence(solver, case, False)
    monkeypatch.setenv("KTN_MID_REFACTOR", "16")
    b = _warm_sequence(solver, case, True)
    for u, v in zip(a, b):
        assert abs(u - v) <= 1e-9 * max(1.0, abs(u))


# ---- the multipliers the cutting-plane loop lives on ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mid_n33", "mid_n65", "mid_row_shapes_max", "mid_eq_range", "mid_n257"])
def test_loop_multipliers_are_optimal_for_the_perturbed_cost(name, monkeypatch):
    """lp_duals() after an exact mid-size solve returns the multipliers of the LP's own cost, computed on the call; dual inheritance,
    purge and the certificate of the loop read lp_y, which k_mid_final fills with those of the perturbed cost.  KTN_RAW_DUALS=1
    makes the accessor return lp_y.  Those are dual feasible for the cost c~ with |c~_j - s c_j| <= 1e-9 (1 + |c_j|) (k_mid_init),
    so against the true cost every column can cost the dual bound at most that times the width of its box: the gap is bounded by
    sum_j 1e-9 (1 + |c_j|) (u_j - l_j), plus the 1e-7 max(1, |pobj|) of the rounding.  Rows, signs and support as for the reported
    set; the two sets agree in sign wherever either is beyond the perturbation's reach."""
    case = MID[name]
    assert np.all(np.isfinite(case.l)) and np.all(np.isfinite(case.u))
    monkeypatch.delenv("KTN_RAW_DUALS", raising=False)
    m = _load(case)
    assert m.lp_solve()[0] == "Optimal"
    y_true = m.lp_duals()
    monkeypatch.setenv("KTN_RAW_DUALS", "1")                                   # (read when the handle is created)
    r = _load(case)
    assert r.lp_solve()[0] == "Optimal" and np.array_equal(r.getsolution(), m.getsolution())
    y_loop = r.lp_duals()
    cert = certify(case.csr(), case.lo, case.hi, case.l, case.u, case.c, case.sense, r.getsolution(), y_loop)
    bound = float(np.sum(1e-9 * (1.0 + np.abs(case.c)) * (case.u - case.l))) + 1e-7 * max(1.0, abs(cert.pobj))
    print(name, "loop multipliers: gap", cert.gap, "bound", bound, "max |y_loop - y_true|", np.max(np.abs(y_loop - y_true)))
    assert cert.sign_ok and cert.row_viol <= 1e-8 and abs(cert.gap) <= bound
    assert not np.array_equal(y_loop, y_true)                                   # two sets, as documented
    big = np.maximum(np.abs(y_loop), np.abs(y_true)) > 1e-6 * max(1.0, np.max(np.abs(y_true)))
    assert np.count_nonzero(big) >= 1 and np.array_equal(np.sign(y_loop[big]), np.sign(y_true[big]))
