"""CPU tier: the exact-rational KKT certificate (tests/exact_lp_ref.py) and the case list of the exact-LP tests
(tests/exact_lp_cases.py).  Keeps the reference honest -- it accepts an independent solver's optimal pair and rejects pairs that are
wrong in known ways -- and proves without a GPU that every case is what the list claims it is."""
import functools

import numpy as np
import pytest

from exact_lp_cases import WARM_SEED, dense_cases, highs_solve, mid_cases, warm_cases, warm_rows
from exact_lp_ref import BOUND_TOL, ROW_TOL, certify, failures

CASES = {c.name: c for c in mid_cases() + dense_cases()}


@functools.lru_cache(maxsize=None)
def _highs(name):
    return highs_solve(CASES[name])


def _cert(case, x, y):
    return certify(case.csr(), case.lo, case.hi, case.l, case.u, case.c, case.sense, x, y)


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_has_the_status_the_list_claims_and_highs_is_certified(name):
    case = CASES[name]
    st, obj, x, y = _highs(name)
    assert st == case.status
    # the conditions of the list: boxed unless the case says otherwise, at most 8 free columns
    free = np.flatnonzero(~np.isfinite(case.l) & ~np.isfinite(case.u))
    assert len(free) <= 8
    if case.n >= 33 and "free" not in case.tags:
        assert np.all(np.isfinite(case.l)) and np.all(np.isfinite(case.u))
    if st != "Optimal":
        return
    cert = _cert(case, x, y)
    assert failures(cert) == [], (cert, failures(cert))
    s = -1.0 if case.sense == "Max" else 1.0
    assert abs(s * obj - cert.pobj) <= 1e-12 * max(1.0, abs(obj))
    info = case.info
    if "active_among" in info:                                           # the planted rows carry a multiplier
        assert np.any(np.abs(y[info["active_among"]]) > 1e-9), y[info["active_among"]]
    if "lower_active" in info:
        assert y[info["lower_active"]] > 1e-6 and y[info["upper_active"]] < -1e-6 and all(y[r] > 1e-6 for r in info["eq_rows"])
    if "repeated_row" in info:
        r = info["repeated_row"]
        cols = case.col[case.rowptr[r]:case.rowptr[r + 1]]
        assert len(set(cols.tolist())) < len(cols)
    if "empty_row" in info:
        r = info["empty_row"]
        assert case.rowptr[r] == case.rowptr[r + 1] and case.hi[r] >= 0.0
    if "nan_row" in info:
        assert np.isnan(case.hi[info["nan_row"]]) and case.lo[info["nan_row"]] == -np.inf
    if "free_cols" in info:
        assert 4 <= len(info["free_cols"]) <= 8 and free.tolist() == info["free_cols"]
    if "flipped" in info:
        assert len(info["flipped"]) >= 1 and np.all(x[info["free_cols"]] >= 0.0)
    elif "free_cols" in info:
        assert np.any(x[info["free_cols"]] < 0.0)                           # a free column has to go below the artificial side at 0
    if "x0" in info:
        assert abs(x[0] - info["x0"]) <= 1e-9 * info["x0"]
    if "swap_row" in info:
        # column 0 occurs in row R alone, R carries a multiplier and x0 is basic: column 0 of the optimal working matrix has its only
        # non-zero in the slot of R, whichever that is
        R = info["swap_row"]
        rows = np.repeat(np.arange(case.m), np.diff(case.rowptr))
        assert rows[case.col == 0].tolist() == [R]
        assert abs(y[R]) > 1e-6 and case.l[0] + 1e-3 < x[0] < case.u[0] - 1e-3
    if "price2" in case.tags:
        assert case.m > 4096 and min(info["active_among"]) >= 4096
    if "longrow" in case.tags:
        r = info["active_among"][0]
        assert case.rowptr[r + 1] - case.rowptr[r] == 300


def test_the_list_covers_what_the_solvers_branch_on():
    mid, dense = mid_cases(), dense_cases()
    assert {c.n for c in mid if "size" in c.tags} == {33, 34, 63, 65, 255, 257, 511, 512}
    assert all(c.m == 3 * c.n for c in mid if "size" in c.tags)
    assert {c.n for c in dense if "size" in c.tags} == {1, 2, 31, 32}
    assert {c.m for c in dense if "size" in c.tags} == {0, 1, 255, 257, 600}
    shapes = [c for c in mid if c.name == "mid_row_shapes"][0]
    assert {1, 7, 8, 9, 17} <= set(np.diff(shapes.rowptr).tolist())
    assert sum(1 for c in mid if c.sense == "Max") == 2 and sum(1 for c in dense if c.sense == "Max") == 2
    eq = [c for c in mid if c.name == "mid_eq_range"][0]
    assert all(eq.lo[r] == eq.hi[r] for r in eq.info["eq_rows"])
    assert all(np.isfinite(eq.lo[r]) and eq.lo[r] < eq.hi[r] < np.inf for r in eq.info["range_rows"])
    assert sorted(c.n for c in mid if c.status == "Infeasible" and "bigbound" not in c.tags) == [40, 40, 300]
    for cases in (mid, dense):
        big = [c for c in cases if "bigbound" in c.tags]
        assert sorted(c.status for c in big) == ["Infeasible", "Optimal"] and all(c.u[0] == 2e7 for c in big)


@pytest.mark.parametrize("solver,case", warm_cases(), ids=lambda v: getattr(v, "name", v))
def test_warm_rows_are_slack_then_cutting(solver, case):
    st, obj, x, _ = highs_solve(case)
    assert st == "Optimal"
    rowptr, col, val, lo, hi = warm_rows(case, x, WARM_SEED)
    ax = np.array([val[rowptr[i]:rowptr[i + 1]] @ x[col[rowptr[i]:rowptr[i + 1]]] for i in range(25)])
    assert np.all(hi[:20] - ax[:20] >= 1.0) and np.all(np.fmax(ax[20:] - hi[20:], lo[20:] - ax[20:]) >= 0.1 - 1e-12)
    assert np.count_nonzero(np.isfinite(lo[20:])) == 2                   # two of the five cuts sit on their row's lower side
    st2, obj2, _, _ = highs_solve(case, (rowptr, col, val, lo, hi))
    assert st2 == "Optimal" and obj2 > obj + 1e-6                        # the cuts bite


# ---- the certificate rejects what is wrong ---------------------------------------------------------------------------------------

def test_certificate_rejects_a_point_moved_along_a_violated_direction():
    case = CASES["mid_n33"]
    _, _, x, y = _highs(case.name)
    i = int(np.argmin(y))                                                  # an active upper side
    assert y[i] < -1e-6
    s = slice(case.rowptr[i], case.rowptr[i + 1])
    a = np.zeros(case.n)
    np.add.at(a, case.col[s], case.val[s])
    cert = _cert(case, x + 1e-6 * a / np.linalg.norm(a), y)
    assert cert.row_viol > 0.9e-6 > ROW_TOL and cert.worst_row == i
    assert any(f.startswith("row %d violated" % i) for f in failures(cert))
    # ... and past a bound
    j = int(np.argmax(np.isfinite(case.u)))
    x2 = x.copy()
    x2[j] = case.u[j] + 1e-6
    cert = _cert(case, x2, y)
    assert cert.bound_viol > BOUND_TOL * max(1.0, abs(case.u[j])) and cert.worst_col == j and failures(cert)


def test_certificate_rejects_a_multiplier_with_its_sign_flipped():
    case = CASES["mid_n33"]
    _, _, x, y = _highs(case.name)
    i = int(np.argmin(y))
    y2 = y.copy()
    y2[i] = -y2[i]                                                          # now points at the absent lower side
    cert = _cert(case, x, y2)
    assert not cert.sign_ok and cert.bad_sign_row == i and failures(cert)
    # a row with both sides: the sign stays legal, the gap does not close
    case = CASES["mid_eq_range"]
    _, _, x, y = _highs(case.name)
    r = case.info["eq_rows"][0]
    assert abs(y[r]) > 1e-6
    y2 = y.copy()
    y2[r] = -y2[r]
    cert = _cert(case, x, y2)
    assert cert.sign_ok and abs(cert.gap) > 1e-7 * max(1.0, abs(cert.pobj)) and failures(cert)


def test_certificate_rejects_the_multipliers_of_a_neighbouring_vertex():
    """min -2 x0 - x1 + x2,  x0 + x1 <= 3,  x0 - x1 <= 1,  0 <= x <= 10.  Vertices (0,0), (1,0), (2,1), (0,3) (x2 = 0).  The
    optimum is (2, 1, 0) with y = (-3/2, -1/2): both rows on their upper side, objective -5 = dual bound, gap exactly 0.  The
    neighbouring vertex (0, 3, 0) -- working set {row 0, x0 >= 0}; what a solver that keeps a perturbed cost could return if
    the perturbation tipped the balance, written down by hand here -- has y = (-1, 0) and the reduced cost -1 on x0, which
    is dual feasible only against the UPPER bound 10: dual bound -13."""
    rowptr, col, val = np.array([0, 2, 4]), np.array([0, 1, 0, 1]), np.array([1.0, 1.0, 1.0, -1.0])
    lo, hi = np.array([-np.inf, -np.inf]), np.array([3.0, 1.0])
    l, u, c = np.zeros(3), np.full(3, 10.0), np.array([-2.0, -1.0, 1.0])
    good = certify((rowptr, col, val), lo, hi, l, u, c, "Min", [2.0, 1.0, 0.0], [-1.5, -0.5])
    assert good.gap == 0.0 and good.row_viol == 0.0 and good.bound_viol == 0.0 and good.sign_ok and good.charge == 0.0
    assert good.pobj == -5.0 and failures(good) == []
    # the same as a Max problem
    gmax = certify((rowptr, col, val), lo, hi, l, u, -c, "Max", [2.0, 1.0, 0.0], [-1.5, -0.5])
    assert gmax.gap == 0.0 and gmax.pobj == -5.0
    for x in ([2.0, 1.0, 0.0], [0.0, 3.0, 0.0]):
        bad = certify((rowptr, col, val), lo, hi, l, u, c, "Min", x, [-1.0, 0.0])
        assert bad.dual_bound == -13.0 and bad.gap == bad.pobj + 13.0 and failures(bad)
    # a free column: the reduced cost that needs the missing bound is charged, not hidden
    lf = np.array([-np.inf, 0.0, 0.0])
    ch = certify((rowptr, col, val), lo, hi, lf, u, c, "Min", [2.0, 1.0, 0.0], [-1.0, -1.0])      # r_0 = -2 + 2 = 0, r_1 = -1: u_1
    assert ch.charge == 0.0
    ch = certify((rowptr, col, val), lo, hi, lf, u, c, "Min", [2.0, 1.0, 0.0], [-2.5, -0.5])      # r_0 = +1 needs l_0 = -inf
    assert ch.charge == 2.0 and ch.worst_rc_col == 0 and failures(ch)


def test_certificate_sums_repeated_columns_and_skips_nan_sides():
    rowptr, col, val = np.array([0, 3, 4]), np.array([0, 1, 0, 1]), np.array([1.0, 1.0, 2.0, 1.0])   # row 0: 3 x0 + x1
    cert = certify((rowptr, col, val), [-np.inf, -np.inf], [5.0, np.nan], [0.0, 0.0], [4.0, 4.0], [-3.0, -1.0], "Min", [1.0, 2.0], [-1.0, 0.0])
    assert cert.row_viol == 0.0 and cert.worst_row == 0 and cert.gap == 0.0                       # r = 0: -5 = -1 * 5
    cert = certify((rowptr, col, val), [-np.inf, -np.inf], [5.0, np.nan], [0.0, 0.0], [4.0, 4.0], [-3.0, -1.0], "Min", [1.0, 2.0], [-1.0, -0.5])
    assert not cert.sign_ok and cert.bad_sign_row == 1
