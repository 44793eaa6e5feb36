"""The seeded case of the KTN_CUT_SUPPORTING_QUAD tests (test code; the reference arithmetic is tests/esh_quad_ref.py).

`case()` is ONE model on n = 600 columns with a point x*, a point x_int and f_tol = quad_ref.F_TOL, rows of the three device-evaluated
kinds interleaved.  Tags of the QUAD rows:

* "part"       convex rows that take part: dense_row with k = 3, 12, 70, banded_row(65, 1) and banded_row(257, 2) (diagonally
               dominant, hence positive definite), a single-entry row, and one dense_row negated with a finite LOWER bound (sigma = -1);
* the fallback classes, each of which keeps Kelley's cut:  "two_sided",  "equality",  "shallow" (its bound leaves x_int less than
  delta = 10 f_tol inside),  "indefinite" (a degree_row, Q without diagonal, signed so that sigma q = d'Qd < 0 along the segment),
  and the epigraph row of the quadratic objective;
* "satisfied"  a convex row that x* does not violate.

Every taking-part row and every fallback row but the shallow one has its bound in the middle, bound = g(x_int) + 1/2 (g(x*) - g(x_int)),
after a linear term t d / |d|^2 on the row's columns (d = x* - x_int) has been added where needed to make sigma (g(x*) - g(x_int)) >= 1:
so phi(0) <= -1/4 and phi(1) >= 1/4 (test_esh_quad_ref.py asserts the margins in mpmath).  SEP rows (convex atoms) are placed the
same way when x* lies outside by 1/2 and are satisfied otherwise; TAPE rows are violated and satisfied in turn."""
import math

import numpy as np

import katana_jl_amd as ktn
import quad_cases as QC
import quad_ref as Q

L = ktn._lib
INF = math.inf
F_TOL = Q.F_TOL
DELTA = 10.0 * F_TOL
TAU = 0.1 * F_TOL                  # esh_root_tol * f_tol
GROUPS = (4, 16, 64, 0)

_CASE = {}


def _g_quad(n, row, x):
    a, T = Q.dense_forms(n, row[1], row[2], row[3], row[4], row[5])
    return float(row[6] + a @ x + 0.5 * x @ T @ x)


def _negated(row):
    return ("quad", row[1], -np.asarray(row[2], dtype=np.float64), row[3], row[4], -np.asarray(row[5], dtype=np.float64), -row[6], False)


def _tilted(n, row, xi, xs, sigma, want=1.0):
    """the row with a linear term added, if needed, so that sigma (g(x*) - g(x_int)) >= want"""
    gap = sigma * (_g_quad(n, row, xs) - _g_quad(n, row, xi))
    if gap >= want:
        return row
    cols = np.unique(np.concatenate([np.asarray(row[1], dtype=np.int64), np.asarray(row[3], dtype=np.int64)]))
    d = xs[cols] - xi[cols]
    add = sigma * (want - gap) * d / float(d @ d)
    return ("quad", np.concatenate([np.asarray(row[1], dtype=np.int64), cols]), np.concatenate([np.asarray(row[2], dtype=np.float64), add]),
            row[3], row[4], row[5], row[6], False)


def case(seed=23):
    if seed in _CASE:
        return _CASE[seed]
    rng = np.random.default_rng(seed)
    n = 600
    xs = rng.uniform(-1.0, 1.0, n)
    xi = rng.uniform(-0.25, 0.25, n)
    indef = QC.degree_row(rng, n, 8)
    if True:                                                                   # sign Q so that d'Qd < 0 along the segment
        _, T = Q.dense_forms(n, indef[1], indef[2], indef[3], indef[4], indef[5])
        d = xs - xi
        if d @ T @ d > 0:
            indef = ("quad", indef[1], indef[2], indef[3], indef[4], -np.asarray(indef[5]), indef[6], False)
    spec = [("part", QC.dense_row(rng, n, 3), 1), ("sep", QC.sep_row(rng, n, 7), 1), ("tape", QC.tape_row(rng, n, 0), 1),
            ("part", ("quad", [17], [0.75], [17], [17], [1.5], -0.25, False), 1),
            ("two_sided", QC.dense_row(rng, n, 5), 1), ("part", QC.dense_row(rng, n, 12), 1), ("sep", QC.sep_row(rng, n, 33), 1),
            ("part", QC.banded_row(rng, n, 65, 1), 1), ("tape", QC.tape_row(rng, n, 1), 1), ("equality", QC.dense_row(rng, n, 4), 1),
            ("part", _negated(QC.dense_row(rng, n, 9)), -1), ("satisfied", QC.dense_row(rng, n, 6), 1),
            ("sep", QC.sep_row(rng, n, 5, linear=True), 1), ("shallow", QC.dense_row(rng, n, 7), 1),
            ("part", QC.banded_row(rng, n, 257, 2), 1), ("sep", QC.sep_row(rng, n, 12), 1), ("indefinite", indef, 1),
            ("tape", QC.tape_row(rng, n, 2), 1), ("part", QC.dense_row(rng, n, 70), 1), ("sep", QC.sep_row(rng, n, 9), 1)]
    rows, tags, sides = [], [], []
    for tag, row, sigma in spec:
        if row[0] == "quad" and tag != "satisfied":
            row = _tilted(n, row, xi, xs, sigma)
        rows.append(row); tags.append(tag); sides.append(sigma)
    om = QC.dense_row(rng, n, 12)
    objective = ("quad", om[1], om[2], om[3], om[4], om[5], 0.125)
    d, layouts = QC.assemble(n, rows, objective)
    C = QC.Case()
    C.n, C.m, C.rows, C.tags, C.sides, C.d, C.layouts, C.objective = n, len(rows), rows, tags, sides, d, layouts, objective
    C.x, C.xi, C.f_tol = xs, xi, F_TOL
    C.kind = np.array([{"sep": L.ROW_SEP, "tape": L.ROW_TAPE, "quad": L.ROW_QUAD}[r[0]] for r in rows])
    # float64 values of every row at the two points (they place the bounds; never a tolerance)
    C.ref = {i: Q.row_ref_mp(*lay, rows[i][6], xs) for i, lay in layouts.items() if i != "obj"}
    gs = QC.row_values_f64(C)
    Ci = QC.Case()
    Ci.rows, Ci.x = rows, xi
    Ci.ref = {i: Q.row_ref_mp(*lay, rows[i][6], xi) for i, lay in layouts.items() if i != "obj"}
    gi = QC.row_values_f64(Ci)
    C.ref_int, C.g_star, C.g_int = Ci.ref, gs, gi
    lb, ub = np.full(C.m, -INF), np.full(C.m, INF)
    ntape = 0
    for i, tag in enumerate(tags):
        mid = gi[i] + 0.5 * (gs[i] - gi[i])
        if tag == "part" and sides[i] < 0:
            lb[i] = mid
        elif tag in ("part", "indefinite"):
            ub[i] = mid
        elif tag == "two_sided":
            lb[i], ub[i] = min(gs[i], gi[i]) - 50.0, mid
        elif tag == "equality":
            lb[i] = ub[i] = mid
        elif tag == "shallow":
            ub[i] = gi[i] + 0.5 * DELTA
        elif tag == "satisfied":
            ub[i] = max(gs[i], gi[i]) + 0.5
        elif tag == "sep":
            if d.row_linear[i]:
                lb[i], ub[i] = gs[i] - 1.0, gs[i] + 1.0
            else:
                ub[i] = mid if gs[i] - gi[i] >= 1.0 else max(gs[i], gi[i]) + 0.5
        else:
            ntape += 1
            ub[i] = gs[i] - 0.5 if ntape % 2 else gs[i] + 0.5
    C.lb, C.ub = lb, ub
    C.violated = ~((gs >= lb - F_TOL) & (gs <= ub + F_TOL))
    # the epigraph row f(x) - t at t = x[n]
    lay = layouts["obj"]
    f64 = float(Q.row_ref_mp(*lay, objective[6], xs).g)
    C.t = math.floor(8.0 * f64) / 8.0 - 0.5                                    # f(x*) - t in [0.5, 0.625): violated (:Min, <= 0)
    C.xt = np.concatenate([xs, [C.t]])
    C.nl = [i for i in range(C.m) if not d.row_linear[i]] + [C.m]
    C.part = [i for i, t in enumerate(tags) if t == "part"]
    C.fallback = [i for i, t in enumerate(tags) if t in ("two_sided", "equality", "shallow", "indefinite")] + [C.m]
    _CASE[seed] = C
    return C


def bound_of(C, i):
    return C.ub[i] if C.sides[i] > 0 else C.lb[i]


# ---- the ellipsoid of quad_cases with radius rho -------------------------------------------------------------------------------
def ellipsoid_rho(n, rho=4.0):
    """quad_cases.ellipsoid(n) with 1/2 (x - x0)'Q(x - x0) <= rho:  f* = c'x0 - sqrt(2 rho c'Q^-1 c); x* stays inside the box for rho = 4"""
    C = QC.ellipsoid(n)
    qic = np.linalg.solve(C.Q, C.c)
    C.rho = rho
    C.fstar = float(C.c @ C.x0 - math.sqrt(2.0 * rho * (C.c @ qic)))
    C.xstar = C.x0 - qic * math.sqrt(2.0 * rho / (C.c @ qic))
    assert np.abs(C.xstar).max() < 10.0
    return C


def ellipsoid_rho_problem(C):
    p = QC.ellipsoid_quad(C)
    return ktn.Problem(C.n, 1, np.full(C.n, -10.0), np.full(C.n, 10.0), [-INF], [C.rho], "Min", p.d)


def ellipsoid_value(C, x):
    x = np.asarray(x, dtype=np.float64)[:C.n]
    return float(0.5 * (x - C.x0) @ C.Q @ (x - C.x0))
