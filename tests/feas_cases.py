"""Seeded cases of the feasible-point search (test code; csrc/feas.hpp, tests/feas_ref.py).  Every case is a SimpleNamespace with

    p         ktn.Problem (the arguments of loadproblem!), p.d its NLPDescription
    xi, xs    the reference point and x* (num_var entries each); both inside [l, u]
    sig       sigma per row (feas_ref.sides), bnd the bound of that side
    search    rows meant to be searched (phi(1) > 0) and to converge; onepass: rows with phi(1) < 0
    loose     rows for which convergence is NOT asserted (the row at the edge of a domain, the rows of the fallback models)

tests/test_feas_ref.py asserts on the CPU that the cases say what they are meant to say; the device tests only run them."""
import math
from types import SimpleNamespace

import numpy as np

import feas_ref as FR
import katana_jl_amd as ktn
import tape_class_cases as TC

L = ktn._lib
INF = math.inf
F_TOL = 1e-6
TAU = 0.1 * F_TOL                  # esh_root_tol * f_tol
ITERS = 20                         # esh_root_iters
GROUPS = (4, 8, 16, 32, 64)
K_LONG = 8192                      # kLongEval of csrc/kernels.hpp: rows beyond it go to k_feas_long
LIN, QUAD, EXP, NEGLOG = 0, 1, 2, 3


def _finish(d, l, u, lb, ub, xi, xs, sense="Min", loose=()):
    C = SimpleNamespace()
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    C.p = ktn.Problem(d.num_var, d.num_constr, np.asarray(l, dtype=np.float64), np.asarray(u, dtype=np.float64), lb, ub, sense, d)
    C.d, C.xi, C.xs = d, np.asarray(xi, dtype=np.float64), np.asarray(xs, dtype=np.float64)
    C.sig = FR.sides(d, lb, ub)
    C.bnd = np.where(C.sig > 0, ub, lb)
    C.part = [int(i) for i in np.flatnonzero(C.sig)]
    C.loose = set(loose)
    C.search, C.onepass = [], []
    return C


def classify(C):
    """fills C.search / C.onepass from the exact phi(1) (mpmath): done once, by the CPU test and by the device tests' fixtures"""
    for i in C.part:
        try:
            f1 = FR.phi_exact(C.d, i, C.xi, C.xs, C.sig[i], C.bnd[i], 1.0)[0]
            fin = math.isfinite(float(f1))
        except FR.NONFINITE:
            f1, fin = INF, False
        (C.onepass if fin and f1 <= 0 else C.search).append(i)
    return C


# ---- separable rows --------------------------------------------------------------------------------------------------------------
def _sep_atoms(rng, cols, side, xi):
    """convex (side +1) / concave (side -1) atoms that grow along the segment: QUAD centred below x_in, EXP with a positive rate, LIN
    with a positive slope, NEGLOG (which falls) kept small"""
    kinds, p0, p1 = [], [], []
    for e, c in enumerate(cols):
        k = (QUAD, EXP, NEGLOG, LIN)[e % 4]
        a, b = {QUAD: (rng.uniform(0.5, 2.0), xi[c] - rng.uniform(0.0, 0.3)), EXP: (rng.uniform(0.5, 1.5), rng.uniform(0.3, 1.0)),
                NEGLOG: (rng.uniform(0.02, 0.05), rng.uniform(0.5, 1.5)), LIN: (rng.uniform(0.2, 1.0), 0.0)}[k]
        kinds.append(k); p0.append(side * a); p1.append(b)
    return kinds, p0, p1


def sep_case(G, seed=5):
    """rows of 1, G - 1, G, G + 1 and 2 G + 1 entries, all four atom kinds, both sides; a searched row and a one-pass row alternate,
    so that a wavefront holds both; one row whose NEGLOG atom leaves its domain exactly at x* (phi(1) = +inf); two linear rows, one
    of them violated by design (info[4])"""
    rng = np.random.default_rng(seed + G)
    n = 2 * G + 4
    xi, xs = rng.uniform(0.05, 0.3, n), rng.uniform(0.5, 1.0, n)
    cinf = n - 1
    xi[cinf], xs[cinf] = 0.6, 0.2                                   # the domain-edge column: x* + p1 = 0 with p1 = -0.2
    rows = []
    for ln in (1, G - 1, G, G + 1, 2 * G + 1):
        for side in (1, -1):
            for want in ("search", "onepass"):
                cols = np.sort(rng.choice(n - 1, ln, replace=False))
                kinds, p0, p1 = _sep_atoms(rng, cols, side, xi)
                row = FR.esh_ref.SepRow(cols, kinds, p0, p1, 0.0)
                g0, g1 = row.eval(xi)[0], row.eval(xs)[0]
                delta = side * (g1 - g0)
                assert delta > 0.05, (ln, side, delta)
                b = g0 + rng.uniform(0.3, 0.7) * (g1 - g0) if want == "search" else g1 + side * 0.25 * delta
                rows.append((cols, kinds, p0, p1, 0.0, b, side, False))
    # phi(1) = +inf: -log(x - 0.2) on the edge column next to a QUAD atom
    cols, kinds, p0, p1 = [0, cinf], [QUAD, NEGLOG], [1.0, 1.0], [0.0, -0.2]
    g0 = FR.esh_ref.SepRow(cols, kinds, p0, p1, 0.0).eval(xi)[0]
    inf_row = len(rows)
    rows.append((cols, kinds, p0, p1, 0.0, g0 + 1.0, 1, False))
    # linear rows: sum x <= (a bound both ends violate by about 0.5), and one both ends satisfy
    s0, s1 = float(np.sum(xi[:4])), float(np.sum(xs[:4]))
    rows.append((np.arange(4), [LIN] * 4, [1.0] * 4, [0.0] * 4, 0.0, min(s0, s1) - 0.5, 1, True))
    rows.append((np.arange(4), [LIN] * 4, [1.0] * 4, [0.0] * 4, 0.0, max(s0, s1) + 1.0, 1, True))
    return _sep_desc(n, rows, xi, xs, loose=(inf_row,))


def _sep_desc(n, rows, xi, xs, loose=(), l=None, u=None):
    rp, col, kind, p0, p1, rc, lb, ub, lin = [0], [], [], [], [], [], [], [], []
    for cols, kinds, a, b, c0, bound, side, is_lin in rows:
        col.extend(int(c) for c in cols); kind.extend(kinds); p0.extend(a); p1.extend(b)
        rp.append(len(col)); rc.append(c0); lin.append(1 if is_lin else 0)
        lb.append(-INF if side > 0 else bound); ub.append(bound if side > 0 else INF)
    m = len(rows)
    d = ktn.NLPDescription(n, rp, col, np.zeros(m, dtype=np.uint8), lin, rc, kind, p0, p1, obj_linear=True, obj_col=np.arange(n),
                           obj_atom_kind=np.zeros(n), obj_p0=-np.ones(n), obj_p1=np.zeros(n), obj_const=0.5)
    return _finish(d, np.full(n, -2.0) if l is None else l, np.full(n, 2.0) if u is None else u, lb, ub, xi, xs, loose=loose)


def long_case(seed=9):
    """one row of kLongEval + 1 QUAD atoms (k_feas_long) next to two short rows"""
    rng = np.random.default_rng(seed)
    n = K_LONG + 1
    xi, xs = rng.uniform(0.0, 0.1, n), rng.uniform(0.5, 1.0, n)
    rows = []
    for ln in (n, 3, 5):
        cols = np.arange(n) if ln == n else np.sort(rng.choice(n, ln, replace=False))
        a = rng.uniform(0.5, 2.0, ln) / ln
        row = FR.esh_ref.SepRow(cols, [QUAD] * ln, list(a), [0.0] * ln, 0.0)
        g0, g1 = row.eval(xi)[0], row.eval(xs)[0]
        rows.append((cols, [QUAD] * ln, list(a), [0.0] * ln, 0.0, g0 + (0.4 if ln == n else 0.7) * (g1 - g0), 1, False))
    return _sep_desc(n, rows, xi, xs)


# ---- the reduction: m_nl rows of one entry each ------------------------------------------------------------------------------------
REDUCE_SIZES = (1, 255, 256, 257, 65537)


def reduce_case(m_nl, where, tie=False):
    """row i: x_c^2 <= b_i on column c = i mod n; x_in = 0, x* = 1, so lambda_i = sqrt(b_i) (1 for b_i = 4).  The blocking row
    (b = 1/4) sits first, in the middle or last; with `tie` a second row on the same column has the same bound: equal bits, and the
    smaller index wins."""
    n = min(m_nl, 64)
    pos = {"first": 0, "middle": m_nl // 2, "last": m_nl - 1}[where]
    col = np.arange(m_nl) % n
    b = np.full(m_nl, 4.0)
    b[pos] = 0.25
    C = SimpleNamespace(m_nl=m_nl, blocking=pos)
    if tie and m_nl > n:
        other = pos + n if pos + n < m_nl else pos - n
        b[other] = 0.25
        C.blocking = min(pos, other)
    d = ktn.NLPDescription(n, np.arange(m_nl + 1), col, np.zeros(m_nl, dtype=np.uint8), np.zeros(m_nl, dtype=np.uint8), np.zeros(m_nl),
                           np.full(m_nl, QUAD, dtype=np.uint8), np.ones(m_nl), np.zeros(m_nl), obj_linear=True, obj_col=np.arange(n),
                           obj_atom_kind=np.zeros(n), obj_p0=-np.ones(n), obj_p1=np.zeros(n))
    C.p = ktn.Problem(n, m_nl, np.full(n, -2.0), np.full(n, 2.0), np.full(m_nl, -INF), b, "Min", d)
    C.d, C.xi, C.xs, C.b = d, np.zeros(n), np.ones(n), b
    return C


# ---- tape rows ---------------------------------------------------------------------------------------------------------------------
def tape_case(nrows, seed=3):
    """nrows tape rows (1 and 65: one lane, and a second wavefront) of the shapes of tests/tape_class_cases.py, all `<=` rows"""
    rng = np.random.default_rng(seed + nrows)
    n = 12
    shapes = (TC.CONE, TC.QUAD3, TC.EXPO)
    cols = TC.distinct_columns(rng, nrows, n)
    groups = [dict(rows=np.arange(k, nrows, 3), cols=cols[k::3], shape=shapes[k]) for k in range(3) if len(np.arange(k, nrows, 3))]
    d = TC.assemble(n, nrows, groups)
    xi, xs = rng.uniform(0.1, 0.3, n), rng.uniform(0.5, 1.0, n)
    ub = np.zeros(nrows)
    for g in groups:
        g0, g1 = g["shape"].f64(xi[g["cols"]])[0], g["shape"].f64(xs[g["cols"]])[0]
        for r, a, b in zip(g["rows"], g0, g1):
            ub[r] = a + rng.uniform(0.3, 0.7) * (b - a) if b - a > 0.05 and r % 2 == 0 else max(a, b) + 0.25
    return _finish(d, np.full(n, -2.0), np.full(n, 2.0), np.full(nrows, -INF), ub, xi, xs)


# ---- KTN_ROW_QUAD rows --------------------------------------------------------------------------------------------------------------
def quad_case(seed=17):
    """row 0: a dense SPD Q on 5 columns with a linear part; row 1: Q on columns 0, 1 and a linear term on column 5, whose Jacobian
    entry has an EMPTY segment; row 2: the concave mirror of row 0 as a `>=` row; row 3: satisfied at x* (one pass)"""
    rng = np.random.default_rng(seed)
    n = 6
    A = rng.normal(size=(5, 5))
    Q = A @ A.T + 5.0 * np.eye(5)
    qr, qc = np.nonzero(np.ones((5, 5)))
    a = rng.uniform(-0.5, 0.5, 5)
    xi, xs = rng.uniform(-0.1, 0.1, n), rng.uniform(0.4, 0.9, n)

    def g(x, s=1.0):
        return s * float(a @ x[:5] + 0.5 * x[:5] @ Q @ x[:5])

    def g1(x):
        return float(x[0] ** 2 + x[1] ** 2 + 0.5 * x[5])
    rows = [(np.arange(5), a, qr, qc, Q[qr, qc], 0.0), ([5], [0.5], [0, 1], [0, 1], [2.0, 2.0], 0.0),
            (np.arange(5), -a, qr, qc, -Q[qr, qc], 0.0), (np.arange(5), a, qr, qc, Q[qr, qc], 0.0)]
    mix = lambda f, t: f(xi) + t * (f(xs) - f(xi))
    lb = [-INF, -INF, mix(lambda x: g(x, -1.0), 0.6), -INF]
    ub = [mix(g, 0.5), mix(g1, 0.4), INF, g(xs) + 1.0]
    d = ktn.nlp.QuadNLP(n, -np.ones(n), 0.25, None, rows)
    return _finish(d, np.full(n, -2.0), np.full(n, 2.0), lb, ub, xi, xs)


def quad_fallback_case(which):
    """one-row models whose closed form fails, so that the row runs the search on its three coefficients:
    "edge"       x_0^2 + x_1^2 <= 1, x_in = (1, 0) ON the boundary, x* = (1, 1): phi(lam) = lam^2, the discriminant is -2 tau < 0 and
                 only lam = 0 is feasible -- the row ends unconverged at lambda = 0 and x_feas = x_in
    "indefinite" 1.8 x - x^2 <= 0.7 on [x_in, x*] = [0, 1]: phi'(1) < 0, so the closed form's sigma P1 > 0 fails; phi <= 0 on
                 [0, 0.5683...] and the search converges there"""
    if which == "edge":
        d = ktn.nlp.QuadNLP(2, -np.ones(2), 0.0, None, [([], [], [0, 1], [0, 1], [2.0, 2.0], 0.0)])
        return _finish(d, [-2.0] * 2, [2.0] * 2, [-INF], [1.0], [1.0, 0.0], [1.0, 1.0], loose=(0,))
    d = ktn.nlp.QuadNLP(1, -np.ones(1), 0.0, None, [([0], [1.8], [0], [0], [-2.0], 0.0)])
    return _finish(d, [-2.0], [2.0], [-INF], [0.7], [0.0], [1.0])


# ---- found codes and refused paths: minimal models -----------------------------------------------------------------------------------
def ball(n=2, lb=-INF, ub=1.0, u=2.0, kind=QUAD, p1=0.0):
    """sum_j atom(x_j) in [lb, ub] over n columns, min -sum x, box [-2, u]"""
    rows = [(np.arange(n), [kind] * n, [1.0] * n, [p1] * n, 0.0, ub, 1, False)]
    C = _sep_desc(n, rows, np.zeros(n), np.full(n, 0.9), u=np.full(n, u))
    if math.isfinite(lb):
        C.p = C.p._replace(l_constr=np.asarray([lb]))
    return C
