"""Seeded case builders for the KTN_ROW_QUAD tests (test code; the reference arithmetic is tests/quad_ref.py).

`mixed_case()` is ONE model that serves every lane-group setting of k_quad_jac: rows of the three device-evaluated kinds interleaved,
a QUAD row first and last, and among the QUAD rows

* a "degree" row per G in {4, 8, 16, 32, 64}: a symmetric Q without diagonal whose rows have 0, 1, G-1, G, G+1 and 2G+1 entries
  (one hub column joined to 2G+1 leaves, three more hubs joined to the first G-1, G, G+1 of them, one column in the linear part only),
  so whichever G a handle runs, segment lengths 0, 1, G-1, G, G+1, 2G+1 are present;
* a row with a single entry, rows with 65 (tridiagonal Q) and 257 (five-band Q) structure entries, a dense 70-column row
  (4 900 Q entries), a QUAD row with an empty Q declared linear, small dense rows, and -- through a quadratic objective on fewer
  columns than the model has -- a `pad_zero` epigraph row;
* four threshold rows on two dyadic columns (x = 1 and x = 1/2, Q = diag(2, 8): both value terms are exactly 1) with dyadic rconst
  and f_tol = 2^-20, so that g is exact in every summation order: exactly at ub + f_tol, one ulp above it, exactly at lb - f_tol,
  one ulp below it.

Every other NL row gets its bound half a unit (at least) away from its exact g, on the violated or the satisfied side in turn:
10^3 times its value bound is far below that (test_quad_ref.py asserts it), so the violated set is unambiguous.
"""
import math

import numpy as np

import katana_jl_amd as ktn
import quad_ref as Q

L = ktn._lib
INF = math.inf
GROUPS = (4, 8, 16, 32, 64)


class Case:
    pass


def _sym(pairs, vals):
    """full symmetric triplets of the off-diagonal / diagonal pairs (r <= c given once)"""
    qr, qc, qv = [], [], []
    for (r, c), v in zip(pairs, vals):
        qr.append(r); qc.append(c); qv.append(v)
        if r != c:
            qr.append(c); qc.append(r); qv.append(v)
    return qr, qc, qv


def degree_row(rng, n, G):
    S = 5 + 2 * G + 1
    cols = rng.choice(n - 2, size=S, replace=False)              # (the last two columns are the threshold rows')
    pairs = [(0, 5 + j) for j in range(2 * G + 1)]
    for hub, deg in ((1, G - 1), (2, G), (3, G + 1)):
        pairs += [(hub, 5 + j) for j in range(deg)]
    pairs = [(int(cols[r]), int(cols[c])) for r, c in pairs]
    qr, qc, qv = _sym(pairs, rng.uniform(-1.0, 1.0, len(pairs)))
    return ("quad", cols, rng.uniform(-1.0, 1.0, S), qr, qc, qv, float(rng.uniform(-1, 1)), False)


def banded_row(rng, n, S, half_band):
    cols = np.sort(rng.choice(n - 2, size=S, replace=False))
    pairs = [(j, j + d) for d in range(half_band + 1) for j in range(S - d)]
    vals = [(2.0 + half_band if r == c else 0.0) + rng.uniform(-0.5, 0.5) for r, c in pairs]
    qr, qc, qv = _sym([(int(cols[r]), int(cols[c])) for r, c in pairs], vals)
    return ("quad", cols, rng.uniform(-1.0, 1.0, S), qr, qc, qv, float(rng.uniform(-1, 1)), False)


def dense_row(rng, n, k):
    cols = rng.choice(n - 2, size=k, replace=False)
    B = rng.uniform(-1.0, 1.0, (k, k))
    M = B @ B.T / k + np.eye(k)
    M = (M + M.T) / 2
    r, c = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    return ("quad", cols, rng.uniform(-1.0, 1.0, k), cols[r.ravel()], cols[c.ravel()], M.ravel(), float(rng.uniform(-1, 1)), False)


def threshold_row(n, rconst):
    return ("quad", [], [], [n - 2, n - 1], [n - 2, n - 1], [2.0, 8.0], rconst, False)


def sep_row(rng, n, k, linear=False):
    cols = np.sort(rng.choice(n - 2, size=k, replace=False))
    kinds = np.zeros(k, dtype=np.uint8) if linear else rng.choice([L.ATOM_LIN, L.ATOM_QUAD, L.ATOM_EXP], size=k).astype(np.uint8)
    return ("sep", cols, kinds, rng.uniform(0.2, 1.0, k), rng.uniform(-0.5, 0.5, k), float(rng.uniform(-1, 1)), linear)


def tape_row(rng, n, which):
    j = [int(c) for c in rng.choice(n - 2, size=4, replace=False)]
    v = ktn.var
    e = [v(j[0]) * v(j[1]) + ktn.exp(v(j[2]) * 0.5) - 1.5,
         ktn.sqrt(v(j[0]) * v(j[0]) + v(j[3]) * v(j[3]) + 1.0) + v(j[1]) * 0.25,
         ktn.sin(v(j[2])) * v(j[0]) + v(j[1]) * v(j[1]) * 0.75][which]
    return ("tape", e)


def assemble(n, rows, objective):
    """NLPDescription of rows of mixed kinds.  rows: ("sep", cols, kinds, p0, p1, rconst, linear) | ("tape", Expr) |
    ("quad", lin_cols, lin_vals, q_rows, q_cols, q_vals, const, linear).  objective: ("quad", lin_cols, lin_vals, q_rows, q_cols,
    q_vals, const) or ("lin", cols, vals).  Returns (description, layouts) with layouts[i] = the _quad_row tuple of QUAD row i."""
    rowptr, col, akind, p0, p1, rkind, rlin, rconst = [0], [], [], [], [], [], [], []
    tptr, top, targ, qptr, qcol, qval = [0], [], [], [0], [], []
    layouts = {}
    for i, r in enumerate(rows):
        if r[0] == "sep":
            _, c, kd, a, b, c0, lin = r
            col += list(c); akind += list(kd); p0 += list(a); p1 += list(b)
            qptr += [len(qcol)] * len(c)
            rkind.append(L.ROW_SEP); rconst.append(c0); rlin.append(1 if lin else 0)
        elif r[0] == "tape":
            e = r[1]
            vs = list(e.variables())
            col += vs; akind += [0] * len(vs); p0 += [0.0] * len(vs); p1 += [0.0] * len(vs)
            qptr += [len(qcol)] * len(vs)
            o, a = e.tape()
            top += o.tolist(); targ += a.tolist()
            rkind.append(L.ROW_TAPE); rconst.append(0.0); rlin.append(0)
        else:
            _, lc, lv, qr, qc, qv, c0, lin = r
            lay = ktn.nlp._quad_row(n, lc, lv, qr, qc, qv)
            layouts[i] = lay
            cols, a, ptr, sc, sv = lay
            assert not (lin and len(sv))
            col += cols.tolist(); akind += [0] * len(cols); p0 += a.tolist(); p1 += [0.0] * len(cols)
            qptr += (ptr[1:] + len(qcol)).tolist(); qcol += sc.tolist(); qval += sv.tolist()
            rkind.append(L.ROW_QUAD); rconst.append(c0); rlin.append(1 if lin else 0)
        rowptr.append(len(col)); tptr.append(len(top))
    kw = {}
    if objective[0] == "quad":
        _, lc, lv, qr, qc, qv, c0 = objective
        lay = ktn.nlp._quad_row(n, lc, lv, qr, qc, qv)
        layouts["obj"] = lay
        kw = dict(obj_linear=len(lay[4]) == 0, obj_kind=L.ROW_QUAD, obj_col=lay[0], obj_p0=lay[1], obj_const=c0,
                  obj_quad_ptr=lay[2], obj_quad_col=lay[3], obj_quad_val=lay[4])
    else:
        _, c, v = objective
        kw = dict(obj_linear=True, obj_kind=L.ROW_SEP, obj_col=c, obj_atom_kind=np.zeros(len(c)), obj_p0=v, obj_p1=np.zeros(len(c)))
    has_quad = any(r[0] == "quad" for r in rows)
    d = ktn.NLPDescription(n, rowptr, col, rkind, rlin, rconst, akind, p0, p1, tptr, top, targ,
                           quad_ptr=qptr if has_quad else None, quad_col=qcol if has_quad else None,
                           quad_val=qval if has_quad else None, **kw)
    return d, layouts


def quad_as_expr(cols, a, ptr, sc, sv, rconst):
    """the same quadratic as an expression:  rconst + sum_e x_e (a_e + 1/2 sum_k q_k x_k)"""
    e = ktn.const(float(rconst))
    for i, c in enumerate(cols):
        inner = ktn.const(float(a[i]))
        for k in range(int(ptr[i]), int(ptr[i + 1])):
            inner = inner + ktn.var(int(sc[k])) * (0.5 * float(sv[k]))
        e = e + ktn.var(int(c)) * inner
    return e


_MIXED = {}


def mixed_case(seed=11):
    """the model of the module docstring with its mpmath reference at its point x (built once per process)"""
    if seed in _MIXED:
        return _MIXED[seed]
    rng = np.random.default_rng(seed)
    n = 600
    x = rng.uniform(-1.0, 1.0, n)
    x[n - 2], x[n - 1] = 1.0, 0.5
    e51 = 2.0 ** -51
    rows = [degree_row(rng, n, 4), sep_row(rng, n, 7), tape_row(rng, n, 0),
            ("quad", [17], [0.75], [17], [17], [1.5], -0.25, False),                      # a single entry
            degree_row(rng, n, 8), sep_row(rng, n, 5, linear=True), banded_row(rng, n, 65, 1), tape_row(rng, n, 1),
            threshold_row(n, 1.0), threshold_row(n, 1.0 + e51),
            degree_row(rng, n, 16),
            ("quad", rng.choice(n - 2, 9, replace=False), rng.uniform(-1, 1, 9), [], [], [], 0.5, True),   # empty Q, declared linear
            banded_row(rng, n, 257, 2), sep_row(rng, n, 33), degree_row(rng, n, 32),
            threshold_row(n, 1.0), threshold_row(n, 1.0 - e51),
            dense_row(rng, n, 70), tape_row(rng, n, 2), degree_row(rng, n, 64)]
    rows += [dense_row(rng, n, 3) for _ in range(7)]
    om = dense_row(rng, n, 12)
    objective = ("quad", om[1], om[2], om[3], om[4], om[5], 0.125)
    d, layouts = assemble(n, rows, objective)
    C = Case()
    C.n, C.x, C.rows, C.d, C.layouts, C.objective = n, x, rows, d, layouts, objective
    m = len(rows)
    C.m = m
    C.kind = np.array([{"sep": L.ROW_SEP, "tape": L.ROW_TAPE, "quad": L.ROW_QUAD}[r[0]] for r in rows])
    C.ref = {i: Q.row_ref_mp(lay[0], lay[1], lay[2], lay[3], lay[4], rows[i][6], x) for i, lay in layouts.items() if i != "obj"}
    # float64 values of the other rows through the description itself (bounds only need half a unit of room)
    lb, ub = np.full(m, -INF), np.full(m, INF)
    thr = {8: "thr_at_ub", 9: "thr_above_ub", 15: "thr_at_lb", 16: "thr_below_lb"}
    C.tags = [thr.get(i, rows[i][0]) for i in range(m)]
    g64 = row_values_f64(C)
    side = 0
    for i in range(m):
        if i in thr:
            if thr[i].endswith("ub"):
                ub[i] = 3.0 - Q.F_TOL
            else:
                lb[i] = 3.0 + Q.F_TOL
        elif d.row_linear[i]:
            lb[i], ub[i] = g64[i] - 1.0, g64[i] + 1.0
        else:
            side += 1
            margin = 0.5 + 0.25 * (i % 3)
            if side % 4 == 3:
                lb[i] = g64[i] + (margin if side % 8 == 3 else -margin)        # lower side: violated / satisfied
            else:
                ub[i] = g64[i] - margin if side % 2 else g64[i] + margin        # upper side: violated / satisfied
    C.lb, C.ub, C.f_tol = lb, ub, Q.F_TOL
    C.g64 = g64
    C.violated = ~((g64 >= lb - Q.F_TOL) & (g64 <= ub + Q.F_TOL))
    C.violated[[8, 15]] = False                                                       # exactly at the thresholds: satisfied
    C.violated[[9, 16]] = True                                                        # one ulp beyond
    # the epigraph row f(x) - t at t = x[n] (the tests append t)
    lay = layouts["obj"]
    f64 = float(Q.row_ref_mp(lay[0], lay[1], lay[2], lay[3], lay[4], objective[6], x).g)
    C.t = math.floor(8.0 * f64) / 8.0 - 0.5                                           # f(x) - t in [0.5, 0.625): violated (:Min, <= 0)
    C.xt = np.concatenate([x, [C.t]])
    C.obj_ref = Q.row_ref_mp(np.concatenate([lay[0], [n]]), np.concatenate([lay[1], [-1.0]]),
                             np.concatenate([lay[2], [lay[2][-1]]]), lay[3], lay[4], objective[6], C.xt)
    _MIXED[seed] = C
    return C


def row_values_f64(C):
    """float64 g of every row (numpy / math; used to place bounds and to state the violated set, never as a tolerance)"""
    import tape_ref
    g = np.zeros(len(C.rows))
    for i, r in enumerate(C.rows):
        if r[0] == "sep":
            _, c, kd, a, b, c0, _lin = r
            xv = C.x[np.asarray(c)]
            v = np.where(kd == L.ATOM_LIN, a * xv, np.where(kd == L.ATOM_QUAD, a * (xv - b) ** 2, a * np.exp(b * xv)))
            g[i] = v.sum() + c0
        elif r[0] == "tape":
            o, a = r[1].tape()
            g[i] = float(tape_ref.evaluate(o, a, C.x).value_f64)
        else:
            g[i] = float(C.ref[i].g)
    return g


def without_quad(C):
    """the SEP / TAPE rows of the case alone, with a linear objective: (description, row indices in the mixed model, lb, ub)"""
    keep = [i for i, r in enumerate(C.rows) if r[0] != "quad"]
    d, _ = assemble(C.n, [C.rows[i] for i in keep], ("lin", [0, 1], [1.0, -1.0]))
    return d, np.array(keep), C.lb[keep], C.ub[keep]


def as_tapes(C):
    """the case with every QUAD row (and the objective) stated as an expression tape"""
    rows = []
    for i, r in enumerate(C.rows):
        if r[0] == "quad" and not r[7]:
            rows.append(("tape", quad_as_expr(*C.layouts[i], r[6])))
        else:
            rows.append(r)
    d, _ = assemble(C.n, rows, ("lin", [0, 1], [1.0, -1.0]))
    return d, rows


# ---- solves with closed forms -----------------------------------------------------------------------------------------------
def spd(rng, n):
    Uo, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return Uo @ np.diag(np.exp(rng.uniform(0.0, math.log(4.0), n))) @ Uo.T


def _full(M):
    n = len(M)
    r, c = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return r.ravel(), c.ravel(), ((M + M.T) / 2).ravel()


def ellipsoid(n, seed=None):
    """min c'x  s.t.  1/2 (x - x0)'Q(x - x0) <= 1,  -10 <= x <= 10:  f* = c'x0 - sqrt(2 c'Q^-1 c),  x* = x0 - Q^-1 c sqrt(2 / c'Q^-1 c)"""
    rng = np.random.default_rng(n if seed is None else seed)
    Qm = spd(rng, n)
    Qm = (Qm + Qm.T) / 2
    x0 = rng.uniform(-1.0, 1.0, n)
    c = rng.uniform(-1.0, 1.0, n)
    qic = np.linalg.solve(Qm, c)
    C = Case()
    C.n, C.Q, C.x0, C.c = n, Qm, x0, c
    C.fstar = float(c @ x0 - math.sqrt(2.0 * (c @ qic)))
    C.xstar = x0 - qic * math.sqrt(2.0 / (c @ qic))
    # 1/2 x'Qx - (Q x0)'x + 1/2 x0'Q x0 <= 1
    C.lin = -(Qm @ x0)
    C.const = 0.5 * float(x0 @ Qm @ x0)
    return C


def ellipsoid_quad(C):
    r, c, v = _full(C.Q)
    d = ktn.QuadNLP(C.n, C.c, 0.0, None, [(np.arange(C.n), C.lin, r, c, v, C.const)])
    return ktn.Problem(C.n, 1, np.full(C.n, -10.0), np.full(C.n, 10.0), [-INF], [1.0], "Min", d)


def ellipsoid_tape(C):
    x = [ktn.var(j) for j in range(C.n)]
    e = ktn.const(C.const)
    for i in range(C.n):
        inner = ktn.const(float(C.lin[i]))
        for j in range(C.n):
            inner = inner + x[j] * (0.5 * float(C.Q[i, j]))
        e = e + x[i] * inner
    obj = ktn.const(0.0)
    for j in range(C.n):
        obj = obj + x[j] * float(C.c[j])
    d = ktn.ExprNLP(C.n, obj, [e])
    return ktn.Problem(C.n, 1, np.full(C.n, -10.0), np.full(C.n, 10.0), [-INF], [1.0], "Min", d)


def qp(n):
    """min 1/2 x'Qx + c'x,  -10 <= x <= 10:  f* = -1/2 c'Q^-1 c  at  x* = -Q^-1 c"""
    rng = np.random.default_rng(100 + n)
    Qm = spd(rng, n)
    Qm = (Qm + Qm.T) / 2
    c = rng.uniform(-1.0, 1.0, n)
    C = Case()
    C.n, C.Q, C.c = n, Qm, c
    qic = np.linalg.solve(Qm, c)
    C.fstar = float(-0.5 * (c @ qic))
    C.xstar = -qic
    return C


def qp_quad(C):
    d = ktn.QuadNLP(C.n, C.c, 0.0, _full(C.Q), [])
    return ktn.Problem(C.n, 0, np.full(C.n, -10.0), np.full(C.n, 10.0), [], [], "Min", d)


def qp_tape(C):
    x = [ktn.var(j) for j in range(C.n)]
    e = ktn.const(0.0)
    for i in range(C.n):
        inner = ktn.const(float(C.c[i]))
        for j in range(C.n):
            inner = inner + x[j] * (0.5 * float(C.Q[i, j]))
        e = e + x[i] * inner
    d = ktn.ExprNLP(C.n, e, [])
    return ktn.Problem(C.n, 0, np.full(C.n, -10.0), np.full(C.n, 10.0), [], [], "Min", d)
