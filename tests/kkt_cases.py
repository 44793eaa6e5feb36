"""Closed-form cases of the NLP-level report (test code): small convex problems whose KKT point is known, each stated once as a
SeparableInstance and built in every row kind from that one statement -- SEP atoms, TAPE rows (the expressions of
helpers.instance_as_expressions), KTN_ROW_QUAD rows (the atoms expanded: a (x - b)^2 = 1/2 (2a) x^2 - 2ab x + a b^2) and HOST
rows (the oracle's evaluator behind CallbackNLP).

    (a) min -sum x_i            s.t. sum x_i^2 <= 1,  box +-2          lambda = sqrt(n) / 2, z = 0
    (b) as (a) with u_1 = 0.1                                          a bound is active, z_1 < 0
    (c) as (a) plus the linear row x_1 + x_2 <= 0.3                    a linear multiplier is active
    (d) as (a) written as -1 <= -sum x_i^2                             the lower side is active, d > 0
    (e) min sum (x_i - 1)^2     s.t. sum x_i <= 1                      a nonlinear objective: the epigraph row
    (f) max  sum x_i            s.t. sum x_i^2 <= 1                    the Max mirror of (a)

`solve(case)` refines the closed-form guess by Newton's method on the KKT system in mpmath (50 digits; the residual is checked
by tests/test_kkt_ref.py) and returns (x, d, z) as mpf lists; `Case.xs, ds, zs` are their float64 roundings.
"""
import numpy as np
from mpmath import mp, mpf
import mpmath

from katana_jl_amd.instances import SeparableInstance, ATOM_LIN, ATOM_QUAD

DPS = 50
NS = (4, 8)
NAMES = ("a", "b", "c", "d", "e", "f")
KINDS = ("sep", "tape", "quad")


class Case:
    pass


def _inst(n, sense, l, u, rows, obj, obj_const=0.0):
    """rows: [(atoms [(col, kind, p0, p1)], rconst, lb, ub)], linear rows first; obj: atoms"""
    rowptr, col, kind, p0, p1, rconst, lb, ub = [0], [], [], [], [], [], [], []
    m_lin = 0
    for atoms, rc, lo, hi in rows:
        for c, k, a, b in atoms:
            col.append(c); kind.append(k); p0.append(a); p1.append(b)
        rowptr.append(len(col)); rconst.append(rc); lb.append(lo); ub.append(hi)
        if all(k == ATOM_LIN for _, k, _, _ in atoms):
            m_lin += 1
    f = np.float64
    return SeparableInstance(
        n=n, l_var=np.asarray(l, dtype=f), u_var=np.asarray(u, dtype=f), sense=sense,
        rowptr=np.asarray(rowptr, dtype=np.int64), col=np.asarray(col, dtype=np.int32), kind=np.asarray(kind, dtype=np.uint8),
        p0=np.asarray(p0, dtype=f), p1=np.asarray(p1, dtype=f), rconst=np.asarray(rconst, dtype=f),
        l_constr=np.asarray(lb, dtype=f), u_constr=np.asarray(ub, dtype=f),
        obj_col=np.asarray([c for c, _, _, _ in obj], dtype=np.int32), obj_kind=np.asarray([k for _, k, _, _ in obj], dtype=np.uint8),
        obj_p0=np.asarray([a for _, _, a, _ in obj], dtype=f), obj_p1=np.asarray([b for _, _, _, b in obj], dtype=f),
        obj_const=float(obj_const), xhat=np.zeros(n), opt_obj=0.0, m_lin=m_lin, m_nl=len(rows) - m_lin)


def make(name, n):
    """the case's instance, its active set and the closed-form starting guess of the Newton refinement"""
    inf = np.inf
    l, u = [-2.0] * n, [2.0] * n
    ball = [(j, ATOM_QUAD, 1.0, 0.0) for j in range(n)]
    C = Case()
    C.name, C.n = name, n
    C.pinned = {}
    s = 1.0 / np.sqrt(n)
    if name in ("a", "f"):
        sense = "Max" if name == "f" else "Min"
        sg = -1.0 if name == "f" else 1.0
        C.inst = _inst(n, sense, l, u, [(ball, -1.0, -inf, 0.0)], [(j, ATOM_LIN, -sg, 0.0) for j in range(n)])
        C.active = {0: "ub"}
        C.x0, C.d0 = [s] * n, {0: -sg * np.sqrt(n) / 2}
    elif name == "b":
        u[0] = 0.1
        C.inst = _inst(n, "Min", l, u, [(ball, -1.0, -inf, 0.0)], [(j, ATOM_LIN, -1.0, 0.0) for j in range(n)])
        C.active, C.pinned = {0: "ub"}, {0: 0.1}
        b = np.sqrt((1 - 0.01) / (n - 1))
        C.x0, C.d0 = [0.1] + [b] * (n - 1), {0: -1 / (2 * b)}
    elif name == "c":
        lin = [(0, ATOM_LIN, 1.0, 0.0), (1, ATOM_LIN, 1.0, 0.0)]
        C.inst = _inst(n, "Min", l, u, [(lin, 0.0, -inf, 0.3), (ball, -1.0, -inf, 0.0)], [(j, ATOM_LIN, -1.0, 0.0) for j in range(n)])
        C.active = {0: "ub", 1: "ub"}
        a = 0.15
        b = np.sqrt((1 - 2 * a * a) / (n - 2))
        C.x0, C.d0 = [a, a] + [b] * (n - 2), {0: -(1 - a / b), 1: -1 / (2 * b)}
    elif name == "d":
        C.inst = _inst(n, "Min", l, u, [([(j, ATOM_QUAD, -1.0, 0.0) for j in range(n)], 0.0, -1.0, inf)],
                       [(j, ATOM_LIN, -1.0, 0.0) for j in range(n)])
        C.active = {0: "lb"}
        C.x0, C.d0 = [s] * n, {0: np.sqrt(n) / 2}
    elif name == "e":
        C.inst = _inst(n, "Min", l, u, [([(j, ATOM_LIN, 1.0, 0.0) for j in range(n)], 0.0, -inf, 1.0)],
                       [(j, ATOM_QUAD, 1.0, 1.0) for j in range(n)])
        C.active = {0: "ub"}
        C.x0, C.d0 = [1.0 / n] * n, {0: -2 * (1 - 1.0 / n)}
    else:
        raise ValueError(name)
    return C


def _atom(kind, a, b, x):
    return (a * x, a) if kind == ATOM_LIN else (a * (x - b) ** 2, 2 * a * (x - b))


def lagrangian_parts(inst, X, D):
    """(f, g list, z list) in the arithmetic of X and D (mpf or float): z = grad f - J'D"""
    n, m = inst.n, inst.num_constr
    z = [0 * X[0]] * n
    f = inst.obj_const + 0 * X[0]
    for c, k, a, b in zip(inst.obj_col, inst.obj_kind, inst.obj_p0, inst.obj_p1):
        v, dv = _atom(int(k), mpf(float(a)), mpf(float(b)), X[int(c)])
        f += v; z[int(c)] += dv
    g = []
    for i in range(m):
        gi = mpf(float(inst.rconst[i]))
        for e in range(int(inst.rowptr[i]), int(inst.rowptr[i + 1])):
            c = int(inst.col[e])
            v, dv = _atom(int(inst.kind[e]), mpf(float(inst.p0[e])), mpf(float(inst.p1[e])), X[c])
            gi += v; z[c] -= D[i] * dv
        g.append(gi)
    return f, g, z


def solve(C):
    """Newton on the KKT system with the case's active set: unknowns the free x_j and the active rows' d_i; equations z_j = 0 for
    the free j and g_i = its active bound.  Returns (x, d, z) as mpf lists."""
    inst, n, m = C.inst, C.n, C.inst.num_constr
    free = [j for j in range(n) if j not in C.pinned]
    act = sorted(C.active)
    with mp.workdps(DPS):
        def unpack(v):
            X = [mpf(0)] * n
            for j, val in C.pinned.items():
                X[j] = mpf(float(val))                           # the double the engine is given as the bound
            for t, j in enumerate(free):
                X[j] = v[t]
            D = [mpf(0)] * m
            for t, i in enumerate(act):
                D[i] = v[len(free) + t]
            return X, D

        def F(*v):
            X, D = unpack(v)
            _, g, z = lagrangian_parts(inst, X, D)
            bound = lambda i: mpf(float(inst.u_constr[i] if C.active[i] == "ub" else inst.l_constr[i]))
            return [z[j] for j in free] + [g[i] - bound(i) for i in act]

        v0 = [mpf(float(C.x0[j])) for j in free] + [mpf(float(C.d0[i])) for i in act]
        v = mpmath.findroot(F, v0, tol=mpf(10) ** (-2 * DPS + 10), maxsteps=50)
        X, D = unpack(list(v))
        _, _, z = lagrangian_parts(inst, X, D)
    return X, D, z


def build(name, n):
    """the case with its solution: C.xm, C.dm, C.zm (mpf), C.xs, C.ds, C.zs (float64), C.fstar"""
    C = make(name, n)
    C.xm, C.dm, C.zm = solve(C)
    C.xs = np.asarray([float(v) for v in C.xm]); C.ds = np.asarray([float(v) for v in C.dm]); C.zs = np.asarray([float(v) for v in C.zm])
    with mp.workdps(DPS):
        C.fstar = float(lagrangian_parts(C.inst, C.xm, C.dm)[0])
    return C


def quad_description(ktn, inst):
    """the instance in KTN_ROW_QUAD rows (nlp.QuadNLP): every atom expanded, Q diagonal"""
    def expand(cols, kinds, p0, p1):
        lc, lv, qr, qv, c0 = [], [], [], [], 0.0
        for c, k, a, b in zip(cols, kinds, p0, p1):
            c, a, b = int(c), float(a), float(b)
            if int(k) == ATOM_LIN:
                lc.append(c); lv.append(a)
            else:
                qr.append(c); qv.append(2.0 * a)
                if b != 0.0:
                    lc.append(c); lv.append(-2.0 * a * b); c0 += a * b * b
        return lc, lv, qr, qv, c0
    rows = []
    for i in range(inst.num_constr):
        s = slice(int(inst.rowptr[i]), int(inst.rowptr[i + 1]))
        lc, lv, qr, qv, c0 = expand(inst.col[s], inst.kind[s], inst.p0[s], inst.p1[s])
        rows.append((lc, lv, qr, qr, qv, c0 + float(inst.rconst[i])))
    lc, lv, qr, qv, c0 = expand(inst.obj_col, inst.obj_kind, inst.obj_p0, inst.obj_p1)
    return ktn.nlp.QuadNLP(inst.n, (lc, lv), c0 + float(inst.obj_const), (qr, qr, qv) if qr else None, rows)


def description(ktn, inst, kind):
    """the NLPDescription of the instance in row kind "sep", "tape", "quad" or "host" """
    if kind == "sep":
        return ktn.SeparableNLP(inst)
    if kind == "tape":
        from helpers import instance_as_expressions
        obj, cons = instance_as_expressions(ktn, inst)
        return ktn.nlp.ExprNLP(inst.n, obj, cons)
    if kind == "quad":
        return quad_description(ktn, inst)
    if kind == "host":
        from helpers import oracle_evaluator
        return ktn.nlp.CallbackNLP(oracle_evaluator(inst), inst.n, inst.num_constr)
    raise ValueError(kind)


def load(ktn, inst, kind, **solver_kw):
    m = ktn.NonlinearModel(ktn.KatanaSolver(**dict(dict(log_level=0), **solver_kw)))
    m.loadproblem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr, inst.u_constr, inst.sense, description(ktn, inst, kind))
    return m
