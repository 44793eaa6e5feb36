"""Models for tests/test_gpu_tape_classes.py: big tape models built VECTORISED (one template tape per shape, tiled with numpy,
VAR / CONST arguments overwritten), the float64 formulas of their shapes, and the edge-row sets of tests/test_gpu_tapes.py
(sections "every opcode and its edges" and "repeated / unsorted / duplicated columns") restated so that they can be replicated
over fresh variables."""
import math
from types import SimpleNamespace

import numpy as np

import katana_jl_amd as ktn

L = ktn._lib
INF = math.inf
OPNAME = {L.OP_CONST: "CONST", L.OP_VAR: "VAR", L.OP_ADD: "ADD", L.OP_SUB: "SUB", L.OP_MUL: "MUL", L.OP_DIV: "DIV",
          L.OP_NEG: "NEG", L.OP_POWC: "POWC", L.OP_EXP: "EXP", L.OP_LOG: "LOG", L.OP_SQRT: "SQRT", L.OP_SIN: "SIN",
          L.OP_COS: "COS"}


class Shape:
    """one row shape over nv variables: the template tape of expr(v_0 .. v_{nv-1}); structure = (v_0 .. v_{nv-1}) in that order"""

    def __init__(self, name, nv, expr, f64):
        self.name, self.nv, self.f64 = name, nv, f64
        e = ktn.Expr.wrap(expr([ktn.var(k) for k in range(nv)]))
        ops, args = e.tape()
        self.ops, self.args = np.asarray(ops, dtype=np.int32), np.asarray(args, dtype=np.float64)
        self.var_pos = np.flatnonzero(self.ops == L.OP_VAR)
        self.var_ord = self.args[self.var_pos].astype(np.int64)

    def names(self):
        return " ".join(OPNAME[int(o)] for o in self.ops)


def _cone_f64(x):
    a, b, c = x[:, 0], x[:, 1], x[:, 2]
    sq = a ** 2 + b ** 2
    r = np.sqrt(sq)
    t = c - 0.25
    w = 0.5 / r                                                       # the reverse sweep's order: adjoint times partial
    return r - t, np.abs(r) + np.abs(c) + 0.25, np.stack([w * (2.0 * a), w * (2.0 * b), np.full(len(a), -1.0)], axis=1)


def _quad3_f64(x):
    a, b, c = x[:, 0], x[:, 1], x[:, 2]
    return ((a ** 2 + b ** 2) + c) - 1.0, a ** 2 + b ** 2 + np.abs(c) + 1.0, np.stack([2.0 * a, 2.0 * b, np.ones(len(a))], axis=1)


def _expo_f64(x):
    a, b, c = x[:, 0], x[:, 1], x[:, 2]
    ea, eb = np.exp(a), np.exp(0.5 * b)
    return (ea + eb) - c, ea + eb + np.abs(c), np.stack([ea, eb * 0.5, np.full(len(a), -1.0)], axis=1)


CONE = Shape("cone", 3, lambda v: ktn.sqrt(v[0] ** 2 + v[1] ** 2) - (v[2] - 0.25), _cone_f64)
QUAD3 = Shape("quad3", 3, lambda v: v[0] ** 2 + v[1] ** 2 + v[2] - 1.0, _quad3_f64)
EXPO = Shape("expo", 3, lambda v: ktn.exp(v[0]) + ktn.exp(0.5 * v[1]) - v[2], _expo_f64)
CONE_NODES = "VAR POWC VAR POWC ADD SQRT VAR CONST SUB SUB"


def distinct_columns(rng, m, n, nv=3):
    """(m, nv) random columns of range(n), distinct within a row"""
    cols = rng.integers(0, n, (m, nv))
    for k in range(1, nv):
        while True:
            bad = np.flatnonzero((cols[:, k:k + 1] == cols[:, :k]).any(axis=1))
            if not len(bad):
                break
            cols[bad, k] = rng.integers(0, n, len(bad))
    return cols


def assemble(n, m, groups):
    """NLPDescription of m rows from `groups`: dicts with rows (ascending row ids), cols ((len(rows), nv), the structure) and
    either shape (a Shape: tape rows) or coef ((len(rows), nv): separable LIN rows, declared linear).  Linear objective x_0."""
    slen, tlen = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
    for g in groups:
        slen[g["rows"]] = g["cols"].shape[1]
        tlen[g["rows"]] = len(g["shape"].ops) if "shape" in g else 0
    rp, tp = np.concatenate([[0], np.cumsum(slen)]), np.concatenate([[0], np.cumsum(tlen)])
    col, p0 = np.zeros(rp[-1], dtype=np.int32), np.zeros(rp[-1])
    ops, args = np.zeros(tp[-1], dtype=np.int32), np.zeros(tp[-1])
    kind, lin = np.zeros(m, dtype=np.uint8), np.zeros(m, dtype=np.uint8)
    for g in groups:
        rows, cols = g["rows"], g["cols"]
        col[rp[rows][:, None] + np.arange(cols.shape[1])] = cols
        if "shape" in g:
            s = g["shape"]
            at = tp[rows][:, None] + np.arange(len(s.ops))
            ops[at] = s.ops
            a = np.tile(s.args, (len(rows), 1))
            a[:, s.var_pos] = cols[:, s.var_ord]
            args[at] = a
            kind[rows] = L.ROW_TAPE
        else:
            p0[rp[rows][:, None] + np.arange(cols.shape[1])] = g["coef"]
            kind[rows], lin[rows] = L.ROW_SEP, 1
    return ktn.NLPDescription(n, rp, col, kind, lin, np.zeros(m), np.zeros(rp[-1]), p0, np.zeros(rp[-1]), tp, ops, args,
                              obj_linear=True, obj_col=[0], obj_atom_kind=[0], obj_p0=[1.0], obj_p1=[0.0])


def signed_point(rng, n):
    """|x_j| in [0.1, 1], random signs"""
    return rng.uniform(0.1, 1.0, n) * rng.choice([-1.0, 1.0], n)


# ---- the edge rows of tests/test_gpu_tapes.py, restated ------------------------------------------------------------------
class Rows:
    """tape rows over variables of their own: rows[i] = (ops, args, structure cols, rconst)"""

    def __init__(self):
        self.x, self.rows = [], []

    def vars(self, *values):
        j0 = len(self.x)
        self.x.extend(float(v) for v in values)
        return [ktn.var(j0 + k) for k in range(len(values))]

    def add(self, e, rconst=0.0, cols=None, what=""):
        e = ktn.Expr.wrap(e)
        ops, args = e.tape()
        self.add_raw(ops, args, e.variables() if cols is None else cols, rconst, what)

    def add_raw(self, ops, args, cols, rconst=0.0, what=""):
        self.rows.append(SimpleNamespace(ops=np.asarray(ops, dtype=np.int32), args=np.asarray(args, dtype=np.float64),
                                         cols=list(cols), rconst=float(rconst), what=what))

    def desc(self):
        rp = np.concatenate([[0], np.cumsum([len(r.cols) for r in self.rows])])
        tp = np.concatenate([[0], np.cumsum([len(r.ops) for r in self.rows])])
        col = np.concatenate([np.asarray(r.cols, dtype=np.int32) for r in self.rows])
        m = len(self.rows)
        return ktn.NLPDescription(len(self.x), rp, col, np.full(m, L.ROW_TAPE), np.zeros(m), [r.rconst for r in self.rows],
                                  None, None, None, tp, np.concatenate([r.ops for r in self.rows]).astype(np.int32),
                                  np.concatenate([r.args for r in self.rows]).astype(np.float64),
                                  obj_linear=True, obj_col=[0], obj_atom_kind=[0], obj_p0=[1.0], obj_p1=[0.0])


POWERS = [0.0, 1.0, 2.0, 3.0, -1.0, -2.0, 0.5, 1.0 / 3.0, 2.5, -0.5]


def edge_rows(R):
    """one copy of every row of the two sections, over fresh variables of R"""
    for p in POWERS:
        for base in (0.37, 1.9, 123.456, 1e-3, 0.0, -0.0, -1.7, -0.25):
            x, = R.vars(base)
            R.add(x ** p, what=("pow", base, p))
        y, z = R.vars(0.8, -1.3)
        R.add(2.0 * (y * z + 1.5) ** p, what=("pow of a product", p))
    for a in [1e-300, 1e-8, -0.3, 0.7, math.pi / 2, math.pi, -math.pi, 1.5 * math.pi, 2 * math.pi, 100 * math.pi,
              np.nextafter(math.pi / 2, 0), 1e6, -1e6 + 0.5, 123456.789, 710.0]:
        x, = R.vars(a)
        R.add(ktn.sin(x), what=("sin", a))
        R.add(ktn.cos(x), what=("cos", a))
        y, = R.vars(a)
        R.add(3.0 * ktn.sin(y) - ktn.cos(y) * 0.5, what=("sin-cos", a))
    for num, den in [(1.5, 0.0), (1.5, -0.0), (-2.0, 0.0), (0.0, 0.0), (1e-100, 1e100), (1e100, 1e-100), (-3.0, 7.0)]:
        a, b = R.vars(num, den)
        R.add(a / b, what=("div", num, den))
    for v in (0.0, -0.0, -1.0, 1e-308, 5e-324, 2.5, 1e300):
        x, = R.vars(v)
        R.add(ktn.log(x), what=("log", v))
        y, = R.vars(v)
        R.add(ktn.sqrt(y), what=("sqrt", v))
    for v in (710.0, -710.0, -750.0, 709.0, 0.5):
        x, = R.vars(v)
        R.add(ktn.exp(x), what=("exp", v))
    a, b = R.vars(0.3, -1.25)
    R.add(-(a - b), what="neg sub")
    R.add(-(-a), rconst=0.125, what="neg neg + rconst")
    R.add(ktn.sin(ktn.const(2.0)), what="sin(2)")
    R.add(ktn.sqrt(ktn.const(2.0)) * ktn.exp(ktn.const(-1.0)) - 1.0, rconst=-0.5, what="constants")
    R.add_raw([], [], [], rconst=0.75, what="empty tape")
    R.add_raw([], [], [a.args[0]], rconst=-2.0, what="empty tape with a structural column")
    # repeated / unsorted / unused / duplicated columns
    x, = R.vars(1.3)
    R.add(x * x * x, what="x*x*x")
    x, = R.vars(-0.7)
    R.add(x / x, what="x/x")
    x, = R.vars(0.9)
    R.add(x - x, what="x-x")
    x, = R.vars(0.6)
    R.add(ktn.sin(x) * ktn.cos(x), what="sin cos")
    v = R.vars(0.4, 1.1, -0.2, 2.0, 0.05)
    e = v[4] ** 3.0 + ktn.exp(v[1]) * v[3] - v[0] / v[2]
    cols = [v[3].args[0], v[0].args[0], v[4].args[0], v[2].args[0], v[1].args[0]]
    R.add(e, cols=cols, what="unsorted")
    unused = R.vars(5.0, -6.0)
    R.add(e, cols=cols[::-1] + [u.args[0] for u in unused], what="unused columns")
    R.add(v[1] * v[1] + ktn.log(v[3]), cols=[v[1].args[0], v[3].args[0], v[1].args[0], unused[0].args[0], v[3].args[0]],
          what="duplicated entries")
    a, b = R.vars(1.5, -2.0)
    R.add(a * b, cols=[b.args[0], a.args[0], b.args[0], a.args[0]], what="a*b, both columns listed twice")


def docs_model(blocks, solver):
    """the docs' model, `blocks` independent copies: min x + y, sqrt(x^2 + y^2) <= z - 0.25, x^2 + y^2 <= -z + 1,
    x, y in [-1, 1], z in [0, 2]"""
    M = ktn.jump_like.Model(solver=solver)
    obj = None
    for _ in range(blocks):
        x, y, z = M.variable(-1.0, 1.0), M.variable(-1.0, 1.0), M.variable(0.0, 2.0)
        obj = x + y if obj is None else obj + x + y
        M.constraint(("<=", ktn.sqrt(x ** 2 + y ** 2), z - 0.25))
        M.constraint(("<=", x ** 2 + y ** 2, -z + 1.0))
    M.objective("Min", obj)
    return M


def cone_family(nrows, nlog, seed=0):
    """the model of test_gpu_supporting_hyperplanes.py (_cone_family), restated: nrows rows sqrt(x^2 + y^2) - z <= -0.25 and nlog
    rows log(w) >= lb, every row on its own variables; min sum z + 0.3 x - 0.2 y + sum w"""
    rng = np.random.default_rng(seed)
    n = 3 * nrows + nlog
    cons, lb, ub, c = [], [], [], np.zeros(n)
    for r in range(nrows):
        x, y, z = ktn.var(3 * r), ktn.var(3 * r + 1), ktn.var(3 * r + 2)
        cons.append(ktn.sqrt(x ** 2 + y ** 2) - z)
        lb.append(-math.inf); ub.append(-0.25)
        c[3 * r:3 * r + 3] = [0.3 + 0.1 * rng.uniform(), -0.2 - 0.1 * rng.uniform(), 1.0]
    for r in range(nlog):
        j = 3 * nrows + r
        cons.append(ktn.log(ktn.var(j)))
        lb.append(float(rng.uniform(-1.0, 0.5))); ub.append(math.inf)
        c[j] = 1.0
    lv = np.full(n, -5.0); uv = np.full(n, 5.0)
    lv[3 * nrows:] = 1e-3
    obj = None
    for j in np.flatnonzero(c):
        t = float(c[j]) * ktn.var(int(j))
        obj = t if obj is None else obj + t
    d = ktn.ExprNLP(n, obj, cons)
    return n, d, lv, uv, np.array(lb), np.array(ub)
