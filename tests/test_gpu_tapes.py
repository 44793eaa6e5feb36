"""GPU tier: expression tapes (KTN_ROW_TAPE rows and objectives, k_tape_eval) against the high-precision reference of
tests/tape_ref.py, at the opcodes, edges, structures and sizes the reference models never reach.

Tolerances: tape rows use the reference's derived bounds (tape_ref.py docstring: value 2E + 4u|exact|, partials
(4L + 8)(u Jmag + eta), exact class where the float64 result is not finite).  Separable rows and the 2e5-row set use
the existing rules of test_gpu_separator.py: Jacobian entries 4 ulp (device libm), g 1e-13 * sum|terms| (association).
"""
import math
import zlib
from types import SimpleNamespace

import ctypes as C
import numpy as np
import pytest

import katana_jl_amd as ktn
import tape_ref
from helpers import assert_planted_objective, instance_as_expressions, julia_shaped_nlp
from kat_util import check_expectation, load_kats
from oracle.katana import linear_oa_cut, round_coefs

pytestmark = pytest.mark.gpu
L = ktn._lib
ULP4 = 4 * np.finfo(float).eps
INF = math.inf


class Rows:
    """tape rows over variables of their own: rows[i] = (ops, args, structure cols, rconst, declared linear)"""

    def __init__(self):
        self.x, self.rows = [], []

    def vars(self, *values):
        j0 = len(self.x)
        self.x.extend(float(v) for v in values)
        return [ktn.var(j0 + k) for k in range(len(values))]

    def add(self, e, rconst=0.0, cols=None, linear=0, what=""):
        e = ktn.Expr.wrap(e)
        ops, args = e.tape()
        self.add_raw(ops, args, e.variables() if cols is None else cols, rconst, linear, what)

    def add_raw(self, ops, args, cols, rconst=0.0, linear=0, what=""):
        self.rows.append(SimpleNamespace(ops=np.asarray(ops, dtype=np.int32), args=np.asarray(args, dtype=np.float64),
                                         cols=list(cols), rconst=float(rconst), linear=int(linear), what=what))

    def desc(self, n=None, **obj):
        n = len(self.x) if n is None else n
        rp = np.concatenate([[0], np.cumsum([len(r.cols) for r in self.rows])])
        tp = np.concatenate([[0], np.cumsum([len(r.ops) for r in self.rows])])
        cat = lambda k, dt: np.concatenate([getattr(r, k) for r in self.rows]).astype(dt) if self.rows else np.zeros(0, dt)
        col = np.concatenate([np.asarray(r.cols, dtype=np.int32) for r in self.rows]) if self.rows else []
        obj = obj or dict(obj_linear=True, obj_col=[0], obj_atom_kind=[0], obj_p0=[1.0], obj_p1=[0.0])
        m = len(self.rows)
        return ktn.NLPDescription(n, rp, col, np.full(m, L.ROW_TAPE), [r.linear for r in self.rows],
                                  [r.rconst for r in self.rows], None, None, None, tp, cat("ops", np.int32),
                                  cat("args", np.float64), **obj)


def load(d, n, m, lb=None, ub=None, lv=-INF, uv=INF, sense="Min", **kw):
    model = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, **kw))
    model.loadproblem(n, m, np.full(n, lv), np.full(n, uv), np.full(m, -INF) if lb is None else lb,
                      np.zeros(m) if ub is None else ub, sense, d)
    sep = ktn.KatanaHipSeparator(model)
    sep.initialize()
    return model, sep


def device_row(sep, i):
    """{column: device partial} of row i; a column listed again in the structure must hold exactly 0 there (only its
    first entry receives the derivative)"""
    by = {}
    for e in range(sep.rowptr[i], sep.rowptr[i + 1]):
        c = int(sep.col[e])
        if c in by:
            assert sep.jac[e] == 0.0, ("duplicated structure entry not 0", i, c, sep.jac[e])
            continue
        by[c] = float(sep.jac[e])
    return by


def check_rows(sep, R, x, rows=None, offset=0):
    refs = []
    for k, r in enumerate(R.rows if rows is None else rows):
        i = offset + k
        ref = tape_ref.evaluate(r.ops, r.args, x, rconst=r.rconst)
        ref.check_value(float(sep.g[i]), (i, r.what))
        ref.check_grad(device_row(sep, i), (i, r.what))
        refs.append(ref)
    return refs


def run(R, **kw):
    x = np.asarray(R.x)
    _, sep = load(R.desc(), len(x), len(R.rows), **kw)
    sep.precompute(x)
    return check_rows(sep, R, x), sep


# ---- a. every opcode and its edges ----------------------------------------------------------------------------------
POWERS = [0.0, 1.0, 2.0, 3.0, -1.0, -2.0, 0.5, 1.0 / 3.0, 2.5, -0.5]


def test_powc_every_exponent_at_positive_zero_and_negative_bases():
    R = Rows()
    for p in POWERS:
        for base in (0.37, 1.9, 123.456, 1e-3, 0.0, -0.0, -1.7, -0.25):
            x, = R.vars(base)
            R.add(x ** p, what=("pow", base, p))
        y, z = R.vars(0.8, -1.3)
        R.add(2.0 * (y * z + 1.5) ** p, what=("pow of a product", p))     # the adjoint that meets the derivative is not 1
    run(R)


def test_sin_cos_at_small_arguments_near_multiples_of_half_pi_and_up_to_1e6():
    R = Rows()
    args = [1e-300, 1e-8, -0.3, 0.7, math.pi / 2, math.pi, -math.pi, 1.5 * math.pi, 2 * math.pi, 100 * math.pi,
            np.nextafter(math.pi / 2, 0), 1e6, -1e6 + 0.5, 123456.789, 710.0]
    for a in args:
        x, = R.vars(a)
        R.add(ktn.sin(x), what=("sin", a))
        R.add(ktn.cos(x), what=("cos", a))
        y, = R.vars(a)
        R.add(3.0 * ktn.sin(y) - ktn.cos(y) * 0.5, what=("sin-cos", a))
    run(R)


def test_div_log_sqrt_exp_at_their_domain_edges():
    R = Rows()
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
    run(R)


def test_neg_sub_constant_only_and_empty_tapes():
    R = Rows()
    a, b = R.vars(0.3, -1.25)
    R.add(-(a - b), what="neg sub")
    R.add(-(-a), rconst=0.125, what="neg neg + rconst")
    R.add(ktn.sin(ktn.const(2.0)), what="sin(2)")
    R.add(ktn.sqrt(ktn.const(2.0)) * ktn.exp(ktn.const(-1.0)) - 1.0, rconst=-0.5, what="constants")
    R.add_raw([], [], [], rconst=0.75, what="empty tape")
    R.add_raw([], [], [0], rconst=-2.0, what="empty tape with a structural column")
    refs, sep = run(R)
    assert refs[4].value_f64 == 0.75 and sep.g[4] == 0.75 and sep.g[5] == -2.0 and sep.jac[sep.rowptr[5]] == 0.0


# ---- b. structure ---------------------------------------------------------------------------------------------------
def test_repeated_unsorted_unused_and_duplicated_columns():
    R = Rows()
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
    cols = [v[3].args[0], v[0].args[0], v[4].args[0], v[2].args[0], v[1].args[0]]       # structure unsorted, tape order differs
    R.add(e, cols=cols, what="unsorted")
    unused = R.vars(5.0, -6.0)
    R.add(e, cols=cols[::-1] + [u.args[0] for u in unused], what="unused columns")
    R.add(v[1] * v[1] + ktn.log(v[3]), cols=[v[1].args[0], v[3].args[0], v[1].args[0], unused[0].args[0], v[3].args[0]],
          what="duplicated entries")
    refs, sep = run(R)
    assert sep.g[2] == 0.0 and sep.jac[sep.rowptr[2]] == 0.0                         # x - x: exactly 0


def test_duplicated_structure_entry_keeps_the_first_slot_rule():
    """duplicated (row, col): the first structure entry gets the derivative, the others exactly 0"""
    R = Rows()
    a, b = R.vars(1.5, -2.0)
    R.add(a * b, cols=[b.args[0], a.args[0], b.args[0], a.args[0]])
    x = np.asarray(R.x)
    _, sep = load(R.desc(), 2, 1)
    sep.precompute(x)
    assert list(sep.jac) == [1.5, -2.0, 0.0, 0.0]


# ---- c. size --------------------------------------------------------------------------------------------------------
def _term(k, x, c):
    return [c * x ** 2, c * ktn.exp(0.1 * x), c * ktn.sin(x), c * ktn.log(x + 3.0), c * ktn.sqrt(x + 2.5)][k % 5]


def test_long_and_deep_tape_rows():
    """one row over 1e5 distinct variables, and left- and right-folded sums 5e4 deep"""
    rng = np.random.default_rng(21)
    R = Rows()
    N = 100000
    v = R.vars(*rng.uniform(-1.0, 1.0, N))
    c = rng.uniform(-2.0, 2.0, N)
    e = _term(0, v[0], c[0])
    for j in range(1, N):
        e = e + _term(j, v[j], c[j])
    R.add(e, rconst=-1.0, what="1e5 variables")
    M = 50000
    w = R.vars(*rng.uniform(-1.5, 1.5, M))
    left = w[0] ** 2
    for j in range(1, M):
        left = left + w[j] ** 2
    R.add(left, what="left fold")
    right = w[M - 1] * w[0]
    for j in range(M - 2, -1, -1):
        right = w[j] * w[(j + 1) % M] + right
    R.add(right, what="right fold (every variable twice)")
    run(R)


def test_2e5_short_tape_rows():
    """many workgroups of short rows: all rows against a vectorised float64 reference (4 ulp / 1e-13 sum|terms|), a
    seeded sample of 1 000 rows and the edge rows against mpmath"""
    rng = np.random.default_rng(5)
    m, n = 200000, 50000
    k = rng.integers(4, 9, m)
    ent = int(k.sum())
    rp = np.concatenate([[0], np.cumsum(k)])
    # distinct columns within a row: a random start plus increasing offsets
    start = rng.integers(0, n - 64, m)
    off = np.concatenate([np.sort(rng.choice(64, size=int(kk), replace=False)) for kk in k])
    col = np.repeat(start, k) + off
    kind = rng.integers(0, 5, ent)
    c = rng.uniform(-2.0, 2.0, ent)
    x = rng.uniform(-1.0, 1.0, n)
    # tape of term t: CONST c, VAR, [kind ops], MUL; rows fold left: t0 t1 ADD t2 ADD ...
    body = {0: [(L.OP_POWC, 2.0)], 1: [(L.OP_CONST, 0.1), ("swapmul",)], 2: [(L.OP_SIN, 0.0)],
            3: [(L.OP_CONST, 3.0), (L.OP_ADD, 0.0), (L.OP_LOG, 0.0)], 4: [(L.OP_CONST, 2.5), (L.OP_ADD, 0.0), (L.OP_SQRT, 0.0)]}
    ops, args, tp = [], [], [0]
    for i in range(m):
        for e in range(rp[i], rp[i + 1]):
            ops.append(L.OP_CONST); args.append(c[e])
            kd = int(kind[e])
            if kd == 1:
                ops += [L.OP_CONST, L.OP_VAR, L.OP_MUL, L.OP_EXP]; args += [0.1, float(col[e]), 0.0, 0.0]
            else:
                ops.append(L.OP_VAR); args.append(float(col[e]))
                for o, a in body[kd]:
                    ops.append(o); args.append(a)
            ops.append(L.OP_MUL); args.append(0.0)
            if e > rp[i]:
                ops.append(L.OP_ADD); args.append(0.0)
        tp.append(len(ops))
    d = ktn.NLPDescription(n, rp, col, np.full(m, L.ROW_TAPE), np.zeros(m), np.zeros(m), None, None, None, tp, ops, args,
                           obj_linear=True, obj_col=[0], obj_atom_kind=[0], obj_p0=[1.0], obj_p1=[0.0])
    _, sep = load(d, n, m)
    sep.precompute(x)
    xv = x[col]
    f = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [xv ** 2, np.exp(0.1 * xv), np.sin(xv), np.log(xv + 3.0)],
                  np.sqrt(xv + 2.5))
    fd = np.select([kind == 0, kind == 2, kind == 3], [2.0 * xv, np.cos(xv), 1.0 / (xv + 3.0)], 0.5 / np.sqrt(xv + 2.5))
    term = c * f
    Jref = np.where(kind == 1, (c * f) * 0.1, c * fd)                 # the reverse sweep's order: adjoint times partial
    assert np.array_equal(sep.col, col)
    assert np.all(np.abs(sep.jac - Jref) <= ULP4 * np.abs(Jref) + 1e-300)
    rows = np.repeat(np.arange(m), k)
    g = np.bincount(rows, weights=term, minlength=m)
    mag = np.bincount(rows, weights=np.abs(term), minlength=m)
    assert np.all(np.abs(sep.g - g) <= 1e-13 * mag)
    R = SimpleNamespace(rows=[])
    sample = np.sort(rng.choice(m, 1000, replace=False))
    for i in sample:
        ref = tape_ref.evaluate(ops[tp[i]:tp[i + 1]], args[tp[i]:tp[i + 1]], x)
        ref.check_value(float(sep.g[i]), i)
        ref.check_grad(device_row(sep, i), i)


def test_tape_objective_over_2e4_variables_epigraph_row_and_pad_zero():
    """a TAPE objective: the epigraph row f(x) - t (structural columns + t) and its cut; one column with a partial just
    below -(1e9 + 0) is kept only if round_coefs forgets the dense row's zeros (pad_zero)"""
    rng = np.random.default_rng(8)
    n, used = 20003, 20000
    cc = rng.uniform(0.5, 1.0, used)
    x = np.concatenate([cc - rng.uniform(0.6, 1.0, used), np.zeros(n - used)])     # partials 2(x - c) in (-2, -1.2)
    x[17] = cc[17]
    v = [ktn.var(j) for j in range(used)]
    f = (v[0] - cc[0]) ** 2
    for j in range(1, used):
        f = f + (v[j] - cc[j]) ** 2
    f = f - (1e9 + 0.5) * v[17] + 1e12
    o, a = f.tape()
    d = ktn.NLPDescription(n, [0, 1], [0], [L.ROW_SEP], [1], [0.0], [0], [1.0], [0.0], obj_linear=False,
                           obj_kind=L.ROW_TAPE, obj_tape_op=o, obj_tape_arg=a)
    model, sep = load(d, n, 1, ub=np.array([1e6]), lv=-10.0, uv=10.0)
    t = 0.0
    xl = np.append(x, t)
    sep.precompute(xl)
    assert sep.num_constr == 2
    assert list(sep.col[sep.rowptr[1]:sep.rowptr[2]]) == list(range(used)) + [n]
    ref = tape_ref.evaluate(o, a, x)
    ref.check_value(float(sep.g[1]), "epigraph value")                # f(x) - t with t = 0
    J = device_row(sep, 1)
    assert J.pop(n) == -1.0
    ref.check_grad(J, "epigraph partials")
    m0 = model.lp_num_rows()
    nviol, _ = sep.sweep(1e-6)
    assert nviol == 1
    rowptr, col, val, lo, hi = model.lp_rows_from(m0)
    assert list(col) == list(range(used)) + [n]
    # the reference's epigraph row is dense (src/nlpeval.jl:49-54): zeros in the n - used columns the tape never names
    dense = [float(ref.grad.get(j, 0.0)) for j in range(n)] + [-1.0]
    want = linear_oa_cut(SimpleNamespace(g=[float(ref.value) - t], jac=dense, xstar=xl, sp_cols=[list(range(n + 1))],
                                         sp_col_inds=[list(range(n + 1))]), xl, None, 0)
    round_coefs(want, 1e9)
    assert val[17] == 0.0 and want.coeffs[17] == 0.0                  # zeroed only because of the padded zeros
    wc = np.asarray(want.coeffs)[list(range(used)) + [n]]
    assert np.array_equal(val == 0.0, wc == 0.0)
    tol = np.array([float(ref.grad_tol(j)) for j in range(used)] + [0.0])
    assert np.all(np.abs(val - wc) <= tol)
    assert lo[0] == -INF and abs(hi[0] - (0.0 - want.constant)) <= 1e-12 * (np.sum(np.abs(xl[col] * val)) + abs(sep.g[1]) + 1)


# ---- d. one model mixing row kinds ----------------------------------------------------------------------------------
class MixedNLP(ktn.NLPDescription):
    """SEP, TAPE, HOST and empty rows in one description; HOST rows are the values of `host(i, x)` -> (g, {slot: J})"""

    def __init__(self, host_rows, host_fn, *a, **kw):
        super().__init__(*a, **kw)
        self.host_rows, self.host_fn = host_rows, host_fn
        m, nnz, n = self.num_constr, len(self.col), self.num_var

        def rows_cb(_user, xp, gp, jp):
            try:
                xv = np.ctypeslib.as_array(xp, (n,)).copy()
                g = np.ctypeslib.as_array(gp, (m,))
                J = np.ctypeslib.as_array(jp, (nnz,))
                for i in self.host_rows:
                    gi, Ji = self.host_fn(i, xv)
                    g[i] = gi
                    J[self.rowptr[i]:self.rowptr[i + 1]] = Ji
                return 0
            except Exception:
                return 1
        self._rows_cb = L.EVAL_ROWS_CB(rows_cb)

    def c_struct(self):
        d = super().c_struct()
        d.eval_rows = C.cast(self._rows_cb, C.c_void_p)
        return d


def test_mixed_row_kinds_precompute_sweep_and_cuts():
    rng = np.random.default_rng(13)
    n, m = 12000, 400
    x = rng.uniform(0.2, 1.2, n)
    kinds = rng.choice(["sep", "tape", "tape_lin", "host", "empty"], m, p=[0.3, 0.35, 0.1, 0.15, 0.1])
    kinds[7] = "sep_long"
    kinds[11] = "tape_big"                                            # round_coefs zeroes entries of its cut
    rowptr, col, akind, p0, p1, rk, rlin, rc = [0], [], [], [], [], [], [], []
    tptr, top, targ = [0], [], []
    spec = {}
    for i, kd in enumerate(kinds):
        r0 = float(rng.uniform(-3, 1))
        if kd in ("sep", "sep_long"):
            kk = 9000 if kd == "sep_long" else int(rng.integers(3, 20))
            cs = np.sort(rng.choice(n, kk, replace=False))
            ak = rng.integers(0, 4, kk)
            a0, a1 = rng.uniform(0.1, 1.0, kk), rng.uniform(0.1, 1.0, kk)
            col += cs.tolist(); akind += ak.tolist(); p0 += a0.tolist(); p1 += a1.tolist()
            rk.append(L.ROW_SEP); rlin.append(int(np.all(ak == 0))); rc.append(r0)
            spec[i] = ("sep", cs, ak, a0, a1, r0)
        elif kd in ("tape", "tape_lin", "tape_big"):
            cs = rng.choice(n, int(rng.integers(2, 9)), replace=False)
            vs = [ktn.var(int(j)) for j in cs]
            if kd == "tape_lin":
                e = 2.0 * vs[0] - vs[1] / 4.0 + 0.5
                for v in vs[2:]:
                    e = e + float(rng.uniform(-1, 1)) * v
            elif kd == "tape_big":
                x[int(cs[0])] = 0.3                                   # partial of vs[0]: 6e9 x - 5e9 = -3.2e9, zeroed
                e = 3e9 * vs[0] ** 2 + 2.0 * vs[1] - 5e9 * vs[0] + ktn.sin(vs[1]) + 1e10
            else:
                e = _term(int(rng.integers(5)), vs[0], float(rng.uniform(-2, 2)))
                for t, v in enumerate(vs[1:]):
                    e = e * 0.5 + _term(int(rng.integers(5)), v, float(rng.uniform(-2, 2))) if t % 2 else e + ktn.exp(v - 1.0) * v
            o, a = e.tape()
            cs = rng.permutation(cs)                                  # structure unsorted
            col += cs.tolist(); akind += [0] * len(cs); p0 += [0.0] * len(cs); p1 += [0.0] * len(cs)
            top += o.tolist(); targ += a.tolist()
            rk.append(L.ROW_TAPE); rlin.append(1 if kd == "tape_lin" else 0); rc.append(r0)
            spec[i] = ("tape", o, a, r0)
        elif kd == "host":
            cs = np.sort(rng.choice(n, int(rng.integers(1, 6)), replace=False))
            w = rng.uniform(-1, 1, len(cs))
            col += cs.tolist(); akind += [0] * len(cs); p0 += [0.0] * len(cs); p1 += [0.0] * len(cs)
            rk.append(L.ROW_HOST); rlin.append(0); rc.append(0.0)
            spec[i] = ("host", cs, w, r0)
        else:
            rk.append(L.ROW_SEP); rlin.append(1); rc.append(r0)
            spec[i] = ("empty", r0)
        rowptr.append(len(col)); tptr.append(len(top))

    def host(i, xv):
        _, cs, w, r0 = spec[i]
        return float(np.sum(w * xv[cs] ** 2) + r0), 2.0 * w * xv[cs]

    host_rows = [i for i in range(m) if kinds[i] == "host"]
    d = MixedNLP(host_rows, host, n, rowptr, col, rk, rlin, rc, akind, p0, p1, tptr, top, targ,
                 obj_linear=True, obj_col=[0], obj_atom_kind=[0], obj_p0=[1.0], obj_p1=[0.0])
    model, sep = load(d, n, m, lv=-5.0, uv=5.0)
    sep.precompute(x)
    from katana_jl_amd.instances import atom_value_deriv

    ref_g, ref_J, ref_tol = np.zeros(m), {}, {}
    for i in range(m):
        s = spec[i]
        a, b = sep.rowptr[i], sep.rowptr[i + 1]
        if s[0] == "sep":
            _, cs, ak, a0, a1, r0 = s
            val, der = atom_value_deriv(ak.astype(np.uint8), a0, a1, x[cs])
            assert np.all(np.abs(sep.jac[a:b] - der) <= ULP4 * np.abs(der) + 1e-300), i
            assert abs(sep.g[i] - (val.sum() + r0)) <= 1e-13 * (np.abs(val).sum() + abs(r0)), i
            ref_g[i], ref_J[i], ref_tol[i] = val.sum() + r0, der, ULP4 * np.abs(der) + 1e-300
        elif s[0] == "tape":
            ref = tape_ref.evaluate(s[1], s[2], x, rconst=s[3])
            ref.check_value(float(sep.g[i]), i)
            ref.check_grad(device_row(sep, i), i)
            ref_g[i] = float(ref.value)
            first = [c not in sep.col[a:a + k] for k, c in enumerate(sep.col[a:b])]       # duplicates: 0 after the first
            ref_J[i] = np.array([float(ref.grad.get(int(c), 0.0)) if f else 0.0 for c, f in zip(sep.col[a:b], first)])
            ref_tol[i] = np.array([float(ref.grad_tol(int(c))) if f else 0.0 for c, f in zip(sep.col[a:b], first)])
        elif s[0] == "host":
            gi, Ji = host(i, x)
            assert sep.g[i] == gi and np.array_equal(sep.jac[a:b], Ji), i          # staged as computed
            ref_g[i], ref_J[i], ref_tol[i] = gi, Ji, 0.0 * Ji
        else:
            assert sep.g[i] == s[1] and a == b
            ref_g[i], ref_J[i], ref_tol[i] = s[1], np.zeros(0), np.zeros(0)
    # sweep over the NL rows: the violated rows in row order, their cuts as linear_oa_cut + round_coefs make them
    nl = [i for i in range(m) if not rlin[i]]
    viol = [i for i in nl if ref_g[i] > 1e-6]
    assert len(nl) > 256 and 11 in viol and 7 in viol
    assert abs(ref_g[11]) > 1e6
    m0 = model.lp_num_rows()
    nviol, maxviol = sep.sweep(1e-6)
    assert nviol == len(viol)
    assert abs(maxviol - max(ref_g[i] for i in viol)) <= 1e-12 * (1 + maxviol)
    rowptr_c, col_c, val_c, lo_c, hi_c = model.lp_rows_from(m0)
    for r, i in enumerate(viol):
        a, b = sep.rowptr[i], sep.rowptr[i + 1]
        cut = linear_oa_cut(SimpleNamespace(g={i: ref_g[i]}, jac=ref_J[i], xstar=x, sp_cols={i: sep.col[a:b]},
                                            sp_col_inds={i: np.arange(b - a)}), x, None, i)
        round_coefs(cut, 1e9)
        ca, cb = rowptr_c[r], rowptr_c[r + 1]
        assert list(col_c[ca:cb]) == list(cut.vars), i
        want = np.asarray(cut.coeffs)
        assert np.array_equal(val_c[ca:cb] == 0.0, want == 0.0), i
        assert np.all(np.abs(val_c[ca:cb] - want) <= np.where(want == 0.0, 0.0, ref_tol[i])), i
        scale = np.sum(np.abs(x[cut.vars] * want)) + abs(ref_g[i]) + 1
        assert lo_c[r] == -INF and abs(hi_c[r] - (0.0 - cut.constant)) <= 1e-12 * scale, i
    assert np.sum(val_c[rowptr_c[viol.index(11)]:rowptr_c[viol.index(11) + 1]] == 0.0) >= 1
    # a non-finite Jacobian entry of a violated tape row: the cut is refused and the model ends in :Error
    R = Rows()
    a, = R.vars(0.0)
    R.add(ktn.sqrt(a) + 1.0)
    mod2, sep2 = load(R.desc(), 1, 1)
    sep2.precompute(np.zeros(1))
    assert sep2.jac[0] == INF
    sep2.sweep(1e-6)
    assert mod2.status() == "Error"


# ---- e. end to end --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,n,m_nl,objective", [("explog", 2000, 300, "linear"), ("quad", 4000, 500, "quad"),
                                                     ("explog", 20000, 2000, "linear")])
def test_same_instance_through_tapes_and_separable_rows(family, n, m_nl, objective):
    inst = ktn.instances.make_instance(n=n, m_nl=m_nl, k=16, family=family, seed=9, objective=objective)
    obj, cons = instance_as_expressions(ktn, inst)
    d_tape = ktn.ExprNLP(inst.n, obj, cons)
    assert int(np.sum(d_tape.row_kind == L.ROW_TAPE)) == inst.m_nl
    assert d_tape.obj_kind == (L.ROW_TAPE if objective == "quad" else L.ROW_SEP)
    res = []
    for d in (d_tape, ktn.SeparableNLP(inst)):
        model = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))
        model.loadproblem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr, inst.u_constr, inst.sense, d)
        sep = ktn.KatanaHipSeparator(model); sep.initialize()
        xs = np.clip(inst.xhat + 0.3, inst.l_var, inst.u_var)
        if objective != "linear":
            xs = np.append(xs, 0.0)
        sep.precompute(xs)
        first = (sep.g.copy(), sep.rowptr.copy(), sep.col.copy(), sep.jac.copy())
        status = model.optimize()
        assert status == "Optimal", (status, d is d_tape)
        assert_planted_objective(model.getobjval(), inst)
        res.append(first)
    (g0, rp0, c0, j0), (g1, rp1, c1, j1) = res
    assert np.array_equal(rp0[:inst.num_constr + 1], rp1[:inst.num_constr + 1])
    assert np.array_equal(c0[:rp0[inst.num_constr]], c1[:rp1[inst.num_constr]])
    from katana_jl_amd.instances import atom_value_deriv
    val, _ = atom_value_deriv(inst.kind, inst.p0, inst.p1, xs[inst.col])
    rows = np.repeat(np.arange(inst.num_constr), np.diff(inst.rowptr))
    mag = np.bincount(rows, weights=np.abs(val), minlength=inst.num_constr) + np.abs(inst.rconst)
    mc = inst.num_constr
    assert np.all(np.abs(g0[:mc] - g1[:mc]) <= 1e-13 * (mag + 1.0))
    e = rp0[mc]
    assert np.all(np.abs(j0[:e] - j1[:e]) <= ULP4 * np.abs(j1[:e]) + 1e-300)


def _convex_models():
    """small convex models that use every opcode (s-expressions of tests/golden/kat_models.json's format)"""
    V = lambda j: ["var", j]
    out = []
    # sin on [0, pi] in a >= row, cos on [pi/2, 3pi/2] in a <= row, x^p (p >= 1) on x >= 0, x^-1 and -log x on x > 0,
    # x^0.5 in a >= row, x^2 / y for y > 0, exp(x - y)
    cons = [
        {"expr": ["-", ["sin", V(0)], 0.5], "lb": 0.0, "ub": math.inf, "linear": False},
        {"expr": ["+", ["cos", V(1)], 0.3], "lb": -math.inf, "ub": 0.0, "linear": False},
        {"expr": ["+", ["^", V(2), 3.0], ["^", V(3), 2.5], ["^", V(4), 1.0], -4.0], "lb": -math.inf, "ub": 0.0, "linear": False},
        {"expr": ["+", ["^", V(5), -1.0], ["neg", ["log", V(6)]], -3.0], "lb": -math.inf, "ub": 0.0, "linear": False},
        {"expr": ["-", ["^", V(7), 0.5], 0.8], "lb": 0.0, "ub": math.inf, "linear": False},
        {"expr": ["-", ["/", ["^", V(8), 2.0], V(9)], 1.0], "lb": -math.inf, "ub": 0.0, "linear": False},
        {"expr": ["-", ["exp", ["-", V(10), V(11)]], 2.0], "lb": -math.inf, "ub": 0.0, "linear": False},
        {"expr": ["+", V(0), V(1), V(2), -6.0], "lb": -math.inf, "ub": 0.0, "linear": True},
    ]
    vars_ = [{"lb": 0.0, "ub": math.pi}, {"lb": math.pi / 2, "ub": 1.5 * math.pi}] + [{"lb": 0.0, "ub": 3.0}] * 3 + \
            [{"lb": 0.2, "ub": 5.0}] * 2 + [{"lb": 0.01, "ub": 4.0}, {"lb": -2.0, "ub": 2.0}, {"lb": 0.5, "ub": 3.0},
                                           {"lb": -2.0, "ub": 2.0}, {"lb": -2.0, "ub": 2.0}]
    c = [-1.0, -0.5, -1.0, -0.7, -0.3, -0.4, 0.6, 0.5, -0.8, 0.3, -1.0, 0.9]
    lin = ["+"] + [["*", c[j], V(j)] for j in range(12)]
    out.append({"id": "every_op_lin", "vars": vars_, "sense": "Min", "objective": lin, "objective_linear": True,
                "constraints": cons})
    quad = ["+", lin, ["^", ["-", V(3), 1.0], 2.0], ["*", 0.5, ["^", ["-", V(8), 0.5], 2.0]]]
    out.append({"id": "every_op_quad", "vars": vars_, "sense": "Min", "objective": quad, "objective_linear": False,
                "constraints": cons})
    return out


@pytest.mark.parametrize("m", _convex_models(), ids=lambda m: m["id"])
def test_convex_models_using_every_opcode_agree_with_the_oracle(m):
    from helpers import hip_model_from_kat, oracle_solve_kat
    om = oracle_solve_kat(m)
    M = hip_model_from_kat(ktn, m)
    status = M.solve()
    assert status == om.status == "Optimal", (status, om.status)
    obj, oobj = M.getobjectivevalue(), om.getobjval()
    assert abs(obj - oobj) <= max(1e-6, 1e-6 * max(abs(obj), abs(oobj))), (obj, oobj)


KATS = load_kats()


@pytest.mark.parametrize("m", KATS, ids=[m["id"] for m in KATS])
def test_reference_models_through_julia_shaped_descriptions(m):
    rng = np.random.default_rng(zlib.crc32(m["id"].encode()))
    n = len(m["vars"])
    d = julia_shaped_nlp(ktn, n, m["objective"], [c["expr"] for c in m["constraints"]],
                         [c["linear"] for c in m["constraints"]], m["objective_linear"], rng)
    model = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))
    model.loadproblem(n, len(m["constraints"]), [v["lb"] for v in m["vars"]], [v["ub"] for v in m["vars"]],
                      [c["lb"] for c in m["constraints"]], [c["ub"] for c in m["constraints"]], m["sense"], d)
    status = model.optimize()
    check_expectation(m, status, model.getobjval(), model.getsolution()[:n])
