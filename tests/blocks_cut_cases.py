"""Seeded builders for the cut-by-cut tests of the device-side batch loop's Kelley path (k_ecp_blocks<0>, csrc/batch_ecp.hpp;
test code; GPU tier: tests/test_gpu_blocks_kelley.py, input conditions: tests/test_blocks_cut_cases.py).  No reference lives here:
the bounds are those of tests/sep_ref.py, tests/tape_ref.py and tests/quad_ref.py.

Part A -- one round at a prescribed point.  The point of a device round is the optimum of the instance's LP, so every instance
of `pinned_batch` has no linear row and the box l_var = u_var = C.x: its first LP has no rows, every column scaling stays 1.0
and the prox clips x to the box, which is C.x bit for bit.  The rows are those of sep_cases.make_case: lengths around the
16-lane trip (A_LENS), all 15 subsets of atom kinds, weights of either sign, all sides, the dyadic threshold rows, a row with
a repeated column, an unsorted row, the round_coefs row; one instance with 150 NL rows (three trips of the 64-group row loop,
the last one ragged), one with fewer than 16.  `pinned_batch(1)` has the edges = 1 rows (value NaN, partials finite) in two
of its instances.  LEFT OUT: empty NL rows and pad_zero rows -- the device loop refuses empty rows and nonlinear objectives at
load (csrc/ecp.hip, optimize_blocks_device); edges = 2 is test_gpu_sep_kernels.test_device_side_batch_loop_non_finite_row_ends_in_error.

Part B -- several rounds at the loop's own points: planted convex instances as separable, tape and KTN_ROW_QUAD rows
(`sep_items`, `tape_items`, `quad_items`, `mixed_items`), a QUAD instance with 70 NL rows (second trip of the 16-lane value
pass) and a tape instance with 1 100 short rows over 64 columns (`many_tape_rows`: second trip of the one-lane-per-row loop;
its arena fits the LDS budget with room for two cuts per row only).

`nl_rows_of` / `row_ref` give one interface to the three references: the exact g, partials and cut constant of an NL row at x
with their bounds against a device value.

Tape rows, the cut constant (tape_ref gives value and Jacobian bounds only; written out as quad_ref's docstring does, u = 2^-53,
h = 2^-1074, first order doubled):
    E_g    = 2 err + 4u |g|                                 (TapeResult.check_value)
    E_J(c) = (4L + 8)(u Jmag_c + eta)                       (TapeResult.grad_tol)
    dot    = sum_e x_e J_e:   E_dot = sum_e (|x_e| E_J(c_e) + 2u |x_e J_e| + h) + 2 (k + 1) u dotmag,   dotmag = sum |x_e J_e|
    b      = fl(g - dot):     E_b = E_g + E_dot + 2u (|g| + dotmag)
    lo = fl(lb - b), hi = fl(ub - b):   E_b + 2u |bound - b|
"""
import math

import numpy as np
from mpmath import mp, mpf

import katana_jl_amd as ktn
import quad_ref
import sep_cases as sc
import sep_ref
import tape_ref
from sep_ref import F_TOL, U

L = ktn._lib
INF = math.inf
H = 2.0 ** -1074
make = ktn.instances.make_instance

# ---- part A ---------------------------------------------------------------------------------------------------------------------
A_LENS = (1, 2, 15, 16, 17, 31, 32, 33, 48, 100)
CUT_COEF_RNG = 4.0
_A_PLAIN = [
    dict(seed=4101, n=128, m_nl=150, profile=A_LENS, repeat_rows=(4, 5, 9, 10, 11), unsorted_rows=(6, 7, 8, 12, 13)),
    dict(seed=4102, n=40, m_nl=12, profile=(1, 2, 15, 16, 17, 31, 32)),
    dict(seed=4103, n=101, m_nl=37, profile=(100, 48, 33, 17, 1)),
    dict(seed=4104, n=64, m_nl=70, profile=(16, 32, 48, 15, 31, 2)),
    dict(seed=4105, n=33, m_nl=21, profile=(33, 32, 31, 1)),
    dict(seed=4106, n=200, m_nl=65, profile=(100, 17, 16, 15)),
    dict(seed=4107, n=17, m_nl=16, profile=(17, 16, 15, 2, 1)),
]
_A_EDGE = [
    dict(seed=4201, n=64, m_nl=40, profile=(1, 16, 17, 33, 48), edges=1),
    dict(seed=4202, n=48, m_nl=14, profile=(2, 15, 32)),
    dict(seed=4203, n=120, m_nl=70, profile=(100, 31, 16, 1), edges=1, edge_len=33),
    dict(seed=4204, n=20, m_nl=9, profile=(17, 2)),
    dict(seed=4205, n=96, m_nl=30, profile=(48, 15, 33)),
    dict(seed=4206, n=35, m_nl=18, profile=(32, 31, 1)),
]


def pinned_case(spec):
    """a sep_cases.make_case model with a linear objective of non-zero costs over every column (C.cost)"""
    kw = dict(spec)
    C = sc.make_case(kw.pop("seed"), kw.pop("n"), kw.pop("m_nl"), list(kw.pop("profile")), cut_coef_rng=CUT_COEF_RNG, **kw)
    rng = np.random.default_rng([spec["seed"], 1])
    C.cost = np.where(rng.random(C.n) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 2.0, C.n)
    C.obj_col, C.obj_kind, C.obj_p0, C.obj_p1, C.obj_const = np.arange(C.n), np.zeros(C.n, dtype=np.uint8), C.cost, np.zeros(C.n), 0.0
    return C


def pinned_problem(C):
    """the model with its box pinned to the evaluation point: l_var = u_var = C.x"""
    return ktn.Problem(C.n, C.m, C.x.copy(), C.x.copy(), C.lb, C.ub, "Min", sc.description(ktn, C))


def pinned_batch(edges=0):
    return [pinned_case(s) for s in (_A_EDGE if edges else _A_PLAIN)]


def mp_sample(C, budget=4000):
    """rows for the mpmath comparison (test_gpu_sep_kernels._mp_sample on these cases): every special row, then bulk rows of
    every length within `budget` entries, drawn in a seeded order"""
    lens = np.diff(C.e_rowptr)
    rows = [r for r in range(len(lens)) if C.e_tags[r] != "bulk"]
    used = int(sum(lens[r] for r in rows))
    seen = {}
    for r in np.random.default_rng(C.m).permutation(len(lens)):
        if C.e_tags[r] != "bulk" or seen.get(int(lens[r]), 0) >= 3 or used + lens[r] > budget:
            continue
        seen[int(lens[r])] = seen.get(int(lens[r]), 0) + 1
        rows.append(int(r)); used += int(lens[r])
    return sorted(rows)


# ---- the device loop's shape rules (csrc/ecp.hip, optimize_blocks_device) -------------------------------------------------------
LDS_BUDGET = 158 * 1024
DEFAULT_CUT_CAPACITY = 12
_THREADS, _Q = 1024, 12


def fuse(items):
    probs = [ktn.batch._as_problem(i) for i in items]
    big, offs, _ = ktn.nlp.fuse_problems(probs, allow_quad=True)
    return probs, big, offs


def device_loop_lds(items, cut_capacity=DEFAULT_CUT_CAPACITY):
    """asserts the rules under which a batch is launched at all and returns the LDS bytes of the launch (the caller compares
    them with LDS_BUDGET)"""
    probs, big, offs = fuse(items)
    d = big.d
    assert d.obj_linear and big.sense == "Min" and d.obj_kind == L.ROW_SEP
    assert np.all(np.isfinite(big.l_var)) and np.all(np.isfinite(big.u_var))
    assert np.all(np.isin(d.row_kind, [L.ROW_SEP, L.ROW_TAPE, L.ROW_QUAD]))
    lens = np.diff(d.rowptr)
    assert np.all(lens > 0), "an empty row"
    blk = np.searchsorted(offs, d.col, side="right") - 1
    first = blk[d.rowptr[:-1]]
    rows = np.repeat(np.arange(d.num_constr), lens)
    assert np.all(blk == first[rows]), "a row over two instances"
    lin = d.row_linear != 0
    assert np.all(np.diff(first[lin]) >= 0) and np.all(np.diff(first[~lin]) >= 0)
    nb = len(offs) - 1
    m_lin = np.bincount(first[lin], minlength=nb)
    m_nl = np.bincount(first[~lin], minlength=nb)
    mmax = int(max(1, np.max(np.maximum(m_lin + cut_capacity * m_nl, m_nl))))
    nmax = int(np.max(np.diff(offs)))
    assert nmax <= 65535 and mmax <= 65535
    return (3 * nmax + 3 * mmax + (_THREADS // 64) * _Q + _Q + 8 + 16) * 8 + (max(nmax, mmax) + 4) * 4


# ---- one interface to the three references ---------------------------------------------------------------------------------------
class NLRow:
    """one NL row of a Problem in local columns: kind, cols (storage order), lb, ub, rconst and the kind's own arrays"""


def nl_rows_of(p):
    """the NL rows (row_linear == 0) of Problem p in row order: the engine's NL slots of the instance"""
    d = p.d
    lb, ub = np.asarray(p.l_constr, dtype=np.float64), np.asarray(p.u_constr, dtype=np.float64)
    out = []
    for i in np.flatnonzero(d.row_linear == 0):
        a, b = int(d.rowptr[i]), int(d.rowptr[i + 1])
        r = NLRow()
        r.index, r.kind, r.cols = int(i), int(d.row_kind[i]), d.col[a:b].astype(np.int64)
        r.lb, r.ub, r.rconst = float(lb[i]), float(ub[i]), float(d.rconst[i])
        if r.kind == L.ROW_SEP:
            r.akind, r.p0, r.p1 = d.atom_kind[a:b], d.p0[a:b], d.p1[a:b]
        elif r.kind == L.ROW_TAPE:
            t0, t1 = int(d.tape_ptr[i]), int(d.tape_ptr[i + 1])
            r.ops, r.args = d.tape_op[t0:t1], d.tape_arg[t0:t1]
        else:
            assert r.kind == L.ROW_QUAD
            q0, q1 = int(d.quad_ptr[a]), int(d.quad_ptr[b])
            r.a, r.seg_ptr, r.seg_col, r.seg_val = d.p0[a:b], d.quad_ptr[a:b + 1] - q0, d.quad_col[q0:q1], d.quad_val[q0:q1]
        out.append(r)
    return out


class CutRef:
    """exact (mpf) g, partials der[e] in storage order and cut constant b of one row at one x, with the bounds e_g, e_der[e], e_b
    of a device value against them"""

    def bound_tol(self, bnd):
        with mp.workprec(sep_ref.PREC):
            return self.e_b + 2 * mpf(U) * abs(mpf(bnd) - self.b)


def row_ref(r, x):
    R = CutRef()
    with mp.workprec(sep_ref.PREC):
        if r.kind == L.ROW_SEP:
            M = sep_ref.row_ref_mp(r.cols, r.akind, r.p0, r.p1, r.rconst, x)
            assert M.g is not None and M.b is not None, "part B rows are finite"
            R.g, R.e_g, R.der, R.b, R.e_b = M.g, M.e_g, M.der, M.b, M.e_b
            R.e_der = [2 * t for t in M.e_der]                       # (sep_ref: the partial's bound is 2 err(der))
        elif r.kind == L.ROW_QUAD:
            M = quad_ref.row_ref_mp(r.cols, r.a, r.seg_ptr, r.seg_col, r.seg_val, r.rconst, x)
            R.g, R.e_g, R.der, R.e_der, R.b, R.e_b = M.g, M.e_g, M.der, M.e_der, M.b, M.e_b
        else:
            T = tape_ref.evaluate(r.ops, r.args, x, r.rconst)
            assert T.value is not None and all(v is not None for v in T.grad.values()), "part B rows are finite"
            u, h = mpf(U), mpf(H)
            R.g = T.value
            R.e_g = 2 * T.err + 4 * u * abs(T.value)
            R.der = [T.grad.get(int(c), mpf(0)) for c in r.cols]      # (a structure column the tape never uses: exactly 0)
            R.e_der = [T.grad_tol(int(c)) for c in r.cols]
            xs = [mpf(float(x[int(c)])) for c in r.cols]
            dot = sum((xx * J for xx, J in zip(xs, R.der)), mpf(0))
            dotmag = sum((abs(xx * J) for xx, J in zip(xs, R.der)), mpf(0))
            e_dot = sum((abs(xx) * e + 2 * u * abs(xx * J) + h for xx, J, e in zip(xs, R.der, R.e_der)), mpf(0))
            e_dot += 2 * (len(r.cols) + 1) * u * dotmag
            R.b = R.g - dot
            R.e_b = R.e_g + e_dot + 2 * u * (abs(R.g) + dotmag)
    return R


def verdict(r, R, f_tol=F_TOL):
    """(+1 cut / -1 no cut / 0 undecided, exact violation max(g - ub, lb - g)): beyond f_tol by more than the bound of g -- plus
    the rounding of the device's own threshold fl(bound +- f_tol), 2u (|bound| + f_tol) -- means cut, inside by more means none"""
    with mp.workprec(sep_ref.PREC):
        best, dec = None, -1
        for bnd, v in ((r.ub, R.g - mpf(r.ub)), (r.lb, mpf(r.lb) - R.g)):
            if math.isinf(bnd):
                continue
            band = R.e_g + 2 * mpf(U) * (abs(mpf(bnd)) + mpf(f_tol))
            d = v - mpf(f_tol)
            dec = max(dec, 1 if d > band else (-1 if d < -band else 0))
            best = v if best is None else max(best, v)
    return dec, best


# ---- part B ---------------------------------------------------------------------------------------------------------------------
def _two_sided(inst, every=5):
    """the lower bounds of an instance with some NL rows made two-sided (a lower bound that never binds): (l_constr, rows)"""
    l = np.array(inst.l_constr, dtype=np.float64)
    rows = list(range(inst.m_lin + 1, inst.num_constr, every))
    l[rows] = -1e6
    return l, rows


def planted(families=("explog", "quad")):
    return [make(n=96, m_nl=12, k=k, family=f, seed=1, B=1.5) for f in families for k in (3, 16, 40)]


def smooth():
    """convex mixed-atom models without linear rows, upper- and lower-sided rows (sep_cases.convex_instance)"""
    return [sc.convex_instance(900 + s) for s in range(2)]


def _as(inst, d):
    l, _ = _two_sided(inst) if inst.m_lin else (inst.l_constr, [])
    return ktn.Problem(inst.n, inst.num_constr, inst.l_var, inst.u_var, l, inst.u_constr, inst.sense, d)


def sep_items():
    return [_as(i, ktn.SeparableNLP(i)) for i in planted() + smooth()]


def tape_items():
    from fuse_helpers import expr_problem
    return [_as(i, expr_problem(i).d) for i in planted(("explog",))[:2] + planted(("quad",))[1:] + smooth()]


def quad_items(G=None, many_rows=False):
    """planted QCQPs with every NL row a QUAD row: complete-graph cross terms on k = 3, 16, 40 columns, or (G) the segment-length
    edges of fuse_quad_cases.degree_graph on k = 2G + 7; many_rows: 70 NL rows of 8 entries next to a 12-row instance"""
    import fuse_quad_cases as FQ
    if many_rows:
        insts = [make(n=200, m_nl=70, k=8, family="quad", seed=3, B=1.5), make(n=96, m_nl=12, k=8, family="quad", seed=4, B=1.5)]
        return [_as(i, FQ.quad_rows_problem(i).d) for i in insts]
    if G is None:
        return [_as(i, FQ.quad_rows_problem(i).d) for i in planted(("quad",))]
    k = 2 * G + 7
    insts = [make(n=max(96, 2 * k), m_nl=m, k=k, family="quad", seed=920 + s, B=1.5) for s, m in enumerate((12, 5, 9))]
    return [_as(i, FQ.quad_rows_problem(i, graph=lambda kk: FQ.degree_graph(kk, G)).d) for i in insts]


def mixed_items():
    """test_gpu_batch_quad's mixed kind: per instance four cones, each a tape row, a QUAD row and a declared-linear separable row"""
    from fuse_quad_cases import cone_problem
    rng = np.random.default_rng(11)
    return [cone_problem(rng, cones=4)[0] for _ in range(4)]


MANY_TAPE_ROWS, MANY_TAPE_COLS, MANY_TAPE_CAPACITY = 1100, 64, 2


def many_tape_rows():
    """one instance with 1 100 convex tape rows a exp(b x_p) + c (x_q - d)^2 + e x_r <= ub over 64 columns (every row has slack
    0.3 at an interior point x0) next to a small planted tape instance, so that the arena and slot offsets of the second are not 0"""
    from fuse_helpers import expr_problem
    n, m = MANY_TAPE_COLS, MANY_TAPE_ROWS
    rng = np.random.default_rng(5150)
    x0 = rng.uniform(-0.5, 0.5, n)
    cost = np.where(rng.random(n) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 2.0, n)
    cons, ub = [], []
    for i in range(m):
        p, q, r = (int(c) for c in rng.choice(n, 3, replace=False))
        a, c = rng.uniform(0.5, 2.0, 2)
        b, e = rng.uniform(0.3, 1.5, 2) * rng.choice([-1.0, 1.0], 2)
        dd = float(x0[q] + rng.choice([-1.0, 1.0]) * rng.uniform(0.3, 1.5))
        cons.append(float(a) * ktn.exp(float(b) * ktn.var(p)) + float(c) * (ktn.var(q) - dd) ** 2 + float(e) * ktn.var(r))
        ub.append(float(a * math.exp(b * x0[p]) + c * (x0[q] - dd) ** 2 + e * x0[r]) + 0.3)
    obj = None
    for j in range(n):
        t = float(cost[j]) * ktn.var(j)
        obj = t if obj is None else obj + t
    big = ktn.Problem(n, m, np.full(n, -1.0), np.full(n, 1.0), np.full(m, -INF), np.asarray(ub), "Min", ktn.ExprNLP(n, obj, cons))
    return [big, expr_problem(planted(("explog",))[0])]
