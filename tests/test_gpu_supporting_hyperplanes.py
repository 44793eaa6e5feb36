"""GPU tier: supporting-hyperplane cuts (cut_algo = KTN_CUT_SUPPORTING, csrc/esh.hpp / esh.hip).

The per-row root search is checked against tests/esh_ref.py cut by cut, the rows that cannot take part against Kelley's cuts
bit for bit, the cuts' validity against the planted optimum over several rounds, and the solves end to end against the
reference's known answers and the CPU oracle."""
import json
import math
import os

import numpy as np
import pytest

import ctypes as C

import mpmath as mp

import esh_ref
import katana_jl_amd as ktn
import tape_ref
from katana_jl_amd.instances import atom_value_deriv
from helpers import (TRAJECTORY_SENSITIVE, hip_load_instance, hip_model_from_kat, instance_as_expressions,
                     oracle_solve_instance, planted_obj_bound)
from kat_util import isapprox, load_family_ext, load_kats
from test_gpu_offfamily import _check_against

pytestmark = pytest.mark.gpu
L = ktn._lib
F_TOL = 1e-6
DELTA = 10 * F_TOL
TAU = 0.1 * F_TOL                     # esh_root_tol * f_tol
ESH = dict(cut_algo="supporting_hyperplane")
ULP4 = 4 * np.finfo(float).eps
HERE = os.path.dirname(os.path.abspath(__file__))




def _rows(inst):
    rp = inst.rowptr
    out = []
    for i in range(inst.num_constr):
        s = slice(rp[i], rp[i + 1])
        out.append(esh_ref.SepRow(inst.col[s], inst.kind[s], inst.p0[s], inst.p1[s], float(inst.rconst[i])))
    return out


def _nl_rows(inst):
    return list(range(inst.m_lin, inst.num_constr))


def _first_round(m):
    m.optimize_begin()
    M0 = m.lp_num_rows()
    m.ecp_step()
    return m.getsolution()[:m._n0], m.lp_rows_from(M0), m.last_sweep_slots()


def _kelley_first_round(inst, l_constr=None, d=None):
    m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))
    m.loadproblem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr if l_constr is None else l_constr, inst.u_constr,
                  inst.sense, ktn.SeparableNLP(inst) if d is None else d)
    return m, _first_round(m)


def _cut(rows_from, k):
    rp, col, val, lo, hi = rows_from
    return col[rp[k]:rp[k + 1]], val[rp[k]:rp[k + 1]], lo[k], hi[k]


def _check_separable_cut(row, xi, xs, lam, bound, a, hi):
    """the cut of an upper-side separable row taken at x_b = x_int + lam (x* - x_int): 0 <= phi(lam) <= tau (mpmath), the
    coefficients grad g(x_b) within 4 ulp, the constant within 1e-13 of the sum of its terms"""
    xb = xi + lam * (xs - xi)                                   # (the kernel's own operations: the same point bit for bit)
    val, der = atom_value_deriv(np.asarray(row.kinds, dtype=np.uint8), np.asarray(row.p0), np.asarray(row.p1), xb[row.cols])
    assert np.all(np.abs(a - der) <= ULP4 * np.abs(der) + 1e-300), np.max(np.abs(a - der) / np.abs(der))
    g = float(np.sum(val)) + row.rconst
    const = g - float(np.sum(xb[row.cols] * der))
    terms = float(np.sum(np.abs(val)) + abs(row.rconst) + np.sum(np.abs(xb[row.cols] * der)) + abs(bound))
    assert abs((bound - hi) - const) <= 1e-13 * terms, (bound - hi, const, terms)
    f = esh_ref.phi(row, xi, xs, 1, bound, lam, mp)[0]
    assert -1e-13 * terms <= float(f) <= TAU + 1e-13 * terms, float(f)
    # x* violates the cut, x_int satisfies it with room to spare
    assert a @ xs[row.cols] > hi and a @ xi[row.cols] <= hi - 0.5 * DELTA


@pytest.mark.parametrize("family,k", [("quad", 64), ("explog", 32)])
def test_first_round_cuts_touch_the_rows_where_the_segment_leaves_them(family, k):
    inst = ktn.instances.make_instance(n=4000, m_nl=400, k=k, family=family, seed=0)
    mk, (xk, rk, sk) = _kelley_first_round(inst)
    m = hip_load_instance(ktn, inst, **ESH)
    xs, rows_from, slots = _first_round(m)
    lams = m.last_sweep_lambdas()
    assert np.array_equal(xs, xk) and np.array_equal(slots, sk)          # the same first LP point and violated rows
    assert m.stat("esh_interior_found") == 1 and m.stat("esh_interior_depth") >= DELTA
    xi = m.interior_point()
    rows, nl = _rows(inst), _nl_rows(inst)
    n_esh = n_kelley = 0
    for k_, s in enumerate(slots):
        i = nl[int(s)]
        cols, a, lo, hi = _cut(rows_from, k_)
        assert np.array_equal(cols, rows[i].cols)
        lam = float(lams[k_])
        assert 0.0 < lam <= 1.0
        if lam == 1.0:                                           # Kelley's cut: the one the Kelley handle emitted, bit for bit
            n_kelley += 1
            kc = _cut(rk, k_)
            assert np.array_equal(kc[1], a) and kc[2] == lo and kc[3] == hi, i
            continue
        n_esh += 1
        _check_separable_cut(rows[i], xi, xs, lam, inst.u_constr[i], a, hi)
    # the kernels' own counters against the cuts counted here
    assert n_esh > 0 and n_esh == m.stat("esh_rows") and n_kelley == m.stat("esh_fallback_rows")


def test_tape_rows_cut_where_the_separable_rows_do():
    inst = ktn.instances.make_instance(n=1500, m_nl=150, k=32, family="explog", seed=1)
    obj, cons = instance_as_expressions(ktn, inst)
    out = []
    xi = None
    for d in (ktn.SeparableNLP(inst), ktn.ExprNLP(inst.n, obj, cons)):
        m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, **ESH))
        m.loadproblem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr, inst.u_constr, inst.sense, d)
        if xi is None:
            xi = m.interior_point()
        else:
            m.set_interior_point(xi)                            # (the same x_int for both forms)
        out.append((m, _first_round(m), m.last_sweep_lambdas()))
    (ms, (xs_s, rs, ss), ls), (mt, (xs_t, rt, st), lt) = out
    assert np.array_equal(xs_s, xs_t) and np.array_equal(ss, st)
    assert ms.stat("esh_rows") > 0 and ms.stat("esh_rows") == mt.stat("esh_rows")
    assert np.all(np.abs(ls - lt) <= TAU)
    for a, b in zip(rs, rt):
        assert np.allclose(a, b, rtol=1e-12, atol=1e-12 * max(1.0, float(np.max(np.abs(a))) if len(a) else 1.0))


def _cone_family(nrows, nlog, seed=0):
    """nrows copies of sqrt(x^2 + y^2) <= z - 0.25 (the docs' cone, through POWC and SQRT) and nlog concave rows
    log(w) >= lb (lower side), every row on its own variables; min sum z + 0.3 x - 0.2 y + sum w"""
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


def test_convex_tape_family_with_a_concave_lower_side_row_cut_by_cut():
    nrows, nlog = 10000, 1000
    n, d, lv, uv, lb, ub = _cone_family(nrows, nlog)
    m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, **ESH))
    m.loadproblem(n, len(lb), lv, uv, lb, ub, "Min", d)
    # The engine's own search finds no point here: the child's LP leaves x = y = 0, where sqrt(x^2 + y^2)
    # has no finite gradient, and its sweep ends :Error.  The caller's point is used.
    assert m.interior_point() is None and m.stat("esh_interior_found") == 0
    x0 = np.zeros(n)
    x0[2:3 * nrows:3] = 4.0                                      # z = 4, x = y = 0.5: 4 - 0.25 - sqrt(0.5) inside
    x0[0:3 * nrows:3] = 0.5
    x0[1:3 * nrows:3] = 0.5
    x0[3 * nrows:] = 4.0                                         # log(4) > 0.5 >= lb
    m.set_interior_point(x0)
    xs, rows_from, slots = _first_round(m)
    lams = m.last_sweep_lambdas()
    xi = m.interior_point()
    assert np.array_equal(xi, x0) and m.stat("esh_interior_depth") >= DELTA
    sides = {1: 0, -1: 0}
    for k_, s in enumerate(slots):
        i = int(s)                                               # (every row is nonlinear: slot == row)
        lam = float(lams[k_])
        if lam == 1.0:
            continue
        side = 1 if math.isfinite(ub[i]) else -1
        bound = ub[i] if side > 0 else lb[i]
        cols, a, lo, hi = _cut(rows_from, k_)
        xb = xi + lam * (xs - xi)
        ops = d.tape_op[d.tape_ptr[i]:d.tape_ptr[i + 1]]
        args = d.tape_arg[d.tape_ptr[i]:d.tape_ptr[i + 1]]
        ref = tape_ref.evaluate(ops, args, xb, rconst=float(d.rconst[i]))
        ref.check_grad({int(c): float(v) for c, v in zip(cols, a)}, i)
        with mp.workprec(200):
            phi = side * (ref.value - mp.mpf(bound))
            const = ref.value - sum(mp.mpf(float(xb[int(c)])) * ref.grad[int(c)] for c in cols)
            slack = 2 * ref.err + sum(ref.grad_tol(int(c)) * abs(float(xb[int(c)])) for c in cols)
            terms = abs(ref.value) + sum(abs(mp.mpf(float(xb[int(c)])) * ref.grad[int(c)]) for c in cols) + abs(bound)
            got = mp.mpf(bound) - mp.mpf(float(hi if side > 0 else lo))
            assert -2 * ref.err <= phi <= TAU + 2 * ref.err, (i, float(phi))
            assert abs(got - const) <= slack + 1e-13 * terms, (i, float(got), float(const))
        # x* violates the cut, x_int satisfies it
        if side > 0:
            assert a @ xs[cols] > hi and a @ xi[cols] <= hi - 0.5 * DELTA
        else:
            assert a @ xs[cols] < lo and a @ xi[cols] >= lo + 0.5 * DELTA
        sides[side] += 1
    assert sides[1] > 0 and sides[-1] > 0, sides
    assert sides[1] + sides[-1] == m.stat("esh_rows")


class _HostRowsNLP(ktn.NLPDescription):
    """a separable description whose rows in `host_rows` are evaluated by the caller (KTN_ROW_HOST) from the same atoms"""

    def __init__(self, inst, host_rows, obj_quad):
        base = ktn.SeparableNLP(inst)
        rk = base.row_kind.copy()
        rk[host_rows] = L.ROW_HOST
        k = len(inst.obj_col)
        super().__init__(inst.n, base.rowptr, base.col, rk, base.row_linear, base.rconst, base.atom_kind, base.p0, base.p1,
                         obj_linear=False, obj_kind=L.ROW_SEP,
                         obj_col=np.concatenate([inst.obj_col, np.arange(inst.n)]),
                         obj_atom_kind=np.concatenate([inst.obj_kind, np.full(inst.n, L.ATOM_QUAD)]),
                         obj_p0=np.concatenate([inst.obj_p0, np.full(inst.n, obj_quad)]),
                         obj_p1=np.concatenate([inst.obj_p1, np.zeros(inst.n)]), obj_const=inst.obj_const)
        rp, nnz, m, n = self.rowptr, len(self.col), self.num_constr, self.num_var
        hr = list(host_rows)

        def rows_cb(_user, xp, gp, jp):
            try:
                xv = np.ctypeslib.as_array(xp, (n,)).copy()
                g = np.ctypeslib.as_array(gp, (m,))
                J = np.ctypeslib.as_array(jp, (nnz,))
                for i in hr:
                    s = slice(rp[i], rp[i + 1])
                    val, der = atom_value_deriv(self.atom_kind[s], self.p0[s], self.p1[s], xv[self.col[s]])
                    g[i] = float(np.sum(val)) + self.rconst[i]
                    J[s] = der
                return 0
            except Exception:
                return 1
        self._rows_cb = L.EVAL_ROWS_CB(rows_cb)

    def c_struct(self):
        d = super().c_struct()
        d.eval_rows = C.cast(self._rows_cb, C.c_void_p)
        return d


def test_rows_that_cannot_take_part_keep_kelleys_cut_bit_for_bit():
    """host rows, nonlinear equalities, two-sided rows, the epigraph row of a nonlinear objective and rows the caller's point
    does not hold 10 f_tol inside: every one of them gets the cut the Kelley handle gives it, bit for bit"""
    inst = ktn.instances.make_instance(n=1000, m_nl=100, k=16, family="explog", seed=2)
    nl = _nl_rows(inst)
    host_rows, eq_rows, two_sided = nl[1::7], nl[2::7], nl[3::7]
    l_constr = inst.l_constr.copy()
    l_constr[two_sided] = -1e6
    l_constr[eq_rows] = inst.u_constr[eq_rows]                  # nonlinear equalities (not convex: never searched)
    # a point with many violated rows: the LP point of a Kelley handle's first round (incl. the epigraph variable); both
    # handles then sweep at exactly that point through the separator API
    probe = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))
    probe.loadproblem(inst.n, inst.num_constr, inst.l_var, inst.u_var, l_constr, inst.u_constr, inst.sense,
                      _HostRowsNLP(inst, host_rows, 1e-3))
    probe.optimize_begin()
    probe.ecp_step()
    xfull = probe.getsolution()
    res = []
    for algo in ("kelley", "supporting_hyperplane"):
        d = _HostRowsNLP(inst, host_rows, 1e-3)
        m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, cut_algo=algo))
        m.loadproblem(inst.n, inst.num_constr, inst.l_var, inst.u_var, l_constr, inst.u_constr, inst.sense, d)
        if algo != "kelley":
            m.set_interior_point(inst.xhat)                      # the planted optimum: not interior for its active rows
        M0 = m.lp_num_rows()
        sep = ktn.KatanaHipSeparator(m)
        sep.initialize()
        sep.precompute(xfull)
        sep.sweep(F_TOL)
        res.append((m, (None, m.lp_rows_from(M0), m.last_sweep_slots()), m.last_sweep_lambdas(), d))
        if algo != "kelley":
            assert m.stat("esh_interior_found") == 1 and m.stat("esh_interior_rounds") == 0
    (mk, (_, rk, sk), _, _), (me, (_, re_, se), lams, d) = res
    assert np.array_equal(sk, se) and len(se) > 0
    rows = _rows(inst)
    g_int = np.array([rows[i].eval(inst.xhat)[0] for i in range(inst.num_constr)])
    m0 = inst.num_constr
    nl_all = nl + [m0]                                            # (NL slots: the constraint rows, then the epigraph row)
    seen = {"host": 0, "equality": 0, "two_sided": 0, "epigraph": 0, "not_interior": 0}
    n_kelley = 0
    for k_, s in enumerate(se):
        i = nl_all[int(s)]
        cls = ("epigraph" if i == m0 else "host" if i in host_rows else "equality" if i in eq_rows else
               "two_sided" if i in two_sided else "not_interior" if not (inst.u_constr[i] - g_int[i] >= DELTA) else None)
        if lams[k_] == 1.0:
            n_kelley += 1
            kc, ec = _cut(rk, k_), _cut(re_, k_)
            assert np.array_equal(kc[0], ec[0]) and np.array_equal(kc[1], ec[1]) and kc[2] == ec[2] and kc[3] == ec[3], i
        if cls is not None:
            seen[cls] += 1
            assert lams[k_] == 1.0, (cls, i)                        # never searched
    assert all(v > 0 for v in seen.values()), seen
    assert n_kelley == me.stat("esh_fallback_rows") and len(se) - n_kelley == me.stat("esh_rows") > 0


@pytest.mark.parametrize("family,k", [("quad", 64), ("explog", 32)])
def test_every_cut_of_several_rounds_keeps_the_planted_optimum(family, k):
    inst = ktn.instances.make_instance(n=3000, m_nl=300, k=k, family=family, seed=3, bound_frac=0.5)
    m = hip_load_instance(ktn, inst, **ESH)
    m.optimize_begin()
    M0 = m.lp_num_rows()
    for _ in range(8):
        if m.ecp_step():
            break
        assert m.getobjval() <= inst.opt_obj + planted_obj_bound(inst)
    rp, col, val, lo, hi = m.lp_rows_from(M0)
    ax = np.array([val[rp[r]:rp[r + 1]] @ inst.xhat[col[rp[r]:rp[r + 1]]] for r in range(len(hi))])
    scale = 1.0 + np.abs(hi)
    assert np.all(ax <= hi + 1e-9 * scale), float(np.max((ax - hi) / scale))
    assert m.stat("esh_rows") > 0


KATS = load_kats()


@pytest.mark.parametrize("m", KATS, ids=[m["id"] for m in KATS])
def test_reference_kat_with_supporting_hyperplanes(m):
    M = hip_model_from_kat(ktn, m, **ESH)
    status = M.solve()
    e = m["expect"]
    assert status == e["status"]
    obj = M.getobjectivevalue()
    assert isapprox(obj, e["obj"], e["obj_atol"], e["obj_rtol"]), (obj, e["obj"])
    if e["x"] is not None:
        x = M.getvalue()
        tol = 3e-3 if m["id"] in TRAJECTORY_SENSITIVE else e["sol_atol"]
        for got, want in zip(x, e["x"]):
            assert isapprox(got, want, tol, tol), (list(x), e["x"])


EXT = load_family_ext()


@pytest.mark.parametrize("m", EXT, ids=[m["id"] for m in EXT])
def test_ball_family_takes_no_more_rounds_than_kelley(m):
    rounds = []
    for algo in ("kelley", "supporting_hyperplane"):
        M = hip_model_from_kat(ktn, m, cut_algo=algo)
        assert M.solve() == m["expect"]["status"]
        obj = M.getobjectivevalue()
        assert isapprox(obj, m["expect"]["obj"], 1e-6, 1e-6), (algo, obj, m["expect"]["obj"])
        rounds.append(M.internal_model.numiters())
    print("%s kelley %d rounds, supporting hyperplanes %d" % (m["id"], rounds[0], rounds[1]))
    assert rounds[1] <= rounds[0]


def _both_ways(inst, ref_obj):
    """Kelley and supporting hyperplanes on one instance, each checked as tests/test_gpu_offfamily.py checks the engine;
    returns the ECP rounds of each"""
    rounds = {}
    for algo in ("kelley", "supporting_hyperplane"):
        m = hip_load_instance(ktn, inst, cut_algo=algo)
        m.optimize()
        _check_against(inst, m, ref_obj)
        rounds[algo] = m.numiters()
    print("rounds", rounds)
    return rounds


def _assert_rounds(case, rounds):
    """fewer rounds than Kelley, except on the cases where the first MI355X run measured more: there at
    most twice Kelley's"""
    if case in MORE_ROUNDS:
        assert rounds["supporting_hyperplane"] <= 2 * rounds["kelley"], (case, rounds)
    else:
        assert rounds["supporting_hyperplane"] < rounds["kelley"], (case, rounds)


# The off-vertex cases of tests/test_gpu_offfamily.py, same shapes.  First MI355X run, rounds Kelley -> supporting hyperplanes:
#   explog n 50 bf 0    267 -> 193, 229 -> 144      quad n 50 bf 0    2230 -> 426, 797 -> 1060
#   explog n 50 bf 0.5   77 ->  70, 121 -> 191      quad n 50 bf 0.5   138 ->  68,  85 ->   72
#   explog n 100 bf 0.5 221 -> 158, 250 -> 349      quad n 100 bf 0.5  371 -> 237, 402 ->  275
#   explog n 200 bf 0.5 192 -> 191, 331 -> 326      (seeds 0, 1)
OFF_SMALL = [dict(n=50, m_nl=5, k=8, family=f, seed=s, bound_frac=b) for f in ("explog", "quad") for b in (0.0, 0.5) for s in (0, 1)] + \
            [dict(n=100, m_nl=10, k=16, family=f, seed=s, bound_frac=0.5) for f in ("explog", "quad") for s in (0, 1)]
OFF_IDS = ["%(family)s_n%(n)d_bf%(bound_frac)g_s%(seed)d" % c for c in OFF_SMALL]
MORE_ROUNDS = {"explog_n50_bf0.5_s1", "quad_n50_bf0_s1", "explog_n100_bf0.5_s1"}


@pytest.mark.parametrize("spec", OFF_SMALL, ids=OFF_IDS)
def test_off_vertex_models_against_the_oracle_with_supporting_hyperplanes(spec):
    inst = ktn.instances.make_instance(**spec)
    rounds = _both_ways(inst, oracle_solve_instance(inst).getobjval())
    _assert_rounds("%(family)s_n%(n)d_bf%(bound_frac)g_s%(seed)d" % spec, rounds)


@pytest.mark.parametrize("family,seed", [("explog", 0), ("explog", 1)])
def test_half_pinned_models_of_200_variables_against_the_committed_oracle_with_supporting_hyperplanes(family, seed):
    fx = json.load(open(os.path.join(HERE, "golden", "offfamily_oracle.json")))
    case = next(c for c in fx["cases"] if c["n"] == 200 and c["family"] == family and c["seed"] == seed and c["bound_frac"] == 0.5)
    inst = ktn.instances.make_instance(n=200, m_nl=20, k=16, family=family, seed=seed, bound_frac=0.5)
    rounds = _both_ways(inst, case["objective"])
    _assert_rounds("%s_n200_bf0.5_s%d" % (family, seed), rounds)


def test_gencut_gives_the_sweeps_cut_and_leaves_the_precompute_alone():
    inst = ktn.instances.make_instance(n=1000, m_nl=100, k=16, family="quad", seed=6)
    m = hip_load_instance(ktn, inst, **ESH)
    xs, rows_from, slots = _first_round(m)
    lams = m.last_sweep_lambdas()
    sep = ktn.KatanaHipSeparator(m)
    sep.initialize()
    sep.precompute(m.getsolution())
    jac0, g0 = sep.jac.copy(), sep.g.copy()
    nl = _nl_rows(inst)
    moved = 0
    for k_, s in enumerate(slots):
        if lams[k_] == 1.0:
            continue
        i = nl[int(s)]
        cols, coefs, const = sep.gencut(xs, None, i)
        c_, a, lo, hi = _cut(rows_from, k_)
        assert np.array_equal(cols, c_) and np.array_equal(coefs, a), i
        assert abs((inst.u_constr[i] - hi) - const) <= 1e-13 * (abs(const) + abs(inst.u_constr[i]) + 1.0), i
        moved += 1
        if moved == 20:
            break
    assert moved > 0
    jac = np.zeros(max(sep.nnz, 1))
    L.check(m._h, m._lib.ktn_sep_get_jac(m._h, jac.ctypes.data_as(C.POINTER(C.c_double)), sep.nnz))
    assert np.array_equal(jac[:sep.nnz], jac0)


def test_no_strictly_interior_point_gives_kelleys_answer():
    # x^2 + y^2 <= 0: the feasible set is a point, nothing is strictly inside
    def build(algo):
        M = ktn.Model(solver=ktn.KatanaSolver(log_level=0, cut_algo=algo))
        x, y = M.variable(-1.0, 1.0), M.variable(-1.0, 1.0)
        M.objective("Min", x + y, linear=True)
        M.constraint((x ** 2 + y ** 2, -math.inf, 0.0), linear=False)
        return M
    out = []
    for algo in ("kelley", "supporting_hyperplane"):
        M = build(algo)
        st = M.solve()
        out.append((st, M.getobjectivevalue(), M.internal_model))
    assert out[1][2].interior_point() is None and out[1][2].stat("esh_interior_found") == 0
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]


def test_caller_point_is_used_as_given_and_reported_back():
    inst = ktn.instances.make_instance(n=400, m_nl=40, k=8, family="quad", seed=4)
    m = hip_load_instance(ktn, inst, **ESH)
    xi = np.zeros(inst.n) if np.all(inst.l_var <= 0) and np.all(inst.u_var >= 0) else 0.5 * (inst.l_var + inst.u_var)
    m.set_interior_point(xi)
    assert np.array_equal(m.interior_point(), xi)
    assert m.stat("esh_interior_rounds") == 0
    m.optimize()
    assert m.status() == "Optimal"
    assert np.array_equal(m.interior_point(), xi)
    m.set_interior_point(None)
    found = m.interior_point()
    assert found is not None and m.stat("esh_interior_found") == 1 and m.stat("esh_interior_depth") >= DELTA


def test_unsupported_combinations_are_refused():
    inst = ktn.instances.make_instance(n=200, m_nl=20, k=4, family="explog", seed=5)
    m = hip_load_instance(ktn, inst, **ESH)
    m.set_blocks([0, inst.n])
    with pytest.raises(L.KatanaHipError) as e:
        m.optimize_blocks()
    assert e.value.code == L.E_UNSUPPORTED
    m2 = hip_load_instance(ktn, inst, **ESH)
    m2.lp_enable_global_lists(inst.m_nl)
    cb = L.EXCHANGE_CB(lambda *a: 0)
    with pytest.raises(L.KatanaHipError) as e:
        m2.set_cut_exchange(cb, 0)
    assert e.value.code == L.E_UNSUPPORTED
    with pytest.raises(L.KatanaHipError) as e:
        ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, cut_algo=7))
    assert e.value.code == L.E_INVALID
