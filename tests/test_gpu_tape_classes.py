"""GPU tier: tape rows evaluated by shape class (k_tape_classed) against the row interpreter (k_tape_eval + k_gj_stats).

The contract is bit identity: every case loads the same model on two (or three) handles made under different settings of
KTN_TAPE_CLASSED (0 = interpreter for every tape row, -1 = classes of >= 64 rows, 1 = classes of >= 2 rows) and compares 100 %
of the rows bit for bit (uint64 views, so NaN patterns and signed zeros count).  Accuracy against references uses the
suite's existing rules: Jacobian entries 4 ulp and g 1e-13 * sum|terms| against a float64 numpy formula, the derived bounds
of tests/tape_ref.py against mpmath on samples."""
import math

import numpy as np
import pytest

import katana_jl_amd as ktn
import tape_ref
import tape_class_cases as T
from helpers import assert_planted_objective, instance_as_expressions

pytestmark = pytest.mark.gpu
L = ktn._lib
ULP4 = 4 * np.finfo(float).eps
INF = math.inf


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_bits(a, b, what):
    a, b = bits(np.asarray(a)), bits(np.asarray(b))
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not np.array_equal(a, b):
        bad = np.flatnonzero(a != b)
        raise AssertionError((what, "differs at", bad[:8], "of", len(bad)))


def handle(monkeypatch, setting, d, n, m, lb=None, ub=None, lv=-INF, uv=INF, **kw):
    monkeypatch.setenv("KTN_TAPE_CLASSED", str(setting))
    model = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, **kw))
    model.loadproblem(n, m, np.full(n, lv) if np.isscalar(lv) else lv, np.full(n, uv) if np.isscalar(uv) else uv,
                      np.full(m, -INF) if lb is None else lb, np.zeros(m) if ub is None else ub, "Min", d)
    sep = ktn.KatanaHipSeparator(model)
    sep.initialize()
    return model, sep


def stats(model):
    return {k: int(model.stat("tape_" + k)) for k in ("classes", "classed_rows", "interp_rows", "class_max_nodes")}


def compare_precompute_and_sweep(handles, x, f_tol=1e-6):
    """precompute at x, then one sweep, on every handle: everything the first handle gives, bit for bit"""
    out = []
    for model, sep in handles:
        sep.precompute(x)
        g, jac = sep.g.copy(), sep.jac.copy()
        m0 = model.lp_num_rows()
        nv, mv = sep.sweep(f_tol)
        out.append((g, jac, nv, mv, model.lp_rows_from(m0), model.status()))
    g0, j0, nv0, mv0, rows0, st0 = out[0]
    for k, (g, jac, nv, mv, rows, st) in enumerate(out[1:]):
        assert_bits(g0, g, ("g", k))
        assert_bits(j0, jac, ("jac", k))
        assert nv == nv0 and st == st0, (k, nv, nv0, st, st0)
        assert_bits(np.array([mv0]), np.array([mv]), ("maxviol", k))
        for name, a, b in zip(("rowptr", "col", "val", "lo", "hi"), rows0, rows):
            assert_bits(a, b, ("lp rows " + name, k))
    return out[0]


def check_formula(sep, shape, rows, cols, x):
    """all `rows` of one shape against its float64 formula: Jacobian 4 ulp, g 1e-13 * sum|terms|"""
    g, mag, J = shape.f64(x[cols])
    assert np.all(np.abs(sep.g[rows] - g) <= 1e-13 * mag), shape.name
    at = sep.rowptr[rows][:, None] + np.arange(shape.nv)
    assert np.array_equal(sep.col[at], cols)
    assert np.all(np.abs(sep.jac[at] - J) <= ULP4 * np.abs(J) + 1e-300), shape.name


def check_mpmath(sep, d, x, sample):
    for i in sample:
        a, b = d.tape_ptr[i], d.tape_ptr[i + 1]
        ref = tape_ref.evaluate(d.tape_op[a:b], d.tape_arg[a:b], x, rconst=float(d.rconst[i]))
        ref.check_value(float(sep.g[i]), i)
        by = {}
        for e in range(sep.rowptr[i], sep.rowptr[i + 1]):
            c = int(sep.col[e])
            if c in by:
                assert sep.jac[e] == 0.0, ("duplicated structure entry not 0", i, c)
                continue
            by[c] = float(sep.jac[e])
        ref.check_grad(by, i)


# ---- a. the docs' cone family ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [10000, 1000000])
def test_cone_family_is_one_class_and_bit_equal_to_the_interpreter(monkeypatch, m):
    assert T.CONE.names() == T.CONE_NODES
    rng = np.random.default_rng(17)
    n = 100000
    cols = T.distinct_columns(rng, m, n)
    x = T.signed_point(rng, n)
    d = T.assemble(n, m, [dict(rows=np.arange(m), cols=cols, shape=T.CONE)])
    hs = [handle(monkeypatch, s, d, n, m) for s in (0, -1)]
    assert stats(hs[0][0]) == dict(classes=0, classed_rows=0, interp_rows=m, class_max_nodes=0)
    assert stats(hs[1][0]) == dict(classes=1, classed_rows=m, interp_rows=0, class_max_nodes=10)
    g, jac, nv, mv, rows, st = compare_precompute_and_sweep(hs, x)
    sep = hs[1][1]
    sep.precompute(x)
    check_formula(sep, T.CONE, np.arange(m), cols, x)
    check_mpmath(sep, d, x, np.sort(rng.choice(m, 500, replace=False)))
    assert nv == int(np.sum(sep.g > 1e-6)) and 0 < nv < m


# ---- b. three shapes interleaved, separable LIN rows in between -----------------------------------------------------------
def test_three_interleaved_shapes_with_separable_rows_in_between(monkeypatch):
    rng = np.random.default_rng(23)
    n, m_tape = 100000, 300000
    period = 4                                                        # rows 4q, 4q+1, 4q+2: tape rows, 4q+3: a LIN row
    m = m_tape // 3 * period
    allrows = np.arange(m)
    tape_rows = allrows[allrows % period != 3]
    assert len(tape_rows) == m_tape
    shapes = (T.CONE, T.QUAD3, T.EXPO)
    groups = []
    for k, s in enumerate(shapes):
        rows = tape_rows[k::3]                                        # tape row t has shape t % 3
        groups.append(dict(rows=rows, cols=T.distinct_columns(rng, len(rows), n), shape=s))
    lin = allrows[allrows % period == 3]
    groups.append(dict(rows=lin, cols=T.distinct_columns(rng, len(lin), n), coef=rng.uniform(-1.0, 1.0, (len(lin), 3))))
    assert len(tape_rows[0::3]) % 64 != 0                             # partial last wavefronts
    x = T.signed_point(rng, n)
    d = T.assemble(n, m, groups)
    hs = [handle(monkeypatch, s, d, n, m, ub=np.where(allrows % period == 3, 1e3, 0.0)) for s in (0, -1)]
    assert stats(hs[1][0]) == dict(classes=3, classed_rows=m_tape, interp_rows=0, class_max_nodes=10)
    assert stats(hs[0][0])["classed_rows"] == 0 and stats(hs[0][0])["interp_rows"] == m_tape
    g, jac, nv, mv, rows, st = compare_precompute_and_sweep(hs, x)
    sep = hs[1][1]
    sep.precompute(x)
    for gr in groups[:3]:
        check_formula(sep, gr["shape"], gr["rows"], gr["cols"], x)
    check_mpmath(sep, d, x, np.sort(rng.choice(tape_rows, 500, replace=False)))
    assert 0 < nv < m_tape


# ---- c. every opcode and its edges, each row a class of 64 + 7 ------------------------------------------------------------
def test_every_opcode_edge_row_as_a_class_with_a_partial_second_wavefront(monkeypatch):
    copies = 64 + 7
    R = T.Rows()
    for _ in range(copies):
        T.edge_rows(R)
    per = len(R.rows) // copies
    x = np.asarray(R.x)
    d = R.desc()
    m = len(R.rows)
    hs = [handle(monkeypatch, s, d, len(x), m) for s in (0, -1)]
    s1 = stats(hs[1][0])
    assert s1["classed_rows"] == m and s1["interp_rows"] == 0 and 0 < s1["classes"] <= per
    compare_precompute_and_sweep(hs, x)
    sep = hs[1][1]
    sep.precompute(x)
    nonfinite = 0
    for i in list(range(per)) + list(range(m - per, m)):              # the first copy (lane 0 of wavefront 0) and the last (lane 6 of wavefront 1)
        r = R.rows[i]
        ref = tape_ref.evaluate(r.ops, r.args, x, rconst=r.rconst)
        ref.check_value(float(sep.g[i]), (i, r.what))
        by = {}
        for e in range(sep.rowptr[i], sep.rowptr[i + 1]):
            c = int(sep.col[e])
            if c in by:
                assert sep.jac[e] == 0.0, ("duplicated structure entry not 0", i, r.what)
                continue
            by[c] = float(sep.jac[e])
        ref.check_grad(by, (i, r.what))
        nonfinite += int(not np.all(np.isfinite(sep.jac[sep.rowptr[i]:sep.rowptr[i + 1]])) or not np.isfinite(sep.g[i]))
    assert nonfinite >= 2                                             # the edges are in there


# ---- d. thresholds ------------------------------------------------------------------------------------------------------
def test_class_size_thresholds_under_the_three_settings(monkeypatch):
    rng = np.random.default_rng(31)
    sizes = [1, 2, 63, 64, 65, 128]
    shapes = [T.Shape("pow%d" % p, 2, (lambda p: lambda v: v[0] ** float(p) + v[1] - 1.0)(p), None) for p in range(3, 9)]
    m = sum(sizes)
    n = 2 * m
    shape_of = rng.permutation(np.repeat(np.arange(6), sizes))        # the classes' members scattered over the rows
    cols = np.arange(n).reshape(m, 2)
    groups = [dict(rows=np.flatnonzero(shape_of == k), cols=cols[shape_of == k], shape=shapes[k]) for k in range(6)]
    d = T.assemble(n, m, groups)
    x = rng.uniform(0.5, 1.5, n)
    hs = [handle(monkeypatch, s, d, n, m) for s in (0, -1, 1)]
    assert stats(hs[0][0]) == dict(classes=0, classed_rows=0, interp_rows=m, class_max_nodes=0)
    nodes = len(shapes[0].ops)
    assert stats(hs[1][0]) == dict(classes=3, classed_rows=64 + 65 + 128, interp_rows=1 + 2 + 63, class_max_nodes=nodes)
    assert stats(hs[2][0]) == dict(classes=5, classed_rows=m - 1, interp_rows=1, class_max_nodes=nodes)
    compare_precompute_and_sweep(hs, x)
    check_mpmath(hs[1][1], d, x, range(m))
    hs[2][1].precompute(x)
    check_mpmath(hs[2][1], d, x, range(m))


# ---- e. a non-finite coefficient in a violated classed row ----------------------------------------------------------------
@pytest.mark.parametrize("violated", [True, False])
def test_non_finite_coefficient_in_a_classed_row_ends_in_error_only_when_the_row_is_violated(monkeypatch, violated):
    m, n = 200, 600
    cols = np.arange(n).reshape(m, 3)
    x = np.tile([0.6, 0.8, 2.0], m)                                   # 1 - (2 - 0.25) < 0: satisfied
    x[3 * 77:3 * 77 + 3] = [0.0, 0.0, -1.0 if violated else 2.0]      # 0 - (z - 0.25); the partials 0.5 / 0 * 0 are NaN
    d = T.assemble(n, m, [dict(rows=np.arange(m), cols=cols, shape=T.CONE)])
    hs = [handle(monkeypatch, s, d, n, m) for s in (0, -1)]
    assert stats(hs[1][0])["classed_rows"] == m
    g, jac, nv, mv, rows, st = compare_precompute_and_sweep(hs, x)
    assert np.isnan(jac[3 * 77]) and np.isnan(jac[3 * 77 + 1])
    assert nv == (1 if violated else 0)
    for model, _ in hs:
        assert (model.status() == "Error") == violated


# ---- f. a class beyond the LDS budget stays with the interpreter ----------------------------------------------------------
def test_a_class_beyond_the_lds_budget_stays_with_the_interpreter(monkeypatch):
    rng = np.random.default_rng(37)
    terms, m = 300, 70

    def fold(v):
        e = v[0] ** 2
        for j in range(1, terms):
            e = e + v[j] ** 2
        return e - 50.0
    s = T.Shape("sum300", terms, fold, None)
    n = 5000
    cols = T.distinct_columns(rng, m, n, terms)
    x = rng.uniform(-1.0, 1.0, n)
    d = T.assemble(n, m, [dict(rows=np.arange(m), cols=cols, shape=s)])
    hs = [handle(monkeypatch, k, d, n, m) for k in (0, -1, 1)]
    for model, _ in hs:                                               # 2 * 900 nodes + 300 entries > 312 cells: the interpreter's
        assert stats(model) == dict(classes=0, classed_rows=0, interp_rows=m, class_max_nodes=0)
    assert hs[1][0].stat("tape_shapes") == 1
    compare_precompute_and_sweep(hs, x)
    check_mpmath(hs[1][1], d, x, [0, 35, 69])


# ---- g. whole solves, bit for bit -----------------------------------------------------------------------------------------
def _solve_pair(monkeypatch, settings, make):
    out = []
    for s in settings:
        monkeypatch.setenv("KTN_TAPE_CLASSED", str(s))
        out.append(make())
    (ma, sa), (mb, sb) = out
    assert sa == sb, (sa, sb)
    assert ma.numiters() == mb.numiters() and ma.numcuts() == mb.numcuts()
    assert_bits(np.array([ma.getobjval()]), np.array([mb.getobjval()]), "objval")
    assert_bits(ma.getsolution(), mb.getsolution(), "x")
    return out


def test_quad_instance_through_expressions_solves_the_same_bit_for_bit(monkeypatch):
    inst = ktn.instances.make_instance(n=2000, m_nl=200, k=16, family="quad", seed=9, objective="quad")
    obj, cons = instance_as_expressions(ktn, inst)

    def make():
        model = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))
        model.loadproblem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr, inst.u_constr, inst.sense,
                          ktn.ExprNLP(inst.n, obj, cons))
        return model, model.optimize()
    (ma, sa), (mb, sb) = _solve_pair(monkeypatch, (0, -1), make)
    assert sa == "Optimal"
    assert stats(ma)["classed_rows"] == 0
    assert stats(mb) == dict(classes=1, classed_rows=inst.m_nl, interp_rows=1, class_max_nodes=int(mb.stat("tape_class_max_nodes")))
    assert_planted_objective(ma.getobjval(), inst)
    assert_planted_objective(mb.getobjval(), inst)


def test_docs_model_in_ten_blocks_solves_to_the_known_optimum_on_both_paths(monkeypatch):
    def make():
        M = T.docs_model(10, ktn.KatanaSolver(log_level=0))
        st = M.solve()
        return M.internal_model, st
    (ma, sa), (mb, sb) = _solve_pair(monkeypatch, (0, 1), make)
    assert sa == "Optimal"
    assert stats(mb)["classes"] == 2 and stats(mb)["classed_rows"] == 20 and stats(ma)["classed_rows"] == 0
    want = 10.0 * (-math.sqrt(2.0) / 2.0)             # both rows active: r = z - 1/4, r^2 = 1 - z: r = 1/2, z = 3/4, x = y = -r / sqrt(2)
    for model in (ma, mb):
        obj = model.getobjval()
        assert abs(obj - want) <= max(1e-6, 1e-6 * max(abs(obj), abs(want))), (obj, want)


def test_docs_model_in_a_thousand_blocks_takes_the_same_forty_iterations(monkeypatch):
    def make():
        M = T.docs_model(1000, ktn.KatanaSolver(log_level=0, iter_cap=40))
        st = M.solve()
        return M.internal_model, st
    (ma, sa), (mb, sb) = _solve_pair(monkeypatch, (0, -1), make)
    assert stats(mb)["classes"] == 2 and stats(mb)["classed_rows"] == 2000 and stats(ma)["classed_rows"] == 0
    assert ma.numcuts() > 2000


# ---- h. supporting-hyperplane cuts: the sweep before the root search is classed -------------------------------------------
def test_supporting_hyperplane_first_round_is_the_same_with_a_classed_sweep(monkeypatch):
    nrows, nlog = 10000, 1000
    n, d, lv, uv, lb, ub = T.cone_family(nrows, nlog)
    x0 = np.zeros(n)
    x0[2:3 * nrows:3] = 4.0
    x0[0:3 * nrows:3] = 0.5
    x0[1:3 * nrows:3] = 0.5
    x0[3 * nrows:] = 4.0
    out = []
    for s in (0, -1):
        monkeypatch.setenv("KTN_TAPE_CLASSED", str(s))
        m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, cut_algo="supporting_hyperplane"))
        m.loadproblem(n, len(lb), lv, uv, lb, ub, "Min", d)
        m.set_interior_point(x0)
        m.optimize_begin()
        M0 = m.lp_num_rows()
        m.ecp_step()
        out.append((m, m.getsolution()[:n], m.lp_rows_from(M0), m.last_sweep_slots(), m.last_sweep_lambdas()))
    (ma, xa, ra, sa, la), (mb, xb, rb, sb, lb_) = out
    assert stats(ma)["classed_rows"] == 0
    assert stats(mb) == dict(classes=2, classed_rows=nrows + nlog, interp_rows=0, class_max_nodes=int(np.max(np.diff(d.tape_ptr))))
    assert_bits(xa, xb, "first LP point")
    assert np.array_equal(sa, sb) and len(sa) > 0
    assert_bits(la, lb_, "lambdas")
    assert np.any(la < 1.0)
    for name, a, b in zip(("rowptr", "col", "val", "lo", "hi"), ra, rb):
        assert_bits(a, b, ("first-round cuts " + name))
