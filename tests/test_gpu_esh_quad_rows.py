"""GPU tier: supporting-hyperplane cuts of KTN_ROW_QUAD rows (cut_algo = KTN_CUT_SUPPORTING_QUAD; csrc/esh_quad.hpp): k_esh_quad and
the emission against mpmath (tests/esh_quad_ref.py) for every lane-group width, the rows that keep Kelley's cut and the SEP / TAPE
rows bit for bit against handles of the two other cut algorithms, ktn_sep_gencut, the auxiliary problem with a QUAD row, solves with
closed-form answers, the LinearQuadraticModel front end and the refused paths."""
import ctypes as C_
import math

import numpy as np
import pytest
from mpmath import mp, mpf

import esh_quad_cases as EC
import esh_quad_ref as ER
import katana_jl_amd as ktn
import kat_util
import quad_ref as Q

pytestmark = pytest.mark.gpu
L = ktn._lib
INF = math.inf
QUAD = dict(cut_algo="supporting_hyperplane_quad")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_bits(a, b, what):
    a, b = bits(np.asarray(a)), bits(np.asarray(b))
    assert a.shape == b.shape and np.array_equal(a, b), (what, np.flatnonzero(a != b)[:8] if a.shape == b.shape else (a.shape, b.shape))


def handle(monkeypatch, G, algo):
    C = EC.case()
    if G:
        monkeypatch.setenv("KTN_ESH_QUAD_GROUP", str(G))
    else:
        monkeypatch.delenv("KTN_ESH_QUAD_GROUP", raising=False)
    model = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, f_tol=C.f_tol, cut_algo=algo))
    model.loadproblem(C.n, C.m, np.full(C.n, -2.0), np.full(C.n, 2.0), C.lb, C.ub, "Min", C.d)
    if algo:
        model.set_interior_point(C.xi)
    sep = ktn.KatanaHipSeparator(model)
    sep.initialize()
    return model, sep


def get_g_jac(model, sep):
    lib, h = model._lib, model._h
    g, jac = np.zeros(sep.num_constr), np.zeros(sep.nnz)
    L.check(h, lib.ktn_sep_get_g(h, g.ctypes.data_as(L.P(L.c_f64)), len(g)))
    L.check(h, lib.ktn_sep_get_jac(h, jac.ctypes.data_as(L.P(L.c_f64)), len(jac)))
    return g, jac


def run(monkeypatch, G, algo):
    """one precompute and one sweep at the case's x*: everything read back"""
    C = EC.case()
    model, sep = handle(monkeypatch, G, algo)
    sep.precompute(C.xt)
    o = dict(model=model, sep=sep)
    o["g"], o["jac"] = get_g_jac(model, sep)
    m0 = model.lp_num_rows()
    o["nviol"], o["maxviol"] = sep.sweep(C.f_tol)
    o["rows"] = model.lp_rows_from(m0)
    o["slots"] = model.last_sweep_slots()
    o["lams"] = model.last_sweep_lambdas()
    o["g2"], o["jac2"] = get_g_jac(model, sep)
    o["cut_of"] = {C.nl[int(s)]: k for k, s in enumerate(o["slots"])}
    return o


def cut(o, i):
    k = o["cut_of"][i]
    rp, col, val, lo, hi = o["rows"]
    return col[rp[k]:rp[k + 1]], val[rp[k]:rp[k + 1]], lo[k], hi[k], float(o["lams"][k])


_OTHER = {}


def other(monkeypatch, algo):
    """the Kelley handle (0) and the KTN_CUT_SUPPORTING handle (1) at the same x*: independent of the lane-group width"""
    if algo not in _OTHER:
        _OTHER[algo] = run(monkeypatch, 0, algo)
    return _OTHER[algo]


def same_cut(a, b, what):
    assert np.array_equal(a[0], b[0]), what
    assert_bits(a[1], b[1], what)
    assert bits(np.float64(a[2])) == bits(np.float64(b[2])) and bits(np.float64(a[3])) == bits(np.float64(b[3])), what
    assert a[4] == b[4], what


@pytest.mark.parametrize("G", EC.GROUPS)
def test_kernel_against_mpmath_and_the_other_rows_bit_for_bit(monkeypatch, G):
    C = EC.case()
    o = run(monkeypatch, G, 2)
    model, sep = o["model"], o["sep"]
    rp = sep.rowptr
    want = [s for s, i in enumerate(C.nl) if i == C.m or C.violated[i]]
    assert o["nviol"] == len(want) and o["slots"].tolist() == want
    assert model.stat("esh_participating_rows") == sum(1 for i in range(C.m) if C.tags[i] in ("part", "shallow", "indefinite", "satisfied")
                                                       or (C.rows[i][0] in ("sep", "tape") and not C.d.row_linear[i]))
    # ---- the rows that take part: the cut at x_b against mpmath
    for i in C.part:
        cols, a, lo, hi, lam = cut(o, i)
        s, bnd = C.sides[i], EC.bound_of(C, i)
        what = (G, i, len(cols))
        assert 0.0 < lam < 1.0, what
        R = ER.cut_ref_mp(C.layouts[i], C.rows[i][6], C.xi, C.x, s, bnd, lam, EC.TAU)
        assert np.array_equal(cols, sep.col[rp[i]:rp[i + 1]]), what
        with mp.workprec(Q.PREC):
            assert 0 <= R.phi <= EC.TAU, what + (float(R.phi),)
            for e in range(R.k):
                assert abs(mpf(float(a[e])) - R.der[e]) <= R.e_der[e], what + (e, a[e], float(R.der[e]), float(R.e_der[e]))
            got, free = (hi, lo) if s > 0 else (lo, hi)
            assert free == (-INF if s > 0 else INF), what
            assert abs(mpf(float(got)) - (mpf(float(bnd)) - R.b)) <= R.bound_tol(bnd), what + (got, float(mpf(float(bnd)) - R.b))
            ax_star = sum((mpf(float(a[e])) * mpf(float(C.x[c])) for e, c in enumerate(cols)), mpf(0))
            ax_int = sum((mpf(float(a[e])) * mpf(float(C.xi[c])) for e, c in enumerate(cols)), mpf(0))
            assert s * (ax_star - mpf(float(got))) > 0 and s * (ax_int - mpf(float(got))) <= 0, what
    # ---- the fallback classes: Kelley's cut, bit for bit
    ok = other(monkeypatch, 0)
    assert np.array_equal(ok["slots"], o["slots"])
    for i in C.fallback:
        ck = cut(ok, i)
        same_cut(cut(o, i), ck, (G, i, "fallback"))
        assert ck[4] == 1.0
    # ---- SEP and TAPE rows: what KTN_CUT_SUPPORTING gives them
    o1 = other(monkeypatch, 1)
    moved1 = 0
    for i in range(C.m):
        if C.rows[i][0] == "quad" or i not in o["cut_of"]:
            continue
        same_cut(cut(o, i), cut(o1, i), (G, i, C.tags[i]))
        moved1 += cut(o1, i)[4] < 1.0
    assert moved1 > 0
    for i in C.part:
        assert cut(o1, i)[4] == 1.0                                                 # (KTN_CUT_SUPPORTING leaves QUAD rows alone)
    # ---- the whole sweep
    assert_bits(o["g2"], o["g"], "g after the sweep")
    assert_bits(o["jac2"], o["jac"], "Jacobian after the sweep")
    assert model.stat("esh_rows") + model.stat("esh_fallback_rows") == o["nviol"]
    assert model.stat("esh_quad_rows") == len(C.part)
    assert model.stat("esh_rows") == len(C.part) + moved1
    o2 = run(monkeypatch, G, 2)
    for key in ("g", "jac", "g2", "jac2", "lams", "slots"):
        assert_bits(o2[key], o[key], (key, "second handle"))
    for a, b in zip(o2["rows"], o["rows"]):
        assert_bits(a, b, "LP rows, second handle")


def test_gencut_gives_the_sweeps_cut_and_puts_the_row_back(monkeypatch):
    C = EC.case()
    o = run(monkeypatch, 0, 2)
    model, sep = handle(monkeypatch, 0, 2)
    sep.precompute(C.xt)
    g0, jac0 = get_g_jac(model, sep)
    rp = sep.rowptr
    for j, i in enumerate(C.part):
        cols, coefs, const = sep.gencut(C.xt, None, i)
        c_, a, lo, hi, lam = cut(o, i)
        assert np.array_equal(cols, c_), i
        assert_bits(coefs, a, ("gencut coefficients", i))
        bnd = EC.bound_of(C, i)
        assert bits(np.float64(bnd - const)) == bits(np.float64(hi if C.sides[i] > 0 else lo)), ("gencut constant", i)
        # the row's own state and a neighbour's, without another precompute
        nb = C.part[(j + 1) % len(C.part)]
        cols_n, coefs_n, _ = sep.gencut(C.xt, None, nb)
        assert_bits(coefs_n, cut(o, nb)[1], ("neighbour", i, nb))
        g1, jac1 = get_g_jac(model, sep)
        assert_bits(jac1, jac0, ("Jacobian after gencut", i))
        assert_bits(g1, g0, ("g after gencut", i))
    for i in C.fallback[:-1]:                                                       # Kelley's cut from gencut too
        cols, coefs, const = sep.gencut(C.xt, None, i)
        assert_bits(coefs, jac0[rp[i]:rp[i + 1]], ("fallback gencut", i))
    m0 = model.lp_num_rows()
    sep.sweep(C.f_tol)
    for a, b in zip(model.lp_rows_from(m0), o["rows"]):
        assert_bits(a, b, "the sweep after the gencuts")


def _solve(p, xint=None, **kw):
    m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, **kw))
    m.loadproblem(*p)
    if xint is not None:
        m.set_interior_point(xint)
    st = m.optimize()
    return st, m.getobjval(), m


@pytest.mark.parametrize("n", [2, 4])
def test_auxiliary_problem_carries_the_quad_row(n):
    """the CPU study on exact LP vertices found a point after 10 rounds (n = 2) and 34 rounds (n = 4)"""
    C = EC.ellipsoid_rho(n)
    m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, esh_interior_iters=200, **QUAD))
    m.loadproblem(*EC.ellipsoid_rho_problem(C))
    assert m.stat("esh_participating_rows") == 1
    xi = m.interior_point()
    print("auxiliary problem n=%d: found=%d rounds=%d s=%.6g" % (n, m.stat("esh_interior_found"), m.stat("esh_interior_rounds"),
                                                                  m.stat("esh_interior_s")))
    assert xi is not None
    assert EC.ellipsoid_value(C, xi) <= C.rho - 10 * 1e-6, EC.ellipsoid_value(C, xi)


@pytest.mark.parametrize("n", [4, 8])
def test_ellipsoid_solves_in_no_more_rounds_than_kelley(n):
    """the CPU study on exact LP vertices: 47 against 64 rounds (n = 4), 158 against 225 (n = 8).

    Under code 2 the engine hands every LP of at most 32 columns to the exact small-LP kernel (lp.hip): with the tolerance
    schedule's loosely solved LP points the same solves took 100 rounds against Kelley's 71 at n = 4 and 231 against 227 at n = 8,
    from vertices 49 and 162 ("Declared-quadratic rows").  Kelley runs with the default schedule here."""
    _rounds_check(n, {})


@pytest.mark.parametrize("n", [4, 8])
def test_ellipsoid_solves_in_fewer_rounds_than_kelley_on_exact_lp_vertices(n):
    """both methods with every LP handed to the exact small-LP kernel (lp_dense_after = -1), the setting of the CPU study: measured
    64 / 49 rounds (n = 4) and 240 / 162 (n = 8)"""
    _rounds_check(n, dict(lp_dense_after=-1))


def _rounds_check(n, opts):
    C = EC.ellipsoid_rho(n)
    p = EC.ellipsoid_rho_problem(C)
    rounds = {}
    for algo in ("kelley", "supporting_hyperplane_quad"):
        st, obj, m = _solve(p, xint=C.x0, cut_algo=algo, **opts)
        rounds[algo] = m.numiters()
        print("ellipsoid rho=4 n=%d %s: %s obj=%.12g f*=%.12g err=%.3g rounds=%d" % (n, algo, st, obj, C.fstar, abs(obj - C.fstar), m.numiters()))
        assert st == "Optimal", (algo, st)
        assert kat_util.isapprox(obj, C.fstar, 1e-6, 1e-6), (algo, obj, C.fstar)
        if algo != "kelley":
            assert m.stat("esh_quad_rows") > 0
    print("rounds n=%d: kelley %d, supporting hyperplanes %d" % (n, rounds["kelley"], rounds["supporting_hyperplane_quad"]))
    assert rounds["supporting_hyperplane_quad"] <= rounds["kelley"], rounds


def test_linear_quadratic_model_hands_the_point_over_after_its_lazy_load():
    import scipy.sparse as sp
    m = ktn.LinearQuadraticModel(ktn.KatanaSolver(log_level=0, **QUAD))
    m.loadproblem(sp.csr_matrix((0, 2)), [-2.0, -2.0], [2.0, 2.0], [1.0, 1.0], [], [], "Max")
    m.addquadconstr([], [], [0, 1], [0, 1], [1.0, 1.0], "<", 1.0)
    m.set_interior_point([0.0, 0.0])                                               # before optimize(): nothing is loaded yet
    st = m.optimize()
    assert st == "Optimal" and kat_util.isapprox(m.getobjval(), math.sqrt(2.0), 1e-6, 1e-6), (st, m.getobjval())
    assert m.stat("esh_quad_rows") > 0 and m.stat("esh_interior_rounds") == 0
    assert np.array_equal(m.interior_point(), [0.0, 0.0])


def test_unsupported_combinations_are_refused_as_under_supporting_hyperplanes():
    C = EC.ellipsoid_rho(4)
    p = EC.ellipsoid_rho_problem(C)
    m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, **QUAD))
    m.loadproblem(*p)
    m.set_blocks([0, C.n])
    with pytest.raises(L.KatanaHipError) as e:
        m.optimize_blocks()
    assert e.value.code == L.E_UNSUPPORTED
    m2 = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, **QUAD))
    m2.loadproblem(*p)
    m2.lp_enable_global_lists(1)
    cb = L.EXCHANGE_CB(lambda *a: 0)
    with pytest.raises(L.KatanaHipError) as e:
        m2.set_cut_exchange(cb, 0)
    assert e.value.code == L.E_UNSUPPORTED
    # a row-sharded handle: refused at loadproblem, before anything is exchanged
    m3 = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, **QUAD))
    ar = L.ALLREDUCE_CB(lambda *a: 1)                                              # (never called: the load is refused first)
    L.check(m3._h, m3._lib.ktn_dist_init_callback(m3._h, 0, 2, C_.cast(ar, C_.c_void_p), None))
    with pytest.raises(L.KatanaHipError) as e:
        m3.loadproblem(*p)
    assert e.value.code == L.E_UNSUPPORTED
    with pytest.raises(L.KatanaHipError) as e:
        ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, cut_algo=3))
    assert e.value.code == L.E_INVALID
