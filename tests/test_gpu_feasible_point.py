"""GPU tier: ktn_get_feasible_point (csrc/feas.hpp, feas.hip) against tests/feas_ref.py, which
tests/test_feas_ref.py pins on the CPU: every search kernel against mpmath for every lane-group width, the reduction at its sizes,
the state rules, the found codes and refused paths, and the two-sided bracket LB <= f* <= f(x_feas) end to end.

In the kernel tests x* is handed in through ktn_sep_precompute (the development switch KTN_FEAS_XSTAR_PRECOMPUTE, read when the
handle is made), the way tests/test_gpu_esh_quad_rows.py hands its point to the sweep; everywhere else x* is the solve's own."""
import ctypes as C_
import math

import numpy as np
import pytest
from mpmath import mp, mpf

import esh_quad_cases as EC
import feas_cases as FC
import feas_ref as FR
import katana_jl_amd as ktn
import kkt_cases
from helpers import hip_model_from_kat
from kat_util import load_family_ext, load_kats

pytestmark = pytest.mark.gpu
L = ktn._lib
INF = math.inf


def handed(monkeypatch, C, G=0, **kw):
    """a handle on the case with x_in = C.xi and x* = C.xs handed in: (model, FeasiblePoint, lambda_i by row)"""
    monkeypatch.setenv("KTN_FEAS_XSTAR_PRECOMPUTE", "1")
    if G:
        monkeypatch.setenv("KTN_FEAS_GROUP", str(G))
    else:
        monkeypatch.delenv("KTN_FEAS_GROUP", raising=False)
    m = ktn.NonlinearModel(ktn.KatanaSolver(**dict(dict(log_level=0, f_tol=FC.F_TOL), **kw)))
    m.loadproblem(*C.p)
    m.set_interior_point(C.xi)
    m.lp_solve()
    sep = ktn.KatanaHipSeparator(m)
    sep.initialize()
    xs = np.zeros(m.num_var)
    xs[:len(C.xs)] = C.xs
    sep.precompute(xs)
    return m, m.feasible_point(), m.feasible_row_lambdas()


def check_rows(C, lams, what):
    """every taking-part row: phi_i(lambda_i) <= E_i in mpmath, and >= -tau - E_i for the rows meant to converge"""
    with mp.workprec(FR.PREC):
        for i in C.part:
            lam = float(lams[i])
            assert 0.0 <= lam <= 1.0, what + (i, lam)
            f, e = FR.phi_exact(C.d, i, C.xi, C.xs, C.sig[i], C.bnd[i], lam)
            assert f <= e, what + (i, lam, float(f), float(e))
            if i in C.onepass:
                assert lam == 1.0, what + (i, lam)
            else:
                assert lam < 1.0, what + (i, lam)
                if i not in C.loose:
                    assert f >= -FC.TAU - e, what + (i, lam, float(f), float(e))
    for i in range(C.d.num_constr):
        if C.sig[i] == 0:
            assert lams[i] == 1.0, what + (i,)


def check_point(C, m, fp, lams, what):
    """the point: lambda* and the blocking row from lambda_i, x_feas the clamped formula at the returned lambda, f(x_feas) against
    mpmath, the linear violation against numpy"""
    print("%r: found %d lambda* %.17g blocking %d unconverged %d back-offs %d margin %.3e" % (what, fp.found, fp.lam, fp.blocking_row,
                                                                                            fp.unconverged, fp.backoffs, fp.nl_margin))
    assert fp.found == 1 and 0 <= fp.backoffs <= 8, what
    assert fp.nl_margin <= 0.0, what
    lam, row = FR.reduce_lambdas(lams, C.sig)
    if fp.backoffs == 0:
        assert fp.lam == lam, what + (fp.lam, lam)
    else:
        assert fp.lam < lam, what
    assert fp.blocking_row == row, what + (fp.blocking_row, row)
    want = FR.x_feas(C.xi, C.xs, fp.lam, C.p.l_var, C.p.u_var)
    assert fp.x.tobytes() == want.tobytes(), what + (np.flatnonzero(fp.x != want)[:5],)
    f, ef = FR.objective_exact(C.d, fp.x)
    with mp.workprec(FR.PREC):
        assert abs(mpf(fp.objval) - f) <= ef, what + (fp.objval, float(f), float(ef))
    lin = FR.linear_violation(C.d, C.p.l_constr, C.p.u_constr, fp.x)
    assert abs(fp.lin_viol - lin) <= 1e-12 * abs(lin), what + (fp.lin_viol, lin)


# ---- 1. the search kernels against mpmath -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sep_cases():
    return {G: FC.classify(FC.sep_case(G)) for G in FC.GROUPS}


@pytest.mark.parametrize("G", FC.GROUPS)
def test_separable_rows_against_mpmath(monkeypatch, sep_cases, G):
    C = sep_cases[G]
    m, fp, lams = handed(monkeypatch, C, G)
    assert m.stat("feas_group") == G
    check_rows(C, lams, ("sep", G))
    check_point(C, m, fp, lams, ("sep", G))
    (inf_row,) = C.loose
    assert 0.0 < lams[inf_row] < 1.0 and math.isfinite(lams[inf_row])            # phi(1) = +inf: bisection first, a finite lambda
    assert fp.unconverged <= 1 and fp.lin_viol > 0.4                              # (only the domain-edge row may run out of passes)
    assert fp.blocking_row in C.search


@pytest.fixture(scope="module")
def long_case():
    return FC.classify(FC.long_case())


def test_long_row_against_mpmath(monkeypatch, long_case):
    C = long_case
    m, fp, lams = handed(monkeypatch, C)
    assert m.stat("sep_long_rows") >= 1
    check_rows(C, lams, ("long",))
    check_point(C, m, fp, lams, ("long",))
    assert fp.blocking_row == 0 and fp.unconverged == 0


@pytest.fixture(scope="module")
def tape_cases():
    return {k: FC.classify(FC.tape_case(k)) for k in (1, 65)}


@pytest.mark.parametrize("nrows", (1, 65))
def test_tape_rows_against_mpmath(monkeypatch, tape_cases, nrows):
    C = tape_cases[nrows]
    m, fp, lams = handed(monkeypatch, C)
    check_rows(C, lams, ("tape", nrows))
    check_point(C, m, fp, lams, ("tape", nrows))
    assert fp.unconverged == 0 and fp.blocking_row in C.search


@pytest.fixture(scope="module")
def quad_cases():
    return FC.classify(FC.quad_case())


@pytest.mark.parametrize("G", FC.GROUPS)
def test_quad_rows_against_mpmath(monkeypatch, quad_cases, G):
    C = quad_cases
    m, fp, lams = handed(monkeypatch, C, G)
    assert m.stat("feas_quad_group") == G
    check_rows(C, lams, ("quad", G))
    check_point(C, m, fp, lams, ("quad", G))
    assert fp.unconverged == 0 and sorted(C.search) == [0, 1, 2] and C.onepass == [3]
    assert m.stat("feas_passes") == len(C.part)                                   # closed form: one evaluation per row


def test_quad_rows_that_take_the_search_on_their_coefficients(monkeypatch):
    I = FC.classify(FC.quad_fallback_case("indefinite"))
    m, fp, lams = handed(monkeypatch, I)
    check_rows(I, lams, ("indefinite",))
    check_point(I, m, fp, lams, ("indefinite",))
    assert m.stat("feas_passes") > 1 and fp.unconverged == 0                      # not the closed form, and it converged
    assert abs(fp.lam - (1.8 - math.sqrt(0.44)) / 2) < 1e-6
    E = FC.classify(FC.quad_fallback_case("edge"))
    m, fp, lams = handed(monkeypatch, E)
    # the discriminant is negative and only lambda = 0 is feasible: never a silent lambda -- the row is counted, the point is x_in
    assert fp.found == 1 and fp.lam == 0.0 and fp.unconverged == 1 and fp.blocking_row == 0
    assert fp.x.tobytes() == E.xi.tobytes() and fp.nl_margin <= 0.0


# ---- 2. the reduction ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m_nl", FC.REDUCE_SIZES)
def test_min_and_argmin_at_the_block_sizes(monkeypatch, m_nl):
    got = {}
    for where in ("first", "middle", "last"):
        for tie in (False, True):
            C = FC.reduce_case(m_nl, where, tie)
            m, fp, lams = handed(monkeypatch, C)
            what = (m_nl, where, tie)
            assert fp.found == 1 and fp.backoffs <= 8 and fp.unconverged == 0, what
            assert fp.blocking_row == C.blocking, what + (fp.blocking_row,)
            assert fp.lam == lams.min() == lams[C.blocking] and 0.49 < fp.lam < 0.5, what
            assert np.count_nonzero(lams < 1.0) == np.count_nonzero(C.b == 0.25), what
            got[what] = fp.lam
    assert len(set(got.values())) == 1                                            # the same row arithmetic wherever the row sits


# ---- 3. state ------------------------------------------------------------------------------------------------------------------------
def _state(m, sep):
    g, jac = np.zeros(sep.num_constr), np.zeros(sep.nnz)
    L.check(m._h, m._lib.ktn_sep_get_g(m._h, g.ctypes.data_as(L.P(L.c_f64)), len(g)))
    L.check(m._h, m._lib.ktn_sep_get_jac(m._h, jac.ctypes.data_as(L.P(L.c_f64)), len(jac)))
    return [g, jac, m.last_sweep_lambdas(), m.getconstrduals(), m.getreducedcosts(), np.asarray([m.getobjbound(), m.getobjgap()])]


@pytest.fixture(scope="module")
def state_instance():
    """a planted instance and an interior point of it (the engine's own, found once by a supporting-hyperplane handle)"""
    inst = ktn.instances.make_instance(n=40, m_nl=6, k=4, m_lin=12, family="explog", seed=3)
    m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, cut_algo="supporting_hyperplane"))
    m.loadproblem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr, inst.u_constr, inst.sense, ktn.SeparableNLP(inst))
    xin = m.interior_point()
    assert xin is not None
    print("interior point: outside [l, u] by %.3e" % max(np.max(inst.l_var - xin), np.max(xin - inst.u_var), 0.0))
    return inst, np.clip(xin, inst.l_var, inst.u_var)      # (the auxiliary LP's point meets the bounds to its tolerance only)


@pytest.mark.parametrize("algo", ("kelley", "supporting_hyperplane"))
def test_the_getter_leaves_the_state_bit_for_bit(state_instance, algo):
    """a twin handle that never asks: ktn_sep_get_g / _get_jac, last_sweep_lambdas, the KKT getters and a following ecp_step agree
    with it to the bit; feas_evals is 0 after the solve steps and 1 after two calls; an LP solve and a new interior point drop the
    cache"""
    inst, xin = state_instance
    flat = lambda fp: np.concatenate([fp.x, np.asarray([float(v) for v in fp[:1] + fp[2:]])]).tobytes()
    runs = []
    for ask in (False, True):
        m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, cut_algo=algo))
        m.loadproblem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr, inst.u_constr, inst.sense, ktn.SeparableNLP(inst))
        m.set_interior_point(xin)
        m.optimize_begin()
        for _ in range(4):
            m.ecp_step()
        sep = ktn.KatanaHipSeparator(m)
        sep.initialize()
        sep.precompute(m.getsolution())
        assert m.stat("feas_evals") == 0                                          # a solve launches nothing for the getter
        if ask:
            a, b = m.feasible_point(), m.feasible_point()
            assert m.stat("feas_evals") == 1                                      # computed once, served from the cache
            assert a.found == 1 and flat(a) == flat(b)
            print("state twin %s: lambda* %.12g blocking %d back-offs %d" % (algo, a.lam, a.blocking_row, a.backoffs))
        s0 = _state(m, sep)
        done = m.ecp_step()
        runs.append(s0 + [m.getsolution(), np.asarray([float(done), m.lp_num_rows(), m.numcuts()])])
        if ask:
            assert m.stat("feas_evals") == 1
            c = m.feasible_point()                                                # an LP solve dropped the cache
            assert m.stat("feas_evals") == 2
            m.set_interior_point(xin)
            d = m.feasible_point()                                                # ... and so does a new interior point
            assert m.stat("feas_evals") == 3 and flat(d) == flat(c)
    for k, (u, v) in enumerate(zip(*runs)):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes(), (algo, k)


# ---- 4. found codes and refused paths ----------------------------------------------------------------------------------------------
def refused(call, code):
    with pytest.raises(L.KatanaHipError) as e:
        call()
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def _ball_model(C, xin=None, **kw):
    m = ktn.NonlinearModel(ktn.KatanaSolver(**dict(dict(log_level=0), **kw)))
    m.loadproblem(*C.p)
    if xin is not None:
        m.set_interior_point(xin)
    return m


def test_found_codes():
    B = FC.ball()
    m = _ball_model(B)                                                            # Kelley without a caller's point: no reference point
    assert m.optimize() == "Optimal"
    fp = m.feasible_point()
    assert fp.found == 0 and np.isnan(fp.x).all() and m.getfeasiblesolution() is None and math.isnan(m.getprimalbound())
    assert m.stat("feas_evals") == 0
    m.set_interior_point(np.zeros(2))                                             # ... with one: found
    fp = m.feasible_point()
    assert fp.found == 1 and fp.nl_margin <= 0.0 and fp.blocking_row == 0 and np.array_equal(m.getfeasiblesolution(), fp.x)
    assert m.getprimalbound() == fp.objval and m.getcertifiedgap() == abs(fp.objval - m.getobjbound())
    m.set_interior_point([0.9, 0.9])                                              # a point that violates the row
    fp = m.feasible_point()
    assert fp.found == -1 and np.isnan(fp.x).all() and fp.blocking_row == 0 and fp.nl_margin > 0.0, fp
    m = _ball_model(FC.ball(u=0.5), [0.0, 0.7])                                   # a point outside a bound that satisfies the row
    m.lp_solve()
    fp = m.feasible_point()
    assert fp.found == -1 and np.isnan(fp.x).all() and fp.blocking_row == -1 and fp.nl_margin <= 0.0, fp
    N = FC.ball(kind=FC.NEGLOG, p1=0.0, ub=5.0)                                   # -log(x_0) - log(x_1) <= 5: not finite at x_in = 0
    m = _ball_model(N, np.zeros(2))
    m.lp_solve()
    fp = m.feasible_point()
    assert fp.found == -1 and fp.blocking_row == 0 and np.isnan(fp.x).all()


def test_refused_paths():
    B = FC.ball()
    m = _ball_model(B, np.zeros(2))
    assert "no LP solve" in refused(m.feasible_point, L.E_INVALID)                # no solve yet
    assert m.optimize() == "Optimal"
    buf, info = np.zeros(2), np.zeros(8)
    p = lambda a: a.ctypes.data_as(C_.POINTER(C_.c_double))
    assert m._lib.ktn_get_feasible_point(m._h, p(buf), 1, p(info), 8) == L.E_INVALID
    assert m._lib.ktn_get_feasible_point(m._h, p(buf), 2, p(info), 7) == L.E_INVALID
    assert m.stat("feas_evals") == 0
    assert m.feasible_point().found == 1
    m.reset()
    refused(m.feasible_point, L.E_INVALID)                                        # ktn_reset drops the answer
    R = FC.ball(lb=0.1)                                                           # a ranged nonlinear row
    m = _ball_model(R, np.full(2, 0.5))
    m.lp_solve()
    assert "two finite sides" in refused(m.feasible_point, L.E_UNSUPPORTED)
    inst = kkt_cases.build("a", 4).inst                                           # KTN_ROW_HOST rows
    m = kkt_cases.load(ktn, inst, "host")
    m.set_interior_point(np.zeros(4))
    m.lp_solve()
    assert "KTN_ROW_HOST" in refused(m.feasible_point, L.E_UNSUPPORTED)
    ms = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))                        # a row-sharded handle
    ar = L.ALLREDUCE_CB(lambda *a: 0)
    L.check(ms._h, ms._lib.ktn_dist_init_callback(ms._h, 0, 1, C_.cast(ar, C_.c_void_p), None))
    ms.loadproblem(*B.p)
    ms.set_interior_point(np.zeros(2))
    ms.lp_solve()
    refused(ms.feasible_point, L.E_UNSUPPORTED)


# ---- 5. end to end: LB <= f* <= f(x_feas) ----------------------------------------------------------------------------------------------
EXT = {m["id"]: m for m in load_family_ext()}


def bracket(m, fstar, what, sense="Min"):
    fp, lb = m.feasible_point(), m.getobjbound()
    s = -1.0 if sense == "Max" else 1.0
    tol = 1e-9 * (1.0 + abs(fstar))
    print("%r: LB %.12g  f* %.12g  f(x_feas) %.12g  certified gap %.3e  getobjgap %.3e  1 - lambda* %.3e  unconverged %d back-offs %d"
          % (what, lb, fstar, fp.objval, m.getcertifiedgap(), m.getobjgap(), 1.0 - fp.lam, fp.unconverged, fp.backoffs))
    assert fp.found == 1 and fp.backoffs <= 8 and fp.nl_margin <= 0.0, what
    assert s * lb - tol <= s * fstar <= s * fp.objval + tol, what + (lb, fstar, fp.objval)
    return fp


@pytest.mark.parametrize("algo", ("kelley", "supporting_hyperplane"))
@pytest.mark.parametrize("n", (33, 64))
def test_ball_family_bracket(n, algo):
    """f* = -sqrt(n).  f(x_feas) - f* <= |f*| (f_tol + tau) / 2 + 1e-6 (1 + |f*|):  |x*|^2 <= 1 + f_tol, phi' ~ 2 at the boundary, so
    1 - lambda* <= (f_tol + tau) / 2 to first order, the objective is linear along the segment from x_in = 0, and the stop rule's own
    objective tolerance"""
    M = hip_model_from_kat(ktn, EXT["501_01_n%d" % n], cut_algo=algo)
    m = ktn.NonlinearModel(M.solver)
    m.loadproblem(*M.problem())
    m.set_interior_point(np.zeros(n))
    assert m.optimize() == "Optimal"
    fstar = -math.sqrt(n)
    fp = bracket(m, fstar, ("ball", n, algo))
    assert fp.objval - fstar <= abs(fstar) * (1e-6 + 1e-7) / 2 + 1e-6 * (1.0 + abs(fstar)), (fp.objval, fstar)


def test_ellipsoid_and_expression_model_bracket():
    C = EC.ellipsoid_rho(8)
    m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, cut_algo="supporting_hyperplane_quad"))
    m.loadproblem(*EC.ellipsoid_rho_problem(C))
    m.set_interior_point(C.x0)
    assert m.optimize() == "Optimal"
    bracket(m, C.fstar, ("ellipsoid", 8))
    # an expression-built model of the reference's suite (tape rows), the reference point the engine's own
    kat = {k["id"]: k for k in load_kats()}["101_01"]
    M = hip_model_from_kat(ktn, kat, cut_algo="supporting_hyperplane")
    assert M.solve() == kat["expect"]["status"]
    m = M.internal_model
    assert m.interior_point() is not None
    bracket(m, kat["expect"]["obj"], ("101_01",), M.sense)
