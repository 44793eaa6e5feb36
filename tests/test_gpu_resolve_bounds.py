"""GPU tier: ktn_set_var_bounds and the re-solve from the kept cut pool (csrc/rebound.hip).  A solved handle
gets new variable bounds in place; the warm solve is compared with a cold solve on a fresh handle loaded with those bounds and with
the CPU oracle, on reference models with tape rows, a nonlinear objective and an LP through LinearQuadraticModel, on a separable
instance, and under supporting-hyperplane cuts.  Changes, from the solved x* with j the variable furthest from both of its bounds
(an infinite bound counts as one unit away from x*_j): u_j <- x*_j - (x*_j - l_j) / 4, the mirrored change of l_j, l_j = u_j =
midpoint, the original bounds again."""
import copy
import math
import os

import numpy as np
import pytest

import katana_jl_amd as ktn
import kat_util
from helpers import hip_load_instance, hip_model_from_kat, max_nl_violation, oracle_solve_instance, oracle_solve_kat, pool_bits
from oracle.evaluators import SexprNLPEvaluator
from test_gpu_quad_rows import lpqp_parts

pytestmark = pytest.mark.gpu
L = ktn._lib
INF = math.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class KatCase:
    """a reference model of tests/golden/kat_models.json through the expression front end"""
    def __init__(self, kid, **solver_kw):
        self.name, self.kw = kid, solver_kw
        self.model = next(m for m in kat_util.load_kats() if m["id"] == kid)
        self.P = hip_model_from_kat(ktn, self.model).problem()
        self.n = self.P.num_var
        self.l0, self.u0 = np.array(self.P.l_var), np.array(self.P.u_var)
        e = self.model["expect"]
        self.atol, self.rtol, self.const = e["obj_atol"], e["obj_rtol"], 0.0

    def fresh(self, l, u):
        m = ktn.NonlinearModel(ktn.KatanaSolver(**dict(dict(log_level=0), **self.kw)))
        m.loadproblem(*self.P._replace(l_var=np.array(l), u_var=np.array(u)))
        return m

    def oracle(self, l, u):
        mm = copy.deepcopy(self.model)
        for v, a, b in zip(mm["vars"], l, u):
            v["lb"], v["ub"] = float(a), float(b)
        om = oracle_solve_kat(mm)
        return om.status, om.getobjval()

    def violation(self, x):
        """the largest violation of a nonlinear row at x under the oracle's evaluator (0 for a model without one)"""
        cons = self.model["constraints"]
        d = SexprNLPEvaluator(self.n, self.model["objective"], [c["expr"] for c in cons], [c["linear"] for c in cons],
                              self.model["objective_linear"])
        g = np.zeros(len(cons))
        d.eval_g(g, np.asarray(x, dtype=np.float64)[:self.n])
        return max([max(g[i] - c["ub"], c["lb"] - g[i]) for i, c in enumerate(cons) if not c["linear"]] + [0.0])


class LqCase(KatCase):
    """an LP of test/lpqp.jl through LinearQuadraticModel (KTN_ROW_QUAD rows without Q)"""
    def __init__(self, kid):
        KatCase.__init__(self, kid)
        self.parts = lpqp_parts(self.model)
        self.const = self.parts[5]

    def fresh(self, l, u):
        A, lo, hi, obj, diag, const = self.parts
        m = ktn.LinearQuadraticModel(ktn.KatanaSolver(log_level=0))
        m.loadproblem(A, np.array(l), np.array(u), obj, lo, hi, self.model["sense"])
        return m


class InstCase:
    """instances.make_instance at n = 40: separable rows"""
    def __init__(self, name="inst40", **solver_kw):
        self.name, self.kw = name, solver_kw
        self.inst = ktn.instances.make_instance(n=40, m_nl=6, k=8, family="explog", seed=11)
        self.n, self.l0, self.u0 = self.inst.n, np.array(self.inst.l_var), np.array(self.inst.u_var)
        self.atol, self.rtol, self.const = 1e-6, 1e-6, 0.0

    def with_bounds(self, l, u):
        inst = copy.copy(self.inst)
        inst.l_var, inst.u_var = np.array(l), np.array(u)
        return inst

    def fresh(self, l, u):
        return hip_load_instance(ktn, self.with_bounds(l, u), **self.kw)

    def oracle(self, l, u):
        om = oracle_solve_instance(self.with_bounds(l, u))
        return om.status, om.getobjval()

    def violation(self, x):
        return max_nl_violation(self.inst, x)


CASES = {"101_01": lambda: KatCase("101_01"), "102_04": lambda: KatCase("102_04"), "lq_001_01": lambda: LqCase("001_01"),
         "inst40": lambda: InstCase(), "inst40_esh": lambda: InstCase("inst40_esh", cut_algo="supporting_hyperplane")}


def changes(x, l0, u0):
    """[(name, l, u)] of the four changes"""
    le = np.where(np.isfinite(l0), l0, x - 1.0)
    ue = np.where(np.isfinite(u0), u0, x + 1.0)
    j = int(np.argmax(np.minimum(x - le, ue - x)))
    out = []
    l, u = l0.copy(), u0.copy()
    u[j] = x[j] - 0.25 * (x[j] - le[j])
    out.append(("upper", l, u))
    l, u = l0.copy(), u0.copy()
    l[j] = x[j] + 0.25 * (ue[j] - x[j])
    out.append(("lower", l, u))
    l, u = l0.copy(), u0.copy()
    l[j] = u[j] = 0.5 * (le[j] + ue[j])
    out.append(("fixed", l, u))
    out.append(("original", l0.copy(), u0.copy()))
    return out


def run_case(name):
    """one case through the unchanged re-solve and the four changes, every check of the file's docstring asserted; returns its rows
    of the table (case, change, cold rounds, warm rounds)"""
    TABLE = []
    C = CASES[name]()
    C.name = name
    m = C.fresh(C.l0, C.u0)
    assert m.optimize() == "Optimal"
    cold0, obj0 = m.numiters(), m.getobjval()
    x = m.getsolution()[:C.n].copy()
    # unchanged bounds: one round is expected, never more than the cold count, the same objective
    m.setvarbounds(C.l0, C.u0)
    assert m.optimize() == "Optimal" and m.numiters() <= cold0
    assert kat_util.isapprox(m.getobjval(), obj0, C.atol, C.rtol)
    print("%s: cold %d rounds, re-solve with unchanged bounds %d round(s)" % (C.name, cold0, m.numiters()))
    TABLE.append((C.name, "unchanged", cold0, m.numiters()))
    for what, l, u in changes(x, C.l0, C.u0):
        before = pool_bits(m)
        m.setvarbounds(l, u)
        assert pool_bits(m) == before, (C.name, what)                        # rows, duals, row count and cut count: bit for bit
        assert m.status() == "None" and m.numiters() == 0
        for getter in (m.getconstrduals, m.getobjbound, m.feasible_point):   # dropped with the solve they described
            with pytest.raises(L.KatanaHipError) as e:
                getter()
            assert e.value.code == L.E_INVALID, (C.name, what, getter)
        st = m.optimize()
        cold = C.fresh(l, u)
        st_cold = cold.optimize()
        ost, oobj = C.oracle(l, u)
        print("%s %s: warm %s %.9f in %d rounds | cold %s %.9f in %d rounds | oracle %s %.9f | clamped %d, warm_solves %d" % (
            C.name, what, st, m.getobjval(), m.numiters(), st_cold, cold.getobjval(), cold.numiters(), ost, oobj,
            m.stat("warm_clamped_cols"), m.stat("warm_solves")))
        assert st == st_cold == ost, (C.name, what, st, st_cold, ost)
        TABLE.append((C.name, what, cold.numiters(), m.numiters()))
        if st != "Optimal":                                                   # (the change emptied the feasible set: the statuses agree, nothing else to compare)
            continue
        assert kat_util.isapprox(m.getobjval(), cold.getobjval(), C.atol, C.rtol), (C.name, what, m.getobjval(), cold.getobjval())
        assert kat_util.isapprox(m.getobjval() + C.const, oobj, C.atol, C.rtol), (C.name, what, m.getobjval() + C.const, oobj)
        xs = m.getsolution()[:C.n]
        assert np.all(xs >= l - 1e-9) and np.all(xs <= u + 1e-9)
        v = C.violation(xs)
        assert v <= 1e-6, (C.name, what, v)                                   # f_tol
        # the getters answer again, and the dual bound lies below the objective
        m.getconstrduals()
        sgn = -1.0 if getattr(C, "model", {}).get("sense") == "Max" else 1.0
        assert sgn * m.getobjbound() <= sgn * m.getobjval() + max(C.atol, C.rtol * abs(m.getobjval())), (C.name, what, m.getobjbound(), m.getobjval())
        m.feasible_point()
    return TABLE


@pytest.fixture(scope="module")
def table():
    """rows of a case, computed once per module"""
    cache = {}

    def rows(name):
        if name not in cache:
            cache[name] = run_case(name)
        return cache[name]
    return rows


@pytest.mark.parametrize("name", list(CASES))
def test_warm_resolve_against_cold_and_oracle(name, table):
    assert len(table(name)) == 5


def test_infeasible_by_a_linear_row_then_restored():
    C = InstCase()
    m = C.fresh(C.l0, C.u0)
    assert m.optimize() == "Optimal"
    obj0, lp0 = m.getobjval(), m.stat("lp_solves")
    rp, col, val, lo, hi = m.lp_rows()
    k = next(k for k in range(len(lo)) if math.isfinite(hi[k]) and rp[k + 1] > rp[k])      # a linear row with an upper side
    c, v = col[rp[k]:rp[k + 1]], val[rp[k]:rp[k + 1]]
    # a box on which that row's smallest value lies above its bound: every column of the row pinned at the end that raises it
    l, u = C.l0.copy(), C.u0.copy()
    for j, a in zip(c, v):
        if a > 0:
            l[j] = u[j]
        elif a < 0:
            u[j] = l[j]
    amin = float(np.sum(np.where(v > 0, v * l[c], v * u[c])))
    assert amin > hi[k] + 1e-3, (amin, hi[k])
    m.setvarbounds(l, u)
    assert m.optimize() == "Infeasible"
    assert m.stat("screen_infeasible_rows") >= 1 and m.stat("lp_solves") == lp0 and m.stat("screen_first_row") <= k
    cold = C.fresh(l, u)
    assert cold.optimize() == "Infeasible"
    m.setvarbounds(C.l0, C.u0)
    assert m.optimize() == "Optimal" and kat_util.isapprox(m.getobjval(), obj0, 1e-6, 1e-6)


def test_infeasible_only_through_a_nonlinear_row():
    # the unit disc of 101_01 with the box moved outside it: the warm solve's status is the cold solve's
    C = KatCase("101_01")
    m = C.fresh(C.l0, C.u0)
    assert m.optimize() == "Optimal"
    l, u = np.array([1.5, 1.5]), np.array([2.0, 2.0])
    m.setvarbounds(l, u)
    st = m.optimize()
    cold = C.fresh(l, u)
    assert st == cold.optimize(), (st, cold.status())
    assert m.stat("screen_infeasible_rows") == 0 or st == "Infeasible"


def test_setter_before_the_first_solve_equals_loading_with_those_bounds():
    C = InstCase()                                                            # linear objective, finite bounds
    x = np.array(C.inst.x_opt if hasattr(C.inst, "x_opt") else 0.5 * (C.l0 + C.u0))[:C.n]
    what, l, u = changes(x, C.l0, C.u0)[0]
    a = C.fresh(C.l0, C.u0)
    a.setvarbounds(l, u)
    sa = a.optimize()
    b = C.fresh(l, u)
    sb = b.optimize()
    assert sa == sb and a.numiters() == b.numiters() and a.numcuts() == b.numcuts()
    assert a.getsolution().tobytes() == b.getsolution().tobytes() and a.getobjval() == b.getobjval()


def test_refusals_and_the_callers_interior_point():
    C = InstCase()
    m = C.fresh(C.l0, C.u0)
    bad = C.l0.copy()
    bad[2] = np.nan
    with pytest.raises(L.KatanaHipError) as e:
        m.setvarbounds(bad, None)
    assert e.value.code == L.E_INVALID
    # a caller's interior point is kept as given: outside the new box it is reported, not replaced.  The point is one the engine
    # found itself on a second handle (so it satisfies the rows: found = 1 under the loaded box); the new box cuts it off in one
    # coordinate and still holds x*, so the problem stays feasible
    e2 = InstCase("inst40_esh", cut_algo="supporting_hyperplane").fresh(C.l0, C.u0)
    assert e2.optimize() == "Optimal"
    xin = np.clip(e2.interior_point()[:C.n], C.l0, C.u0)
    assert m.optimize() == "Optimal"
    obj0, x = m.getobjval(), m.getsolution()[:C.n].copy()
    m.set_interior_point(xin)
    assert m.feasible_point().found == 1
    j = int(np.argmax(np.abs(x - xin)))
    assert abs(x[j] - xin[j]) > 1e-3
    l, u = C.l0.copy(), C.u0.copy()
    if x[j] > xin[j]:
        l[j] = 0.5 * (x[j] + xin[j])
    else:
        u[j] = 0.5 * (x[j] + xin[j])
    m.setvarbounds(l, u)
    assert m.optimize() == "Optimal" and kat_util.isapprox(m.getobjval(), obj0, 1e-6, 1e-6)
    assert m.feasible_point().found == -1
    # a handle with a cut exchange installed
    g = C.fresh(C.l0, C.u0)
    g.lp_enable_global_lists(C.inst.m_nl)
    keep = L.EXCHANGE_CB(lambda *a: 0)
    g.set_cut_exchange(keep, 0)
    for call in (lambda: g.setvarbounds(C.l0, C.u0), lambda: g.setobj(np.zeros(C.n))):
        with pytest.raises(L.KatanaHipError) as e:
            call()
        assert e.value.code == L.E_UNSUPPORTED


def test_warm_rounds_are_fewer_in_total_and_the_table_is_written(table):
    TABLE = [r for name in CASES for r in table(name)]
    rows = [r for r in TABLE if r[1] != "unchanged"]
    assert len(rows) == 4 * len(CASES)
    cold, warm = sum(r[2] for r in rows), sum(r[3] for r in rows)
    lines = ["%-12s %-10s %6s %6s" % ("case", "change", "cold", "warm")] + ["%-12s %-10s %6d %6d" % r for r in TABLE]
    lines.append("%-12s %-10s %6d %6d   (the four changes of every case; 'unchanged' rows left out)" % ("total", "", cold, warm))
    print("\n".join(lines))
    out = os.environ.get("KTN_RESOLVE_TABLE")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert warm < cold, (warm, cold)
