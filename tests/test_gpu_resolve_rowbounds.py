"""GPU tier: ktn_set_row_bounds and the re-solve from the kept, shifted cut pool (csrc/rebound.hip; DESIGN.md section 14 "Row
bounds").  A solved handle gets new constraint bounds in place; the warm solve is compared with a cold solve on a fresh handle
loaded with those bounds and with the CPU oracle, over the cases of tests/test_gpu_resolve_bounds.py.  Changes, with i the nonlinear
row (for the LP: the linear row) of largest multiplier and b its finite bound: b loosened by 0.25 max(1, |b|); b tightened by STEP;
the original bounds again.  STEP was chosen on the CPU with the oracle: for every row that can be picked in these cases (each
nonlinear row of 101_01, 102_04 and inst40, each row of the LP 001_01) the oracle still reports "Optimal" with that row tightened by
0.25 -- and each run asserts it again as a precondition."""
import copy
import math
import os

import numpy as np
import pytest

import katana_jl_amd as ktn
import kat_util
from helpers import hip_load_instance, max_nl_violation, oracle_evaluator, oracle_solve_instance, oracle_solve_kat
from oracle.evaluators import SexprNLPEvaluator
from test_gpu_resolve_bounds import CASES, InstCase, KatCase, LqCase

pytestmark = pytest.mark.gpu
L = ktn._lib
INF = math.inf
STEP = 0.25
F_TOL = 1e-6


def row_data(C):
    """(lb0, ub0, candidate rows) in the engine's row order: the nonlinear rows, for the LP every row"""
    if isinstance(C, InstCase):
        return np.array(C.inst.l_constr, dtype=np.float64), np.array(C.inst.u_constr, dtype=np.float64), list(range(C.inst.m_lin, C.inst.num_constr))
    if isinstance(C, LqCase):
        return np.array(C.parts[1], dtype=np.float64), np.array(C.parts[2], dtype=np.float64), list(range(len(C.parts[1])))
    cons = C.model["constraints"]
    return np.array(C.P.l_constr, dtype=np.float64), np.array(C.P.u_constr, dtype=np.float64), [i for i, c in enumerate(cons) if not c["linear"]]


def fresh(C, lb, ub):
    if isinstance(C, InstCase):
        inst = copy.copy(C.inst)
        inst.l_constr, inst.u_constr = np.array(lb), np.array(ub)
        return hip_load_instance(ktn, inst, **C.kw)
    if isinstance(C, LqCase):
        A, _, _, obj, _, _ = C.parts
        m = ktn.LinearQuadraticModel(ktn.KatanaSolver(log_level=0))
        m.loadproblem(A, C.l0, C.u0, obj, np.array(lb), np.array(ub), C.model["sense"])
        return m
    m = ktn.NonlinearModel(ktn.KatanaSolver(**dict(dict(log_level=0), **C.kw)))
    m.loadproblem(*C.P._replace(l_constr=np.array(lb), u_constr=np.array(ub)))
    return m


def oracle(C, lb, ub, lb0, ub0):
    if isinstance(C, InstCase):
        inst = copy.copy(C.inst)
        inst.l_constr, inst.u_constr = np.array(lb), np.array(ub)
        om = oracle_solve_instance(inst)
        return om.status, om.getobjval()
    mm = copy.deepcopy(C.model)                                                   # (the model's bounds carry the row's constant: move them by the same amount)
    for i, c in enumerate(mm["constraints"]):
        if lb[i] != lb0[i]:
            c["lb"] = float(c["lb"] + (lb[i] - lb0[i]))
        if ub[i] != ub0[i]:
            c["ub"] = float(c["ub"] + (ub[i] - ub0[i]))
    om = oracle_solve_kat(mm)
    return om.status, om.getobjval()


def violation(C, x, lb, ub):
    """the largest violation of a nonlinear row at x under the oracle's evaluator and the bounds given"""
    if isinstance(C, LqCase):
        return 0.0
    if isinstance(C, InstCase):
        d, mc, rows = oracle_evaluator(C.inst), C.inst.num_constr, range(C.inst.m_lin, C.inst.num_constr)
    else:
        cons = C.model["constraints"]
        d = SexprNLPEvaluator(C.n, C.model["objective"], [c["expr"] for c in cons], [c["linear"] for c in cons], C.model["objective_linear"])
        mc, rows = len(cons), [i for i, c in enumerate(cons) if not c["linear"]]
    g = np.zeros(mc)
    d.eval_g(g, np.asarray(x, dtype=np.float64)[:C.n])
    return max([max(g[i] - ub[i], lb[i] - g[i]) for i in rows] + [0.0])


def changes(i, lb0, ub0):
    upper = math.isfinite(ub0[i])
    b = ub0[i] if upper else lb0[i]
    out = []
    for name, delta in (("loosened", 0.25 * max(1.0, abs(b))), ("tightened", -STEP)):
        lb, ub = lb0.copy(), ub0.copy()
        if upper:
            ub[i] = b + delta
        else:
            lb[i] = b - delta
        out.append((name, lb, ub))
    out.append(("original", lb0.copy(), ub0.copy()))
    return out


def run_case(name):
    C = CASES[name]()
    C.name = name
    lb0, ub0, cand = row_data(C)
    m = fresh(C, lb0, ub0)
    assert m.optimize() == "Optimal"
    d = m.getconstrduals()
    i = cand[int(np.argmax(np.abs(d[cand])))]
    sgn = -1.0 if getattr(C, "model", {}).get("sense") == "Max" else 1.0
    table = []
    for what, lb, ub in changes(i, lb0, ub0):
        m.setconstrbounds(lb, ub)
        assert m.status() == "None" and m.numiters() == 0
        st = m.optimize()
        cold = fresh(C, lb, ub)
        st_cold = cold.optimize()
        ost, oobj = oracle(C, lb, ub, lb0, ub0)
        print("%s row %d %s: warm %s %.9f in %d rounds | cold %s %.9f in %d rounds | oracle %s %.9f | rebase_rows %d, bound %.9f" % (
            name, i, what, st, m.getobjval(), m.numiters(), st_cold, cold.getobjval(), cold.numiters(), ost, oobj, m.stat("rebase_rows"),
            m.getobjbound() if st == "Optimal" else math.nan))
        assert ost == "Optimal", (name, what, ost)                                # precondition: STEP keeps the problem feasible
        assert st == st_cold == ost, (name, what, st, st_cold, ost)
        assert kat_util.isapprox(m.getobjval(), cold.getobjval(), C.atol, C.rtol), (name, what, m.getobjval(), cold.getobjval())
        assert kat_util.isapprox(m.getobjval() + C.const, oobj, C.atol, C.rtol), (name, what, m.getobjval() + C.const, oobj)
        v = violation(C, m.getsolution()[:C.n], lb, ub)
        assert v <= F_TOL, (name, what, v)
        tol = max(C.atol, C.rtol * abs(oobj))
        assert sgn * (m.getobjbound() + C.const) <= sgn * oobj + tol, (name, what, m.getobjbound(), oobj)
        table.append((name, what, cold.numiters(), m.numiters()))
    return table


@pytest.fixture(scope="module")
def table():
    cache = {}

    def rows(name):
        if name not in cache:
            cache[name] = run_case(name)
        return cache[name]
    return rows


@pytest.mark.parametrize("name", list(CASES))
def test_warm_resolve_against_cold_and_oracle(name, table):
    assert len(table(name)) == 3


def test_rounds_table_is_written(table):
    """what is observed, not promised: cold against warm cutting-plane rounds over the cases (KTN_ROWBOUNDS_TABLE names a file)"""
    TABLE = [r for name in CASES for r in table(name)]
    cold, warm = sum(r[2] for r in TABLE), sum(r[3] for r in TABLE)
    lines = ["%-12s %-10s %6s %6s" % ("case", "change", "cold", "warm")] + ["%-12s %-10s %6d %6d" % r for r in TABLE]
    lines.append("%-12s %-10s %6d %6d" % ("total", "", cold, warm))
    print("\n".join(lines))
    out = os.environ.get("KTN_ROWBOUNDS_TABLE")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert len(TABLE) == 3 * len(CASES)


def test_crossed_and_impossible_linear_rows_end_infeasible_then_restore():
    C = InstCase()
    lb0, ub0, _ = row_data(C)
    m = fresh(C, lb0, ub0)
    assert m.optimize() == "Optimal"
    obj0, lp0 = m.getobjval(), m.stat("lp_solves")
    # a crossed linear row: no LP is solved
    k = 4
    lb, ub = lb0.copy(), ub0.copy()
    lb[k] = ub0[k] + 1.0
    m.setconstrbounds(lb, ub)
    assert m.stat("screen_crossed_rows") == 1
    assert m.optimize() == "Infeasible"
    assert m.stat("screen_crossed_rows") >= 1 and m.stat("lp_solves") == lp0
    # a linear row tightened past what the box allows: the screen proves it
    m.setconstrbounds(lb0, ub0)
    assert m.stat("screen_crossed_rows") == 0
    amin, _ = m.lp_row_activity()
    _, _, _, _, hi = m.lp_rows()
    assert math.isfinite(amin[k]) and math.isfinite(hi[k]) and amin[k] < hi[k]
    ub = ub0.copy()
    ub[k] = ub0[k] - (hi[k] - amin[k]) - 1.0                                       # the row's upper bound one unit below its smallest value over the box
    m.setconstrbounds(lb0, ub)
    assert m.optimize() == "Infeasible"
    assert m.stat("screen_infeasible_rows") >= 1 and m.stat("screen_first_row") <= k and m.stat("lp_solves") == lp0
    cold = fresh(C, lb0, ub)
    assert cold.optimize() == "Infeasible"
    # the original bounds: the original objective
    m.setconstrbounds(lb0, ub0)
    assert m.optimize() == "Optimal" and kat_util.isapprox(m.getobjval(), obj0, 1e-6, 1e-6)
    assert max_nl_violation(C.inst, m.getsolution()) <= F_TOL


def test_setter_before_the_first_solve_equals_loading_with_those_bounds():
    C = InstCase()
    lb0, ub0, cand = row_data(C)
    lb, ub = lb0.copy(), ub0.copy()
    ub[cand[0]] += 0.25
    ub[2] -= 0.125
    a = fresh(C, lb0, ub0)
    a.setconstrbounds(lb, ub)
    sa = a.optimize()
    b = fresh(C, lb, ub)
    sb = b.optimize()
    assert sa == sb and a.numiters() == b.numiters() and a.numcuts() == b.numcuts()
    assert a.getsolution().tobytes() == b.getsolution().tobytes() and a.getobjval() == b.getobjval()
