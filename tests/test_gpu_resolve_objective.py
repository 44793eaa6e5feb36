"""GPU tier: ktn_set_linear_objective and the re-solve from the kept cut pool (csrc/rebound.hip): the cost
is changed on the n = 40 separable instance and on a QuadNLP with a linear objective; the warm solve against a cold solve on a
fresh handle loaded with the new cost, against the CPU oracle (the instance) or the closed form (the ellipsoid of
tests/quad_cases.py: f* = c'x0 - sqrt(2 c'Q^-1 c)), and the reduced costs against tests/kkt_ref.py with the NEW objective."""
import copy
import math

import numpy as np
import pytest

import katana_jl_amd as ktn
import kat_util
import kkt_ref
import quad_cases as QC
from helpers import hip_load_instance, max_nl_violation, oracle_solve_instance

pytestmark = pytest.mark.gpu
L = ktn._lib


def instance(sense="Min"):
    inst = ktn.instances.make_instance(n=40, m_nl=6, k=8, family="explog", seed=11)
    if sense == "Max":                                    # the same problem stated as a maximisation of the negated cost
        inst = copy.copy(inst)
        inst.sense, inst.obj_p0, inst.obj_const = "Max", -np.asarray(inst.obj_p0), -inst.obj_const
    return inst


def with_cost(inst, c, c0):
    out = copy.copy(inst)
    out.obj_p0, out.obj_const = np.asarray(c, dtype=np.float64)[np.asarray(inst.obj_col)], float(c0)
    return out


@pytest.mark.parametrize("sense", ["Min", "Max"])
def test_cost_change_on_the_instance(sense):
    inst = instance(sense)
    assert np.all(np.asarray(inst.obj_kind) == L.ATOM_LIN) and len(set(inst.obj_col)) == len(inst.obj_col)
    m = hip_load_instance(ktn, inst)
    assert m.optimize() == "Optimal"
    cuts, rows = m.numcuts(), [a.tobytes() for a in m.lp_rows()]
    rng = np.random.default_rng(3)
    c = np.zeros(inst.n)
    c[np.asarray(inst.obj_col)] = np.asarray(inst.obj_p0) * rng.uniform(0.5, 1.5, len(inst.obj_col))
    c0 = 0.25
    m.setobj(c, c0)
    assert m.status() == "None" and m.numcuts() == cuts and [a.tobytes() for a in m.lp_rows()] == rows
    got_c, got_c0 = m.lp_objective()
    assert got_c[:inst.n].tobytes() == c.tobytes() and got_c0 == c0
    with pytest.raises(L.KatanaHipError) as e:
        m.getreducedcosts()
    assert e.value.code == L.E_INVALID
    st = m.optimize()
    new = with_cost(inst, c, c0)
    cold = hip_load_instance(ktn, new)
    st_cold = cold.optimize()
    om = oracle_solve_instance(new)
    print("%s: warm %s %.9f in %d rounds | cold %s %.9f in %d rounds | oracle %s %.9f" % (
        sense, st, m.getobjval(), m.numiters(), st_cold, cold.getobjval(), cold.numiters(), om.status, om.getobjval()))
    assert st == st_cold == om.status == "Optimal"
    assert kat_util.isapprox(m.getobjval(), cold.getobjval(), 1e-6, 1e-6) and kat_util.isapprox(m.getobjval(), om.getobjval(), 1e-6, 1e-6)
    x = m.getsolution()[:inst.n]
    assert max_nl_violation(inst, x) <= 1e-6
    # the report reads the new objective row: z = c_new - J(x*)'d
    d, z = m.getconstrduals(), m.getreducedcosts()
    R = kkt_ref.kkt_sep(new, x, d)
    assert np.all(np.abs(z - R.z) <= 2 * R.e_z), np.max(np.abs(z - R.z))
    old = kkt_ref.kkt_sep(inst, x, d)
    assert np.max(np.abs(z - old.z)) > 1e-3                                   # (and not the old one)
    # an entry outside the pattern
    if len(inst.obj_col) < inst.n:
        bad = c.copy()
        bad[np.setdiff1d(np.arange(inst.n), inst.obj_col)[0]] = 1.0
        with pytest.raises(L.KatanaHipError) as e:
            m.setobj(bad)
        assert e.value.code == L.E_INVALID


def test_cost_change_on_a_quadnlp_with_a_linear_objective():
    C = QC.ellipsoid(6)
    p = QC.ellipsoid_quad(C)
    m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))
    m.loadproblem(*p)
    assert m.optimize() == "Optimal" and abs(m.getobjval() - C.fstar) <= 1e-5
    c = C.c * np.linspace(0.6, 1.4, C.n)
    m.setobj(c)
    st = m.optimize()
    cold = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))
    r, cc, v = QC._full(C.Q)
    cold.loadproblem(*p._replace(d=ktn.QuadNLP(C.n, c, 0.0, None, [(np.arange(C.n), C.lin, r, cc, v, C.const)])))
    st_cold = cold.optimize()
    fstar = float(c @ C.x0 - math.sqrt(2.0 * (c @ np.linalg.solve(C.Q, c))))
    print("ellipsoid: warm %s %.9f in %d rounds | cold %s %.9f in %d rounds | closed form %.9f" % (
        st, m.getobjval(), m.numiters(), st_cold, cold.getobjval(), cold.numiters(), fstar))
    assert st == st_cold == "Optimal"
    assert abs(m.getobjval() - cold.getobjval()) <= 1e-5 and abs(m.getobjval() - fstar) <= 1e-5
    z, d = m.getreducedcosts(), m.getconstrduals()
    x = m.getsolution()[:C.n]
    want = c - d[0] * (C.Q @ x + C.lin)                                       # c_new - J(x*)'d
    assert np.max(np.abs(z - want)) <= 1e-9 * (1.0 + np.max(np.abs(want))), (z, want)


def test_refusals():
    # a nonlinear objective
    inst = ktn.instances.make_instance(n=40, m_nl=6, k=8, family="explog", seed=11, objective="quad")
    m = hip_load_instance(ktn, inst)
    with pytest.raises(L.KatanaHipError) as e:
        m.setobj(np.zeros(inst.n))
    assert e.value.code == L.E_UNSUPPORTED
    # an entry outside the pattern of a QuadNLP's objective
    C = QC.ellipsoid(4)
    c = C.c.copy()
    c[1] = 0.0
    r, cc, v = QC._full(C.Q)
    q = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))
    q.loadproblem(*QC.ellipsoid_quad(C)._replace(d=ktn.QuadNLP(C.n, c, 0.0, None, [(np.arange(C.n), C.lin, r, cc, v, C.const)])))
    with pytest.raises(L.KatanaHipError) as e:
        q.setobj(C.c)
    assert e.value.code == L.E_INVALID
    q.setobj(2.0 * c)                                                         # inside it: accepted before the first solve too
    assert q.optimize() == "Optimal"


def test_linear_quadratic_model_reloads_for_a_cost_outside_the_loaded_pattern():
    # min x0  s.t.  x0 + x1 >= 1, 0 <= x <= 2: the loaded cost has no entry on x1
    m = ktn.LinearQuadraticModel(ktn.KatanaSolver(log_level=0))
    m.loadproblem(np.array([[1.0, 1.0]]), [0.0, 0.0], [2.0, 2.0], [1.0, 0.0], [1.0], [np.inf], "Min")
    assert m.optimize() == "Optimal" and abs(m.getobjval()) <= 1e-6
    m.setobj([3.0, 0.0])                                                      # inside the pattern: in place, the handle is not re-loaded
    assert not m._lq["dirty"] and m.status() == "None"
    assert m.optimize() == "Optimal" and abs(m.getobjval()) <= 1e-6
    m.setobj([1.0, 2.0])                                                      # outside it: the next optimize() loads the LP again
    assert m._lq["dirty"]
    assert m.optimize() == "Optimal" and abs(m.getobjval() - 1.0) <= 1e-6
    assert abs(m.getsolution()[0] - 1.0) <= 1e-5
