"""GPU tier: the screen that follows ktn_set_var_bounds (csrc/rebound.hpp k_row_activity<G>, k_rebound)
against the exact reference tests/rebound_ref.py, which tests/test_rebound_ref.py pins on the CPU -- for every lane-group width,
at the row lengths around it, with coefficients of both signs and exact zeros, columns with one or two infinite bounds and
fixed columns -- and the engine driven through it: a crossed column, a tight but feasible box."""
import math

import numpy as np
import pytest

import katana_jl_amd as ktn
import rebound_cases as RC
import rebound_ref as R
from helpers import hip_load_instance

pytestmark = pytest.mark.gpu
L = ktn._lib
INF = math.inf
EPS = 2.0 ** -52


def base_model(n):
    """n variables in [-10, 10], one linear row x_0 + x_1 <= 15, minimise sum x: the small loaded problem the cases' rows are appended to"""
    d = ktn.NLPDescription(n, [0, 2], [0, 1], [L.ROW_SEP], [1], [0.0], [0, 0], [1.0, 1.0], [0.0, 0.0], obj_linear=True,
                           obj_kind=L.ROW_SEP, obj_col=np.arange(n), obj_atom_kind=np.zeros(n), obj_p0=np.ones(n), obj_p1=np.zeros(n))
    m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))
    m.loadproblem(n, 1, np.full(n, -10.0), np.full(n, 10.0), [-INF], [15.0], "Min", d)
    return m


def loaded(case):
    m = base_model(case["n"])
    m.lp_append_rows(case["rowptr"], case["col"], case["val"], case["lo"], case["hi"])
    m.setvarbounds(case["l"], case["u"])
    return m


def check_against_reference(m, case, exact):
    """amin / amax of every row the engine holds (the base row included) against the reference on those very rows; returns the
    reference's (count, first, redundant)"""
    amin, amax = m.lp_row_activity()
    assert m.stat("screen_group") == case["G"], (m.stat("screen_group"), case["G"])
    rp, col, val, lo, hi = m.lp_rows()
    assert len(amin) == len(lo) == len(case["lo"]) + 1 <= 48
    rows, count, first, red, crossed = R.screen(rp, col, val, lo, hi, case["l"], case["u"], RC.TOL0)
    worst = 0.0
    for k, r in enumerate(rows):
        n_k = int(rp[k + 1] - rp[k])
        bound = (n_k + 2) * EPS * float(r["S"])
        for got, want in ((amin[k], r["amin"]), (amax[k], r["amax"])):
            if isinstance(want, float):                                       # infinite exactly where the reference has it
                assert got == want, (case["G"], k, got, want)
                continue
            assert math.isfinite(got), (case["G"], k, got)
            err = abs(float(R.Fraction(float(got)) - want))
            if exact:
                assert err == 0.0, (case["G"], k, got, float(want))
            assert err <= bound, (case["G"], k, n_k, err, bound)
            worst = max(worst, err / bound if bound > 0 else 0.0)
    print("G %d: %d rows, largest error over its bound %.3g; proving %d first %d redundant %d" % (case["G"], len(rows), worst, count, first, red))
    assert m.stat("activity_infeasible_rows") == count and m.stat("activity_first_row") == first
    return count, first, red


@pytest.mark.parametrize("G", [4, 8, 16, 32, 64])
def test_row_activity_far_from_the_threshold(G):
    case = RC.group_case(G)
    m = loaded(case)
    count, first, red = check_against_reference(m, case, exact=False)
    assert count == sum(case["want"]) and first == 1 + case["want"].index(True)       # (row 0 is the base problem's)
    # the engine: the solve ends at the screen, before any LP
    lp0 = m.stat("lp_solves")
    assert m.optimize() == "Infeasible" and m.status() == "Infeasible"
    assert m.stat("screen_runs") == 1 and m.stat("screen_infeasible_rows") == count and m.stat("screen_first_row") == first
    assert m.stat("screen_crossed_cols") == 0 and m.stat("lp_solves") == lp0 and m.numiters() == 0


@pytest.mark.parametrize("G", [4, 8, 16, 32, 64])
def test_verdicts_one_float_either_side_of_the_threshold(G):
    case = RC.grid_case(G)
    m = loaded(case)
    count, first, red = check_against_reference(m, case, exact=True)
    assert count == sum(case["want"]) == len(case["want"]) // 2 and first == 1
    assert m.stat("activity_redundant_rows") == red
    # row by row: with the proving rows' bounds opened, what is left proves nothing -- the 'not proving' halves of the pairs hold
    keep = np.asarray(case["want"])
    lo, hi = case["lo"].copy(), case["hi"].copy()
    lo[keep], hi[keep] = -INF, INF
    m2 = loaded(dict(case, lo=lo, hi=hi))
    m2.lp_row_activity()
    assert m2.stat("activity_infeasible_rows") == 0 and m2.stat("activity_first_row") == -1


def test_clamp_counts_and_buffer_size():
    case = RC.group_case(8)
    m = base_model(case["n"])
    x0 = m.getsolution()
    assert not np.any(x0)                                                     # the loaded point is the origin
    l, u = case["l"].copy(), case["u"].copy()
    u[5], l[5] = 1.0, 2.0                                                     # one crossed column
    m.setvarbounds(l, u)
    want, moved, crossed = R.clamp(list(x0[:case["n"]]), list(l), list(u))
    assert crossed == 1
    assert m.getsolution()[:case["n"]].tobytes() == np.asarray(want).tobytes()
    assert m.stat("warm_clamped_cols") == moved > 0
    amin, amax = np.zeros(1), np.zeros(1)
    m.lp_append_rows(case["rowptr"], case["col"], case["val"], case["lo"], case["hi"])
    with pytest.raises(L.KatanaHipError) as e:                                # m < M
        L.check(m._h, m._lib.ktn_lp_row_activity(m._h, amin.ctypes.data_as(L.P(L.c_f64)), amax.ctypes.data_as(L.P(L.c_f64)), 1))
    assert e.value.code == L.E_INVALID
    with pytest.raises(L.KatanaHipError) as e:
        m.setvarbounds(np.full(case["n"], np.nan), None)
    assert e.value.code == L.E_INVALID


def test_nan_coefficient_proves_nothing():
    m = base_model(16)
    m.lp_append_rows([0, 2, 4], [2, 3, 4, 5], [1.0, float("nan"), 1.0, 1.0], [-INF, -INF], [-100.0, -100.0])
    amin, amax = m.lp_row_activity()
    assert amin[1] == -INF and amax[1] == INF                                # the row with the NaN: both sides undecidable
    assert amin[2] == -20.0 and amax[2] == 20.0 and m.stat("activity_infeasible_rows") == 1 and m.stat("activity_first_row") == 2
    rp, col, val, lo, hi = m.lp_rows()
    rows, count, first, red, crossed = R.screen(rp, col, val, lo, hi, np.full(16, -10.0), np.full(16, 10.0), RC.TOL0)
    assert (count, first) == (1, 2) and rows[1]["amin"] == -INF and rows[1]["amax"] == INF


def test_engine_crossed_column_and_tight_box():
    inst = ktn.instances.make_instance(n=40, m_nl=6, k=8, family="explog", seed=11)
    m = hip_load_instance(ktn, inst)
    assert m.optimize() == "Optimal"
    obj, x = m.getobjval(), m.getsolution()[:inst.n]
    cuts, lp0 = m.numcuts(), m.stat("lp_solves")
    # a crossed column alone
    l, u = inst.l_var.copy(), inst.u_var.copy()
    l[3], u[3] = x[3] + 0.5, x[3] - 0.5
    m.setvarbounds(l, u)
    assert m.status() == "None" and m.numcuts() == cuts
    assert m.optimize() == "Infeasible"
    assert m.stat("screen_crossed_cols") == 1 and m.stat("lp_solves") == lp0 and m.numiters() == 0
    # a tight but feasible box around the solution is not flagged, and the solve from the kept pool finds the optimum again
    m.setvarbounds(np.maximum(inst.l_var, x - 1e-3), np.minimum(inst.u_var, x + 1e-3))
    assert m.optimize() == "Optimal"
    assert m.stat("screen_runs") == 2 and m.stat("screen_infeasible_rows") == 0 and m.stat("screen_crossed_cols") == 0
    assert m.stat("lp_solves") > lp0 and m.numcuts() >= cuts
    assert abs(m.getobjval() - obj) <= 1e-6 * max(1.0, abs(obj))
    # the screen runs once per change of bounds: a solve without one launches none
    m.reset()
    assert m.optimize() == "Optimal" and m.stat("screen_runs") == 2
