"""GPU tier: ktn_blocks_get_feasible_points / FusedBatch.feasible_points (csrc/feas.hpp): five small instances
fused into one block-diagonal problem and solved by the device-side loop -- one without nonlinear rows, one with an infeasible
reference point, one Max.  Every instance's answer is the single-handle answer of the same instance with the same x* and x_in, to
the bit in lambda and x_feas (the single handle takes x* through ktn_sep_precompute: KTN_FEAS_XSTAR_PRECOMPUTE)."""
import math

import numpy as np
import pytest

import katana_jl_amd as ktn
import kkt_cases
from katana_jl_amd.batch import FusedBatch

pytestmark = pytest.mark.gpu
L = ktn._lib
G = 8                                                              # one lane-group width on both sides (KTN_FEAS_GROUP)


def _lp_only(n=4):
    """min -sum x  s.t.  sum x <= 1, x in [-2, 2]: no nonlinear row"""
    A = kkt_cases
    return A._inst(n, "Min", [-2.0] * n, [2.0] * n, [([(j, A.ATOM_LIN, 1.0, 0.0) for j in range(n)], 0.0, -np.inf, 1.0)],
                   [(j, A.ATOM_LIN, -1.0, 0.0) for j in range(n)])


@pytest.fixture(scope="module")
def batch():
    cases = [kkt_cases.build("a", 4), None, kkt_cases.build("c", 4), kkt_cases.build("f", 4), kkt_cases.build("d", 8)]
    insts = [c.inst if c is not None else _lp_only() for c in cases]
    # the optimum, and the multipliers of the LINEAR rows at it: x_feas may violate a linear row by info[4] (the LP's tolerance; linear
    # rows are not searched), which moves the optimum by at most that times the row's multiplier
    fstars = [(c.fstar, float(np.abs(c.ds[:c.inst.m_lin]).sum())) if c is not None else (-1.0, 1.0) for c in cases]
    probs = [ktn.Problem(i.n, i.num_constr, i.l_var, i.u_var, i.l_constr, i.u_constr, i.sense, ktn.SeparableNLP(i)) for i in insts]
    points = [np.zeros(p.num_var) for p in probs]
    points[2] = np.full(4, 0.9)                                    # violates sum x^2 <= 1: this instance has no usable reference point
    return insts, probs, points, fstars


def test_each_instance_equals_its_single_handle_answer(monkeypatch, batch):
    insts, probs, points, fstars = batch
    monkeypatch.setenv("KTN_FEAS_GROUP", str(G))
    monkeypatch.delenv("KTN_FEAS_XSTAR_PRECOMPUTE", raising=False)
    fb = FusedBatch(ktn.KatanaSolver(log_level=0, lp_max_iter=400000), probs, False, True)
    fb.set_interior_points(points)
    res = fb.solve(cut_capacity=128)
    assert res[0]["ecp_blocks_launches"] == 1 and res[0]["ecp_blocks_fallbacks"] == 0      # the device-side loop ended the batch
    assert fb.m.stat("feas_evals") == 0
    fps = fb.feasible_points()
    again = fb.feasible_points()
    assert fb.m.stat("feas_evals") == 1 and len(fps) == 5
    bounds = fb.dual_bounds()
    x = fb.m.getsolution()
    monkeypatch.setenv("KTN_FEAS_XSTAR_PRECOMPUTE", "1")
    for k, (inst, p, fp) in enumerate(zip(insts, probs, fps)):
        assert again[k].x.tobytes() == fp.x.tobytes() and again[k].found == fp.found
        xs = x[int(fb.offs[k]):int(fb.offs[k + 1])]
        m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))
        m.loadproblem(*p)
        m.set_interior_point(points[k])
        m.lp_solve()
        sep = ktn.KatanaHipSeparator(m)
        sep.initialize()
        sep.precompute(xs)
        one = m.feasible_point()
        print("instance %d (%s): found %d / %d  lambda %.17g  f(x_feas) %.12g  bound %.12g  blocking %d  back-offs %d"
              % (k, inst.sense, fp.found, one.found, fp.lam, fp.objval, bounds[k][0], fp.blocking_row, fp.backoffs))
        assert fp.found == one.found == (-1 if k == 2 else 1), k
        assert len(fp.x) == inst.n and fp.x.tobytes() == one.x.tobytes(), k
        assert fp.blocking_row == one.blocking_row and fp.unconverged == one.unconverged and fp.backoffs == one.backoffs, k
        if k == 2:
            assert np.isnan(fp.x).all() and fp.blocking_row == inst.num_constr - 1      # the first offending row: the ball, behind the linear row
            continue
        assert np.float64(fp.lam).tobytes() == np.float64(one.lam).tobytes(), (k, fp.lam, one.lam)
        assert fp.nl_margin == one.nl_margin and fp.lin_viol == one.lin_viol, k
        assert abs(fp.objval - one.objval) <= 1e-12 * (1.0 + abs(one.objval)), (k, fp.objval, one.objval)
        s = -1.0 if inst.sense == "Max" else 1.0
        fstar, dlin = fstars[k]
        tol = 1e-9 * (1.0 + abs(fstar)) + dlin * fp.lin_viol
        assert s * bounds[k][0] - tol <= s * fstar <= s * fp.objval + tol, (k, bounds[k][0], fstar, fp.objval)
    assert fps[1].lam == 1.0 and fps[1].blocking_row == -1 and fps[1].nl_margin == -math.inf      # no nonlinear rows: lambda_b = 1
    assert fps[3].objval > 0 and fps[0].objval < 0                                                 # each in its own sense


def test_count_only_and_small_buffers(batch):
    insts, probs, points, fstars = batch
    fb = FusedBatch(ktn.KatanaSolver(log_level=0), probs, False, True)
    m = fb.m
    import ctypes as C
    n = C.c_int64(0)
    null = C.POINTER(C.c_double)()
    assert m._lib.ktn_blocks_get_feasible_points(m._h, null, 0, null, 0, C.byref(n)) == 0 and n.value == 8 * 5
    x, info = np.zeros(m.num_var), np.zeros(8 * 5)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert m._lib.ktn_blocks_get_feasible_points(m._h, p(x), len(x), p(info), 39, C.byref(n)) == L.E_INVALID
    assert m._lib.ktn_blocks_get_feasible_points(m._h, p(x), len(x), p(info), 40, C.byref(n)) == L.E_INVALID      # no LP solve yet
    assert "no LP solve" in m._lib.ktn_last_error(m._h).decode()
