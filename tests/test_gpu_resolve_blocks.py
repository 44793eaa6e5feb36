"""GPU tier: FusedBatch.set_var_bounds / set_costs (ktn_set_var_bounds, ktn_set_linear_objective on a fused batch; DESIGN.md
section 14): six small instances solved by the device-side loop, new bounds on two of them, and the records and solutions of the
next solve() against a fresh FusedBatch built from the modified instances -- bit for bit; the four untouched instances' records
equal their records before the change."""
import copy

import numpy as np
import pytest

import katana_jl_amd as ktn
from katana_jl_amd.batch import FusedBatch

pytestmark = pytest.mark.gpu


def instances():
    return [ktn.instances.make_instance(n=24, m_nl=4, k=6, family="explog" if s % 2 else "quad", seed=40 + s) for s in range(6)]


def records(fb):
    return fb.m.blocks_results().copy()


def test_bounds_on_two_instances_equal_a_fresh_batch():
    insts = instances()
    solver = ktn.KatanaSolver(log_level=0)
    fb = FusedBatch(solver, insts)
    out0 = fb.solve()
    assert all(o["status"] == "Optimal" for o in out0) and fb.m.stat("ecp_blocks_launches") == 1
    rec0 = records(fb).reshape(len(insts), -1)
    mod = [copy.copy(i) for i in insts]
    l_list, u_list = [None] * 6, [None] * 6
    for k in (1, 4):                                       # both bounds of every variable three quarters of the way towards the solution
        x = out0[k]["x"]
        l, u = x - 0.25 * (x - insts[k].l_var), x + 0.25 * (insts[k].u_var - x)
        l_list[k], u_list[k] = l, u
        mod[k].l_var, mod[k].u_var = l, u
    fb.set_var_bounds(l_list, u_list)
    out1 = fb.solve()
    rec1 = records(fb).reshape(len(insts), -1)
    fresh = FusedBatch(solver, mod)
    out2 = fresh.solve()
    rec2 = records(fresh).reshape(len(insts), -1)
    assert fb.m.stat("ecp_blocks_fallbacks") == 0 and fresh.m.stat("ecp_blocks_fallbacks") == 0
    assert rec1.tobytes() == rec2.tobytes()
    for a, b in zip(out1, out2):
        assert a["status"] == b["status"] == "Optimal" and a["x"].tobytes() == b["x"].tobytes() and a["objval"] == b["objval"]
    for k in (0, 2, 3, 5):
        assert rec1[k].tobytes() == rec0[k].tobytes(), k
    for k in (1, 4):                                       # x* of the first solve is still feasible: the same optimum, inside the new box
        assert abs(out1[k]["objval"] - out0[k]["objval"]) <= 1e-5 * max(1.0, abs(out0[k]["objval"]))
        assert np.all(out1[k]["x"] <= u_list[k]) and np.all(out1[k]["x"] >= l_list[k])


def test_costs_on_two_instances_equal_a_fresh_batch():
    insts = instances()
    solver = ktn.KatanaSolver(log_level=0)
    fb = FusedBatch(solver, insts)
    fb.solve()
    mod = [copy.copy(i) for i in insts]
    c_list = [None] * 6
    for k in (0, 3):
        c = np.zeros(insts[k].n)
        c[np.asarray(insts[k].obj_col)] = 1.25 * np.asarray(insts[k].obj_p0)
        c_list[k] = c
        mod[k].obj_p0 = c[np.asarray(insts[k].obj_col)]
    fb.set_costs(c_list)
    out1 = fb.solve()
    fresh = FusedBatch(solver, mod)
    out2 = fresh.solve()
    assert records(fb).tobytes() == records(fresh).tobytes()
    for a, b in zip(out1, out2):
        assert a["status"] == b["status"] == "Optimal" and a["x"].tobytes() == b["x"].tobytes() and a["objval"] == b["objval"]
