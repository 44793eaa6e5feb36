"""GPU tier: throughput mode for expression-built models -- fused batches of Problems with tape rows solved by the
device-side loop (ktn_optimize_blocks, k_ecp_blocks evaluating tape rows), against the separable device loop, closed
forms and the ordinary loop."""
import math

import numpy as np
import pytest

import katana_jl_amd as ktn
from katana_jl_amd.batch import FusedBatch
from fuse_helpers import expr_problem, julia_problem, separable_problem
from helpers import assert_planted_objective

pytestmark = pytest.mark.gpu


def solver():
    return ktn.KatanaSolver(log_level=0, lp_max_iter=400000)


def close(a, b):
    return abs(a - b) <= max(1e-6, 1e-6 * max(abs(a), abs(b)))


def assert_device_loop(res, tape_rows):
    assert res[0]["ecp_blocks_launches"] == 1 and res[0]["ecp_blocks_fallbacks"] == 0, res[0]
    assert res[0]["ecp_blocks_tape_rows"] == tape_rows


@pytest.fixture(scope="module")
def cfg5():
    insts = [ktn.instances.make_config("cfg5_one", seed=s) for s in range(64)]
    sep = FusedBatch(solver(), insts).solve()
    assert sep[0]["ecp_blocks_launches"] == 1 and sep[0]["ecp_blocks_fallbacks"] == 0
    return insts, sep


def check_cfg5(res, insts, sep):
    for r, s, inst in zip(res, sep, insts):
        assert r["status"] == "Optimal"
        assert_planted_objective(r["objval"], inst)
        assert close(r["objval"], s["objval"]), (r["objval"], s["objval"])


def test_cfg5_batch_as_expressions_runs_in_the_device_loop(cfg5):
    insts, sep = cfg5
    res = FusedBatch(solver(), [expr_problem(i) for i in insts]).solve()
    assert_device_loop(res, 64 * 100)
    check_cfg5(res, insts, sep)


def test_cfg5_batch_julia_shaped_runs_in_the_device_loop(cfg5):
    insts, sep = cfg5
    rng = np.random.default_rng(5)
    res = FusedBatch(solver(), [julia_problem(i, rng) for i in insts]).solve()
    assert_device_loop(res, 64 * 100)
    check_cfg5(res, insts, sep)


def cone_model(rng, ub_x=2.0):
    """Katana.jl's documentation example, four times: (x, y, z) in [-2, 2]^3 with sqrt(x^2 + y^2) <= z - 0.25 and
    x^2 + y^2 <= 1 - z, which together confine (x, y) to the disk of radius 0.5; objective sum a x + b y"""
    M = ktn.Model(None)
    obj, best = 0.0, 0.0
    for blk in range(4):
        x = M.variable(-2.0, ub_x if blk == 0 else 2.0)
        y, z = M.variable(-2.0, 2.0), M.variable(-2.0, 2.0)
        M.constraint(ktn.sqrt(x * x + y * y) <= z - 0.25)
        M.constraint(x * x + y * y <= 1.0 - z)
        M.constraint(x + y + z <= 3.0)                  # (a linear row that never binds)
        a, b = rng.uniform(0.5, 2.0, 2) * rng.choice([-1.0, 1.0], 2)
        obj = obj + a * x + b * y
        best -= 0.5 * math.hypot(a, b)
    M.objective("Min", obj)
    return M, best


def ordinary(models):
    out, _ = ktn.solve_batch(solver(), models, threads=16)
    return out


def test_rows_that_are_not_separable_cone_and_paraboloid():
    rng = np.random.default_rng(11)
    cases = [cone_model(rng) for _ in range(128)]
    models = [m for m, _ in cases]
    res = FusedBatch(solver(), models).solve(cut_capacity=48)
    assert_device_loop(res, 128 * 8)
    ref = ordinary(models)
    for r, o, (_, best) in zip(res, ref, cases):
        assert r["status"] == "Optimal" and o["status"] == "Optimal"
        assert close(r["objval"], best), (r["objval"], best)
        assert close(r["objval"], o["objval"]), (r["objval"], o["objval"])


def test_mixed_batch_of_separable_and_tape_descriptions():
    insts = [ktn.instances.make_instance(n=300, m_nl=30, k=8, family="explog", seed=700 + s) for s in range(16)]
    probs = [separable_problem(i) if s % 2 == 0 else expr_problem(i) for s, i in enumerate(insts)]
    res = FusedBatch(solver(), probs).solve()
    assert_device_loop(res, 8 * 30)
    ref = ordinary(probs)
    for r, o, inst in zip(res, ref, insts):
        assert r["status"] == "Optimal" and o["status"] == "Optimal"
        assert_planted_objective(r["objval"], inst)
        assert close(r["objval"], o["objval"]), (r["objval"], o["objval"])


def test_tape_batches_that_do_not_qualify_still_fall_back():
    rng = np.random.default_rng(12)
    # one infinite variable bound: not launched; the host-driven loop answers like the ordinary one
    cases = [cone_model(rng, ub_x=math.inf if k == 3 else 2.0) for k in range(8)]
    models = [m for m, _ in cases]
    res = FusedBatch(solver(), models).solve()
    assert res[0]["ecp_blocks_launches"] == 0
    ref = ordinary(models)
    for r, o, (_, best) in zip(res, ref, cases):
        assert r["status"] == "Optimal" and o["status"] == "Optimal"
        assert close(r["objval"], o["objval"]) and close(r["objval"], best), (r["objval"], o["objval"], best)
    # room for one cut per NL row: a curved face overflows its arena and the batch comes from the host-driven loop
    cases = [cone_model(rng) for _ in range(8)]
    res = FusedBatch(solver(), [m for m, _ in cases]).solve(cut_capacity=1)
    assert res[0]["ecp_blocks_launches"] == 1 and res[0]["ecp_blocks_fallbacks"] == 1
    for r, (_, best) in zip(res, cases):
        assert r["status"] == "Optimal"
        assert close(r["objval"], best), (r["objval"], best)
