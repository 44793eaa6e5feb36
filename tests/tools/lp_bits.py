"""What the three PDHG loops decide, dumped bit for bit -- the tool for comparing two builds of the library on the LP side.

    KTN_LIB=/path/to/libkatana_hip.so python tests/tools/lp_bits.py dump OUT.npz
    python tests/tools/lp_bits.py compare A.npz B.npz          # one line per array; exit status 1 on any difference

`dump` runs whole solves at the tests' own small sizes through each loop that takes check decisions:
  host/...    Engine::lp_solve_core: the reference KATs and the six fuzz models of tests/test_gpu_kats.py, a quad-objective instance
              (stalled-row exit, consolidation), an explog instance at the default parameters and with lp_stag_factor = 0, and a model
              with a free variable (the has_inf_bound rules).  Per solve: status, the LP counters, numiters, objective, x.
  blocks/...  k_pdhg_blocks: solve_batch(fused, per_instance_lp) on 16 cfg5_one instances.  Per instance status, objective, x; the
              launch counters.
  ecp/...     k_ecp_blocks<0> and <1>: the 16-instance batch of tests/test_gpu_blocks_supporting.py with and without supporting
              cuts and the 16-instance tape batch of tests/test_gpu_batch_tapes.py.  Per instance the eight result slots and x, the
              lambdas of every cut row, and the supporting-hyperplane counters summed over the batch (the ABI has no per-instance
              accessor for them).
One process per build (KTN_LIB is read at import); `compare` needs no GPU."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from sweep_bits import compare     # noqa: E402  (the same array-by-array comparison)

LP_STATS = ("pdhg_iters", "lp_restarts", "lp_eta_backoffs", "lp_divergence_backoffs", "lp_stagnation_exits", "lp_stalled_row_exits",
            "lp_consolidations", "lp_solves")
STATUS = ("Optimal", "Infeasible", "Unbounded", "UserLimit", "Error")


def status_code(s):
    return float(STATUS.index(s)) if s in STATUS else -1.0


def record(out, name, status, im, objval, x):
    out[name + "/status_counters"] = np.array([status_code(status)] + [im.stat(s) for s in LP_STATS] + [float(im.numiters())])
    out[name + "/objval"] = np.array([float(objval)])
    out[name + "/x"] = np.asarray(x, dtype=np.float64).copy()


def host_cases(ktn, out):
    from fuzz_models import model_at
    from helpers import hip_load_instance, hip_model_from_kat
    from kat_util import load_kats
    todo = [("kat_" + m["id"], m, {}) for m in load_kats()]
    todo += [("fuzz_%d_%d" % (s, i), model_at(s, i), dict(lp_max_iter=400000))
             for s, i in ((2, 62), (2, 138), (2, 109), (13, 142), (55, 106), (144, 51))]
    for name, m, kw in todo:
        M = hip_model_from_kat(ktn, m, **kw)
        status = M.solve()
        im = M.internal_model
        record(out, "host/" + name, status, im, im.getobjval(), im.getsolution())
    print("host: %d small models" % len(todo), flush=True)
    make = ktn.instances.make_instance
    for name, inst, kw in (("quad3000", make(n=3000, m_nl=300, k=16, family="quad", seed=1, objective="quad"), {}),
                           ("explog5000", make(n=5000, m_nl=500, k=32, family="explog", seed=7), {}),
                           ("explog5000_stag0", make(n=5000, m_nl=500, k=32, family="explog", seed=7), dict(lp_stag_factor=0.0))):
        im = hip_load_instance(ktn, inst, **kw)
        status = im.optimize()
        record(out, "host/" + name, status, im, im.getobjval(), im.getsolution())
        print("host: %s %s, %d PDHG iterations, %d stagnation / %d stalled-row exits, %d consolidations" % (
            name, status, im.stat("pdhg_iters"), im.stat("lp_stagnation_exits"), im.stat("lp_stalled_row_exits"), im.stat("lp_consolidations")), flush=True)
    # a free variable: min t  s.t.  exp(y) + y^2 <= t,  y in [-2, 2],  t free
    t, y = ktn.var(0), ktn.var(1)
    M = ktn.Model(solver=ktn.KatanaSolver(log_level=0))
    M.variable()
    M.variable(-2.0, 2.0)
    M.objective("Min", t)
    M.constraint(ktn.exp(y) + y ** 2 - t <= 0.0)
    status = M.solve()
    record(out, "host/free_variable", status, M.internal_model, M.internal_model.getobjval(), M.internal_model.getsolution())


def blocks_cases(ktn, out):
    from katana_jl_amd.batch import FusedBatch
    insts = [ktn.instances.make_config("cfg5_one", seed=s) for s in range(16)]
    fb = FusedBatch(ktn.KatanaSolver(log_level=0), insts, per_instance_lp=True, device_loop=False)     # = solve_batch(fused, per_instance_lp)
    res = fb.solve()
    out["blocks/status"] = np.array([status_code(r["status"]) for r in res])
    out["blocks/objval"] = np.array([r["objval"] for r in res])
    out["blocks/x"] = np.concatenate([r["x"] for r in res])
    out["blocks/counters"] = np.array([fb.m.stat(s) for s in ("blk_lp_launches", "blk_pdhg_iters_sum", "blk_pdhg_iters_max", "blk_lp_fallbacks",
                                                              "pdhg_iters")] + [float(fb.m.numiters())])
    print("blocks: %d launches, %d fallbacks" % (res[0]["blk_lp_launches"], res[0]["blk_lp_fallbacks"]), flush=True)


def ecp_record(out, name, fb, res):
    m = fb.m
    out[name + "/results"] = m.blocks_results()
    out[name + "/x"] = np.concatenate([r["x"] for r in res])
    out[name + "/objval"] = np.array([r["objval"] for r in res])
    out[name + "/status"] = np.array([status_code(r["status"]) for r in res])
    out[name + "/lam"] = np.concatenate([m.blocks_cuts(b)["lam"] for b in range(len(res))])
    out[name + "/esh_counters"] = np.array([m.stat(s) for s in ("esh_rows", "esh_fallback_rows", "esh_newton_steps", "esh_quad_rows")])
    out[name + "/launch_counters"] = np.array([m.stat(s) for s in ("ecp_blocks_launches", "ecp_blocks_fallbacks", "ecp_blocks_pdhg_sum")])
    print("%s: %d launches, %d fallbacks, %d PDHG iterations" % (name, m.stat("ecp_blocks_launches"), m.stat("ecp_blocks_fallbacks"),
                                                                 m.stat("ecp_blocks_pdhg_sum")), flush=True)


def ecp_cases(ktn, out):
    from fuse_helpers import expr_problem, separable_problem
    from katana_jl_amd.batch import FusedBatch
    F_TOL = 1e-6                                  # (tests/test_gpu_supporting_hyperplanes.py)
    make = ktn.instances.make_instance
    insts = [make(n=200, m_nl=20, k=8, family=f, seed=s) for f in ("explog", "quad") for s in range(8)]
    for name, algo, supporting in (("kelley", "kelley", False), ("supporting", "supporting_hyperplane", True)):
        fb = FusedBatch(ktn.KatanaSolver(log_level=0, f_tol=F_TOL, cut_algo=algo, lp_max_iter=400000), insts)
        res = fb.solve(cut_capacity=48, supporting=supporting)
        ecp_record(out, "ecp/" + name, fb, res)
    insts = [make(n=300, m_nl=30, k=8, family="explog", seed=700 + s) for s in range(16)]
    probs = [separable_problem(i) if s % 2 == 0 else expr_problem(i) for s, i in enumerate(insts)]
    fb = FusedBatch(ktn.KatanaSolver(log_level=0, lp_max_iter=400000), probs)
    ecp_record(out, "ecp/tapes", fb, fb.solve())


def dump(path):
    import katana_jl_amd as ktn
    out = {}
    for part in (host_cases, blocks_cases, ecp_cases):
        part(ktn, out)
        print("%s: %d arrays so far" % (part.__name__, len(out)), flush=True)
    np.savez(path, **out)
    print("library %s: %d arrays -> %s" % (ktn._lib.LIB_PATH, len(out), path))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
