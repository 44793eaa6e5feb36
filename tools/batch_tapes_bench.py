"""Throughput mode for expression-built models: 512 x cfg5 three ways, alternated round by round.

  (a) separable   -- SeparableInstances through the device loop (FusedBatch: fuse_instances + ktn_optimize_blocks)
  (b) expressions -- the same instances written as expressions (ExprNLP: every NL row a tape), fused by nlp.fuse_problems,
                     through the device loop
  (c) per-handle  -- the expression form, one handle per instance, ordinary loop, 16 host threads (solve_batch)

Each line: solve seconds, seconds including load (fusion + ktn_loadproblem [+ ktn_set_blocks]), instances/s including load,
and the largest objective difference against the planted optimum.  Building the expressions is reported once (describe_s).
Usage: python tools/batch_tapes_bench.py [instances=512] [rounds=3] [threads=16]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import katana_jl_amd as ktn                                        # noqa: E402
from katana_jl_amd.batch import FusedBatch                          # noqa: E402
from fuse_helpers import expr_problem                               # noqa: E402

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 512
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
threads = int(sys.argv[3]) if len(sys.argv) > 3 else 16
insts = [ktn.instances.make_config("cfg5_one", seed=s) for s in range(nb)]
t0 = time.perf_counter()
probs = [expr_problem(i) for i in insts]
print(json.dumps({"instances": nb, "describe_s": time.perf_counter() - t0}), flush=True)


def solver():
    return ktn.KatanaSolver(log_level=0, lp_max_iter=400000)


def report(mode, rnd, res, solve_s, total_s):
    err = max(abs(r["objval"] - i.opt_obj) / max(1.0, abs(i.opt_obj)) for r, i in zip(res, insts))
    line = {"mode": mode, "round": rnd, "instances": len(res), "optimal": sum(r["status"] == "Optimal" for r in res),
            "solve_s": solve_s, "total_s": total_s, "instances_per_s": len(res) / total_s, "max_obj_relerr": err}
    for k in ("ecp_blocks_launches", "ecp_blocks_fallbacks", "ecp_blocks_tape_rows", "ecp_blocks_pdhg_sum"):
        if k in res[0]:
            line[k] = res[0][k]
    print(json.dumps(line), flush=True)


def fused(items):
    t0 = time.perf_counter()
    fb = FusedBatch(solver(), items)
    t1 = time.perf_counter()
    res = fb.solve()
    t2 = time.perf_counter()
    return res, t2 - t1, t2 - t0


for rnd in range(rounds):
    res, s, t = fused(insts)
    report("a_separable_device_loop", rnd, res, s, t)
    res, s, t = fused(probs)
    report("b_expressions_device_loop", rnd, res, s, t)
    res, wall = ktn.solve_batch(solver(), probs, threads=threads)
    report("c_expressions_per_handle_%d_threads" % threads, rnd, res, wall, wall)
