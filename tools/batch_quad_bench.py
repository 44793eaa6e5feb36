"""Throughput mode on declared-quadratic rows: 512 instances shaped like cfg5 (n=1000, m_nl=100, k=16,
family="quad") whose NL rows carry a complete-graph cross term (tests/fuse_quad_cases.py), three ways, alternated round by round.

  a  QUAD rows, fused by nlp.fuse_problems, device loop (FusedBatch)
  b  the same quadratics as expression tapes (quad_cases.quad_as_expr), fused, device loop
  c  hand-fused QUAD batch: one description over all instances' columns + ktn_set_blocks + ktn_optimize_blocks.  Before the device
     loop took QUAD rows this call fell back to the ordinary loop: run `forms=c` on that commit for the "before" figure.

Each line: solve seconds, seconds including load, instances/s including load, the largest objective difference against the
planted optimum.  Building the descriptions is reported once per form (describe_s).
Usage: python tools/batch_quad_bench.py [instances=512] [rounds=3] [forms=abc]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import katana_jl_amd as ktn                                        # noqa: E402
from katana_jl_amd.batch import FusedBatch                          # noqa: E402
import fuse_quad_cases as FQ                                        # noqa: E402
import quad_cases as QC                                             # noqa: E402

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 512
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
forms = sys.argv[3] if len(sys.argv) > 3 else "abc"
insts = [ktn.instances.make_instance(n=1000, m_nl=100, k=16, family="quad", seed=s) for s in range(nb)]


def solver():
    return ktn.KatanaSolver(log_level=0, lp_max_iter=400000)


def hand_fused():
    """(Problem, offsets): every instance's rows with its columns shifted, assembled as ONE description"""
    offs = np.concatenate([[0], np.cumsum([i.n for i in insts])]).astype(np.int64)
    rows, ocol, oval = [], [], []
    for inst, o in zip(insts, offs):
        for r in FQ.quad_rows(inst):
            if r[0] == "sep":
                rows.append(("sep", np.asarray(r[1]) + o) + r[2:])
            else:
                rows.append(("quad", r[1] + o, r[2], r[3] + o, r[4] + o) + r[5:])
        ocol.append(inst.obj_col + o); oval.append(inst.obj_p0)
    d, _ = QC.assemble(int(offs[-1]), rows, ("lin", np.concatenate(ocol), np.concatenate(oval)))
    cat = lambda attr: np.concatenate([getattr(i, attr) for i in insts])
    return ktn.Problem(int(offs[-1]), d.num_constr, cat("l_var"), cat("u_var"), cat("l_constr"), cat("u_constr"), "Min", d), offs


built = {}
for f, make in (("a", lambda: [FQ.quad_rows_problem(i) for i in insts]),
                ("b", lambda: [FQ.quad_rows_problem(i, as_tapes=True) for i in insts]), ("c", hand_fused)):
    if f in forms:
        t0 = time.perf_counter()
        built[f] = make()
        print(json.dumps({"form": f, "instances": nb, "describe_s": time.perf_counter() - t0}), flush=True)


def report(mode, rnd, objs, statuses, stats, solve_s, total_s):
    err = max(abs(v - i.opt_obj) / max(1.0, abs(i.opt_obj)) for v, i in zip(objs, insts))
    line = {"mode": mode, "round": rnd, "instances": nb, "optimal": sum(s == "Optimal" for s in statuses),
            "solve_s": solve_s, "total_s": total_s, "instances_per_s": nb / total_s, "max_obj_relerr": err}
    line.update(stats)
    print(json.dumps(line), flush=True)


def fused(mode, rnd, items):
    t0 = time.perf_counter()
    fb = FusedBatch(solver(), items)
    t1 = time.perf_counter()
    res = fb.solve()
    t2 = time.perf_counter()
    keys = ("ecp_blocks_launches", "ecp_blocks_fallbacks", "ecp_blocks_quad_rows", "ecp_blocks_tape_rows", "ecp_blocks_pdhg_sum")
    report(mode, rnd, [r["objval"] for r in res], [r["status"] for r in res], {k: res[0][k] for k in keys if k in res[0]}, t2 - t1, t2 - t0)


def by_hand(rnd, big, offs):
    t0 = time.perf_counter()
    m = ktn.NonlinearModel(solver())
    m.loadproblem(*big)
    m.set_blocks(offs)
    t1 = time.perf_counter()
    status = m.optimize_blocks()
    x = m.getsolution()
    t2 = time.perf_counter()
    objs = [float(np.sum(i.obj_p0 * x[o:o + i.n][i.obj_col])) for i, o in zip(insts, offs)]
    stats = {k: m.stat(k) for k in ("ecp_blocks_launches", "ecp_blocks_fallbacks", "ecp_blocks_quad_rows")}
    report("c_hand_fused_optimize_blocks", rnd, objs, [status] * nb, stats, t2 - t1, t2 - t0)


for rnd in range(rounds):
    if "a" in built:
        fused("a_quad_rows_device_loop", rnd, built["a"])
    if "b" in built:
        fused("b_quadratics_as_tapes_device_loop", rnd, built["b"])
    if "c" in built:
        by_hand(rnd, *built["c"])
