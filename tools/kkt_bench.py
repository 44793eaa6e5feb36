"""One solve of a BASELINE configuration, then -- with --getters -- the NLP-level report (constraint duals, reduced costs, dual
bound), timed.  Meant to be put under `rocprofv3 --kernel-trace --stats`: without --getters the trace must
show no k_row_duals / k_lagr_grad / k_dual_terms / k_dual_bound / k_dual_final launch; with it their durations go next to the byte
model of DESIGN.md section 4.

    python tools/kkt_bench.py cfg3 [--getters] [--reps 5] [--seed 0]

KTN_PKG_ROOT=<checkout> imports the package from another (built) checkout."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("KTN_PKG_ROOT") or ROOT)
import katana_jl_amd as ktn   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--getters", action="store_true")
    ap.add_argument("--reps", type=int, default=5, help="evaluations of the report (each after a re-solve of the final LP, which drops the cache)")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    inst = ktn.instances.make_config(a.config, seed=a.seed)
    m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))
    m.loadproblem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr, inst.u_constr, inst.sense, ktn.SeparableNLP(inst))
    t0 = time.perf_counter()
    status = m.optimize()
    out = dict(config=a.config, status=status, iters=m.numiters(), numcuts=m.numcuts(), objval=m.getobjval(), opt_obj=inst.opt_obj,
               pdhg_iters=m.stat("pdhg_iters"), solve_s=time.perf_counter() - t0, nnz=int(len(inst.col) + len(inst.obj_col)), n=int(inst.n),
               m=int(inst.num_constr))
    if a.getters:
        walls = []
        for r in range(a.reps):
            if r:
                m.lp_solve(1e-7, 1e-7)                              # same LP, warm: the cache is dropped, the multipliers barely move
            t1 = time.perf_counter()
            d, z, lb, gap = m.getconstrduals(), m.getreducedcosts(), m.getobjbound(), m.getobjgap()
            walls.append(time.perf_counter() - t1)
        out.update(bound=lb, gap=gap, kkt_evals=m.stat("kkt_evals"), kkt_group=m.stat("kkt_group"), kkt_mirror_bytes=m.stat("kkt_mirror_bytes"),
                   getters_first_s=walls[0], getters_later_s=sorted(walls[1:])[len(walls[1:]) // 2] if len(walls) > 1 else None,
                   d_nonzero=int((d != 0).sum()), z_nonzero=int((z != 0).sum()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
