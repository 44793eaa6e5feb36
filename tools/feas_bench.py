"""One solve of a BASELINE configuration, then the feasible point and the primal bound, timed; the lines go to
profiles/feasible_point.txt (--out) as they are printed.

    python tools/feas_bench.py cfg3 --algo supporting_hyperplane [--reps 5] [--seed 0] [--out profiles/feasible_point.txt]
    python tools/feas_bench.py cfg5 --batch 512                  # per instance of a fused batch: the spread over the instances

The reference point is the engine's own (the auxiliary problem of the supporting-hyperplane modes; own_point_outside_box_by says how
far outside a variable bound it lay before the engine clamped it).  Reported: the getter's first call (buffers allocated,
the taking-part rows found), a later call (after a re-solve of the final LP, which drops the cache) and a cached call in wall time,
f(x_feas) - planted optimum, 1 - lambda*, the certified gap |f(x_feas) - bound| next to getobjgap() = f(x*) - bound, rows
unconverged, back-offs.  Put under `rocprofv3 --kernel-trace --stats` for the kernels' own time (k_feas_*).
KTN_PKG_ROOT=<checkout> imports the package from another (built) checkout."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("KTN_PKG_ROOT") or ROOT)
import katana_jl_amd as ktn   # noqa: E402
from katana_jl_amd.batch import FusedBatch   # noqa: E402


def emit(out, path):
    line = json.dumps(out)
    print(line)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(line + "\n")


def single(a):
    inst = ktn.instances.make_config(a.config, seed=a.seed)
    m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, cut_algo=a.algo))
    m.loadproblem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr, inst.u_constr, inst.sense, ktn.SeparableNLP(inst))
    t0 = time.perf_counter()
    status = m.optimize()
    out = dict(config=a.config, algo=a.algo, status=status, iters=m.numiters(), pdhg_iters=m.stat("pdhg_iters"), objval=m.getobjval(),
               opt_obj=inst.opt_obj, solve_s=time.perf_counter() - t0, n=int(inst.n), m=int(inst.num_constr), feas_evals_after_solve=m.stat("feas_evals"))
    t1 = time.perf_counter()
    fp = m.feasible_point()
    out["first_call_s"] = time.perf_counter() - t1
    xin = m.interior_point()
    if xin is not None:
        out["own_point_outside_box_by"] = float(max(np.max(inst.l_var - xin), np.max(xin - inst.u_var), 0.0))
    walls = []
    for _ in range(a.reps):
        m.lp_solve(1e-7, 1e-7)                                      # same LP, warm: the cache is dropped, x* barely moves
        t1 = time.perf_counter()
        fp = m.feasible_point()
        walls.append(time.perf_counter() - t1)
    t1 = time.perf_counter()
    m.feasible_point()
    out.update(later_call_s=sorted(walls)[len(walls) // 2], cached_call_s=time.perf_counter() - t1, found=fp.found, lam_gap=1.0 - fp.lam,
               f_feas_minus_planted=fp.objval - inst.opt_obj, f_star_minus_planted=m.getobjval() - inst.opt_obj,
               certified_gap=m.getcertifiedgap(), objgap=m.getobjgap(), nl_margin=fp.nl_margin, lin_viol=fp.lin_viol,
               unconverged=fp.unconverged, backoffs=fp.backoffs, feas_evals=m.stat("feas_evals"), feas_passes=m.stat("feas_passes"),
               feas_group=m.stat("feas_group"))
    emit(out, a.out)


def batch(a):
    name = a.config + "_one" if a.config == "cfg5" else a.config          # (cfg5 is the batch; its instances are cfg5_one)
    insts = [ktn.instances.make_config(name, seed=a.seed + k) for k in range(a.batch)]
    fb = FusedBatch(ktn.KatanaSolver(log_level=0, cut_algo=a.algo), insts, False, True)
    t0 = time.perf_counter()
    res = fb.solve()
    out = dict(config=a.config, batch=a.batch, algo=a.algo, status=res[0]["status"], solve_s=time.perf_counter() - t0,
               ecp_blocks_launches=res[0]["ecp_blocks_launches"])
    if fb.m.interior_point() is None:
        out["note"] = "no reference point"
        emit(out, a.out)
        return
    t1 = time.perf_counter()
    fps = fb.feasible_points()
    out["first_call_s"] = time.perf_counter() - t1
    found = np.asarray([f.found for f in fps])
    ok = found == 1
    q = lambda v: [float(np.min(v)), float(np.median(v)), float(np.max(v))] if len(v) else None
    out.update(found_1=int(ok.sum()), found_other=sorted(set(int(f) for f in found[~ok])),
               lam_gap_min_med_max=q(np.asarray([1.0 - f.lam for f in fps])[ok]),
               f_feas_minus_planted_min_med_max=q(np.asarray([f.objval - i.opt_obj for f, i in zip(fps, insts)])[ok]),
               unconverged_max=int(max(f.unconverged for f in fps)), backoffs_max=int(max(f.backoffs for f in fps)))
    emit(out, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--algo", default="supporting_hyperplane")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    (batch if a.batch else single)(a)


if __name__ == "__main__":
    main()
