"""Re-solve after a bound change from the kept cut pool against a cold re-load: cfg3 (the bench.py workload's
generator, seed 0) is solved once; then `--children` children follow, each tightening one bound of the parent's solution x* --
child i takes the variable i-th furthest from both of its bounds and sets u_j = x*_j - (x*_j - l_j) / 4 (odd i: the mirrored change
of l_j).  Every child is solved warm (ktn_set_var_bounds + solve on a handle in the parent's state) and cold (ktn_loadproblem with
the child's bounds on a second live handle, plus the solve), alternating warm and cold, `--reps` times after one warm-up; the
figures are medians.  Every warm solve is a FIRST visit of its child: before it, outside the clock, the warm handle is put back
into the parent's state by ktn_loadproblem with the parent's bounds and the parent solve, so its pool holds the parent's cuts and
nothing an earlier repetition or child added (pool_rows_before reports it).  Timing is a host clock around calls
that end in a stream synchronisation.  Reported per child and in total: rounds, PDHG iterations and seconds for both, the spread
(min - max) of the cold runs, and the screen's kernel time at that pool size from device events (stat "screen_kernel_s").

With --rows the children move a CONSTRAINT bound instead (ktn_set_row_bounds; DESIGN.md section 14 "Row bounds"): child i takes the
nonlinear row with the i-th largest multiplier at the parent's solution and loosens its upper bound by 0.25 (odd i: tightens it by
1/64); warm is setconstrbounds + solve, cold the re-load with the child's row bounds + solve.  "rebase_kernel_us" is the time of
k_rebase_cuts on the parent's pool from device events (stat "rebase_kernel_s"), "rebase_rows" the cut rows it moved.

    python tools/resolve_bench.py [--config cfg3] [--children 16] [--reps 7] [--seed 0] [--rows] [--out profiles/resolve_warm.txt]
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


def emit(out, path):
    line = json.dumps(out)
    print(line, flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(line + "\n")


def load(m, inst, l, u, ub=None):
    m.loadproblem(inst.n, inst.num_constr, l, u, inst.l_constr, inst.u_constr if ub is None else ub, inst.sense, ktn.SeparableNLP(inst))


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--children", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rows", action="store_true", help="children move a constraint bound instead of a variable bound")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    inst = ktn.instances.make_config(a.config, seed=a.seed)
    l0, u0 = np.array(inst.l_var, dtype=np.float64), np.array(inst.u_var, dtype=np.float64)
    warm, cold = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0)), ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))
    load(warm, inst, l0, u0)
    st, t_parent = timed(warm.optimize)
    x = warm.getsolution()[:inst.n].copy()
    p0 = warm.stat("pdhg_iters")
    _, t_load = timed(lambda: load(cold, inst, l0, u0))
    emit(dict(config=a.config, seed=a.seed, parent_status=st, parent_rounds=warm.numiters(), parent_pdhg=p0, parent_solve_s=t_parent,
              parent_obj=warm.getobjval(), pool_rows=warm.lp_num_rows(), load_s=t_load, n=int(inst.n), m=int(inst.num_constr)), a.out)
    order = np.argsort(-np.minimum(x - l0, u0 - x))
    ub0 = np.array(inst.u_constr, dtype=np.float64)
    if a.rows:                                              # the nonlinear rows by multiplier, largest first
        d = np.abs(warm.getconstrduals())
        order = inst.m_lin + np.argsort(-d[inst.m_lin:], kind="stable")
    med = lambda v: float(np.median(v))
    tot = dict(warm_s=0.0, cold_s=0.0, warm_rounds=0, cold_rounds=0, warm_pdhg=0.0, cold_pdhg=0.0)
    for i in range(a.children):
        j = int(order[i])
        l, u = l0.copy(), u0.copy()
        ub = ub0.copy()
        if a.rows:
            ub[j] += 0.25 if i % 2 == 0 else -1.0 / 64
        elif i % 2 == 0:
            u[j] = x[j] - 0.25 * (x[j] - l0[j])
        else:
            l[j] = x[j] + 0.25 * (u0[j] - x[j])
        W, C = [], []
        for rep in range(a.reps + 1):                       # (rep 0: the warm-up of both)
            # warm: from the parent's pool and point -- the parent loaded and solved afresh, outside the clock
            load(warm, inst, l0, u0)
            warm.optimize()
            rows_before = warm.lp_num_rows()
            pw = warm.stat("pdhg_iters")
            (sw, tw) = timed(lambda: ((warm.setconstrbounds(None, ub) if a.rows else warm.setvarbounds(l, u)), warm.optimize())[1])
            rec_w = (tw, warm.numiters(), warm.stat("pdhg_iters") - pw, sw, warm.getobjval(), warm.stat("screen_kernel_s"), warm.lp_num_rows(), rows_before,
                     warm.stat("rebase_kernel_s"), warm.stat("rebase_rows"))
            pc = cold.stat("pdhg_iters")
            (sc, tc) = timed(lambda: (load(cold, inst, l, u, ub), cold.optimize())[1])
            rec_c = (tc, cold.numiters(), cold.stat("pdhg_iters") - pc, sc, cold.getobjval())
            if rep:
                W.append(rec_w); C.append(rec_c)
        out = dict(child=i, var=j, side=("loosened" if i % 2 == 0 else "tightened") if a.rows else ("upper" if i % 2 == 0 else "lower"), warm_status=W[0][3], cold_status=C[0][3],
                   warm_s=med([w[0] for w in W]), cold_s=med([c[0] for c in C]), cold_s_min=min(c[0] for c in C), cold_s_max=max(c[0] for c in C),
                   warm_s_min=min(w[0] for w in W), warm_s_max=max(w[0] for w in W),
                   warm_rounds=int(med([w[1] for w in W])), cold_rounds=int(med([c[1] for c in C])),
                   warm_pdhg=med([w[2] for w in W]), cold_pdhg=med([c[2] for c in C]), warm_obj=W[-1][4], cold_obj=C[-1][4],
                   screen_kernel_us=1e6 * med([w[5] for w in W]), pool_rows=int(W[-1][6]), pool_rows_before=int(W[-1][7]))
        if a.rows:
            out.update(row=j, rebase_kernel_us=1e6 * med([w[8] for w in W]), rebase_rows=int(W[-1][9]))
        for k in tot:
            tot[k] += out[k]
        emit(out, a.out)
    emit(dict(total=tot, speedup=tot["cold_s"] / tot["warm_s"] if tot["warm_s"] > 0 else None, children=a.children, reps=a.reps), a.out)


if __name__ == "__main__":
    main()
