"""Warm against cold re-solves of a resident batch in the device-side loop (KTN_BLOCKS_WARM; DESIGN.md section 14 "In the
device-side loop"): 512 x cfg5 loaded once and solved once, then three kinds of change, each solved WARM (from every instance's
own cuts, multipliers and x) and COLD (solve() on the same handle: ktn_reset and the loaded rows) --
  (i)   unchanged data;
  (ii)  every instance's box cut down by one bound that removes its optimum (the child of a branching step): the upper bound of
        its most interior variable a quarter of the way below the optimum;
  (iii) every instance's costs scaled by 1.25;
  (iv)  row bounds (FusedBatch.set_row_bounds; DESIGN.md section 14 "Row bounds"): the upper bound of every nonlinear row loosened
        by 0.25 in the even instances and tightened by 1/64 in the odd ones; the line below the table gives the time of
        k_blocks_rebase from device events and the cut rows it moved.
Median of REPS timed solves after one warm-up.  Every timed warm solve starts from the same state: the arenas of a cold solve
of the loaded data.  Writes profiles/blocks_warm.txt (or argv[2]); no speed-up is promised, the figure to compare a warm
solve against is the cold solve of the same handle in the same run.

    python tools/blocks_warm_bench.py [instances = 512] [out = profiles/blocks_warm.txt] [cases = all, or a comma list of their names]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import katana_jl_amd as ktn
from katana_jl_amd.batch import FusedBatch

REPS = 7
nb = int(sys.argv[1]) if len(sys.argv) > 1 else 512
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "blocks_warm.txt")
insts = [ktn.instances.make_config("cfg5_one", seed=s) for s in range(nb)]
# (lp_max_iter: the device loop has no exit for an infeasible LP that no row proves; an instance the cut bound empties runs
#  LP after LP to that many iterations until it ends :UserLimit or overflows, warm and cold alike -- at 1e5 that is tens of
#  seconds per solve.  A cold cfg5 instance needs about 5e3 iterations in all.)
fb = FusedBatch(ktn.KatanaSolver(log_level=0, lp_max_iter=20000), insts)
m = fb.m
base = fb.solve(fallback=False)
assert all(r["status"] == "Optimal" for r in base)
l0, u0 = [np.array(i.l_var, dtype=np.float64) for i in insts], [np.array(i.u_var, dtype=np.float64) for i in insts]


def cost(inst, f):
    c = np.zeros(inst.n)
    c[np.asarray(inst.obj_col)] = f * np.asarray(inst.obj_p0)
    return c


def branched():
    us = []
    for inst, r, l, u in zip(insts, base, l0, u0):
        x = np.asarray(r["x"])
        j = int(np.argmax(np.minimum(x - l, u - x)))
        u = u.copy()
        u[j] = x[j] - 0.25 * (x[j] - l[j])
        us.append(u)
    return us


ub0 = [np.array(i.u_constr, dtype=np.float64) for i in insts]


def moved_rows():
    out = []
    for k, (inst, u) in enumerate(zip(insts, ub0)):
        u = u.copy()
        u[inst.m_lin:] += 0.25 if k % 2 == 0 else -1.0 / 64
        out.append(u)
    return out


CASES = [("unchanged", lambda: None),
         ("one bound", lambda: fb.set_var_bounds(l0, branched())),
         ("costs x 1.25", lambda: fb.set_costs([cost(i, 1.25) for i in insts])),
         ("row bounds", lambda: fb.set_row_bounds(None, moved_rows()))]
if len(sys.argv) > 3 and sys.argv[3] != "all":
    CASES = [c for c in CASES if c[0] in sys.argv[3].split(",")]


def restore():
    fb.set_var_bounds(l0, u0)
    fb.set_costs([cost(i, 1.0) for i in insts])
    fb.set_row_bounds(None, ub0)


def timed(**kw):
    pd0 = m.stat("ecp_blocks_pdhg_sum")
    t0 = time.perf_counter()
    res = fb.solve(fallback=False, **kw)
    dt = time.perf_counter() - t0
    rec = m.blocks_results()
    return dict(t=dt, rounds=rec[:, 1].copy(), pdhg=m.stat("ecp_blocks_pdhg_sum") - pd0, optimal=int(np.sum(rec[:, 0] == 1)),
                overflow=int(np.sum(rec[:, 7])), obj=np.array([r["objval"] for r in res]), rows=float(rec[:, 6].sum()))


lines = ["%d x cfg5, device-side loop, default cut capacity; median of %d after a warm-up; times in ms" % (nb, REPS),
         "%-13s %-5s %8s %7s %7s %11s %8s %9s %9s %10s %9s" % ("change", "start", "solve", "rounds", "rounds", "PDHG iter.", "optimal", "rows", "rows", "rewarm", "max |obj"),
         "%-13s %-5s %8s %7s %7s %11s %8s %9s %9s %10s %9s" % ("", "", "ms", "median", "max", "sum", "", "at end", "dropped", "kernel us", "diff| rel")]
for name, apply in CASES:
    warm, cold = [], []
    for rep in range(REPS + 1):
        restore()
        fb.solve(fallback=False)                              # the state every warm solve starts from
        apply()
        rebase = (m.stat("rebase_kernel_s"), m.stat("rebase_rows")) if name == "row bounds" else None
        w = timed(warm=True)
        w["rebase"] = rebase
        w["dropped"], w["kernel"] = m.stat("ecp_blocks_warm_dropped_rows"), m.stat("ecp_blocks_rewarm_kernel_s")
        w["states"] = (m.stat("ecp_blocks_warm_instances"), m.stat("ecp_blocks_warm_cold_instances"), m.stat("ecp_blocks_warm_infeasible"))
        c = timed()
        print("%s rep %d: warm %.3f s, cold %.3f s" % (name, rep, w["t"], c["t"]), flush=True)
        if rep:                                               # (rep 0: warm-up)
            warm.append(w); cold.append(c)
    both = (warm[-1]["rounds"] > 0) & (cold[-1]["rounds"] > 0)
    diff = float(np.max(np.abs(warm[-1]["obj"] - cold[-1]["obj"])[both] / np.maximum(1.0, np.abs(cold[-1]["obj"][both]))))
    for tag, runs in (("warm", warm), ("cold", cold)):
        r = runs[-1]
        lines.append("%-13s %-5s %8.2f %7.0f %7.0f %11.0f %4d/%-3d %9.0f %9s %10s %9s" % (
            name, tag, 1e3 * statistics.median(x["t"] for x in runs), np.median(r["rounds"]), np.max(r["rounds"]),
            statistics.median(x["pdhg"] for x in runs), r["optimal"], nb, r["rows"],
            "%.0f" % r["dropped"] if tag == "warm" else "-", "%.1f" % (1e6 * statistics.median(x["kernel"] for x in runs)) if tag == "warm" else "-",
            "%.1e" % diff if tag == "warm" else "-"))
    lines.append("%-13s       states of the warm launch (warm / cold / infeasible): %d / %d / %d; overflows warm %d cold %d" % (
        (name,) + tuple(int(v) for v in warm[-1]["states"]) + (warm[-1]["overflow"], cold[-1]["overflow"])))
    if name == "row bounds":
        lines.append("%-13s       k_blocks_rebase: median %.1f us (min %.1f, max %.1f), %d cut rows moved" % (
            name, 1e6 * statistics.median(x["rebase"][0] for x in warm), 1e6 * min(x["rebase"][0] for x in warm),
            1e6 * max(x["rebase"][0] for x in warm), int(warm[-1]["rebase"][1])))
text = "\n".join(lines)
print(text)
with open(out_path, "w") as f:
    f.write(text + "\n")
