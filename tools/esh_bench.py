"""Supporting-hyperplane cuts against Kelley's: every case solved both ways, one JSON line per run.

  vertex family   cfg3, cfg3_qp, cfg2 (seed 0)
  off the vertex  make_instance(n, m_nl = n / 10, k = 16) at n = 200 / 500 / 1000, bound_frac 0 and 0.5, explog and quad
  n-ball          the reference's test/misc.jl family, min sum(x) s.t. sum(x^2) <= 1, at n = 128 / 512 (optimum -sqrt(n))

Each line: status, ECP rounds, PDHG iterations, solve seconds (or the stated round budget), objective error against the
planted value, and the interior-point and root-search seconds and counts of the supporting-hyperplane run.
Usage: python tools/esh_bench.py [iter_cap=300] [cases=all|vertex|off|ball]"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import katana_jl_amd as ktn                                        # noqa: E402

iter_cap = int(sys.argv[1]) if len(sys.argv) > 1 else 300
which = sys.argv[2] if len(sys.argv) > 2 else "all"
STATS = ("pdhg_iters", "esh_rows", "esh_fallback_rows", "esh_newton_steps", "esh_root_time_s", "esh_interior_found",
         "esh_interior_rounds", "esh_interior_s", "esh_interior_depth", "esh_interior_time_s")


def run(name, load, opt, algo):
    m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, iter_cap=iter_cap, cut_algo=algo))
    load(m)
    t0 = time.perf_counter()
    st = m.optimize()
    t = time.perf_counter() - t0
    line = {"case": name, "cut_algo": algo, "status": st, "rounds": m.numiters(), "solve_s": t, "iter_cap": iter_cap,
            "obj_err": abs(m.getobjval() - opt) / max(1.0, abs(opt))}
    for k in STATS:
        v = m.stat(k)
        line[k] = v if v == v else None
    print(json.dumps(line), flush=True)


def instance_case(name, inst):
    def load(m):
        m.loadproblem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr, inst.u_constr, inst.sense,
                      ktn.SeparableNLP(inst))
    for algo in ("kelley", "supporting_hyperplane"):
        run(name, load, inst.opt_obj, algo)


def ball_case(n):
    def load(m):
        M = ktn.Model(solver=m.solver)
        xs = [M.variable(-1.0, 1.0) for _ in range(n)]
        obj = xs[0]
        for x in xs[1:]:
            obj = obj + x
        sq = xs[0] ** 2
        for x in xs[1:]:
            sq = sq + x ** 2
        M.objective("Min", obj, linear=True)
        M.constraint((sq, -math.inf, 1.0), linear=False)
        p = M.problem()
        m.loadproblem(p.num_var, p.num_constr, p.l_var, p.u_var, p.l_constr, p.u_constr, p.sense, p.d)
    for algo in ("kelley", "supporting_hyperplane"):
        run("nball_%d" % n, load, -math.sqrt(n), algo)


if which in ("all", "vertex"):
    for cfg in ("cfg3", "cfg3_qp", "cfg2"):
        instance_case(cfg, ktn.instances.make_config(cfg, seed=0))
if which in ("all", "off"):
    for n in (200, 500, 1000):
        for bf in (0.0, 0.5):
            for fam in ("explog", "quad"):
                instance_case("off_%s_n%d_bf%g" % (fam, n, bf),
                              ktn.instances.make_instance(n=n, m_nl=n // 10, k=16, family=fam, seed=0, bound_frac=bf))
if which in ("all", "ball"):
    for n in (128, 512):
        ball_case(n)
