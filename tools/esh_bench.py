"""Supporting-hyperplane cuts against Kelley's: every case solved both ways, one JSON line per run.

  vertex family   cfg3, cfg3_qp, cfg2 (seed 0)
  off the vertex  make_instance(n, m_nl = n / 10, k = 16) at n = 200 / 500 / 1000, bound_frac 0 and 0.5, explog and quad
  n-ball          the reference's test/misc.jl family, min sum(x) s.t. sum(x^2) <= 1, at n = 128 / 512 (optimum -sqrt(n))
  quad            KTN_ROW_QUAD rows, Kelley against supporting_hyperplane_quad (closed-form boundary point): the ellipsoid
                  min c'x s.t. 1/2 (x - x0)'Q(x - x0) <= 4 at n = 8 / 16 / 40 with the caller's point x0 and with the engine's own
                  (where its auxiliary problem finds one), and one QCQP of 200 rows 1/2 x'Q_i x <= 1 on 16 of 2 000 columns each
                  (the rows of tools/quad_bench.py), interior point 0, against the Kelley run's objective

  batch           throughput mode (only when asked for by name): 512 x make_config("cfg5_one", seed = s) as ONE fused batch in the
                  device-side loop (FusedBatch), Kelley against supporting hyperplanes inside the loop -- once with the engine's own
                  interior point (the auxiliary problem of the fused batch, solved by the host-driven loop) and once with a caller's
                  point (the point the engine found, read back and handed over per instance: what a caller who solves the same
                  constraint sets again would keep).  solve() after a warm-up solve, `reps` times per variant, the variants alternating;
                  per line: solve seconds (median, min, max), seconds to find x_int, per-instance rounds (median, max), PDHG iterations
                  (sum, max), ecp_blocks_fallbacks, the worst objective error against the planted values

Each line: status, ECP rounds, PDHG iterations, solve seconds (or the stated round budget), objective error against the
planted value, and the interior-point and root-search seconds and counts of the supporting-hyperplane run.
Usage: python tools/esh_bench.py [iter_cap=300] [cases=all|vertex|off|ball|quad|batch] [instances=512] [reps=7]"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                 # noqa: E402
import katana_jl_amd as ktn                                        # noqa: E402

iter_cap = int(sys.argv[1]) if len(sys.argv) > 1 else 300
which = sys.argv[2] if len(sys.argv) > 2 else "all"
STATS = ("pdhg_iters", "esh_rows", "esh_fallback_rows", "esh_newton_steps", "esh_root_time_s", "esh_interior_found",
         "esh_interior_rounds", "esh_interior_s", "esh_interior_depth", "esh_interior_time_s", "esh_quad_rows")


def run(name, load, opt, algo, **kw):
    m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, iter_cap=iter_cap, cut_algo=algo, **kw))
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
    return m


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


def ellipsoid_case(n, rho=4.0):
    """tests/quad_cases.ellipsoid with radius rho: f* = c'x0 - sqrt(2 rho c'Q^-1 c)"""
    rng = np.random.default_rng(n)
    Uo, _ = np.linalg.qr(rng.standard_normal((n, n)))
    Q = Uo @ np.diag(np.exp(rng.uniform(0.0, math.log(4.0), n))) @ Uo.T
    Q = (Q + Q.T) / 2
    x0, c = rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)
    fstar = float(c @ x0 - math.sqrt(2.0 * rho * (c @ np.linalg.solve(Q, c))))
    r, cc = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    d = ktn.QuadNLP(n, c, 0.0, None, [(np.arange(n), -(Q @ x0), r.ravel(), cc.ravel(), Q.ravel(), 0.5 * float(x0 @ Q @ x0))])

    def load(point):
        def f(m):
            m.loadproblem(n, 1, np.full(n, -10.0), np.full(n, 10.0), [-math.inf], [rho], "Min", d)
            if point is not None:
                m.set_interior_point(point)
        return f
    run("ellipsoid_%d" % n, load(None), fstar, "kelley")
    run("ellipsoid_%d_centre" % n, load(x0), fstar, "supporting_hyperplane_quad")
    run("ellipsoid_%d_engine" % n, load(None), fstar, "supporting_hyperplane_quad", esh_interior_iters=200)


def qcqp_case(n=2000, m=200, k=16):
    """the rows of tools/quad_bench.py (Q_i = 2 I + random symmetric off-diagonal entries of size 1 / k on k distinct columns),
    min c'x in the +-10 box; x = 0 is 1 inside every row.  No closed form: obj_err is against the Kelley run's objective"""
    rng = np.random.default_rng(1000 + k)
    cols = np.stack([np.sort(rng.choice(n, k, replace=False)) for _ in range(m)])
    R = rng.uniform(-1.0, 1.0, (m, k, k)) / k
    R[:, np.arange(k), np.arange(k)] = 0.0
    Qm = (R + R.transpose(0, 2, 1)) / 2 + 2.0 * np.eye(k)
    c = rng.uniform(-1.0, 1.0, n)
    c[np.setdiff1d(np.arange(n), cols.ravel())] = 0.0               # (columns in no row would only sit at a box bound)
    rows = [(cols[i], np.zeros(k), np.repeat(cols[i], k), np.tile(cols[i], k), Qm[i].ravel(), 0.0) for i in range(m)]
    d = ktn.QuadNLP(n, c, 0.0, None, rows)

    def load(point):
        def f(mm):
            mm.loadproblem(n, m, np.full(n, -10.0), np.full(n, 10.0), np.full(m, -math.inf), np.ones(m), "Min", d)
            if point is not None:
                mm.set_interior_point(point)
        return f
    mk = run("qcqp_%dx%d" % (m, k), load(None), 0.0, "kelley")
    run("qcqp_%dx%d_zero" % (m, k), load(np.zeros(n)), mk.getobjval(), "supporting_hyperplane_quad")


if which in ("all", "quad"):
    for n in (8, 16, 40):
        ellipsoid_case(n)
    qcqp_case()


def batch_case(nb, reps):
    from katana_jl_amd.batch import FusedBatch
    insts = [ktn.instances.make_config("cfg5_one", seed=s) for s in range(nb)]

    def handle(algo, points=None):
        fb = FusedBatch(ktn.KatanaSolver(log_level=0, lp_max_iter=400000, cut_algo=algo), insts)
        if points is not None:
            fb.set_interior_points(points)
        return fb
    variants = [("kelley", handle("kelley"))]
    own = handle("supporting_hyperplane")
    variants.append(("supporting_engine_point", own))
    for _, fb in variants:
        fb.solve()                                                  # warm-up (the engine's own point is found here, once per load)
    xi = own.m.interior_point()
    find_s = own.m.stat("esh_interior_time_s")
    if xi is not None:
        given = handle("supporting_hyperplane", [xi[own.offs[k]:own.offs[k + 1]] for k in range(nb)])
        given.solve()
        variants.append(("supporting_caller_point", given))
    times = {name: [] for name, _ in variants}
    last = {}
    for _ in range(reps):                                           # alternate the variants: other work shares the host
        for name, fb in variants:
            t0 = time.perf_counter()
            res = fb.solve()                                        # (getsolution() inside: ends in a device synchronise)
            times[name].append(time.perf_counter() - t0)
            last[name] = res
    for name, fb in variants:
        res, t = last[name], sorted(times[name])
        rec = fb.m.blocks_results()
        err = max(abs(r["objval"] - i.opt_obj) / max(1.0, abs(i.opt_obj)) for r, i in zip(res, insts))
        line = {"case": "batch_%dx_cfg5_one" % nb, "variant": name, "status": res[0]["status"], "reps": reps,
                "solve_s_median": t[len(t) // 2], "solve_s_min": t[0], "solve_s_max": t[-1],
                "xint_find_s": (find_s if name == "supporting_engine_point" else 0.0),
                "xint_found": (None if name == "kelley" else fb.m.stat("esh_interior_found")),
                "rounds_median": float(np.median(rec[:, 1])), "rounds_max": float(rec[:, 1].max()), "rounds_sum": float(rec[:, 1].sum()),
                "pdhg_sum": float(rec[:, 4].sum()), "pdhg_max": float(rec[:, 4].max()), "lp_rows_max": float(rec[:, 6].max()),
                "ecp_blocks_fallbacks": res[0]["ecp_blocks_fallbacks"], "ecp_blocks_launches": res[0]["ecp_blocks_launches"],
                "ecp_blocks_esh_rows": res[0]["ecp_blocks_esh_rows"], "esh_fallback_rows_cumulative": fb.m.stat("esh_fallback_rows"),
                "obj_err_max": err}
        print(json.dumps(line), flush=True)


if which == "batch":
    batch_case(int(sys.argv[3]) if len(sys.argv) > 3 else 512, int(sys.argv[4]) if len(sys.argv) > 4 else 7)
