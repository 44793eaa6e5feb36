"""Everything the separator side computes, dumped bit for bit -- the tool for comparing two builds of the library.

    KTN_LIB=/path/to/libkatana_hip.so python tests/tools/sweep_bits.py dump OUT.npz
    python tests/tools/sweep_bits.py compare A.npz B.npz          # one line per array; exit status 1 on any difference

`dump` loads the models the GPU tests already build (tests/sep_cases.py, tape_class_cases.py, quad_cases.py, esh_quad_cases.py,
the fused batches of sep_cases.py and fuse_quad_cases.py) at the tests' own sizes and runs, per model, precompute!,
gencut of every row, one sweep and the cut emission -- or, for the fused batches, the device-side loop -- under the switches that
select each kernel form.  Every output a caller can see goes into the .npz: g, the Jacobian, the cut constants, the violated slots,
maxviol, the status (a non-finite coefficient in a violated row: Error), the appended LP rows (columns, values, bounds), lambda and
the supporting-hyperplane counters, the per-instance results of a batch; and the load statistics that say which form ran.  Per
model, before its first sweep, also the LP as loadproblem left it: its rows from 0 with their bounds, the cost vector and c0.
One process per build (KTN_LIB is read at import); `compare` needs no GPU."""
import contextlib
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

GENCUT_ROWS = 3000        # gencut is one call per row: models with more rows take an evenly spaced sample of this many


@contextlib.contextmanager
def env(**kw):
    """the engine reads its development switches per handle, at ktn_create"""
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def get_g_jac(ktn, model, sep):
    L = ktn._lib
    g, jac = np.zeros(max(sep.num_constr, 1)), np.zeros(max(sep.nnz, 1))
    L.check(model._h, model._lib.ktn_sep_get_g(model._h, g.ctypes.data_as(L.P(L.c_f64)), sep.num_constr))
    L.check(model._h, model._lib.ktn_sep_get_jac(model._h, jac.ctypes.data_as(L.P(L.c_f64)), sep.nnz))
    return g[:sep.num_constr], jac[:sep.nnz]


def lp_as_loaded(ktn, out, name, model):
    """the LP of a freshly loaded model: the linear rows, the epigraph cut at the box vertex if there is one, cost and c0"""
    L = ktn._lib
    for k, a in zip(("rowptr", "col", "val", "lo", "hi"), model.lp_rows_from(0)):
        out[name + "/load_lp_" + k] = np.array(a)
    c, c0 = np.zeros(model.num_var + 1), ctypes.c_double(0.0)        # (one more than num_var: the epigraph variable, when there is one)
    L.check(model._h, model._lib.ktn_lp_get_objective(model._h, c.ctypes.data_as(L.P(L.c_f64)), len(c), ctypes.byref(c0)))
    out[name + "/load_lp_c_c0"] = np.concatenate([c, [c0.value]])


def precompute_and_sweep(ktn, out, name, model, x, f_tol, stats=()):
    """the LP as loaded; precompute! at x, gencut, one sweep with its emission: all of it into out[name/...]"""
    lp_as_loaded(ktn, out, name, model)
    sep = ktn.KatanaHipSeparator(model)
    sep.initialize()
    sep.precompute(x)
    out[name + "/g"], out[name + "/jac"] = sep.g.copy(), sep.jac.copy()
    m = sep.num_constr
    rows = np.arange(m) if m <= GENCUT_ROWS else np.unique(np.linspace(0, m - 1, GENCUT_ROWS).astype(np.int64))
    cuts = [sep.gencut(x, None, int(i)) for i in rows]
    out[name + "/gencut_const"] = np.array([c[2] for c in cuts])
    out[name + "/gencut_coefs"] = np.concatenate([c[1] for c in cuts]) if cuts else np.zeros(0)
    m0 = model.lp_num_rows()
    nv, mv = sep.sweep(f_tol)
    out[name + "/nviol_maxviol"] = np.array([float(nv), mv])
    out[name + "/status"] = np.array([model.status()])
    for k, a in zip(("rowptr", "col", "val", "lo", "hi"), model.lp_rows_from(m0)):
        out[name + "/lp_" + k] = np.array(a)
    out[name + "/slots"] = model.last_sweep_slots()
    out[name + "/lam"] = model.last_sweep_lambdas()
    out[name + "/g_after_sweep"], out[name + "/jac_after_sweep"] = get_g_jac(ktn, model, sep)
    out[name + "/stats"] = np.array([model.stat(s) for s in stats])
    return sep


SEP_STATS = ("sweep_group", "sweep_rows_per_group", "sweep_blocked", "sweep_batched", "precompute_multirow", "sep_long_rows")
ESH_STATS = ("esh_rows", "esh_fallback_rows", "esh_newton_steps", "esh_quad_rows", "esh_participating_rows", "sep_long_rows")


def separable_cases(ktn, out):
    import sep_cases as sc
    todo = []
    for G in (8, 16, 32, 64):
        for R in (1, 2, 4):
            todo.append(("row_G%d_R%d" % (G, R), dict(KTN_SWEEP_ROWS=R, KTN_SWEEP_BATCHED=0),
                         lambda e, G=G, R=R: sc.row_kernel_case(G, 1 + (R + G // 8) % 3, e)))
    todo.append(("long", {}, lambda e: sc.long_case(e)))
    for cfg, n in ((None, 20000), (1, 24577), (2, 40000)):
        todo.append(("blocked_cfg%s_n%d" % (cfg, n), dict(KTN_BLK_CFG=cfg), lambda e, cfg=cfg, n=n: sc.blocked_case(n, 16384 if cfg == 2 else 8192, e)))
    for m_nl, n in ((2047, 8192), (2049, 8193), (5000, 30000)):
        todo.append(("batch_m%d_n%d" % (m_nl, n), dict(KTN_SWEEP_BATCHED=1), lambda e, m_nl=m_nl, n=n: sc.batch_case(m_nl, n, e)))
    for name, switches, make in todo:
        for edges in (0, 1, 2):
            C = make(edges)
            with env(**switches):
                model = sc.load(ktn, C)
            precompute_and_sweep(ktn, out, "%s_e%d" % (name, edges), model, C.x, C.f_tol, SEP_STATS)
        print(name, flush=True)
    # precompute! four rows per lane group (k_sep_sweep<8, 4, true>): the size depends on the device's CU count
    cus = int(subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                             check=True, capture_output=True, text=True, timeout=300).stdout.split()[-1])
    C = sc.mat_case(cus)
    with env(KTN_SWEEP_BATCHED=0):
        model = sc.load(ktn, C)
    precompute_and_sweep(ktn, out, "mat_e2", model, C.x, C.f_tol, SEP_STATS)


def tape_cases(ktn, out):
    import tape_class_cases as T
    INF = float("inf")
    stats = ("tape_classes", "tape_classed_rows", "tape_interp_rows")

    def run(name, setting, d, n, m, x):
        with env(KTN_TAPE_CLASSED=setting):
            model = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))
            model.loadproblem(n, m, np.full(n, -INF), np.full(n, INF), np.full(m, -INF), np.zeros(m), "Min", d)
        precompute_and_sweep(ktn, out, name, model, x, 1e-6, stats)
    # classes of 1, 2, 63, 64, 65 and 128 rows: classed and interpreted rows in one model (test_gpu_tape_classes.py, d.)
    rng = np.random.default_rng(31)
    sizes = [1, 2, 63, 64, 65, 128]
    shapes = [T.Shape("pow%d" % p, 2, (lambda p: lambda v: v[0] ** float(p) + v[1] - 1.0)(p), None) for p in range(3, 9)]
    m = sum(sizes)
    n = 2 * m
    shape_of = rng.permutation(np.repeat(np.arange(6), sizes))
    cols = np.arange(n).reshape(m, 2)
    d = T.assemble(n, m, [dict(rows=np.flatnonzero(shape_of == k), cols=cols[shape_of == k], shape=shapes[k]) for k in range(6)])
    x = rng.uniform(0.5, 1.5, n)
    for setting in (0, -1, 1):
        run("tape_thresholds_s%d" % setting, setting, d, n, m, x)
    # every opcode and its edges (NaN and infinite values and partials), each row a class of 64 + 7 (c.)
    R = T.Rows()
    for _ in range(64 + 7):
        T.edge_rows(R)
    x = np.asarray(R.x)
    for setting in (0, -1):
        run("tape_edges_s%d" % setting, setting, R.desc(), len(x), len(R.rows), x)


def quad_cases(ktn, out):
    import quad_cases as QC
    import quad_ref as Q
    C = QC.mixed_case()
    for G in (0, 4, 64):
        with env(KTN_QUAD_GROUP=G or None):
            model = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, f_tol=Q.F_TOL))
            model.loadproblem(C.n, C.m, np.full(C.n, -2.0), np.full(C.n, 2.0), C.lb, C.ub, "Min", C.d)
        precompute_and_sweep(ktn, out, "quad_mixed_G%d" % G, model, C.xt, C.f_tol, ("quad_rows", "quad_group"))


def long_convex_case():
    """three convex separable rows beyond 8 192 entries (k_esh_long) and three short ones: QUAD, EXP and NEGLOG atoms with positive
    weights, LIN atoms of either sign, x_int near the origin, x* in the box; a row whose value grows by at least 1 from x_int to x*
    gets its bound in the middle (it takes part in the root search), the others are satisfied"""
    rng = np.random.default_rng(41)
    n = 12000
    lens = [8193, 40, 9000, 9217, 7, 64]
    xi, xs = rng.uniform(-0.1, 0.1, n), rng.uniform(-1.0, 1.0, n)
    col = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in lens]).astype(np.int32)
    kind = rng.integers(0, 4, len(col)).astype(np.uint8)
    p0 = rng.uniform(0.5, 2.0, len(col)) * np.where(kind == 0, rng.choice([-1.0, 1.0], len(col)), 1.0)
    p1 = np.where(kind == 1, rng.uniform(-0.5, 0.5, len(col)), np.where(kind == 2, rng.uniform(-1.0, 1.0, len(col)), 3.0))
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return n, rowptr, col, kind, p0, p1, xi, xs


def supporting_hyperplane_cases(ktn, out):
    import esh_quad_cases as EC
    from katana_jl_amd.instances import atom_value_deriv
    INF = float("inf")
    # separable, tape and QUAD rows, taking part and falling back (test_gpu_esh_quad_rows.py)
    C = EC.case()
    for algo in ("supporting_hyperplane", "supporting_hyperplane_quad"):
        model = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, f_tol=C.f_tol, cut_algo=algo))
        model.loadproblem(C.n, C.m, np.full(C.n, -2.0), np.full(C.n, 2.0), C.lb, C.ub, "Min", C.d)
        model.set_interior_point(C.xi)
        precompute_and_sweep(ktn, out, "esh_case_" + algo, model, C.xt, C.f_tol, ESH_STATS)
    # long separable rows
    n, rowptr, col, kind, p0, p1, xi, xs = long_convex_case()
    m = len(rowptr) - 1
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    g = [np.bincount(rows, weights=atom_value_deriv(kind, p0, p1, x[col])[0], minlength=m) for x in (xi, xs)]
    ub = np.where(g[1] - g[0] >= 1.0, 0.5 * (g[0] + g[1]), np.maximum(g[0], g[1]) + 0.5)
    assert np.sum(g[1] - g[0] >= 1.0) >= 3
    d = ktn.NLPDescription(n, rowptr, col, np.zeros(m, dtype=np.uint8), np.zeros(m, dtype=np.uint8), np.zeros(m), kind, p0, p1)
    model = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, f_tol=1e-6, cut_algo="supporting_hyperplane"))
    model.loadproblem(n, m, np.full(n, -1.0), np.full(n, 1.0), np.full(m, -INF), ub, "Min", d)
    model.set_interior_point(xi)
    precompute_and_sweep(ktn, out, "esh_long", model, xs, 1e-6, ESH_STATS)
    # a first round through the whole step (LP solve, interior point found by the engine, sweep, root search, emission)
    inst = ktn.instances.make_instance(n=4000, m_nl=400, k=32, family="explog", seed=0)
    model = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, cut_algo="supporting_hyperplane"))
    model.loadproblem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr, inst.u_constr, inst.sense, ktn.SeparableNLP(inst))
    name = "esh_first_round"
    lp_as_loaded(ktn, out, name, model)
    model.optimize_begin()
    m0 = model.lp_num_rows()
    model.ecp_step()
    out[name + "/x"] = model.getsolution()
    for k, a in zip(("rowptr", "col", "val", "lo", "hi"), model.lp_rows_from(m0)):
        out[name + "/lp_" + k] = np.array(a)
    out[name + "/slots"], out[name + "/lam"] = model.last_sweep_slots(), model.last_sweep_lambdas()
    out[name + "/stats"] = np.array([model.stat(s) for s in ESH_STATS])


def batch_cases(ktn, out):
    """the device-side loop (ktn_optimize_blocks): 16 convex mixed-atom separable models; 32 blocks of four cones, each with a
    tape row, a QUAD row and a linear row"""
    import sep_cases as sc
    from sep_ref import F_TOL
    from katana_jl_amd.batch import FusedBatch
    from fuse_quad_cases import cone_problem
    batches = [("batch_sep", [sc.convex_instance(900 + s) for s in range(16)],
                ktn.KatanaSolver(log_level=0, f_tol=F_TOL, lp_max_iter=400000, iter_cap=400), 128),
               ("batch_sep_nonfinite", [sc.convex_instance(900 + s, bad=(s == 5)) for s in range(16)],
                ktn.KatanaSolver(log_level=0, f_tol=F_TOL, lp_max_iter=400000, iter_cap=400), 128)]
    rng = np.random.default_rng(11)
    batches.append(("batch_cones", [cone_problem(rng, cones=4)[0] for _ in range(32)], ktn.KatanaSolver(log_level=0, lp_max_iter=400000), 48))
    for name, items, solver, cap in batches:
        res = FusedBatch(solver, items).solve(cut_capacity=cap)
        out[name + "/x"] = np.concatenate([r["x"] for r in res])
        out[name + "/objval"] = np.array([r["objval"] for r in res])
        out[name + "/status"] = np.array([r["status"] for r in res])
        keys = ("iters", "pdhg_iters", "ecp_blocks_launches", "ecp_blocks_fallbacks", "ecp_blocks_pdhg_sum")
        out[name + "/counters"] = np.array([float(res[0][k]) for k in keys])


def dump(path):
    import katana_jl_amd as ktn
    out = {}
    for part in (separable_cases, tape_cases, quad_cases, supporting_hyperplane_cases, batch_cases):
        part(ktn, out)
        print("%s: %d arrays so far" % (part.__name__, len(out)), flush=True)
    np.savez(path, **out)
    print("library %s: %d arrays -> %s" % (ktn._lib.LIB_PATH, len(out), path))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    names = sorted(set(a.files) | set(b.files))
    bad = 0
    for k in names:
        if k not in a.files or k not in b.files:
            verdict = "MISSING in " + (pa if k not in a.files else pb)
        else:
            u, v = a[k], b[k]
            if u.dtype == np.float64 and v.dtype == np.float64 and u.shape == v.shape:      # bit patterns: NaN payloads and signed zeros count
                same = np.array_equal(u.view(np.uint64), v.view(np.uint64))
            else:
                same = u.shape == v.shape and np.array_equal(u, v)
            verdict = "identical" if same else "DIFFERENT"
            if same and u.dtype == np.float64:
                assert np.array_equal(u, v, equal_nan=True)
        bad += verdict != "identical"
        shape = a[k].shape if k in a.files else b[k].shape
        nan = int(np.isnan(a[k]).sum()) if k in a.files and a[k].dtype == np.float64 else 0
        small = "  " + " ".join(str(v) for v in a[k].tolist()) if k in a.files and 0 < a[k].size <= 6 else ""       # statistics, counters, status
        print("%-52s %-10s %-12s nan=%-6d %s%s" % (k, a[k].dtype if k in a.files else "-", "x".join(map(str, shape)), nan, verdict, small))
    print("%d arrays, %d not identical" % (len(names), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
