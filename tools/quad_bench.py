"""The sweep over KTN_ROW_QUAD rows (k_quad_jac + k_quad_stats) on `rows` dense quadratics  1/2 x'Q_i x <= 1  over k random distinct
columns of 1e5 variables (Q_i = 2 I + random symmetric off-diagonal entries), and the same rows as expression tapes
sum_i x_i (x_i + sum_{j > i} q_ij x_j): 4 k (k + 1) / 2 - 1 nodes -- at k = 8 that is 143 nodes, 294 of the shape-class kernel's 312
LDS cells, so the classed kernel takes the row; from k = 9 on the row interpreter does.
usage: quad_bench.py k [rows=10000] [reps=12] [--tape | --no-tape | --esh]
  default   one QUAD handle and one tape handle of THIS build in one process (profile = 1): g and the Jacobian compared
            (relative, 1e-12), then both timed, alternating, by the events around their launches of the sweep (quad_eval_time_s /
            tape_eval_time_s): us per sweep min / median / max, algorithmic bytes, the fraction of the 8 TB/s HBM peak, load_s
  --no-tape the QUAD handle alone (k = 128: the tape form is 3.3e8 nodes)
  --tape    the tape handle alone, existing API only (load, precompute, then reset + precompute + sweep `reps` times): the driver to
            put under rocprofv3 --kernel-trace --stats.  KTN_PKG_ROOT=<checkout> imports the package from another (built) checkout,
            e.g. the parent commit's, whose description struct differs from this one's
  --esh     the QUAD handle alone with cut_algo = supporting_hyperplane_quad and the interior point 0 (every row violated at x, every
            row moved): precompute + sweep `reps` times, the driver to put under rocprofv3 --kernel-trace --stats for k_esh_quad
            next to k_quad_jac"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("KTN_PKG_ROOT") or ROOT)
import numpy as np
import katana_jl_amd as ktn

L = ktn._lib
args = [a for a in sys.argv[1:] if not a.startswith("--")]
tape_only, quad_only, esh_only = "--tape" in sys.argv, "--no-tape" in sys.argv, "--esh" in sys.argv
k = int(args[0]) if len(args) > 0 else 32
m = int(float(args[1])) if len(args) > 1 else 10000
reps = int(args[2]) if len(args) > 2 else 12
n = 100000
INF = float("inf")
rng = np.random.default_rng(1000 + k)
cols = np.sort(rng.integers(0, n, (m, k)), axis=1)
while True:                                                     # distinct columns per row: redraw the rows with a repeat
    bad = (np.diff(cols, axis=1) == 0).any(axis=1)
    if not bad.any():
        break
    cols[bad] = np.sort(rng.integers(0, n, (int(bad.sum()), k)), axis=1)
R = rng.uniform(-1.0, 1.0, (m, k, k)) / k
R[:, np.arange(k), np.arange(k)] = 0.0
Qm = (R + R.transpose(0, 2, 1)) / 2 + 2.0 * np.eye(k)           # Q_ii = 2: the tape's diagonal products x_i * x_i need no constant
del R
x = rng.uniform(-1.0, 1.0, n)
rowptr = np.arange(m + 1, dtype=np.int64) * k


def quad_desc():
    qcol = np.broadcast_to(cols[:, None, :], (m, k, k)).reshape(-1).astype(np.int32)
    return ktn.NLPDescription(n, rowptr, cols.reshape(-1), np.full(m, L.ROW_QUAD), np.zeros(m), np.zeros(m), None, None, None,
                              obj_linear=True, obj_kind=L.ROW_SEP, obj_col=[0], obj_atom_kind=[0], obj_p0=[1.0], obj_p1=[0.0],
                              quad_ptr=np.arange(m * k + 1, dtype=np.int64) * k, quad_col=qcol, quad_val=Qm.reshape(-1))


def tape_desc():
    ops, vpos, vidx, cpos, ci, cj = [], [], [], [], [], []
    for i in range(k):
        vpos.append(len(ops)); vidx.append(i); ops.append(L.OP_VAR)
        vpos.append(len(ops)); vidx.append(i); ops.append(L.OP_VAR)         # w_ii = Q_ii / 2 = 1
        for j in range(i + 1, k):
            vpos.append(len(ops)); vidx.append(j); ops.append(L.OP_VAR)
            cpos.append(len(ops)); ci.append(i); cj.append(j); ops.append(L.OP_CONST)
            ops.append(L.OP_MUL)
            ops.append(L.OP_ADD)
        ops.append(L.OP_MUL)
        if i > 0:
            ops.append(L.OP_ADD)
    Lr = len(ops)
    targ = np.zeros((m, Lr))
    targ[:, vpos] = cols[:, vidx]
    targ[:, cpos] = Qm[:, ci, cj]
    return ktn.NLPDescription(n, rowptr, cols.reshape(-1), np.full(m, L.ROW_TAPE), np.zeros(m), np.zeros(m), None, None, None,
                              np.arange(m + 1, dtype=np.int64) * Lr, np.tile(np.asarray(ops, dtype=np.int32), m), targ.reshape(-1),
                              obj_linear=True, obj_kind=L.ROW_SEP, obj_col=[0], obj_atom_kind=[0], obj_p0=[1.0], obj_p1=[0.0]), Lr


def load(d, profile, **kw):
    t0 = time.perf_counter()
    model = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, profile=profile, purge_age=0, cut_cap_factor=0.0, **kw))
    model.loadproblem(n, m, np.full(n, -INF), np.full(n, INF), np.full(m, -INF), np.ones(m), "Min", d)
    load_s = time.perf_counter() - t0
    sep = ktn.KatanaHipSeparator(model); sep.initialize()
    return model, sep, load_s


if tape_only:
    d, Lr = tape_desc()
    model, sep, load_s = load(d, 0)
    sep.precompute(x)
    for r in range(reps):
        model.reset(); sep.precompute(x)
        nv, mv = sep.sweep(1e-6)
    print(json.dumps(dict(form="tape", k=k, rows=m, reps=reps, tape_ops_per_row=Lr, violated=nv, maxviol=mv, load_s=round(load_s, 3),
                          classed_rows=int(model.stat("tape_classed_rows")), interp_rows=int(model.stat("tape_interp_rows")))))
    sys.exit(0)

if esh_only:
    model, sep, load_s = load(quad_desc(), 0, cut_algo="supporting_hyperplane_quad")
    model.set_interior_point(np.zeros(n))
    for r in range(reps):
        model.reset(); sep.precompute(x)
        nv, mv = sep.sweep(1e-6)
    print(json.dumps(dict(form="quad, supporting hyperplanes", k=k, rows=m, reps=reps, violated=nv, load_s=round(load_s, 3),
                          esh_quad_rows=int(model.stat("esh_quad_rows")), esh_fallback_rows=int(model.stat("esh_fallback_rows")))))
    sys.exit(0)

ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))                      # (device initialisation is not part of load_s)
H = {"quad": load(quad_desc(), 1)}
if not quad_only:
    H["tape"] = load(tape_desc()[0], 1)
res = {}
for label, (model, sep, load_s) in H.items():
    sep.precompute(x)
    res[label] = dict(g=sep.g.copy(), jac=sep.jac.copy(), nv=sep.sweep(1e-6)[0], us=[])
out = dict(k=k, rows=m, reps=reps, violated=res["quad"]["nv"], quad_group=int(H["quad"][0].stat("quad_group")),
           quad_nnz=int(H["quad"][0].stat("quad_nnz")))
if "tape" in res:
    a, b = res["quad"], res["tape"]
    out["agree"] = dict(g=float(np.max(np.abs(a["g"] - b["g"]) / (1.0 + np.abs(b["g"])))), jac=float(np.max(np.abs(a["jac"] - b["jac"]))),
                        violated=a["nv"] == b["nv"])
for r in range(reps):                                           # alternating: both see the same drift of the machine
    for label, (model, sep, load_s) in H.items():
        key = label + "_eval"
        model.reset(); sep.precompute(x)
        t0, n0 = model.stat(key + "_time_s"), model.stat(key + "_launches")
        sep.sweep(1e-6)
        assert model.stat(key + "_launches") - n0 == 1
        res[label]["us"].append(1e6 * (model.stat(key + "_time_s") - t0))
for label, (model, sep, load_s) in H.items():
    us = np.sort(res[label]["us"])
    nbytes = model.stat(label + "_eval_bytes") / max(model.stat(label + "_eval_launches"), 1.0)
    out[label] = dict(us_min=round(float(us[0]), 1), us_median=round(float(np.median(us)), 1), us_max=round(float(us[-1]), 1),
                      algorithmic_bytes=int(nbytes), hbm_peak_fraction=round(nbytes / (float(np.median(us)) * 1e-6) / 8e12, 4),
                      load_s=round(load_s, 3))
if "tape" in res:
    out["tape"].update(classed_rows=int(H["tape"][0].stat("tape_classed_rows")), interp_rows=int(H["tape"][0].stat("tape_interp_rows")))
    out["speedup_median"] = round(out["tape"]["us_median"] / out["quad"]["us_median"], 2)
    ok = out["agree"]["g"] <= 1e-12 and out["agree"]["jac"] <= 1e-12 * k and out["agree"]["violated"]
else:
    ok = True
print(json.dumps(out))
sys.exit(0 if ok else 1)
