"""The sweep over tape rows: the row interpreter (k_tape_eval + k_gj_stats, KTN_TAPE_CLASSED=0) against the shape-class kernel
(k_tape_classed) on the same model and point, in ONE process (the switch is read per handle): results compared bitwise
(g, Jacobian, violated rows, largest violation, the cuts appended), then both timed, alternating, by the events around
the tape launches of the sweep (tape_eval_time_s).  Prints microseconds per sweep (min / median / max over the repetitions),
algorithmic bytes, the fraction of the 8 TB/s HBM peak and load_s for both.
usage: tape_bench.py [family=cone|mixed] [rows=1000000] [reps=8] [--plain]
  cone    rows sqrt(x_a^2 + x_b^2) - (x_c - 0.25) on random distinct columns of 1e5 variables
  mixed   that row, x^2 + y^2 + z - 1 and exp(x) + exp(0.5 y) - z interleaved (row t has shape t % 3)
  --plain one handle under the environment as it is, existing API only (load, precompute, then sweep + reset `reps` times):
          the driver to put under rocprofv3 --kernel-trace --stats, also with an older build through KTN_LIB"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import katana_jl_amd as ktn
import tape_class_cases as T

args = [a for a in sys.argv[1:] if not a.startswith("--")]
plain = "--plain" in sys.argv
family = args[0] if len(args) > 0 else "cone"
m = int(float(args[1])) if len(args) > 1 else 1000000
reps = int(args[2]) if len(args) > 2 else 8
n = 100000
rng = np.random.default_rng(17)
shapes = (T.CONE,) if family == "cone" else (T.CONE, T.QUAD3, T.EXPO)
rows = np.arange(m)
d = T.assemble(n, m, [dict(rows=rows[k::len(shapes)], cols=T.distinct_columns(rng, len(rows[k::len(shapes)]), n), shape=s)
                      for k, s in enumerate(shapes)])
x = T.signed_point(rng, n)
INF = float("inf")


def load(setting):
    if setting is not None:
        os.environ["KTN_TAPE_CLASSED"] = str(setting)
    t0 = time.perf_counter()
    model = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, profile=0 if plain else 1, purge_age=0, cut_cap_factor=0.0))
    model.loadproblem(n, m, np.full(n, -INF), np.full(n, INF), np.full(m, -INF), np.zeros(m), "Min", d)
    load_s = time.perf_counter() - t0
    sep = ktn.KatanaHipSeparator(model); sep.initialize()
    return model, sep, load_s


if plain:
    model, sep, load_s = load(None)
    sep.precompute(x)
    for r in range(reps):
        nv, mv = sep.sweep(1e-6)
        model.reset(); sep.precompute(x)
    print(json.dumps(dict(family=family, rows=m, reps=reps, violated=nv, maxviol=mv, load_s=round(load_s, 3))))
    sys.exit(0)

ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))                      # (device initialisation is not part of load_s)
bits = lambda a: np.ascontiguousarray(a).view(np.uint64) if np.asarray(a).dtype == np.float64 else np.asarray(a)
H = {"interpreter": load(0), "classed": load(-1)}
os.environ.pop("KTN_TAPE_CLASSED", None)
res = {}
for label, (model, sep, load_s) in H.items():
    sep.precompute(x)
    g, jac = sep.g.copy(), sep.jac.copy()
    m0 = model.lp_num_rows()
    nv, mv = sep.sweep(1e-6)
    res[label] = dict(g=g, jac=jac, nv=nv, mv=mv, rows=model.lp_rows_from(m0), us=[])
a, b = res["interpreter"], res["classed"]
same = dict(g=bool(np.array_equal(bits(a["g"]), bits(b["g"]))), jac=bool(np.array_equal(bits(a["jac"]), bits(b["jac"]))),
            violated=a["nv"] == b["nv"], maxviol=bool(np.array_equal(bits(np.array([a["mv"]])), bits(np.array([b["mv"]])))),
            lp_rows=all(bool(np.array_equal(bits(p), bits(q))) for p, q in zip(a["rows"], b["rows"])))
for r in range(reps):                                           # alternating: both see the same drift of the machine
    for label, (model, sep, load_s) in H.items():
        model.reset(); sep.precompute(x)
        t0, n0 = model.stat("tape_eval_time_s"), model.stat("tape_eval_launches")
        sep.sweep(1e-6)
        assert model.stat("tape_eval_launches") - n0 == 1
        res[label]["us"].append(1e6 * (model.stat("tape_eval_time_s") - t0))
out = dict(family=family, rows=m, reps=reps, bitwise_equal=same, violated=a["nv"])
for label, (model, sep, load_s) in H.items():
    us = np.sort(res[label]["us"])
    nbytes = model.stat("tape_eval_bytes") / max(model.stat("tape_eval_launches"), 1.0)
    out[label] = dict(us_min=round(float(us[0]), 1), us_median=round(float(np.median(us)), 1), us_max=round(float(us[-1]), 1),
                      algorithmic_bytes=int(nbytes), hbm_peak_fraction=round(nbytes / (float(np.median(us)) * 1e-6) / 8e12, 4),
                      load_s=round(load_s, 3), classes=int(model.stat("tape_classes")), classed_rows=int(model.stat("tape_classed_rows")),
                      interp_rows=int(model.stat("tape_interp_rows")), class_copy_bytes=int(model.stat("tape_class_dev_bytes")))
out["speedup_median"] = round(out["interpreter"]["us_median"] / out["classed"]["us_median"], 2)
print(json.dumps(out))
sys.exit(0 if all(same.values()) else 1)
