"""Test helpers shared by the CPU and GPU tiers."""
import numpy as np

from oracle.evaluators import SeparableNLPEvaluator, SexprNLPEvaluator
from oracle.katana import KatanaModelParams, KatanaNonlinearModel as OracleModel


def oracle_evaluator(inst):
    return SeparableNLPEvaluator(inst.n, inst.rowptr, inst.col, inst.kind, inst.p0, inst.p1, inst.rconst,
                                 inst.obj_col, inst.obj_kind, inst.obj_p0, inst.obj_p1, inst.obj_const)


def oracle_solve_instance(inst, fast=True, **params):
    d = oracle_evaluator(inst)
    om = OracleModel(KatanaModelParams(**params), fast=fast)
    om.loadproblem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr, inst.u_constr, inst.sense, d)
    om.optimize()
    return om


def oracle_solve_kat(m, **kw):
    n = len(m["vars"])
    d = SexprNLPEvaluator(n, m["objective"], [c["expr"] for c in m["constraints"]],
                          [c["linear"] for c in m["constraints"]], m["objective_linear"])
    om = OracleModel(KatanaModelParams(), **kw)
    om.loadproblem(n, len(m["constraints"]), [v["lb"] for v in m["vars"]], [v["ub"] for v in m["vars"]],
                   [c["lb"] for c in m["constraints"]], [c["ub"] for c in m["constraints"]], m["sense"], d)
    om.optimize()
    return om


def hip_model_from_kat(ktn, m, **solver_kw):
    import json, os
    solver_kw = dict(json.loads(os.environ.get("KTN_TEST_OPTS", "{}")), **solver_kw)      # experiments: override solver defaults
    M = ktn.Model(solver=ktn.KatanaSolver(**dict(dict(log_level=0), **solver_kw)))
    for v in m["vars"]:
        M.variable(v["lb"], v["ub"])
    M.objective(m["sense"], ktn.from_sexpr(m["objective"]), linear=m["objective_linear"])
    for c in m["constraints"]:
        M.constraint((ktn.from_sexpr(c["expr"]), c["lb"], c["ub"]), linear=c["linear"])
    return M


def hip_load_instance(ktn, inst, **solver_kw):
    m = ktn.NonlinearModel(ktn.KatanaSolver(**dict(dict(log_level=0), **solver_kw)))
    m.loadproblem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr, inst.u_constr, inst.sense,
                  ktn.SeparableNLP(inst))
    return m


def pool_arrays(m):
    """the cut pool as a caller reads it: ((rowptr, col, val, lo, hi), duals, number of rows, number of cuts)"""
    return m.lp_rows(), m.lp_duals(), m.lp_num_rows(), m.numcuts()


def pool_bits(m):
    """pool_arrays with every array as its bytes: two pools are equal bit for bit when these lists are"""
    rows, duals, nrows, ncuts = pool_arrays(m)
    return [a.tobytes() for a in rows] + [duals.tobytes(), nrows, ncuts]


def planted_obj_bound(inst, f_tol=1e-6, lp_gap=1e-7):
    """Per-instance bound on |objective - planted optimum| at a point that meets the stop rule (src/model.jl:257,273).
    xhat is a KKT point with multipliers lambda_i (NL rows), mu_r (linear rows) and bound multipliers, so for the convex
    problem  f(x) >= f(xhat) - sum_i lambda_i max(g_i(x), 0) - sum_r mu_r max(a_r'x - b_r, 0)  for x inside the box.  The
    loop stops with every g_i <= f_tol; the LP leaves the linear rows within its row tolerance (0.3 f_tol, accepted up to
    twice that: DESIGN.md section 5), the box is met exactly (the prox clips), and the LP objective is certified to the
    relative duality-gap floor lp_gap.  With a nonlinear objective the epigraph row f(x) - t <= 0 is one more NL row
    with multiplier 1."""
    lam = inst.meta["lam_sum"] + (1.0 if inst.meta.get("objective") == "quad" else 0.0)
    return f_tol * (lam + 0.6 * inst.meta["mu_sum"]) + lp_gap * (1.0 + 2.0 * abs(inst.opt_obj))


def assert_planted_objective(obj, inst, f_tol=1e-6):
    """The objective assertions of every planted-optimum test, in this order:
    (1) the reference's own acceptance test, isapprox(obj, expected; atol = rtol = 1e-6) (test/runtests.jl:16-17, test/2d.jl:19),
        with the planted optimum as the expected value;
    (2) the per-instance Lagrangian bound of planted_obj_bound -- looser than (1) on the large configurations (its
        0.6 sum(mu) f_tol term dominates), kept because it is what the stop rule guarantees a priori."""
    tol = max(1e-6, 1e-6 * max(abs(obj), abs(inst.opt_obj)))
    assert abs(obj - inst.opt_obj) <= tol, ("reference tolerance 1e-6/1e-6", obj, inst.opt_obj, abs(obj - inst.opt_obj), tol)
    assert abs(obj - inst.opt_obj) <= planted_obj_bound(inst, f_tol=f_tol), ("planted bound", obj, inst.opt_obj)


def max_nl_violation(inst, x):
    """max over NL rows of g_i(x) - ub_i under the oracle's evaluator"""
    d = oracle_evaluator(inst)
    g = np.zeros(inst.num_constr)
    d.eval_g(g, np.asarray(x)[:inst.n])
    return float(np.max(g[inst.m_lin:] - inst.u_constr[inst.m_lin:])) if inst.m_nl else 0.0


# KATs whose *solution vector / tight objective* check depends on which LP vertices the LP
# solver happens to visit (GLPK in the reference): the stop rule g <= f_tol = 1e-6 bounds the
# tangential error of x only by ~sqrt(2 f_tol) = 1.4e-3 on these flat optima, while the
# reference's tests ask for 1e-3 (or rtol 1e-7 on 202_04).  Status and objective at the
# suite-wide 1e-6 tolerance are asserted for every KAT; for these ids x is asserted at 3e-3.
TRAJECTORY_SENSITIVE = {"105_04", "202_04", "501_02_n3", "501_02_n4", "501_02_n9"}


def instance_as_expressions(ktn, inst):
    """(objective, constraints) of a SeparableInstance written as expressions, atom by atom in storage order, folded left
    to right: LIN p0*x, QUAD p0*(x-p1)^2, EXP p0*exp(p1*x), NEGLOG -p0*log(x+p1); every row ends with + rconst."""
    def atoms(cols, kinds, p0, p1):
        e = None
        for j, k, a, b in zip(cols, kinds, p0, p1):
            x = ktn.var(int(j))
            a, b = float(a), float(b)
            t = [a * x, a * (x - b) ** 2, a * ktn.exp(b * x), (-a) * ktn.log(x + b)][int(k)]
            e = t if e is None else e + t
        return e
    rp = inst.rowptr
    cons = []
    for i in range(inst.num_constr):
        s = slice(rp[i], rp[i + 1])
        e = atoms(inst.col[s], inst.kind[s], inst.p0[s], inst.p1[s])
        cons.append(ktn.const(float(inst.rconst[i])) if e is None else e + float(inst.rconst[i]))
    obj = atoms(inst.obj_col, inst.obj_kind, inst.obj_p0, inst.obj_p1) + float(inst.obj_const)
    return obj, cons


def julia_shaped_nlp(ktn, n, objective, constraints, constr_linear, obj_linear, rng):
    """Restatement of build_ktn_nlp_desc (katana.jl_amd/julia/KatanaHIP.jl) for s-expression models: every row a TAPE row
    (linear rows too) with row_linear as declared, n-ary + and * folded left to right, the Jacobian structure taken from a
    COO list in shuffled order and converted to CSR row by row in COO order, the objective a TAPE even when linear."""
    from oracle import sexpr
    L = ktn._lib
    coo = [(i, j) for i, s in enumerate(constraints) for j in sexpr.variables(s)]
    coo = [coo[k] for k in rng.permutation(len(coo))]
    m = len(constraints)
    counts = np.bincount([i for i, _ in coo], minlength=m) if coo else np.zeros(m, dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    fill = rowptr[:-1].copy()
    col = np.zeros(len(coo), dtype=np.int32)
    for i, j in coo:
        col[fill[i]] = j
        fill[i] += 1
    tptr, top, targ = [0], [], []
    for s in constraints:
        o, a = ktn.from_sexpr(s).tape()
        top.extend(o.tolist()); targ.extend(a.tolist())
        tptr.append(len(top))
    oo, oa = ktn.from_sexpr(objective).tape()
    return ktn.NLPDescription(n, rowptr, col, np.full(m, L.ROW_TAPE), [1 if f else 0 for f in constr_linear], np.zeros(m),
                              None, None, None, tptr, top, targ, obj_linear=bool(obj_linear), obj_kind=L.ROW_TAPE,
                              obj_tape_op=oo, obj_tape_arg=oa)
