"""GPU tier: KTN_ROW_QUAD rows -- k_quad_jac / k_quad_stats against mpmath (tests/quad_ref.py) for every lane-group setting, the same
rows as expression tapes, solves with closed-form answers, the LinearQuadraticModel front end, the paths that do not take such
rows, and the validation of the quad_* arrays at ktn_loadproblem."""
import math

import numpy as np
import pytest
from mpmath import mp, mpf

import katana_jl_amd as ktn
import kat_util
import quad_cases as QC
import quad_ref as Q
import tape_ref

pytestmark = pytest.mark.gpu
L = ktn._lib
INF = math.inf


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_bits(a, b, what):
    a, b = bits(np.asarray(a)), bits(np.asarray(b))
    assert a.shape == b.shape and np.array_equal(a, b), (what, np.flatnonzero(a != b)[:8] if a.shape == b.shape else (a.shape, b.shape))


def handle(monkeypatch, G, d, n, m, lb, ub, lv=-2.0, uv=2.0, sense="Min", **kw):
    if G:
        monkeypatch.setenv("KTN_QUAD_GROUP", str(G))
    else:
        monkeypatch.delenv("KTN_QUAD_GROUP", raising=False)
    model = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, f_tol=Q.F_TOL, **kw))
    model.loadproblem(n, m, np.full(n, lv), np.full(n, uv), lb, ub, sense, d)
    sep = ktn.KatanaHipSeparator(model)
    sep.initialize()
    return model, sep


def pick_group(avg):
    g = 4
    while g < 64 and 2 * g <= avg:
        g <<= 1
    return g


def after_sweep(model, sep):
    lib, h = model._lib, model._h
    g, jac = np.zeros(sep.num_constr), np.zeros(sep.nnz)
    L.check(h, lib.ktn_sep_get_g(h, g.ctypes.data_as(L.P(L.c_f64)), len(g)))
    L.check(h, lib.ktn_sep_get_jac(h, jac.ctypes.data_as(L.P(L.c_f64)), len(jac)))
    return g, jac


def run_mixed(monkeypatch, G):
    """precompute at the case's point, gencut of every row, one sweep: everything read back"""
    C = QC.mixed_case()
    lb, ub = C.lb, C.ub
    model, sep = handle(monkeypatch, G, C.d, C.n, C.m, lb, ub)
    sep.precompute(C.xt)
    out = dict(model=model, sep=sep, g=sep.g.copy(), jac=sep.jac.copy())
    out["cuts"] = [sep.gencut(C.xt, None, i) for i in range(C.m + 1)]
    m0 = model.lp_num_rows()
    out["nviol"], out["maxviol"] = sep.sweep(C.f_tol)
    out["rows"] = model.lp_rows_from(m0)
    out["slots"] = model.last_sweep_slots()
    out["g2"], out["jac2"] = after_sweep(model, sep)
    return C, out


@pytest.mark.parametrize("G", [4, 16, 64, 0])
def test_kernels_against_mpmath_through_precompute_and_sweep(monkeypatch, G):
    C, o = run_mixed(monkeypatch, G)
    model, sep = o["model"], o["sep"]
    quad_rows = [i for i in range(C.m) if C.kind[i] == L.ROW_QUAD]
    qnnz = sum(len(C.layouts[i][4]) for i in quad_rows) + len(C.layouts["obj"][4])
    nent = sum(len(C.layouts[i][0]) for i in quad_rows) + len(C.layouts["obj"][0]) + 1
    assert model.stat("quad_rows") == len(quad_rows) + 1 and model.stat("quad_nnz") == qnnz
    assert model.stat("quad_group") == (G if G else pick_group(qnnz / nent))
    refs = dict(C.ref)
    refs[C.m] = C.obj_ref                                                                # the epigraph row f(x) - t
    rp = sep.rowptr
    for i, R in refs.items():
        what = (G, i, C.tags[i] if i < C.m else "epigraph")
        R.check_g(o["g"][i], what)
        R.check_der(o["jac"][rp[i]:rp[i + 1]], what)
        cols, coefs, const = o["cuts"][i]
        assert np.array_equal(cols, sep.col[rp[i]:rp[i + 1]]), what
        R.check_der(coefs, what + ("gencut",))
        R.check_b(const, what + ("gencut",))
    assert np.array_equal(sep.col[rp[C.m]:rp[C.m + 1]], np.concatenate([C.layouts["obj"][0], [C.n]]))
    assert o["jac"][rp[C.m + 1] - 1] == -1.0                                              # t: coefficient -1, empty segment
    # the sweep: the exact violated set, in NL-slot order
    nl = [i for i in range(C.m) if not C.d.row_linear[i]] + [C.m]
    viol = np.concatenate([C.violated, [True]])
    want = [s for s, i in enumerate(nl) if viol[i]]
    assert o["nviol"] == len(want) and o["slots"].tolist() == want, (o["slots"].tolist(), want)
    assert_bits(o["g2"], o["g"], "g after the sweep")
    assert_bits(o["jac2"], o["jac"], "Jacobian after the sweep")
    e_lb, e_ub = np.concatenate([C.lb, [-INF]]), np.concatenate([C.ub, [0.0]])
    with np.errstate(invalid="ignore"):
        dv = np.maximum(o["g"][[nl[s] for s in want]] - e_ub[[nl[s] for s in want]], e_lb[[nl[s] for s in want]] - o["g"][[nl[s] for s in want]])
    assert o["maxviol"] == dv.max()
    top = nl[want[int(np.argmax(dv))]]
    if top in refs:
        with mp.workprec(Q.PREC):
            R = refs[top]
            exact = max(R.g - mpf(e_ub[top]), mpf(e_lb[top]) - R.g)
            assert abs(mpf(o["maxviol"]) - exact) <= R.e_g + 2 * mpf(Q.U) * abs(exact)
    # the appended LP rows
    rowptr, col, val, lo, hi = o["rows"]
    assert len(lo) == len(want)
    for k, s in enumerate(want):
        i = nl[s]
        c, v = col[rowptr[k]:rowptr[k + 1]], val[rowptr[k]:rowptr[k + 1]]
        assert np.array_equal(c, sep.col[rp[i]:rp[i + 1]]), (G, i)
        assert_bits(v, o["jac"][rp[i]:rp[i + 1]], ("cut coefficients", G, i))             # (no coefficient is 1e9 below the largest)
        if i not in refs:
            continue
        R = refs[i]
        for name, got, bnd in (("lo", lo[k], e_lb[i]), ("hi", hi[k], e_ub[i])):
            if math.isfinite(bnd):
                with mp.workprec(Q.PREC):
                    assert abs(mpf(got) - (mpf(bnd) - R.b)) <= R.bound_tol(bnd), (G, i, name, got)
            else:
                assert got == bnd, (G, i, name, got)
    # two runs on two handles: bit-identical
    _, o2 = run_mixed(monkeypatch, G)
    for key in ("g", "jac", "g2", "jac2"):
        assert_bits(o2[key], o[key], (key, "second handle"))
    assert o2["nviol"] == o["nviol"] and bits(np.float64(o2["maxviol"])) == bits(np.float64(o["maxviol"]))
    for a, b in zip(o2["rows"], o["rows"]):
        assert_bits(a, b, "LP rows, second handle")


def test_same_model_as_tapes_and_untouched_paths_bit_for_bit(monkeypatch):
    C, o = run_mixed(monkeypatch, 0)
    sep = o["sep"]
    rp = sep.rowptr
    d_t, rows_t = QC.as_tapes(C)
    mt, st = handle(monkeypatch, 0, d_t, C.n, C.m, C.lb, C.ub)
    st.precompute(C.x)
    for i, R in C.ref.items():
        if C.d.row_linear[i]:
            continue
        ops, args = rows_t[i][1].tape()
        T = tape_ref.evaluate(ops, args, C.x)
        with mp.workprec(Q.PREC):
            tol = R.e_g + 2 * T.err + 4 * mpf(Q.U) * abs(T.value)
            assert abs(mpf(float(o["g"][i])) - mpf(float(st.g[i]))) <= tol, (i, o["g"][i], st.g[i], float(tol))
            tj = dict(zip(st.col[st.rowptr[i]:st.rowptr[i + 1]].tolist(), st.jac[st.rowptr[i]:st.rowptr[i + 1]].tolist()))
            for e, c in enumerate(sep.col[rp[i]:rp[i + 1]].tolist()):
                # (a column whose Q row and linear coefficient are empty does not occur in the expression's product terms alone)
                jt = tj.get(c, 0.0)
                tolj = R.e_der[e] + T.grad_tol(c) if c in tj else R.e_der[e]
                assert abs(mpf(float(o["jac"][rp[i] + e])) - mpf(jt)) <= tolj, (i, c, o["jac"][rp[i] + e], jt)
    # the SEP / TAPE rows of the mixed model: bit for bit what a handle without the QUAD rows gives
    d_c, keep, lb_c, ub_c = QC.without_quad(C)
    mc, sc = handle(monkeypatch, 0, d_c, C.n, len(keep), lb_c, ub_c)
    sc.precompute(C.x)
    cuts_c = [sc.gencut(C.x, None, k) for k in range(len(keep))]
    m0 = mc.lp_num_rows()
    sc.sweep(C.f_tol)
    rows_c = mc.lp_rows_from(m0)
    g2c, jac2c = after_sweep(mc, sc)
    for k, i in enumerate(keep):
        assert_bits(o["g"][i], sc.g[k], ("g", i))
        assert_bits(o["g2"][i], g2c[k], ("g after the sweep", i))
        assert_bits(o["jac"][rp[i]:rp[i + 1]], sc.jac[sc.rowptr[k]:sc.rowptr[k + 1]], ("jac", i))
        assert_bits(o["jac2"][rp[i]:rp[i + 1]], jac2c[sc.rowptr[k]:sc.rowptr[k + 1]], ("jac after the sweep", i))
        assert_bits(o["cuts"][i][1], cuts_c[k][1], ("gencut coefficients", i))
        assert bits(np.float64(o["cuts"][i][2])) == bits(np.float64(cuts_c[k][2])), ("gencut constant", i)
    nl = [i for i in range(C.m) if not C.d.row_linear[i]] + [C.m]
    cut_rows = [nl[s] for s in o["slots"]]
    rowptr, col, val, lo, hi = o["rows"]
    sel = [k for k, i in enumerate(cut_rows) if i < C.m and C.kind[i] != L.ROW_QUAD]
    rc, cc, vc, loc, hic = rows_c
    assert len(sel) == len(loc)
    for kc, k in enumerate(sel):
        assert np.array_equal(col[rowptr[k]:rowptr[k + 1]], cc[rc[kc]:rc[kc + 1]])
        assert_bits(val[rowptr[k]:rowptr[k + 1]], vc[rc[kc]:rc[kc + 1]], ("LP row", k))
        assert bits(np.float64(lo[k])) == bits(np.float64(loc[kc])) and bits(np.float64(hi[k])) == bits(np.float64(hic[kc]))


def solve(p, **kw):
    m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, **kw))
    m.loadproblem(*p)
    st = m.optimize()
    return st, m.getobjval(), m.getsolution()[:p.num_var], m


@pytest.mark.parametrize("n", [4, 8, 40])
def test_ellipsoid_against_its_closed_form(n):
    """the reference's acceptance rule against the closed form, the tape form of the same model as the control.  (n = 40, the
    mid-size LP range: Kelley's method takes 3 939 rounds on the QUAD form and 3 625 on the tape form, about 25 s each.)"""
    C = QC.ellipsoid(n)
    for form, p in (("tape (control)", QC.ellipsoid_tape(C)), ("quad", QC.ellipsoid_quad(C))):
        st, obj, x, m = solve(p)
        print("ellipsoid n=%d %s: %s obj=%.12g f*=%.12g err=%.3g iters=%d" % (n, form, st, obj, C.fstar, abs(obj - C.fstar), m.numiters()))
        assert st == "Optimal", (form, st)
        assert kat_util.isapprox(obj, C.fstar, 1e-6, 1e-6), (form, obj, C.fstar)
        if n <= 8:
            assert np.abs(x - C.xstar).max() <= 1e-3, (form, x, C.xstar)
    assert m.stat("quad_rows") == 2 and m.stat("quad_nnz") == n * n                      # (the constraint and the linear objective's row)


@pytest.mark.parametrize("n", [4, 8])
def test_qp_against_its_closed_form(n):
    C = QC.qp(n)
    for form, p in (("tape (control)", QC.qp_tape(C)), ("quad", QC.qp_quad(C))):
        st, obj, x, m = solve(p)
        print("qp n=%d %s: %s obj=%.12g f*=%.12g err=%.3g iters=%d" % (n, form, st, obj, C.fstar, abs(obj - C.fstar), m.numiters()))
        assert st == "Optimal", (form, st)
        assert kat_util.isapprox(obj, C.fstar, 1e-6, 1e-6), (form, obj, C.fstar)


def lpqp_parts(model):
    """(A, rowlb, rowub, obj, quadratic diagonal, constant) of a test/lpqp.jl fixture: affine rows, and an objective that is affine
    or a sum of (x_j - p)^2"""
    n = len(model["vars"])
    A, lo, hi = [], [], []
    for c in model["constraints"]:
        co, c0 = ktn.from_sexpr(c["expr"]).affine()
        A.append([co.get(j, 0.0) for j in range(n)]); lo.append(c["lb"] - c0); hi.append(c["ub"] - c0)
    obj, diag, const = np.zeros(n), np.zeros(n), 0.0
    aff = ktn.from_sexpr(model["objective"]).affine()
    if aff is not None:
        for j, v in aff[0].items():
            obj[j] = v
        const = aff[1]
    else:
        terms = model["objective"][1:]
        assert model["objective"][0] == "+"
        for t in terms:
            assert t[0] == "^" and t[2] == 2.0 and t[1][0] == "-" and t[1][1][0] == "var", t
            j, p = t[1][1][1], float(t[1][2])
            diag[j] += 2.0; obj[j] += -2.0 * p; const += p * p                              # (x - p)^2 = 1/2 * 2 x^2 - 2 p x + p^2
    return np.array(A), lo, hi, obj, diag, const


@pytest.mark.parametrize("kid", ["001_01", "001_02", "002_01", "002_02"])
def test_linear_quadratic_model_on_the_lpqp_models(kid):
    model = next(m for m in kat_util.load_kats() if m["id"] == kid and m["ref"].startswith("test/lpqp.jl"))
    A, lo, hi, obj, diag, const = lpqp_parts(model)
    m = ktn.LinearQuadraticModel(ktn.KatanaSolver(log_level=0))
    m.loadproblem(A, [v["lb"] for v in model["vars"]], [v["ub"] for v in model["vars"]], obj, lo, hi, model["sense"])
    if diag.any():
        m.setquadobj(np.flatnonzero(diag), np.flatnonzero(diag), diag[diag != 0])
    st = m.optimize()
    assert m.stat("quad_rows") == len(lo) + 1
    kat_util.check_expectation(model, st, m.getobjval() + const, m.getsolution()[:len(obj)])


def test_linear_quadratic_model_unit_disc_through_addquadconstr():
    import scipy.sparse as sp
    m = ktn.LinearQuadraticModel(ktn.KatanaSolver(log_level=0))
    m.loadproblem(sp.csr_matrix((0, 2)), [-2.0, -2.0], [2.0, 2.0], [1.0, 1.0], [], [], "Max")
    m.addquadconstr([], [], [0, 1], [0, 1], [1.0, 1.0], "<", 1.0)
    st = m.optimize()
    assert st == "Optimal" and kat_util.isapprox(m.getobjval(), math.sqrt(2.0), 1e-6, 1e-6), (st, m.getobjval())
    assert np.abs(m.getsolution()[:2] - math.sqrt(0.5)).max() <= 1e-3


def test_optimize_blocks_falls_back_to_the_ordinary_loop():
    Cs = [QC.ellipsoid(4), QC.ellipsoid(4, seed=21)]
    rows, cvec = [], []
    for k, C in enumerate(Cs):
        r, c, v = QC._full(C.Q)
        rows.append((np.arange(4) + 4 * k, C.lin, r + 4 * k, c + 4 * k, v, C.const))
        cvec += C.c.tolist()
    d = ktn.QuadNLP(8, cvec, 0.0, None, rows)
    out = []
    for blocks in (True, False):
        m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))
        m.loadproblem(8, 2, np.full(8, -10.0), np.full(8, 10.0), [-INF, -INF], [1.0, 1.0], "Min", d)
        m.set_blocks([0, 4, 8])
        st = m.optimize_blocks() if blocks else m.optimize()
        out.append((st, m.getobjval(), m.getsolution(), m.numiters(), m.numcuts()))
    assert out[0][0] == out[1][0] == "Optimal"
    assert out[0][1] == out[1][1] and np.array_equal(out[0][2], out[1][2]) and out[0][3:] == out[1][3:], out
    assert abs(out[0][1] - (Cs[0].fstar + Cs[1].fstar)) <= 1e-4


def test_supporting_hyperplanes_keep_kelleys_cut_on_quad_rows(monkeypatch):
    C = QC.mixed_case()
    keep = [i for i in range(C.m) if C.kind[i] != L.ROW_TAPE]
    rows = [C.rows[i] for i in keep]
    d, _ = QC.assemble(C.n, rows, ("lin", [0, 1], [1.0, -1.0]))
    lb, ub = C.lb[keep], C.ub[keep]
    out = []
    for algo in ("kelley", "supporting_hyperplane"):
        model, sep = handle(monkeypatch, 0, d, C.n, len(keep), lb, ub, cut_algo=algo, esh_interior_iters=10)
        if algo != "kelley":
            xi = model.interior_point()                                                 # found or not: no error
            assert xi is None or len(xi) == C.n
        sep.precompute(C.x)
        m0 = model.lp_num_rows()
        nv, _ = sep.sweep(C.f_tol)
        out.append((model, nv, model.last_sweep_slots(), model.lp_rows_from(m0)))
    (mk, nvk, sk, rk), (me, nve, se, re_) = out
    assert nvk == nve and np.array_equal(sk, se)
    nl = [k for k in range(len(keep)) if not d.row_linear[k]]
    nquad = 0
    for j, s in enumerate(sk):
        if rows[nl[s]][0] != "quad":
            continue
        nquad += 1
        for a, b in ((rk[1], re_[1]), (rk[2], re_[2])):
            assert np.array_equal(a[rk[0][j]:rk[0][j + 1]], b[re_[0][j]:re_[0][j + 1]]), ("cut of QUAD row", keep[nl[s]])
        assert rk[3][j] == re_[3][j] and rk[4][j] == re_[4][j]
    assert nquad >= 5 and me.stat("esh_fallback_rows") >= nquad
    assert me.stat("esh_fallback_rows") + me.stat("esh_rows") == nve


def small_desc(**over):
    """two rows on three columns: row 0 QUAD with Q on (0, 1), row 1 separable"""
    kw = dict(num_var=3, rowptr=[0, 2, 3], col=[0, 1, 2], row_kind=[L.ROW_QUAD, L.ROW_SEP], row_linear=[0, 1], rconst=[0.0, 0.0],
              atom_kind=[0, 0, 0], p0=[1.0, 1.0, 1.0], p1=[0.0, 0.0, 0.0], quad_ptr=[0, 2, 4, 4], quad_col=[0, 1, 0, 1],
              quad_val=[2.0, 0.5, 0.5, 2.0], obj_linear=True, obj_kind=L.ROW_SEP, obj_col=[0], obj_atom_kind=[0], obj_p0=[1.0],
              obj_p1=[0.0])
    kw.update(over)
    return ktn.NLPDescription(**kw)


@pytest.mark.parametrize("what, over, msg", [
    ("QUAD rows without quad_ptr", dict(quad_ptr=None, quad_col=None, quad_val=None), "quad_ptr"),
    ("non-monotone quad_ptr", dict(quad_ptr=[0, 2, 1, 4]), "monotone"),
    ("quad_col outside the row's structure", dict(quad_col=[0, 2, 0, 1]), "structure"),
    ("quad_col out of range", dict(quad_col=[0, 7, 0, 1]), "structure"),
    ("a segment on a row that is not QUAD", dict(quad_ptr=[0, 2, 3, 4]), "not KTN_ROW_QUAD"),
    ("row_linear on a QUAD row with a Q", dict(row_linear=[1, 1]), "row_linear"),
    ("obj_linear with an objective Q", dict(obj_kind=L.ROW_QUAD, obj_col=[0, 1], obj_p0=[1.0, 1.0], obj_atom_kind=None, obj_p1=None,
                                            obj_quad_ptr=[0, 1, 2], obj_quad_col=[0, 1], obj_quad_val=[1.0, 1.0]), "obj_linear"),
    ("non-monotone obj_quad_ptr", dict(obj_linear=False, obj_kind=L.ROW_QUAD, obj_col=[0, 1], obj_p0=[1.0, 1.0], obj_atom_kind=None,
                                       obj_p1=None, obj_quad_ptr=[0, 2, 1], obj_quad_col=[0, 1], obj_quad_val=[1.0, 1.0]), "monotone"),
])
def test_loadproblem_refuses_malformed_quad_arrays(what, over, msg):
    m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))
    args = (3, 2, np.full(3, -1.0), np.full(3, 1.0), [-INF, -INF], [1.0, 1.0], "Min")
    with pytest.raises(L.KatanaHipError, match=msg) as ei:
        m.loadproblem(*args, small_desc(**over))
    assert ei.value.code == L.E_INVALID, what
    m.loadproblem(*args, small_desc())                                                    # the handle is still usable
    assert m.stat("quad_rows") == 1 and m.stat("quad_nnz") == 4
