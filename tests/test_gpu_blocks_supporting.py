"""GPU tier: supporting-hyperplane cuts inside the device-side batch loop (ktn_optimize_blocks_ex with KTN_BLOCKS_SUPPORTING;
k_ecp_blocks<1> of csrc/batch_ecp.hpp).

One round is read back cut by cut (ktn_blocks_get_cuts) and checked against tests/esh_ref.py / tests/esh_quad_ref.py in mpmath; the
rows that cannot take part -- and every tape row -- against the Kelley device loop of the same build, bit for bit; whole solves
against the planted optima and the Kelley device loop.

The interior points are the caller's unless a test says otherwise, by the rule of
test_gpu_supporting_hyperplanes.test_caller_point_is_used_as_given_and_reported_back: 0 where the box contains it, else the box
midpoint.  The generator's box half-width is B = 1.5 here: with its default of 10 the midpoint of a pinned variable's range lies
near +-5, where no row of the "quad" family holds it inside, so no cut of that family would move."""
import math

import mpmath as mp
import numpy as np
import pytest

import esh_quad_ref as ER
import esh_ref
import katana_jl_amd as ktn
import quad_cases as QC
import quad_ref as Q
import sep_cases as sc
from fuse_helpers import expr_problem
from helpers import assert_planted_objective
from katana_jl_amd.batch import FusedBatch
from test_gpu_supporting_hyperplanes import DELTA, F_TOL, TAU, _check_separable_cut, _cone_family, _rows

pytestmark = pytest.mark.gpu
L = ktn._lib
INF = math.inf
make = ktn.instances.make_instance
ESH = "supporting_hyperplane"
ESHQ = "supporting_hyperplane_quad"


def solver(algo="kelley", **kw):
    return ktn.KatanaSolver(log_level=0, f_tol=F_TOL, cut_algo=algo, **dict(dict(lp_max_iter=400000), **kw))


def caller_point(inst):
    inside = np.all(np.asarray(inst.l_var) <= 0) and np.all(np.asarray(inst.u_var) >= 0)
    return np.zeros(len(inst.l_var)) if inside else 0.5 * (np.asarray(inst.l_var) + np.asarray(inst.u_var))


def depth_mp(row, xi, bound):
    """bound - g(x_int) of an upper-side separable row, in mpmath"""
    return -float(esh_ref.phi(row, xi, xi, 1, bound, 0.0, mp)[0])


def as_problem(inst, l_constr=None):
    return ktn.Problem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr if l_constr is None else l_constr, inst.u_constr,
                       inst.sense, ktn.SeparableNLP(inst))


def one_round(items, algo, points=None, supporting=None):
    """one cutting-plane round of the device loop without the fall-back: (batch, status, x)"""
    fb = FusedBatch(solver(algo, iter_cap=1), items)
    if points is not None:
        fb.set_interior_points(points)
    st = fb.m.optimize_blocks(supporting=(algo != "kelley") if supporting is None else supporting, fallback=False)
    return fb, st, fb.m.getsolution()


def cuts_of(fb, b):
    c = fb.m.blocks_cuts(b)
    rp = c["rowptr"]
    return [(c["col"][rp[k]:rp[k + 1]] - int(fb.offs[b]), c["val"][rp[k]:rp[k + 1]], c["lo"][k], c["hi"][k], int(c["slot"][k]), float(c["lam"][k]))
            for k in range(len(c["lo"]))]


def same_cut(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3] and a[4] == b[4], what


def linear_only(inst):
    """the instance without its nonlinear rows (the generator makes none with m_nl = 0): an LP, its optimum from HiGHS"""
    import dataclasses
    import scipy.sparse as sp
    from scipy.optimize import linprog
    e = int(inst.rowptr[inst.m_lin])
    A = sp.csr_matrix((inst.p0[:e], inst.col[:e], inst.rowptr[:inst.m_lin + 1]), shape=(inst.m_lin, inst.n))
    assert np.all(inst.kind[:e] == 0)
    c = np.zeros(inst.n)
    c[inst.obj_col] = inst.obj_p0
    r = linprog(c, A_ub=A, b_ub=inst.u_constr[:inst.m_lin] - inst.rconst[:inst.m_lin], bounds=list(zip(inst.l_var, inst.u_var)), method="highs")
    assert r.status == 0
    return dataclasses.replace(inst, rowptr=inst.rowptr[:inst.m_lin + 1], col=inst.col[:e], kind=inst.kind[:e], p0=inst.p0[:e], p1=inst.p1[:e],
                               rconst=inst.rconst[:inst.m_lin], l_constr=inst.l_constr[:inst.m_lin], u_constr=inst.u_constr[:inst.m_lin],
                               xhat=r.x, opt_obj=float(r.fun + inst.obj_const), m_nl=0, meta=dict(inst.meta, m_nl=0, lam_sum=0.0))


# ---- the batch of tests 1 and 6: rows shorter than, equal to and longer than one 16-lane trip, both families, one instance
# without nonlinear rows
@pytest.fixture(scope="module")
def batch1():
    insts = [make(n=96, m_nl=12, k=k, family=f, seed=1, B=1.5) for f in ("explog", "quad") for k in (3, 16, 40)]
    insts.append(make(n=96, m_nl=12, k=16, family="quad", seed=0, B=1.5))
    insts.append(linear_only(make(n=96, m_nl=12, k=16, family="explog", seed=2, B=1.5)))
    assert len(insts) == 8 and insts[-1].m_nl == 0
    return insts, [caller_point(i) for i in insts]


def check_separable_round(fb, x, insts, points, nl0):
    """every cut of every instance after one round; returns (moved, kelley, moved per family)"""
    moved = kelley = 0
    by_family = {}
    for b, inst in enumerate(insts):
        xs, xi = x[fb.offs[b]:fb.offs[b + 1]][:inst.n], points[b]
        rows = _rows(inst)
        seen = set()
        for cols, a, lo, hi, slot, lam in cuts_of(fb, b):
            i = inst.m_lin + slot - nl0[b]
            assert inst.m_lin <= i < inst.num_constr and i not in seen, (b, slot)
            seen.add(i)
            assert np.array_equal(cols, rows[i].cols), (b, i)
            assert 0.0 < lam <= 1.0 and lo == -INF
            deep = depth_mp(rows[i], xi, inst.u_constr[i]) >= DELTA
            if lam == 1.0:
                assert not deep, (b, i, "a row that holds the point inside keeps Kelley's cut")
                kelley += 1
                continue
            assert deep, (b, i)
            _check_separable_cut(rows[i], xi, xs, lam, inst.u_constr[i], a, hi)
            moved += 1
            by_family[inst.meta["family"]] = by_family.get(inst.meta["family"], 0) + 1
        if inst.m_nl == 0:
            assert not seen
    return moved, kelley, by_family


def test_one_round_cut_by_cut_on_separable_rows(batch1):
    insts, points = batch1
    fb, st, x = one_round(insts, ESH, points)
    assert st in ("UserLimit", "Optimal")
    assert fb.m.stat("ecp_blocks_launches") == 1 and fb.m.stat("ecp_blocks_fallbacks") == 0 and fb.m.stat("esh_interior_rounds") == 0
    nl0 = np.concatenate([[0], np.cumsum([i.m_nl for i in insts])])
    moved, kelley, fam = check_separable_round(fb, x, insts, points, nl0)
    print("one round: %d cuts moved %s, %d at x*" % (moved, fam, kelley))
    assert fam.get("explog", 0) > 0 and fam.get("quad", 0) > 0, fam
    res = fb.m.blocks_results()
    assert res.shape == (8, 8) and np.all(res[:, 1] == 1) and np.all(res[:, 7] == 0)
    assert int(np.sum(res[:, 6]) - sum(i.m_lin for i in insts)) == moved + kelley
    assert res[-1, 0] == L.STATUS_OPTIMAL and res[-1, 6] == insts[-1].m_lin          # the instance without nonlinear rows
    assert fb.m.stat("esh_rows") == moved == fb.m.stat("ecp_blocks_esh_rows") and fb.m.stat("esh_fallback_rows") == kelley
    assert fb.m.stat("esh_newton_steps") >= moved and fb.m.stat("esh_quad_rows") == 0
    # the host-loop read-back keeps describing host-loop sweeps only
    assert len(fb.m.last_sweep_lambdas()) == 0


def test_rows_that_cannot_take_part_keep_kelleys_cut(batch1):
    """two-sided rows, nonlinear equalities, rows the point does not hold delta inside and every tape row: the cut of the Kelley
    device loop, bit for bit, lambda = 1, counted as fallback rows"""
    insts, points = batch1
    insts, points = insts[:7], points[:7]
    items, two_sided, equal = [], {}, {}
    for b, inst in enumerate(insts):
        l = inst.l_constr.copy()
        nl = list(range(inst.m_lin, inst.num_constr))
        two_sided[b], equal[b] = nl[1::5], nl[2::5]
        l[two_sided[b]] = -1e6
        l[equal[b]] = inst.u_constr[equal[b]]
        items.append(as_problem(inst, l))
    tape_of = 1                                                    # an instance built from expressions: its rows are tape rows
    items.append(expr_problem(insts[tape_of]))
    pts = points + [points[tape_of]]
    fe, _, xe = one_round(items, ESH, pts)
    fk, _, xk = one_round(items, "kelley")
    assert fe.m.stat("ecp_blocks_launches") == 1 and fk.m.stat("ecp_blocks_launches") == 1
    assert np.array_equal(xe, xk)                                  # the LP text is shared by the two instantiations
    assert fe.m.stat("ecp_blocks_tape_rows") == insts[tape_of].m_nl
    nl0 = np.concatenate([[0], np.cumsum([i.m_nl for i in insts] + [insts[tape_of].m_nl])])
    seen = dict(two_sided=0, equality=0, not_inside=0, tape=0)
    moved = kelley = 0
    for b in range(8):
        inst = insts[b] if b < 7 else insts[tape_of]
        rows = _rows(inst)
        ce, ck = cuts_of(fe, b), cuts_of(fk, b)
        assert len(ce) == len(ck) > 0
        for e, k in zip(ce, ck):
            assert k[5] == 1.0 and e[4] == k[4]
            i = inst.m_lin + e[4] - nl0[b]
            cls = ("tape" if b == 7 else "two_sided" if i in two_sided[b] else "equality" if i in equal[b] else
                   "not_inside" if not depth_mp(rows[i], pts[b], inst.u_constr[i]) >= DELTA else None)
            if cls is not None:
                seen[cls] += 1
                assert e[5] == 1.0, (b, i, cls)
            if e[5] == 1.0:
                kelley += 1
                same_cut(e, k, (b, i, cls))
            else:
                moved += 1
    assert all(v > 0 for v in seen.values()), seen
    assert moved > 0 and fe.m.stat("esh_rows") == moved and fe.m.stat("esh_fallback_rows") == kelley
    assert np.all(np.concatenate([fk.m.blocks_cuts(b)["lam"] for b in range(8)]) == 1.0)


# ---- QUAD rows -------------------------------------------------------------------------------------------------------------------
def ellipsoid_item(n, rho, seed=None, tilt=0.0, indefinite=False):
    """min c'x s.t. 1/2 (x - x0)'Q(x - x0) [+ tilt v'(x - x0)] <= rho over [-10, 10]^n and a linear row that never binds.  The first
    LP point is the box vertex x_j = -10 sign(c_j); `indefinite` subtracts 1.5 (v'Qv) v v' from Q with v along vertex - x0, so that
    d'Qd < 0 on the segment from x0, and the tilt keeps the row violated at the vertex."""
    C = QC.ellipsoid(n, seed)
    C.rho = rho
    Qm, lin, const = C.Q, C.lin, C.const
    d = -10.0 * np.sign(C.c) - C.x0
    v = d / np.linalg.norm(d)
    if indefinite:
        Qm = Qm - 1.5 * float(v @ Qm @ v) * np.outer(v, v)
        Qm = (Qm + Qm.T) / 2
        lin, const = -(Qm @ C.x0), 0.5 * float(C.x0 @ Qm @ C.x0)
    if tilt:
        lin, const = lin + tilt * v, const - tilt * float(v @ C.x0)
    r, c, q = QC._full(Qm)
    rows = [("quad", np.arange(n), lin, r, c, q, const, False),
            ("sep", np.arange(n), np.zeros(n, dtype=np.uint8), np.ones(n), np.zeros(n), 0.0, True)]
    desc, layouts = QC.assemble(n, rows, ("lin", np.arange(n), C.c))
    C.Qm, C.layout, C.rconst = Qm, layouts[0], const
    C.g = lambda x: float(0.5 * (x - C.x0) @ Qm @ (x - C.x0) + tilt * (v @ (x - C.x0)))
    return C, ktn.Problem(n, 2, np.full(n, -10.0), np.full(n, 10.0), [-INF, -INF], [rho, 10.0 * n + 1.0], "Min", desc)


@pytest.fixture(scope="module")
def quad_batch():
    cases = [ellipsoid_item(n, rho) for n in (2, 4, 8) for rho in (4.0, 1.0)]
    cases.append(ellipsoid_item(4, 4.0, seed=41, tilt=200.0, indefinite=True))
    cases.append(ellipsoid_item(4, 4.0, seed=42))
    points = [C.x0.copy() for C, _ in cases]
    # the last instance's point: on the ray towards the first LP point, half of delta inside the bound
    C = cases[-1][0]
    d = -10.0 * np.sign(C.c) - C.x0
    points[-1] = C.x0 + d * math.sqrt((C.rho - 0.5 * DELTA) / C.g(C.x0 + d))
    tags = ["part"] * 6 + ["indefinite", "shallow"]
    for (C, _), p, t in zip(cases, points, tags):
        depth = C.rho - C.g(p)
        assert (depth >= DELTA) == (t != "shallow") and depth > 0, (t, depth)
    return cases, points, tags


@pytest.mark.parametrize("G", [4, 16, 64, 0])
def test_quad_rows_closed_form_in_the_device_loop(monkeypatch, quad_batch, G):
    cases, points, tags = quad_batch
    items = [p for _, p in cases]
    if G:
        monkeypatch.setenv("KTN_ECP_QUAD_GROUP", str(G))
    else:
        monkeypatch.delenv("KTN_ECP_QUAD_GROUP", raising=False)
    fe, _, xe = one_round(items, ESHQ, points)
    fk, _, xk = one_round(items, "kelley")
    assert fe.m.stat("ecp_blocks_launches") == 1 and fe.m.stat("ecp_blocks_quad_rows") == 8
    assert np.array_equal(xe, xk)
    moved = 0
    for b, ((C, _), xi, tag) in enumerate(zip(cases, points, tags)):
        xs = xe[fe.offs[b]:fe.offs[b + 1]]
        ce, ck = cuts_of(fe, b), cuts_of(fk, b)
        assert len(ce) == len(ck) == 1 and ce[0][4] == b, (b, tag)
        cols, a, lo, hi, slot, lam = ce[0]
        assert np.array_equal(cols, np.arange(C.n))
        if tag == "indefinite":
            dd = xs - xi
            assert dd @ C.Qm @ dd < 0
        if tag != "part":
            assert lam == 1.0, (b, tag)
            same_cut(ce[0], ck[0], (b, tag))
            continue
        moved += 1
        assert 0.0 < lam < 1.0 and lo == -INF
        R = ER.cut_ref_mp(C.layout, C.rconst, xi, xs, 1, C.rho, lam, TAU)
        with mp.workprec(Q.PREC):
            assert 0 <= R.phi <= TAU, (b, float(R.phi))
            for e in range(R.k):
                assert abs(mp.mpf(float(a[e])) - R.der[e]) <= R.e_der[e], (b, e, a[e], float(R.der[e]), float(R.e_der[e]))
            assert abs(mp.mpf(float(hi)) - (mp.mpf(C.rho) - R.b)) <= R.bound_tol(C.rho), (b, hi, float(mp.mpf(C.rho) - R.b))
        assert a @ xs > hi and a @ xi <= hi - 0.5 * DELTA
    assert moved == 6 == fe.m.stat("esh_quad_rows") == fe.m.stat("esh_rows") and fe.m.stat("esh_fallback_rows") == 2


# ---- whole solves ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch16():
    insts = [make(n=200, m_nl=20, k=8, family=f, seed=s) for f in ("explog", "quad") for s in range(8)]
    kel = FusedBatch(solver(), insts)
    rk = kel.solve(cut_capacity=48)
    assert rk[0]["ecp_blocks_launches"] == 1 and rk[0]["ecp_blocks_fallbacks"] == 0
    return insts, rk, kel.m.blocks_results()


@pytest.fixture(scope="module")
def solved16(batch16):
    insts = batch16[0]
    fb = FusedBatch(solver(ESH), insts)
    res = fb.solve(cut_capacity=48, supporting=True)                # (the engine's own interior point: the auxiliary problem of the batch)
    return fb, res


def test_every_cut_of_a_whole_solve_keeps_the_planted_optimum(batch16, solved16):
    insts = batch16[0]
    fb, res = solved16
    assert res[0]["ecp_blocks_launches"] == 1 and res[0]["ecp_blocks_fallbacks"] == 0, res[0]
    assert fb.m.stat("esh_interior_found") == 1 and res[0]["ecp_blocks_esh_rows"] > 0
    for b, (r, inst) in enumerate(zip(res, insts)):
        assert r["status"] == "Optimal"
        assert_planted_objective(r["objval"], inst)
        c = fb.m.blocks_cuts(b)
        rp, col = c["rowptr"], c["col"] - int(fb.offs[b])
        ax = np.array([c["val"][rp[k]:rp[k + 1]] @ inst.xhat[col[rp[k]:rp[k + 1]]] for k in range(len(c["hi"]))])
        scale = 1.0 + np.abs(c["hi"])
        assert len(ax) > 0 and np.all(ax <= c["hi"] + 1e-9 * scale), (b, float(np.max((ax - c["hi"]) / scale)))
        assert np.all((c["lam"] > 0) & (c["lam"] <= 1.0))


def test_rounds_against_the_kelley_device_loop(batch16, solved16):
    """The yardstick is the Kelley device loop of the same build.  First MI355X run, per-instance rounds Kelley -> supporting
    hyperplanes (the engine's own interior point), explog seeds 0-7 then quad seeds 0-7:
        6->6 11->5 12->6 10->7 7->7 12->7 10->5 6->4      11->6 14->8 10->8 9->7 9->7 15->9 5->7 11->8
    sums 158 -> 107, PDHG iterations 20 464 -> 9 077 (DESIGN.md section 11 "In the device-side loop").  The sum is asserted; one
    instance goes the other way -- quad seed 6, 5 -> 7 rounds -- so per instance the bound is twice Kelley's rounds, the rule of
    test_gpu_supporting_hyperplanes._assert_rounds."""
    insts, rk, resk = batch16
    fb, res = solved16
    rese = fb.m.blocks_results()
    rounds_k, rounds_e = resk[:, 1].astype(int), rese[:, 1].astype(int)
    print("rounds kelley -> supporting:", " ".join("%d->%d" % (a, b) for a, b in zip(rounds_k, rounds_e)))
    print("pdhg kelley %d supporting %d" % (resk[:, 4].sum(), rese[:, 4].sum()))
    more = [b for b in range(16) if rounds_e[b] > rounds_k[b]]
    assert np.all(rounds_e <= 2 * rounds_k), (rounds_k, rounds_e)
    assert set(more) <= MORE_ROUNDS, more
    assert rounds_e.sum() <= rounds_k.sum(), (rounds_k.sum(), rounds_e.sum())


def test_the_engines_own_interior_point(batch1):
    insts, _ = batch1
    fb = FusedBatch(solver(ESH), insts)
    res = fb.solve()
    assert fb.m.stat("esh_interior_found") == 1 and fb.m.stat("ecp_blocks_launches") == 1
    for r, inst in zip(res, insts):
        assert r["status"] == "Optimal"
        tol = max(1e-6, 1e-6 * max(abs(r["objval"]), abs(inst.opt_obj)))
        assert abs(r["objval"] - inst.opt_obj) <= tol, (r["objval"], inst.opt_obj)


def test_no_interior_point_launches_kelleys_kernel():
    """the docs' cone rows: the engine's search finds no point (its LP leaves x = y = 0, where the cone has no finite gradient)"""
    items = []
    for s in range(4):
        n, d, lv, uv, lb, ub = _cone_family(8, 0, seed=s)
        items.append(ktn.Problem(n, len(lb), lv, uv, lb, ub, "Min", d))
    out = []
    for algo in (ESH, "kelley"):
        fb = FusedBatch(solver(algo), items)
        res = fb.solve()
        out.append((fb, res, fb.m.getsolution(), fb.m.blocks_results()))
    (fe, re_, xe, be), (fk, rk, xk, bk) = out
    assert fe.m.interior_point() is None and fe.m.stat("esh_interior_found") == 0
    assert fe.m.stat("ecp_blocks_launches") == 1 and re_[0]["ecp_blocks_esh_rows"] == 0
    assert np.array_equal(xe, xk) and np.array_equal(be, bk)
    for a, b in zip(re_, rk):
        assert a["status"] == b["status"] and a["objval"] == b["objval"]
    for blk in range(4):
        ce, ck = fe.m.blocks_cuts(blk), fk.m.blocks_cuts(blk)
        assert np.all(ce["lam"] == 1.0) and len(ce["lam"]) > 0
        for key in ce:
            assert np.array_equal(ce[key], ck[key]), (blk, key)


def test_flags():
    insts = [make(n=200, m_nl=20, k=8, family="explog", seed=20 + s) for s in range(4)]
    out = []
    for ex in (False, True):
        fb = FusedBatch(solver(), insts)
        m = fb.m
        with pytest.raises(L.KatanaHipError) as e:
            m.blocks_cuts(0)
        assert e.value.code == L.E_INVALID
        with pytest.raises(L.KatanaHipError) as e:
            m.blocks_results()
        assert e.value.code == L.E_INVALID
        st = STATUS[L.check(m._h, m._lib.ktn_optimize_blocks_ex(m._h, 0, 0))] if ex else m.optimize_blocks()
        out.append((st, m.getobjval(), m.numiters(), m.numcuts(), m.getsolution(),
                    {k: m.stat(k) for k in ("ecp_blocks_launches", "ecp_blocks_fallbacks", "ecp_blocks_pdhg_sum", "ecp_blocks_rows",
                                            "ecp_blocks_esh_rows", "esh_rows", "pdhg_iters")}))
    a, b = out
    assert a[0] == b[0] == "Optimal" and a[1] == b[1] and a[2:4] == b[2:4] and np.array_equal(a[4], b[4]) and a[5] == b[5], (a[5], b[5])
    # arenas that overflow: room for one cut per NL row on smooth models
    smooth = [sc.convex_instance(900 + s) for s in range(8)]
    fb = FusedBatch(solver(), smooth)
    st = fb.m.optimize_blocks(1, fallback=False)
    assert st != "Optimal"
    assert fb.m.stat("ecp_blocks_launches") == 1 and fb.m.stat("ecp_blocks_fallbacks") == 0
    res = fb.m.blocks_results()
    assert np.any(res[:, 7] == 1) and st == STATUS[int(res[res[:, 0] != L.STATUS_OPTIMAL][0, 0])]
    # a supporting-hyperplane handle without the flag is refused, as by ktn_optimize_blocks
    fe = FusedBatch(solver(ESH), insts)
    for call in (lambda: fe.m.optimize_blocks(), lambda: fe.m.optimize_blocks(fallback=False)):
        with pytest.raises(L.KatanaHipError) as e:
            call()
        assert e.value.code == L.E_UNSUPPORTED


STATUS = ktn.solver.STATUS_SYMBOLS
MORE_ROUNDS = {14}                     # batch16[14] = quad seed 6: 5 -> 7 rounds on the first MI355X run
