"""GPU tier: constraint duals, reduced costs and the dual bound of a solved NLP (ktn_get_constr_duals / ktn_get_reduced_costs /
ktn_get_dual_bound, csrc/kkt.hpp) against tests/kkt_ref.py, which tests/test_kkt_ref.py pins on the CPU.

Measured on an MI355X (printed by the tests with -s, recorded in profiles/kkt_planted.txt; measured, not guaranteed): see the
docstring of test_validity_on_the_planted_family_with_the_first_order_lp."""
import ctypes as C

import numpy as np
import pytest

import katana_jl_amd as ktn
from katana_jl_amd import _lib as L
from katana_jl_amd.batch import FusedBatch
from helpers import hip_load_instance
import kkt_cases
import kkt_ref

pytestmark = pytest.mark.gpu

EXACT = dict(lp_dense_after=-1)


def report(m):
    """(d, z, bound, gap) and the number of evaluations they cost"""
    e0 = m.stat("kkt_evals")
    d, z, lb, gap = m.getconstrduals(), m.getreducedcosts(), m.getobjbound(), m.getobjgap()
    return d, z, lb, gap, m.stat("kkt_evals") - e0


def refused(call, code):
    with pytest.raises(L.KatanaHipError) as e:
        call()
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


# ---- 1. aggregation is exactly the sum over the lists ----------------------------------------------------------------------
def small_model():
    """6 variables, 2 linear rows, 3 NL rows"""
    A = kkt_cases
    Q, LIN, inf = A.ATOM_QUAD, A.ATOM_LIN, np.inf
    rows = [([(4, LIN, 1.0, 0.0), (5, LIN, 1.0, 0.0)], 0.0, -inf, 1.0),
            ([(0, LIN, 1.0, 0.0), (5, LIN, 1.0, 0.0)], 0.0, -10.0, inf),
            ([(0, Q, 1.0, 0.0), (1, Q, 1.0, 0.0)], -4.0, -inf, 0.0),
            ([(2, Q, 1.0, 0.0), (3, Q, 1.0, 0.0)], -4.0, -inf, 0.0),
            ([(4, Q, 1.0, 0.0), (5, Q, 1.0, 0.0)], -9.0, -inf, 0.0)]
    obj = [(0, LIN, -2.0, 0.0), (1, LIN, -1.0, 0.0), (2, LIN, -1.0, 0.0), (3, LIN, -1.0, 0.0), (4, LIN, -1.0, 0.0), (5, LIN, -1.5, 0.0)]
    return A._inst(6, "Min", [-3.0] * 6, [3.0] * 6, rows, obj)


def test_aggregation_is_the_sum_over_the_lists():
    inst = small_model()
    m = hip_load_instance(ktn, inst, **EXACT)
    m.lp_enable_global_lists(3)
    refused(m.getconstrduals, L.E_INVALID)                       # no LP solve yet
    inf = np.inf
    # hand-made cuts: three for NL row 0 (two active at the LP optimum, one slack), one for NL row 1, none for NL row 2
    # (an append links at most one cut per NL row -- k_append_link --, as a sweep produces them: one call per cut of row 0)
    m.lp_append_rows([0, 2], [0, 1], [1.0, 1.0], [-inf], [1.0], nl_id=[0])
    m.lp_append_rows([0, 2], [0, 1], [1.0, -1.0], [-inf], [0.2], nl_id=[0])
    m.lp_append_rows([0, 1, 3], [0, 2, 3], [1.0, 1.0, 1.0], [-inf] * 2, [2.5, 1.0], nl_id=[0, 1])
    ids = np.asarray([-1, -1, 0, 0, 0, 1])

    def check(ids):
        st, _ = m.lp_solve()
        assert st == "Optimal"
        y = m.lp_duals()
        assert len(y) == len(ids) and np.count_nonzero(y) >= 3
        d, z, lb, gap, evals = report(m)
        assert evals == 1
        want = kkt_ref.aggregate(y, ids, 3)
        assert d[:2].tobytes() == y[:2].tobytes(), (d[:2], y[:2])
        assert d[2:].tobytes() == want.tobytes(), (d[2:], want)
        return d

    d = check(ids)
    assert d[2] < 0 and d[3] < 0 and d[4] == 0.0
    assert m.lp_purge() == 0                                       # nothing to drop, but the caller touched the rows
    refused(m.getconstrduals, L.E_INVALID)
    check(ids)
    m.lp_truncate(m.lp_num_rows() - 1)                             # NL row 1 loses its only cut
    msg = refused(m.getreducedcosts, L.E_INVALID)
    assert "no LP solve" in msg
    refused(m.getobjbound, L.E_INVALID)
    d = check(ids[:-1])
    assert d[3] == 0.0


# ---- 2. k_lagr_grad against the reference ----------------------------------------------------------------------------------
GROUPS = (0, 4, 8, 16, 32, 64)


@pytest.fixture(scope="module")
def planted300():
    return {fam: ktn.instances.make_instance(n=300, m_nl=40 if fam == "explog" else 600, k=8, m_lin=100, family=fam)
            for fam in ("explog", "explog+t")}


def check_against_sep_ref(inst, m, what):
    x = m.getsolution()[:inst.n]
    d, z, lb, gap, evals = report(m)
    assert evals == 1, what
    R = kkt_ref.kkt_sep(inst, x, d)
    bad = ~(np.abs(z - R.z) <= 2 * R.e_z)
    assert not bad.any(), (what, np.flatnonzero(bad)[:5], z[bad][:5], R.z[bad][:5], R.e_z[bad][:5])
    assert abs(lb - R.LB) <= 2 * R.e_LB and abs(gap - R.gap) <= 2 * R.e_LB, (what, lb, R.LB, gap, R.gap, R.e_LB)
    d2, z2, lb2, gap2, evals2 = report(m)                          # cached: the same bits, no further evaluation
    assert evals2 == 0 and d2.tobytes() == d.tobytes() and z2.tobytes() == z.tobytes() and (lb2, gap2) == (lb, gap), what
    return x, d, z, lb, gap, R


@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("fam", ("explog", "explog+t"))
def test_lagr_grad_against_the_reference(planted300, monkeypatch, fam, G):
    inst = planted300[fam]
    if G:
        monkeypatch.setenv("KTN_KKT_GROUP", str(G))
    m = hip_load_instance(ktn, inst)
    assert m.optimize() == "Optimal"
    x, d, z, lb, gap, R = check_against_sep_ref(inst, m, (fam, G))
    assert m.stat("kkt_group") == (G if G else m.stat("kkt_group")) and m.stat("kkt_group") in (4, 8, 16, 32, 64)
    lens = np.bincount(inst.col, minlength=inst.n)
    assert (lens == 0).any() or fam == "explog+t"                   # columns that appear in no row ...
    if fam == "explog+t":
        assert lens[-1] == 600 > 64 * 8                             # ... and one that makes more than eight trips at every G
    assert lb <= inst.opt_obj + R.e_LB + 1e-12 * (1.0 + abs(inst.opt_obj)), (lb, inst.opt_obj, R.e_LB)
    # a second REAL evaluation on unchanged inputs: the same solve again from the loaded state (the engine's solve is
    # deterministic), whose report must come out of the kernels with the same bits
    m.reset()
    assert m.optimize() == "Optimal" and m.getsolution()[:inst.n].tobytes() == x.tobytes()
    d3, z3, lb3, gap3, ev = report(m)
    assert ev == 1
    assert d3.tobytes() == d.tobytes() and z3.tobytes() == z.tobytes() and (lb3, gap3) == (lb, gap)


def other_kind_models():
    """name -> (Problem, exact-reference description, optimum or None).  The QUAD and TAPE models are the ellipsoid of
    tests/quad_cases.py (a dense symmetric Q: off-diagonal segments of 8 entries); one more TAPE model with exp / log nodes and the
    HOST model are a planted instance, whose reference description is the separable statement itself."""
    import quad_cases as QC
    E = QC.ellipsoid(8)
    inst = ktn.instances.make_instance(n=40, m_nl=6, k=4, m_lin=12, family="explog", seed=3)
    prob = lambda kind: ktn.Problem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr, inst.u_constr, inst.sense,
                                    kkt_cases.description(ktn, inst, kind))
    pq, pt, pe = QC.ellipsoid_quad(E), QC.ellipsoid_tape(E), prob("tape")
    return {"quad": (pq, pq.d, E.fstar), "tape": (pt, pt.d, E.fstar), "tape_explog": (pe, pe.d, inst.opt_obj),
            "host": (prob("host"), ktn.SeparableNLP(inst), inst.opt_obj)}


@pytest.fixture(scope="module")
def other_kinds():
    return other_kind_models()


@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("kind", ("quad", "tape", "tape_explog", "host"))
def test_lagr_grad_on_the_other_row_kinds(other_kinds, monkeypatch, kind, G):
    """TAPE, KTN_ROW_QUAD and HOST rows against the description-driven reference (kkt_ref.kkt_desc: the rows through tape_ref /
    quad_ref / sep_ref in mpmath, independent of the engine), at every lane-group width: z, bound and gap within the derived
    bound of the exact values, and the bound below the known optimum.  A precompute made BEFORE the report must survive it:
    the report evaluates into buffers of its own."""
    p, ref_d, fstar = other_kinds[kind]
    if G:
        monkeypatch.setenv("KTN_KKT_GROUP", str(G))
    m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, **(EXACT if kind in ("quad", "tape") else {})))
    m.loadproblem(*p)
    assert m.optimize() == "Optimal"
    sep = ktn.KatanaHipSeparator(m)
    sep.initialize()
    x0 = np.zeros(m.num_var); x0[:p.num_var] = 0.25
    sep.precompute(x0)
    g0, j0 = sep.g.copy(), sep.jac.copy()
    x = m.getsolution()
    d, z, lb, gap, evals = report(m)
    assert evals == 1 and (not G or m.stat("kkt_group") == G)
    g1, j1 = np.zeros_like(g0), np.zeros_like(j0)
    L.check(m._h, m._lib.ktn_sep_get_g(m._h, g1.ctypes.data_as(C.POINTER(C.c_double)), len(g1)))
    L.check(m._h, m._lib.ktn_sep_get_jac(m._h, j1.ctypes.data_as(C.POINTER(C.c_double)), len(j1)))
    assert g1.tobytes() == g0.tobytes() and j1.tobytes() == j0.tobytes()
    R = kkt_ref.kkt_desc(ref_d, p.l_constr, p.u_constr, p.l_var, p.u_var, p.sense, x, d)
    kkt_ref.check_device(R, z, lb, gap, (kind, G))
    assert np.count_nonzero(d) >= 1 and np.isfinite(lb)
    assert lb <= fstar + float(R.e_LB) + 1e-12 * (1.0 + abs(fstar)), (lb, fstar, float(R.e_LB))


def test_report_after_a_solve_that_purged():
    """the loop's own purge (rows compacted with their multipliers, lists relinked) and appends do not void the report: after an
    optimize! in which cuts were purged the getters answer, agree with the reference at the returned (x, d) and give a valid bound"""
    inst = ktn.instances.make_instance(n=300, m_nl=40, k=8, m_lin=100, family="explog", bound_frac=0.5)
    # (purging from the first cut on, with no minimum share, slows this solve to thousands of rounds: the first 60 are enough --
    #  the report is defined after any LP solve, and the round that hits the cap ends like any other: solve, purge, sweep, append)
    m = hip_load_instance(ktn, inst, purge_min_rows=1, purge_min_frac=0.0, iter_cap=60)
    status = m.optimize()
    x, d, z, lb, gap, R = check_against_sep_ref(inst, m, "purged")
    print("purged solve: status %s iters %d purges %d rows purged %d  LB %.12g opt %.12g gap %.3e"
          % (status, m.numiters(), m.stat("purges"), m.stat("purged_rows"), lb, inst.opt_obj, gap))
    assert m.stat("purges") > 0 and m.stat("purged_rows") > 0
    assert np.all(d <= 0.0) and np.isfinite(lb)
    assert lb <= inst.opt_obj + R.e_LB + 1e-12 * (1.0 + abs(inst.opt_obj)), (lb, inst.opt_obj)


# ---- 3. closed forms with the exact LP ---------------------------------------------------------------------------------------
CLOSED = [(name, n, kind) for name in kkt_cases.NAMES for n in kkt_cases.NS for kind in kkt_cases.KINDS] + [("a", n, "host") for n in kkt_cases.NS]


@pytest.fixture(scope="module")
def closed_cases():
    return {(name, n): kkt_cases.build(name, n) for name in kkt_cases.NAMES for n in kkt_cases.NS}


@pytest.mark.parametrize("name,n,kind", CLOSED, ids=lambda v: str(v))
def test_closed_forms_with_the_exact_lp(closed_cases, name, n, kind):
    """|d - d*| <= 1e-2 max(1, |d*|), |z - z*| <= 1e-2 max(1, |z*|_inf, |d*|_inf): a cut with a non-zero multiplier is active at
    the LP point x^; for g = |x|^2 - 1 a cut taken at x_k is active at x^ iff |x_k - x^|^2 = |x^|^2 - 1 <= f_tol, so
    |x_k - x^| <= 1e-3; grad g is 2-Lipschitz and stationarity is linear in the multipliers, so the aggregated multiplier is exact
    to first order in 1e-3 / min_j |x*_j|, and min_j |x*_j| >= 0.1 in these cases."""
    Cs = closed_cases[(name, n)]
    m = kkt_cases.load(ktn, Cs.inst, kind, **EXACT)
    assert m.optimize() == "Optimal"
    d, z, lb, gap, evals = report(m)
    print("closed form %s n=%d %s: iters %d  max|d-d*| %.3e  max|z-z*| %.3e  bound %.12g (f* %.12g)  gap %.3e  epi %r"
          % (name, n, kind, m.numiters(), np.max(np.abs(d - Cs.ds)), np.max(np.abs(z - Cs.zs)), lb, Cs.fstar, gap, m.stat("kkt_epi_dual")))
    assert evals == 1
    assert np.all(np.abs(d - Cs.ds) <= 1e-2 * np.maximum(1.0, np.abs(Cs.ds))), (d, Cs.ds)
    assert np.all(np.abs(z - Cs.zs) <= 1e-2 * max(1.0, np.max(np.abs(Cs.zs)), np.max(np.abs(Cs.ds)))), (z, Cs.zs)
    if Cs.inst.sense == "Min":
        assert lb <= Cs.fstar + 1e-9
    else:
        assert lb >= Cs.fstar - 1e-9                               # an upper bound
    assert gap >= -1e-9
    if name == "f":                                                # the negatives of case (a)'s
        A = closed_cases[("a", n)]
        assert np.all(np.abs(d + A.ds) <= 1e-2 * np.maximum(1.0, np.abs(A.ds))) and np.all(np.abs(z + A.zs) <= 1e-2 * max(1.0, np.max(np.abs(A.ds))))
    if name == "e":
        assert abs(abs(m.stat("kkt_epi_dual")) - 1.0) <= 1e-9
    else:
        assert np.isnan(m.stat("kkt_epi_dual"))


# ---- 4. validity on the planted family with the first-order LP ---------------------------------------------------------------
@pytest.mark.parametrize("bf", (1.0, 0.5))
@pytest.mark.parametrize("fam", ("quad", "explog"))
def test_validity_on_the_planted_family_with_the_first_order_lp(fam, bf):
    """Default LP schedule.  Asserted: the signs (every row is a `<=` row: d <= 0 exactly), LB <= opt_obj within the reference's
    roundoff bound, LB / gap / z equal to the reference at the returned (x, d) within roundoff, LB finite.  NOT asserted -- nothing
    predicts them for a first-order LP -- and only printed: the size of the gap and the distance of d to the planted multipliers.
    Values read on an MI355X are recorded in DESIGN.md section 12 and profiles/kkt_planted.txt."""
    inst = ktn.instances.make_instance(n=300, m_nl=40, k=8, m_lin=100, family=fam, bound_frac=bf)
    m = hip_load_instance(ktn, inst)
    status = m.optimize()                                          # (recorded, not asserted: the report is defined after ANY LP solve)
    x, d, z, lb, gap, R = check_against_sep_ref(inst, m, (fam, bf))
    planted = -np.concatenate([inst.mu, inst.lam])
    print("planted %s bound_frac %g: status %s code %d iters %d  obj %.12g opt %.12g  LB %.12g  gap %.3e  max|d - planted| %.3e  max|z - nu| %.3e"
          % (fam, bf, status, m._lib.ktn_get_status(m._h), m.numiters(), m.getobjval(), inst.opt_obj, lb, gap, np.max(np.abs(d - planted)),
             np.max(np.abs(z - inst.nu))))
    assert np.all(d <= 0.0), d[d > 0]
    assert np.isfinite(lb)
    assert lb <= inst.opt_obj + R.e_LB + 1e-12 * (1.0 + abs(inst.opt_obj)), (lb, inst.opt_obj)


# ---- 5. throughput mode ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch16():
    return [ktn.instances.make_instance(n=40, m_nl=6, k=4, m_lin=12, seed=s) for s in range(16)]


def check_batch_against_ref(fb, insts, x):
    dd, zz, bb = fb.constr_duals(), fb.reduced_costs(), fb.dual_bounds()
    assert len(dd) == len(zz) == len(bb) == len(insts)
    for i, inst in enumerate(insts):
        xi = x[int(fb.offs[i]):int(fb.offs[i + 1])]
        assert len(dd[i]) == inst.num_constr and len(zz[i]) == inst.n
        R = kkt_ref.kkt_sep(inst, xi, dd[i])
        assert np.all(np.abs(zz[i] - R.z) <= 2 * R.e_z), (i, np.max(np.abs(zz[i] - R.z)))
        lb, gap = bb[i]
        npos = int(np.count_nonzero(dd[i] > 0.0))
        print("instance %d: bound %.12g (opt %.12g) gap %.3e  multipliers of the wrong side: %d %r" % (i, lb, inst.opt_obj, gap, npos, dd[i][dd[i] > 0.0][:3]))
        if np.isfinite(R.LB):
            assert abs(lb - R.LB) <= 2 * R.e_LB and abs(gap - R.gap) <= 2 * R.e_LB, (i, lb, R.LB, gap, R.gap, R.e_LB)
            assert lb <= inst.opt_obj + R.e_LB + 1e-12 * (1.0 + abs(inst.opt_obj)), (i, lb, inst.opt_obj)
        else:
            # a multiplier on the infinite side of a row (every row here is a `<=` row): the bound is -inf by definition, in the
            # reference as on the device -- trivially valid; what is compared is that both say so
            assert npos > 0 and lb == R.LB and gap == R.gap, (i, lb, R.LB, gap, R.gap)
    return dd


def test_throughput_mode_device_loop(batch16):
    fb = FusedBatch(ktn.KatanaSolver(log_level=0, lp_max_iter=400000), batch16, False, True)
    res = fb.solve(cut_capacity=128)
    br = fb.m.blocks_results()
    assert res[0]["ecp_blocks_launches"] == 1 and res[0]["ecp_blocks_fallbacks"] == 0
    assert np.all(br[:, 0] == L.STATUS_OPTIMAL) and np.all(br[:, 7] == 0)          # the device loop ended every instance
    dd = check_batch_against_ref(fb, batch16, fb.m.getsolution())
    nl0 = 0
    for i, inst in enumerate(batch16):
        cuts, y = fb.m.blocks_cuts(i), fb.m.blocks_duals(i)
        assert len(y) == len(cuts["slot"])
        want = kkt_ref.aggregate(y, cuts["slot"] - nl0, inst.m_nl)
        assert dd[i][inst.m_lin:].tobytes() == want.tobytes(), (i, dd[i][inst.m_lin:], want)
        nl0 += inst.m_nl
    assert fb.m.stat("kkt_evals") == 1


def test_throughput_mode_host_loop(batch16):
    fb = FusedBatch(ktn.KatanaSolver(log_level=0), batch16, False, False)
    m = fb.m
    base = m.lp_num_rows()
    slots = []
    m.optimize_begin()
    done = False
    while not done:
        done = m.ecp_step()
        slots.extend(m.last_sweep_slots().tolist())
    assert m.optimize_end() == "Optimal" and m.stat("purges") == 0
    assert m.lp_num_rows() == base + len(slots)
    y = m.lp_duals()
    dd = check_batch_against_ref(fb, batch16, m.getsolution())
    want = kkt_ref.aggregate(y[base:], np.asarray(slots), sum(i.m_nl for i in batch16))
    lin0 = nl0 = 0
    for i, inst in enumerate(batch16):
        assert dd[i][:inst.m_lin].tobytes() == y[lin0:lin0 + inst.m_lin].tobytes()
        assert dd[i][inst.m_lin:].tobytes() == want[nl0:nl0 + inst.m_nl].tobytes()
        lin0 += inst.m_lin; nl0 += inst.m_nl


def test_throughput_mode_quadratic_objectives(closed_cases):
    """a batch of Problems with a quadratic objective each (case (e)): fusion gives every instance an epigraph row and variable
    of its own, which the per-instance output must not show"""
    cs = [closed_cases[("e", n)] for n in (4, 8, 4, 8)]
    probs = [ktn.Problem(c.inst.n, c.inst.num_constr, c.inst.l_var, c.inst.u_var, c.inst.l_constr, c.inst.u_constr, c.inst.sense,
                         kkt_cases.quad_description(ktn, c.inst)) for c in cs]
    fb = FusedBatch(ktn.KatanaSolver(log_level=0, **EXACT), probs, False, True)
    res = fb.solve(cut_capacity=128)
    dd, zz, bb = fb.constr_duals(), fb.reduced_costs(), fb.dual_bounds()
    for c, r, d, z, (lb, gap) in zip(cs, res, dd, zz, bb):
        assert r["status"] == "Optimal" and len(d) == c.inst.num_constr and len(z) == c.inst.n and len(r["x"]) == c.inst.n
        print("fused (e) n=%d: d %r (d* %r)  bound %.9g (f* %.9g) gap %.3e" % (c.n, d, c.ds, lb, c.fstar, gap))
        assert lb <= c.fstar + 1e-9 and gap >= -1e-9 and np.isfinite(lb)
        assert np.all(d <= 0.0)


# ---- 6. refused paths --------------------------------------------------------------------------------------------------------
def test_refused_paths(closed_cases):
    inst = closed_cases[("c", 4)].inst
    m = hip_load_instance(ktn, inst, **EXACT)
    for call in (m.getconstrduals, m.getreducedcosts, m.getobjbound):
        assert "no LP solve" in refused(call, L.E_INVALID)                 # before any solve
    assert m.optimize() == "Optimal"
    small = np.zeros(1)
    p = small.ctypes.data_as(C.POINTER(C.c_double))
    assert m._lib.ktn_get_constr_duals(m._h, p, inst.num_constr - 1) == L.E_INVALID
    assert m._lib.ktn_get_reduced_costs(m._h, p, inst.n - 1) == L.E_INVALID
    assert m.stat("kkt_evals") == 0
    d = m.getconstrduals()
    m.reset()
    refused(m.getconstrduals, L.E_INVALID)                                 # ktn_reset drops the report
    assert m.optimize() == "Optimal" and m.getconstrduals().tobytes() == d.tobytes()
    # a handle that is part of a row-sharded LP (world 1 is enough to set the mode) ...
    ms = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0, **EXACT))
    ar = L.ALLREDUCE_CB(lambda *a: 0)
    L.check(ms._h, ms._lib.ktn_dist_init_callback(ms._h, 0, 1, C.cast(ar, C.c_void_p), None))
    ms.loadproblem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr, inst.u_constr, inst.sense, ktn.SeparableNLP(inst))
    assert ms.optimize() == "Optimal"
    for call in (ms.getconstrduals, ms.getreducedcosts, ms.getobjbound):
        refused(call, L.E_UNSUPPORTED)
    # ... or one with a cut exchange set
    mx = hip_load_instance(ktn, inst, **EXACT)
    mx.lp_enable_global_lists(inst.m_nl)
    cb = L.EXCHANGE_CB(lambda *a: 0)
    mx.set_cut_exchange(cb, 0)
    mx.lp_solve()
    refused(mx.getconstrduals, L.E_UNSUPPORTED)
    mx.set_cut_exchange(None, 0)
    assert len(mx.getconstrduals()) == inst.num_constr
