"""GPU tier: the per-instance LP of throughput mode -- k_pdhg_blocks (csrc/batch_lp.hpp) behind Engine::build_blocks and
Engine::lp_solve_blocks (csrc/lp.hip) -- against the exact-rational KKT certificate of tests/exact_lp_ref.py, block by block, on
the planted block-diagonal LPs of tests/blk_lp_cases.py.

Every feasible case is loaded on two fresh handles; the first gets set_blocks, the second runs the ordinary launch-per-step loop
(the reference implementation: tests/test_gpu_lp_kernels.py, test_gpu_lp_matches_highs).  Both are solved with
lp_solve(1e-8, 1e-8) and judged per block -- a sum over blocks would hide a bad small block behind a large one -- by the bar the
project asserts for its first-order path (test_gpu_exact_lp.py, the mid_free8 test): status Optimal, rows to 1e-7, bounds to 1e-12,
sign-feasible multipliers, |gap| and the charge of reduced costs on missing bounds within 1e-6 max(1, |pobj_b|), the block's
objective within the same of the planted one.  The ordinary handle is asserted first: the block path is not judged while its
reference fails, and never by its own check sums.

Measured on an MI355X (iterations: largest block of the one launch / sum over the blocks / the ordinary loop on the whole LP):
see DESIGN.md section 3, "The per-instance LP against exact certificates"."""
import functools

import numpy as np
import pytest

import blk_lp_cases as bc
import katana_jl_amd as ktn
from exact_lp_cases import highs_solve
from exact_lp_ref import certify
from helpers import assert_planted_objective, max_nl_violation

pytestmark = pytest.mark.gpu

TOL = 1e-8
ROW_BAR, BOUND_BAR, REL_BAR = 1e-7, 1e-12, 1e-6
# a solve that does not get there ends as a failed assertion, not as ten million iterations inside one launch
MAX_ITER = 400000


def planted_objectives(case):
    s = -1.0 if case.sense == "Max" else 1.0
    return [s * float(case.c[case.offsets[b]:case.offsets[b + 1]] @ case.x[case.offsets[b]:case.offsets[b + 1]]) for b in range(case.nblocks)]


def block_bar(case, x, y, want, label, rows=None):
    """certify every block on its own rows and columns; prints every figure, returns what misses the bar as a list of strings"""
    bad = []
    for b in range(case.nblocks):
        sub, idx = bc.block_lp(case, b, rows)
        c0, c1 = int(case.offsets[b]), int(case.offsets[b + 1])
        cert = certify(sub.csr(), sub.lo, sub.hi, sub.l, sub.u, sub.c, sub.sense, x[c0:c1], y[idx])
        scale = max(1.0, abs(want[b]))
        print("%s %s block %d n %d m %d: row_viol %.3e bound_viol %.3e sign_ok %s gap %.3e charge %.3e pobj %.12g planted %.12g (scale %.3g)"
              % (case.name, label, b, sub.n, sub.m, cert.row_viol, cert.bound_viol, cert.sign_ok, cert.gap, cert.charge, cert.pobj, want[b], scale))
        miss = []
        if not cert.row_viol <= ROW_BAR: miss.append("row %d violated by %.3e" % (cert.worst_row, cert.row_viol))
        if not cert.bound_viol <= BOUND_BAR: miss.append("column %d outside its bound by %.3e" % (cert.worst_col, cert.bound_viol))
        if not cert.sign_ok: miss.append("multiplier of row %d points at an absent side" % cert.bad_sign_row)
        if not abs(cert.gap) <= REL_BAR * scale: miss.append("gap %.3e" % cert.gap)
        if not cert.charge <= REL_BAR * scale: miss.append("charge %.3e (column %d)" % (cert.charge, cert.worst_rc_col))
        if not abs(cert.pobj - want[b]) <= REL_BAR * scale: miss.append("objective %.12g, planted %.12g" % (cert.pobj, want[b]))
        bad += ["%s block %d: %s" % (label, b, s) for s in miss]
    return bad


def solve(case, blocks, **kw):
    m = bc.load(ktn, case, blocks, **dict(dict(lp_max_iter=MAX_ITER), **kw))
    st, it = m.lp_solve(TOL, TOL)
    return m, st, it


def no_exact_solver(m):
    return m.stat("dense_lp_solves") == 0 and m.stat("mid_lp_solves") == 0


@functools.lru_cache(maxsize=None)
def reference(name, mixed):
    """the ordinary loop on the case: (status, x, y, pdhg_iters, lp_cold_restarts), solved once per session"""
    case = bc.case(name, mixed)
    m, st, it = solve(case, False)
    assert no_exact_solver(m) and m.stat("blk_lp_launches") == 0
    return st, m.getsolution(), m.lp_duals(), m.stat("pdhg_iters"), m.stat("lp_cold_restarts")


def both_meet_the_bar(name, mixed, launches=1):
    """the method of the module docstring; returns the block handle"""
    case = bc.case(name, mixed)
    want = planted_objectives(case)
    st_ref, x_ref, y_ref, it_ref, _ = reference(name, mixed)
    m, st, it = solve(case, True)
    print("%s %s: status %s (ordinary loop: %s), iterations of the one launch max %d sum %d, ordinary loop %d, ratio max / ordinary %.2f"
          % (name, "mixed" if mixed else "blockwise", st, st_ref, m.stat("blk_pdhg_iters_max"), m.stat("blk_pdhg_iters_sum"), it_ref,
             m.stat("blk_pdhg_iters_max") / max(it_ref, 1.0)))
    bad_ref = block_bar(case, x_ref, y_ref, want, "ordinary")
    bad = block_bar(case, m.getsolution(), m.lp_duals(), want, "blocks")
    assert st_ref == "Optimal" and bad_ref == [], (st_ref, bad_ref)          # the reference first
    assert st == "Optimal" and bad == [], (st, bad)
    assert no_exact_solver(m)
    assert m.stat("blk_lp_launches") == launches
    if launches:
        assert m.stat("blk_lp_fallbacks") == 0 and m.stat("blk_pdhg_iters_max") > 0 and m.stat("pdhg_iters") == m.stat("blk_pdhg_iters_max")
    return m


@pytest.mark.parametrize("mixed", bc.ORDERS, ids=("mixed", "blockwise"))
@pytest.mark.parametrize("name", ["edges", "two_trips", "ranges", "empties", "empties_rowless_first", "max_sense", "one_block"])
def test_block_lp_meets_the_bar_per_block(name, mixed):
    """both row orders: the mixed one runs k_row_block and the stable sort on interleaved keys.  k_block_rows reads the SORTED keys,
    so it meets a skipped block (prevb + 1 < b) only where a block owns no rows, whatever the stored order: the two `empties` cases,
    which also have the trailing empty block; `empties_rowless_first` has no row without entries, so its empty first block owns
    none and the fill starts from prevb = -1 with a first key above 0"""
    both_meet_the_bar(name, mixed)


def test_runaway_free_columns_restart_cold():
    """the ordinary loop on `edges`: the 8-pass power iteration under-estimates sigma_max (0.92), the residual grows check after
    check, and the free columns -- every fifth -- keep what they picked up (|x| 1e13 after 65 iterations, objective 4e13 after
    400 000 before the cold restart was built).  The solve now starts again from the point of the box nearest to 0 with the safe
    step; test_block_lp_meets_the_bar_per_block asserts the bar on the answer"""
    st, _, _, it, cold = reference("edges", True)
    print("edges, ordinary loop:", st, it, "iterations, cold restarts", cold)
    assert st == "Optimal" and cold >= 1 and it < 20000


def test_x_step_trips_agree_under_a_shift_of_the_local_index():
    """`shifted` under the offsets [0, 1 025] and under [0, 1, 1 025]: column 0 has no rows, cost 0 and l = u = 0, so it adds 0 to
    every sum and the arithmetic of every other column is the same; only the local index of the last column moves from the x-step's
    second trip (1 024) into its first (1 023).  The check iterations update every column with loops of their own, so a plain step
    that skips outputs of a trip still ends at a KKT point and passes the bar; it cannot keep this agreement.  The two launches
    take their decisions from sums of 1 025 terms added in another order (n u = 1e-13 relative), which reach the iterates through
    the primal weight alone, at the restarts -- some 30 of them -- and from there through steps whose lengths add up to no more
    than 100 |z|: the same number of iterations, and answers within 30 * 1e-13 * 100 |z| < 1e-9 (1 + |z|)"""
    case = bc.case("shifted")
    out = []
    for offsets in ([0, case.n], case.offsets):
        m = bc.load(ktn, case, False, lp_max_iter=MAX_ITER)
        m.set_blocks(np.asarray(offsets, dtype=np.int64))
        st, _ = m.lp_solve(TOL, TOL)
        assert st == "Optimal" and m.stat("blk_lp_launches") == 1 and m.stat("blk_lp_fallbacks") == 0 and no_exact_solver(m)
        out.append((m.stat("blk_pdhg_iters_max"), m.getsolution(), m.lp_duals()))
    (it_a, x_a, y_a), (it_b, x_b, y_b) = out
    print("shifted: iterations", it_a, it_b, "max |dx|", np.max(np.abs(x_a - x_b)), "max |dy|", np.max(np.abs(y_a - y_b)))
    assert it_a == it_b
    assert np.max(np.abs(x_a - x_b) / (1.0 + np.abs(x_b))) <= 1e-9 and np.max(np.abs(y_a - y_b) / (1.0 + np.abs(y_b))) <= 1e-9
    assert block_bar(case, x_b, y_b, planted_objectives(case), "blocks") == []


@pytest.mark.parametrize("mixed", bc.ORDERS, ids=("mixed", "blockwise"))
def test_block_too_big_for_lds_is_answered_by_the_ordinary_loop(mixed):
    m = both_meet_the_bar("too_big", mixed, launches=0)
    assert m.stat("blk_lp_fallbacks") == 0 and m.stat("pdhg_iters") > 0


@pytest.mark.parametrize("mixed", bc.ORDERS, ids=("mixed", "blockwise"))
def test_long_row_bypasses_the_block_path(mixed):
    """lp_solve itself does not write `lp_long_rows`; ktn_lp_scaling does, from the same Engine::find_long_rows, on a handle with
    lp_ruiz_warm > 0.  The block path was not refused for its size: by the formula of Engine::lp_solve_blocks, (3 nmax + 3 mmax +
    (kBlkThreads / 64) kBlkQ + kBlkQ + 8) doubles + (mmax + 2) ints with kBlkThreads = 1 024 and kBlkQ = 12, the largest block needs
    78 KB of the 150 KB"""
    m = both_meet_the_bar("long_row", mixed, launches=0)
    case = bc.case("long_row", mixed)
    nmax, mmax = int(np.max(np.diff(case.offsets))), int(np.max(np.bincount(case.row_block)))
    assert (3 * nmax + 3 * mmax + 16 * 12 + 12 + 8) * 8 + (mmax + 2) * 4 < 0.6 * bc.LDS_LIMIT and m.stat("blk_lp_fallbacks") == 0
    third = bc.load(ktn, case, True, lp_ruiz_warm=2)
    third.lp_scaling()
    assert third.stat("lp_long_rows") >= 1


def test_block_lp_is_deterministic():
    """no atomics, every sum in a fixed order: two fresh handles agree bit for bit"""
    case = bc.case("edges")
    a, st_a, _ = solve(case, True)
    b, st_b, _ = solve(case, True)
    assert st_a == st_b == "Optimal" and a.stat("blk_lp_launches") == b.stat("blk_lp_launches") == 1
    assert a.stat("blk_pdhg_iters_sum") == b.stat("blk_pdhg_iters_sum") and no_exact_solver(a) and no_exact_solver(b)
    assert np.array_equal(a.getsolution(), b.getsolution()) and np.array_equal(a.lp_duals(), b.lp_duals())


def _resolve_with_cuts(case, blocks, touched):
    """solve, append two rows per touched block that cut the point found off, solve again on the same handle; returns the handle,
    the statuses, the rows and the per-block reference objectives of the grown LP (HiGHS on the touched blocks)"""
    m, st1, _ = solve(case, blocks)
    extra = bc.cut_rows(case, m.getsolution(), touched)
    m.lp_append_rows(*extra)
    st2, _ = m.lp_solve(TOL, TOL)
    rows = m.lp_rows()
    assert len(rows[3]) == case.m + 2 * len(touched)
    want = planted_objectives(case)
    s = -1.0 if case.sense == "Max" else 1.0
    for b in touched:
        sub, _ = bc.block_lp(case, b, rows)
        hs = highs_solve(sub)
        assert hs[0] == "Optimal"
        assert s * hs[1] > want[b] + 1e-3                                    # the cuts bite
        want[b] = s * hs[1]
    return m, st1, st2, rows, want


def test_warm_resolve_after_rows_are_appended_rebuilds_the_blocks():
    """the second solve starts from the first's (x, y) and primal weights (d_blkomega) and needs the block row lists rebuilt: the
    appended rows come last in row order and belong to blocks 3 and 5"""
    case = bc.case("edges")
    touched = (3, 5)
    r, st1, st2, rows_r, want_r = _resolve_with_cuts(case, False, touched)
    bad_ref = block_bar(case, r.getsolution(), r.lp_duals(), want_r, "ordinary", rows_r)
    assert (st1, st2) == ("Optimal", "Optimal") and bad_ref == [], (st1, st2, bad_ref)
    m, st1, st2, rows, want = _resolve_with_cuts(case, True, touched)
    print("edges re-solve: launches", m.stat("blk_lp_launches"), "fallbacks", m.stat("blk_lp_fallbacks"), "iterations max (both launches)",
          m.stat("blk_pdhg_iters_max"), "sum", m.stat("blk_pdhg_iters_sum"), "ordinary loop (both solves)", r.stat("pdhg_iters"))
    bad = block_bar(case, m.getsolution(), m.lp_duals(), want, "blocks", rows)
    assert (st1, st2) == ("Optimal", "Optimal") and bad == [], (st1, st2, bad)
    assert m.stat("blk_lp_launches") == 2 and m.stat("blk_lp_fallbacks") == 0 and no_exact_solver(m) and no_exact_solver(r)


def test_sign_infeasible_dual_warm_start():
    """lp_pdhg_raw leaves its y0 in place as the next solve's start (prep_row does not project it): every multiplier points at the
    side its row does NOT have wherever a row has only one.  The x it leaves is clamped into [l, u] by prep_col, so only the free
    and the one-sided columns start at 7, beyond every planted value"""
    case = bc.case("edges")
    want = planted_objectives(case)
    lo = np.where(np.isnan(case.lo), -np.inf, case.lo)
    y0 = np.where(np.isfinite(lo) & ~np.isfinite(case.hi), -1.5, 1.5)
    y0[np.isfinite(lo) & np.isfinite(case.hi)] *= -1.0
    x0 = np.full(case.n, 7.0)
    out = []
    for blocks in (False, True):
        m = bc.load(ktn, case, blocks, lp_max_iter=MAX_ITER)
        m.lp_pdhg_raw(x0, y0, 1e-3, 1.0, 1)
        st, _ = m.lp_solve(TOL, TOL)
        out.append((m, st, block_bar(case, m.getsolution(), m.lp_duals(), want, "blocks" if blocks else "ordinary")))
    (r, st_r, bad_r), (m, st, bad) = out
    print("edges from a sign-infeasible start: iterations max", m.stat("blk_pdhg_iters_max"), "sum", m.stat("blk_pdhg_iters_sum"),
          "ordinary loop", r.stat("pdhg_iters"))
    assert st_r == "Optimal" and bad_r == [], (st_r, bad_r)
    assert st == "Optimal" and bad == [], (st, bad)
    assert m.stat("blk_lp_launches") == 1 and m.stat("blk_lp_fallbacks") == 0 and no_exact_solver(m) and no_exact_solver(r)


@pytest.mark.parametrize("name", bc.INFEASIBLE)
def test_infeasible_block_sends_the_batch_to_the_ordinary_loop(name):
    """a block kernel has no infeasibility certificate: the bad block spends its budget and reports USERLIMIT, the launch counts one
    fall-back and the ordinary loop says Infeasible.  The budget is 4 x what the ordinary loop needs on a fresh handle with the
    default lp_max_iter (measured here, first): the margin is for its different restart schedule after the hand-over"""
    case = bc.case(name)
    r = bc.load(ktn, case, False)
    st_ref, it_ref = r.lp_solve(TOL, TOL)
    print(name, "ordinary loop:", st_ref, "after", it_ref, "iterations")
    assert st_ref == "Infeasible" and no_exact_solver(r)                      # (otherwise the case is wrong)
    m = bc.load(ktn, case, True, lp_max_iter=4 * it_ref)
    st, it = m.lp_solve(TOL, TOL)
    print(name, "blocks:", st, "lp_max_iter", 4 * it_ref, "iterations of the launch max", m.stat("blk_pdhg_iters_max"), "then the ordinary loop", it)
    assert st == "Infeasible"
    assert m.stat("blk_lp_launches") == 1 and m.stat("blk_lp_fallbacks") == 1 and no_exact_solver(m)


def test_block_that_cannot_finish_hands_a_feasible_lp_to_the_ordinary_loop():
    """`ranges` with a budget of 1.1 x the ordinary loop's iterations (4 447 when this was written; the block kernel's rule set
    needs 5 342 for its slower block): the launch spends the budget and reports USERLIMIT for that block, lp_solve counts one
    fall-back and runs the ordinary loop, whose start the launch has left untouched -- the iterations of the reference handle
    exactly -- and whose answer meets the bar"""
    case = bc.case("ranges")
    st_ref, _, _, it_ref, _ = reference("ranges", True)
    budget = int(1.1 * it_ref)
    m, st, it = solve(case, True, lp_max_iter=budget)
    print("ranges, budget", budget, ":", st, "launch max", m.stat("blk_pdhg_iters_max"), "then the ordinary loop", it, "(reference handle", it_ref, ")")
    assert st_ref == "Optimal" and st == "Optimal" and no_exact_solver(m)
    assert m.stat("blk_lp_launches") == 1 and m.stat("blk_lp_fallbacks") == 1 and m.stat("blk_pdhg_iters_max") == budget
    assert it == it_ref and m.stat("pdhg_iters") == it_ref
    assert block_bar(case, m.getsolution(), m.lp_duals(), planted_objectives(case), "ordinary after the launch") == []


# ---- heterogeneous batches through the two batch front ends ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hetero_instances():
    """six instances of different sizes and both families.  The per-instance LP passes over 1 024 columns / 1 280 rows, the device
    loop (ecp_spmv<4, 4> of csrc/batch_ecp.hpp) over 1 024 of either, and refuses more than 158 KB of LDS for
    (3 nmax + 3 mmax + (kEcpThreads / 64) kEcpQ + kEcpQ + 8 + 16) doubles + (max(nmax, mmax) + 4) ints, mmax = m_lin + cap m_nl,
    cap = 12, kEcpThreads = 1 024, kEcpQ = 12 (Engine::optimize_blocks_device): the largest instance needs 145.2 KB of them.
    Columns 40 < 64, 300, 1 000 and 1 023 < 1 024 < 1 100 and 1 030; LP rows 20 ... 950 < 1 024 < 1 100 (instance 4) and > 1 280
    (1 300 linear rows of instance 3 alone, its cuts on top)"""
    mk = ktn.instances.make_instance
    return (mk(n=40, m_nl=6, k=4, family="quad", seed=11, m_lin=14),
            mk(n=300, m_nl=40, k=8, family="explog", seed=12),
            mk(n=1000, m_nl=100, k=8, family="quad", seed=13),
            mk(n=1100, m_nl=250, k=8, family="explog", seed=14, m_lin=1300),
            mk(n=1030, m_nl=60, k=8, family="quad", seed=15, m_lin=1040),
            mk(n=1023, m_nl=80, k=16, family="explog", seed=16, m_lin=900))


@pytest.mark.parametrize("front", ["per_instance_lp", "device_loop"])
def test_heterogeneous_batch(front):
    insts = list(hetero_instances())
    assert max(i.n for i in insts) > 1024 and min(i.n for i in insts) < 64 and len({i.meta["family"] for i in insts}) == 2
    big = insts[3]
    mmax = big.m_lin + 12 * big.m_nl
    lds = (3 * big.n + 3 * mmax + 16 * 12 + 12 + 8 + 16) * 8 + (max(big.n, mmax) + 4) * 4
    assert 140 * 1024 < lds <= 158 * 1024
    kw = dict(per_instance_lp=True, device_loop=False) if front == "per_instance_lp" else dict(device_loop=True)
    res, _ = ktn.solve_batch(ktn.KatanaSolver(log_level=0), insts, fused=True, **kw)
    print(front, {k: res[0][k] for k in ("status", "iters", "blk_lp_launches", "blk_lp_fallbacks", "blk_pdhg_iters_sum", "ecp_blocks_launches",
                                        "ecp_blocks_fallbacks", "ecp_blocks_pdhg_sum", "pdhg_iters")})
    if front == "per_instance_lp":
        assert res[0]["blk_lp_launches"] >= 2 and res[0]["blk_lp_fallbacks"] == 0
    else:
        assert res[0]["ecp_blocks_launches"] == 1 and res[0]["ecp_blocks_fallbacks"] == 0
    for k, (r, inst) in enumerate(zip(res, insts)):
        print(front, "instance", k, "objective", r["objval"], "planted", inst.opt_obj, "max NL violation", max_nl_violation(inst, r["x"]),
              "max |x - xhat|", np.max(np.abs(r["x"] - inst.xhat)))
    for r, inst in zip(res, insts):
        assert r["status"] == "Optimal"
        assert_planted_objective(r["objval"], inst)
        assert max_nl_violation(inst, r["x"]) <= 1e-6 * (1 + 1e-6)
        assert np.max(np.abs(r["x"] - inst.xhat)) <= 1e-3
