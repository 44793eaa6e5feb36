"""GPU tier: the warm re-solve of a resident batch (KTN_BLOCKS_WARM, ktn_blocks_rewarm; csrc/batch_warm.hpp, DESIGN.md section 14
"In the device-side loop") on the ten instances of tests/blocks_warm_cases.py.

k_blocks_rewarm is checked against the plain-Python model of tests/blocks_warm_ref.py: records equal, arenas bit for bit.  The warm
launch is checked against a fresh batch solved cold on the modified instances, instance by instance through ktn_blocks_get_results
(both with fallback=False: the device loop has no exit for an LP that is infeasible without a row proving it, such an instance
runs out of LP iterations or of arena room, warm and cold alike -- the solver of this file caps the iterations at LP_MAX_ITER so
that this costs a fraction of a second; the bound changes of tests/test_gpu_resolve_bounds.py::changes do that to several of these
small instances, whose feasible sets are tight around the planted optimum.  Statuses are compared instance by instance and must be
equal; the one exception is an instance whose box a kept cut proves empty, which ends "Infeasible" warm where the cold loop cannot
finish.  CAP_SOLVE leaves every such instance room to meet the iteration limit: at 24 cuts per NL row 'fixed' instance 2 overflowed
warm (108 rows) where the cold run ended "UserLimit" at 97 rows).

A supporting launch after a KELLEY launch is the cold launch (the kept rows would have no lambda): nothing to test there."""
import os

import numpy as np
import pytest

import katana_jl_amd as ktn
from katana_jl_amd import _lib as L
from katana_jl_amd.batch import FusedBatch
import blocks_warm_cases as BC
import blocks_warm_ref as W
import kat_util
from test_gpu_resolve_bounds import changes

pytestmark = pytest.mark.gpu
LP_MAX_ITER = 30000            # (the cold solves of this batch need at most 7e3 PDHG iterations per instance in total)
F_TOL = 1e-6
CAP_MODEL = 8                  # room for 32 cuts per instance: cold, three instances end above 16 cuts (they compact), the others below
CAP_SOLVE = 48                 # (room for 192 cuts per instance: an instance that cannot finish meets the LP iteration limit first, warm and cold)
OPT = L.STATUS_OPTIMAL


def solver(**kw):
    return ktn.KatanaSolver(log_level=0, **dict(dict(lp_max_iter=LP_MAX_ITER), **kw))


@pytest.fixture(scope="module")
def world():
    items, viol, boxes, xhat = BC.batch()
    return dict(items=items, viol=viol, boxes=boxes, xhat=xhat)


def change_lists(world, out0, k):
    ls, us, name = [], [], None
    for b, (l0, u0) in enumerate(world["boxes"]):
        name, l, u = changes(np.asarray(out0[b]["x"]), l0, u0)[k]
        ls.append(l); us.append(u)
    return name, ls, us


def model_rewarm(fb, lin, cap, l_list, u_list, set_bounds=True):
    """set the boxes (set_bounds=False: they are the ones in force), run ktn_blocks_rewarm and the model on what stood before it;
    every record and arena compared; returns the model's (record, arena before, arena after) per instance"""
    m, offs = fb.m, fb.offs
    if set_bounds:
        fb.set_var_bounds(l_list, u_list)
    before, x_before = BC.read_arenas(fb, lin, cap), m.getsolution()
    rec = m.blocks_rewarm()
    assert m.blocks_rewarm().tobytes() == rec.tobytes()                              # idempotent
    after, x_after = BC.read_arenas(fb, lin, cap), m.getsolution()
    assert [a.M for a in BC.read_arenas(fb, lin, cap)] == [a.M for a in after]         # ... and the second call moved nothing
    tol0 = float(m.params.lp_tol_floor) * float(m.params.f_tol)
    out = []
    for b in range(len(before)):
        xb = [float(v) for v in x_before[offs[b]:offs[b + 1]]]
        bl, bu = m_bounds(fb, b, l_list, u_list)
        mrec, mafter, mx = W.rewarm(before[b], bl, bu, xb, tol0, float(m.params.purge_margin))
        print("instance %d: engine %s | model %s" % (b, list(rec[b]), mrec))
        assert [float(v) for v in mrec] == [float(v) for v in rec[b]], (b, mrec, list(rec[b]))
        assert BC.cut_bits(mafter) == BC.cut_bits(after[b]), b
        assert mx == [float(v) for v in x_after[offs[b]:offs[b + 1]]], b
        if mrec[0] == 1:
            W.check_invariants(before[b], after[b], mrec)
        out.append((mrec, before[b], mafter))
    return out


def m_bounds(fb, b, l_list, u_list):
    """instance b's box as the engine holds it (an instance's own variables are all of its columns in this batch)"""
    n = int(fb.offs[b + 1] - fb.offs[b])
    assert len(l_list[b]) == n
    return [float(v) for v in l_list[b]], [float(v) for v in u_list[b]]


def test_rewarm_against_the_model(world):
    items, boxes = world["items"], world["boxes"]
    fb = FusedBatch(solver(), items)
    out0 = fb.solve(cut_capacity=CAP_MODEL)
    assert all(o["status"] == "Optimal" for o in out0) and fb.m.stat("ecp_blocks_fallbacks") == 0
    lin = BC.linear_rows(fb)
    assert len(lin[6]) == 12 and BC.nl_counts(fb, lin)[6] == 0 and len(lin[7]) == 0 and len(lin[8]) == BC.BIG_LIN >= 1100
    # ---- 1. the loaded boxes again: nothing is screened out, x stays, the arenas above half fill compact at the optimum
    res = model_rewarm(fb, lin, CAP_MODEL, [l for l, _ in boxes], [u for _, u in boxes])
    assert all(r[0][0] == 1 for r in res)
    compacted = [b for b, (r, a0, a1) in enumerate(res) if r[3] > 0]
    over_half = [b for b, (r, a0, a1) in enumerate(res) if a0.M - a0.m_lin > (a0.cap_rows - a0.m_lin) // 2]
    untouched = [b for b, (r, a0, a1) in enumerate(res) if a0.M > a0.m_lin and b not in over_half]
    assert len(compacted) >= 2 and len(untouched) >= 2 and set(compacted) <= set(over_half), (compacted, over_half, untouched)
    head_dropped = adjacent = list_emptied = False
    x_all = fb.m.getsolution()
    for b in compacted:
        r, a0, a1 = res[b]
        xs = [float(v) for v in x_all[fb.offs[b]:fb.offs[b + 1]]]
        idle = [W.idle_row(a0.cols[q], a0.vals[q], a0.lo[q], a0.hi[q], a0.y[q], xs, float(fb.m.params.purge_margin)) for q in range(a0.m_lin, a0.M)]
        gone = [a0.m_lin + k for k, i in enumerate(idle) if i]
        assert len(gone) == r[3]
        head_dropped = head_dropped or any(h in gone for h in a0.last)
        adjacent = adjacent or any(q + 1 in gone for q in gone)
        list_emptied = list_emptied or any(h0 >= 0 and h1 < 0 for h0, h1 in zip(a0.last, a1.last))
    assert head_dropped and adjacent and list_emptied                                 # a list head went, two neighbours went, a whole list went
    assert fb.m.stat("ecp_blocks_warm_dropped_rows") == sum(r[0][3] for r in res) > 0
    # ---- 2. screen cases with margins far above tau_k (about 1e-6 here): crossed columns on instance 1, a box that one linear
    # row of instance 3 excludes by more than 1e-3; the others keep their boxes.  The compacted arenas of step 1 are the input.
    l_list, u_list = [l.copy() for l, _ in boxes], [u.copy() for _, u in boxes]
    l_list[1][2], u_list[1][2] = u_list[1][2], l_list[1][2]
    l_list[1][5], u_list[1][5] = u_list[1][5], l_list[1][5]
    k = excluded_box(lin[3], l_list[3], u_list[3])
    res = model_rewarm(fb, lin, CAP_MODEL, l_list, u_list)
    assert res[1][0][0] == 2 and res[1][0][6] == 2 and res[3][0][0] == 2 and 0 <= res[3][0][5] <= k
    assert [r[0][0] for b, r in enumerate(res) if b not in (1, 3)] == [1] * 8
    assert fb.m.stat("ecp_blocks_warm_infeasible") == 2 and fb.m.stat("ecp_blocks_warm_instances") == 8


def excluded_box(rows, l, u):
    """pins the columns of the first linear row with a finite upper side where its smallest value lies above the bound (l, u are
    changed in place); returns the row"""
    k = next(k for k, r in enumerate(rows) if np.isfinite(r[3]))
    cols, vals, _, hi = rows[k]
    for j, a in zip(cols, vals):
        if a > 0:
            l[j] = u[j]
        elif a < 0:
            u[j] = l[j]
    amin = sum(a * (l[j] if a > 0 else u[j]) for j, a in zip(cols, vals))
    assert amin > hi + 1e-3, (amin, hi)
    return k


@pytest.fixture(scope="module")
def warm_table(world):
    """the unchanged batch and the four changes, each solved warm on one resident handle and cold on a fresh batch; every check
    of 'warm solve is right' asserted on the way; returns the rows (change, cold rounds, warm rounds) summed over the instances"""
    items, viol, boxes = world["items"], world["viol"], world["boxes"]
    fb = FusedBatch(solver(), items)
    out0 = fb.solve(cut_capacity=CAP_SOLVE)
    assert all(o["status"] == "Optimal" for o in out0)
    rec0 = fb.m.blocks_results().copy()
    rows = []
    cases = [("unchanged", [l for l, _ in boxes], [u for _, u in boxes])] + [change_lists(world, out0, k) for k in range(4)]
    for name, l_list, u_list in cases:
        fb.set_var_bounds(l_list, u_list)
        rewarm_rec = fb.m.blocks_rewarm().copy()
        outw = fb.solve(cut_capacity=CAP_SOLVE, warm=True, fallback=False)
        recw = fb.m.blocks_results().copy()
        fresh = FusedBatch(solver(), [BC.with_box(it, l, u) for it, l, u in zip(items, l_list, u_list)])
        outc = fresh.solve(cut_capacity=CAP_SOLVE, fallback=False)
        recc = fresh.m.blocks_results().copy()
        state = fb.m.stat("ecp_blocks_warm_infeasible")
        assert fb.m.stat("ecp_blocks_fallbacks") == 0 and fresh.m.stat("ecp_blocks_fallbacks") == 0
        for b in range(len(items)):
            print("%-9s instance %d: warm status %d rounds %d pdhg %d rows %d obj %.9f | cold status %d rounds %d pdhg %d rows %d obj %.9f" % (
                name, b, recw[b, 0], recw[b, 1], recw[b, 4], recw[b, 6], outw[b]["objval"], recc[b, 0], recc[b, 1], recc[b, 4], recc[b, 6], outc[b]["objval"]))
        # status per instance: equal.  The one exception is what the warm path knows and the cold one cannot: an instance whose box
        # a KEPT CUT proves empty ends :Infeasible warm without an LP, while the cold loop, which has no exit for an infeasible LP,
        # runs out of iterations or of room on it.
        for b in range(len(items)):
            sw, sc = int(recw[b, 0]), int(recc[b, 0])
            if sw == L.STATUS_INFEASIBLE:
                assert sc != OPT and recw[b, 4] == 0 and rewarm_rec[b, 0] == 2 and rewarm_rec[b, 5] >= 0, (name, b, sw, sc)
                continue
            assert sw == sc, (name, b, sw, sc)
            if sw != OPT:
                continue
            assert kat_util.isapprox(outw[b]["objval"], outc[b]["objval"], 1e-6, 1e-6), (name, b, outw[b]["objval"], outc[b]["objval"])
            x = np.asarray(outw[b]["x"])
            assert np.all(x >= l_list[b] - 1e-9) and np.all(x <= u_list[b] + 1e-9)
            assert viol[b](x) <= F_TOL, (name, b, viol[b](x))
        rows.append((name, int(recc[:, 1].sum()), int(recw[:, 1].sum()), int(recc[:, 4].sum()), int(recw[:, 4].sum()), int(state)))
    assert fb.m.stat("ecp_blocks_warm_launches") == len(cases)
    return dict(rows=rows, fb=fb, rec0=rec0)


def test_warm_solve_equals_a_fresh_cold_batch(warm_table):
    assert len(warm_table["rows"]) == 5


def test_warm_rounds_are_fewer_in_total_and_the_table_is_written(warm_table):
    rows = warm_table["rows"]
    cold, warm = sum(r[1] for r in rows), sum(r[2] for r in rows)
    lines = ["%-10s %6s %6s %9s %9s %10s" % ("change", "cold", "warm", "cold pdhg", "warm pdhg", "infeasible")]
    lines += ["%-10s %6d %6d %9d %9d %10d" % r for r in rows]
    lines.append("%-10s %6d %6d   (cutting-plane rounds summed over the ten instances)" % ("total", cold, warm))
    print("\n".join(lines))
    out = os.environ.get("KTN_BLOCKS_WARM_TABLE")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert warm < cold, (warm, cold)


@pytest.fixture(scope="module")
def interior(world):
    """an interior point per instance: the engine's own (the auxiliary problem of the fused batch, found once by a handle in
    supporting-hyperplane mode), split by instance.  It is not a usable reference point for every instance (instance 2: found = -1
    after a cold launch too), so the test holds the warm launch to what the cold launch finds with the same points."""
    fb = FusedBatch(solver(cut_algo="supporting_hyperplane"), world["items"])
    xi = fb.m.interior_point()
    assert xi is not None
    return [np.array(xi[int(fb.offs[b]):int(fb.offs[b + 1])]) for b in range(len(world["items"]))]


def test_kkt_report_and_feasible_points_after_a_warm_launch(world, interior):
    """after a warm launch whose rewarm COMPACTED arenas (capacity CAP_MODEL, as in the test against the model), so that the report
    walks the lists as k_blocks_rewarm re-threaded them: bound <= objective <= primal bound per instance, the multipliers of the
    NL rows the sums over the re-threaded lists"""
    items = world["items"]
    fb = FusedBatch(solver(), items)
    out0 = fb.solve(cut_capacity=CAP_MODEL)
    d0 = fb.constr_duals()
    fb.set_interior_points(interior)
    found0 = [p.found for p in fb.feasible_points()]                                  # what the cold launch gives with these points
    assert sum(f == 1 for f in found0) >= 5, found0
    rec = fb.m.blocks_rewarm()
    assert rec[:, 3].sum() > 0 and np.all(rec[:, 0] == 1)
    # the multiplier of an NL row is the sum over its list, newest first: the dropped rows carried 0.0, so the re-threaded lists
    # give the same bits
    for b, (da, db) in enumerate(zip(d0, fb.constr_duals())):
        assert da.tobytes() == db.tobytes(), b
    out = fb.solve(cut_capacity=CAP_MODEL, warm=True, fallback=False)
    assert fb.m.stat("ecp_blocks_warm_launches") == 1 and fb.m.stat("ecp_blocks_warm_dropped_rows") > 0 and fb.m.stat("ecp_blocks_warm_instances") == 10
    assert all(o["status"] == "Optimal" for o in out)
    duals, bounds = fb.constr_duals(), fb.dual_bounds()
    fb.set_interior_points(interior)
    pts = fb.feasible_points()
    assert len(duals) == len(bounds) == len(pts) == 10
    for b, ((bound, gap), fp) in enumerate(zip(bounds, pts)):
        obj = out[b]["objval"]
        slack = 1e-6 * max(1.0, abs(obj))
        print("instance %d: bound %.9f objective %.9f primal %.9f found %d" % (b, bound, obj, fp.objval, fp.found))
        assert fp.found == found0[b], (b, fp.found, found0[b])
        assert bound <= obj + slack, (b, bound, obj)
        if found0[b] == 1:                                                              # (at least five instances: asserted above)
            assert obj <= fp.objval + slack, (b, obj, fp.objval)
        assert len(duals[b]) == len(d0[b]) and np.all(np.isfinite(duals[b]))


def test_a_warm_flag_without_a_previous_launch_is_the_cold_launch(world):
    items = world["items"]
    a, twin = FusedBatch(solver(), items), FusedBatch(solver(), items)
    oa = a.solve(warm=True)
    ot = twin.solve()
    assert a.m.stat("ecp_blocks_warm_launches") == 0 and a.m.stat("ecp_blocks_launches") == 1
    assert a.m.blocks_results().tobytes() == twin.m.blocks_results().tobytes()
    assert a.m.getsolution().tobytes() == twin.m.getsolution().tobytes() and [o["status"] for o in oa] == [o["status"] for o in ot]
    a.solve(warm=True)                                                                # now there is one: a warm launch
    assert a.m.stat("ecp_blocks_warm_launches") == 1
    a.solve()                                                                         # a plain solve() after it: reset, cold
    assert a.m.blocks_results().tobytes() == twin.m.blocks_results().tobytes() and a.m.getsolution().tobytes() == twin.m.getsolution().tobytes()
    assert a.m.stat("ecp_blocks_warm_launches") == 1
    with pytest.raises(L.KatanaHipError) as e:                                        # reset dropped the warm state ... until the next launch
        a.m.reset()
        a.m.blocks_rewarm()
    assert e.value.code == L.E_INVALID


def test_infeasible_per_instance_then_restored(world):
    items, boxes = world["items"], world["boxes"]
    fb = FusedBatch(solver(), items)
    out0 = fb.solve()
    lin = BC.linear_rows(fb)
    l_list, u_list = [l.copy() for l, _ in boxes], [u.copy() for _, u in boxes]
    l_list[1][0], u_list[1][0] = u_list[1][0], l_list[1][0]                           # crossed
    excluded_box(lin[3], l_list[3], u_list[3])
    fb.set_var_bounds(l_list, u_list)
    st = fb.solve(warm=True)[0]["status"]                                             # (fallback allowed: the screen's verdict must not trigger it)
    rec = fb.m.blocks_results()
    assert st == "Infeasible" and fb.m.stat("ecp_blocks_fallbacks") == 0
    for b in range(10):
        assert rec[b, 0] == (L.STATUS_INFEASIBLE if b in (1, 3) else OPT), (b, rec[b])
    assert rec[1, 4] == 0 and rec[3, 4] == 0 and rec[1, 1] == 0 and rec[3, 1] == 0       # no LP at all
    fb.set_var_bounds([l for l, _ in boxes], [u for _, u in boxes])
    out = fb.solve(warm=True, fallback=False)
    assert all(o["status"] == "Optimal" for o in out) and np.all(fb.m.blocks_results()[:, 0] == OPT)
    assert fb.m.stat("ecp_blocks_warm_cold_instances") == 2                           # the two start from their linear rows again
    for b in range(10):
        assert kat_util.isapprox(out[b]["objval"], out0[b]["objval"], 1e-6, 1e-6), b


def shrunk(world, out0):
    """both bounds of every variable a quarter of the way towards the solution: the optimum stays"""
    ls, us = [], []
    for (l0, u0), o in zip(world["boxes"], out0):
        x = np.asarray(o["x"])
        ls.append(l0 + 0.25 * (x - l0)); us.append(u0 - 0.25 * (u0 - x))
    return ls, us


def alternate(world, n):
    """n warm re-solves alternating between the shrunk and the loaded boxes at the default capacity; (batch, [records], [x])"""
    fb = FusedBatch(solver(), world["items"])
    out0 = fb.solve()
    two = [shrunk(world, out0), ([l for l, _ in world["boxes"]], [u for _, u in world["boxes"]])]
    recs, xs = [fb.m.blocks_results().copy()], [fb.m.getsolution().copy()]
    for k in range(n):
        fb.set_var_bounds(*two[k % 2])
        out = fb.solve(warm=True)
        recs.append(fb.m.blocks_results().copy()); xs.append(fb.m.getsolution().copy())
        assert all(o["status"] == "Optimal" for o in out), (k, [o["status"] for o in out])
    return fb, recs, xs


def test_capacity_holds_over_eight_warm_resolves(world):
    fb, recs, _ = alternate(world, 8)
    for k, r in enumerate(recs):
        print("solve %d: rows %s rounds %s" % (k, list(r[:, 6].astype(int)), list(r[:, 1].astype(int))))
        assert np.all(r[:, 7] == 0) and np.all(r[:, 0] == OPT), k
    assert fb.m.stat("ecp_blocks_fallbacks") == 0 and fb.m.stat("ecp_blocks_warm_launches") == 8


def test_the_same_sequence_on_two_handles_is_bit_identical(world):
    fa, ra, xa = alternate(world, 3)
    fb, rb, xb = alternate(world, 3)
    assert [r.tobytes() for r in ra] == [r.tobytes() for r in rb] and [x.tobytes() for x in xa] == [x.tobytes() for x in xb]
    la, lb = BC.linear_rows(fa), BC.linear_rows(fb)
    for a, b in zip(BC.read_arenas(fa, la, 12), BC.read_arenas(fb, lb, 12)):
        assert BC.cut_bits(a) == BC.cut_bits(b)


def test_supporting_variant_moves_and_keeps_the_lambdas(world):
    """a supporting launch at a capacity where the instance with the most cuts is above half fill: k_blocks_rewarm against the
    model with lambdas that are not all 1 (bit for bit, the moved ones included), then the warm supporting launch keeps them"""
    items = world["items"]
    fb = FusedBatch(solver(cut_algo="supporting_hyperplane"), items)
    out0 = fb.solve(cut_capacity=CAP_SOLVE, supporting=True)                           # (the engine's own interior point)
    assert all(o["status"] == "Optimal" for o in out0) and fb.m.stat("ecp_blocks_esh_rows") > 0
    lin = BC.linear_rows(fb)
    most = max(a.M - a.m_lin for a in BC.read_arenas(fb, lin, CAP_SOLVE))
    cap = -(-most // 4)                                                               # 4 NL rows per instance: room 4 cap >= most > 2 cap
    out0 = fb.solve(cut_capacity=cap, supporting=True)
    assert all(o["status"] == "Optimal" for o in out0) and fb.m.stat("ecp_blocks_fallbacks") == 0
    boxes = world["boxes"]
    res = model_rewarm(fb, lin, cap, [l for l, _ in boxes], [u for _, u in boxes], set_bounds=False)
    moved = [(r, a0, a1) for r, a0, a1 in res if r[3] > 0]
    assert moved and any(v != 1.0 for r, a0, a1 in moved for v in a1.lam[a1.m_lin:]), [r for r, _, _ in res]
    assert any(a1.lam[a1.m_lin:] != a0.lam[a0.m_lin:a0.m_lin + a1.M - a1.m_lin] for r, a0, a1 in moved)      # some lambda changed its row
    out = fb.solve(cut_capacity=cap, supporting=True, warm=True)
    assert fb.m.stat("ecp_blocks_warm_launches") == 1 and fb.m.stat("ecp_blocks_fallbacks") == 0
    after = BC.read_arenas(fb, lin, cap)
    for b, ((r, a0, a1), a2) in enumerate(zip(res, after)):
        assert out[b]["status"] == "Optimal" and kat_util.isapprox(out[b]["objval"], out0[b]["objval"], 1e-6, 1e-6), b
        n = a1.M - a1.m_lin
        assert a2.M >= a1.M and [v.hex() for v in a2.lam[a2.m_lin:a2.m_lin + n]] == [v.hex() for v in a1.lam[a1.m_lin:]], b
    assert fb.m.stat("ecp_blocks_tape_rows") == 1                                      # the tape row counts as a fallback row, as in a cold launch
