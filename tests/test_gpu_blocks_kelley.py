"""GPU tier: the Kelley path of the device-side batch loop (k_ecp_blocks<0>, csrc/batch_ecp.hpp) cut by cut -- the sweep inside the
workgroup (16 lanes per separable row, one lane per tape row, the two QUAD passes), its verdict, the rank scan, the emit pass with
round_coefs, the cut constant and the row bounds, and the hand-over of the previous cut's multiplier -- against the 200-bit
references of tests/sep_ref.py, tests/tape_ref.py and tests/quad_ref.py, on the cases of tests/blocks_cut_cases.py (whose input
conditions tests/test_blocks_cut_cases.py asserts).  Every launch is ktn_optimize_blocks_ex without the fall-back and asserts
that the device loop ran.  Tolerances come from the three reference modules; the only literals are f_tol = 2^-20 (sep_ref.F_TOL)
and the cap on undecided rows.

Part A pins the point of the first round (the box is the point) and checks that round alone.  Part B launches a fresh batch with
iter_cap = 1 .. 4: the loop is deterministic, so run r repeats run r - 1 bit for bit and then takes round r's cuts at the point
it returns.  An instance that has met the stop rule may go on cutting in certificate-refinement passes at points it does not
return: its records are compared between runs, not with the reference.
An instance without linear rows solves an LP without rows first: its point must be the box vertex that the signs of the costs
pick.  (Before the loop defined ys[0], y0s[0] and yts[0] for such an LP, a NaN left in LDS by an earlier workgroup -- the NaN row
values of part A's edges = 1 batch are one source -- reached A'y through ecp_spmv's 0.0 * v[0] and the round was taken at l_var
instead; which workgroup met such leftovers varied from run to run.)

Each test prints the largest |device - reference| / bound per quantity."""
import numpy as np
import pytest
from mpmath import mp, mpf

import blocks_cut_cases as bc
import katana_jl_amd as ktn
import sep_cases as sc
import sep_ref
from katana_jl_amd.batch import FusedBatch
from sep_ref import F_TOL, U

pytestmark = pytest.mark.gpu
L = ktn._lib
INF = float("inf")
UNDECIDED_CAP = 1
STATUS = ktn.solver.STATUS_SYMBOLS
KIND = {L.ROW_SEP: "sep", L.ROW_TAPE: "tape", L.ROW_QUAD: "quad"}


def solver(**kw):
    return ktn.KatanaSolver(log_level=0, f_tol=F_TOL, **dict(dict(lp_max_iter=400000), **kw))


class Worst:
    """asserts err <= bound and keeps the largest err / bound per quantity"""

    def __init__(self):
        self.r = {}

    def __call__(self, name, err, bound, what):
        err, bound = float(err), float(bound)
        assert err <= bound, (name, what, err, bound)
        self.r[name] = max(self.r.get(name, 0.0), err / bound if bound > 0 else 0.0)

    def __str__(self):
        return "  ".join("%s %.3f" % kv for kv in sorted(self.r.items()))


class Run:
    pass


def launch(items, r, cut_capacity=0, **kw):
    """a fresh batch through the device loop with iter_cap = r, no fall-back; everything read back"""
    fb = FusedBatch(solver(iter_cap=r, **kw), items)
    st = fb.m.optimize_blocks(cut_capacity, fallback=False)
    assert fb.m.stat("ecp_blocks_launches") == 1 and fb.m.stat("ecp_blocks_fallbacks") == 0
    R = Run()
    R.fb, R.status, R.x, R.res = fb, st, fb.m.getsolution(), fb.m.blocks_results()
    assert R.res.shape == (len(items), 8)
    R.cuts, R.duals = [], []
    for b in range(len(items)):
        c = fb.m.blocks_cuts(b)
        c["col"] = c["col"].astype(np.int64) - int(fb.offs[b])
        R.cuts.append(c)
        R.duals.append(fb.m.blocks_duals(b))
        assert len(R.duals[b]) == len(c["lo"]) == len(c["rowptr"]) - 1
    R.nl0 = np.concatenate([[0], np.cumsum([int(np.sum(ktn.batch._as_problem(p).d.row_linear == 0)) for p in items])])
    return R


def check_bound(W, name, dev, bnd, exact_b, tol, what):
    """a cut row's bound fl(bnd - b): +-inf exactly, else within tol of the exact value"""
    if np.isinf(bnd):
        assert dev == bnd, (name, what, dev, bnd)
        return
    with mp.workprec(sep_ref.PREC):
        W(name, abs(mpf(float(dev)) - (mpf(float(bnd)) - exact_b)) if np.isfinite(dev) else INF, tol, what)


# ---- A. one round at a prescribed point -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edges", [0, 1])
def test_one_round_at_a_prescribed_point_on_separable_rows(edges):
    cases = bc.pinned_batch(edges)
    run = launch([bc.pinned_problem(C) for C in cases], 1, cut_coef_rng=bc.CUT_COEF_RNG)
    # the input condition: the point of the round is the prescribed one, bit for bit
    assert np.array_equal(run.x, np.concatenate([C.x for C in cases]))
    assert run.fb.m.stat("ecp_blocks_tape_rows") == 0 and run.fb.m.stat("ecp_blocks_quad_rows") == 0
    W = Worst()
    seen = dict(zeroed=0, nan=0, thr_cut=0, thr_kept=0, trips=set())
    sides = set()
    for b, C in enumerate(cases):
        R = sc.reference(C)
        E = sc.expected_sweep(C, R)
        c, res = run.cuts[b], run.res[b]
        slots = c["slot"] - run.nl0[b]
        assert np.all(np.diff(slots) > 0), (b, "slots ascending, each once")
        assert np.array_equal(slots, E.viol_slots), (b, sorted(set(slots.tolist()) ^ set(E.viol_slots.tolist())))
        assert STATUS[int(res[0])] == "UserLimit" and res[1] == 1 and res[3] == res[6] == E.nviol > 0 and res[7] == 0, (b, res)
        if np.isfinite(E.maxviol):
            W("max_viol", abs(res[5] - E.maxviol), E.maxviol_tol, b)
        else:
            assert res[5] == INF and C.edges == 1, (b, res[5])
        assert np.array_equal(c["rowptr"], E.cut_rowptr) and np.array_equal(c["col"], E.col), (b, "cut columns / storage order")
        assert np.all(c["lam"] == 1.0) and np.all(run.duals[b] == 0.0)
        val = c["val"]
        assert np.all(val[E.zeroed] == 0.0), (b, "round_coefs kept a coefficient", np.flatnonzero(E.zeroed & (val != 0.0))[:5])
        assert np.all(val[~E.zeroed] != 0.0), (b, "round_coefs dropped a coefficient", np.flatnonzero(~E.zeroed & (val == 0.0))[:5])
        keep = ~E.zeroed
        err = np.abs(val - E.coef)[keep]
        assert np.all(err <= E.coef_tol[keep]), (b, "coefficient", np.flatnonzero(keep)[err > E.coef_tol[keep]][:5])
        pos = E.coef_tol[keep] > 0                               # (LIN atoms: the coefficient is exact)
        if pos.any():
            W("coef(f64)", float(np.max(err[pos] / E.coef_tol[keep][pos])), 1.0, b)
        for name, dv, want, tol in (("lo", c["lo"], E.lo, E.lo_tol), ("hi", c["hi"], E.hi, E.hi_tol)):
            fin = np.isfinite(want)
            with np.errstate(invalid="ignore"):
                bad = fin & ~(np.abs(dv - want) <= tol)
            assert not bad.any(), (b, name, E.viol_rows[bad][:5], dv[bad][:5], want[bad][:5], tol[bad][:5])
            if fin.any():
                W(name + "(f64)", float(np.max(np.abs(dv[fin] - want[fin]) / tol[fin])), 1.0, b)
            okc = (np.isnan(dv[~fin]) & np.isnan(want[~fin])) | (dv[~fin] == want[~fin])
            assert okc.all(), (b, name + " class", E.viol_rows[~fin][~okc][:5], dv[~fin][~okc][:5], want[~fin][~okc][:5])
            seen["nan"] += int(np.isnan(dv).sum())
        seen["zeroed"] += int(E.zeroed.sum())
        for r in E.viol_rows[np.isfinite(R.g[E.viol_rows])]:
            sides.add(("two" if np.isfinite(C.e_lb[r]) and np.isfinite(C.e_ub[r]) else "one", "above" if R.g[r] > C.e_ub[r] else "below"))
        seen["trips"] |= set((slots // 64).tolist())
        # the sample against mpmath: verdict, partials, row bounds
        at = {int(r): k for k, r in enumerate(E.viol_rows)}
        for r in bc.mp_sample(C):
            M = sc.row_mp(C, r)
            lb, ub = C.e_lb[r], C.e_ub[r]
            sat = M.g is not None and M.g >= lb - F_TOL and M.g <= ub + F_TOL
            assert (r in at) == (not sat), (b, C.e_tags[r], r, "verdict")
            if C.e_threshold[r]:
                seen["thr_kept" if sat else "thr_cut"] += 1
            if sat:
                continue
            k = at[r]
            a, e = int(c["rowptr"][k]), int(c["rowptr"][k + 1])
            for j in range(e - a):
                if E.zeroed[a + j]:
                    continue
                with mp.workprec(sep_ref.PREC):
                    W("coef", abs(mpf(float(val[a + j])) - M.der[j]), 2 * M.e_der[j], (b, r, j))
            if M.b is None:
                assert np.isnan(c["lo"][k]) and np.isnan(c["hi"][k]), (b, r)
                continue
            check_bound(W, "lo", c["lo"][k], lb, M.b, M.bound_tol(lb) if np.isfinite(lb) else 0, (b, r))
            check_bound(W, "hi", c["hi"][k], ub, M.b, M.bound_tol(ub) if np.isfinite(ub) else 0, (b, r))
    print("part A edges=%d  |device - reference| / bound:  %s" % (edges, W))
    # what the test is about occurred
    assert seen["zeroed"] > 0 and seen["thr_cut"] == seen["thr_kept"] == 2 * len(cases), seen
    assert sides == {("one", "above"), ("one", "below"), ("two", "above"), ("two", "below")}, sides
    assert (seen["nan"] > 0) == bool(edges)
    if not edges:
        assert {0, 1, 2} <= seen["trips"] and min(C.m_nl for C in cases) < 16 and max(C.m_nl for C in cases) == 150


# ---- B. several rounds at the loop's own points -----------------------------------------------------------------------------------
class Tally:
    def __init__(self):
        self.W = Worst()
        self.undecided = self.handovers = self.handovers_nonzero = self.idle_rounds = self.rowless = 0
        self.cut = set()                   # (kind, row form, side)
        self.rounds_with_cuts = {}         # instance -> rounds in which it took cuts
        self.slots = set()


def same_prefix(a, b, n, what):
    """the first n cut rows of read-back a are those of b, bit for bit"""
    assert len(b["lo"]) >= n and len(a["lo"]) >= n, what
    e = int(b["rowptr"][n])
    assert np.array_equal(a["rowptr"][:n + 1], b["rowptr"][:n + 1]), what
    for key, cnt in (("col", e), ("val", e), ("lo", n), ("hi", n), ("slot", n)):
        assert np.array_equal(a[key][:cnt], b[key][:cnt]), (what, key)


def check_rounds(items, runs, T):
    """runs[r - 1]: the launch with iter_cap = r"""
    probs = [ktn.batch._as_problem(p) for p in items]
    for b, p in enumerate(probs):
        rows = bc.nl_rows_of(p)
        m_lin = int(np.sum(p.d.row_linear != 0))
        for ri, run in enumerate(runs):
            r = ri + 1
            res, c, y = run.res[b], run.cuts[b], run.duals[b]
            status = STATUS[int(res[0])]
            assert status in ("UserLimit", "Optimal") and res[7] == 0, (b, r, res)
            assert res[3] == res[6] == m_lin + len(c["lo"]), (b, r, res)
            assert np.all(c["lam"] == 1.0)
            n_prev = 0
            if ri:
                prev = runs[ri - 1]
                n_prev = int(prev.res[b][6]) - m_lin
                same_prefix(c, prev.cuts[b], n_prev, (b, r))
                if STATUS[int(prev.res[b][0])] == "Optimal":          # done earlier: the same records in every later run
                    assert np.array_equal(res, prev.res[b]) and len(c["lo"]) == n_prev and np.array_equal(y, prev.duals[b]), (b, r)
                    assert np.array_equal(run.x[run.fb.offs[b]:run.fb.offs[b + 1]], prev.x[prev.fb.offs[b]:prev.fb.offs[b + 1]])
                    continue
            if status == "Optimal":                                   # met the stop rule in this run: see the module docstring
                assert res[1] <= r
                continue
            assert res[1] == r, (b, r, res)
            x = run.x[run.fb.offs[b]:run.fb.offs[b + 1]]
            if ri == 0 and m_lin == 0:
                # the first LP of an instance without linear rows has no rows at all: its optimum is the vertex of the box that the
                # signs of the costs pick, exactly (the prox clips)
                cost = np.zeros(p.num_var)
                cost[p.d.obj_col] = p.d.obj_p0
                assert p.sense == "Min" and np.all(cost != 0.0) and len(x) == p.num_var
                assert np.array_equal(x, np.where(cost > 0.0, p.l_var, p.u_var)), (b, "first point of an LP without rows", x)
                T.rowless += 1
            slots = (c["slot"] - run.nl0[b])[n_prev:]
            assert np.all(np.diff(slots) > 0) and (len(slots) == 0 or (slots[0] >= 0 and slots[-1] < len(rows))), (b, r, slots)
            at = {int(s): n_prev + k for k, s in enumerate(slots)}
            vmax, vtol = None, 0
            for i, row in enumerate(rows):
                R = bc.row_ref(row, x)
                dec, v = bc.verdict(row, R)
                what = (b, r, KIND[row.kind], i)
                if dec == 0:
                    T.undecided += 1
                else:
                    assert (i in at) == (dec > 0), what + ("verdict", float(v))
                if i not in at:
                    continue
                k = at[i]
                a, e = int(c["rowptr"][k]), int(c["rowptr"][k + 1])
                assert np.array_equal(c["col"][a:e], row.cols), what + ("columns / storage order",)
                with mp.workprec(sep_ref.PREC):
                    for j in range(e - a):
                        T.W("coef " + KIND[row.kind], abs(mpf(float(c["val"][a + j])) - R.der[j]), R.e_der[j], what + (j,))
                    tol_v = R.e_g + 2 * mpf(U) * abs(v)
                    if vmax is None or v > vmax:
                        vmax = v
                    vtol = max(vtol, tol_v)
                for name, dv, bnd in (("lo ", c["lo"][k], row.lb), ("hi ", c["hi"][k], row.ub)):
                    check_bound(T.W, name + KIND[row.kind], dv, bnd, R.b, R.bound_tol(bnd) if np.isfinite(bnd) else 0, what)
                form = "two" if np.isfinite(row.lb) and np.isfinite(row.ub) else ("up" if np.isfinite(row.ub) else "lo")
                with mp.workprec(sep_ref.PREC):
                    T.cut.add((KIND[row.kind], form, "above" if R.g > row.ub else "below"))
                T.slots.add(i)
                # the multiplier: the previous cut of the slot hands its own over and keeps exactly 0
                before = np.flatnonzero((c["slot"] - run.nl0[b])[:n_prev] == i)
                if len(before):
                    assert y[before[-1]] == 0.0 and np.isfinite(y[k]), what + ("hand-over", y[before[-1]], y[k])
                    T.handovers += 1
                    T.handovers_nonzero += int(y[k] != 0.0)
                else:
                    assert y[k] == 0.0, what + ("first cut of its slot", y[k])
            if vmax is None:                                          # a round without a new cut: every row satisfied (asserted above)
                assert res[5] == 0.0, (b, r, res)
                T.idle_rounds += 1
            else:
                with mp.workprec(sep_ref.PREC):
                    T.W("max_viol", abs(mpf(float(res[5])) - vmax), vtol, (b, r))
                T.rounds_with_cuts.setdefault(b, set()).add(r)


def run_rounds(items, rounds=4, cut_capacity=0):
    T = Tally()
    runs = [launch(items, r, cut_capacity) for r in range(1, rounds + 1)]
    check_rounds(items, runs, T)
    print("rounds 1-%d: undecided %d, hand-overs %d (%d non-zero), rounds without a cut %d, cut %s" %
          (rounds, T.undecided, T.handovers, T.handovers_nonzero, T.idle_rounds, sorted(T.cut)))
    print("|device - reference| / bound:  %s" % T.W)
    assert T.undecided <= UNDECIDED_CAP, T.undecided
    assert T.handovers > 0 and T.handovers_nonzero > 0           # a multiplier was handed over, and not only zeros
    return runs, T


def test_rounds_on_separable_rows():
    runs, T = run_rounds(bc.sep_items())
    assert runs[0].fb.m.stat("ecp_blocks_tape_rows") == 0 and runs[0].fb.m.stat("ecp_blocks_quad_rows") == 0
    assert {("sep", "up", "above"), ("sep", "lo", "below"), ("sep", "two", "above")} <= T.cut, T.cut
    assert T.rowless == 2                                       # the two instances without linear rows: their first point is the box vertex
    assert any(len(v) >= 3 for v in T.rounds_with_cuts.values()), T.rounds_with_cuts


def test_rounds_on_tape_rows():
    items = bc.tape_items()
    runs, T = run_rounds(items)
    assert runs[0].fb.m.stat("ecp_blocks_tape_rows") == sum(len(bc.nl_rows_of(p)) for p in items)
    assert {("tape", "up", "above"), ("tape", "lo", "below"), ("tape", "two", "above")} <= T.cut, T.cut
    assert T.rowless == 2
    assert any(len(v) >= 3 for v in T.rounds_with_cuts.values()), T.rounds_with_cuts


def _quad_rounds(items, rounds=4):
    runs, T = run_rounds(items, rounds)
    assert runs[0].fb.m.stat("ecp_blocks_quad_rows") == sum(len(bc.nl_rows_of(p)) for p in items)
    assert {("quad", "up", "above"), ("quad", "two", "above")} <= T.cut, T.cut
    assert any(len(v) >= 3 for v in T.rounds_with_cuts.values()), T.rounds_with_cuts
    return T


def test_rounds_on_quad_rows_with_complete_graphs():
    _quad_rounds(bc.quad_items())


@pytest.mark.parametrize("G", [4, 16, 64])
def test_rounds_on_quad_rows_at_forced_lane_counts(monkeypatch, G):
    """the entry pass with G lanes per Jacobian entry on segments of 1, G - 1, G, G + 1 and 2G + 1 entries"""
    monkeypatch.setenv("KTN_ECP_QUAD_GROUP", str(G))             # (read while the batch is created: every launch of run_rounds)
    _quad_rounds(bc.quad_items(G))


def test_rounds_on_seventy_quad_rows():
    """a second trip of the 16-lanes-per-row value pass: rows beyond slot 63 are judged and cut"""
    T = _quad_rounds(bc.quad_items(many_rows=True))
    assert max(T.slots) >= 64, sorted(T.slots)


def test_rounds_on_tape_quad_and_separable_rows_in_one_instance():
    items = bc.mixed_items()
    runs, T = run_rounds(items)
    assert runs[0].fb.m.stat("ecp_blocks_tape_rows") == 16 and runs[0].fb.m.stat("ecp_blocks_quad_rows") == 16
    assert {k for k, _, _ in T.cut} == {"tape", "quad"}, T.cut
    assert any(len(v) >= 3 for v in T.rounds_with_cuts.values()), T.rounds_with_cuts


def test_two_rounds_on_eleven_hundred_tape_rows():
    """the second trip of the one-lane-per-tape-row loop: slots beyond 1 023 are judged and cut, in the rank scan, the capacity pass
    and the emit pass alike"""
    items = bc.many_tape_rows()
    runs, T = run_rounds(items, 2, bc.MANY_TAPE_CAPACITY)
    assert runs[0].fb.m.stat("ecp_blocks_tape_rows") == bc.MANY_TAPE_ROWS + len(bc.nl_rows_of(items[1]))
    first = set((runs[1].cuts[0]["slot"] - runs[1].nl0[0]).tolist())
    assert max(first) >= 1024 and min(first) < 1024, (min(first), max(first))
    assert len(T.rounds_with_cuts.get(0, ())) == 2, T.rounds_with_cuts
