"""CPU tier of the cut-pool tests: the plain-Python model of the pool (tests/pool_ref.py) run over every script of
tests/pool_cases.py -- its invariants, the outcomes the scripts are built for, and that the scripts tell every listed defect
(pool_ref.MUTATIONS, applied to the model itself) from the model.  tests/test_gpu_pool.py runs the same scripts on the engine."""
import math

import pytest

import pool_cases as PC
import pool_ref


@pytest.fixture(scope="module")
def scripts():
    return PC.all_scripts()                    # (building them asserts the threshold gaps of every row of every purge)


def by_name(scripts, name):
    return next(S for S in scripts if S.name == name)


def weighted(m, s):
    """sum over list s of y * (largest |coefficient|): what dedupe's  y[head] += y[r] * nr / nh  conserves"""
    rows = m.list_rows(s)
    if any(m.row_norm(r) is None for r in rows):
        return None
    return sum(m.y[r] * m.row_norm(r) for r in rows)


def test_invariants_after_every_step(scripts):
    for S in scripts:
        ids = {}
        base = PC.snapshot(S.new_model())
        m_prev = ([0.0] * S.n_lists, [-1] * S.n_lists, [0.0] * S.n_lists)
        for i, step, m, out in PC.run_model(S):
            what = (S.name, i, step[0])
            if step[0] == "append":
                ids.update({t: g for t, g in zip(step[3], step[2]) if 0 <= g < S.n_lists})
            # lists: strictly descending (list_rows asserts it), newest first, every row with an id in exactly its own list
            seen = {}
            for s in range(S.n_lists):
                rows = m.list_rows(s)
                assert rows == sorted(rows, reverse=True) and all(r >= m.M_base for r in rows), what
                for r in rows:
                    assert r not in seen and ids.get(m.tag[r]) == s, (what, r, s)
                    seen[r] = s
            assert sorted(seen) == [r for r in range(m.M) if m.tag[r] in ids], what
            # base rows never move
            assert m.tag[:m.M_base] == ["base%d" % k for k in range(m.M_base)], what
            head = lambda snap: (snap[0][:m.M_base + 1], snap[1][:snap[0][m.M_base]], snap[2][:snap[0][m.M_base]], snap[3][:m.M_base], snap[4][:m.M_base])
            assert head(PC.snapshot(m)) == head(base), what
            assert len(m.y) == len(m.age) == len(m.prev) == m.M and S.after[i] == m.tag, what
            if step[0] == "append" and S.params["lp_dual_inherit"]:
                for s in range(S.n_lists):                         # the list's multiplier mass moves to the new head, none is lost
                    assert m.list_sums()[s] == m_prev[0][s], (what, s)
                    if m_prev[1][s] >= 0 and m.heads[s] != m_prev[1][s]:
                        assert m.y[m_prev[1][s]] == 0.0, (what, s)
            if step[0] == "purge":
                for s in range(S.n_lists):                         # dedupe conserves y * norm over each list (rows that aged out had y = 0)
                    if m_prev[2][s] is not None and weighted(m, s) is not None:
                        assert math.isclose(weighted(m, s), m_prev[2][s], rel_tol=1e-12, abs_tol=0.0), (what, s)
            m_prev = (m.list_sums(), list(m.heads), [weighted(m, s) for s in range(S.n_lists)])


def test_ageing_outcomes(scripts):
    for p in (1, 2, 3):
        S = by_name(scripts, "ageing/p%d/plain" % p)
        purges = [i for i, st in enumerate(S.steps) if st[0] == "purge"]
        gone = {t: 1 + k for k, i in reversed(list(enumerate(purges))) for t in set(S.after[i - 1]) - set(S.after[i])}
        e = S.expect
        assert len(purges) == e["calls"] and gone["reset"] == e["reset_gone_at"] == e["reset_tight_at"] + p
        for t in ("idle0", "idle1", "idle2", "both_idle", "nan_bound", "empty_idle", "float0", "float2"):
            assert gone[t] == p, (p, t, gone)                      # idle on every call: gone at call purge_age
        kept = S.after[-1]
        for t in ("has_y", "on_margin", "in_margin", "both_tight", "empty_tight", "float1", "float3"):
            assert t in kept, (p, t)
        assert S.exact_ties == e["calls"]                          # the row with slack == margin * scale, at every call
        assert any(S.model.slack_scale(r, PC.grid_x(12))[0] > PC.MARGIN * S.model.slack_scale(r, PC.grid_x(12))[1]
                   for r in range(S.model.M_base)), "no base row is idle"
    S = by_name(scripts, "ageing/p2/min_frac")
    assert S.removed == [0, 0, 12, 0]
    purges = [i for i, st in enumerate(S.steps) if st[0] == "purge"]
    assert S.after[purges[1]] == S.after[purges[1] - 1] and "late0" not in S.after[purges[2]] and "idle0" not in S.after[purges[2]]
    S = by_name(scripts, "ageing/p2/min_rows")
    assert S.removed == [0] * 4 and S.model.age == [0] * S.model.M and S.model.stats["purges"] == 0


def test_dedupe_outcomes(scripts):
    S = by_name(scripts, "dedupe/eps%g" % PC.EPS)
    purge = next(i for i, st in enumerate(S.steps) if st[0] == "purge")
    dropped = set(S.after[purge - 1]) - set(S.after[purge])
    assert dropped == {"l0_times3", "l0_within", "l1_half", "l2_head_idle"}, dropped
    ms = [m for _, _, m, _ in PC.run_model(S)]                    # (one model, stepped: look at it at the end)
    m = ms[-1]
    y = dict(zip(m.tag, m.y))
    # the new head of every list took what the old head held after the purge: its own y plus the scaled y of its duplicates
    pt = next(st for st in S.steps if st[0] == "point")
    y0 = dict(zip(S.after[purge - 1], pt[2]))
    assert y["new0"] == y0["l0_head"] + y0["l0_times3"] * 3.0 + y0["l0_within"] * 1.0 and y["l0_head"] == 0.0
    assert y["new1"] == y0["l1_head"] + y0["l1_half"] * 0.5 and y["l1_head"] == 0.0
    assert y["new2"] == y0["l2_dup_b"] and y["l2_dup_a"] == y0["l2_dup_a"]          # the head went by age: the next row is the head
    assert y["new3"] == y0["l3_zero_head"] and y["new4"] == y0["l4_nan_head"]
    S0 = by_name(scripts, "dedupe/eps0")
    assert S0.model.stats["deduped_rows"] == 0 and S0.removed == [1]


def test_truncate_and_relink_outcomes(scripts):
    S = by_name(scripts, "truncate")
    m = S.model
    y = dict(zip(m.tag, m.y))
    assert [m.tag[r] for r in m.list_rows(0)] == ["g5", "g4"] and [m.tag[r] for r in m.list_rows(1)] == ["h4", "h3", "h0"]
    assert [m.tag[r] for r in m.list_rows(2)] == ["k2", "k1"]
    assert y["g5"] == -0.375 + (-0.5) * (4.0 / 2.0) and y["g4"] == 0.0           # g1 (y -0.5, norm 4) merged into g4 (norm 2)
    R = by_name(scripts, "relink")
    assert [R.model.tag[r] for r in R.model.list_rows(0)] == ["new0", "a"]
    assert [R.model.tag[r] for r in R.model.list_rows(1)] == ["new1", "e", "d", "c"]


CAUGHT_BY = {"keep_le": "ageing/", "age_no_reset": "ageing/", "idle_ge": "ageing/", "dedupe_no_scale": "dedupe/", "dedupe_vs_previous": "dedupe/",
             "relink_no_tail": "relink", "copy_short": "groups/", "clip_keeps_head": "truncate"}


@pytest.mark.parametrize("mut", sorted(CAUGHT_BY))
def test_the_scripts_tell_each_defect_from_the_model(scripts, mut):
    """every listed defect, applied to the model, changes what the engine would show (rows, bounds, multipliers, counters, the
    value a purge returns) in at least one script of the family built for it -- or breaks a list"""
    caught = []
    for S in scripts:
        good = [(PC.snapshot(m), out) for _, _, m, out in PC.run_model(S)]
        try:
            bad = []
            for _, _, m, out in PC.run_model(S, mut):
                bad.append((PC.snapshot(m), out))
                for s in range(S.n_lists):
                    m.list_rows(s)
        except (AssertionError, IndexError):
            caught.append(S.name)
            continue
        if bad != good:
            caught.append(S.name)
    assert any(name.startswith(CAUGHT_BY[mut]) for name in caught), (mut, caught)
    if mut == "copy_short":                                               # the lane tail, at every lane-group width
        assert {"groups/G%d" % G for G in PC.GROUPS} <= set(caught), caught


def test_lane_groups_of_the_group_scripts(scripts):
    for G in PC.GROUPS:
        S = by_name(scripts, "groups/G%d" % G)
        assert S.groups[0] == G and S.model.stats["deduped_rows"] == 5 and S.model.stats["purges"] == 2
        lens = {len(c) for st in S.steps if st[0] == "append" for c, _, _, _ in st[1]}
        assert {0, 1, G - 1, G, G + 1, 2 * G + 1} <= lens


def test_select_deepest():
    P = pool_ref.PoolRef([], 0)
    depths = [0.5, 0.0, 0.25, 0.25, 0.25, 1.0, -0.125, 0.125, 2.0]
    flagged = [True, False, True, True, True, True, True, True, True]
    assert P.select_deepest(depths, flagged, 8) == ([0, 2, 3, 4, 5, 6, 7, 8], False)         # no more flagged than the cap: no selection
    assert P.select_deepest(depths, flagged, 4) == ([0, 2, 3, 4, 5, 8], True)                # the three ties at the threshold all stay
    assert P.select_deepest(depths, flagged, 3) == ([0, 5, 8], True)
    assert P.select_deepest(depths, flagged, 7) == ([0, 2, 3, 4, 5, 7, 8], True)             # depth <= 0: the smallest key, first to go
    assert pool_ref.depth_key(0.0) == 0 and pool_ref.depth_key(5e-324) == 1
    bad = pool_ref.PoolRef([], 0, mut="reflag_le")
    assert bad.select_deepest(depths, flagged, 4) == ([0, 5, 8], True)
    C, d, flagged, kept, selected = PC.selection_plan(8)
    assert selected and len(kept) == 9 and {22, 25, 33} <= set(kept) and 35 not in kept and flagged[35]
    assert bad.select_deepest(d.tolist(), flagged.tolist(), 8)[0] != kept
    assert PC.selection_plan(1000)[3:] == (list(map(int, flagged.nonzero()[0])), False)


def test_engine_list_plan_and_the_mirror_script(scripts):
    for inherit in (0, 1):
        C, sweeps, m, removed = PC.engine_lists_plan(inherit)
        assert [len(s) for s in sweeps] == [30, 30, 30] and removed == 11 and m.stats["deduped_rows"] == 7
        for s in range(40):
            m.list_rows(s)
    S = by_name(scripts, "mirror")
    assert S.csc == [(1, 0), (1, 1), (1, 2), (1, 3), (2, 3), (3, 3), (3, 4)]
    # the column sum in row order against the order the append-only update receives the entries in (its ordering pass removed)
    assert pool_ref.lane_group_sum([1.0, PC.BIG, -PC.BIG], 4) != pool_ref.lane_group_sum([1.0, -PC.BIG, PC.BIG], 4)
    assert pool_ref.lane_group_sum([0.5, 0.25, 0.125, 1.0, 2.0], 4) == 3.875
