"""CPU tier: the plain-Python model of k_blocks_rewarm (tests/blocks_warm_ref.py) -- eligibility, the screen, the clamp, the idle
test, the compaction and the relink -- on small hand-built arenas and on seeded random ones, and the invariants every compaction
must keep: links strictly descend, every list's multipliers are conserved, nothing moves at or below half fill, linear rows never
move.  Every deliberate defect the model can be given (MUTATIONS) is told from it by at least one of these checks."""
import random

import pytest

import blocks_warm_ref as W

TOL0, MARGIN = 1e-8, 1e-3
N = 6                                                       # columns of the hand-built instance: x in [0, 1]^6


def hand_arena(cap_rows=2 + 8, status=W.STATUS_OPTIMAL, overflow=0, lam=False):
    """two linear rows, six cuts of two NL slots; at x = (0.5, ...) the cuts 3, 4 (adjacent), 7 (a list head) are idle:
         row  slot  y     a'x       hi
          2    0    0.0   0.50    0.50   tight (slack 0)
          3    0    0.0   0.50    2.00   idle
          4    1    0.0   0.50    3.00   idle
          5    1   -0.7   1.00    1.00   active
          6    0   -0.2   0.25    0.25   active, slot 0's survivor head
          7    0    0.0   0.50    9.00   idle, slot 0's head"""
    cols = [[0, 1], [2, 3, 4], [0], [1], [2], [3, 4], [5], [0]]
    vals = [[1.0, 1.0], [1.0, -1.0, 1.0], [1.0], [1.0], [1.0], [1.0, 1.0], [0.5], [1.0]]
    lo = [-W.INF] * 8
    hi = [1.5, 0.75, 0.5, 2.0, 3.0, 1.0, 0.25, 9.0]
    y = [0.0, -0.1, 0.0, 0.0, 0.0, -0.7, -0.2, 0.0]
    prev = [-1, -1, -1, 2, -1, 4, 3, 6]
    last = [7, 5]
    return W.Arena(2, cap_rows, cols, vals, lo, hi, y, prev, last, [1.0, 1.0, 1.0, 0.5, 0.25, 1.0, 0.75, 1.0] if lam else None, status, overflow)


BOX = ([0.0] * N, [1.0] * N)
X = [0.5] * N


def run(a, l=BOX[0], u=BOX[1], x=X, mut=None):
    return W.rewarm(a, l, u, x, TOL0, MARGIN, mut)


def test_eligibility_only_an_optimal_record_without_overflow_is_warm():
    for status, overflow in ((2, 0), (W.STATUS_OPTIMAL, 1), (0, 0)):
        a = hand_arena(status=status, overflow=overflow)
        rec, after, x = run(a, x=[2.0] * N)
        assert rec == [0, 8, a.nnz, 0, 0, -1, 0, 0] and x == [2.0] * N              # nothing touched, x not even clamped
        assert after.hi == a.hi and after.prev == a.prev and after.last == a.last


def test_crossed_columns_end_the_instance_before_anything_else():
    l = [0.0, 0.6, 0.0, 0.0, 0.9, 0.0]
    u = [1.0, 0.5, 1.0, 1.0, 0.8, 1.0]
    rec, after, x = run(hand_arena(), l, u, [5.0] * N)
    assert rec[0] == 2 and rec[6] == 2 and rec[3] == rec[4] == 0 and rec[5] == -1 and x == [5.0] * N and after.M == 8


def test_clamp_counts_the_columns_it_moves():
    rec, _, x = run(hand_arena(cap_rows=2 + 20), x=[-1.0, 0.5, 2.0, 1.0, 0.0, 0.25])
    assert rec[0] == 1 and rec[4] == 2 and x == [0.0, 0.5, 1.0, 1.0, 0.0, 0.25]


def test_screen_finds_the_smallest_proving_row_among_linear_rows_and_cuts():
    # x0 >= 0.9: cut 2 (x0 <= 0.5) is impossible by 0.4, far above tau ~ 1e-8; x0 + x1 <= 1.5 with x1 >= 0.8 as well: row 0 by 0.2
    l = [0.9, 0.0, 0.0, 0.0, 0.0, 0.0]
    rec, after, x = run(hand_arena(), l, BOX[1])
    assert rec[0] == 2 and rec[5] == 2 and rec[3] == 0 and after.M == 8 and x[0] == 0.9 and rec[4] == 1
    l = [0.9, 0.8, 0.0, 0.0, 0.0, 0.0]
    assert run(hand_arena(), l, BOX[1])[0][5] == 0
    # a violation below the threshold proves nothing: x0 >= 0.5 + 5e-9
    rec = run(hand_arena(cap_rows=2 + 20), [0.5 + 5e-9] + [0.0] * 5, BOX[1])[0]
    assert rec[0] == 1 and rec[5] == -1
    assert run(hand_arena(cap_rows=2 + 20), [0.5 + 5e-9] + [0.0] * 5, BOX[1], mut="screen_no_tau")[0][0] == 2


def test_redundant_rows_are_counted_not_removed():
    rec, after, _ = run(hand_arena(cap_rows=2 + 20))
    # over [0, 1]^6: rows 3 (x1 <= 2), 4 (x2 <= 3), 7 (x0 <= 9) can never bind; row 1 (x2 - x3 + x4 <= 0.75) can, as the rest
    assert rec[7] == 3 and after.M == 8 and rec[3] == 0


def test_compaction_drops_a_list_head_and_two_adjacent_rows_and_relinks():
    a = hand_arena(lam=True)
    rec, after, _ = run(a)
    assert rec == [1, 5, 2 + 3 + 1 + 2 + 1, 3, 0, -1, 0, 3]
    assert after.hi == [1.5, 0.75, 0.5, 1.0, 0.25] and after.y == [0.0, -0.1, 0.0, -0.7, -0.2] and after.lam == [1.0, 1.0, 1.0, 1.0, 0.75]
    assert after.cols == [[0, 1], [2, 3, 4], [0], [3, 4], [5]]
    assert after.last == [4, 3] and after.prev == [-1, -1, -1, -1, 2]              # slot 0: 6 -> 2 became 4 -> 2; slot 1: its tail went
    assert after.slots() == [-1, -1, 0, 1, 0]
    W.check_invariants(a, after, rec)


def test_a_list_whose_rows_all_went_ends_at_minus_one():
    a = hand_arena()
    a.y[5] = 0.0
    a.hi[5] = 4.0                                              # slot 1's only active cut is idle now: both its rows go
    rec, after, _ = run(a)
    assert rec[3] == 4 and after.last == [3, -1] and after.prev == [-1, -1, -1, 2]
    W.check_invariants(a, after, rec)


def test_nothing_moves_at_or_below_half_fill():
    a = hand_arena(cap_rows=2 + 12)                            # 6 cuts in room for 12: exactly half
    rec, after, _ = run(a)
    assert rec[0] == 1 and rec[3] == 0 and after.M == 8 and after.prev == a.prev and after.last == a.last
    b = hand_arena(cap_rows=2 + 11)                            # 6 > 11 // 2
    assert run(b)[0][3] == 3


def test_idle_is_strict_and_needs_a_zero_multiplier():
    a = hand_arena()
    a.hi[3] = 0.5 + MARGIN * 1.0                               # slack == margin * scale exactly: 0.501 - 0.5 rounds to it or not --
    slack = a.hi[3] - 0.5                                      # take the slack the floats give and put the margin on it
    assert W.idle_row(a.cols[3], a.vals[3], a.lo[3], a.hi[3], 0.0, X, slack) is False
    assert W.idle_row(a.cols[3], a.vals[3], a.lo[3], a.hi[3], 0.0, X, slack, ge=True) is True
    assert W.idle_row(a.cols[3], a.vals[3], a.lo[3], a.hi[3], -1e-300, X, 0.5 * slack) is False
    # a row without a finite bound is slack by +inf; a NaN activity is passed over by min: slack stays +inf
    assert W.idle_row([0], [1.0], -W.INF, W.INF, 0.0, X, MARGIN) is True


def random_arena(rng, m_lin, n_slots, n_cuts, cap_mul, n):
    cols, vals, lo, hi, y, prev = [], [], [], [], [], []
    for _ in range(m_lin):
        k = rng.randint(1, 5)
        cols.append(rng.sample(range(n), k)); vals.append([rng.choice((-1.0, 1.0)) * rng.uniform(0.5, 2.0) for _ in range(k)])
        lo.append(-W.INF); hi.append(50.0); y.append(rng.choice((0.0, -0.3))); prev.append(-1)
    last = [-1] * n_slots
    for r in range(m_lin, m_lin + n_cuts):
        k = rng.randint(1, 6)
        c = rng.sample(range(n), k)
        v = [rng.uniform(0.25, 1.5) for _ in range(k)]
        ax = sum(vv * 0.5 for vv in v)
        kind = rng.choice(("idle", "idle", "tight", "active"))
        cols.append(c); vals.append(v); lo.append(-W.INF)
        hi.append(ax + (rng.uniform(0.5, 3.0) if kind == "idle" else 0.0))
        y.append(-rng.uniform(0.1, 1.0) if kind == "active" else 0.0)
        s = rng.randrange(n_slots)
        prev.append(last[s]); last[s] = r
    return W.Arena(m_lin, m_lin + cap_mul * n_slots, cols, vals, lo, hi, y, prev, last, [rng.uniform(0.1, 1.0) for _ in cols])


@pytest.mark.parametrize("seed", range(12))
def test_invariants_on_random_arenas(seed):
    rng = random.Random(seed)
    n = 12
    n_slots = rng.randint(1, 5)
    cap_mul = rng.randint(3, 8)
    a = random_arena(rng, rng.randint(0, 4), n_slots, rng.randint(0, cap_mul * n_slots), cap_mul, n)
    rec, after, x = W.rewarm(a, [0.0] * n, [1.0] * n, [0.5] * n, TOL0, MARGIN)
    assert rec[0] == 1
    W.check_invariants(a, after, rec)
    rec2, after2, _ = W.rewarm(after, [0.0] * n, [1.0] * n, x, TOL0, MARGIN)       # a second pass finds nothing left to drop
    assert rec2[3] == 0 and after2.hi == after.hi and after2.prev == after.prev and after2.last == after.last


@pytest.mark.parametrize("mut", [m for m in W.MUTATIONS if m != "screen_no_tau"])
def test_every_defect_is_told_from_the_model(mut):
    """some arena among the hand-built and the random ones on which the defective model breaks an invariant or differs from the model"""
    told = False
    arenas = [hand_arena(lam=True), hand_arena(cap_rows=2 + 12)]
    arenas[0].y[3] = -0.4                                      # a slack cut that still carries a multiplier: it stays
    rng = random.Random(99)
    arenas += [random_arena(rng, 2, 3, 3 * k, 6, 12) for k in range(2, 7)]
    for a, margin in [(a, mg) for a in arenas for mg in (MARGIN, 0.0)]:      # (margin 0: a tight row sits exactly on the idle threshold)
        n = 12 if a is not arenas[0] and a is not arenas[1] else N
        good = W.rewarm(a, [0.0] * n, [1.0] * n, [0.5] * n, TOL0, margin)
        bad = W.rewarm(a, [0.0] * n, [1.0] * n, [0.5] * n, TOL0, margin, mut)
        differs = bad[0] != good[0] or bad[1].hi != good[1].hi or bad[1].prev != good[1].prev or bad[1].last != good[1].last
        try:
            W.check_invariants(a, bad[1], bad[0])
            broke = False
        except AssertionError:
            broke = True
        told = told or differs or broke
    assert told, mut
