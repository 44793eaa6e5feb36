"""CPU tier: the rule of ktn_set_row_bounds (tests/rowbound_ref.py) -- its accuracy against exact rational arithmetic, its
identity cases and its validation.

Accuracy.  hi was stored as fl(ub - b); the setter forms d = fl(ub' - ub) and stores fl(hi + d); a fresh cut would get ub' - b.
With u = 2^-53, rounding to nearest gives |fl(z) - z| <= half an ulp of fl(z) <= u |fl(z)| and the sharper |fl(z) - z| <= u |z| / (1 + u):
    |hi - (ub - b)| <= u |hi|                                   (the first form)
    |d - (ub' - ub)| <= u |ub' - ub| / (1 + u),  hence  |d| <= |ub' - ub| (1 + u)
    |fl(hi + d) - (hi + d)| <= u (|hi| + |d|) / (1 + u) <= u (|hi| + |ub' - ub|)
Since ub' - b = (ub - b) + (ub' - ub), the three add up to
    |fl(hi + d) - (ub' - b)| <= 2 u (|hi| + |ub' - ub|) = 2^-52 (|hi| + |ub' - ub|).
Measured over the 20 000 draws below: the worst ratio error / bound is 0.963 (seed 7)."""
import math
import random
from fractions import Fraction

import pytest

import rowbound_ref as R
from pool_ref import PoolRef

INF = math.inf


def draws(seed, count):
    rng = random.Random(seed)
    for _ in range(count):
        scale = 10.0 ** rng.uniform(-6, 6)
        ub, b = rng.uniform(-1, 1) * scale, rng.uniform(-1, 1) * 10.0 ** rng.uniform(-6, 6)
        nub = ub + rng.uniform(-1, 1) * 10.0 ** rng.uniform(-8, 6)
        yield ub, b, nub


def test_shift_is_within_the_derived_bound_of_the_exact_fresh_cut():
    worst = Fraction(0)
    for ub, b, nub in draws(7, 20000):
        hi = ub - b                                                               # rounded once, as the cut was stored
        got = R.shift(hi, ub, nub)
        exact = Fraction(nub) - Fraction(b)
        bound = Fraction(2) ** -52 * (abs(Fraction(hi)) + abs(Fraction(nub) - Fraction(ub)))
        err = abs(Fraction(got) - exact)
        assert err <= bound, (ub, b, nub, float(err), float(bound))
        if bound > 0:
            worst = max(worst, err / bound)
    print("worst error / bound: %.3f" % float(worst))
    assert 0 < worst <= 1


def test_equal_sides_and_zero_deltas_are_the_identity():
    for v in (1.5, -0.0, 0.0, INF, -INF, 1e-320):
        for b in (2.0, INF, -INF, -0.0, 0.0):
            got = R.shift(v, b, b)
            assert math.copysign(1.0, got) == math.copysign(1.0, v) and (got == v)      # bit for bit, the sign of a zero included
    assert R.shift(INF, INF, INF) == INF and R.shift(-INF, -INF, -INF) == -INF            # no inf - inf
    assert R.shift(3.0, 0.0, -0.0) == 3.0                                                  # -0.0 == 0.0: not written


def pool_with_lists():
    p = PoolRef([([0], [1.0], -INF, 4.0)], n_lists=3)                                      # row 0: a linear row, in no list
    rows = [([0, 1], [1.0, 2.0], -INF, 1.0), ([1, 2], [0.5, 1.0], -2.0, 2.0), ([0, 1], [1.5, 1.0], -INF, 0.75)]
    p.append(rows, [0, 1, 2], inherit=False)
    p.append([([0, 1], [0.5, 2.5], -INF, 1.25), ([2], [1.0], -INF, 8.0)], [0, -1], inherit=False)      # a second cut of list 0, a row without id
    return p


def test_rebase_moves_list_rows_only_and_only_changed_sides():
    p = pool_with_lists()
    list_row = [2, 3, 5]                                                                   # the constraint of each list
    lb = [0.0, -INF, -INF, 0.0, 0.0, -INF]
    ub = [1.0, 4.0, 3.0, 4.0, 1.0, 1.0]
    nlb, nub = list(lb), list(ub)
    nub[2] = 3.5                                                                           # list 0: both of its cuts
    nlb[3], nub[3] = 0.25, 4.0                                                             # list 1: the lower side alone
    before = (list(p.lo), list(p.hi))
    assert R.owners(p, list_row) == [-1, 2, 3, 5, 2, -1]
    moved = R.rebase(p, list_row, lb, ub, nlb, nub)
    assert moved == 3
    assert p.hi == [4.0, 1.5, 2.0, 0.75, 1.75, 8.0]
    assert p.lo == [-INF, -INF, -1.75, -INF, -INF, -INF]
    assert R.rebase(p, list_row, nlb, nub, nlb, nub) == 0                                  # the bounds in force again: nothing moves
    p2 = pool_with_lists()
    assert R.rebase(p2, list_row, lb, ub, lb, ub) == 0 and (p2.lo, p2.hi) == before


@pytest.mark.parametrize("old,new,ok", [
    ((-INF, 1.0), (-INF, 2.0), True), ((-INF, 1.0), (-INF, INF), False), ((-INF, 1.0), (0.0, 1.0), False),
    ((0.0, 1.0), (-1.0, 3.0), True), ((0.0, 1.0), (0.0, INF), False), ((0.0, INF), (0.5, INF), True),
    ((-INF, 1.0), (INF, 1.0), False), ((0.0, 1.0), (2.0, 1.0), True)])
def test_a_nonlinear_row_may_not_gain_or_lose_a_side(old, new, ok):
    code, crossed, lin = R.validate([old[0]], [old[1]], [new[0]], [new[1]], [True])
    assert (code == R.E_OK) == ok and not lin
    if ok:
        assert crossed == (1 if new[0] > new[1] else 0)


def test_linear_rows_are_free_and_crossed_rows_are_counted():
    lb, ub = [-INF, 0.0, 0.0], [1.0, INF, 2.0]
    code, crossed, lin = R.validate(lb, ub, [0.0, -INF, 3.0], [INF, 5.0, 2.0], [False, False, False])
    assert (code, crossed, lin) == (R.E_OK, 1, True)
    assert R.validate(lb, ub, lb, ub, [False, True, False]) == (R.E_OK, 0, False)
    assert R.validate(lb, ub, [math.nan, 0.0, 0.0], ub, [False, False, False])[0] == R.E_INVALID
