"""CPU tier: the exact reference of the bound-change screen (tests/rebound_ref.py) against brute force over the box's vertices and
against the conventions of DESIGN.md section 14, and the case builders the GPU tests share (tests/rebound_cases.py)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import rebound_cases as RC
import rebound_ref as R

INF = float("inf")


def test_activity_equals_brute_force_over_the_vertices():
    rng = np.random.default_rng(5)
    l, u, kind = RC.make_bounds(64, rng)
    for trial in range(60):
        L = int(rng.integers(1, 11))
        c = rng.choice(64, L, replace=False)
        v = rng.uniform(-3.0, 3.0, L)
        v[rng.random(L) < 0.2] = 0.0
        big = 2.0 ** 60
        lf = np.where(np.isinf(l[c]), -big, l[c])
        uf = np.where(np.isinf(u[c]), big, u[c])
        amin, amax, S = R.row_activity(v, lf, uf)                      # the reference on the box with the replaced bounds ...
        bmin, bmax = R.brute_force(v, l[c], u[c], big)                 # ... against every vertex of it
        assert amin == bmin and amax == bmax, (trial, amin, bmin, amax, bmax)
        assert S >= abs(amin) and S >= abs(amax)
        amin_i, amax_i, _ = R.row_activity(v, l[c], u[c])              # and with the infinite bounds: infinite exactly where a
        nz = v != 0.0                                                  # non-zero coefficient meets one on that side
        want_min = bool(np.any(nz & np.where(v > 0, np.isinf(l[c]), np.isinf(u[c]))))
        want_max = bool(np.any(nz & np.where(v > 0, np.isinf(u[c]), np.isinf(l[c]))))
        assert (amin_i == -INF) == want_min and (amax_i == INF) == want_max


def test_conventions():
    # a zero coefficient times an infinite bound contributes 0
    assert R.row_activity([0.0, 2.0], [-INF, 1.0], [INF, 3.0]) == (Fraction(2), Fraction(6), Fraction(6))
    # an all-infinite row proves nothing whatever its bounds
    r = R.row_verdict([1.0, -1.0], [-INF, -INF], [INF, INF], 5.0, 4.0, RC.TOL0)
    assert r["amin"] == -INF and r["amax"] == INF and not r["proving"] and not r["redundant"]
    # l = u: amin = amax, the row is an evaluation
    r = R.row_verdict([2.0, -3.0], [1.5, 0.5], [1.5, 0.5], -INF, 1.0, RC.TOL0)
    assert r["amin"] == r["amax"] == Fraction(3, 2) and r["proving"]
    assert not R.row_verdict([2.0, -3.0], [1.5, 0.5], [1.5, 0.5], 1.5, 1.5, RC.TOL0)["proving"]
    # a crossed column keeps the formula (v > 0 takes l for the minimum), and the column count reports it
    amin, amax, _ = R.row_activity([1.0], [2.0], [1.0])
    assert (amin, amax) == (Fraction(2), Fraction(1))
    assert R.screen([0, 1], [0], [1.0], [-INF], [INF], [2.0], [1.0], RC.TOL0)[4] == 1
    # the threshold: tol0 alone for an exact row at zero, and the rounding term grows with the length and the magnitudes
    assert R.tau(0, Fraction(0), 0.0, 3e-7) == 3e-7
    assert R.tau(3, Fraction(8), -8.0, 3e-7) == 3e-7 + (5.0 * 2.0 ** -52) * 16.0
    # a NaN coefficient makes both sides infinite: the row proves nothing and is not redundant
    r = R.row_verdict([1.0, float("nan")], [0.0, 0.0], [1.0, 1.0], 5.0, -5.0, RC.TOL0)
    assert r["amin"] == -INF and r["amax"] == INF and r["S"] == Fraction(1) and not r["proving"] and not r["redundant"]
    # NaN row bounds are vacuous sides
    assert not R.row_verdict([1.0], [0.0], [1.0], float("nan"), float("nan"), RC.TOL0)["proving"]
    # clamp: a crossed column goes to l, moved columns are counted
    assert R.clamp([0.0, 5.0, 1.0, 2.0], [1.0, 0.0, 0.0, 3.0], [2.0, 4.0, 2.0, 1.0]) == ([1.0, 4.0, 1.0, 3.0], 3, 1)


@pytest.mark.parametrize("G", [4, 8, 16, 32, 64])
def test_case_builders(G):
    case = RC.group_case(G)
    assert len(case["lo"]) <= 48 and case["n"] <= 3000
    lens = np.diff(case["rowptr"])
    assert set(RC.group_lengths(G)) == set(int(x) for x in lens)
    assert (max(lens) > RC.K_LONG_ROW) == (G == 64)
    assert any(case["want"]) and not all(case["want"])
    v = case["val"]
    assert np.any(v > 0) and np.any(v < 0) and np.any(v == 0.0)
    rows, count, first, red, crossed = R.screen(case["rowptr"], case["col"], v, case["lo"], case["hi"], case["l"], case["u"], RC.TOL0)
    assert count == sum(case["want"]) and first == case["want"].index(True) and crossed == 0
    infs = [(r["amin"] == -INF, r["amax"] == INF) for r in rows]
    assert (True, False) in infs and (False, True) in infs                # rows with either one infinite side ...
    assert (True, True) in infs and (False, False) in infs               # ... with two, with none
    for L_ in RC.group_lengths(G):                                        # and either one-sided kind at every length the lane groups loop over
        if L_ <= RC.K_LONG_ROW:
            here = {infs[k] for k in range(len(rows)) if lens[k] == L_}
            assert {(True, False), (False, True), (True, True), (False, False)} <= here, (G, L_, here)
    grid = RC.grid_case(G)
    rows = R.screen(grid["rowptr"], grid["col"], grid["val"], grid["lo"], grid["hi"], grid["l"], grid["u"], RC.TOL0)[0]
    for k in range(0, len(rows), 2):                                      # a pair: one float apart, opposite verdicts
        assert rows[k]["proving"] and not rows[k + 1]["proving"]
        side = "hi" if k % 4 == 0 else "lo"
        assert math.nextafter(grid[side][k], grid[side][k + 1]) == grid[side][k + 1]
