"""Case builders of the screen tests (tests/test_rebound_ref.py on the CPU, tests/test_gpu_rebound_screen.py on the GPU): variable
bounds of every kind and LP rows whose verdict is known by construction -- far from the threshold, or one float on either side
of it -- checked against the exact reference (tests/rebound_ref.py) while they are built."""
import math

import numpy as np

import rebound_ref as R

INF = float("inf")
TOL0 = 0.3 * 1e-6                      # lp_tol_floor * f_tol of the default parameters, as the engine forms it
K_LONG_ROW = 2048                      # Engine::kLongRow


def pick_group(avg_len):
    """Engine's pick_group (csrc/engine.hpp)"""
    g = 4
    while g < 64 and 2 * g <= avg_len:
        g <<= 1
    return g


def group_lengths(G):
    """row lengths of a case whose mean length makes pick_group give G: 1, G - 1, G, G + 1, 4 G + 3 -- and under G = 64, where any
    mean from 64 up will do, one row beyond kLongRow"""
    return [1, G - 1, G, G + 1, 4 * G + 3] + ([K_LONG_ROW + 52] if G == 64 else [])


def make_bounds(n, rng, grid=None):
    """column kinds by j mod 8: 0, 5, 6, 7 finite box; 1 l = -inf; 2 u = +inf; 3 free; 4 fixed (l = u).  grid: a power of two all
    finite bounds are multiples of."""
    if grid:
        a = rng.integers(-64, 64, n) * grid
        w = rng.integers(1, 64, n) * grid
    else:
        a = rng.uniform(-5.0, 5.0, n)
        w = rng.uniform(0.1, 4.0, n)
    l, u = a.astype(np.float64), (a + w).astype(np.float64)
    kind = np.arange(n) % 8
    l[(kind == 1) | (kind == 3)] = -INF
    u[(kind == 2) | (kind == 3)] = INF
    u[kind == 4] = l[kind == 4]
    return l, u, kind


def _coefs(k, rng, grid):
    """k non-zero coefficients of both signs"""
    if grid:
        v = rng.integers(1, 32, k) * grid
    else:
        v = rng.uniform(0.05, 3.0, k)
    return v * rng.choice([-1.0, 1.0], k)


def _row(rng, L, kind, grid, flavour):
    """(cols, vals) of one row of L entries.  flavour: 'fin' -- finite and fixed columns under non-zero coefficients, a third of the
    entries (as far as the finite columns reach) on columns with infinite bounds under exact zeros; 'min_inf' -- amin = -inf, amax
    finite; 'max_inf' -- the mirror; 'both_inf' -- free columns among the entries."""
    fin = np.flatnonzero((kind == 0) | (kind >= 4))
    inf_cols = np.flatnonzero((kind >= 1) & (kind <= 3))
    if flavour == "fin":
        k_fin = min(L - L // 3, len(fin))
        cols = np.concatenate([rng.choice(fin, k_fin, replace=False), rng.choice(inf_cols, L - k_fin, replace=False)])
        vals = np.concatenate([_coefs(k_fin, rng, grid), np.zeros(L - k_fin)])
    else:
        # the one-sided columns that send only the wanted side to infinity under a coefficient of the sign given
        k_inf = max(1, L // 4)
        if flavour == "both_inf":
            ic = rng.choice(np.flatnonzero(kind == 3), k_inf, replace=False)
            iv = _coefs(k_inf, rng, grid)
        else:
            lo_open, hi_open = np.flatnonzero(kind == 1), np.flatnonzero(kind == 2)
            ka = k_inf // 2
            ic = np.concatenate([rng.choice(lo_open, k_inf - ka, replace=False), rng.choice(hi_open, ka, replace=False)])
            sgn = np.concatenate([np.ones(k_inf - ka), -np.ones(ka)])          # +v on l = -inf, -v on u = +inf: the MIN side is infinite
            iv = np.abs(_coefs(k_inf, rng, grid)) * (sgn if flavour == "min_inf" else -sgn)
        cols = np.concatenate([ic, rng.choice(fin, L - k_inf, replace=False)])
        vals = np.concatenate([iv, _coefs(L - k_inf, rng, grid)])
        if L >= 4:
            vals[-1] = 0.0                               # an exact zero under a finite column too
    p = rng.permutation(L)
    return cols[p].astype(np.int32), vals[p].astype(np.float64)


def _far(a, sign):
    """a bound a relative 1e-3 away from the activity a, on the side given"""
    return float(a) + sign * 1e-3 * (1.0 + abs(float(a)))


def group_case(G, seed=0, n=3000, tol0=TOL0):
    """Rows of the lengths of group_lengths(G), five per length (two for the long one), with verdicts at least 100 tau from the
    threshold: dict(n, l, u, rowptr, col, val, lo, hi, G, want) -- want[k]: True proving, False not."""
    rng = np.random.default_rng(1000 * G + seed)
    l, u, kind = make_bounds(n, rng)
    rows, lo, hi, want = [], [], [], []
    for L in group_lengths(G):
        flavours = ["fin", "fin", "min_inf", "max_inf", "both_inf"] if L <= K_LONG_ROW else ["fin", "fin"]
        for t, fl in enumerate(flavours):
            c, v = _row(rng, L, kind, None, fl)
            amin, amax, _ = R.row_activity(v, l[c], u[c])
            if fl == "fin" and t == 0:                   # impossible through its upper side; the lower side is open
                b_lo, b_hi, w = -INF, _far(amin, -1.0), True
            elif fl == "fin":                            # feasible, tight on one side, loose on the other
                tight = L % 2 == 1 and float(amax) - float(amin) > 0.1
                b_lo, b_hi, w = (_far(amin, +1.0) if tight else float(amin) - 1.0), float(amax) + 1.0, False
            elif fl == "min_inf":                        # amin = -inf: only the lower side can prove -- and does
                b_lo, b_hi, w = _far(amax, +1.0), INF, True
            elif fl == "max_inf":
                b_lo, b_hi, w = -INF, _far(amin, -1.0), True
            else:                                        # both infinite: nothing can be proven whatever the bounds
                b_lo, b_hi, w = 1.0, 2.0, False
            rows.append((c, v)); lo.append(b_lo); hi.append(b_hi); want.append(w)
    case = _assemble(n, l, u, rows, lo, hi, G, want)
    for k, r in enumerate(R.screen(case["rowptr"], case["col"], case["val"], case["lo"], case["hi"], l, u, tol0)[0]):
        assert r["proving"] == want[k], (G, k)
        for ex, t in ((r["ex_hi"], r["t_hi"]), (r["ex_lo"], r["t_lo"])):         # at least 100 tau away on either side (or undecidable: infinite)
            assert not math.isfinite(ex) or ex >= 100.0 * t or ex <= -100.0 * t, (G, k, ex, t)
    return case


def _assemble(n, l, u, rows, lo, hi, G, want):
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64)
    assert pick_group(rowptr[-1] / len(rows)) == G, (G, rowptr[-1] / len(rows))
    return dict(n=n, l=l, u=u, rowptr=rowptr, col=np.concatenate([c for c, _ in rows]).astype(np.int32),
                val=np.concatenate([v for _, v in rows]).astype(np.float64), lo=np.asarray(lo, dtype=np.float64),
                hi=np.asarray(hi, dtype=np.float64), G=G, want=list(want))


def _threshold_pair(proving_at, sure, never):
    """the two neighbouring floats between `sure` (proving) and `never` (not proving) where the verdict flips: (last proving, first not)"""
    a, b = float(sure), float(never)
    assert proving_at(a) and not proving_at(b)
    while True:
        mid = 0.5 * (a + b)
        if mid == a or mid == b:
            return a, b
        if proving_at(mid):
            a = mid
        else:
            b = mid


def grid_case(G, seed=0, n=1024, tol0=TOL0):
    """Dyadic-grid rows (every bound a multiple of 2^-4, every coefficient of 2^-3: every sum is exact in any order) in pairs whose
    row bound sits one float on either side of the threshold: through the upper side (rows 4 i, 4 i + 1) and through the lower side
    (4 i + 2, 4 i + 3).  Lengths as in group_case without the long row."""
    rng = np.random.default_rng(7000 * G + seed)
    l, u, kind = make_bounds(n, rng, grid=2.0 ** -4)
    rows, lo, hi, want = [], [], [], []
    for L in [x for x in group_lengths(G) if x <= K_LONG_ROW]:
        c, v = _row(rng, L, kind, 2.0 ** -3, "fin")
        amin, amax, _ = R.row_activity(v, l[c], u[c])
        amin, amax = float(amin), float(amax)
        up = lambda b: R.row_verdict(v, l[c], u[c], -INF, b, tol0)["proving"]
        dn = lambda b: R.row_verdict(v, l[c], u[c], b, INF, tol0)["proving"]
        h1, h0 = _threshold_pair(up, amin - 1.0, amin)
        l1, l0 = _threshold_pair(dn, amax + 1.0, amax)
        for b_lo, b_hi, w in ((-INF, h1, True), (-INF, h0, False), (l1, INF, True), (l0, INF, False)):
            rows.append((c, v)); lo.append(b_lo); hi.append(b_hi); want.append(w)
    return _assemble(n, l, u, rows, lo, hi, G, want)
