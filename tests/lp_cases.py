"""LPs and states for the LP kernel tests (tests/test_lp_ref.py on the CPU, tests/test_gpu_lp_kernels.py on the GPU).

Every case is an `lp_ref.LP` plus a state: x, y, anchors x0 != x, y0 != y, eta, omega.  Values spread over four decades; rows
cycle through <=, ranged, equality, free (both sides infinite), NaN-sided and >=; variables through boxed, lower-only,
upper-only, free and fixed; every second dual starts sign-INfeasible; x starts partly outside its box (the prep kernel clips).
"""
import functools

import numpy as np

import lp_ref

INF = float("inf")
K_LONG = 2048                                    # Engine::kLongRow
# 0, 1 and G - 1, G, G + 1, 2G + 3 for G = 4 ... 64, and 200
EDGE_LENGTHS = sorted({0, 1, 200} | {v for g in (4, 8, 16, 32, 64) for v in (g - 1, g, g + 1, 2 * g + 3)})


def _values(rng, k):
    return rng.choice([-1.0, 1.0], k) * 10.0 ** rng.uniform(-2.0, 2.0, k)


def _finish(rng, rows, n, sense, eta=2e-3, omega=1.7):
    """rows: list of sorted column arrays -> the LP with cycled row / variable kinds and a state"""
    m = len(rows)
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int64) if m else np.zeros(0, dtype=np.int64)
    val = _values(rng, len(col))
    mid = rng.normal(size=m) * 3.0
    wid = rng.uniform(0.5, 4.0, m)
    lo, hi = mid - wid, mid + wid
    kind = np.arange(m) % 6
    lo[kind == 0] = -INF                                     # <=
    lo[kind == 2] = hi[kind == 2]                            # equality
    lo[kind == 3] = -INF; hi[kind == 3] = INF                # free
    lo[kind == 4] = np.nan                                   # NaN side: vacuous
    hi[kind == 5] = INF                                      # >=
    vk = np.arange(n) % 5
    l, u = rng.uniform(-3.0, -0.5, n), rng.uniform(0.5, 3.0, n)
    u[vk == 1] = INF; l[vk == 2] = -INF
    l[vk == 3] = -INF; u[vk == 3] = INF
    u[vk == 4] = l[vk == 4]                                  # fixed
    c = _values(rng, n) * 0.1
    lp = lp_ref.LP(rowptr, col, val, lo, hi, c, l, u, sense)
    lp.lo_raw, lp.hi_raw = lo, hi                            # (with the NaNs, as the handle gets them)
    x, x0 = rng.normal(size=n) * 2.5, rng.normal(size=n) * 2.5
    y, y0 = rng.normal(size=m), rng.normal(size=m)
    sign_ok = np.arange(m) % 2 == 0                          # every second dual sign-feasible, the others as drawn
    flo, fhi = np.isfinite(lp.lo), np.isfinite(lp.hi)
    for v in (y, y0):
        v[sign_ok & ~flo] = np.minimum(v[sign_ok & ~flo], 0.0)
        v[sign_ok & ~fhi] = np.maximum(v[sign_ok & ~fhi], 0.0)
    return dict(lp=lp, x=x, y=y, x0=x0, y0=y0, eta=eta, omega=omega)


def _pick(rng, lo, hi, k):
    return np.sort(rng.choice(np.arange(lo, hi), size=k, replace=False))


@functools.lru_cache(maxsize=None)
def ragged(sense="Min"):
    """517 x 389: rows [0, 300) take every edge length from columns [40, 389); columns [0, 40) take every edge length from rows
    [300, 517), which also hold a few entries of their own"""
    rng = np.random.default_rng(11)
    m, n, r0, c0 = 517, 389, 300, 40
    rows = [_pick(rng, c0, n, EDGE_LENGTHS[i % len(EDGE_LENGTHS)]) for i in range(r0)]
    low = [[] for _ in range(m - r0)]
    for j in range(c0):
        for i in _pick(rng, 0, m - r0, EDGE_LENGTHS[j % len(EDGE_LENGTHS)]):
            low[i].append(j)
    for i in range(m - r0):
        rows.append(np.array(sorted(low[i]) + list(_pick(rng, c0, n, i % 4)), dtype=np.int64))
    case = _finish(rng, rows, n, sense)
    lp = case["lp"]
    assert set(EDGE_LENGTHS) <= set(lp.rlen.tolist()) and set(EDGE_LENGTHS) <= set(lp.clen[:c0].tolist())
    return case


@functools.lru_cache(maxsize=None)
def long_rows():
    """n = 4200; rows of exactly 2048 (not long), 2049, 3100 and 4101 entries among 300 short ones"""
    rng = np.random.default_rng(12)
    n = 4200
    rows = [_pick(rng, 0, n, 1 + i % 7) for i in range(300)]
    for at, k in ((17, K_LONG), (101, K_LONG + 1), (102, 3100), (299, 4101)):
        rows[at] = _pick(rng, 0, n, k)
    return _finish(rng, rows, n, "Min", eta=5e-4)


@functools.lru_cache(maxsize=None)
def long_cols(with_long_rows=False):
    """2100 rows of 3 entries that all contain column 0; column 1 has exactly 2048 entries (not long); optionally two long rows"""
    rng = np.random.default_rng(13)
    n = 4200 if with_long_rows else 300
    rows = []
    for i in range(2100):
        extra = _pick(rng, 2, n, 1 if i < K_LONG else 2)
        rows.append(np.concatenate([[0, 1] if i < K_LONG else [0], extra]).astype(np.int64))
    if with_long_rows:
        rows[5] = _pick(rng, 2, n, K_LONG + 1)             # (without columns 0 and 1: column 0 stays the only long one)
        rows[2099] = _pick(rng, 2, n, 4101)
    case = _finish(rng, rows, n, "Max", eta=5e-4)
    lp = case["lp"]
    assert lp.clen[0] == (2098 if with_long_rows else 2100) and lp.clen[1] == (K_LONG - 1 if with_long_rows else K_LONG)
    return case


@functools.lru_cache(maxsize=None)
def tiled(long_row=False):
    """8200 x 8200, 3 entries per row and a few rows of 64: 3 output tiles of 4096 and 2 input blocks of 8192 (the second 8
    wide) on both copies; rows and columns >= 8192 do not meet, so the cell (tile 2, block 1) is empty on both copies"""
    rng = np.random.default_rng(14)
    n = m = 8200
    rows = []
    for i in range(m):
        hi_col = 8192 if i >= 8192 else n
        rows.append(_pick(rng, 0, hi_col, 64 if i % 1000 == 7 else 3))
    if long_row:
        rows[4100] = _pick(rng, 0, n, 3000)
    return _finish(rng, rows, n, "Min", eta=2e-3)


@functools.lru_cache(maxsize=None)
def degenerate_scaling():
    """an empty row, an empty column and a row whose only entry is 1e-300, inside a small ragged matrix"""
    rng = np.random.default_rng(15)
    m, n = 40, 30
    rows = [_pick(rng, 1, n, 1 + i % 6) for i in range(m)]      # column 0: empty
    rows[3] = np.zeros(0, dtype=np.int64)                        # empty row
    rows[9] = np.array([4], dtype=np.int64)
    case = _finish(rng, rows, n, "Min")
    lp = case["lp"]
    lp.val[lp.rowptr[9]] = 1e-300
    assert lp.clen[0] == 0 and lp.rlen[3] == 0
    return case


def load(ktn, case, **solver_kw):
    """a handle that holds exactly the case's LP: a row-less model with the linear objective, then lp_append_rows"""
    lp = case["lp"]
    d = ktn.NLPDescription(lp.n, [0], [], [], [], [], [], [], [], obj_linear=True, obj_col=np.arange(lp.n), obj_atom_kind=np.zeros(lp.n),
                           obj_p0=lp.c, obj_p1=np.zeros(lp.n), obj_const=0.0)
    m = ktn.NonlinearModel(ktn.KatanaSolver(**dict(dict(log_level=0), **solver_kw)))
    m.loadproblem(lp.n, 0, lp.l, lp.u, [], [], lp.sense, d)
    m.lp_append_rows(lp.rowptr, lp.col.astype(np.int32), lp.val, lp.lo_raw, lp.hi_raw)
    rowptr, col, val, lo, hi = m.lp_rows()
    assert np.array_equal(rowptr, lp.rowptr) and np.array_equal(col, lp.col) and np.array_equal(val, lp.val)
    assert np.array_equal(lo, lp.lo_raw, equal_nan=True) and np.array_equal(hi, lp.hi_raw, equal_nan=True)
    assert np.array_equal(m.lp_objective()[0], lp.c)
    return m
