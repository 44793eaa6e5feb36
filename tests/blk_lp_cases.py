"""Block-diagonal LPs with a planted primal-dual pair, for the per-instance LP of throughput mode (csrc/batch_lp.hpp behind
NonlinearModel.set_blocks + lp_solve): tests/test_blk_lp_cases.py on the CPU, tests/test_gpu_blk_lp.py on the GPU.

Every block is drawn on its own: rows cycle through <=, ranged, equality, free (both sides infinite), NaN-sided and >=, variables
through boxed, lower-only, upper-only, free and fixed (the cycles of tests/lp_cases.py); values spread over two decades.  The
planted point xhat is a vertex: every tight row that can be given one owns a PIVOT column (an entry of magnitude 3 .. 10) that is
strictly inside its bounds, every other column that has a finite bound sits on one with a non-zero reduced cost r of the matching
sign, every tight row carries a multiplier of the sign of its tight side (y > 0 lower side, y < 0 upper side), and the cost is
c = s (A'y + r).  Free columns are the first to be given a pivot row; one that finds none stays inside with r = 0.  (x, y) is then
a KKT pair of  min s c'x  up to the rounding of c.  Every fifth column is free.  With as many free
columns a step that is too long meets no bound that would stop it: the ordinary loop's 8-pass power iteration put sigma_max of
`edges` at 0.92 (a block-diagonal matrix has one near-largest singular value per block), its iterates reached |x| = 1e13 in 65
iterations and were not back after 400 000.  Engine::lp_solve_core now starts such a solve again, cold, with the safe step
(`lp_cold_restarts`), and the block kernel, which has no growing-residual rule, starts with the safe step next to columns without
a bound; `edges`, `two_trips` and `long_row` run into it.  Three blocks are capped at SLOW_MAX_FREE = 8 free columns (the
limit of exact_lp_cases.py; the columns of a free turn beyond the eighth are boxed), for time alone: with every fifth column free
the ordinary loop -- the reference of the GPU tier -- does not diverge on them, its step is the safe one and its residual decays,
but it was still 6e-9, 4e-7 and 3e-7 (relative) off the planted objective after 400 000, 100 000 and 100 000 iterations: the 257-
column block of `edges`, the 1 025-column block of `two_trips` and the 3 300-column block of `too_big`.

The sizes follow the constants of csrc/batch_lp.hpp as they stand: an x-step pass of k_pdhg_blocks covers TX * kBlkThreads / GX =
4 * 1024 / 4 = 1 024 columns, a y-step pass TY * kBlkThreads / GY = 5 * 1024 / 4 = 1 280 rows, blk_dots issues 2 G = 8 entries per
range before its tail loop, the check loops stride by 256 outputs, Engine::lp_solve_blocks refuses more than 150 KB of LDS
(3 (nmax + mmax) doubles + mmax ints + 1 K), Engine::kLongRow = 2 048, and lp_mid_max_var = 512.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

from exact_lp_cases import LpCase

INF = float("inf")
X_PASS, Y_PASS, K_LONG, LDS_LIMIT, MID_MAX_VAR = 1024, 1280, 2048, 150 * 1024, 512
RANGE_LENGTHS = (0, 1, 3, 4, 5, 7, 8, 9, 20, 200)
SLOW_MAX_FREE = 8


@dataclass
class BlkCase:
    name: str
    n: int
    rowptr: np.ndarray
    col: np.ndarray
    val: np.ndarray
    lo: np.ndarray               # (with the NaNs, as the handle gets them)
    hi: np.ndarray
    l: np.ndarray
    u: np.ndarray
    c: np.ndarray
    offsets: np.ndarray          # block column offsets, [nblocks + 1]
    row_block: np.ndarray        # block of every row: that of its first column; rows without entries belong to block 0 (k_row_block)
    x: np.ndarray                # planted pair; NaN in the blocks that have none (status_b != "Optimal")
    y: np.ndarray
    sense: str = "Min"
    status: str = "Optimal"
    block_status: tuple = ()
    info: dict = field(default_factory=dict)

    @property
    def m(self):
        return len(self.lo)

    @property
    def nblocks(self):
        return len(self.offsets) - 1


def block_lp(case, b, rows=None):
    """block b as an LP of its own (an exact_lp_cases.LpCase with local column ids) and the global ids of its rows; `rows` =
    (rowptr, col, val, lo, hi) replaces the case's rows (lp_rows() of a handle that has grown)"""
    rowptr, col, val, lo, hi = (case.rowptr, case.col, case.val, case.lo, case.hi) if rows is None else rows
    c0, c1 = int(case.offsets[b]), int(case.offsets[b + 1])
    rb = row_blocks(rowptr, col, case.offsets)
    idx = np.flatnonzero(rb == b)
    lens = np.diff(rowptr)[idx]
    ent = np.concatenate([np.arange(rowptr[i], rowptr[i + 1]) for i in idx]).astype(np.int64) if len(idx) else np.zeros(0, dtype=np.int64)
    lcol = col[ent].astype(np.int64) - c0
    assert len(lcol) == 0 or (lcol.min() >= 0 and lcol.max() < c1 - c0), "row with entries in two blocks"
    sub = LpCase("%s[%d]" % (case.name, b), c1 - c0, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), lcol.astype(np.int32),
                 val[ent].copy(), lo[idx].copy(), hi[idx].copy(), case.l[c0:c1].copy(), case.u[c0:c1].copy(), case.c[c0:c1].copy(),
                 sense=case.sense)
    return sub, idx


def row_blocks(rowptr, col, offsets):
    """block of every row as k_row_block finds it: the last b with offsets[b] <= first column; rows without entries: 0"""
    m = len(rowptr) - 1
    rb = np.zeros(m, dtype=np.int64)
    has = np.diff(rowptr) > 0
    first = col[rowptr[:-1][has]].astype(np.int64)
    rb[has] = np.searchsorted(np.asarray(offsets[1:], dtype=np.int64), first, side="right")
    return rb


# ---- one block ---------------------------------------------------------------------------------------------------------------------

def _values(rng, k):
    return rng.choice([-1.0, 1.0], k) * 10.0 ** rng.uniform(-1.0, 1.0, k)


def _pick(rng, lo, hi, k):
    return np.sort(rng.choice(np.arange(lo, hi), size=k, replace=False))


def _structure(rng, n, row_lens, low_col_lens, low_rows):
    """rows as sorted local column arrays.  Without low columns every row draws its length from all n columns.  With them (the
    recipe of lp_cases.ragged): the rows of `row_lens` draw from the columns behind the low ones, and `low_rows` further rows
    hold the low columns -- column j in low_col_lens[j] of them -- plus i % 4 entries of their own"""
    n_low = len(low_col_lens)
    rows = [_pick(rng, n_low, n, k) for k in row_lens]
    if n_low:
        low = [[] for _ in range(low_rows)]
        for j, k in enumerate(low_col_lens):
            for i in _pick(rng, 0, low_rows, k):
                low[i].append(j)
        rows += [np.array(sorted(low[i]) + list(_pick(rng, n_low, n, i % 4)), dtype=np.int64) for i in range(low_rows)]
    return rows


def make_block(n, row_lens, seed, tight_share=0.3, low_col_lens=(), low_rows=0, boxed=False, max_free=None):
    """dict(rows, val, lo, hi, l, u, cs = s c, x, y) of one block with local column ids"""
    rng = np.random.default_rng(seed)
    rows = _structure(rng, n, list(row_lens), list(low_col_lens), low_rows)
    m = len(rows)
    vals = [_values(rng, len(r)) for r in rows]
    # variables: boxed, lower-only, upper-only, free, fixed
    vk = np.arange(n) % 5
    if max_free is not None:
        vk[np.flatnonzero(vk == 3)[max_free:]] = 0                # (the others of the free turn are boxed)
    if boxed:
        vk[:] = 0
    l, u = rng.uniform(-3.0, -0.5, n), rng.uniform(0.5, 3.0, n)
    u[vk == 1] = INF; l[vk == 2] = -INF
    l[vk == 3] = -INF; u[vk == 3] = INF
    u[vk == 4] = l[vk == 4]
    rk = np.arange(m) % 6                                        # <=, ranged, equality, free, NaN-sided, >=
    can_be_tight = np.array([rk[i] != 3 and len(rows[i]) > 0 for i in range(m)], dtype=bool)
    # pivots: free columns first (each looks for a row that holds it), then the equality rows, then further rows up to the share
    pivot_of_row = np.full(m, -1)
    is_pivot = np.zeros(n, dtype=bool)
    holders = [[] for _ in range(n)]
    for i in rng.permutation(m):
        if can_be_tight[i]:
            for p, j in enumerate(rows[i]):
                holders[j].append((i, p))
    for j in np.flatnonzero(vk == 3):
        for i, p in holders[j]:
            if pivot_of_row[i] < 0:
                pivot_of_row[i] = p; is_pivot[j] = True
                break
    want = int(round(tight_share * m))
    order = [i for i in rng.permutation(m) if can_be_tight[i] and rk[i] == 2] + [i for i in rng.permutation(m) if can_be_tight[i] and rk[i] != 2]
    tight = pivot_of_row >= 0
    for i in order:
        if pivot_of_row[i] >= 0:
            continue
        if rk[i] != 2 and np.count_nonzero(tight) >= want:
            continue
        free_pos = [p for p, j in enumerate(rows[i]) if not is_pivot[j] and vk[j] in (0, 1, 2)]
        if free_pos:
            p = free_pos[rng.integers(len(free_pos))]
            pivot_of_row[i] = p; is_pivot[rows[i][p]] = True
            tight[i] = True
        elif rk[i] == 2:
            tight[i] = True                                      # an equality row is tight with or without a pivot
    for i in np.flatnonzero(pivot_of_row >= 0):
        p = pivot_of_row[i]
        vals[i][p] = np.sign(vals[i][p]) * 10.0 ** rng.uniform(0.5, 1.0)
    # the point: pivots and free columns inside, everything else on a bound
    inside = is_pivot | (vk == 3)
    at_lower = ~inside & ((vk == 1) | (vk == 4) | ((vk == 0) & (rng.random(n) < 0.5)))
    at_upper = ~inside & ~at_lower
    span_lo = np.where(np.isfinite(l), l, -3.0)
    span_hi = np.where(np.isfinite(u), u, 3.0)
    x = span_lo + rng.uniform(0.2, 0.8, n) * (span_hi - span_lo)
    x[at_lower] = l[at_lower]
    x[at_upper] = u[at_upper]
    r = np.zeros(n)
    r[at_lower] = rng.uniform(0.5, 1.5, np.count_nonzero(at_lower))
    r[at_upper] = -rng.uniform(0.5, 1.5, np.count_nonzero(at_upper))
    fixed = vk == 4
    r[fixed] *= rng.choice([-1.0, 1.0], np.count_nonzero(fixed))
    # rows: sides around a'x, multipliers on the tight ones
    lo, hi, y = np.zeros(m), np.zeros(m), np.zeros(m)
    aty = np.zeros(n)
    for i in range(m):
        ax = float(vals[i] @ x[rows[i]]) if len(rows[i]) else 0.0
        below, above = ax - rng.uniform(0.5, 2.0), ax + rng.uniform(0.5, 2.0)
        mult = rng.uniform(0.5, 1.5)
        k = rk[i]
        if k == 0:
            lo[i], hi[i] = -INF, (ax if tight[i] else above)
            y[i] = -mult if tight[i] else 0.0
        elif k == 1:
            upper_side = bool(rng.random() < 0.5)
            lo[i], hi[i] = below, above
            if tight[i]:
                if upper_side:
                    hi[i], y[i] = ax, -mult
                else:
                    lo[i], y[i] = ax, mult
        elif k == 2:
            lo[i] = hi[i] = ax
            y[i] = (mult if rng.random() < 0.5 else -mult) if tight[i] else 0.0
        elif k == 3:
            lo[i], hi[i] = -INF, INF
        elif k == 4:
            lo[i], hi[i] = np.nan, (ax if tight[i] else above)
            y[i] = -mult if tight[i] else 0.0
        else:
            lo[i], hi[i] = (ax if tight[i] else below), INF
            y[i] = mult if tight[i] else 0.0
        if y[i] != 0.0:
            np.add.at(aty, rows[i], y[i] * vals[i])
    return dict(n=n, rows=rows, vals=vals, lo=lo, hi=hi, l=l, u=u, cs=aty + r, x=x, y=y, feasible=True)


def _infeasible_block(n, row_lens, seed, empty_row):
    """a feasible block plus two contradictory rows  g'x <= t,  2 g'x >= 2 t + 2  -- or, for the twin, an empty row whose sides
    exclude 0 (exact_lp_cases._mid_infeasible_empty_row)"""
    blk = make_block(n, row_lens, seed, boxed=True)
    rng = np.random.default_rng(seed + 1000)
    if empty_row:
        extra = [(np.zeros(0, dtype=np.int64), np.zeros(0), -INF, -1.0)]
    else:
        cols = _pick(rng, 0, n, min(n, 4))
        g = rng.uniform(0.5, 1.5, len(cols)) * rng.choice([-1.0, 1.0], len(cols))
        t = float(g @ blk["x"][cols])
        extra = [(cols, g, -INF, t), (cols, 2.0 * g, 2.0 * t + 2.0, INF)]
    for cols, g, lo, hi in extra:
        blk["rows"].append(cols); blk["vals"].append(g)
        blk["lo"] = np.append(blk["lo"], lo); blk["hi"] = np.append(blk["hi"], hi); blk["y"] = np.append(blk["y"], np.nan)
    blk["feasible"] = False
    return blk


# ---- the block-diagonal LP ---------------------------------------------------------------------------------------------------------

def assemble(name, blocks, sense="Min", mixed=True, seed=0, status="Optimal"):
    """blocks: list of make_block results (or None for an empty block).  mixed: the rows of all blocks in a seeded permutation;
    otherwise block after block"""
    sizes = [0 if b is None else b["n"] for b in blocks]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offsets[-1])
    owner, rows, vals, lo, hi, y = [], [], [], [], [], []
    l, u, cs, x = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for b, blk in enumerate(blocks):
        if blk is None:
            continue
        c0, c1 = offsets[b], offsets[b + 1]
        l[c0:c1], u[c0:c1], cs[c0:c1] = blk["l"], blk["u"], blk["cs"]
        x[c0:c1] = blk["x"] if blk["feasible"] else np.nan
        for i in range(len(blk["rows"])):
            owner.append(b); rows.append(blk["rows"][i] + c0); vals.append(blk["vals"][i])
            lo.append(blk["lo"][i]); hi.append(blk["hi"][i]); y.append(blk["y"][i] if blk["feasible"] else np.nan)
    m = len(rows)
    perm = np.random.default_rng(seed + 77).permutation(m) if mixed else np.arange(m)
    rows, vals = [rows[i] for i in perm], [vals[i] for i in perm]
    lo, hi, y = np.array(lo)[perm], np.array(hi)[perm], np.array(y)[perm]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = (np.concatenate(rows) if m else np.zeros(0)).astype(np.int32)
    val = (np.concatenate(vals) if m else np.zeros(0)).astype(np.float64)
    s = -1.0 if sense == "Max" else 1.0
    rb = row_blocks(rowptr, col, offsets)
    # (a row without entries is certified with block 0, wherever it was drawn: it owes nothing to any column and its y is 0)
    bstat = tuple("Optimal" if (blk is None or blk["feasible"]) else "Infeasible" for blk in blocks)
    return BlkCase(name, n, rowptr, col, val, lo, hi, l, u, s * cs, offsets, rb, x, y, sense=sense, status=status, block_status=bstat,
                   info=dict(mixed=mixed, owner=np.array(owner, dtype=np.int64)[perm] if m else np.zeros(0, dtype=np.int64)))


def _lens(rng, m, lo=2, hi=8):
    return rng.integers(lo, hi + 1, m).tolist()


def _std_block(n, m, seed, **kw):
    """a block of n columns and m rows of 2 .. 8 entries (no more than n)"""
    rng = np.random.default_rng(seed + 5000)
    return make_block(n, [min(k, n) for k in _lens(rng, m)], seed, **kw)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

def _edges_blocks():
    """column counts 1, 3, 255, 257, 1 023 and 1 024 (the strides of the check loops and the x-step pass, from below and exactly),
    with 2, 4, 200, 300, 700 and 800 rows: fewer outputs than lane groups in the first four"""
    return [_std_block(n, m, 100 + n, max_free=SLOW_MAX_FREE if n == 257 else None)
            for n, m in ((1, 2), (3, 4), (255, 200), (257, 300), (1023, 700), (1024, 800))]


def _two_trips_blocks():
    """columns and rows cross their pass sizes independently: 1 025 x 1 279, (2 049 + 5) x 1 280, 300 x 1 281, 700 x 2 561, and a
    block below both"""
    shapes = ((X_PASS + 1, Y_PASS - 1), (2 * X_PASS + 1 + 5, Y_PASS), (300, Y_PASS + 1), (700, 2 * Y_PASS + 1), (400, 300))
    seeds = (200, 201, 202, 203, 204)
    return [_std_block(n, m, seed, tight_share=0.2, max_free=SLOW_MAX_FREE if n == X_PASS + 1 else None) for seed, (n, m) in zip(seeds, shapes)]


def _ranges_blocks():
    """two blocks of 389 columns: rows of every length of RANGE_LENGTHS (30 times each) from the columns [40, 389), columns [0, 40)
    of every length of RANGE_LENGTHS from 260 further rows"""
    out = []
    for i in range(2):
        row_lens = [RANGE_LENGTHS[k % len(RANGE_LENGTHS)] for k in range(300)]
        col_lens = [RANGE_LENGTHS[j % len(RANGE_LENGTHS)] for j in range(40)]
        out.append(make_block(389, row_lens, 300 + i, low_col_lens=col_lens, low_rows=260))
    return out


def _empties_blocks(empty_rows=True):
    """an empty first block, two empty blocks in a row in the middle, an empty last block, a block with columns and no rows, and a
    block with two empty rows whose sides contain 0.  Rows without entries belong to block 0, so with them the empty first block
    owns rows; without them (`empties_rowless_first`) the first sorted key is above 0 and k_block_rows fills blk_rowptr[0 .. 1]
    from the row at position 0"""
    rng = np.random.default_rng(400)
    with_empty_rows = make_block(120, _lens(rng, 60) + ([0, 0] if empty_rows else []), 401)
    return [None, _std_block(300, 240, 402), None, None, with_empty_rows, make_block(37, [], 403), _std_block(200, 150, 404), None]


def _shifted_blocks():
    """a column without rows, fixed at 0 and of cost 0, in front of a block of X_PASS columns: under the offsets [0, 1, 1 025] the
    last column is local column 1 023 of the x-step's first trip, under [0, 1 025] local column 1 024 of its second.  (Eight free columns: two launches are
    compared with each other here, over as few iterations as the shape allows)"""
    one = dict(n=1, rows=[], vals=[], lo=np.zeros(0), hi=np.zeros(0), l=np.zeros(1), u=np.zeros(1), cs=np.zeros(1), x=np.zeros(1),
               y=np.zeros(0), feasible=True)
    return [one, _std_block(X_PASS, 800, 900, max_free=SLOW_MAX_FREE)]


def _too_big_blocks():
    """one block of 3 300 columns and 3 300 rows -- 3 (n + m) doubles are 158 400 B > 150 KB -- between two small ones"""
    return [_std_block(60, 40, 500), _std_block(3300, 3300, 501, tight_share=0.2, max_free=SLOW_MAX_FREE), _std_block(90, 70, 502)]


def _long_row_blocks():
    """a block of 2 200 columns with one row of 2 060 > kLongRow entries, next to a small block"""
    rng = np.random.default_rng(600)
    lens = _lens(rng, 900)
    lens[417] = K_LONG + 12
    return [_std_block(80, 60, 601), make_block(2200, lens, 602, tight_share=0.2)]


def _infeasible_blocks(empty_row):
    """every variable of these two cases is boxed.  The ordinary loop accepts a Farkas certificate only when A'y vanishes on the
    columns with an infinite bound, to 1e-9 (1 + |y|), over the WHOLE LP: a feasible block with one-sided columns keeps A'y near its
    costs there, and the bad block's multipliers then have to grow to 1e9 of that first (measured with the variable kinds of the
    other cases: Infeasible after 8 157 404 and 6 366 203 iterations)"""
    rng = np.random.default_rng(700)
    bad = _infeasible_block(8, [min(k, 8) for k in _lens(rng, 6)], 702, empty_row)
    a, b = _std_block(300, 220, 701, boxed=True), _std_block(290, 200, 703, boxed=True)
    if empty_row:                                                # (rows without entries belong to block 0: the bad block comes first)
        return [bad, a, b]
    return [a, bad, b]


@functools.lru_cache(maxsize=None)
def case(name, mixed=True):
    if name == "edges":
        return assemble(name, _edges_blocks(), mixed=mixed, seed=1)
    if name == "max_sense":
        return assemble(name, _edges_blocks(), sense="Max", mixed=mixed, seed=1)
    if name == "two_trips":
        return assemble(name, _two_trips_blocks(), mixed=mixed, seed=2)
    if name == "ranges":
        return assemble(name, _ranges_blocks(), mixed=mixed, seed=3)
    if name == "empties":
        return assemble(name, _empties_blocks(), mixed=mixed, seed=4)
    if name == "empties_rowless_first":
        return assemble(name, _empties_blocks(False), mixed=mixed, seed=4)
    if name == "shifted":
        return assemble(name, _shifted_blocks(), mixed=mixed, seed=9)
    if name == "one_block":
        return assemble(name, [_std_block(700, 500, 800)], mixed=mixed, seed=8)
    if name == "too_big":
        return assemble(name, _too_big_blocks(), mixed=mixed, seed=5)
    if name == "long_row":
        return assemble(name, _long_row_blocks(), mixed=mixed, seed=6)
    if name == "infeasible_block":
        return assemble(name, _infeasible_blocks(False), mixed=mixed, seed=7, status="Infeasible")
    if name == "infeasible_empty_row":
        return assemble(name, _infeasible_blocks(True), mixed=mixed, seed=7, status="Infeasible")
    raise KeyError(name)


FEASIBLE = ("edges", "two_trips", "ranges", "empties", "empties_rowless_first", "max_sense", "one_block", "shifted", "too_big", "long_row")
INFEASIBLE = ("infeasible_block", "infeasible_empty_row")
ORDERS = (True, False)                                           # mixed, block after block


def cut_rows(case_, x, blocks, depth=0.1, seed=5, per_block=2):
    """(rowptr, col, val, lo, hi) of rows  a'x <= a'x* - depth  with a on the block's own columns (global ids), `per_block` for each
    block of `blocks`: they cut the point x off.  (A cut whose columns all sit on bounds that hold them can leave nothing feasible:
    the default seed is one with which blocks 3 and 5 of `edges` stay feasible and lose 0.3 of objective each, which the CPU tier
    asserts with HiGHS)"""
    rng = np.random.default_rng(seed)
    rowptr, col, val, lo, hi = [0], [], [], [], []
    for _ in range(per_block):
        for b in blocks:                                          # (block by block in turn: the appended rows interleave too)
            c0, c1 = int(case_.offsets[b]), int(case_.offsets[b + 1])
            cols = _pick(rng, c0, c1, min(6, c1 - c0))
            a = rng.uniform(0.5, 1.5, len(cols)) * rng.choice([-1.0, 1.0], len(cols))
            col.extend(cols.tolist()); val.extend(a.tolist()); rowptr.append(len(col))
            lo.append(-INF); hi.append(float(a @ x[cols]) - depth)
    return (np.array(rowptr, dtype=np.int64), np.array(col, dtype=np.int32), np.array(val), np.array(lo), np.array(hi))


def load(ktn, case_, blocks, **solver_kw):
    """a handle that holds exactly the case's LP (lp_cases.load: a row-less model with the linear objective, then lp_append_rows),
    with set_blocks when `blocks` is set"""
    n = case_.n
    d = ktn.NLPDescription(n, [0], [], [], [], [], [], [], [], obj_linear=True, obj_col=np.arange(n), obj_atom_kind=np.zeros(n),
                           obj_p0=case_.c, obj_p1=np.zeros(n), obj_const=0.0)
    m = ktn.NonlinearModel(ktn.KatanaSolver(**dict(dict(log_level=0), **solver_kw)))
    m.loadproblem(n, 0, case_.l, case_.u, [], [], case_.sense, d)
    m.lp_append_rows(case_.rowptr, case_.col, case_.val, case_.lo, case_.hi)
    rowptr, col, val, lo, hi = m.lp_rows()
    assert np.array_equal(rowptr, case_.rowptr) and np.array_equal(col, case_.col) and np.array_equal(val, case_.val)
    assert np.array_equal(lo, case_.lo, equal_nan=True) and np.array_equal(hi, case_.hi, equal_nan=True)
    assert np.array_equal(m.lp_objective()[0], case_.c)
    if blocks:
        m.set_blocks(case_.offsets)
    return m
