"""ktn_set_row_bounds as plain Python over the list model of the pool (tests/pool_ref.py): what csrc/rebound.hip validates and what
k_rebase_cuts / k_blocks_rebase (csrc/rebound.hpp, csrc/batch_warm.hpp) write.  No GPU, no numpy.

A cut of nonlinear row i taken at a point with tangent constant b is stored as lo = lb_i - b, hi = ub_i - b.  New bounds move it:
    hi <- hi + (ub' - ub)        lo <- lo + (lb' - lb)
the difference formed once per row, each operation one IEEE double operation (Python floats are those).  A side whose old and new
bound are equal is left untouched, two equal infinities included, so a zero delta is the identity and inf - inf is never formed."""
import math

E_OK, E_INVALID = 0, -1


def same_side(old, new):
    """a nonlinear row keeps its pattern of finite sides; an infinite side stays the infinity it is"""
    return math.isfinite(new) if math.isfinite(old) else new == old


def validate(lb, ub, nlb, nub, is_nl):
    """(code, crossed rows, a linear row changed): NaN and a nonlinear row gaining or losing a side are refused; linear rows may do
    either; lb' > ub' is counted, not refused"""
    assert len(lb) == len(ub) == len(nlb) == len(nub) == len(is_nl)
    for a, b in zip(nlb, nub):
        if a != a or b != b:
            return E_INVALID, 0, False
    crossed, lin_changed = 0, False
    for l0, u0, l1, u1, nl in zip(lb, ub, nlb, nub, is_nl):
        if nl:
            if not (same_side(l0, l1) and same_side(u0, u1)):
                return E_INVALID, 0, False
        elif not (l0 == l1 and u0 == u1):
            lin_changed = True
        if l1 > u1:
            crossed += 1
    return E_OK, crossed, lin_changed


def shift(value, old, new):
    """one side of one cut"""
    if old == new:
        return value
    return value + (new - old)


def rebase(pool, list_row, lb, ub, nlb, nub):
    """pool: a PoolRef whose list s holds the cuts of constraint list_row[s]; moves every list row in place, returns the number of
    rows of lists with a changed bound (the engine's "rebase_rows")"""
    moved = 0
    for s, i in enumerate(list_row):
        if lb[i] == nlb[i] and ub[i] == nub[i]:
            continue
        for r in pool.list_rows(s):
            pool.lo[r] = shift(pool.lo[r], lb[i], nlb[i])
            pool.hi[r] = shift(pool.hi[r], ub[i], nub[i])
            moved += 1
    return moved


def owners(pool, list_row):
    """per pool row the constraint whose list holds it, -1 for a row in no list"""
    out = [-1] * pool.M
    for s, i in enumerate(list_row):
        for r in pool.list_rows(s):
            out[r] = i
    return out
