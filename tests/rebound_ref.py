"""Exact reference of the screen that follows a change of variable bounds (csrc/rebound.hpp): the smallest
and the largest value of every LP row over the box, in fractions.Fraction on the float inputs, and the verdict with the
threshold formed in floats exactly as the kernel forms it.

Row k, entries e with coefficient v_e on column c, box [l, u]:
    amin_k = sum_e (v_e > 0 ? v_e l_c : v_e < 0 ? v_e u_c : 0)        amax_k = sum_e (v_e > 0 ? v_e u_c : v_e < 0 ? v_e l_c : 0)
A zero coefficient contributes 0 whatever the bound; an infinite term makes the value -inf (+inf for amax) and stays out of the
finite sum; a NaN coefficient makes both values infinite.  S_k = sum_e of the larger finite one of the entry's two absolute terms.
    tau_k(b) = tol0 + ((len_k + 2) 2^-52) (S_k + |b|)       (floats, one rounding per operation, in this order)
The row proves the box infeasible when amin_k - hi_k > tau_k(hi_k) or lo_k - amax_k > tau_k(lo_k); it is redundant when
amax_k <= hi_k and amin_k >= lo_k."""
import itertools
import math
from fractions import Fraction

INF = float("inf")
EPS = 2.0 ** -52


def _term(v, b):
    """v * b exactly; None for an infinite term (v != 0 and b infinite)"""
    if math.isinf(b):
        return None
    return Fraction(v) * Fraction(b)


def row_activity(vals, ls, us):
    """(amin, amax, S) of one row: amin / amax are Fractions or -inf / +inf, S a Fraction.  vals, ls, us: the row's coefficients and
    the bounds of their columns, entry by entry."""
    smin = smax = S = Fraction(0)
    inf_min = inf_max = False
    for v, l, u in zip(vals, ls, us):
        v, l, u = float(v), float(l), float(u)
        if v == 0.0:
            continue
        if v != v:                                       # a NaN coefficient: both sides undecidable, nothing can be proven
            inf_min = inf_max = True
            continue
        tmin, tmax = (_term(v, l), _term(v, u)) if v > 0.0 else (_term(v, u), _term(v, l))
        if tmin is None:
            inf_min = True
        else:
            smin += tmin
        if tmax is None:
            inf_max = True
        else:
            smax += tmax
        S += max(abs(tmin) if tmin is not None else Fraction(0), abs(tmax) if tmax is not None else Fraction(0))
    return (-INF if inf_min else smin), (INF if inf_max else smax), S


def as_float(a):
    return a if isinstance(a, float) else float(a)       # (float(Fraction) rounds to nearest)


def tau(length, S, bound, tol0):
    return tol0 + (float(length + 2) * EPS) * (as_float(S) + abs(bound))


def _exact(a):
    """a Fraction for a finite value, the float itself for an infinite one"""
    if isinstance(a, Fraction):
        return a
    return a if math.isinf(a) else Fraction(a)


def _excess(a, b):
    """a - b rounded once; a, b Fractions or floats"""
    a, b = _exact(a), _exact(b)
    if isinstance(a, float) or isinstance(b, float):
        return as_float(a) - as_float(b)                 # (an infinite operand: -inf, +inf or NaN, as the kernel's subtraction)
    return float(a - b)


def _le(a, b):
    a, b = _exact(a), _exact(b)
    if isinstance(a, float) or isinstance(b, float):
        return as_float(a) <= as_float(b)
    return a <= b


def row_verdict(vals, ls, us, lo, hi, tol0):
    """dict(amin, amax, S, proving, redundant, ex_hi, ex_lo, t_hi, t_lo) of one row: ex_* the two excesses (rounded once), t_* their
    thresholds -- what the case builders use to stay away from, or sit next to, the threshold."""
    amin, amax, S = row_activity(vals, ls, us)
    n = len(vals)
    lo, hi = float(lo), float(hi)
    if lo != lo:
        lo = -INF                                        # (a NaN row bound is a vacuous side)
    if hi != hi:
        hi = INF
    ex_hi, ex_lo = _excess(amin, hi), _excess(lo, amax)
    t_hi, t_lo = tau(n, S, hi, tol0), tau(n, S, lo, tol0)
    proving = bool(ex_hi > t_hi) or bool(ex_lo > t_lo)
    redundant = _le(amax, hi) and _le(lo, amin)
    return dict(amin=amin, amax=amax, S=S, proving=proving, redundant=redundant, ex_hi=ex_hi, ex_lo=ex_lo, t_hi=t_hi, t_lo=t_lo)


def screen(rowptr, col, val, lo, hi, l, u, tol0):
    """The screen over all rows of a CSR matrix: (rows, count, first, redundant, crossed) -- rows: the row_verdict dicts; count /
    first: proving rows and the smallest proving index (-1: none); redundant: the count; crossed: columns with l_j > u_j."""
    rows = []
    for k in range(len(rowptr) - 1):
        s = slice(int(rowptr[k]), int(rowptr[k + 1]))
        c = [int(j) for j in col[s]]
        rows.append(row_verdict(list(val[s]), [l[j] for j in c], [u[j] for j in c], lo[k], hi[k], tol0))
    prov = [k for k, r in enumerate(rows) if r["proving"]]
    crossed = sum(1 for a, b in zip(l, u) if float(a) > float(b))
    return rows, len(prov), (prov[0] if prov else -1), sum(1 for r in rows if r["redundant"]), crossed


def brute_force(vals, ls, us, big=2.0 ** 60):
    """(min, max) of sum_e v_e x_e over the vertices of the box, infinite bounds replaced by -+big: Fractions.  For rows of at most
    ten entries with l <= u."""
    assert len(vals) <= 10
    ends = []
    for l, u in zip(ls, us):
        l = -big if l == -INF else (big if l == INF else float(l))
        u = big if u == INF else (-big if u == -INF else float(u))
        ends.append((Fraction(l), Fraction(u)))
    best_lo = best_hi = None
    for pick in itertools.product((0, 1), repeat=len(vals)):
        s = sum((Fraction(float(v)) * ends[e][p] for e, (v, p) in enumerate(zip(vals, pick))), Fraction(0))
        best_lo = s if best_lo is None or s < best_lo else best_lo
        best_hi = s if best_hi is None or s > best_hi else best_hi
    return best_lo, best_hi


def clamp(x, l, u):
    """(x clamped into [l, u] with a crossed column at l_j, columns moved, columns crossed): what k_rebound does"""
    out, moved, crossed = [], 0, 0
    for xj, lj, uj in zip(x, l, u):
        if lj > uj:
            nx = lj
            crossed += 1
        else:
            nx = lj if xj < lj else (uj if xj > uj else xj)
        moved += 0 if nx == xj else 1
        out.append(nx)
    return out, moved, crossed
