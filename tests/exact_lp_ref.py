"""Exact-rational KKT certificate of an LP answer -- TEST INFRASTRUCTURE (CPU, stdlib `fractions`).

    min / max  c'x   s.t.  lo_i <= a_i'x <= hi_i,   l <= x <= u

Every double is an exact rational, so whether a returned pair (x, y) is primal feasible, sign feasible and closes the duality
gap can be computed with NO rounding and without trusting any solver.  `certify` holds no threshold: it returns the exact
figures (rounded to double only on the way out) and the callers apply the tolerances.

Conventions (the engine's): y_i > 0 is a multiplier of the row's LOWER side, y_i < 0 of its UPPER side; a NaN
row bound means that side is vacuous; repeated column entries of a row are summed; s = -1 for "Max", so that the problem
certified is always  min s c'x.
"""
import math
from dataclasses import dataclass
from fractions import Fraction

ZERO = Fraction(0)


@dataclass
class Certificate:
    row_viol: float        # max over rows of a_i'x - hi_i and lo_i - a_i'x (-inf when no row has a finite side)
    worst_row: int         # the row that attains it (-1: none)
    bound_viol: float      # max over columns of l_j - x_j and x_j - u_j (-inf when no bound is finite)
    worst_col: int
    bound_at: float        # the bound that `bound_viol` was measured against
    sign_ok: bool          # y_i > 0 only with lo_i finite, y_i < 0 only with hi_i finite
    bad_sign_row: int      # first row that breaks it (-1: none)
    pobj: float            # s c'x
    dual_bound: float      # sum_i y_i (lo_i | hi_i) + sum_j r_j (l_j | u_j) over the FINITE bounds, r = s c - A'y
    charge: float          # sum over the r_j that need an infinite bound of |r_j| max(1, |x_j|)
    gap: float             # pobj - dual_bound
    worst_rc_col: int      # column with the largest charged |r_j| (-1: none)


def _finite(v):
    return v == v and not math.isinf(v)


def certify(A_csr, lo, hi, l, u, c, sense, x, y):
    rowptr, col, val = A_csr
    m, n = len(rowptr) - 1, len(x)
    assert len(lo) == len(hi) == len(y) == m and len(l) == len(u) == len(c) == n
    s = -1 if sense == "Max" else 1
    xf = [Fraction(float(v)) for v in x]
    r = [s * Fraction(float(v)) for v in c]                      # becomes s c - A'y
    row_viol, worst_row = None, -1
    sign_ok, bad_sign_row = True, -1
    dual = ZERO
    for i in range(m):
        b, e = int(rowptr[i]), int(rowptr[i + 1])
        cols = [int(col[k]) for k in range(b, e)]
        vals = [Fraction(float(val[k])) for k in range(b, e)]
        ax = sum((a * xf[j] for a, j in zip(vals, cols)), ZERO)
        lo_i, hi_i = float(lo[i]), float(hi[i])
        for v in ((ax - Fraction(hi_i)) if _finite(hi_i) else None, (Fraction(lo_i) - ax) if _finite(lo_i) else None):
            if v is not None and (row_viol is None or v > row_viol):
                row_viol, worst_row = v, i
        yi = float(y[i])
        if yi != 0.0:
            yf = Fraction(yi)
            side = lo_i if yi > 0 else hi_i
            if _finite(side):
                dual += yf * Fraction(side)
            elif sign_ok:
                sign_ok, bad_sign_row = False, i
            for a, j in zip(vals, cols):
                r[j] -= yf * a
    bound_viol, worst_col, bound_at = None, -1, 0.0
    charge, worst_rc, worst_rc_col = ZERO, ZERO, -1
    for j in range(n):
        lj, uj = float(l[j]), float(u[j])
        for v, b in (((Fraction(lj) - xf[j]) if _finite(lj) else None, lj), ((xf[j] - Fraction(uj)) if _finite(uj) else None, uj)):
            if v is not None and (bound_viol is None or v > bound_viol):
                bound_viol, worst_col, bound_at = v, j, b
        if r[j] != 0:
            side = lj if r[j] > 0 else uj
            if _finite(side):
                dual += r[j] * Fraction(side)
            else:
                ch = abs(r[j]) * max(Fraction(1), abs(xf[j]))
                charge += ch
                if abs(r[j]) > worst_rc:
                    worst_rc, worst_rc_col = abs(r[j]), j
    pobj = sum((s * Fraction(float(cj)) * xj for cj, xj in zip(c, xf)), ZERO)
    ninf = float("-inf")
    return Certificate(row_viol=ninf if row_viol is None else float(row_viol), worst_row=worst_row,
                       bound_viol=ninf if bound_viol is None else float(bound_viol), worst_col=worst_col, bound_at=bound_at,
                       sign_ok=sign_ok, bad_sign_row=bad_sign_row, pobj=float(pobj), dual_bound=float(dual), charge=float(charge),
                       gap=float(pobj - dual), worst_rc_col=worst_rc_col)


# the tolerances of test_exact_small_lp_kernel_matches_highs, on data of that scale
ROW_TOL, BOUND_TOL, GAP_REL, CHARGE_REL = 1e-8, 1e-9, 1e-7, 1e-8


def failures(cert):
    """what of a Certificate misses the tolerances above: a list of strings that name the row / column (empty: accepted)"""
    bad = []
    scale = max(1.0, abs(cert.pobj))
    if cert.row_viol > ROW_TOL:
        bad.append("row %d violated by %.3e" % (cert.worst_row, cert.row_viol))
    if cert.bound_viol > BOUND_TOL * max(1.0, abs(cert.bound_at)):
        bad.append("column %d outside its bound %.17g by %.3e" % (cert.worst_col, cert.bound_at, cert.bound_viol))
    if not cert.sign_ok:
        bad.append("multiplier of row %d points at an absent side" % cert.bad_sign_row)
    if not abs(cert.gap) <= GAP_REL * scale:
        bad.append("gap %.3e (pobj %.17g, dual bound %.17g)" % (cert.gap, cert.pobj, cert.dual_bound))
    if not cert.charge <= CHARGE_REL * scale:
        bad.append("reduced costs on infinite bounds charge %.3e (largest at column %d)" % (cert.charge, cert.worst_rc_col))
    return bad
