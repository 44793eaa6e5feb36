"""Reference of the supporting-hyperplane root search (csrc/esh.hpp) in float64 and mpmath.

A row is either separable (atoms over columns, as in katana.jl_amd/instances.py) or an s-expression (oracle/sexpr.py).
On the segment x(lam) = x_int + lam (x* - x_int) the search solves phi(lam) = sigma (g(x(lam)) - bound) = 0 with the
engine's bracketed Newton from lam = 1; `exact_root` is the mpmath root, `quad_root` the closed form for quadratic and
linear atoms (phi is then a quadratic in lam)."""
import math

import mpmath as mp
import numpy as np

LIN, QUAD, EXP, NEGLOG = 0, 1, 2, 3


def atom(kind, p0, p1, x, lib=math):
    """value and derivative of one separable atom (csrc/kernels.hpp atom_eval)"""
    if kind == LIN:
        return p0 * x, p0
    if kind == QUAD:
        d = x - p1
        return p0 * d * d, 2 * p0 * d
    if kind == EXP:
        e = p0 * lib.exp(p1 * x)
        return e, p1 * e
    s = x + p1
    return -p0 * lib.log(s), -p0 / s


class SepRow:
    """g(x) = sum_e atom_e(x[col_e]) + rconst"""

    def __init__(self, cols, kinds, p0, p1, rconst=0.0):
        self.cols = np.asarray(cols, dtype=np.int64)
        self.kinds, self.p0, self.p1 = list(kinds), list(p0), list(p1)
        self.rconst = rconst

    def eval(self, x, lib=math):
        g, grad = (mp.mpf(self.rconst) if lib is mp else self.rconst), []
        for c, k, a, b in zip(self.cols, self.kinds, self.p0, self.p1):
            v, d = atom(k, a, b, x[int(c)], lib)
            g = g + v
            grad.append(d)
        return g, grad


class SexprRow:
    """g(x) from an s-expression (oracle/sexpr.py); float64 only (mpmath through tape_ref for tape rows)"""

    def __init__(self, expr, cols):
        from oracle import sexpr
        self.expr, self.cols, self._s = expr, np.asarray(cols, dtype=np.int64), sexpr

    def eval(self, x, lib=math):
        with np.errstate(all="ignore"):
            g, gr = self._s.eval_grad(self.expr, np.asarray(x, dtype=np.float64))
        if isinstance(gr, dict):
            return float(g), [float(gr.get(int(c), 0.0)) for c in self.cols]
        gr = np.asarray(gr, dtype=np.float64)
        return float(g), [float(gr[int(c)]) for c in self.cols]


def point(xi, xs, lam, lib=math):
    if lib is mp:
        return [mp.mpf(a) + mp.mpf(lam) * (mp.mpf(b) - mp.mpf(a)) for a, b in zip(xi, xs)]
    if lam == 1.0:
        return np.asarray(xs, dtype=np.float64).copy()
    xi, xs = np.asarray(xi, dtype=np.float64), np.asarray(xs, dtype=np.float64)
    return xi + lam * (xs - xi)


def phi(row, xi, xs, side, bound, lam, lib=math):
    """phi(lam), phi'(lam) and the gradient entries of the row at x(lam)"""
    x = point(xi, xs, lam, lib)
    g, grad = row.eval(x, lib)
    if lib is mp:
        d = sum(gd * (mp.mpf(xs[int(c)]) - mp.mpf(xi[int(c)])) for gd, c in zip(grad, row.cols))
    else:
        d = sum(gd * (xs[int(c)] - xi[int(c)]) for gd, c in zip(grad, row.cols))
    return side * (g - bound), side * d, grad, g


def root_search(row, xi, xs, side, bound, tol, iters=20):
    """the engine's search in float64: returns (lam_b or None, passes); lam_b is the last point with a finite phi >= 0 below 1"""
    lo, hi, lam, best = 0.0, 1.0, 1.0, None
    passes = 0
    for _ in range(iters):
        f, df, grad, _g = phi(row, xi, xs, side, bound, lam)
        passes += 1
        fin = math.isfinite(f) and all(math.isfinite(v) for v in grad)
        if not (f < 0.0):
            hi = lam
            if fin and lam < 1.0:
                best = lam
            if fin and f <= tol:
                break
        else:
            lo = lam
        nl = lam - f / df if df != 0.0 else math.nan
        if not (fin and df > 0.0 and math.isfinite(nl) and lo < nl < hi):
            nl = 0.5 * (lo + hi)
        lam = nl
    return best, passes


def exact_root(row, xi, xs, side, bound, dps=50):
    """the root of phi in (0, 1] at `dps` digits (bisection; phi(0) < 0 < phi(1))"""
    with mp.workdps(dps):
        lo, hi = mp.mpf(0), mp.mpf(1)
        for _ in range(dps * 4):
            mid = (lo + hi) / 2
            f = phi(row, xi, xs, side, bound, mid, mp)[0]
            if f < 0:
                lo = mid
            else:
                hi = mid
        return hi


def quad_root(row, xi, xs, side, bound):
    """closed-form root for rows of LIN and QUAD atoms: phi(lam) = A lam^2 + B lam + C (mpmath, 50 digits)"""
    with mp.workdps(50):
        A = B = mp.mpf(0)
        C = mp.mpf(row.rconst) - mp.mpf(bound)
        for c, k, a, b in zip(row.cols, row.kinds, row.p0, row.p1):
            x0, d = mp.mpf(xi[int(c)]) - mp.mpf(b) * (k == QUAD), mp.mpf(xs[int(c)]) - mp.mpf(xi[int(c)])
            a = mp.mpf(a)
            if k == LIN:
                B += a * d
                C += a * mp.mpf(xi[int(c)])
            elif k == QUAD:
                A += a * d * d
                B += 2 * a * x0 * d
                C += a * x0 * x0
            else:
                raise ValueError("quad_root: LIN and QUAD atoms only")
        A, B, C = side * A, side * B, side * C
        if A == 0:
            return -C / B
        disc = mp.sqrt(B * B - 4 * A * C)
        roots = [(-B + disc) / (2 * A), (-B - disc) / (2 * A)]
        return min(r for r in roots if 0 < r <= 1 + mp.mpf(10) ** -30)


def cut_at(row, xi, xs, side, bound, lam):
    """the gradient cut at x(lam) as (coefficients, constant): g(x_b) + grad'(x - x_b)  ->  grad'x + (g - grad'x_b)"""
    x = point(xi, xs, lam)
    g, grad = row.eval(x)
    const = g - sum(gd * x[int(c)] for gd, c in zip(grad, row.cols))
    return np.asarray(grad, dtype=np.float64), const


def lambda_from_coefficient(kind, p0, p1, coef, xi_c, xs_c):
    """invert one atom's derivative: the lam at which the atom on this column has derivative `coef`"""
    if kind == QUAD:
        x = coef / (2.0 * p0) + p1
    elif kind == EXP:
        x = math.log(coef / (p0 * p1)) / p1
    elif kind == NEGLOG:
        x = -p0 / coef - p1
    else:
        raise ValueError("a linear atom's derivative does not depend on x")
    return (x - xi_c) / (xs_c - xi_c)
