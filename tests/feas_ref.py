"""Reference of the feasible-point search (csrc/feas.hpp) in float64 and mpmath.

Definitions (restated from include/katana_hip.h):

    x*            what getsolution() returns; x_in the reference point (the caller's interior point, or the engine's own)
    taking part   a caller row that is not declared linear, of kind SEP, TAPE or QUAD, with exactly one finite side
                  (sigma = +1: g <= ub, -1: g >= lb; b that bound); never the epigraph row, never a free row
    phi_i(lam)    sigma_i (g_i(x_in + lam (x* - x_in)) - b_i), the point formed as the device forms it (`device_point`)
    lambda_i      1 where phi_i(1) <= 0 and is finite; otherwise a point of [0, 1) with -tau <= phi_i(lambda_i) <= 0,
                  tau = esh_root_tol * f_tol, by bracketed Newton on phi + tau / 2 from lam = 1 (`search`); a row that runs out of
                  passes takes the bracket's lower end, the last point with a finite phi <= 0 (0 to begin with)
    lambda*       min_i lambda_i; the blocking row is the smallest row index attaining a minimum below 1
    x_feas        clamp(device_point(x_in, x*, lambda*), l, u)

`phi_exact` evaluates a row of an NLPDescription in mpmath at a float64 point through sep_ref / tape_ref / quad_ref (kkt_ref._row_exact)
and returns, with phi, the bound E_i those modules derive for a DEVICE evaluation of the row at that point.  `lambda_bar` is the
exact boundary point: 1 where phi(1) <= 0, else the root of phi on (0, 1) (mpmath bisection for separable rows, esh_ref.exact_root;
bisection over float64 lam on the exact phi otherwise)."""
import math

import numpy as np
from mpmath import mp, mpf

import esh_ref
import kkt_ref

ROW_SEP, ROW_TAPE, ROW_HOST, ROW_QUAD = 0, 1, 2, 3
NONFINITE = (ValueError, ZeroDivisionError, TypeError)      # what the reference modules raise where a row is not finite
PREC = kkt_ref.PREC


def sides(d, lb, ub):
    """sigma per row of the description (0: the row does not take part); raises on a nonlinear row with two finite sides"""
    out = np.zeros(d.num_constr, dtype=np.int64)
    for i in range(d.num_constr):
        if d.row_linear[i] or int(d.row_kind[i]) not in (ROW_SEP, ROW_TAPE, ROW_QUAD):
            continue
        lf, uf = math.isfinite(lb[i]), math.isfinite(ub[i])
        if lf and uf:
            raise ValueError("row %d has two finite sides" % i)
        out[i] = 1 if uf else (-1 if lf else 0)
    return out


def device_point(xi, xs, lam):
    """esh_point of csrc/esh.hpp in float64: x* itself at lam == 1, x_in + lam (x* - x_in) (three roundings) otherwise"""
    xi, xs = np.asarray(xi, dtype=np.float64), np.asarray(xs, dtype=np.float64)
    if lam == 1.0:
        return xs.copy()
    return xi + np.float64(lam) * (xs - xi)


def x_feas(xi, xs, lam, l, u):
    return np.minimum(np.maximum(device_point(xi, xs, lam), l), u)


def search(phi_fn, tau, iters=20):
    """feas_step of csrc/feas.hpp in float64.  phi_fn(lam) -> (phi, dphi, finite).  Returns (lambda_i, converged, passes)."""
    lo, hi, lam = 0.0, 1.0, 1.0
    for k in range(iters):
        f, df, fin = phi_fn(lam)
        if fin and f <= 0.0:
            lo = lam
            if lam == 1.0 or f >= -tau:
                return lo, True, k + 1
        else:
            hi = lam
        with np.errstate(all="ignore"):
            nl = lam - (f + 0.5 * tau) / df if df != 0.0 else math.nan
        if not (fin and df > 0.0 and math.isfinite(nl) and lo < nl < hi):
            nl = 0.5 * (lo + hi)
        lam = nl
    return lo, False, iters


def sep_row(d, i):
    """row i of the description as an esh_ref.SepRow"""
    b, e = int(d.rowptr[i]), int(d.rowptr[i + 1])
    return esh_ref.SepRow(d.col[b:e], [int(k) for k in d.atom_kind[b:e]], [float(v) for v in d.p0[b:e]], [float(v) for v in d.p1[b:e]],
                          float(d.rconst[i]))


def row_exact(d, i, x):
    """(g, E) of row i at the float64 point x: exact to PREC bits, E the bound of a device evaluation (sep_ref / tape_ref / quad_ref)"""
    b, e = int(d.rowptr[i]), int(d.rowptr[i + 1])
    k, cols = int(d.row_kind[i]), d.col[b:e]
    x = np.asarray(x, dtype=np.float64)
    if k == ROW_SEP:
        g, eg, _ = kkt_ref._row_exact(k, cols, x, sep=(d.atom_kind[b:e], d.p0[b:e], d.p1[b:e]), rconst=float(d.rconst[i]))
    elif k == ROW_TAPE:
        tb, te = int(d.tape_ptr[i]), int(d.tape_ptr[i + 1])
        g, eg, _ = kkt_ref._row_exact(k, cols, x, tape=(d.tape_op[tb:te], d.tape_arg[tb:te]), rconst=float(d.rconst[i]))
    else:
        g, eg, _ = kkt_ref._row_exact(k, cols, x, quad=(d.p0[b:e], d.quad_ptr[b:e + 1], d.quad_col, d.quad_val), rconst=float(d.rconst[i]))
    return g, eg


def objective_exact(d, x):
    """(f, E) of the objective row at the float64 point x (the caller's sense; the device forms f = (f - t) + t)"""
    x = np.asarray(x, dtype=np.float64)
    with mp.workprec(PREC):
        if d.obj_kind == ROW_SEP:
            f, ef, _ = kkt_ref._row_exact(ROW_SEP, d.obj_col, x, sep=(d.obj_atom_kind, d.obj_p0, d.obj_p1), rconst=d.obj_const)
        elif d.obj_kind == ROW_TAPE:
            cols = sorted({int(a) for o, a in zip(d.obj_tape_op, d.obj_tape_arg) if int(o) == 1})
            f, ef, _ = kkt_ref._row_exact(ROW_TAPE, cols, x, tape=(d.obj_tape_op, d.obj_tape_arg), rconst=d.obj_const)
        else:
            f, ef, _ = kkt_ref._row_exact(ROW_QUAD, d.obj_col, x, quad=(d.obj_p0, d.obj_quad_ptr, d.obj_quad_col, d.obj_quad_val), rconst=d.obj_const)
        return f, ef + 8 * mpf(kkt_ref.U) * abs(f)


def phi_exact(d, i, xi, xs, side, bound, lam):
    """(phi, E_i) of row i at the device's point for lam, in mpmath"""
    with mp.workprec(PREC):
        g, eg = row_exact(d, i, device_point(xi, xs, lam))
        return side * (g - mpf(float(bound))), eg


def phi_f64(d, i, xi, xs, side, bound):
    """lam -> (phi, dphi, finite) in float64 for the reference search: separable rows through esh_ref.phi, the others from the exact
    value rounded and a central difference of it (the reference search needs a derivative, not the device's bits)"""
    if int(d.row_kind[i]) == ROW_SEP:
        row = sep_row(d, i)

        def fn(lam):
            with np.errstate(all="ignore"):
                try:
                    f, df, grad, _ = esh_ref.phi(row, np.asarray(xi, dtype=np.float64), np.asarray(xs, dtype=np.float64), side, bound, lam)
                except NONFINITE:
                    return math.inf, math.nan, False
            return f, df, math.isfinite(f) and all(math.isfinite(v) for v in grad)
        return fn

    def fn(lam):
        h = 1e-6
        with mp.workprec(PREC):
            try:
                f = float(phi_exact(d, i, xi, xs, side, bound, lam)[0])
                a = float(phi_exact(d, i, xi, xs, side, bound, max(lam - h, 0.0))[0])
                b = float(phi_exact(d, i, xi, xs, side, bound, min(lam + h, 1.0))[0]) if lam < 1.0 else f
            except NONFINITE:
                return math.inf, math.nan, False
        df = (b - a) / (min(lam + h, 1.0) - max(lam - h, 0.0))
        return f, df, math.isfinite(f) and math.isfinite(df)
    return fn


def lambda_bar(d, i, xi, xs, side, bound):
    """the exact boundary point of row i on the segment as an mpf: 1 where phi(1) <= 0, else the root of phi in (0, 1)"""
    with mp.workprec(PREC):
        try:
            f1 = phi_exact(d, i, xi, xs, side, bound, 1.0)[0]
        except NONFINITE:
            f1 = mp.inf
        if mp.isfinite(f1) and f1 <= 0:
            return mpf(1)
        if int(d.row_kind[i]) == ROW_SEP and mp.isfinite(f1):
            return esh_ref.exact_root(sep_row(d, i), xi, xs, side, bound)
        lo, hi = 0.0, 1.0
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if phi_exact(d, i, xi, xs, side, bound, mid)[0] < 0:
                lo = mid
            else:
                hi = mid
        return mpf(hi)


def reduce_lambdas(lams, sig):
    """(lambda*, blocking row) from lambda_i by row: the minimum over the taking-part rows and the smallest row attaining it when
    it lies below 1 (-1 otherwise)"""
    best, row = 1.0, -1
    for i, (lam, s) in enumerate(zip(lams, sig)):
        if s != 0 and lam < best:
            best, row = float(lam), i
    return best, row


def linear_violation(d, lb, ub, x):
    """the largest violation of a declared-linear separable row at x, in numpy"""
    worst = 0.0
    for i in range(d.num_constr):
        if not d.row_linear[i]:
            continue
        b, e = int(d.rowptr[i]), int(d.rowptr[i + 1])
        g = float(np.dot(d.p0[b:e], np.asarray(x)[d.col[b:e]]) + d.rconst[i])
        worst = max(worst, g - ub[i], lb[i] - g)
    return worst
