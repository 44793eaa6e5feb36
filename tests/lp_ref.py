"""High-precision reference for the LP kernels: scaling, PDHG step, check sums (test code).

The LP is `(rowptr, col, val, lo, hi, c, l, u, sense)`:  min s c'x,  l <= x <= u,  lo <= A x <= hi,  s = +1 (Min) / -1 (Max).
Everything below is written ONCE, over numpy arrays, and runs either in float64 (`F64`: the bulk twin) or on object arrays
of mpmath numbers at 200 bits (`MP`: the reference proper; about 3 us per arithmetic operation).

Scaled problem (kernels.hpp k_prep_both, k_scale_vals), with the row factors dr and the column factors dc:

    A^_ij = dr_i a_ij dc_j    c^ = s c dc    l^ = l / dc   u^ = u / dc    lo^ = lo dr   hi^ = hi dr   (NaN row bound = vacuous side)
    x^ = clip(x / dc, l^, u^)    y^ = y / dr

One PDHG point from (x^, y^) (k_pdhg_x, k_pdhg_y), tau = eta / omega, sigma = eta omega:

    xt = clip(x^ - tau (c^ - A^'y^), l^, u^)     v = y^ - sigma A^(2 xt - x^)     yt = v + sigma clip(-v / sigma, lo^, hi^)

and the reflected Halpern update with weight w = (k + 1) / (k + 2) and anchors:  z <- w (2 zt - z) + (1 - w) z0.

Check sums (kernels.hpp above chk_row_accumulate and k_chk_cols), dy = yt - y^, dx = xt - x^, r = c^ - A^'yt, r0 = -A^'yt:

    rows     q0 = sum dy (A^ dx)      q1 = sum dy^2      q2 = sum [lo^ yt if yt > 0, lo^ finite | hi^ yt if yt < 0, hi^ finite]
             q3 = sum (yt - y0)^2     q4 = sum yt^2      q10 = the absolute values of q2's terms
             q12 = max_i max(lo^ - A^xt, A^xt - hi^, 0)_i / dr_i
    columns  q16+5 = sum dx^2         q16+6 = c^'xt      q16+7 = sum [l^ r if r > 0, l^ finite | u^ r if r < 0, u^ finite]
             q16+8 = sum (xt - x0)^2  q16+9 = sum xt^2   q16+10, q16+11: q16+7 and its absolute terms with r0 in place of r
             q16+13 = max_j (|r_j| where the bound on r's side is infinite) / dc_j      q16+14 = the same for r0, not divided

Ruiz / Pock-Chambolle equilibration (k_scale_stat_upd_both): `passes` max-norm passes, then one sum-norm pass; in each, with the
factors of the pass before on BOTH sides,  stat_i = dr_i * red_e(|a_e| dc_col(e)),  dr_i <- dr_i / sqrt(stat_i)  where stat_i is
positive and finite (an empty row or column keeps its factor), and the same for the columns.

Error bounds
------------
u = 2^-53; + - * / sqrt correctly rounded (-ffp-contract=off: no fused operation).  First-order forward bounds, every final
bound DOUBLED for the higher-order terms (as tests/sep_ref.py does).  e(.) is an absolute error bound.

* A sum of k terms t_e in ANY order: (D + 1) u sum |t_e| + sum e(t_e), D <= k the longest chain of additions; D = k is used
  throughout, so the bound holds for every summation shape the kernels have (lane groups, trips, long-row workgroups, tiles).
* Scaled data: A^ takes two roundings, e = 2u |A^|; c^, l^, u^, lo^, hi^, y^ one, e = u |.|; x^ = clip(fl(x / dc), l^, u^) and clip
  is non-expansive in all three arguments: e(x^) = u |x^|.
* g = A^'y^:  e(g) = (D + 1) u S + sum (2u |A^| |y^| + |A^| e(y^)),  S = sum |A^| |y^|.
  r = c^ - g:  e(r) = u |c^| + e(g) + u |r|.    z = x^ - fl(tau r):  e(z) = e(x^) + tau e(r) + u |tau r| + u |z|.
  xt = clip(z, l^, u^):  e(xt) = e(z) + u |xt|   (the u |xt|: the rounded bound, when the clip is active).
* h = A^(2 xt - x^), computed either from xbar = fl(2 xt - x^) or as 2 fl(A^xt) - fl(A^x^) (check form); both are covered by
  e(h) = (D + 4) u sum |A^| (2 |xt| + |x^|) + sum |A^| (2 e(xt) + e(x^)) + u |h|.   The check form's A^xt and A^x^ alone:
  e(A^p) = (D + 3) u sum |A^| |p| + sum |A^| e(p).
* v = y^ - fl(sigma h):  e(v) = e(y^) + sigma e(h) + u |sigma h| + u |v|.
  yt = F(v) = v + sigma clip(-v / sigma, lo^, hi^).  F is non-expansive, and its own roundings (the quotient, the rounded bound,
  the product, the sum) add u (|v| + 2 sigma |clip| + |yt|):   e(yt) = e(v) + u (|v| + 2 sigma |clip| + |yt|).
* Halpern, a = fl(2 zt - z), z+ = fl(fl(w a) + fl(fl(1 - w) z0)):
  e(z+) = w (2 e(zt) + e(z)) + (1 - w) e(z0) + u (2 |w a| + 2 |(1 - w) z0| + |z+|).
* Check sums, N terms each: (N + 1) u sum |term| + sum e(term) with
    dy, dx, yt - y0, xt - x0:  the operands' errors + u |difference|;     squares p^2:  2 |p| e(p) + u p^2;
    dy (A^ dx):  |dy| e(A^dx) + |A^dx| e(dy) + u |term|,  e(A^dx) = e(A^xt) + e(A^x^) + u |A^dx|;    c^ xt:  |c^| e(xt) + u |c^| |xt| + u |term|;
    dual-objective terms b p (b the bound picked by the sign of p; p = yt, r or r0):  B e(p) + 2u |b p|,  B the largest FINITE
    bound of the row / column -- the term is continuous and piecewise linear in p through the sign test at p = 0, with slopes lo^
    and hi^ (an infinite side contributes nothing on either side of an exact zero), so B e(p) also covers a sign that flips within e(p);
    the same bound for the sums of absolute terms.
* Maxima take the error of their argument:  q12: (e(A^xt) + u |bound| + u |bound - A^xt|) / dr + u viol;   q16+13: e(r) / dc + u |r| / dc;
  q16+14: e(A^'yt); the bound of a maximum is the largest bound of its candidates.
* Scaling, relative errors.  d+ = d / sqrt(d stat') = sqrt(d / stat'), stat' = red |a| d_other:  e+ <= e_self / 2 + e_other / 2 + 4u for a
  max-norm pass (product, statistic's product, square root, quotient; max is non-expansive), hence <= e + 4u with e the largest
  error over both sides; the sum-norm pass adds (k + 1) u for the sum of the k terms of the longest row or column.
  E_scale = 2 ((4 passes + 4 + k + 1) u).

A device value passes against the MP value within the bound, against the F64 twin (itself within the bound) within twice the bound.
"""
import numpy as np
from mpmath import mp, mpf
import mpmath

U = 2.0 ** -53
PREC = 200
INF = float("inf")


class Arith:
    """float64 or mpmath-at-200-bits arrays under one set of numpy expressions"""

    def __init__(self, exact):
        self.exact = exact
        self._sqrt = np.frompyfunc(lambda v: mpmath.sqrt(v), 1, 1)

    def arr(self, a):
        a = np.asarray(a, dtype=np.float64)
        if not self.exact:
            return a.copy()
        out = np.empty(a.shape, dtype=object)
        out[...] = [mpf(float(v)) for v in a.ravel()] if a.ndim else mpf(float(a))
        return out

    def num(self, v):
        return mpf(float(v)) if self.exact else float(v)

    def zeros(self, n):
        return self.arr(np.zeros(n))

    def sqrt(self, a):
        return self._sqrt(a) if self.exact else np.sqrt(a)

    def f64(self, a):
        return np.array([float(v) for v in np.asarray(a).ravel()], dtype=np.float64).reshape(np.shape(a))


F64, MP = Arith(False), Arith(True)


def _prec(fn):
    def wrapped(*a, **kw):
        with mp.workprec(PREC):
            return fn(*a, **kw)
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


class LP:
    def __init__(self, rowptr, col, val, lo, hi, c, l, u, sense="Min"):
        self.rowptr = np.asarray(rowptr, dtype=np.int64); self.col = np.asarray(col, dtype=np.int64)
        self.val = np.asarray(val, dtype=np.float64)
        self.lo = np.asarray(lo, dtype=np.float64).copy(); self.hi = np.asarray(hi, dtype=np.float64).copy()
        self.c = np.asarray(c, dtype=np.float64); self.l = np.asarray(l, dtype=np.float64); self.u = np.asarray(u, dtype=np.float64)
        self.sense = sense
        self.m, self.n = len(self.rowptr) - 1, len(self.c)
        self.lo[np.isnan(self.lo)] = -INF                  # NaN bound = vacuous side
        self.hi[np.isnan(self.hi)] = INF
        self.row = np.repeat(np.arange(self.m), np.diff(self.rowptr))
        self.perm = np.argsort(self.col, kind="stable")    # the column mirror: a column's entries in row order
        self.cptr = np.concatenate([[0], np.cumsum(np.bincount(self.col, minlength=self.n))]).astype(np.int64)
        self.rlen, self.clen = np.diff(self.rowptr), np.diff(self.cptr)

    def dense(self):
        A = np.zeros((self.m, self.n))
        np.add.at(A, (self.row, self.col), self.val)
        return A


def _segsum(v, ptr, zero):
    """sum of v[ptr[i]:ptr[i+1]] for every i (empty segments give `zero`)"""
    n = len(ptr) - 1
    out = np.empty(n, dtype=v.dtype); out[...] = zero
    ne = ptr[1:] > ptr[:-1]
    if ne.any():
        out[ne] = np.add.reduceat(v, ptr[:-1][ne])
    return out


def _segmax(v, ptr, zero):
    n = len(ptr) - 1
    out = np.empty(n, dtype=v.dtype); out[...] = zero
    ne = ptr[1:] > ptr[:-1]
    if ne.any():
        out[ne] = np.maximum.reduceat(v, ptr[:-1][ne])
    return out


def rows_dot(lp, Av, p, zero=0.0):
    return _segsum(Av * p[lp.col], lp.rowptr, zero)


def cols_dot(lp, Av, p, zero=0.0):
    return _segsum((Av * p[lp.row])[lp.perm], lp.cptr, zero)


def _clip(v, a, b):
    return np.minimum(np.maximum(v, a), b)


class Scaled:
    pass


@_prec
def scale_problem(lp, dr, dc, ar):
    S = Scaled()
    S.lp, S.ar = lp, ar
    S.dr, S.dc = ar.arr(dr), ar.arr(dc)
    S.A = S.dr[lp.row] * ar.arr(lp.val) * S.dc[lp.col]
    s = -1.0 if lp.sense == "Max" else 1.0
    S.c = ar.arr(s * lp.c) * S.dc
    S.l, S.u = ar.arr(lp.l) / S.dc, ar.arr(lp.u) / S.dc
    S.lo, S.hi = ar.arr(lp.lo) * S.dr, ar.arr(lp.hi) * S.dr
    S.zero = ar.num(0.0)
    return S


@_prec
def scale_state(S, x, y):
    return _clip(S.ar.arr(x) / S.dc, S.l, S.u), S.ar.arr(y) / S.dr


@_prec
def pdhg_point(S, xh, yh, tau, sigma):
    """(xt, yt) and the intermediates the bounds and the check sums need"""
    lp, ar = S.lp, S.ar
    tau, sigma = ar.num(tau), ar.num(sigma)
    P = Scaled()
    P.g = cols_dot(lp, S.A, yh, S.zero)
    P.r = S.c - P.g
    P.z = xh - tau * P.r
    P.xt = _clip(P.z, S.l, S.u)
    P.axt, P.axk = rows_dot(lp, S.A, P.xt, S.zero), rows_dot(lp, S.A, xh, S.zero)
    P.h = 2 * P.axt - P.axk
    P.v = yh - sigma * P.h
    P.cl = _clip(-P.v / sigma, S.lo, S.hi)
    P.yt = P.v + sigma * P.cl
    return P


@_prec
def halpern(S, z, zt, z0, k):
    w = S.ar.num((k + 1.0) / (k + 2.0))              # the float64 weight the host passes to the kernels
    return w * (2 * zt - z) + (1 - w) * z0


@_prec
def check_sums(S, xh, yh, x0h, y0h, P):
    """the 32 sums of a check at (xh, yh) with anchors (x0h, y0h); P = pdhg_point(S, xh, yh, ...)"""
    lp, ar = S.lp, S.ar
    q = [S.zero] * 32
    flo, fhi = np.isfinite(lp.lo), np.isfinite(lp.hi)
    fl_, fu_ = np.isfinite(lp.l), np.isfinite(lp.u)
    tot = lambda a: (a.sum() if len(a) else S.zero) + S.zero
    big = lambda a: (np.maximum.reduce(a) if len(a) else S.zero)
    yt, xt = P.yt, P.xt
    dy = yt - yh
    q[0] = tot(dy * (P.axt - P.axk)); q[1] = tot(dy * dy)
    pos, neg = (yt > 0) & flo, (yt < 0) & fhi
    t2 = np.where(pos, np.where(flo, S.lo, 0) * yt, np.where(neg, np.where(fhi, S.hi, 0) * yt, S.zero))
    q[2] = tot(t2); q[10] = tot(np.abs(t2))
    q[3] = tot((yt - y0h) ** 2); q[4] = tot(yt * yt)
    viol = np.maximum(np.maximum(np.where(flo, S.lo, 0) - P.axt, S.zero) * flo, np.maximum(P.axt - np.where(fhi, S.hi, 0), S.zero) * fhi) / S.dr
    q[12] = big(viol)
    aty = cols_dot(lp, S.A, yt, S.zero)
    dx = xt - xh
    q[16 + 5] = tot(dx * dx); q[16 + 6] = tot(S.c * xt)
    q[16 + 8] = tot((xt - x0h) ** 2); q[16 + 9] = tot(xt * xt)
    for r, qs, qa, qm, div in ((S.c - aty, 16 + 7, None, 16 + 13, S.dc), (-aty, 16 + 10, 16 + 11, 16 + 14, None)):
        pos, neg = r > 0, r < 0
        t = np.where(pos & fl_, np.where(fl_, S.l, 0) * r, np.where(neg & fu_, np.where(fu_, S.u, 0) * r, S.zero))
        bad = np.where(pos & ~fl_, r, np.where(neg & ~fu_, -r, S.zero))
        q[qs] = tot(t)
        if qa is not None:
            q[qa] = tot(np.abs(t))
        q[qm] = big(bad / div if div is not None else bad)
    P.aty = aty
    return np.array(q, dtype=object) if ar.exact else np.array(q, dtype=np.float64)


# ------------------------------------------------------------------------------------------------- bounds (float64)
class Bounds:
    pass


def state_bounds(S, xh, yh):
    return U * np.abs(xh), U * np.abs(yh)


def point_bounds(S, xh, yh, P, tau, sigma, ex, ey):
    """first-order bounds (NOT yet doubled) of the quantities of pdhg_point, from the F64 twin's values"""
    lp = S.lp
    aA = np.abs(S.A)
    B = Bounds()
    Dc, Dr = lp.clen.astype(float), lp.rlen.astype(float)
    B.g = (Dc + 3) * U * cols_dot(lp, aA, np.abs(yh)) + cols_dot(lp, aA, ey)
    B.r = U * np.abs(S.c) + B.g + U * np.abs(P.r)
    B.z = ex + tau * B.r + U * np.abs(tau * P.r) + U * np.abs(P.z)
    B.xt = B.z + U * np.abs(P.xt)
    B.axt = (Dr + 3) * U * rows_dot(lp, aA, np.abs(P.xt)) + rows_dot(lp, aA, B.xt)
    B.axk = (Dr + 3) * U * rows_dot(lp, aA, np.abs(xh)) + rows_dot(lp, aA, ex)
    B.h = (Dr + 4) * U * rows_dot(lp, aA, 2 * np.abs(P.xt) + np.abs(xh)) + rows_dot(lp, aA, 2 * B.xt + ex) + U * np.abs(P.h)
    B.v = ey + sigma * B.h + U * np.abs(sigma * P.h) + U * np.abs(P.v)
    B.yt = B.v + U * (np.abs(P.v) + 2 * sigma * np.abs(P.cl) + np.abs(P.yt))
    return B


def halpern_bound(z, zt, z0, zn, k, ez, ezt, ez0):
    w = (k + 1.0) / (k + 2.0)
    return w * (2 * ezt + ez) + (1 - w) * ez0 + U * (2 * np.abs(w * (2 * zt - z)) + 2 * np.abs((1 - w) * z0) + np.abs(zn))


def check_bounds(S, xh, yh, x0h, y0h, P, B, ex, ey, ex0, ey0):
    """first-order bounds (NOT yet doubled) of the 32 check sums; P must carry aty (check_sums ran on it)"""
    lp = S.lp
    aA = np.abs(S.A)
    m, n = lp.m, lp.n
    e = np.zeros(32)
    ssum = lambda N, t, et: (N + 1) * U * np.sum(np.abs(t)) + np.sum(et)
    sq = lambda p, ep: (p * p, 2 * np.abs(p) * ep + U * p * p)
    flo, fhi, fl_, fu_ = np.isfinite(lp.lo), np.isfinite(lp.hi), np.isfinite(lp.l), np.isfinite(lp.u)
    yt, xt = P.yt, P.xt
    dy = yt - yh; edy = B.yt + ey + U * np.abs(dy)
    adx = P.axt - P.axk; eadx = B.axt + B.axk + U * np.abs(adx)
    t = dy * adx
    e[0] = ssum(m, t, np.abs(dy) * eadx + np.abs(adx) * edy + U * np.abs(t))
    e[1] = ssum(m, *sq(dy, edy))
    Brow = np.maximum(np.where(flo, np.abs(S.lo), 0.0), np.where(fhi, np.abs(S.hi), 0.0))
    t2 = np.where((yt > 0) & flo, np.where(flo, S.lo, 0) * yt, np.where((yt < 0) & fhi, np.where(fhi, S.hi, 0) * yt, 0.0))
    e[2] = e[10] = ssum(m, t2, Brow * B.yt + 2 * U * np.abs(t2))
    d0 = yt - y0h
    e[3] = ssum(m, *sq(d0, B.yt + ey0 + U * np.abs(d0)))
    e[4] = ssum(m, *sq(yt, B.yt))
    with np.errstate(invalid="ignore"):
        dlo, dhi = np.where(flo, S.lo - P.axt, 0.0), np.where(fhi, P.axt - S.hi, 0.0)
    viol = np.maximum(np.maximum(dlo, dhi), 0.0) / S.dr
    ev = (B.axt + U * Brow + U * np.maximum(np.abs(dlo), np.abs(dhi))) / S.dr + U * viol
    e[12] = np.max(ev) if m else 0.0
    Dc = lp.clen.astype(float)
    eaty = (Dc + 3) * U * cols_dot(lp, aA, np.abs(yt)) + cols_dot(lp, aA, B.yt)
    dx = xt - xh
    e[16 + 5] = ssum(n, *sq(dx, B.xt + ex + U * np.abs(dx)))
    t = S.c * xt
    e[16 + 6] = ssum(n, t, np.abs(S.c) * B.xt + 2 * U * np.abs(t))
    d0 = xt - x0h
    e[16 + 8] = ssum(n, *sq(d0, B.xt + ex0 + U * np.abs(d0)))
    e[16 + 9] = ssum(n, *sq(xt, B.xt))
    Bcol = np.maximum(np.where(fl_, np.abs(S.l), 0.0), np.where(fu_, np.abs(S.u), 0.0))
    for r, er, qs, qa, qm, div in ((S.c - P.aty, U * np.abs(S.c) + eaty + U * np.abs(S.c - P.aty), 16 + 7, None, 16 + 13, S.dc),
                                   (-P.aty, eaty, 16 + 10, 16 + 11, 16 + 14, None)):
        t = np.where((r > 0) & fl_, np.where(fl_, S.l, 0) * r, np.where((r < 0) & fu_, np.where(fu_, S.u, 0) * r, 0.0))
        e[qs] = ssum(n, t, Bcol * er + 2 * U * np.abs(t))
        if qa is not None:
            e[qa] = e[qs]
        e[qm] = np.max(er / div + U * np.abs(r) / div) if div is not None else np.max(er)
    return e


# ------------------------------------------------------------------------------------------------- scaling
@_prec
def ruiz(lp, passes, ar, return_pre=True):
    """(dr, dc, dr_r, dc_r): `passes` max-norm passes and one sum-norm pass; dr_r, dc_r are the factors before the last"""
    aval = ar.arr(np.abs(lp.val))
    dr, dc = ar.arr(np.ones(lp.m)), ar.arr(np.ones(lp.n))
    zero = ar.num(0.0)
    dr_r, dc_r = dr, dc
    for it in range(passes + 1):
        last = it == passes
        if last:
            dr_r, dc_r = dr.copy(), dc.copy()
        red = _segsum if last else _segmax
        sr = dr * red(aval * dc[lp.col], lp.rowptr, zero)
        sc = dc * red((aval * dr[lp.row])[lp.perm], lp.cptr, zero)
        new = []
        for d, st in ((dr, sr), (dc, sc)):
            ok = np.array([bool(v > 0) and np.isfinite(float(v)) for v in st], dtype=bool)
            dn = d.copy()
            if ok.any():
                dn[ok] = d[ok] / ar.sqrt(st[ok])
            new.append(dn)
        dr, dc = new
    return dr, dc, dr_r, dc_r


def scale_bound(lp, passes, last=True):
    """relative bound of the factors after `passes` max-norm passes (and the sum-norm pass), doubled"""
    k = int(max(lp.rlen.max() if lp.m else 0, lp.clen.max() if lp.n else 0))
    return 2 * (4 * passes + ((4 + k + 1) if last else 0)) * U


# ------------------------------------------------------------------------------------------------- one call for the tests
class Case:
    """reference values and DOUBLED bounds of: the scaled state, one plain step from it (xn, yn), the point (xt, yt), the check
    sums q, and the step after a restart at (xt, yt) (xr, yr) -- in float64 (`.f`) and, with exact=True, in mpmath (`.x`,
    converted to float64 after the computation)"""
    pass


def _run(lp, dr, dc, x, y, x0, y0, eta, omega, k, ar):
    tau, sigma = eta / omega, eta * omega              # the float64 step sizes of the host code
    S = scale_problem(lp, dr, dc, ar)
    xh, yh = scale_state(S, x, y)
    x0h, y0h = scale_state(S, x0, y0)
    P = pdhg_point(S, xh, yh, tau, sigma)
    R = Scaled()
    R.S, R.P, R.xh, R.yh, R.x0h, R.y0h = S, P, xh, yh, x0h, y0h
    R.xn, R.yn = halpern(S, xh, P.xt, x0h, k), halpern(S, yh, P.yt, y0h, k)
    R.q = check_sums(S, xh, yh, x0h, y0h, P)
    P2 = pdhg_point(S, P.xt, P.yt, tau, sigma)         # after a restart: state = anchors = (xt, yt), k = 0
    R.P2 = P2
    R.xr, R.yr = halpern(S, P.xt, P2.xt, P.xt, 0), halpern(S, P.yt, P2.yt, P.yt, 0)
    return R


NAMES = ("xh", "yh", "x0h", "y0h", "xt", "yt", "xn", "yn", "xr", "yr", "q")


def _values(R, ar):
    d = dict(xh=R.xh, yh=R.yh, x0h=R.x0h, y0h=R.y0h, xt=R.P.xt, yt=R.P.yt, xn=R.xn, yn=R.yn, xr=R.xr, yr=R.yr, q=R.q)
    return {k_: ar.f64(v) for k_, v in d.items()}


def case(lp, dr, dc, x, y, x0, y0, eta, omega, k, exact=True):
    C = Case()
    tau, sigma = eta / omega, eta * omega
    R = _run(lp, dr, dc, x, y, x0, y0, eta, omega, k, F64)
    C.f = _values(R, F64)
    S, P = R.S, R.P
    ex, ey = state_bounds(S, R.xh, R.yh)
    ex0, ey0 = state_bounds(S, R.x0h, R.y0h)
    B = point_bounds(S, R.xh, R.yh, P, tau, sigma, ex, ey)
    bq = check_bounds(S, R.xh, R.yh, R.x0h, R.y0h, P, B, ex, ey, ex0, ey0)
    B2 = point_bounds(S, P.xt, P.yt, R.P2, tau, sigma, B.xt, B.yt)
    C.b = dict(xh=2 * ex, yh=2 * ey, x0h=2 * ex0, y0h=2 * ey0, xt=2 * B.xt, yt=2 * B.yt, q=2 * bq,
               xn=2 * halpern_bound(R.xh, P.xt, R.x0h, R.xn, k, ex, B.xt, ex0),
               yn=2 * halpern_bound(R.yh, P.yt, R.y0h, R.yn, k, ey, B.yt, ey0),
               xr=2 * halpern_bound(P.xt, R.P2.xt, P.xt, R.xr, 0, B.xt, B2.xt, B.xt),
               yr=2 * halpern_bound(P.yt, R.P2.yt, P.yt, R.yr, 0, B.yt, B2.yt, B.yt))
    C.x = _values(_run(lp, dr, dc, x, y, x0, y0, eta, omega, k, MP), MP) if exact else None
    return C


def compare(C, name, dev):
    """largest |dev - ref| / bound over the entries of quantity `name` (<= 1 passes): against the exact values where the case has
    them, else against the float64 twin with twice the bound; an entry whose bound is 0 must match exactly"""
    ref, slack = (C.x[name], 1.0) if C.x is not None else (C.f[name], 2.0)
    dev = np.asarray(dev, dtype=np.float64)
    assert dev.shape == ref.shape, (name, dev.shape, ref.shape)
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(C.b[name])), name
    if not np.all(np.isfinite(dev)):
        return INF
    d, b = np.abs(dev - ref), slack * C.b[name]
    ratio = np.where(d == 0.0, 0.0, d / np.where(b > 0, b, 1.0))
    ratio = np.where((b == 0) & (d > 0), INF, ratio)
    return float(np.max(ratio)) if ratio.size else 0.0
