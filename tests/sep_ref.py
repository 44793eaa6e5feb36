"""High-precision reference for separable-atom rows (test code).

A row is `(col, kind, p0, p1, rconst)`: g(x) = sum_e atom_e(x[col_e]) + rconst with the atoms of include/katana_hip.h
(KTN_ATOM_*) and the formulas of kernels.hpp `atom_eval`:

    LIN     val = a x               der = a
    QUAD    val = a (x - b)^2       der = 2 a (x - b)
    EXP     val = a exp(b x)        der = b a exp(b x)
    NEGLOG  val = -a log(x + b)     der = -a / (x + b)

`row_ref_mp` evaluates one row in mpmath at 200 bits: the exact g, every exact partial J_c, the exact cut constant
b = g - sum x_c J_c (src/algorithms.jl:3-18), mag = sum |term| + |rconst| and dotmag = sum |x_c J_c|.  `rows_ref_f64`
does the same for all rows of a CSR structure at once in float64 numpy (for the bulk of large cases: mpmath costs
about 70 us per entry).  Both carry the float64 class (NaN, +inf, -inf) wherever the float64 result is not finite, under
the convention of oracle/evaluators.py `_atoms`: log of a negative is NaN, -a log 0 = +inf with partial -inf, exp
overflows to +inf.

Error bounds (u = 2^-53; + - * / correctly rounded, a fused multiply-add only removes a rounding; device exp / log within
4 ulp, the project's convention, and 1 ulp <= 2u relative, so 8u; h = 2^-1074 the spacing of the subnormals).  First-order
forward errors of the formulas as `atom_eval` writes them, with d_k relative roundings |d_k| <= u:

* LIN     val = fl(a x): |err| <= u |val|.  der = a: exact.
* QUAD    d = fl(x - b) = (x - b)(1 + d1), val = fl(fl(a d) d) = a (x-b)^2 (1 + d1)^2 (1 + d2)(1 + d3): <= 4u |val|.
          der = fl(fl(2 a) d), 2a exact: <= 2u |der|.
* EXP     t = fl(b x) = b x (1 + d1) gives exp(t) = exp(b x) exp(b x d1): a relative error of |b x| u in the value; exp itself
          8u; e = fl(a exp): u.  val: <= (|b x| + 9) u |val| + (4 |a| + 1) h   (the h term: a result of exp in the subnormal
          range -- exp(-750) rounds to 0 -- has an absolute, not a relative, error; times a, and the product's own h).
          der = fl(b e): one more rounding: <= (|b x| + 10) u |der| + (|b| (4 |a| + 1) + 1) h.
* NEGLOG  s = fl(x + b) = (x + b)(1 + d1): an absolute error of |a / s| |s| u = |a| u in the value; log 8u, the product u.
          val: <= |a| u + 9u |val|.   der = fl(-a / s): <= 2u |der|.
* x_c J_c (the cut constant's terms): fl(x der): <= |x| err(der) + u |x der| + h.

Sums.  g = (sum of k terms) + rconst, computed in ANY order by k additions; a term takes part in at most D of them and each
rounds a partial sum that is at most mag in absolute value, so the additions contribute at most D u mag, D <= k: with the
final rounding, (k + 1) u mag.  A kernel with a documented summation shape has a smaller D (`depth`): its longest chain of
additions -- e.g. k_sep_eval_long: ceil(k / 1024) per thread, 6 butterfly levels, 15 wavefront partials in order, rconst.

    E_g   = 2 (sum_e err(val_e) + (D + 1) u mag)              (first order, doubled for the higher-order terms)
    E_dot = 2 (sum_e err(x_e der_e) + (D + 1) u dotmag)
    E_b   = E_g + E_dot + 2u (mag + dotmag)                   (b = fl(g - dot))
    partial J_e:   2 err(der_e)                               (single formulas: a few ulp each; LIN exactly)
    cut bounds lo = fl(lb - b), hi = fl(ub - b):   E_b + 2u |bound - b|      (src/model.jl:74-75)

A device value passes against the exact value within the bound.  Against the float64 evaluation (itself within the bound of
the exact value, whatever numpy's summation order) it passes within TWICE the bound (`RowsRef.slack` = 2).
Where the float64 result is not finite the device must give exactly its class.  Edge rows keep to ONE non-finite source, so
the class does not depend on the order of the sum.
"""
import math

import numpy as np
from mpmath import mp, mpf
import mpmath

LIN, QUAD, EXP, NEGLOG = 0, 1, 2, 3
U = 2.0 ** -53
H = 2.0 ** -1074
PREC = 200
F_TOL = 2.0 ** -20          # dyadic, so that threshold rows are exact (the new tests' only literal tolerance)


def same_class(a, b):
    """NaN matches NaN, inf matches inf of the same sign, finite values match exactly"""
    if a != a or b != b:
        return a != a and b != b
    return a == b


def atoms_f64(kind, p0, p1, xv):
    """value and derivative of every atom in float64 under the oracle's convention (oracle/evaluators.py `_atoms`)"""
    kind = np.asarray(kind)
    p0 = np.asarray(p0, dtype=np.float64); p1 = np.asarray(p1, dtype=np.float64); xv = np.asarray(xv, dtype=np.float64)
    val = np.empty_like(xv); der = np.empty_like(xv)
    with np.errstate(all="ignore"):
        m = kind == LIN
        val[m] = p0[m] * xv[m]; der[m] = p0[m]
        m = kind == QUAD
        d = xv[m] - p1[m]
        val[m] = p0[m] * d * d; der[m] = 2.0 * p0[m] * d
        m = kind == EXP
        e = p0[m] * np.exp(p1[m] * xv[m])
        val[m] = e; der[m] = p1[m] * e
        m = kind == NEGLOG
        s = xv[m] + p1[m]
        val[m] = -p0[m] * np.log(s); der[m] = -p0[m] / s
    return val, der


def atom_bounds(kind, p0, p1, xv, val, der):
    """(err(val), err(der), err(x der)) of the module docstring, from |val| and |der| (float64 arrays; non-finite entries
    give non-finite bounds, which nobody reads)"""
    kind = np.asarray(kind)
    a, b, x = np.abs(p0), np.abs(p1), np.abs(xv)
    av, ad = np.abs(val), np.abs(der)
    ev = np.zeros_like(av); ed = np.zeros_like(av)
    with np.errstate(all="ignore"):
        m = kind == LIN
        ev[m] = U * av[m]
        m = kind == QUAD
        ev[m] = 4 * U * av[m]; ed[m] = 2 * U * ad[m]
        m = kind == EXP
        bx = b[m] * x[m]
        ev[m] = (bx + 9) * U * av[m] + (4 * a[m] + 1) * H
        ed[m] = (bx + 10) * U * ad[m] + (b[m] * (4 * a[m] + 1) + 1) * H
        m = kind == NEGLOG
        ev[m] = a[m] * U + 9 * U * av[m]; ed[m] = 2 * U * ad[m]
        edot = x * ed + U * x * ad + H
    return ev, ed, edot


def long_row_depth(k):
    """longest chain of additions of k_sep_eval_long (kernels.hpp): 1 024 thread-strided partial sums, a 64-lane butterfly,
    the 16 wavefront partials in order, then rconst"""
    return -(-k // 1024) + 6 + 15 + 1                           # (k: an int or an integer array)


class RowRef:
    """One row.  g, b, dot: exact (mpf) or None where the float64 value is not finite; g_f64, b_f64: the float64 values
    (their class counts where they are not finite); der: list of exact partials (None where not finite); der_f64: float64
    partials; val_f64: float64 terms; mag, dotmag; e_g, e_b: the bounds; e_der: per-entry bound of the partials."""
    slack = 1

    def check_g(self, dev, what=""):
        _check(dev, self.g, self.g_f64, self.e_g, self.slack, ("g", what))

    def check_b(self, dev, what=""):
        _check(dev, self.b, self.b_f64, self.e_b, self.slack, ("cut constant", what))

    def check_der(self, dev, what=""):
        assert len(dev) == len(self.der_f64), ("row length", what, len(dev), len(self.der_f64))
        for e, dv in enumerate(dev):
            _check(dv, self.der[e], self.der_f64[e], self.e_der[e], 2 * self.slack, ("partial", what, e))

    def bound_tol(self, bnd):
        """tolerance of a cut's row bound fl(bnd - b) for a finite constraint bound bnd"""
        return self.slack * (self.e_b + 2 * U * abs(bnd - self.b_f64))


def _finite(v):
    return v == v and abs(v) != math.inf


def _check(dev, exact, f64, bound, factor, what):
    dev = float(dev)
    if not _finite(f64):
        assert same_class(dev, f64), ("class",) + what + (dev, f64)
        return
    tol = factor * bound
    err = abs(mpf(dev) - exact) if _finite(dev) else mpf("inf")
    assert err <= tol, what + (dev, float(exact), float(err), float(tol))


def row_ref_mp(col, kind, p0, p1, rconst, x, depth=None):
    """the row in mpmath at PREC bits"""
    col = np.asarray(col, dtype=np.int64); kind = np.asarray(kind, dtype=np.int64)
    p0 = np.asarray(p0, dtype=np.float64); p1 = np.asarray(p1, dtype=np.float64)
    xv = np.asarray(x, dtype=np.float64)[col] if len(col) else np.zeros(0)
    k = len(col)
    D = k if depth is None else depth
    R = RowRef()
    val, der = atoms_f64(kind, p0, p1, xv)
    ev, ed, edot = atom_bounds(kind, p0, p1, xv, val, der)
    with np.errstate(all="ignore"):
        R.val_f64, R.der_f64 = val, der
        R.g_f64 = float(np.sum(val) + rconst) if k else float(rconst)
        dot64 = float(np.sum(xv * der)) if k else 0.0
        R.b_f64 = R.g_f64 - dot64
    with mp.workprec(PREC):
        g = mpf(rconst); mag = abs(mpf(rconst)); dot = mpf(0); dotmag = mpf(0)
        sev = mpf(0); sed = mpf(0)
        R.der = []
        for e in range(k):
            a, b, xx, kd = mpf(float(p0[e])), mpf(float(p1[e])), mpf(float(xv[e])), int(kind[e])
            v = d = None
            if kd == LIN:
                v, d = a * xx, a
            elif kd == QUAD:
                v, d = a * (xx - b) ** 2, 2 * a * (xx - b)
            elif kd == EXP:
                ex = mpmath.exp(b * xx)
                v, d = a * ex, b * a * ex
            else:
                s = xx + b
                if s > 0:
                    v = -a * mpmath.log(s)
                if s != 0:
                    d = -a / s
            if not _finite(val[e]):
                v = None
            if not _finite(der[e]):
                d = None
            R.der.append(d)
            if v is not None and g is not None:
                g += v; mag += abs(v); sev += mpf(float(ev[e]))
            else:
                g = None
            if d is not None and dot is not None:
                dot += xx * d; dotmag += abs(xx * d); sed += mpf(float(edot[e]))
            else:
                dot = None
        R.g = g if _finite(R.g_f64) else None
        assert R.g is not None or not _finite(R.g_f64), "a finite float64 g without an exact value: one non-finite source per row"
        R.dot = dot
        R.b = (R.g - dot) if (R.g is not None and dot is not None and _finite(R.b_f64)) else None
        assert R.b is not None or not _finite(R.b_f64), "a finite float64 cut constant without an exact value"
        R.mag, R.dotmag = mag, dotmag
        R.e_g = 2 * (sev + (D + 1) * mpf(U) * mag) if R.g is not None else None
        R.e_b = (R.e_g + 2 * (sed + (D + 1) * mpf(U) * dotmag) + 2 * mpf(U) * (mag + dotmag)) if R.b is not None else None
        R.e_der = [mpf(float(t)) if _finite(t) else None for t in ed]
    R.k = k
    return R


class RowsRef:
    """All rows of a CSR structure in float64 (arrays indexed by row; jac, e_der by entry).  A device value is within
    `slack` = 2 bounds of these (module docstring)."""
    slack = 2


def rows_ref_f64(rowptr, col, kind, p0, p1, rconst, x, depth=None):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    m = len(rowptr) - 1
    lens = np.diff(rowptr)
    rows = np.repeat(np.arange(m), lens)
    xv = np.asarray(x, dtype=np.float64)[np.asarray(col, dtype=np.int64)]
    val, der = atoms_f64(kind, p0, p1, xv)
    ev, ed, edot = atom_bounds(kind, p0, p1, xv, val, der)
    rconst = np.asarray(rconst, dtype=np.float64)
    R = RowsRef()
    with np.errstate(all="ignore"):
        bc = lambda w: np.bincount(rows, weights=w, minlength=m) if len(rows) else np.zeros(m)
        R.g = bc(val) + rconst
        R.dot = bc(xv * der)
        R.b = R.g - R.dot
        R.mag = bc(np.abs(val)) + np.abs(rconst)
        R.dotmag = bc(np.abs(xv * der))
        D = (lens if depth is None else np.asarray(depth)).astype(np.float64)
        R.e_g = 2 * (bc(ev) + (D + 1) * U * R.mag)
        R.e_b = R.e_g + 2 * (bc(edot) + (D + 1) * U * R.dotmag) + 2 * U * (R.mag + R.dotmag)
    R.val, R.jac, R.e_der, R.rows, R.lens = val, der, ed, rows, lens
    return R


def check_rows_f64(R, rows_sel, dev_g, dev_b=None, what=""):
    """bulk comparison of device g (and cut constants) with the float64 reference on the selected rows"""
    rows_sel = np.asarray(rows_sel, dtype=np.int64)
    for name, dev, ref, tol in (("g", dev_g, R.g, R.e_g), ("b", dev_b, R.b, R.e_b)):
        if dev is None:
            continue
        dv, rf, tl = np.asarray(dev)[rows_sel], ref[rows_sel], RowsRef.slack * tol[rows_sel]
        fin = np.isfinite(rf)
        with np.errstate(all="ignore"):
            bad = fin & ~(np.abs(dv - rf) <= tl)
        assert not bad.any(), (what, name, rows_sel[bad][:5], dv[bad][:5], rf[bad][:5], tl[bad][:5])
        nf = ~fin
        okc = (np.isnan(dv[nf]) & np.isnan(rf[nf])) | (dv[nf] == rf[nf])
        assert okc.all(), (what, name + " class", rows_sel[nf][~okc][:5], dv[nf][~okc][:5], rf[nf][~okc][:5])


def check_jac_f64(R, entry_sel, dev_jac, what=""):
    """bulk comparison of device partials (entries entry_sel of the structure) with the float64 reference"""
    dv, rf, tl = np.asarray(dev_jac), R.jac[entry_sel], RowsRef.slack * 2 * R.e_der[entry_sel]
    fin = np.isfinite(rf)
    with np.errstate(all="ignore"):
        bad = fin & ~(np.abs(dv - rf) <= tl)
    assert not bad.any(), (what, "partial", np.flatnonzero(bad)[:5], dv[bad][:5], rf[bad][:5], tl[bad][:5])
    nf = ~fin
    okc = (np.isnan(dv[nf]) & np.isnan(rf[nf])) | (dv[nf] == rf[nf])
    assert okc.all(), (what, "partial class", np.flatnonzero(nf)[~okc][:5])
