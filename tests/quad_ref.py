"""High-precision reference for KTN_ROW_QUAD rows (test code).

A row is `(cols, a, seg_ptr, seg_col, seg_val, rconst)` in the layout of nlp._quad_row / include/katana_hip.h:

    s_e = sum_{k in seg(e)} q_k x[seg_col_k]          J_e = a_e + s_e
    g   = rconst + sum_e x_e (a_e + 1/2 s_e)          b   = g - sum_e x_e J_e        (src/algorithms.jl:3-18)

`row_ref_mp` evaluates these formulas as they stand in mpmath at 200 bits -- for ANY segments: J_e is the derivative of g only when
the segments are those of a symmetric Q, which is the caller's contract and not the kernels' business.

Error bounds (u = 2^-53, h = 2^-1074; + - * correctly rounded, a fused multiply-add only removes a rounding; first-order forward
errors, doubled for the higher-order terms, derived as in tests/sep_ref.py).  smag_e = sum_k |q_k x_k|, L_e the segment length:

* s_e: L products, one rounding each (u smag), summed in ANY order by L additions -- (L + 1) u smag as for a sum of L terms:
      E_s = 2 (L + 2) u smag                                    (an empty segment: s = 0 exactly)
* J_e = fl(a + s): one more rounding:   E_J = E_s + 2u |J_e|
* the value term t_e = fl(x fl(a + 1/2 s)); 1/2 s is exact:  err(a + 1/2 s) <= 1/2 E_s + u |a + 1/2 s|, the product one more:
      E_t = |x| (1/2 E_s + 2u |a + 1/2 s|) + 2u |t_e| + h
* g = (sum of k terms) + rconst in any order:   E_g = sum_e E_t + 2 (k + 1) u mag,   mag = sum |t_e| + |rconst|
* dot = sum x_e J_e:   E_dot = sum_e (|x| E_J + 2u |x J_e| + h) + 2 (k + 1) u dotmag,   dotmag = sum |x_e J_e|
* b = fl(g - dot):   E_b = E_g + E_dot + 2u (mag + dotmag)
* a cut's row bounds lo = fl(lb - b), hi = fl(ub - b):   E_b + 2u |bound - b|          (src/model.jl:74-75)
"""
import numpy as np
from mpmath import mp, mpf

U = 2.0 ** -53
H = 2.0 ** -1074
PREC = 200
F_TOL = 2.0 ** -20          # dyadic, so that threshold rows are exact


class QuadRowRef:
    """exact (mpf) s, der (J_e), g, b and the bounds e_s, e_der (per entry), e_g, e_b of one row at one x"""

    def check_g(self, dev, what=""):
        _check(dev, self.g, self.e_g, ("g", what))

    def check_b(self, dev, what=""):
        _check(dev, self.b, self.e_b, ("cut constant", what))

    def check_der(self, dev, what=""):
        assert len(dev) == len(self.der), ("row length", what, len(dev), len(self.der))
        for e, dv in enumerate(dev):
            _check(dv, self.der[e], self.e_der[e], ("partial", what, e))

    def bound_tol(self, bnd):
        """tolerance of a cut's row bound fl(bnd - b) for a finite constraint bound bnd"""
        with mp.workprec(PREC):
            return self.e_b + 2 * mpf(U) * abs(mpf(bnd) - self.b)


def _check(dev, exact, bound, what):
    dev = float(dev)
    with mp.workprec(PREC):
        ok = dev == dev and abs(dev) != np.inf and abs(mpf(dev) - exact) <= bound
        assert ok, what + (dev, float(exact), float(abs(mpf(dev) - exact)) if dev == dev else dev, float(bound))


def row_ref_mp(cols, a, seg_ptr, seg_col, seg_val, rconst, x):
    cols = np.asarray(cols, dtype=np.int64)
    x = np.asarray(x, dtype=np.float64)
    k = len(cols)
    R = QuadRowRef()
    with mp.workprec(PREC):
        u, h = mpf(U), mpf(H)
        g = mpf(float(rconst)); mag = abs(g); dot = mpf(0); dotmag = mpf(0); set_ = mpf(0); sed = mpf(0)
        R.s, R.der, R.e_s, R.e_der = [], [], [], []
        for e in range(k):
            s = mpf(0); smag = mpf(0)
            L = int(seg_ptr[e + 1] - seg_ptr[e])
            for q in range(int(seg_ptr[e]), int(seg_ptr[e + 1])):
                t = mpf(float(seg_val[q])) * mpf(float(x[int(seg_col[q])]))
                s += t; smag += abs(t)
            ae, xe = mpf(float(a[e])), mpf(float(x[cols[e]]))
            e_s = 2 * (L + 2) * u * smag if L else mpf(0)
            J = ae + s
            e_J = e_s + 2 * u * abs(J)
            half = ae + s / 2
            t = xe * half
            e_t = abs(xe) * (e_s / 2 + 2 * u * abs(half)) + 2 * u * abs(t) + h
            g += t; mag += abs(t); set_ += e_t
            dot += xe * J; dotmag += abs(xe * J); sed += abs(xe) * e_J + 2 * u * abs(xe * J) + h
            R.s.append(s); R.der.append(J); R.e_s.append(e_s); R.e_der.append(e_J)
        R.g, R.dot, R.b = g, dot, g - dot
        R.mag, R.dotmag = mag, dotmag
        R.e_g = set_ + 2 * (k + 1) * u * mag
        R.e_b = R.e_g + sed + 2 * (k + 1) * u * dotmag + 2 * u * (mag + dotmag)
    R.k = k
    return R


def dense_forms(n, lin_cols, lin_vals, q_rows, q_cols, q_vals):
    """(a, T): the dense linear vector and the dense matrix the triplets SUM to (no convention applied)"""
    a = np.zeros(n); T = np.zeros((n, n))
    np.add.at(a, np.asarray(lin_cols, dtype=np.int64), np.asarray(lin_vals, dtype=np.float64))
    np.add.at(T, (np.asarray(q_rows, dtype=np.int64), np.asarray(q_cols, dtype=np.int64)), np.asarray(q_vals, dtype=np.float64))
    return a, T
