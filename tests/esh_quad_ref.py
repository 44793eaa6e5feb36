"""High-precision reference for the supporting-hyperplane cut of a KTN_ROW_QUAD row (test code; csrc/esh_quad.hpp).

A row is `(cols, a, seg_ptr, seg_col, seg_val, rconst)` in quad_ref's layout, with the segments of a SYMMETRIC Q.  For an interior
point x_int, an LP point x*, a side sigma, the row's bound and a REPORTED lambda (a float64), `cut_ref_mp` gives in mpmath at
quad_ref.PREC, with d = x* - x_int and x_b = x_int + lambda d formed exactly (never rounded):

    phi(lambda) = sigma (g(x_b) - bound)        grad g(x_b)_e = a_e + s_e(x_b)        b = g(x_b) - grad g(x_b) . x_b

`root_mp` gives the lambda with phi = tau / 2 (the kernel's target) from the exact P1 = grad g(x*) . d and q = d'Qd.

Error bounds of what the device computes (u = 2^-53, h = 2^-1074; + - * / sqrt correctly rounded, fma one rounding, the library is
built with -ffp-contract=off; first-order forward errors, doubled for the higher-order terms, as in tests/quad_ref.py).  E*_e, E0_e
are quad_ref.row_ref_mp's e_der at x* and at x_int, Eg* its e_g at x*: the kernel reads those Jacobians and that g as k_quad_jac /
k_quad_stats left them.  mu = 1 - lambda, k the row length:

* d_e = fl(x* - x_int): u |d_e|
* J_b,e = fma(lambda, fl(J*_e - J0_e), J0_e) = lambda J* + (1 - lambda) J0 + lambda delta (J* - J0), rounded once:
      E_Jb = lambda E* + mu E0 + 2u (lambda |J* - J0| + |J_b|) + h
* P1 = sum_e J*_e d_e, a product of two inexact factors each, then k terms summed in any order (P0 likewise with J0, E0):
      E_P1 = sum_e (|d_e| E*_e + 4u |J*_e d_e| + h) + 2 (k + 1) u sum_e |J*_e d_e|
* q = fl(P1 - P0):   E_q = E_P1 + E_P0 + 2u (|P1| + |P0|)
* c = fl(fl(sigma (g* - bound)) - tau / 2):   E_c = Eg* + 2u |g* - bound| + 2u |c|
* the root.  phi'(mu) at the root is -D, D = sqrt(disc) = sigma P1 - mu sigma q, so a perturbation of the coefficients moves the
  root by (E_c + mu E_P1 + 1/2 mu^2 E_q) / D.  The formula itself: disc = fl(fl(sp1^2) - fl(fl(2 sq) c)) with error at most
  3u (sp1^2 + 2 |sq c|), its root err(disc) / (2 D) + u D, the denominator S = sp1 + D one more rounding, the quotient and the
  product 2 c two more, lambda = fl(1 - mu) a last one:
      E_lam = 2 [ (E_c + mu E_P1 + 1/2 mu^2 E_q) / D + mu ((3u (sp1^2 + 2 |sq c|) / (2 D) + u D + u S) / S + 2u) + u ]
  and phi moves with lambda by at most |P1| + |q| on the segment:   E_phi = E_lam (|P1| + |q|)
* g_b = fl(fl(g* - fl(m P1)) + fl(fl(1/2 fl(m m)) q)), m = fl(1 - lambda) (u |mu|), T1 = mu P1, T2 = 1/2 mu^2 q:
      E_gb = Eg* + mu E_P1 + 1/2 mu^2 E_q + 4u |T1| + 8u |T2| + 4u (|g*| + |T1| + |T2|) + h
* x_b,e = fl(x_int + fl(lambda d_e)):   E_xb = 4u |lambda d_e| + 2u |x_b,e| + h
* dot = sum_e x_b,e J_b,e:   E_dot = sum_e (|x_b| E_Jb + |J_b| E_xb + 2u |x_b J_b| + h) + 2 (k + 1) u sum_e |x_b J_b|
* b = fl(g_b - dot):   E_b = E_gb + E_dot + 2u (|g_b| + sum_e |x_b J_b|)
* a cut's row bound fl(bound - b):   E_b + 2u |bound - b|          (src/model.jl:74-75)
"""
import numpy as np
from mpmath import mp, mpf, sqrt as mpsqrt

import quad_ref as Q

U, H, PREC = Q.U, Q.H, Q.PREC


class QuadCutRef:
    """exact (mpf) phi, xb, der (grad g(x_b) per entry), g, b, P1, q, and the bounds e_der (per entry), e_g, e_b, e_lam, e_phi"""

    def bound_tol(self, bnd):
        with mp.workprec(PREC):
            return self.e_b + 2 * mpf(U) * abs(mpf(bnd) - self.b)

    def bounds(self):
        """every error bound of this row, as floats"""
        return [float(v) for v in self.e_der] + [float(self.e_g), float(self.e_b), float(self.e_lam), float(self.e_phi)]


def _seg_sums(layout, xv):
    """s_e = sum_k q_k x[seg_col_k] for mpf values xv by column"""
    cols, a, ptr, sc, sv = layout[:5]
    return [sum((mpf(float(sv[k])) * xv[int(sc[k])] for k in range(int(ptr[e]), int(ptr[e + 1]))), mpf(0)) for e in range(len(cols))]


def cut_ref_mp(layout, rconst, x_int, x_star, sigma, bound, lam, tau):
    cols, a, ptr, sc, sv = layout[:5]
    cols = np.asarray(cols, dtype=np.int64)
    k = len(cols)
    R0 = Q.row_ref_mp(cols, a, ptr, sc, sv, rconst, x_int)
    R1 = Q.row_ref_mp(cols, a, ptr, sc, sv, rconst, x_star)
    R = QuadCutRef()
    with mp.workprec(PREC):
        u, h, lm = mpf(U), mpf(H), mpf(float(lam))
        mu = 1 - lm
        touched = set(int(c) for c in cols) | set(int(c) for c in sc)
        xi = {c: mpf(float(x_int[c])) for c in touched}
        d = {c: mpf(float(x_star[c])) - xi[c] for c in touched}
        xb = {c: xi[c] + lm * d[c] for c in touched}
        s = _seg_sums(layout, xb)
        R.xb = [xb[int(c)] for c in cols]
        R.der = [mpf(float(a[e])) + s[e] for e in range(k)]
        R.g = mpf(float(rconst)) + sum((R.xb[e] * (mpf(float(a[e])) + s[e] / 2) for e in range(k)), mpf(0))
        dotmag = sum((abs(R.xb[e] * R.der[e]) for e in range(k)), mpf(0))
        R.b = R.g - sum((R.xb[e] * R.der[e] for e in range(k)), mpf(0))
        R.phi = sigma * (R.g - mpf(float(bound)))
        de = [d[int(c)] for c in cols]
        R.P1 = sum((R1.der[e] * de[e] for e in range(k)), mpf(0))
        R.P0 = sum((R0.der[e] * de[e] for e in range(k)), mpf(0))
        R.q = R.P1 - R.P0
        m1 = sum((abs(R1.der[e] * de[e]) for e in range(k)), mpf(0))
        m0 = sum((abs(R0.der[e] * de[e]) for e in range(k)), mpf(0))
        e_p1 = sum((abs(de[e]) * R1.e_der[e] + 4 * u * abs(R1.der[e] * de[e]) + h for e in range(k)), mpf(0)) + 2 * (k + 1) * u * m1
        e_p0 = sum((abs(de[e]) * R0.e_der[e] + 4 * u * abs(R0.der[e] * de[e]) + h for e in range(k)), mpf(0)) + 2 * (k + 1) * u * m0
        e_q = e_p1 + e_p0 + 2 * u * (abs(R.P1) + abs(R.P0))
        R.e_p1, R.e_q = e_p1, e_q
        R.e_der = [lm * R1.e_der[e] + mu * R0.e_der[e] + 2 * u * (lm * abs(R1.der[e] - R0.der[e]) + abs(R.der[e])) + h for e in range(k)]
        # the root's sensitivity, at the exact coefficients
        c = sigma * (R1.g - mpf(float(bound))) - mpf(float(tau)) / 2
        sp1, sq = sigma * R.P1, sigma * R.q
        disc = sp1 * sp1 - 2 * sq * c
        R.c, R.disc = c, disc
        if disc > 0 and sp1 > 0:
            D = mpsqrt(disc)
            S = sp1 + D
            e_c = R1.e_g + 2 * u * abs(R1.g - mpf(float(bound))) + 2 * u * abs(c)
            mur = 2 * c / S
            R.e_lam = 2 * ((e_c + abs(mur) * e_p1 + mur * mur * e_q / 2) / D +
                           abs(mur) * ((3 * u * (sp1 * sp1 + 2 * abs(sq * c)) / (2 * D) + u * D + u * S) / S + 2 * u) + u)
            R.e_phi = R.e_lam * (abs(R.P1) + abs(R.q))
            R.lam_root = 1 - mur
        else:
            R.e_lam = R.e_phi = mpf("inf")
            R.lam_root = None
        t1, t2 = mu * R.P1, mu * mu * R.q / 2
        R.e_g = R1.e_g + abs(mu) * e_p1 + mu * mu * e_q / 2 + 4 * u * abs(t1) + 8 * u * abs(t2) + 4 * u * (abs(R1.g) + abs(t1) + abs(t2)) + h
        e_dot = mpf(0)
        for e in range(k):
            e_xb = 4 * u * abs(lm * de[e]) + 2 * u * abs(R.xb[e]) + h
            e_dot += abs(R.xb[e]) * R.e_der[e] + abs(R.der[e]) * e_xb + 2 * u * abs(R.xb[e] * R.der[e]) + h
        e_dot += 2 * (k + 1) * u * dotmag
        R.e_b = R.e_g + e_dot + 2 * u * (abs(R.g) + dotmag)
    R.k = k
    return R


def closed_form_f64(layout, rconst, x_int, x_star, sigma, bound, tau):
    """the kernel's formulas in float64 numpy (Jacobians and g from numpy, in its own summation order): lambda, or None when the
    row would keep Kelley's cut"""
    cols, a, ptr, sc, sv = layout[:5]
    cols = np.asarray(cols, dtype=np.int64)
    a, sc, sv = np.asarray(a, dtype=np.float64), np.asarray(sc, dtype=np.int64), np.asarray(sv, dtype=np.float64)

    def jac_g(x):
        s = np.array([np.sum(sv[ptr[e]:ptr[e + 1]] * x[sc[ptr[e]:ptr[e + 1]]]) for e in range(len(cols))])
        return a + s, float(rconst + np.sum(x[cols] * (a + 0.5 * s)))
    js, gs = jac_g(np.asarray(x_star, dtype=np.float64))
    j0, _ = jac_g(np.asarray(x_int, dtype=np.float64))
    d = np.asarray(x_star, dtype=np.float64)[cols] - np.asarray(x_int, dtype=np.float64)[cols]
    p1, p0 = float(np.sum(js * d)), float(np.sum(j0 * d))
    q = p1 - p0
    c = sigma * (gs - bound) - 0.5 * tau
    sp1, sq = sigma * p1, sigma * q
    disc = sp1 * sp1 - 2.0 * sq * c
    if not (np.isfinite([p1, p0, gs, c, disc]).all() and sq >= 0.0 and sp1 > 0.0 and disc >= 0.0 and c > 0.0):
        return None
    lam = 1.0 - 2.0 * c / (sp1 + np.sqrt(disc))
    return lam if 0.0 < lam < 1.0 else None
