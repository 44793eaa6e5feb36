"""Reference of the NLP-level report (test code; include/katana_hip.h "Lagrange multipliers ...", csrc/kkt.hpp): from a point x
and constraint duals d the reduced costs z, the dual bound LB and the gap, in float64 numpy and in mpmath at 200 bits.

    z_j = grad f_j(x) - sum_i d_i J_ij(x)
    Min form (s = +1 for Min, -1 for Max; dm = s d, zm = s z, fm = s f):
        T  = sum_i [dm+_i (g_i - lb_i) - dm-_i (g_i - ub_i)] + sum_j [zm+_j (x_j - l_j) + zm-_j (u_j - x_j)]
        LB = s (fm - T),   gap = T                      (0 * inf counts as 0; an infinite term makes LB = -+inf)

Roundoff bounds, in the style of sep_ref.py (u = 2^-53, first order, doubled for the higher-order terms).  Column j has len_j
entries; its sum is taken in SOME order by len_j additions after len_j products and is subtracted from grad f_j: a term takes
part in at most D = len_j + 1 roundings of partial sums that are at most mag_j = |grad f_j| + sum_i |d_i J_ij| in absolute
value, and its own product rounds once:

    E_z_j  = 2 (sum_i |d_i| err(J_ij) + err(grad f_j) + (D + 1) u mag_j)

(the kernel's own chain -- ceil(len_j / G) per lane, log2 G butterfly levels, one subtraction -- is shorter for every G).  The
bound T adds m + n terms in some order; term_i = dm_i (g_i - b_i) has error |dm_i| (err(g_i) + u |g_i - b_i|) + u |term_i|,
term_j = zm_j (x_j - b_j) has error E_z_j w_j + u w_j |z_j| + u |term_j| with w_j = |x_j - b_j| -- or, where |z_j| <= E_z_j (the sign
of z_j, and with it the side, is within roundoff), the larger of the two sides' widths:

    E_LB = 2 (sum err(term) + (m + n + 2) u (sum |term| + |f|) + err(f))

A device value passes against the float64 evaluation within TWICE the bound, against the exact value within the bound.

`kkt_sep` / `kkt_sep_mp` take a SeparableInstance; `kkt_desc` takes ANY NLPDescription of device-evaluated rows and evaluates
every row in mpmath through the row kind's own reference -- sep_ref.row_ref_mp, tape_ref.evaluate, quad_ref.row_ref_mp --, whose
bounds of g_i and J_ij enter E_z and E_LB as err(.) above; `check_device` compares a device result with it.
"""
import math

import numpy as np
from mpmath import mp, mpf
import mpmath

import sep_ref

U = sep_ref.U
PREC = 200


class KktRef:
    """z, e_z [n]; LB, gap, e_LB; f, T (float64)"""


def _csr_rows(rowptr):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def kkt_from_jac(n, rowptr, col, jac, g, lb, ub, gradf, f, x, l, u, d, sense="Min", e_jac=None, e_g=None, e_gradf=None, e_f=0.0):
    """The report from materialised values: jac by entry of the CSR structure (rowptr, col) of the m constraint rows, g [m],
    gradf dense [n], f; e_*: the error bounds of those inputs (None: exact)."""
    s = -1.0 if sense == "Max" else 1.0
    col = np.asarray(col, dtype=np.int64)
    rows = _csr_rows(rowptr)
    m = len(rowptr) - 1
    jac, g, d = np.asarray(jac, dtype=np.float64), np.asarray(g, dtype=np.float64), np.asarray(d, dtype=np.float64)
    x, l, u = (np.asarray(a, dtype=np.float64)[:n] for a in (x, l, u))
    gradf = np.asarray(gradf, dtype=np.float64)
    e_jac = np.zeros(len(col)) if e_jac is None else np.asarray(e_jac)
    e_g = np.zeros(m) if e_g is None else np.asarray(e_g)
    e_gradf = np.zeros(n) if e_gradf is None else np.asarray(e_gradf)
    bc = lambda w: np.bincount(col, weights=w, minlength=n)[:n] if len(col) else np.zeros(n)
    R = KktRef()
    with np.errstate(all="ignore"):
        R.z = gradf - bc(d[rows] * jac)
        mag = np.abs(gradf) + bc(np.abs(d[rows] * jac))
        lens = bc(np.ones(len(col)))
        R.e_z = 2 * (bc(np.abs(d[rows]) * e_jac) + e_gradf + (lens + 2) * U * mag)
        dm, zm = s * d, s * R.z
        lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
        wr = np.where(dm > 0, g - lb, np.where(dm < 0, ub - g, 0.0))           # >= 0 at a feasible point
        tr = np.where(dm != 0, np.abs(dm) * wr, 0.0)
        er = np.where(dm != 0, np.abs(dm) * (e_g + U * np.abs(wr)) + U * np.abs(tr), 0.0)
        wl, wu = x - l, u - x
        wc = np.where(zm > 0, wl, np.where(zm < 0, wu, 0.0))
        tc = np.where(zm != 0, np.abs(zm) * wc, 0.0)
        amb = np.abs(R.z) <= R.e_z                                            # the side is within roundoff
        wmax = np.where(amb, np.maximum(np.abs(wl), np.abs(wu)), np.abs(wc))
        ec = R.e_z * wmax + U * wmax * np.abs(R.z) + U * np.abs(tc)
        T = float(np.sum(tr) + np.sum(tc))
        tot = float(np.sum(np.abs(tr)) + np.sum(np.abs(tc)))
        R.T, R.f = T, float(f)
        R.LB = s * (s * float(f) - T)
        R.gap = T
        R.e_LB = 2 * (float(np.sum(er) + np.sum(ec)) + (m + n + 2) * U * (tot + abs(float(f))) + float(e_f))
    return R


def _sep_objective(inst, x):
    """f, dense grad f and their error bounds for the separable objective of a SeparableInstance"""
    oc = np.asarray(inst.obj_col, dtype=np.int64)
    xv = np.asarray(x, dtype=np.float64)[oc]
    val, der = sep_ref.atoms_f64(inst.obj_kind, inst.obj_p0, inst.obj_p1, xv)
    ev, ed, _ = sep_ref.atom_bounds(inst.obj_kind, inst.obj_p0, inst.obj_p1, xv, val, der)
    n = inst.n
    gradf = np.bincount(oc, weights=der, minlength=n)
    e_gradf = np.bincount(oc, weights=ed, minlength=n) + U * np.bincount(oc, weights=np.abs(der), minlength=n)
    f = float(np.sum(val) + inst.obj_const)
    magf = float(np.sum(np.abs(val)) + abs(inst.obj_const))
    e_f = 2 * (float(np.sum(ev)) + (len(oc) + 2) * U * magf)
    return f, gradf, e_f, e_gradf


def kkt_sep(inst, x, d, sense=None):
    """the report of a SeparableInstance at (x, d) in float64, with the bounds of the module docstring"""
    x = np.asarray(x, dtype=np.float64)[:inst.n]
    RR = sep_ref.rows_ref_f64(inst.rowptr, inst.col, inst.kind, inst.p0, inst.p1, inst.rconst, x)
    f, gradf, e_f, e_gradf = _sep_objective(inst, x)
    return kkt_from_jac(inst.n, inst.rowptr, inst.col, RR.jac, RR.g, inst.l_constr, inst.u_constr, gradf, f, x, inst.l_var, inst.u_var, d,
                        sense=sense or inst.sense, e_jac=2 * RR.e_der, e_g=RR.e_g, e_gradf=e_gradf, e_f=e_f)


def _mp_atom(kind, a, b, xx):
    if kind == sep_ref.LIN:
        return a * xx, a
    if kind == sep_ref.QUAD:
        return a * (xx - b) ** 2, 2 * a * (xx - b)
    if kind == sep_ref.EXP:
        ex = mpmath.exp(b * xx)
        return a * ex, b * a * ex
    s = xx + b
    return -a * mpmath.log(s), -a / s


def kkt_sep_mp(inst, x, d, sense=None):
    """(z list, LB, gap) of a SeparableInstance at the float64 point (x, d), exact to 200 bits"""
    s = -1 if (sense or inst.sense) == "Max" else 1
    with mp.workprec(PREC):
        n, m = inst.n, inst.num_constr
        X = [mpf(float(v)) for v in np.asarray(x)[:n]]
        Dv = [mpf(float(v)) for v in d]
        z = [mpf(0)] * n
        f = mpf(float(inst.obj_const))
        for c, k, a, b in zip(inst.obj_col, inst.obj_kind, inst.obj_p0, inst.obj_p1):
            v, dv = _mp_atom(int(k), mpf(float(a)), mpf(float(b)), X[int(c)])
            f += v
            z[int(c)] += dv
        T = mpf(0)
        rp = inst.rowptr
        for i in range(m):
            gi = mpf(float(inst.rconst[i]))
            for e in range(int(rp[i]), int(rp[i + 1])):
                c = int(inst.col[e])
                v, dv = _mp_atom(int(inst.kind[e]), mpf(float(inst.p0[e])), mpf(float(inst.p1[e])), X[c])
                gi += v
                z[c] -= Dv[i] * dv
            dm = s * Dv[i]
            if dm > 0:
                T += dm * (gi - mpf(float(inst.l_constr[i])))
            elif dm < 0:
                T += -dm * (mpf(float(inst.u_constr[i])) - gi)
        for j in range(n):
            zm = s * z[j]
            if zm > 0:
                T += zm * (X[j] - mpf(float(inst.l_var[j])))
            elif zm < 0:
                T += -zm * (mpf(float(inst.u_var[j])) - X[j])
        return z, s * (s * f - T), T


def aggregate(y, slots, n_slots, newest_first=True):
    """the sum of y per slot, added in the order of k_row_duals: from the newest cut (the highest row) to the oldest, starting
    from 0.0 -- bit for bit what the device adds"""
    out = np.zeros(n_slots)
    order = range(len(y) - 1, -1, -1) if newest_first else range(len(y))
    for r in order:
        if slots[r] >= 0:
            out[int(slots[r])] = out[int(slots[r])] + y[r]
    return out


# ---- any NLPDescription of device-evaluated rows: SEP through sep_ref, TAPE through tape_ref, KTN_ROW_QUAD through quad_ref ----
ROW_SEP, ROW_TAPE, ROW_HOST, ROW_QUAD = 0, 1, 2, 3


def _row_exact(kind, cols, x, sep=None, tape=None, quad=None, rconst=0.0):
    """One row in mpmath: (g, bound of a device g, {column: (partial, bound of a device partial)}); the partials of a column that
    the row's structure names more than once are added, as J'd adds them"""
    import tape_ref
    import quad_ref
    J = {}

    def add(c, v, e):
        pv, pe = J.get(int(c), (mpf(0), mpf(0)))
        J[int(c)] = (pv + v, pe + e)
    if kind == ROW_SEP:
        ak, p0, p1 = sep
        R = sep_ref.row_ref_mp(cols, ak, p0, p1, rconst, x)
        for e, c in enumerate(cols):
            add(c, R.der[e], 2 * R.e_der[e])
        return R.g, R.e_g, J
    if kind == ROW_TAPE:
        ops, args = tape
        R = tape_ref.evaluate(ops, args, x, rconst=rconst)
        for c in cols:
            if int(c) not in J:
                J[int(c)] = (R.grad.get(int(c), mpf(0)), R.grad_tol(int(c)))
        return R.value, 2 * R.err + 4 * mpf(U) * abs(R.value), J
    if kind == ROW_QUAD:
        a, ptr, sc, sv = quad
        R = quad_ref.row_ref_mp(cols, a, np.asarray(ptr) - ptr[0], sc[ptr[0]:ptr[-1]], sv[ptr[0]:ptr[-1]], rconst, x)
        for e, c in enumerate(cols):
            add(c, R.der[e], R.e_der[e])
        return R.g, R.e_g, J
    raise ValueError("row kind %d has no description to evaluate" % kind)


def kkt_desc(d, l_constr, u_constr, l_var, u_var, sense, x, dv):
    """The report of an NLPDescription (katana_jl_amd.nlp) at the float64 point (x, dv), exact to 200 bits, with the bounds of a
    DEVICE result: R.z / R.e_z (lists of mpf), R.LB, R.gap, R.e_LB, R.f.  The bounds are those of the module docstring with the
    rows' own bounds (sep_ref, tape_ref, quad_ref) for err(g_i), err(J_ij), err(grad f_j), err(f)."""
    s = -1 if sense == "Max" else 1
    n, m = d.num_var, d.num_constr
    x = np.asarray(x, dtype=np.float64)[:n]
    with mp.workprec(PREC):
        u = mpf(U)

        def row(i):
            b, e = int(d.rowptr[i]), int(d.rowptr[i + 1])
            k = int(d.row_kind[i])
            cols = d.col[b:e]
            if k == ROW_SEP:
                return _row_exact(k, cols, x, sep=(d.atom_kind[b:e], d.p0[b:e], d.p1[b:e]), rconst=float(d.rconst[i]))
            if k == ROW_TAPE:
                tb, te = int(d.tape_ptr[i]), int(d.tape_ptr[i + 1])
                return _row_exact(k, cols, x, tape=(d.tape_op[tb:te], d.tape_arg[tb:te]), rconst=float(d.rconst[i]))
            return _row_exact(k, cols, x, quad=(d.p0[b:e], d.quad_ptr[b:e + 1], d.quad_col, d.quad_val), rconst=float(d.rconst[i]))

        if d.obj_kind == ROW_SEP:
            f, e_f, gf = _row_exact(ROW_SEP, d.obj_col, x, sep=(d.obj_atom_kind, d.obj_p0, d.obj_p1), rconst=d.obj_const)
        elif d.obj_kind == ROW_TAPE:
            cols = sorted({int(a) for o, a in zip(d.obj_tape_op, d.obj_tape_arg) if int(o) == 1})
            f, e_f, gf = _row_exact(ROW_TAPE, cols, x, tape=(d.obj_tape_op, d.obj_tape_arg), rconst=d.obj_const)
        else:
            f, e_f, gf = _row_exact(ROW_QUAD, d.obj_col, x, quad=(d.obj_p0, d.obj_quad_ptr, d.obj_quad_col, d.obj_quad_val), rconst=d.obj_const)
        e_f = e_f + 8 * u * abs(f)                                   # (the device forms f = (f - t) + t from the epigraph row)
        z = [gf.get(j, (mpf(0), mpf(0)))[0] for j in range(n)]
        ez = [gf.get(j, (mpf(0), mpf(0)))[1] for j in range(n)]
        mag = [abs(v) for v in z]
        lens = [0] * n
        T = mpf(0); tot = mpf(0); err = mpf(0)
        for i in range(m):
            g, e_g, J = row(i)
            di = mpf(float(dv[i]))
            for c, (v, e) in J.items():
                z[c] -= di * v; ez[c] += abs(di) * e; mag[c] += abs(di * v); lens[c] += 1
            dm = s * di
            if dm != 0:
                w = (g - mpf(float(l_constr[i]))) if dm > 0 else (mpf(float(u_constr[i])) - g)
                t = abs(dm) * w
                T += t; tot += abs(t); err += abs(dm) * (e_g + u * abs(w)) + u * abs(t)
        e_z = [ez[j] + 2 * (lens[j] + 2) * u * mag[j] for j in range(n)]
        for j in range(n):
            zm = s * z[j]
            wl, wu = mpf(float(x[j])) - mpf(float(l_var[j])), mpf(float(u_var[j])) - mpf(float(x[j]))
            w = wl if zm > 0 else (wu if zm < 0 else mpf(0))
            t = abs(zm) * w
            T += t; tot += abs(t)
            wmax = max(abs(wl), abs(wu)) if abs(z[j]) <= e_z[j] else abs(w)
            err += e_z[j] * wmax + u * wmax * abs(z[j]) + u * abs(t)
        R = KktRef()
        R.z, R.e_z, R.f, R.T = z, e_z, f, T
        R.LB, R.gap = s * (s * f - T), T
        R.e_LB = 2 * (err + (m + n + 2) * u * (tot + abs(f))) + e_f
    return R


def check_device(R, z, lb, gap, what=""):
    """device z, bound and gap against the exact report within its bounds (no slack: only the device's own error enters)"""
    with mp.workprec(PREC):
        for j in range(len(R.z)):
            assert abs(mpf(float(z[j])) - R.z[j]) <= R.e_z[j], (what, "z", j, float(z[j]), float(R.z[j]), float(R.e_z[j]))
        assert abs(mpf(float(lb)) - R.LB) <= R.e_LB, (what, "bound", lb, float(R.LB), float(R.e_LB))
        assert abs(mpf(float(gap)) - R.gap) <= R.e_LB, (what, "gap", gap, float(R.gap), float(R.e_LB))
