"""Device-evaluable NLP descriptions: what `d::AbstractNLPEvaluator` is to the reference's
loadproblem! (src/model.jl:86).  An NLPDescription owns the numpy arrays behind a
`ktn_nlp_desc` (include/katana_hip.h) and answers the structural queries the reference asks
its evaluator (jac_structure, isconstrlinear, isobjlinear); values and derivatives are
computed on the device only."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib as L
from .expr import Expr


# the arguments of loadproblem! (src/model.jl:81-86): NonlinearModel.loadproblem(*problem)
Problem = namedtuple("Problem", "num_var num_constr l_var u_var l_constr u_constr sense d")


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype)) if a is not None and a.size else C.POINTER(ctype)()


class NLPDescription:
    def __init__(self, num_var, rowptr, col, row_kind, row_linear, rconst, atom_kind, p0, p1,
                 tape_ptr=None, tape_op=None, tape_arg=None,
                 obj_linear=True, obj_kind=L.ROW_SEP, obj_col=None, obj_atom_kind=None, obj_p0=None, obj_p1=None,
                 obj_const=0.0, obj_tape_op=None, obj_tape_arg=None,
                 quad_ptr=None, quad_col=None, quad_val=None, obj_quad_ptr=None, obj_quad_col=None, obj_quad_val=None):
        i64, i32, u8, f64 = np.int64, np.int32, np.uint8, np.float64
        self.num_var = int(num_var)
        self.rowptr = np.ascontiguousarray(rowptr, dtype=i64)
        self.num_constr = len(self.rowptr) - 1
        self.col = np.ascontiguousarray(col, dtype=i32)
        nnz = len(self.col)
        self.row_kind = np.ascontiguousarray(row_kind, dtype=u8)
        self.row_linear = np.ascontiguousarray(row_linear, dtype=u8)
        self.rconst = np.ascontiguousarray(rconst, dtype=f64)
        self.atom_kind = np.ascontiguousarray(atom_kind if atom_kind is not None else np.zeros(nnz), dtype=u8)
        self.p0 = np.ascontiguousarray(p0 if p0 is not None else np.zeros(nnz), dtype=f64)
        self.p1 = np.ascontiguousarray(p1 if p1 is not None else np.zeros(nnz), dtype=f64)
        self.tape_ptr = np.ascontiguousarray(tape_ptr if tape_ptr is not None else np.zeros(self.num_constr + 1), dtype=i64)
        self.tape_op = np.ascontiguousarray(tape_op if tape_op is not None else [], dtype=i32)
        self.tape_arg = np.ascontiguousarray(tape_arg if tape_arg is not None else [], dtype=f64)
        self.obj_linear = bool(obj_linear)
        self.obj_kind = int(obj_kind)
        self.obj_col = np.ascontiguousarray(obj_col if obj_col is not None else [], dtype=i32)
        k = len(self.obj_col)
        self.obj_atom_kind = np.ascontiguousarray(obj_atom_kind if obj_atom_kind is not None else np.zeros(k), dtype=u8)
        self.obj_p0 = np.ascontiguousarray(obj_p0 if obj_p0 is not None else np.zeros(k), dtype=f64)
        self.obj_p1 = np.ascontiguousarray(obj_p1 if obj_p1 is not None else np.zeros(k), dtype=f64)
        self.obj_const = float(obj_const)
        self.obj_tape_op = np.ascontiguousarray(obj_tape_op if obj_tape_op is not None else [], dtype=i32)
        self.obj_tape_arg = np.ascontiguousarray(obj_tape_arg if obj_tape_arg is not None else [], dtype=f64)
        # KTN_ROW_QUAD rows: Q segments per Jacobian entry (None: no such rows) and per objective entry
        opt = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)
        self.quad_ptr, self.quad_col, self.quad_val = opt(quad_ptr, i64), opt(quad_col, i32), opt(quad_val, f64)
        self.obj_quad_ptr, self.obj_quad_col, self.obj_quad_val = opt(obj_quad_ptr, i64), opt(obj_quad_col, i32), opt(obj_quad_val, f64)
        assert self.quad_ptr is None or len(self.quad_ptr) == nnz + 1
        assert self.obj_quad_ptr is None or len(self.obj_quad_ptr) == k + 1
        assert len(self.row_kind) == self.num_constr and len(self.row_linear) == self.num_constr
        assert len(self.rconst) == self.num_constr and len(self.p0) == nnz and len(self.p1) == nnz

    # ---- the structural part of the MathProgBase evaluator interface --------------------
    def isobjlinear(self):
        return self.obj_linear

    def isconstrlinear(self, i):
        return bool(self.row_linear[i])

    def jac_structure(self):
        rows = np.repeat(np.arange(self.num_constr), np.diff(self.rowptr))
        return rows, self.col

    def features_available(self):
        return ["Grad", "Jac"]

    def c_struct(self):
        d = L.KtnNlpDesc()
        d.num_var, d.num_constr = self.num_var, self.num_constr
        d.rowptr, d.col = _ptr(self.rowptr, C.c_int64), _ptr(self.col, C.c_int32)
        d.row_kind, d.row_linear = _ptr(self.row_kind, C.c_uint8), _ptr(self.row_linear, C.c_uint8)
        d.rconst, d.atom_kind = _ptr(self.rconst, C.c_double), _ptr(self.atom_kind, C.c_uint8)
        d.p0, d.p1 = _ptr(self.p0, C.c_double), _ptr(self.p1, C.c_double)
        d.tape_ptr, d.tape_op, d.tape_arg = (_ptr(self.tape_ptr, C.c_int64), _ptr(self.tape_op, C.c_int32),
                                             _ptr(self.tape_arg, C.c_double))
        d.obj_linear, d.obj_kind, d.obj_nnz = int(self.obj_linear), self.obj_kind, len(self.obj_col)
        d.obj_col, d.obj_atom_kind = _ptr(self.obj_col, C.c_int32), _ptr(self.obj_atom_kind, C.c_uint8)
        d.obj_p0, d.obj_p1, d.obj_const = _ptr(self.obj_p0, C.c_double), _ptr(self.obj_p1, C.c_double), self.obj_const
        d.obj_tape_len = len(self.obj_tape_op)
        d.obj_tape_op, d.obj_tape_arg = _ptr(self.obj_tape_op, C.c_int32), _ptr(self.obj_tape_arg, C.c_double)
        d.quad_ptr, d.quad_col, d.quad_val = _ptr(self.quad_ptr, C.c_int64), _ptr(self.quad_col, C.c_int32), _ptr(self.quad_val, C.c_double)
        d.obj_quad_ptr, d.obj_quad_col, d.obj_quad_val = (_ptr(self.obj_quad_ptr, C.c_int64), _ptr(self.obj_quad_col, C.c_int32),
                                                          _ptr(self.obj_quad_val, C.c_double))
        return d


def SeparableNLP(inst):
    """NLPDescription of a katana_jl_amd.instances.SeparableInstance (or any object with the
    same array attributes)."""
    m = len(inst.rowptr) - 1
    rp = np.asarray(inst.rowptr)
    kind = np.ascontiguousarray(inst.kind, dtype=np.uint8)                       # a row is nonlinear iff one of its atoms is (LIN = 0)
    nonlin = np.zeros(m, dtype=np.uint8)
    nz = np.flatnonzero(np.diff(rp) > 0)                                         # reduce over the non-empty rows only: reduceat
    if len(nz):                                                                  # runs a slice up to the NEXT start, so an empty
        nonlin[nz] = np.maximum.reduceat(kind, rp[:-1][nz])                      # row in between (or at the end) must not be a start
    return NLPDescription(
        inst.n, inst.rowptr, inst.col, np.zeros(m, dtype=np.uint8), (nonlin == 0).astype(np.uint8), inst.rconst,
        inst.kind, inst.p0, inst.p1,
        obj_linear=bool(np.all(np.asarray(inst.obj_kind) == L.ATOM_LIN)), obj_kind=L.ROW_SEP,
        obj_col=inst.obj_col, obj_atom_kind=inst.obj_kind, obj_p0=inst.obj_p0, obj_p1=inst.obj_p1,
        obj_const=inst.obj_const)


def ExprNLP(num_var, objective, constraints, constr_linear=None, obj_linear=None):
    """NLPDescription from expressions.  Affine rows become separable rows of LIN atoms (their
    tangent at the origin is the row itself, src/model.jl:115-118); every other row becomes a
    tape row."""
    rowptr, col, akind, p0, p1, rkind, rlin, rconst = [0], [], [], [], [], [], [], []
    tptr, top, targ = [0], [], []
    for i, e in enumerate(constraints):
        e = Expr.wrap(e)
        aff = e.affine()
        declared = constr_linear[i] if constr_linear is not None else (aff is not None)
        if aff is not None:
            co, c0 = aff
            for j in sorted(co):
                col.append(j); akind.append(L.ATOM_LIN); p0.append(co[j]); p1.append(0.0)
            rkind.append(L.ROW_SEP); rconst.append(c0)
        else:
            for j in e.variables():
                col.append(j); akind.append(0); p0.append(0.0); p1.append(0.0)
            o, a = e.tape()
            top.extend(o.tolist()); targ.extend(a.tolist())
            rkind.append(L.ROW_TAPE); rconst.append(0.0)
        rlin.append(1 if declared else 0)
        rowptr.append(len(col)); tptr.append(len(top))
    objective = Expr.wrap(objective)
    oaff = objective.affine()
    is_lin = obj_linear if obj_linear is not None else (oaff is not None)
    kw = {}
    if oaff is not None:
        co, c0 = oaff
        js = sorted(co)
        kw = dict(obj_kind=L.ROW_SEP, obj_col=js, obj_atom_kind=np.zeros(len(js)), obj_p0=[co[j] for j in js],
                  obj_p1=np.zeros(len(js)), obj_const=c0)
    else:
        o, a = objective.tape()
        kw = dict(obj_kind=L.ROW_TAPE, obj_tape_op=o, obj_tape_arg=a)
    return NLPDescription(num_var, rowptr, col, rkind, rlin, rconst, akind, p0, p1, tptr, top, targ,
                          obj_linear=is_lin, **kw)


def _quad_row(num_var, lin_cols, lin_vals, q_rows, q_cols, q_vals):
    """One quadratic form  a'x + 1/2 x'Qx  in the engine's layout: (cols, a, seg_ptr, seg_col, seg_val).  cols is the sorted union
    of the columns of the linear part and of Q; a the linear coefficients on it (duplicates summed); entry e's segment
    [seg_ptr[e], seg_ptr[e+1]) is row cols[e] of Q sorted by column (duplicate triplets summed, in the order given).  Q arrives
    as SYMMETRIC triplets -- both (r, c) and (c, r) -- which is the caller's contract (include/katana_hip.h) and is not checked."""
    i64, f64 = np.int64, np.float64
    lc, lv = np.asarray(lin_cols, dtype=i64).reshape(-1), np.asarray(lin_vals, dtype=f64).reshape(-1)
    qr, qc, qv = (np.asarray(q_rows, dtype=i64).reshape(-1), np.asarray(q_cols, dtype=i64).reshape(-1),
                  np.asarray(q_vals, dtype=f64).reshape(-1))
    if len(lc) != len(lv) or not (len(qr) == len(qc) == len(qv)):
        raise ValueError("QuadNLP: index and value arrays of one row differ in length")
    every = np.concatenate([lc, qr, qc])
    if len(every) and (every.min() < 0 or every.max() >= num_var):
        raise ValueError("QuadNLP: column index out of range")
    cols = np.unique(every)
    a = np.zeros(len(cols))
    np.add.at(a, np.searchsorted(cols, lc), lv)
    key, inv = np.unique(qr * np.int64(max(num_var, 1)) + qc, return_inverse=True)
    val = np.zeros(len(key))
    np.add.at(val, inv.reshape(-1), qv)
    r, c = key // max(num_var, 1), key % max(num_var, 1)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(np.searchsorted(cols, r), minlength=len(cols)))]).astype(i64)
    return cols.astype(np.int32), a, ptr, c.astype(np.int32), val


def QuadNLP(num_var, obj_c, obj_c0, obj_Q, rows):
    """NLPDescription of a linear / quadratic program in KTN_ROW_QUAD rows (include/katana_hip.h), declared by the caller:

        objective   obj_c'x + obj_c0 + 1/2 x'Qx        obj_c: dense [num_var] or (cols, vals); obj_Q: (q_rows, q_cols, q_vals) or None
        rows[i]     (lin_cols, lin_vals, q_rows, q_cols, q_vals, const):   lin'x + const + 1/2 x'Q_i x

    in the ENGINE's convention: Q as symmetric triplets stored in full, duplicates summed (solver.quad_triplets_to_engine converts
    MathProgBase's two conventions).  Builds the sorted union structure per row, the full segments and row_linear (1 where a
    row's Q is empty; obj_linear likewise)."""
    if isinstance(obj_c, tuple):
        oc, ov = obj_c
    else:
        ov = np.asarray(obj_c, dtype=np.float64).reshape(-1)
        if len(ov) != num_var:
            raise ValueError("QuadNLP: obj_c must have num_var entries (or be a (cols, vals) pair)")
        oc = np.flatnonzero(ov)
        ov = ov[oc]
    oq = obj_Q if obj_Q is not None else ([], [], [])
    ocols, oa, optr, oqc, oqv = _quad_row(num_var, oc, ov, *oq)
    rowptr, col, p0, rconst, rlin, qptr, qcol, qval = [0], [], [], [], [], [np.zeros(1, dtype=np.int64)], [], []
    nq = 0
    for row in rows:
        lc, lv, qr, qc, qv, c0 = row
        cols, a, ptr, sc, sv = _quad_row(num_var, lc, lv, qr, qc, qv)
        col.append(cols); p0.append(a); rconst.append(float(c0)); rlin.append(1 if len(sv) == 0 else 0)
        rowptr.append(rowptr[-1] + len(cols))
        qptr.append(ptr[1:] + nq); qcol.append(sc); qval.append(sv)
        nq += len(sv)
    cat = lambda parts, t: np.concatenate(parts).astype(t) if parts else np.zeros(0, dtype=t)
    m = len(rlin)
    col = cat(col, np.int32)
    return NLPDescription(
        num_var, rowptr, col, np.full(m, L.ROW_QUAD, dtype=np.uint8), rlin, rconst, None, cat(p0, np.float64), None,
        obj_linear=len(oqv) == 0, obj_kind=L.ROW_QUAD, obj_col=ocols, obj_p0=oa, obj_const=float(obj_c0),
        quad_ptr=np.concatenate(qptr), quad_col=cat(qcol, np.int32), quad_val=cat(qval, np.float64),
        obj_quad_ptr=optr, obj_quad_col=oqc, obj_quad_val=oqv)


class CallbackNLP(NLPDescription):
    """The fallback for evaluators that cannot hand over expressions (SURVEY.md section 8b "Evaluator consumed"): wraps an
    object with the MathProgBase.AbstractNLPEvaluator methods the reference calls -- `jac_structure()`,
    `eval_g(g, x)`, `eval_jac_g(J, x)`, `eval_f(x)`, `eval_grad_f(grad, x)`, `isconstrlinear(i)`, `isobjlinear()`
    (src/separators.jl:88-113, src/model.jl:116,125,159, src/nlpeval.jl:31-63) -- and declares every row KTN_ROW_HOST.
    Values and derivatives are then computed by that object on the host, once per sweep; constraint checks, cuts and the
    LP stay on the device.  The COO structure is converted to CSR exactly as initialize! does (src/separators.jl:92-104:
    row by row, entries in COO order)."""

    def __init__(self, evaluator, num_var, num_constr):
        if hasattr(evaluator, "initialize"):
            evaluator.initialize(["Grad", "Jac"])                      # src/separators.jl:88
        rows, cols = evaluator.jac_structure()
        rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64)
        order = np.argsort(rows, kind="stable")
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=num_constr))])
        nnz = len(rows)
        lin = [1 if evaluator.isconstrlinear(i) else 0 for i in range(num_constr)]
        super().__init__(num_var, rowptr, cols[order], np.full(num_constr, L.ROW_HOST), lin, np.zeros(num_constr),
                         None, None, None, obj_linear=bool(evaluator.isobjlinear()), obj_kind=L.ROW_HOST)
        self.evaluator = evaluator
        n, m = int(num_var), int(num_constr)

        def rows_cb(_user, xp, gp, jp):
            try:
                x = np.ctypeslib.as_array(xp, (n,)).copy()
                g = np.zeros(m); J = np.zeros(nnz)
                with np.errstate(all="ignore"):
                    evaluator.eval_g(g, x)                              # src/separators.jl:113
                    evaluator.eval_jac_g(J, x)                          # src/separators.jl:112
                if m:
                    np.ctypeslib.as_array(gp, (m,))[:] = g
                if nnz:
                    np.ctypeslib.as_array(jp, (nnz,))[:] = J[order]
                return 0
            except Exception:                                           # never unwind through the C ABI
                return 1

        def obj_cb(_user, xp, fp, gradp):
            try:
                x = np.ctypeslib.as_array(xp, (n,)).copy()
                grad = np.zeros(n)
                with np.errstate(all="ignore"):
                    f = evaluator.eval_f(x)                             # src/nlpeval.jl:35
                    evaluator.eval_grad_f(grad, x)                      # src/nlpeval.jl:37-41
                fp[0] = float(f)
                if n:
                    np.ctypeslib.as_array(gradp, (n,))[:] = grad
                return 0
            except Exception:
                return 1

        self._rows_cb = L.EVAL_ROWS_CB(rows_cb)       # keep the trampolines alive as long as the description
        self._obj_cb = L.EVAL_OBJ_CB(obj_cb)

    def c_struct(self):
        d = super().c_struct()
        d.eval_rows = C.cast(self._rows_cb, C.c_void_p)
        d.eval_obj = C.cast(self._obj_cb, C.c_void_p)
        d.eval_user = None
        return d


def tape_affine(ops, args):
    """(coef dict, constant) of a postfix tape that is affine, else None: one pass that carries affine forms through
    CONST, VAR, ADD, SUB, NEG, and MUL or DIV with one constant side.  The values are those of Expr.affine() of the tape's
    source expression (a + s*b: a[k] + s*b[k] where both hold k, 0.0 + s*b[k] where only b does)."""
    st = []
    for o, c in zip(np.asarray(ops).tolist(), np.asarray(args).tolist()):
        if o == L.OP_CONST:
            st.append(({}, float(c)))
        elif o == L.OP_VAR:
            st.append(({int(c): 1.0}, 0.0))
        elif o == L.OP_NEG:
            co, k = st.pop()
            st.append(({j: -v for j, v in co.items()}, -k))
        elif o in (L.OP_ADD, L.OP_SUB, L.OP_MUL, L.OP_DIV):
            (cb, kb), (ca, ka) = st.pop(), st.pop()
            if o in (L.OP_ADD, L.OP_SUB):
                s = 1.0 if o == L.OP_ADD else -1.0
                co = dict(ca)
                for j, v in cb.items():
                    co[j] = co.get(j, 0.0) + s * v
                st.append((co, ka + s * kb))
            elif o == L.OP_MUL and not ca:
                st.append(({j: ka * v for j, v in cb.items()}, ka * kb))
            elif o == L.OP_MUL and not cb:
                st.append(({j: kb * v for j, v in ca.items()}, ka * kb))
            elif o == L.OP_DIV and not cb:
                st.append(({j: v / kb for j, v in ca.items()}, ka / kb))
            else:
                return None
        else:
            return None
    if not st:
        return {}, 0.0
    assert len(st) == 1, "malformed tape"
    return st[0]


def _linear_objective(d, k):
    """(cols, coefs, constant) of problem k's objective, which must be declared linear and be linear"""
    if isinstance(d, CallbackNLP) or d.obj_kind == L.ROW_HOST:
        raise ValueError("problem %d: host-evaluated rows or objective (CallbackNLP) cannot be fused" % k)
    if not d.obj_linear:
        raise ValueError("problem %d: nonlinear objective; a fused batch needs linear or KTN_ROW_QUAD objectives" % k)
    if d.obj_kind == L.ROW_SEP:
        if len(d.obj_atom_kind) and np.any(d.obj_atom_kind != L.ATOM_LIN):
            raise ValueError("problem %d: objective declared linear has nonlinear atoms" % k)
        return d.obj_col.astype(np.int64), d.obj_p0.copy(), d.obj_const
    if d.obj_kind == L.ROW_QUAD:                                        # what every QuadNLP with obj_Q=None produces
        if d.obj_quad_val is not None and len(d.obj_quad_val):
            raise ValueError("problem %d: KTN_ROW_QUAD objective declared linear has a non-empty Q" % k)
        return d.obj_col.astype(np.int64), d.obj_p0.copy(), d.obj_const
    aff = tape_affine(d.obj_tape_op, d.obj_tape_arg)
    if aff is None:
        raise ValueError("problem %d: objective declared linear is not affine (CONST, VAR, +, -, neg, * or / by a constant)" % k)
    co, c0 = aff
    js = sorted(co)
    return np.asarray(js, dtype=np.int64), np.asarray([co[j] for j in js], dtype=np.float64), c0 + d.obj_const


def quad_objective_bound(d, l_var, u_var, k=0):
    """R with |a'x + 1/2 x'Qx| <= R on the box, for the KTN_ROW_QUAD objective of description d:
    R = sum_j |a_j| m_j + 1/2 sum_jk |q_jk| m_j m_k with m_j = max(|l_j|, |u_j|) over the objective's columns (interval
    arithmetic term by term).  ValueError when a column the objective touches has an infinite bound."""
    cols = d.obj_col.astype(np.int64)
    m = np.maximum(np.abs(np.asarray(l_var, dtype=np.float64)), np.abs(np.asarray(u_var, dtype=np.float64)))
    bad = cols[~np.isfinite(m[cols])]
    if len(bad):
        raise ValueError("problem %d: column %d of the quadratic objective has an infinite bound; the per-instance epigraph "
                         "variable of a fused batch needs a finite interval" % (k, int(bad[0])))
    seg = np.repeat(cols, np.diff(d.obj_quad_ptr))
    return float(np.sum(np.abs(d.obj_p0) * m[cols]) + 0.5 * np.sum(np.abs(d.obj_quad_val) * m[seg] * m[d.obj_quad_col]))


def fuse_problems(problems, allow_quad=False):
    """Block-diagonal union of independent problems (Problem tuples of NLPDescriptions, any mix of separable, tape and
    KTN_ROW_QUAD rows): rows instance after instance, columns shifted by each instance's column offset, tapes copied with their
    VAR arguments shifted, Q segments concatenated with their pointers shifted by the running Q-entry count (a description
    without quad arrays contributes empty segments; the fused description carries quad arrays only if some instance has QUAD
    rows).  A linear objective (separable LIN atoms, an affine tape, or a KTN_ROW_QUAD objective declared linear) enters the
    fused :Min objective as LIN atoms, negated for a :Max instance.  A QUADRATIC objective (KTN_ROW_QUAD, not linear) gets its
    own epigraph at fusion -- the engine refuses a shared epigraph variable under ktn_set_blocks --: instance k gains one last
    variable t_k in [-R, R] (quad_objective_bound) and one last QUAD row  a'x + 1/2 x'Qx - t_k <= 0  (a and Q negated for
    :Max), and its objective becomes t_k + const.  Nonlinear separable or tape objectives are refused: no closed-form bound
    for t exists there.
    KTN_ROW_QUAD rows and objectives are taken with allow_quad=True only (FusedBatch passes it): a caller that hands the fused
    problem to an engine without QUAD rows in its device-side batch loop relied on the ValueError, and the default keeps it.
    Returns (Problem, col_offsets[len + 1], objinfo) with objinfo[k] = (cols, coefs, constant) of instance k's objective in
    ITS own sense and local columns: objval_k = coefs . x_k[cols] + constant (an epigraph instance: ([n_k], [+-1], const);
    its own variables are the first n_k of its column range)."""
    problems = list(problems)
    if not problems:
        raise ValueError("fuse_problems: no problems")
    i64, f64 = np.int64, np.float64
    flat = lambda p, attr: np.asarray(getattr(p, attr), dtype=f64).reshape(-1)
    ds, epi = [], []
    for k, p in enumerate(problems):
        d = p.d
        if isinstance(d, CallbackNLP) or np.any(d.row_kind == L.ROW_HOST) or d.obj_kind == L.ROW_HOST:
            raise ValueError("problem %d: host-evaluated rows or objective (CallbackNLP) cannot be fused" % k)
        if not allow_quad and (np.any(d.row_kind == L.ROW_QUAD) or d.obj_kind == L.ROW_QUAD):
            raise ValueError("problem %d: KTN_ROW_QUAD rows or objective (QuadNLP) are fused with allow_quad=True only "
                             "(FusedBatch passes it)" % k)
        if p.sense not in ("Min", "Max"):
            raise ValueError("problem %d: sense must be 'Min' or 'Max'" % k)
        if d.num_var != int(p.num_var) or d.num_constr != int(p.num_constr):
            raise ValueError("problem %d: num_var / num_constr do not match the description" % k)
        ds.append(d)
        epi.append(d.obj_kind == L.ROW_QUAD and not d.obj_linear)
    has_quad = any(epi) or any(np.any(d.row_kind == L.ROW_QUAD) for d in ds)
    # per instance: extra entries / Q entries / rows / columns of its epigraph row
    xe = [len(d.obj_col) + 1 if e else 0 for d, e in zip(ds, epi)]
    own_q = [0 if d.quad_ptr is None else int(d.quad_ptr[-1] - d.quad_ptr[0]) for d in ds]
    nq = [q + (len(d.obj_quad_val) if e else 0) for d, q, e in zip(ds, own_q, epi)]
    offs = np.concatenate([[0], np.cumsum([d.num_var + int(e) for d, e in zip(ds, epi)])]).astype(i64)
    eoff = np.concatenate([[0], np.cumsum([len(d.col) + x for d, x in zip(ds, xe)])]).astype(i64)
    toff = np.concatenate([[0], np.cumsum([len(d.tape_op) for d in ds])]).astype(i64)
    qoff = np.concatenate([[0], np.cumsum(nq)]).astype(i64)
    rowptr, tape_ptr, col, targs = [np.zeros(1, dtype=i64)], [np.zeros(1, dtype=i64)], [], []
    rkind, rlin, rconst, akind, p0, p1 = [], [], [], [], [], []
    qptr, qcol, qval = [np.zeros(1, dtype=i64)], [], []
    lv, uv, lc, uc = [], [], [], []
    info, ocol, op0, oconst = [], [], [], 0.0
    for k, (p, d, o) in enumerate(zip(problems, ds, offs)):
        sgn = -1.0 if p.sense == "Max" else 1.0
        rowptr.append(d.rowptr[1:] + eoff[k]); tape_ptr.append(d.tape_ptr[1:] + toff[k])
        col.append(d.col + np.int32(o))
        a = d.tape_arg.copy()
        isvar = d.tape_op == L.OP_VAR
        a[isvar] = a[isvar] + float(o)                                  # every other argument bit for bit
        targs.append(a)
        rkind.append(d.row_kind); rlin.append(d.row_linear); rconst.append(d.rconst)
        akind.append(d.atom_kind); p0.append(d.p0); p1.append(d.p1)
        lv.append(flat(p, "l_var")); uv.append(flat(p, "u_var")); lc.append(flat(p, "l_constr")); uc.append(flat(p, "u_constr"))
        if has_quad:
            if d.quad_ptr is None:
                qptr.append(np.full(len(d.col), qoff[k], dtype=i64))
            else:
                qptr.append(d.quad_ptr[1:] - d.quad_ptr[0] + qoff[k])
                seg = slice(int(d.quad_ptr[0]), int(d.quad_ptr[-1]))
                qcol.append(d.quad_col[seg] + np.int32(o)); qval.append(d.quad_val[seg])
        if not epi[k]:
            cols, coefs, c0 = _linear_objective(d, k)
            info.append((cols, coefs, float(c0)))
            ocol.append(cols + o); op0.append(sgn * coefs); oconst += sgn * c0
            continue
        # the instance's own epigraph: variable t (local index n_k) and the QUAD row  sgn (a'x + 1/2 x'Qx) - t <= 0
        n_k, nob = d.num_var, len(d.obj_col)
        R = quad_objective_bound(d, lv[-1], uv[-1], k)
        qb = qoff[k] + own_q[k]                                         # the row's first Q entry
        rowptr.append(np.asarray([eoff[k] + len(d.col) + nob + 1], dtype=i64)); tape_ptr.append(np.asarray([toff[k + 1]], dtype=i64))
        col.append(np.concatenate([d.obj_col.astype(i64) + o, [o + n_k]]).astype(np.int32))
        rkind.append(np.asarray([L.ROW_QUAD], dtype=np.uint8)); rlin.append(np.zeros(1, dtype=np.uint8)); rconst.append(np.zeros(1))
        akind.append(np.zeros(nob + 1, dtype=np.uint8)); p0.append(np.concatenate([sgn * d.obj_p0, [-1.0]])); p1.append(np.zeros(nob + 1))
        seg = d.obj_quad_ptr[1:] - d.obj_quad_ptr[0] + qb
        qptr.append(np.concatenate([seg, seg[-1:] if nob else [qb]]).astype(i64))      # t: the empty segment
        qcol.append(d.obj_quad_col + np.int32(o)); qval.append(sgn * d.obj_quad_val)
        lv.append(np.asarray([-R])); uv.append(np.asarray([R])); lc.append(np.asarray([-np.inf])); uc.append(np.zeros(1))
        info.append((np.asarray([n_k], dtype=i64), np.asarray([sgn]), float(d.obj_const)))
        ocol.append(np.asarray([o + n_k], dtype=i64)); op0.append(np.ones(1)); oconst += sgn * d.obj_const
    cat = np.concatenate
    nobj = int(sum(len(c) for c in ocol))
    quad = {}
    if has_quad:
        quad = dict(quad_ptr=cat(qptr), quad_col=cat(qcol + [np.zeros(0, dtype=np.int32)]).astype(np.int32),
                    quad_val=cat(qval + [np.zeros(0)]).astype(f64))
    fused = NLPDescription(
        int(offs[-1]), cat(rowptr).astype(i64), cat(col).astype(np.int32), cat(rkind), cat(rlin), cat(rconst),
        cat(akind), cat(p0), cat(p1), cat(tape_ptr).astype(i64), cat([d.tape_op for d in ds]), cat(targs),
        obj_linear=True, obj_kind=L.ROW_SEP, obj_col=cat(ocol).astype(np.int32), obj_atom_kind=np.zeros(nobj),
        obj_p0=cat(op0), obj_p1=np.zeros(nobj), obj_const=oconst, **quad)
    big = Problem(fused.num_var, fused.num_constr, cat(lv), cat(uv), cat(lc), cat(uc), "Min", fused)
    return big, offs, info
