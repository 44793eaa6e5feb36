"""High-precision reference for postfix expression tapes (test code).

`evaluate(ops, args, x)` runs a tape (the KTN_OP_* arrays of katana.jl_amd/expr.py, include/katana_hip.h) three ways,
all iteratively so that 1e5-deep tapes need no recursion:

* in mpmath at `mp.prec` = 200 bits: the exact value and the exact gradient (reverse mode);
* in float64 under the NaNMath convention of oracle/sexpr.py (log / sqrt / pow outside their domain give NaN, division
  by zero gives +-inf, exp overflows to +inf; derivative rules as there: pow with p = 2 -> 2a, p = 1 -> 1, else
  p * a^(p-1); log' = 1/a; sqrt' = 0.5/sqrt(a)): only to find the components whose float64 result is not finite, and
  their class (NaN, +inf or -inf);
* once more in mpmath with every partial and adjoint replaced by its absolute value: `jmag`.

Error bounds (u = 2^-53):

* value: E = sum over nodes |adj_node| * (u |v_node| + eta) * c_op, adj the exact adjoint, c_op = 1 for + - * / sqrt,
  0 for CONST VAR NEG, 4 for exp log pow sin cos (the ULP4 convention for the device libm).  A device value passes when
  |dev - exact| <= 2E + 4u|exact|  (first-order forward error of the evaluation, doubled, plus the final rounding).
  eta = 2^-1075 is the absolute rounding error of a result in the subnormal range (exp(-750) rounds to 0): without it
  the relative bound would reject a correctly rounded underflow.
* Jacobian: |J_dev - J_exact| <= (4L + 8) (u Jmag + eta), with L the number of ops other than + and - on the longest path from
  a leaf to the root: every path's product of partials carries at most L factors, each a rounded product of a libm
  result (<= 4 ulp) and an adjoint, and Jmag sums the absolute values of those products over all paths.
* non-finite: where the float64 result is not finite the device must give exactly its class (NaN, or inf with its
  sign).  Edge rows keep to one non-finite source, so forward mode (oracle/sexpr.py) and reverse mode cannot
  legitimately differ; `evaluate(..., cross_check=True)` asserts that they do not.
"""
import math

import mpmath
from mpmath import mp, mpf

from oracle import sexpr

(OP_CONST, OP_VAR, OP_ADD, OP_SUB, OP_MUL, OP_DIV, OP_NEG, OP_POWC, OP_EXP, OP_LOG, OP_SQRT, OP_SIN,
 OP_COS) = range(13)
U = 2.0 ** -53
ETA = mpf(2) ** -1075       # absolute rounding error of a result in the subnormal range (0.0 as a float64)
PREC = 200
_NAME = {OP_ADD: "+", OP_SUB: "-", OP_MUL: "*", OP_DIV: "/", OP_NEG: "neg", OP_EXP: "exp", OP_LOG: "log",
         OP_SQRT: "sqrt", OP_SIN: "sin", OP_COS: "cos"}
_C_OP = {OP_CONST: 0, OP_VAR: 0, OP_NEG: 0, OP_ADD: 1, OP_SUB: 1, OP_MUL: 1, OP_DIV: 1, OP_SQRT: 1,
         OP_EXP: 4, OP_LOG: 4, OP_POWC: 4, OP_SIN: 4, OP_COS: 4}


def _finite(v):
    return v == v and abs(v) != math.inf


class TapeResult:
    """value: exact value (mpf, None where the float64 value is not finite); value_f64: float64 NaNMath value; err: the
    bound E; grad / grad_f64 / jmag: {column: ...} (grad None where the float64 component is not finite); L: as above"""

    def check_value(self, dev, what=""):
        if not _finite(self.value_f64):
            assert same_class(dev, self.value_f64), ("value class", what, dev, self.value_f64)
            return
        ex = self.value
        with mp.workprec(PREC):
            tol = 2 * self.err + 4 * mpf(U) * abs(ex)
            ok = _finite(dev) and abs(mpf(dev) - ex) <= tol
        assert ok, ("value", what, dev, float(ex), float(abs(mpf(dev) - ex)), float(tol))

    def grad_tol(self, c):
        """the bound on |J_dev - J_exact| of column c (mpf; 0 for a column the tape does not use)"""
        with mp.workprec(PREC):
            return (4 * self.L + 8) * (mpf(U) * self.jmag[c] + ETA) if c in self.jmag else mpf(0)

    def check_grad(self, dev_by_col, what=""):
        """dev_by_col: {column: device partial (per-column sum over the row's structure entries)}.  Columns of the
        structure the tape never uses must be exactly 0."""
        for c, dv in dev_by_col.items():
            if c not in self.grad_f64:
                assert dv == 0.0, ("unused column not exactly 0", what, c, dv)
                continue
            want = self.grad_f64[c]
            if not _finite(want):
                assert same_class(dv, want), ("partial class", what, c, dv, want)
                continue
            ex = self.grad[c]
            with mp.workprec(PREC):
                tol = self.grad_tol(c)
                ok = _finite(dv) and abs(mpf(dv) - ex) <= tol
            assert ok, ("partial", what, c, dv, float(ex), float(abs(mpf(dv) - ex)), float(tol))
        missing = set(self.grad_f64) - set(dev_by_col)
        assert not missing, ("tape columns missing from the device row", what, sorted(missing)[:5])


def same_class(a, b):
    """NaN matches NaN, inf matches inf of the same sign, finite values match exactly"""
    if a != a or b != b:
        return a != a and b != b
    return a == b


def _f64_unary(op, v, p=0.0):
    if op == OP_NEG:
        return -v
    if op == OP_POWC:
        return sexpr._pow(v, p)
    if op == OP_EXP:
        return sexpr._exp(v)
    if op == OP_LOG:
        return sexpr._log(v)
    if op == OP_SQRT:
        return sexpr._sqrt(v)
    if op == OP_SIN:
        return math.sin(v) if _finite(v) else math.nan
    return math.cos(v) if _finite(v) else math.nan


def _f64_binary(op, a, b):
    if op == OP_ADD:
        return a + b
    if op == OP_SUB:
        return a - b
    if op == OP_MUL:
        return sexpr._mul(a, b)
    return sexpr._div(a, b)


def _mp_pow(a, p):
    """a^p for real a and p (C pow: 0^0 = 1); None where not a finite real"""
    if a == 0:
        return None if p < 0 else (mpf(1) if p == 0 else mpf(0))
    if a < 0 and p != int(p):
        return None
    return mpmath.power(a, p) if a > 0 else mpmath.power(-a, p) * (-1 if int(p) % 2 else 1)


def _mp_value(op, a, b, c):
    """exact value, None where it does not exist as a finite real"""
    if op in (OP_ADD, OP_SUB, OP_MUL, OP_DIV) and (a is None or b is None):
        return None
    if op >= OP_ADD and a is None:
        return None
    if op == OP_ADD:
        return a + b
    if op == OP_SUB:
        return a - b
    if op == OP_MUL:
        return a * b
    if op == OP_DIV:
        return None if b == 0 else a / b
    if op == OP_NEG:
        return -a
    if op == OP_POWC:
        return _mp_pow(a, mpf(c))
    if op == OP_EXP:
        return mpmath.exp(a)
    if op == OP_LOG:
        return None if a <= 0 else mpmath.log(a)
    if op == OP_SQRT:
        return None if a < 0 else mpmath.sqrt(a)
    if op == OP_SIN:
        return mpmath.sin(a)
    return mpmath.cos(a)


def _mp_partials(op, a, b, v, c):
    """exact partials of node value v = op(a[, b]) w.r.t. its operands; None where not finite"""
    if op == OP_ADD:
        return mpf(1), mpf(1)
    if op == OP_SUB:
        return mpf(1), mpf(-1)
    if op == OP_MUL:
        return b, a
    if op == OP_DIV:
        return (None, None) if (b == 0 or v is None) else (1 / b, -v / b)
    if op == OP_NEG:
        return mpf(-1), None
    if op == OP_POWC:
        p = mpf(c)
        if p == 2:
            return 2 * a, None
        if p == 1:
            return mpf(1), None
        if a == 0 and p < 1:
            return None, None             # p a^(p-1) at a = 0: inf, or 0 * inf = NaN for p = 0
        q = _mp_pow(a, p - 1)
        return (None if q is None else p * q), None
    if op == OP_EXP:
        return v, None                    # (None where exp overflows float64)
    if op == OP_LOG:
        return (None if a == 0 else 1 / a), None      # 1/a also below 0, where the value is NaN (oracle/sexpr.py)
    if op == OP_SQRT:
        return (None, None) if (v is None or v == 0) else (mpf("0.5") / v, None)
    if op == OP_SIN:
        return mpmath.cos(a), None
    return -mpmath.sin(a), None


def _f64_partials(op, a, b, v, c):
    """float64 partials under oracle/sexpr.py's rules (IEEE: 0 * inf = NaN when they meet an adjoint)"""
    if op == OP_ADD:
        return 1.0, 1.0
    if op == OP_SUB:
        return 1.0, -1.0
    if op == OP_MUL:
        return b, a
    if op == OP_DIV:
        return sexpr._div(1.0, b), -sexpr._div(v, b)
    if op == OP_NEG:
        return -1.0, None
    if op == OP_POWC:
        if c == 2.0:
            return 2.0 * a, None
        if c == 1.0:
            return 1.0, None
        return sexpr._mul(c, sexpr._pow(a, c - 1.0)), None
    if op == OP_EXP:
        return v, None
    if op == OP_LOG:
        return sexpr._div(1.0, a), None
    if op == OP_SQRT:
        return (sexpr._div(0.5, v) if v == v else math.nan), None
    if op == OP_SIN:
        return (math.cos(a) if _finite(a) else math.nan), None
    return (-math.sin(a) if _finite(a) else math.nan), None


def tape_to_sexpr(ops, args):
    """postfix tape -> nested-list expression of oracle/sexpr.py (iterative; for cross-checks of small tapes)"""
    st = []
    for o, a in zip(ops, args):
        o = int(o)
        if o == OP_CONST:
            st.append(float(a))
        elif o == OP_VAR:
            st.append(["var", int(a)])
        elif o in (OP_ADD, OP_SUB, OP_MUL, OP_DIV):
            r = st.pop(); l = st.pop()
            st.append([_NAME[o], l, r])
        elif o == OP_POWC:
            st.append(["^", st.pop(), float(a)])
        else:
            st.append([_NAME[o], st.pop()])
    assert len(st) == 1
    return st[0]


def evaluate(ops, args, x, rconst=0.0, cross_check=None):
    """Reference value and gradient of `tape + rconst` at x.  An empty tape is the constant rconst."""
    ops = [int(o) for o in ops]
    args = [float(a) for a in args]
    n = len(ops)
    R = TapeResult()
    if n == 0:
        ops, args, n = [OP_CONST], [0.0], 1
    with mp.workprec(PREC):
        ka, kb = [0] * n, [0] * n
        fv, mv = [0.0] * n, [None] * n
        st = []
        for i in range(n):
            o, c = ops[i], args[i]
            if o == OP_CONST:
                fv[i], mv[i] = c, mpf(c)
            elif o == OP_VAR:
                fv[i] = float(x[int(c)]); mv[i] = mpf(fv[i])
            elif o in (OP_ADD, OP_SUB, OP_MUL, OP_DIV):
                kb[i] = st.pop(); ka[i] = st.pop()
                fv[i] = _f64_binary(o, fv[ka[i]], fv[kb[i]])
                mv[i] = _mp_value(o, mv[ka[i]], mv[kb[i]], c)
            else:
                ka[i] = st.pop()
                fv[i] = _f64_unary(o, fv[ka[i]], c)
                mv[i] = _mp_value(o, mv[ka[i]], None, c)
            if not _finite(fv[i]):
                mv[i] = None                  # a float64 overflow (exp(710)) is a class, not a value
            st.append(i)
        assert len(st) == 1, "malformed tape"
        # reverse sweeps: exact adjoint, float64 adjoint, |.| adjoint; path depth in non-+/- ops
        ma, fa, aa = [mpf(0)] * n, [0.0] * n, [mpf(0)] * n
        depth = [0] * n
        root = n - 1
        ma[root], fa[root], aa[root] = mpf(1), 1.0, mpf(1)
        E = mpf(0)
        L = 0
        grad, gf, jm = {}, {}, {}
        for i in range(n - 1, -1, -1):
            o, w, wf, wa = ops[i], ma[i], fa[i], aa[i]
            if w is not None and mv[i] is not None:
                E += abs(w) * (abs(mv[i]) * U + ETA) * _C_OP[o]
            if o == OP_CONST:
                continue
            if o == OP_VAR:
                j = int(args[i])
                L = max(L, depth[i])
                gf[j] = gf.get(j, 0.0) + wf
                jm[j] = jm.get(j, mpf(0)) + wa
                if j not in grad:
                    grad[j] = mpf(0)
                grad[j] = None if (grad[j] is None or w is None) else grad[j] + w
                continue
            d = depth[i] + (0 if o in (OP_ADD, OP_SUB) else 1)
            a = ka[i]
            b = kb[i] if o in (OP_ADD, OP_SUB, OP_MUL, OP_DIV) else None
            pa, pb = _mp_partials(o, mv[a], mv[b] if b is not None else None, mv[i], args[i]) \
                if (mv[a] is not None and (b is None or mv[b] is not None)) else (None, None)
            fpa, fpb = _f64_partials(o, fv[a], fv[b] if b is not None else None, fv[i], args[i])
            for k, p, fp in ((a, pa, fpa),) + (((b, pb, fpb),) if b is not None else ()):
                depth[k] = d
                ma[k] = None if (w is None or p is None) else ma[k] + w * p      # (a tape is a tree: one parent each)
                fa[k] = fa[k] + sexpr._mul(wf, fp)
                aa[k] = aa[k] + wa * (abs(p) if p is not None else mpf(0))
        R.value_f64 = fv[root] + rconst
        R.value = None if mv[root] is None else mv[root] + mpf(rconst)
        if rconst != 0.0 and R.value is not None:
            E += abs(R.value) * U + ETA       # the device's final  g = v + rconst
        if not _finite(R.value_f64):
            R.value = None
        R.err = E
        R.L = L
        R.grad_f64 = gf
        R.grad = {j: (v if _finite(gf[j]) else None) for j, v in grad.items()}
        R.jmag = jm
        for j in gf:
            assert not _finite(gf[j]) or R.grad[j] is not None, \
                ("a finite float64 partial whose exact value does not exist: keep edge rows to one non-finite source", j)
        if _finite(R.value_f64) and R.value is None:
            raise AssertionError("a finite float64 value whose exact value does not exist: keep edge rows to one non-finite source")
    if cross_check is None:
        cross_check = n <= 400 and (not _finite(R.value_f64) or not all(_finite(v) for v in gf.values()))
    if cross_check:
        # forward mode (oracle/sexpr.py) gives the same non-finite classes
        s = tape_to_sexpr(ops, args)
        v, g = sexpr.eval_grad(s, x)
        assert same_class(v + rconst, R.value_f64) or (_finite(v) and _finite(R.value_f64)), ("forward/reverse value class", v, R.value_f64)
        for j, gv in gf.items():
            fw = g.get(j, 0.0)
            assert (_finite(fw) and _finite(gv)) or same_class(fw, gv), ("forward/reverse partial class", j, fw, gv)
    return R
