"""Expression graphs -> device tapes.

Stands where JuMP's expression graph (`MathProgBase.constr_expr` / `obj_expr`, :ExprGraph)
stands for the reference: the host describes every nonlinear row as an expression, this
module flattens it to the postfix tape the HIP tape interpreter evaluates (opcodes
KTN_OP_* of include/katana_hip.h), finds the row's variables (= its Jacobian structure,
`jac_structure`, src/separators.jl:92) and recognises affine rows (`isconstrlinear` /
`isobjlinear`, src/model.jl:116,125).
"""
import math

import numpy as np

from . import _lib as L

_UNARY = {"neg": L.OP_NEG, "exp": L.OP_EXP, "log": L.OP_LOG, "sqrt": L.OP_SQRT, "sin": L.OP_SIN, "cos": L.OP_COS}
_BINARY = {"+": L.OP_ADD, "-": L.OP_SUB, "*": L.OP_MUL, "/": L.OP_DIV}


class Expr:
    """Immutable expression node: ("const", c) | ("var", j) | (op, args...)."""
    __slots__ = ("op", "args")

    def __init__(self, op, *args):
        self.op = op
        self.args = args

    # -- operator overloading -------------------------------------------------
    @staticmethod
    def wrap(o):
        return o if isinstance(o, Expr) else Expr("const", float(o))

    def __add__(self, o): return Expr("+", self, Expr.wrap(o))
    def __radd__(self, o): return Expr("+", Expr.wrap(o), self)
    def __sub__(self, o): return Expr("-", self, Expr.wrap(o))
    def __rsub__(self, o): return Expr("-", Expr.wrap(o), self)
    def __mul__(self, o): return Expr("*", self, Expr.wrap(o))
    def __rmul__(self, o): return Expr("*", Expr.wrap(o), self)
    def __truediv__(self, o): return Expr("/", self, Expr.wrap(o))
    def __rtruediv__(self, o): return Expr("/", Expr.wrap(o), self)
    def __neg__(self): return Expr("neg", self)
    def __pow__(self, p): return Expr("^", self, float(p))

    # comparison operators build constraints (jump_like.Model.constraint)
    def __le__(self, o): return ("<=", self, Expr.wrap(o))
    def __ge__(self, o): return (">=", self, Expr.wrap(o))

    # -- analysis ---------------------------------------------------------------
    def variables(self):
        acc = set()
        stack = [self]
        while stack:
            e = stack.pop()
            if e.op == "var":
                acc.add(e.args[0])
            elif e.op != "const":
                stack.extend(a for a in e.args if isinstance(a, Expr))
        return sorted(acc)

    def affine(self):
        """Return (coef dict, constant) when the expression is affine, else None.

        Iterative (a left-folded sum of N terms nests N levels deep).  Each node's result belongs to its parent alone,
        so a sum merges the smaller coefficient dict into the larger one in place (_merge); values and key order are
        those of building a fresh `dict(a)` at every node and adding `s * b[k]` key by key."""
        # post-order over the tree: (node, children done?); results (coefs, constant, keys that may hold -0.0) on `out`
        stack, out = [(self, False)], []
        reordered = False
        while stack:
            e, done = stack.pop()
            op = e.op
            if op == "const":
                out.append(({}, e.args[0], set()))
                continue
            if op == "var":
                out.append(({e.args[0]: 1.0}, 0.0, set()))
                continue
            binary = op in ("+", "-", "*", "/")
            if not done:
                stack.append((e, True))
                if binary:
                    stack.append((e.args[1], False))
                stack.append((e.args[0], False))
                continue
            b = out.pop() if binary else None
            a = out.pop()
            if op in ("+", "-"):
                if a is None or b is None:
                    out.append(None)
                    continue
                s = 1.0 if op == "+" else -1.0
                reordered = reordered or len(b[0]) > len(a[0])
                co, z = _merge(a, b, s)
                out.append((co, a[1] + s * b[1], z))
            elif op == "neg":
                out.append(None if a is None else _scaled({k: -v for k, v in a[0].items()}, -a[1]))
            elif op == "*":
                if a is None or b is None:
                    out.append(None)
                elif not a[0]:
                    out.append(_scaled({k: a[1] * v for k, v in b[0].items()}, a[1] * b[1]))
                elif not b[0]:
                    out.append(_scaled({k: b[1] * v for k, v in a[0].items()}, a[1] * b[1]))
                else:
                    out.append(None)
            elif op == "/":
                if a is None or b is None or b[0]:
                    out.append(None)
                else:
                    out.append(_scaled({k: v / b[1] for k, v in a[0].items()}, a[1] / b[1]))
            elif op == "^":
                if a is not None and not a[0]:
                    out.append(({}, a[1] ** e.args[1], set()))
                elif a is not None and e.args[1] == 1.0:
                    out.append(a)
                else:
                    out.append(None)
            elif a is not None and not a[0]:         # unary function of a constant
                f = {"exp": np.exp, "log": np.log, "sqrt": np.sqrt, "sin": np.sin, "cos": np.cos}[op]
                out.append(({}, float(f(a[1])), set()))
            else:
                out.append(None)
        res = out.pop()
        if res is None:
            return None
        co = {j: res[0][j] for j in self._first_occurrence()} if reordered else res[0]
        return co, res[1]

    def _first_occurrence(self):
        """variables in left-to-right leaf order, each once (the key order of affine()'s dict)"""
        seen, order, stack = set(), [], [self]
        while stack:
            e = stack.pop()
            if e.op == "var":
                if e.args[0] not in seen:
                    seen.add(e.args[0]); order.append(e.args[0])
            elif e.op != "const":
                stack.extend(reversed([a for a in e.args if isinstance(a, Expr)]))
        return order

    def tape(self):
        """Postfix tape: (ops int32[], args float64[]).  Iterative post-order walk."""
        ops, args = [], []
        stack = [(self, False)]
        while stack:
            e, done = stack.pop()
            if e.op == "const":
                ops.append(L.OP_CONST); args.append(e.args[0])
            elif e.op == "var":
                ops.append(L.OP_VAR); args.append(float(e.args[0]))
            elif e.op in _BINARY:
                if done:
                    ops.append(_BINARY[e.op]); args.append(0.0)
                else:
                    stack += [(e, True), (e.args[1], False), (e.args[0], False)]
            elif e.op == "^":
                if done:
                    ops.append(L.OP_POWC); args.append(float(e.args[1]))
                else:
                    stack += [(e, True), (e.args[0], False)]
            elif e.op in _UNARY:
                if done:
                    ops.append(_UNARY[e.op]); args.append(0.0)
                else:
                    stack += [(e, True), (e.args[0], False)]
            else:
                raise ValueError("Unsupported operator %r" % (e.op,))
        return np.asarray(ops, dtype=np.int32), np.asarray(args, dtype=np.float64)


def _negzero(v):
    return v == 0.0 and math.copysign(1.0, v) < 0.0


def _scaled(co, c0):
    return co, c0, {k for k, v in co.items() if _negzero(v)}


def _merge(a, b, s):
    """(coefs, keys that may hold -0.0) of a + s*b, for results (coefs, constant, -0.0 keys) owned by the caller.  The
    values are those of `co = dict(a); co[k] = co.get(k, 0.0) + s * v for k, v in b` -- a alone: a[k]; both: a[k] + s b[k];
    b alone: 0.0 + s b[k] -- computed in place in the larger dict; with s = 1 the last is b[k] itself except for -0.0,
    which is why the -0.0 keys are tracked.  Key order is restored by affine()."""
    (ca, _, za), (cb, _, zb) = a, b
    if len(ca) >= len(cb):
        for k, v in cb.items():
            w = ca.get(k, 0.0) + s * v
            ca[k] = w
            if _negzero(w):
                za.add(k)
        return ca, za
    if s != 1.0:
        co = dict(ca)
        for k, v in cb.items():
            co[k] = co.get(k, 0.0) + s * v
        return co, {k for k, v in co.items() if _negzero(v)}
    for k in zb:
        if k not in ca and _negzero(cb[k]):
            cb[k] = 0.0 + cb[k]             # = +0.0
    for k, v in ca.items():
        w = cb.get(k)
        cb[k] = v if w is None else v + w
    return cb, {k for k in (za | zb) if _negzero(cb[k])}


def var(j): return Expr("var", int(j))
def const(c): return Expr("const", float(c))
def exp(a): return Expr("exp", Expr.wrap(a))
def log(a): return Expr("log", Expr.wrap(a))
def sqrt(a): return Expr("sqrt", Expr.wrap(a))
def sin(a): return Expr("sin", Expr.wrap(a))
def cos(a): return Expr("cos", Expr.wrap(a))


def from_sexpr(s):
    """Nested-list form (tests/golden/kat_models.json) -> Expr.  n-ary + and * fold left to right.  Iterative: the
    nesting depth of `s` is not limited by Python's recursion limit."""
    stack, out = [(s, False)], []
    while stack:
        s, done = stack.pop()
        if isinstance(s, (int, float)):
            out.append(const(s))
            continue
        op = s[0]
        if op == "var":
            out.append(var(s[1]))
            continue
        if op in ("+", "*"):
            kids = s[1:]
        elif op in ("-", "/"):
            kids = s[1:3]
        elif op == "^" or op in _UNARY:
            kids = s[1:2]
        else:
            raise ValueError("unknown op %r" % (op,))
        if not done:
            stack.append((s, True))
            stack.extend((k, False) for k in reversed(kids))
            continue
        args = out[len(out) - len(kids):]
        del out[len(out) - len(kids):]
        if op == "^":
            out.append(args[0] ** float(s[2]))
        elif op in ("+", "*"):
            e = args[0]
            for a in args[1:]:
                e = Expr(op, e, a)
            out.append(e)
        else:
            out.append(Expr(op, *args))
    return out.pop()
