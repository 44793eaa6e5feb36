"""CPU tier: the host-side tape compiler (katana.jl_amd/expr.py) and the high-precision tape reference (tape_ref.py).

The compiler is iterative; its output must be bit-identical to the recursive formulation it replaced, which is kept
below as the pinned baseline (run on expressions shallow enough for it)."""
import math

import numpy as np
import pytest

import katana_jl_amd as ktn
import tape_ref
from fuzz_models import model_at
from kat_util import load_kats
from oracle import sexpr
from test_expr import _eval_tape

L = ktn._lib
Expr = ktn.Expr


# ---- the recursive compiler as it was (baseline) --------------------------------------------------------------------
def _old_affine(self):
    op = self.op
    if op == "const":
        return {}, self.args[0]
    if op == "var":
        return {self.args[0]: 1.0}, 0.0
    if op in ("+", "-"):
        a, b = _old_affine(self.args[0]), _old_affine(self.args[1])
        if a is None or b is None:
            return None
        s = 1.0 if op == "+" else -1.0
        co = dict(a[0])
        for k, v in b[0].items():
            co[k] = co.get(k, 0.0) + s * v
        return co, a[1] + s * b[1]
    if op == "neg":
        a = _old_affine(self.args[0])
        return None if a is None else ({k: -v for k, v in a[0].items()}, -a[1])
    if op == "*":
        a, b = _old_affine(self.args[0]), _old_affine(self.args[1])
        if a is None or b is None:
            return None
        if not a[0]:
            return {k: a[1] * v for k, v in b[0].items()}, a[1] * b[1]
        if not b[0]:
            return {k: b[1] * v for k, v in a[0].items()}, a[1] * b[1]
        return None
    if op == "/":
        a, b = _old_affine(self.args[0]), _old_affine(self.args[1])
        if a is None or b is None or b[0]:
            return None
        return {k: v / b[1] for k, v in a[0].items()}, a[1] / b[1]
    if op == "^":
        a = _old_affine(self.args[0])
        if a is not None and not a[0]:
            return {}, a[1] ** self.args[1]
        if a is not None and self.args[1] == 1.0:
            return a
        return None
    a = _old_affine(self.args[0])
    if a is not None and not a[0]:
        f = {"exp": np.exp, "log": np.log, "sqrt": np.sqrt, "sin": np.sin, "cos": np.cos}[op]
        return {}, float(f(a[1]))
    return None


_UN = {"neg": L.OP_NEG, "exp": L.OP_EXP, "log": L.OP_LOG, "sqrt": L.OP_SQRT, "sin": L.OP_SIN, "cos": L.OP_COS}
_BIN = {"+": L.OP_ADD, "-": L.OP_SUB, "*": L.OP_MUL, "/": L.OP_DIV}


def _old_tape(self):
    ops, args = [], []

    def emit(e):
        if e.op == "const":
            ops.append(L.OP_CONST); args.append(e.args[0])
        elif e.op == "var":
            ops.append(L.OP_VAR); args.append(float(e.args[0]))
        elif e.op in _BIN:
            emit(e.args[0]); emit(e.args[1])
            ops.append(_BIN[e.op]); args.append(0.0)
        elif e.op == "^":
            emit(e.args[0])
            ops.append(L.OP_POWC); args.append(float(e.args[1]))
        else:
            emit(e.args[0])
            ops.append(_UN[e.op]); args.append(0.0)
    emit(self)
    return np.asarray(ops, dtype=np.int32), np.asarray(args, dtype=np.float64)


def _old_from_sexpr(s):
    if isinstance(s, (int, float)):
        return ktn.const(s)
    op = s[0]
    if op == "var":
        return ktn.var(s[1])
    if op == "^":
        return _old_from_sexpr(s[1]) ** float(s[2])
    if op in ("+", "*"):
        e = _old_from_sexpr(s[1])
        for a in s[2:]:
            e = Expr(op, e, _old_from_sexpr(a))
        return e
    if op in ("-", "/"):
        return Expr(op, _old_from_sexpr(s[1]), _old_from_sexpr(s[2]))
    return Expr(op, _old_from_sexpr(s[1]))


def _same_tree(a, b):
    st = [(a, b)]
    while st:
        x, y = st.pop()
        if isinstance(x, Expr) != isinstance(y, Expr):
            return False
        if not isinstance(x, Expr):
            if not _bits_equal(x, y):
                return False
            continue
        if x.op != y.op or len(x.args) != len(y.args):
            return False
        st.extend(zip(x.args, y.args))
    return True


def _bits_equal(a, b):
    if isinstance(a, float) or isinstance(b, float):
        return type(a) is type(b) and np.float64(a).tobytes() == np.float64(b).tobytes()
    return a == b


def _same_affine(new, old):
    if old is None or new is None:
        return old is None and new is None
    return (list(new[0]) == list(old[0]) and all(_bits_equal(new[0][k], old[0][k]) for k in old[0])
            and _bits_equal(new[1], old[1]))


def _same_tape(new, old):
    return (new[0].dtype == old[0].dtype and new[1].dtype == old[1].dtype and np.array_equal(new[0], old[0])
            and new[1].tobytes() == old[1].tobytes())


def _rand_expr(rng, depth, nv):
    """random shallow expressions over every operator, with signed zeros and repeated / cancelling variables"""
    if depth == 0 or rng.random() < 0.25:
        r = rng.random()
        if r < 0.55:
            return ktn.var(int(rng.integers(nv)))
        return ktn.const(float(rng.choice([0.0, -0.0, 1.0, -1.0, 2.5, -3.0, 0.5, 1e-300])))
    k = rng.integers(12)
    a = _rand_expr(rng, depth - 1, nv)
    if k < 6:
        b = _rand_expr(rng, depth - 1, nv)
        return [a + b, a - b, a * b, a / b, a + b, -1.0 * a - b][k]
    if k == 6:
        return a ** float(rng.choice([0.0, 1.0, 2.0, 3.0, -1.0, 0.5]))
    return [-a, ktn.exp(a), ktn.log(a), ktn.sqrt(a), ktn.sin(a)][k - 7]


def test_compiler_matches_the_recursive_baseline_on_every_reference_model():
    for m in load_kats():
        for s in [m["objective"]] + [c["expr"] for c in m["constraints"]]:
            e, e0 = ktn.from_sexpr(s), _old_from_sexpr(s)
            assert _same_tree(e, e0), m["id"]
            assert _same_tape(e.tape(), _old_tape(e0)), m["id"]
            assert _same_affine(e.affine(), _old_affine(e0)), m["id"]
    for seed, idx in [(1, 3), (2, 0), (5, 7), (11, 2)]:
        m = model_at(seed, idx)
        for s in [m["objective"]] + [c["expr"] for c in m["constraints"]]:
            e = ktn.from_sexpr(s)
            assert _same_tape(e.tape(), _old_tape(e)) and _same_affine(e.affine(), _old_affine(e))


def test_compiler_matches_the_recursive_baseline_on_random_expressions():
    rng = np.random.default_rng(3)
    n_aff = 0
    with np.errstate(all="ignore"):
        for _ in range(3000):
            e = _rand_expr(rng, int(rng.integers(1, 7)), 5)
            assert _same_tape(e.tape(), _old_tape(e))
            try:
                old = _old_affine(e)
            except (ZeroDivisionError, OverflowError) as exc:       # a constant 0.0 ** -1.0 and the like: same error
                with pytest.raises(type(exc)):
                    e.affine()
                continue
            assert _same_affine(e.affine(), old), (old, e.affine())
            n_aff += old is not None
    assert n_aff > 300


def test_affine_keeps_signed_zeros_and_key_order_of_the_baseline():
    x = [ktn.var(j) for j in range(6)]
    z = -0.0 * x[2]                                  # coefficient -0.0
    cases = [
        x[0] + (x[1] + (z + x[3])),                  # right-folded: merged into the larger dict
        x[0] + (z + (x[4] + (x[5] + x[1]))),
        (x[3] + z) + x[0],
        x[0] - (z - (x[4] + x[5])),
        z + (x[2] + (x[1] + x[0])),
        (x[0] - x[0]) + (x[1] + (x[2] + (-1.0 * x[0]))),
        -(x[1] + (z + x[4])) + (x[5] + (x[2] + (x[3] + x[0]))),
    ]
    for e in cases:
        assert _same_affine(e.affine(), _old_affine(e)), (e.affine(), _old_affine(e))


@pytest.mark.parametrize("n", [300, 700])
def test_folded_sums_as_deep_as_the_baseline_allows_match_it(n):
    x = [ktn.var(j) for j in range(n)]
    rng = np.random.default_rng(n)
    c = rng.normal(size=n)
    left = x[0] * c[0]
    for j in range(1, n):
        left = left + c[j] * x[j] if j % 3 else left - c[j] * x[j]
    right = x[n - 1] * c[n - 1]
    for j in range(n - 2, -1, -1):
        right = c[j] * x[j] + right if j % 3 else c[j] * x[j] - right
    nonlin = x[0] ** 2
    for j in range(1, n):
        nonlin = x[j] ** 2 + nonlin
    for e in (left, right, nonlin):
        assert _same_tape(e.tape(), _old_tape(e)) and _same_affine(e.affine(), _old_affine(e))


def _fold(terms, op, right):
    if right:
        e = terms[-1]
        for t in reversed(terms[:-1]):
            e = Expr(op, t, e)
        return e
    e = terms[0]
    for t in terms[1:]:
        e = Expr(op, e, t)
    return e


@pytest.mark.parametrize("right", [False, True], ids=["left", "right"])
@pytest.mark.parametrize("op", ["+", "*"])
def test_folded_sums_and_products_of_1e5_terms_compile_and_evaluate(op, right):
    N = 100000
    rng = np.random.default_rng(17)
    if op == "+":
        x = rng.uniform(-2.0, 2.0, N)
        terms = [ktn.var(j) ** 2 for j in range(N)]
    else:
        x = rng.uniform(0.999, 1.001, N)
        terms = [ktn.var(j) for j in range(N)]
    e = _fold(terms, op, right)
    ops, args = e.tape()
    assert len(ops) == (3 if op == "+" else 2) * N - 1
    assert e.variables() == list(range(N))
    assert e.affine() is None
    ref = tape_ref.evaluate(ops, args, x)
    assert len(ref.grad) == N
    ref.check_value(_eval_tape(ops, args, x), "stack evaluator")
    s = tape_ref.tape_to_sexpr(ops, args)
    e2 = ktn.from_sexpr(s)                                         # 1e5-deep nested lists as well
    assert _same_tape(e2.tape(), (ops, args))


def test_affine_sums_of_1e5_terms_in_both_foldings():
    N = 100000
    terms = [(j % 7 - 3.0) * ktn.var(j) for j in range(N)]
    for right in (False, True):
        co, c0 = _fold(terms + [ktn.const(2.0)], "+", right).affine()
        assert list(co) == list(range(N)) and c0 == 2.0
        assert all(co[j] == j % 7 - 3.0 for j in range(N))


def test_exprnlp_loads_a_2000_term_quadratic_row():
    N = 2000
    d = ktn.ExprNLP(N, ktn.var(0), [sum(ktn.var(j) ** 2 for j in range(N)) - 1.0])
    assert list(d.row_kind) == [L.ROW_TAPE] and list(d.col) == list(range(N))
    assert len(d.tape_op) == 3 * N + 3                            # 0 + x0^2 + ... + x_{N-1}^2 - 1


# ---- the reference itself --------------------------------------------------------------------------------------------
def test_reference_agrees_with_the_oracle_forward_mode_on_the_reference_models():
    rng = np.random.default_rng(4)
    for m in load_kats():
        n = len(m["vars"])
        x = rng.uniform(0.3, 1.7, n)
        for s in [m["objective"]] + [c["expr"] for c in m["constraints"]]:
            ops, args = ktn.from_sexpr(s).tape()
            r = tape_ref.evaluate(ops, args, x)
            v, g = sexpr.eval_grad(s, x)
            r.check_value(v, m["id"])
            r.check_grad({j: g.get(j, 0.0) for j in r.grad_f64}, m["id"])


def test_reference_classes_and_bounds_on_edges():
    v = [ktn.var(j) for j in range(3)]
    x = np.array([0.0, -2.0, 4.0])
    nan, inf = math.nan, math.inf
    cases = [   # expression, expected value class / value, expected partial of column 0 or 1
        (ktn.log(v[0]), -inf, {0: inf}),
        (ktn.sqrt(v[0]), 0.0, {0: inf}),
        (ktn.sqrt(v[1]), nan, {1: nan}),
        (v[0] ** -1.0, inf, {0: -inf}),
        (v[0] ** 0.0, 1.0, {0: nan}),
        (v[1] ** (1.0 / 3.0), nan, {1: nan}),
        (v[1] ** 3.0, -8.0, {1: 12.0}),
        (v[2] / v[0], inf, {2: inf, 0: -inf}),
        (ktn.exp(v[2] * 200.0), inf, {2: inf}),
    ]
    for e, val, grad in cases:
        ops, args = e.tape()
        r = tape_ref.evaluate(ops, args, x, cross_check=True)
        assert tape_ref.same_class(r.value_f64, val), (ops, r.value_f64)
        for j, gv in grad.items():
            assert tape_ref.same_class(r.grad_f64[j], gv), (ops, j, r.grad_f64[j])
    # a wrong last bit in a finite value or partial is outside the bound where the bound is tight
    ops, args = (v[2] * v[2]).tape()
    r = tape_ref.evaluate(ops, args, x)
    r.check_value(16.0); r.check_grad({2: 8.0})
    with pytest.raises(AssertionError):
        r.check_grad({2: 8.0 + 8 * 2 ** -52 * 8})
    with pytest.raises(AssertionError):
        r.check_grad({2: 8.0, 1: 1e-300})                          # a column the tape does not use must be exactly 0
