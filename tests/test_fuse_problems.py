"""CPU tier: nlp.fuse_problems -- the block-diagonal union of expression-built problems (separable and tape rows) that
throughput mode loads as one problem.  Structure, tapes (against the reference of tests/tape_ref.py), objectives."""
import math

import numpy as np
import pytest

import katana_jl_amd as ktn
import tape_ref
from fuse_helpers import expr_problem, julia_problem

L = ktn._lib


def mixed_problems():
    rng = np.random.default_rng(7)
    sizes = [(40, 6, 4), (25, 3, 3), (60, 9, 5), (33, 4, 4), (50, 7, 6)]
    insts = [ktn.instances.make_instance(n=n, m_nl=m, k=k, family="explog", seed=90 + s) for s, (n, m, k) in enumerate(sizes)]
    probs = [expr_problem(i) if s % 2 == 0 else julia_problem(i, rng) for s, i in enumerate(insts)]
    return insts, probs


def test_fused_structure_offsets_kinds_and_tapes():
    insts, probs = mixed_problems()
    big, offs, info = ktn.fuse_problems(probs)
    d = big.d
    assert big.sense == "Min" and big.num_var == sum(i.n for i in insts) == offs[-1]
    assert list(offs) == list(np.concatenate([[0], np.cumsum([p.num_var for p in probs])]))
    assert big.num_constr == sum(p.num_constr for p in probs)
    np.testing.assert_array_equal(big.l_var, np.concatenate([p.l_var for p in probs]))
    np.testing.assert_array_equal(big.u_constr, np.concatenate([p.u_constr for p in probs]))
    r0 = e0 = t0 = 0
    x = np.random.default_rng(3).uniform(0.5, 1.5, big.num_var)
    ntape = 0
    for k, p in enumerate(probs):
        s = p.d
        m = s.num_constr
        # rows instance after instance: rowptr, col (shifted), kinds, declared linearity, constants, atoms
        np.testing.assert_array_equal(d.rowptr[r0:r0 + m + 1], s.rowptr + e0)
        nnz = len(s.col)
        np.testing.assert_array_equal(d.col[e0:e0 + nnz], s.col + offs[k])
        np.testing.assert_array_equal(d.row_kind[r0:r0 + m], s.row_kind)
        np.testing.assert_array_equal(d.row_linear[r0:r0 + m], s.row_linear)
        np.testing.assert_array_equal(d.rconst[r0:r0 + m], s.rconst)
        np.testing.assert_array_equal(d.atom_kind[e0:e0 + nnz], s.atom_kind)
        np.testing.assert_array_equal(d.p0[e0:e0 + nnz], s.p0)
        np.testing.assert_array_equal(d.tape_ptr[r0:r0 + m + 1], s.tape_ptr + t0)
        tl = len(s.tape_op)
        np.testing.assert_array_equal(d.tape_op[t0:t0 + tl], s.tape_op)
        isvar = s.tape_op == L.OP_VAR
        np.testing.assert_array_equal(d.tape_arg[t0:t0 + tl][isvar], s.tape_arg[isvar] + offs[k])
        assert d.tape_arg[t0:t0 + tl][~isvar].tobytes() == s.tape_arg[~isvar].tobytes()          # bit for bit
        # every fused tape row: value and gradient equal the original row's at the instance's slice, exactly
        xk = x[offs[k]:offs[k + 1]]
        for i in range(m):
            if s.row_kind[i] != L.ROW_TAPE:
                continue
            ntape += 1
            so, sa = s.tape_op[s.tape_ptr[i]:s.tape_ptr[i + 1]], s.tape_arg[s.tape_ptr[i]:s.tape_ptr[i + 1]]
            g = r0 + i
            fo, fa = d.tape_op[d.tape_ptr[g]:d.tape_ptr[g + 1]], d.tape_arg[d.tape_ptr[g]:d.tape_ptr[g + 1]]
            ref = tape_ref.evaluate(so, sa, xk, s.rconst[i])
            fus = tape_ref.evaluate(fo, fa, x, d.rconst[g])
            assert fus.value_f64 == ref.value_f64 and fus.value == ref.value
            assert fus.grad_f64 == {j + offs[k]: v for j, v in ref.grad_f64.items()}
            assert fus.grad == {j + offs[k]: v for j, v in ref.grad.items()}
            # the row's structure names exactly the tape's variables
            assert sorted(d.col[d.rowptr[g]:d.rowptr[g + 1]]) == sorted(fus.grad_f64)
        r0 += m; e0 += nnz; t0 += tl
    assert ntape == sum(i.num_constr for k, i in enumerate(insts) if k % 2) + sum(i.m_nl for k, i in enumerate(insts) if k % 2 == 0)
    assert len(d.rowptr) == r0 + 1 and len(d.col) == e0 and len(d.tape_op) == t0


def test_fused_objective_is_the_sum_of_the_instances():
    insts, probs = mixed_problems()
    big, offs, info = ktn.fuse_problems(probs)
    d = big.d
    assert d.obj_kind == L.ROW_SEP and d.obj_linear and np.all(d.obj_atom_kind == L.ATOM_LIN)
    x = np.random.default_rng(5).uniform(-1, 1, big.num_var)
    tot = 0.0
    for k, inst in enumerate(insts):
        cols, coefs, c0 = info[k]
        xk = x[offs[k]:offs[k + 1]]
        want = float(np.dot(inst.obj_p0, xk[inst.obj_col]) + inst.obj_const)
        got = float(np.sum(coefs * xk[cols]) + c0)
        assert abs(got - want) <= 1e-12 * (1 + abs(want))
        tot += got
    fused = float(np.sum(d.obj_p0 * x[d.obj_col]) + d.obj_const)
    assert abs(fused - tot) <= 1e-12 * (1 + abs(tot))


def test_tape_objective_declared_linear_gives_the_atoms_of_affine():
    x = [ktn.var(j) for j in range(6)]
    e = 2.5 * x[3] - (x[0] - 4.0 * x[5]) / 8.0 + (-x[3]) * 3.0 + 0.1 * (x[1] + x[0]) + 7.0 - x[5] * -0.5
    co, c0 = e.affine()
    o, a = e.tape()
    d = ktn.NLPDescription(6, [0], [], [], [], [], None, None, None, obj_linear=True, obj_kind=L.ROW_TAPE,
                           obj_tape_op=o, obj_tape_arg=a, obj_const=0.25)
    p = ktn.Problem(6, 0, np.zeros(6), np.ones(6), [], [], "Min", d)
    big, offs, info = ktn.fuse_problems([p, p])
    cols, coefs, const = info[0]
    js = sorted(co)
    assert list(cols) == js and [float(v) for v in coefs] == [co[j] for j in js] and const == c0 + 0.25
    np.testing.assert_array_equal(big.d.obj_col, np.concatenate([js, np.asarray(js) + 6]))
    np.testing.assert_array_equal(big.d.obj_p0, np.concatenate([coefs, coefs]))
    assert big.d.obj_const == 2 * (c0 + 0.25)


def test_non_affine_objective_declared_linear_is_refused():
    x = [ktn.var(j) for j in range(3)]
    for e in (x[0] * x[1] + x[2], ktn.exp(x[0]), x[0] / x[1], x[2] ** 2.0):
        o, a = e.tape()
        d = ktn.NLPDescription(3, [0], [], [], [], [], None, None, None, obj_linear=True, obj_kind=L.ROW_TAPE,
                               obj_tape_op=o, obj_tape_arg=a)
        good = expr_problem(ktn.instances.make_instance(n=20, m_nl=3, k=3, seed=1))
        with pytest.raises(ValueError, match="problem 1"):
            ktn.fuse_problems([good, ktn.Problem(3, 0, np.zeros(3), np.ones(3), [], [], "Min", d)])


def test_max_objectives_are_negated_in_and_restored_out():
    inst = ktn.instances.make_instance(n=30, m_nl=4, k=3, seed=11)
    pmin = expr_problem(inst)
    pmax = pmin._replace(sense="Max")
    big, offs, info = ktn.fuse_problems([pmin, pmax])
    d = big.d
    k0 = len(info[0][0])
    np.testing.assert_array_equal(d.obj_p0[k0:], -info[1][1])
    np.testing.assert_array_equal(d.obj_p0[:k0], info[0][1])
    assert d.obj_const == info[0][2] - info[1][2]
    # reported in its own sense: the Max instance's coefficients are its own, not the negated ones
    np.testing.assert_array_equal(info[1][1], info[0][1])
    # FusedBatch reports each instance's objective from objinfo (own sense), checked without a GPU on a fake solution
    x = np.random.default_rng(2).uniform(0, 1, big.num_var)
    vals = [float(np.sum(c * x[offs[k]:offs[k + 1]][j]) + c0) for k, (j, c, c0) in enumerate(info)]
    fused = float(np.sum(d.obj_p0 * x[d.obj_col]) + d.obj_const)
    assert abs(fused - (vals[0] - vals[1])) <= 1e-12 * (1 + abs(fused))


def test_host_rows_and_nonlinear_objectives_are_refused():
    inst = ktn.instances.make_instance(n=20, m_nl=3, k=3, seed=4)
    good = expr_problem(inst)

    class Ev:
        def jac_structure(self): return [0], [0]
        def isconstrlinear(self, i): return False
        def isobjlinear(self): return True
        def eval_g(self, g, x): g[0] = x[0] ** 2
        def eval_jac_g(self, J, x): J[0] = 2 * x[0]
        def eval_f(self, x): return x[0]
        def eval_grad_f(self, g, x): g[0] = 1.0

    host = ktn.Problem(2, 1, np.zeros(2), np.ones(2), [-math.inf], [1.0], "Min", ktn.CallbackNLP(Ev(), 2, 1))
    with pytest.raises(ValueError, match="problem 1"):
        ktn.fuse_problems([good, host])
    v = [ktn.var(0), ktn.var(1)]
    nl = ktn.Problem(2, 1, np.zeros(2), np.ones(2), [-math.inf], [1.0], "Min",
                     ktn.ExprNLP(2, ktn.exp(v[0]) + v[1], [v[0] * v[0] + v[1]]))
    assert not nl.d.obj_linear
    with pytest.raises(ValueError, match="problem 2"):
        ktn.fuse_problems([good, good, nl])


def test_jump_like_model_problem_without_solving():
    M = ktn.Model(None)
    x = M.variables(3, lb=-2.0, ub=2.0)
    M.objective("Max", 2.0 * x[0] - x[2] + 1.0)
    M.constraint(x[0] * x[0] + x[1] * x[1] <= 1.0)
    M.constraint(x[0] + x[2] >= -1.0)
    p = M.problem()
    assert isinstance(p, ktn.Problem) and M.internal_model is None
    assert (p.num_var, p.num_constr, p.sense) == (3, 2, "Max")
    np.testing.assert_array_equal(p.l_var, [-2.0] * 3)
    np.testing.assert_array_equal(p.u_constr, [0.0, math.inf])
    assert list(p.d.row_kind) == [L.ROW_TAPE, L.ROW_SEP]
    big, offs, info = ktn.fuse_problems([p, M.problem()])
    assert list(offs) == [0, 3, 6] and list(big.d.row_kind) == [L.ROW_TAPE, L.ROW_SEP] * 2
    assert list(info[0][0]) == [0, 2] and list(info[0][1]) == [2.0, -1.0] and info[0][2] == 1.0
