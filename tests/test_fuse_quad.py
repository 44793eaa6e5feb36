"""CPU tier: nlp.fuse_problems on KTN_ROW_QUAD rows and objectives -- Q segments concatenated and shifted, the per-instance
epigraph of a quadratic objective and its interval bound, and batches without QUAD rows fused exactly as before."""
import math

import numpy as np
import pytest

import katana_jl_amd as ktn
import fuse_quad_cases as FQ
from fuse_helpers import expr_problem, separable_problem

L = ktn._lib
make = ktn.instances.make_instance


def quad_inst(seed, **kw):
    return make(**dict(dict(n=60, m_nl=6, k=5, family="quad", seed=seed), **kw))


def test_quad_rows_of_a_mixed_batch_are_concatenated_and_shifted():
    insts = [quad_inst(1), make(n=40, m_nl=5, k=4, family="explog", seed=2), make(n=30, m_nl=4, k=3, family="explog", seed=3),
             quad_inst(4, n=50)]
    probs = [FQ.quadnlp_problem(insts[0]), expr_problem(insts[1]), separable_problem(insts[2]), FQ.quad_rows_problem(insts[3])]
    assert probs[0].d.obj_kind == L.ROW_QUAD and probs[0].d.obj_linear and np.all(probs[0].d.row_kind == L.ROW_QUAD)
    assert probs[1].d.quad_ptr is None and probs[2].d.quad_ptr is None
    big, offs, info = ktn.fuse_problems(probs, allow_quad=True)
    d = big.d
    assert list(offs) == [0, 60, 100, 130, 180]
    nnz = len(d.col)
    assert len(d.quad_ptr) == nnz + 1 and d.quad_ptr[0] == 0 and np.all(np.diff(d.quad_ptr) >= 0)
    assert d.quad_ptr[-1] == len(d.quad_col) == len(d.quad_val) == len(probs[0].d.quad_val) + len(probs[3].d.quad_val)
    seg = np.diff(d.quad_ptr)
    row_of = np.repeat(np.arange(d.num_constr), np.diff(d.rowptr))
    assert np.all(seg[d.row_kind[row_of] != L.ROW_QUAD] == 0)
    assert np.all(seg[d.row_linear[row_of] == 1] == 0)                      # QUAD rows declared linear: empty Q
    assert np.any(seg > 0)
    for i in np.flatnonzero(d.row_kind == L.ROW_QUAD):                      # what ktn_loadproblem will demand
        b, e = d.rowptr[i], d.rowptr[i + 1]
        assert np.all(np.isin(d.quad_col[d.quad_ptr[b]:d.quad_ptr[e]], d.col[b:e]))
    # the linear objective of kind QUAD entered as LIN atoms
    np.testing.assert_array_equal(info[0][0], probs[0].d.obj_col)
    np.testing.assert_array_equal(info[0][1], probs[0].d.obj_p0)
    assert d.obj_kind == L.ROW_SEP and d.obj_linear and np.all(d.obj_atom_kind == L.ATOM_LIN)
    # every fused QUAD row against the instance's own row at a random point, float64 numpy from the arrays
    x = np.random.default_rng(7).uniform(-1.0, 1.0, big.num_var)
    fused = FQ.quad_row_values(d, x)
    row0, seen = 0, 0
    for k, p in enumerate(probs):
        if p.d.quad_ptr is not None:
            for i, g in FQ.quad_row_values(p.d, x[offs[k]:offs[k + 1]]).items():
                gf = fused[row0 + i]
                assert abs(gf - g) <= 1e-13 * (1.0 + abs(g)), (k, i, gf, g)
                seen += 1
        row0 += p.d.num_constr
    assert seen == len(fused) == insts[0].num_constr + insts[3].m_nl


def test_quadratic_objective_becomes_a_per_instance_epigraph():
    insts = [make(n=40, m_nl=5, k=4, family="explog", objective="quad", seed=20 + s) for s in range(3)]
    probs = [FQ.quad_objective_problem(insts[0], ncross=6), separable_problem(make(n=30, m_nl=4, k=3, family="explog", seed=5)),
             FQ.quad_objective_problem(insts[2], ncross=6, sense="Max")]
    assert not probs[0].d.obj_linear and probs[0].d.obj_kind == L.ROW_QUAD
    big, offs, info = ktn.fuse_problems(probs, allow_quad=True)
    d = big.d
    assert list(offs) == [0, 41, 71, 112]                                   # column offsets count t
    assert big.num_var == 112 and big.num_constr == sum(p.num_constr for p in probs) + 2
    rng = np.random.default_rng(3)
    row0 = 0
    for k, p in enumerate(probs):
        n_k, o = p.num_var, offs[k]
        if k == 1:
            assert offs[k + 1] - o == n_k
            row0 += p.num_constr
            continue
        sg = -1.0 if p.sense == "Max" else 1.0
        r = row0 + p.num_constr                                             # the instance's last row
        b, e = d.rowptr[r], d.rowptr[r + 1]
        assert d.row_kind[r] == L.ROW_QUAD and d.row_linear[r] == 0 and d.rconst[r] == 0.0
        assert big.l_constr[r] == -math.inf and big.u_constr[r] == 0.0
        # last entry t: coefficient -1, empty segment
        assert d.col[e - 1] == o + n_k and d.p0[e - 1] == -1.0 and d.quad_ptr[e] == d.quad_ptr[e - 1]
        np.testing.assert_array_equal(d.col[b:e - 1], p.d.obj_col + o)
        np.testing.assert_array_equal(d.p0[b:e - 1], sg * p.d.obj_p0)        # a :Max instance enters negated
        np.testing.assert_array_equal(d.quad_val[d.quad_ptr[b]:d.quad_ptr[e]], sg * p.d.obj_quad_val)
        np.testing.assert_array_equal(d.quad_col[d.quad_ptr[b]:d.quad_ptr[e]], p.d.obj_quad_col + o)
        np.testing.assert_array_equal(np.diff(d.quad_ptr[b:e]), np.diff(p.d.obj_quad_ptr))
        # R by the formula, entry by entry
        m = np.maximum(np.abs(p.l_var), np.abs(p.u_var))
        R = sum(abs(a) * m[j] for j, a in zip(p.d.obj_col, p.d.obj_p0))
        for ei, j in enumerate(p.d.obj_col):
            for q in range(p.d.obj_quad_ptr[ei], p.d.obj_quad_ptr[ei + 1]):
                R += 0.5 * abs(p.d.obj_quad_val[q]) * m[j] * m[p.d.obj_quad_col[q]]
        assert big.l_var[o + n_k] == -big.u_var[o + n_k] and abs(big.u_var[o + n_k] - R) <= 1e-12 * R and R > 0
        # objinfo contract: ([n_k], [+-1], const); the fused objective carries +1 on t
        cols, coefs, c0 = info[k]
        assert list(cols) == [n_k] and list(coefs) == [sg] and c0 == p.d.obj_const
        at = np.flatnonzero(d.obj_col == o + n_k)
        assert len(at) == 1 and d.obj_p0[at[0]] == 1.0
        # with t at the (negated) objective value the row is tight and the instance reports its own objective
        x = rng.uniform(-1.0, 1.0, n_k)
        f = FQ.quad_objective_value(p.d, x)
        assert abs(f) <= R
        xt = np.zeros(big.num_var)
        xt[o:o + n_k] = x
        xt[o + n_k] = sg * (f - p.d.obj_const)
        g = FQ.quad_row_values(d, xt)[r]
        assert abs(g) <= 1e-12 * (1.0 + abs(f))
        assert abs(float(np.sum(coefs * xt[o:offs[k + 1]][cols]) + c0) - f) <= 1e-12 * (1.0 + abs(f))
        row0 = r + 1
    assert abs(d.obj_const - (probs[0].d.obj_const + probs[1].d.obj_const - probs[2].d.obj_const)) <= 1e-12 * abs(probs[0].d.obj_const)


def test_quadratic_objective_needs_finite_bounds_and_other_nonlinear_objectives_are_refused():
    inst = make(n=40, m_nl=5, k=4, family="explog", objective="quad", seed=31)
    good = FQ.quad_objective_problem(inst, ncross=6)
    u = np.array(good.u_var, dtype=np.float64)
    u[7] = math.inf
    with pytest.raises(ValueError, match=r"problem 1.*column 7"):
        ktn.fuse_problems([good, good._replace(u_var=u)], allow_quad=True)
    # a nonlinear SEPARABLE objective (the same instance before it was restated) still has no epigraph here
    with pytest.raises(ValueError, match="problem 1"):
        ktn.fuse_problems([good, separable_problem(inst)], allow_quad=True)


def test_quad_models_are_fused_on_request_only():
    p = FQ.quad_rows_problem(quad_inst(6))
    with pytest.raises(ValueError, match="problem 1.*allow_quad"):
        ktn.fuse_problems([separable_problem(quad_inst(7)), p])
    big, offs, _ = ktn.fuse_problems([p, p], allow_quad=True)
    assert list(offs) == [0, 60, 120] and big.d.quad_ptr[-1] == 2 * p.d.quad_ptr[-1]


def test_a_batch_without_quad_rows_fuses_as_before():
    insts = [make(n=30, m_nl=4, k=3, family="explog", seed=41), make(n=20, m_nl=3, k=3, family="explog", seed=42)]
    probs = [expr_problem(insts[0]), separable_problem(insts[1])._replace(sense="Max")]
    big, offs, info = ktn.fuse_problems(probs)
    d, (a, b) = big.d, [p.d for p in probs]
    assert d.quad_ptr is None and d.quad_col is None and d.quad_val is None and d.obj_quad_ptr is None
    assert list(offs) == [0, 30, 50]
    cat = np.concatenate
    np.testing.assert_array_equal(d.rowptr, cat([a.rowptr, b.rowptr[1:] + len(a.col)]))
    np.testing.assert_array_equal(d.col, cat([a.col, b.col + 30]))
    for attr in ("row_kind", "row_linear", "rconst", "atom_kind", "p0", "p1", "tape_op"):
        np.testing.assert_array_equal(getattr(d, attr), cat([getattr(a, attr), getattr(b, attr)]))
    np.testing.assert_array_equal(d.tape_ptr, cat([a.tape_ptr, b.tape_ptr[1:] + len(a.tape_op)]))
    np.testing.assert_array_equal(d.tape_arg, cat([a.tape_arg, b.tape_arg]))       # (b has no tape: nothing to shift)
    np.testing.assert_array_equal(d.obj_col, cat([info[0][0], info[1][0] + 30]))
    np.testing.assert_array_equal(d.obj_p0, cat([info[0][1], -info[1][1]]))
    assert d.obj_const == info[0][2] - info[1][2] and d.obj_kind == L.ROW_SEP and d.obj_linear
    for attr in ("l_var", "u_var", "l_constr", "u_constr"):
        np.testing.assert_array_equal(getattr(big, attr), cat([getattr(p, attr) for p in probs]))
    assert (big.num_var, big.num_constr, big.sense) == (50, a.num_constr + b.num_constr, "Min")
