"""CPU tier: the front end of the KTN_ROW_QUAD rows (no device): MathProgBase's two quadratic conventions against dense numpy,
the structure nlp.QuadNLP builds, the unambiguity of the GPU cases' violated sets (tests/quad_cases.py), and the paths that
refuse such rows."""
import math

import numpy as np
import pytest
from mpmath import mp, mpf

import katana_jl_amd as ktn
from katana_jl_amd.distributed import shard_rows
import quad_cases as QC
import quad_ref as Q

L = ktn._lib


def triplet_sets(rng, n):
    """random triplets: with duplicates, with a pair given in both orders, diagonal-only, empty"""
    k = 3 * n
    r, c = rng.integers(0, n, k), rng.integers(0, n, k)
    v = rng.uniform(-2.0, 2.0, k)
    yield "random with duplicates", np.concatenate([r, r[:5]]), np.concatenate([c, c[:5]]), np.concatenate([v, v[:5] * 0.5])
    yield "a pair in both orders", np.array([0, 1, 2, 1]), np.array([1, 0, 2, 2]), np.array([1.5, -0.25, 2.0, 0.75])
    yield "diagonal only", np.arange(n), np.arange(n), rng.uniform(0.5, 2.0, n)
    yield "empty", np.zeros(0, dtype=int), np.zeros(0, dtype=int), np.zeros(0)


@pytest.mark.parametrize("n", [3, 7])
def test_the_two_mathprogbase_conventions_against_dense_numpy(n):
    rng = np.random.default_rng(n)
    for what, r, c, v in triplet_sets(rng, n):
        _, T = Q.dense_forms(n, [], [], r, c, v)
        for conv, M in (("objective", T + T.T - np.diag(np.diag(T))), ("constraint", T + T.T)):
            er, ec, ev = ktn.quad_triplets_to_engine(r, c, v, conv)
            _, E = Q.dense_forms(n, [], [], er, ec, ev)
            assert np.array_equal(E, E.T), (what, conv)
            assert np.allclose(E, M, rtol=0, atol=1e-14), (what, conv)
            for _ in range(3):
                x = rng.uniform(-1.0, 1.0, n)
                want = (0.5 * (np.diag(T) @ (x * x)) + x @ (T - np.diag(np.diag(T))) @ x) if conv == "objective" else x @ T @ x
                assert abs(0.5 * x @ E @ x - want) <= 1e-12 * (1.0 + np.abs(T).sum()), (what, conv)
    with pytest.raises(ValueError):
        ktn.quad_triplets_to_engine([0], [0], [1.0], "other")


def test_quadnlp_structure_sorted_union_symmetric_segments_and_empty_segments():
    d = ktn.QuadNLP(6, [0.0, 1.0, 0.0, 0.0, 0.0, 2.0], 3.0, ([4, 1, 1, 4, 1], [4, 1, 4, 1, 1], [2.0, 3.0, 0.5, 0.5, 1.0]),
                    [([5, 0, 5], [1.0, 2.0, 0.25], [], [], [], 1.0),
                     ([2], [1.0], [3, 1, 3, 1], [3, 1, 1, 3], [1.0, 1.0, 0.2, 0.2], 0.0),
                     ([], [], [], [], [], -1.0)])
    assert d.rowptr.tolist() == [0, 2, 5, 5] and d.col.tolist() == [0, 5, 1, 2, 3]
    assert d.p0.tolist() == [2.0, 1.25, 0.0, 1.0, 0.0] and d.rconst.tolist() == [1.0, 0.0, -1.0]
    assert d.row_kind.tolist() == [L.ROW_QUAD] * 3 and d.row_linear.tolist() == [1, 0, 1]
    assert d.quad_ptr.tolist() == [0, 0, 0, 2, 2, 4]                     # column 2 is in the linear part only: an empty segment
    assert d.quad_col.tolist() == [1, 3, 1, 3] and d.quad_val.tolist() == [1.0, 0.2, 0.2, 1.0]
    assert d.obj_kind == L.ROW_QUAD and not d.obj_linear and d.obj_const == 3.0
    assert d.obj_col.tolist() == [1, 4, 5] and d.obj_p0.tolist() == [1.0, 0.0, 2.0]
    assert d.obj_quad_ptr.tolist() == [0, 2, 4, 4] and d.obj_quad_col.tolist() == [1, 4, 1, 4]
    assert d.obj_quad_val.tolist() == [4.0, 0.5, 0.5, 2.0]               # duplicates summed
    c = d.c_struct()
    assert c.quad_ptr[5] == 4 and c.obj_quad_ptr[3] == 4 and c.obj_kind == L.ROW_QUAD
    lin = ktn.QuadNLP(3, ([2, 0], [1.0, -1.0]), 0.0, None, [])
    assert lin.obj_linear and lin.obj_col.tolist() == [0, 2] and lin.obj_quad_ptr.tolist() == [0, 0, 0]
    plain = ktn.ExprNLP(2, ktn.var(0), [ktn.var(0) * ktn.var(1)])
    assert plain.quad_ptr is None and not plain.c_struct().quad_ptr and not plain.c_struct().obj_quad_ptr
    with pytest.raises(ValueError):
        ktn.QuadNLP(3, [0.0] * 3, 0.0, None, [([3], [1.0], [], [], [], 0.0)])


def test_the_mixed_case_holds_what_the_kernels_have_to_meet():
    C = QC.mixed_case()
    assert C.kind[0] == L.ROW_QUAD and C.kind[-1] == L.ROW_QUAD and set(C.kind) == {L.ROW_SEP, L.ROW_TAPE, L.ROW_QUAD}
    seglens = set()
    rowlens = set()
    for i, lay in C.layouts.items():
        seglens |= set(np.diff(lay[2]).tolist())
        rowlens.add(len(lay[0]))
        E = np.zeros((C.n, C.n))
        for e, c in enumerate(lay[0]):
            E[c, lay[3][lay[2][e]:lay[2][e + 1]]] = lay[4][lay[2][e]:lay[2][e + 1]]
        assert np.array_equal(E, E.T), ("symmetric segments", i)
    for G in QC.GROUPS:
        assert {0, 1, G - 1, G, G + 1, 2 * G + 1} <= seglens, G
    assert {1, 65, 257, 70} <= rowlens and 4900 in [len(lay[4]) for lay in C.layouts.values()]
    quad = np.flatnonzero(C.kind == L.ROW_QUAD)
    assert any(C.d.row_linear[i] and len(C.layouts[i][4]) == 0 for i in quad)
    assert len(C.objective[1]) < C.n                                                     # the epigraph row has implicit zeros
    n_all, n_nl = len(quad) + 1, int((C.d.row_linear[quad] == 0).sum()) + 1             # (+ 1: the epigraph row)
    for G2 in QC.GROUPS:                                                                 # rows per 256-thread block of k_quad_stats
        assert n_all % (256 // G2) != 0 and n_nl % (256 // G2) != 0


def test_every_kernel_case_has_an_unambiguous_violated_set():
    C = QC.mixed_case()
    with mp.workprec(Q.PREC):
        for i, R in C.ref.items():
            if C.d.row_linear[i]:
                continue
            tag = C.tags[i]
            g = float(R.g)
            if tag.startswith("thr"):
                assert mpf(g) == R.g, "threshold rows are exact"
                want = {"thr_at_ub": C.ub[i] + C.f_tol, "thr_above_ub": np.nextafter(C.ub[i] + C.f_tol, math.inf),
                        "thr_at_lb": C.lb[i] - C.f_tol, "thr_below_lb": np.nextafter(C.lb[i] - C.f_tol, -math.inf)}[tag]
                assert g == want, (i, tag, g, want)
                assert bool(C.violated[i]) == (tag in ("thr_above_ub", "thr_below_lb"))
                continue
            for thr in (C.ub[i] + C.f_tol, C.lb[i] - C.f_tol):
                if math.isfinite(thr):
                    assert abs(R.g - mpf(thr)) >= 1000 * R.e_g, (i, float(R.g), thr, float(R.e_g))
            assert bool(C.violated[i]) == (not (g >= C.lb[i] - C.f_tol and g <= C.ub[i] + C.f_tol))
    nl = np.flatnonzero(C.d.row_linear == 0)
    assert C.violated[nl].any() and (~C.violated[nl]).any()
    assert C.violated[np.flatnonzero((C.kind == L.ROW_QUAD) & (C.d.row_linear == 0))].sum() >= 5


def test_reference_of_a_small_row_by_hand():
    # g = 1 + 2 x0 + 1/2 (x0 (3 x0 + x1) + x1 (x0 + 5 x1)) at x = (2, -1):  1 + 4 + 1/2 (2 * 5 + (-1) * (-3)) = 11.5
    cols, a, ptr, sc, sv = ktn.nlp._quad_row(2, [0], [2.0], [0, 0, 1, 1], [0, 1, 0, 1], [3.0, 1.0, 1.0, 5.0])
    R = Q.row_ref_mp(cols, a, ptr, sc, sv, 1.0, [2.0, -1.0])
    assert float(R.g) == 11.5 and [float(v) for v in R.der] == [7.0, -3.0] and float(R.b) == 11.5 - (14.0 + 3.0)
    assert 0 < R.e_g < 1e-13 and 0 < R.e_b < 1e-13


def test_fuse_problems_and_shard_rows_refuse_quad_rows():
    C = QC.ellipsoid(4)
    p = QC.ellipsoid_quad(C)
    with pytest.raises(ValueError, match="QUAD"):
        ktn.fuse_problems([p, p])
    inst = ktn.instances.make_instance(n=40, m_nl=8, k=4, family="explog", seed=1)
    inst.quad_ptr = np.zeros(len(inst.col) + 1, dtype=np.int64)
    with pytest.raises(ValueError, match="QUAD"):
        shard_rows(inst, 0, 2)


def test_linear_quadratic_model_is_a_model_class_with_the_lpqp_surface():
    M = ktn.LinearQuadraticModel
    assert isinstance(M, type) and issubclass(M, ktn.KatanaNonlinearModel)
    for name in ("loadproblem", "setquadobj", "addquadconstr", "optimize", "getobjval", "getsolution", "status"):
        assert callable(getattr(M, name))
