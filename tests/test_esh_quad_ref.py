"""CPU tier: the case of tests/esh_quad_cases.py meets its own conditions in mpmath, the closed form of csrc/esh_quad.hpp in float64
meets the mpmath root within the reference's bound, and KTN_CUT_SUPPORTING_QUAD is stated in every layer that runs without a GPU."""
import os
import re

import numpy as np
import pytest
from mpmath import mp, mpf

import esh_quad_cases as EC
import esh_quad_ref as ER
import katana_jl_amd as ktn
import quad_ref as Q

L = ktn._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "katana_hip.h")).read()
JL = open(os.path.join(ROOT, "katana.jl_amd", "julia", "KatanaHIP.jl")).read()


def _ref(C, i, lam):
    return ER.cut_ref_mp(C.layouts[i], C.rows[i][6], C.xi, C.x, C.sides[i], EC.bound_of(C, i), lam, EC.TAU)


def test_the_case_meets_its_own_conditions():
    C = EC.case()
    assert [len(C.layouts[i][0]) for i in C.part] == [3, 1, 12, 65, 9, 257, 70]
    assert sorted(set(C.tags)) == ["equality", "indefinite", "part", "satisfied", "sep", "shallow", "tape", "two_sided"]
    assert sum(1 for i in C.part if C.sides[i] < 0) == 1
    viol_kinds = {C.rows[i][0] for i in range(C.m) if C.violated[i]}
    sat_kinds = {C.rows[i][0] for i in range(C.m) if not C.violated[i]}
    assert viol_kinds == sat_kinds == {"sep", "tape", "quad"}
    with mp.workprec(Q.PREC):
        for i in C.part + [i for i, t in enumerate(C.tags) if t in ("two_sided", "equality", "indefinite")]:
            s, b = C.sides[i], mpf(float(EC.bound_of(C, i)))
            assert s * (C.ref_int[i].g - b) <= -0.25 and s * (C.ref[i].g - b) >= 0.25, (i, C.tags[i])
        i = C.tags.index("shallow")
        margin = mpf(float(C.ub[i])) - C.ref_int[i].g
        assert 0 < margin and margin + C.ref_int[i].e_g < EC.DELTA and C.ref[i].g - mpf(float(C.ub[i])) >= 0.25
        i = C.tags.index("indefinite")
        R = _ref(C, i, 0.5)
        assert C.sides[i] * R.q < -R.e_q, (float(R.q), float(R.e_q))               # negative by more than its bound: never moved


def test_closed_form_in_float64_meets_the_mpmath_root_within_the_bound():
    C = EC.case()
    for i in C.part:
        lam = ER.closed_form_f64(C.layouts[i], C.rows[i][6], C.xi, C.x, C.sides[i], EC.bound_of(C, i), EC.TAU)
        assert lam is not None and 0.0 < lam < 1.0, i
        R = _ref(C, i, lam)
        worst = max(R.bounds())
        assert worst <= EC.TAU / 4, (i, worst)                                      # every bound of the reference, at this lambda
        with mp.workprec(Q.PREC):
            assert abs(mpf(lam) - R.lam_root) <= R.e_lam, (i, lam, float(R.lam_root), float(R.e_lam))
            assert 0 <= R.phi <= EC.TAU, (i, float(R.phi))
            assert abs(R.phi - mpf(EC.TAU) / 2) <= R.e_phi, (i, float(R.phi), float(R.e_phi))
    for tag in ("indefinite",):
        i = C.tags.index(tag)
        assert ER.closed_form_f64(C.layouts[i], C.rows[i][6], C.xi, C.x, 1, C.ub[i], EC.TAU) is None


def test_the_interpolated_gradient_is_the_gradient_at_the_point():
    """grad g is affine: the reference's grad g(x_b), evaluated from Q at x_b, is the interpolation the kernel forms"""
    C = EC.case()
    i = C.part[2]
    R = _ref(C, i, 0.375)
    with mp.workprec(Q.PREC):
        for e in range(R.k):
            want = C.ref_int[i].der[e] + mpf(0.375) * (C.ref[i].der[e] - C.ref_int[i].der[e])
            assert abs(R.der[e] - want) <= mpf(2) ** -150
        assert abs(R.g - (C.ref[i].g - mpf(0.625) * R.P1 + mpf(0.625) ** 2 * R.q / 2)) <= mpf(2) ** -150


def test_header_python_and_julia_state_the_new_code():
    assert re.search(r"#define\s+KTN_CUT_SUPPORTING_QUAD\s+2\b", HEADER)
    assert '"esh_quad_rows"' in HEADER
    assert L.CUT_SUPPORTING_QUAD == 2
    assert ktn.KatanaSolver(cut_algo="supporting_hyperplane_quad").gpu_options["cut_algo"] == 2
    assert ktn.solver.CUT_ALGOS["supporting_hyperplane_quad"] == 2
    assert ktn.KatanaSolver(cut_algo=2).gpu_options["cut_algo"] == 2
    with pytest.raises(ValueError):
        ktn.KatanaSolver(cut_algo="newton")
    assert re.search(r"const KTN_CUT_SUPPORTING_QUAD\s*=\s*Int32\(2\)", JL)
    assert re.search(r"export .*\bsupporting_hyperplane_quad_cut\b", JL)
    assert re.search(r"^supporting_hyperplane_quad_cut\(sep, a, b, i\) =", JL, re.M)
    body = JL[JL.index("function cut_algo_of(s)"):]
    body = body[:body.index("\nend")]
    assert "sep.algo === supporting_hyperplane_quad_cut" in body and "KTN_CUT_SUPPORTING_QUAD" in body


def test_linear_quadratic_model_keeps_and_clears_a_pending_interior_point():
    """on the Python object, without a handle: before optimize() nothing is loaded, so the point waits on the object"""
    m = ktn.LinearQuadraticModel.__new__(ktn.LinearQuadraticModel)
    m._lq = dict(n=2, dirty=True)
    m._xint_pending = None
    src = [0.25, -0.5]
    m.set_interior_point(src)
    assert np.array_equal(m._xint_pending, [0.25, -0.5])
    src[0] = 9.0
    assert m._xint_pending[0] == 0.25                                             # (a copy: the caller's array may change)
    with pytest.raises(ValueError):
        m.set_interior_point([0.0, 0.0, 0.0])
    m.set_interior_point(None)
    assert m._xint_pending is None
