"""CPU tier: the supporting-hyperplane option (cut_algo) through every layer that runs without a GPU -- the header, the
library's defaults, the Python and Julia bindings -- and the reference search of tests/esh_ref.py against closed forms and
mpmath roots."""
import math
import os
import re

import mpmath as mp
import numpy as np
import pytest

import esh_ref
import katana_jl_amd as ktn
from katana_jl_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "katana_hip.h")).read()
JL = open(os.path.join(ROOT, "katana.jl_amd", "julia", "KatanaHIP.jl")).read()
NEW = ["cut_algo", "esh_root_iters", "esh_root_tol", "esh_interior_iters"]


def test_header_defines_the_cut_algorithms_and_appends_the_fields():
    assert re.search(r"#define\s+KTN_CUT_KELLEY\s+0\b", HEADER)
    assert re.search(r"#define\s+KTN_CUT_SUPPORTING\s+1\b", HEADER)
    body = HEADER[HEADER.index("typedef struct {\n    double  f_tol;"):HEADER.index("} ktn_params;")]
    fields = re.findall(r"^\s+(?:int32_t|int64_t|double)\s+(\w+);", body, re.M)
    assert fields[-5:] == ["lp_mid_max_var"] + NEW
    for fn in ("ktn_set_interior_point", "ktn_get_interior_point"):
        assert re.search(r"\bint %s\(" % fn, HEADER) and fn in L.PROTOTYPES


def test_library_defaults_of_the_new_fields():
    p = L.KtnParams()
    L.lib().ktn_default_params(p)
    assert (p.cut_algo, p.esh_root_iters, p.esh_root_tol, p.esh_interior_iters) == (0, 20, 0.1, 50)
    assert L.lib().ktn_sizeof_params() == __import__("ctypes").sizeof(L.KtnParams)
    assert (L.CUT_KELLEY, L.CUT_SUPPORTING) == (0, 1)


def test_python_and_julia_mirrors_carry_the_fields():
    py = [n for n, _ in L.KtnParams._fields_]
    assert py[-5:] == ["lp_mid_max_var"] + NEW
    jl = JL[JL.index("struct KtnParams"):]
    jl = jl[:jl.index("\nend")]
    assert "cut_algo::Int32; esh_root_iters::Int32; esh_root_tol::Cdouble; esh_interior_iters::Int32" in jl


def test_solver_maps_the_cut_algorithm_names():
    assert ktn.KatanaSolver().gpu_options["cut_algo"] == L.CUT_KELLEY
    assert ktn.KatanaSolver(cut_algo="kelley").gpu_options["cut_algo"] == L.CUT_KELLEY
    assert ktn.KatanaSolver(cut_algo="supporting_hyperplane").gpu_options["cut_algo"] == L.CUT_SUPPORTING
    assert ktn.KatanaSolver(cut_algo=1).gpu_options["cut_algo"] == L.CUT_SUPPORTING
    with pytest.raises(ValueError):
        ktn.KatanaSolver(cut_algo="newton")
    # jump_like.Model takes the solver unchanged
    M = ktn.Model(solver=ktn.KatanaSolver(cut_algo="supporting_hyperplane"))
    assert M.solver.gpu_options["cut_algo"] == 1


def test_julia_binding_passes_the_fields_and_defines_the_marker():
    assert re.search(r"export .*\bsupporting_hyperplane_cut\b", JL)
    assert re.search(r"^supporting_hyperplane_cut\(sep, a, b, i\) =", JL, re.M)
    assert "sep.algo === supporting_hyperplane_cut" in JL and "KTN_CUT_SUPPORTING" in JL
    call = JL[JL.index("prm = KtnParams("):]
    call = call[:call.index(")\n")]
    assert "cut_algo_of(s), d.esh_root_iters, d.esh_root_tol, d.esh_interior_iters" in call
    # as many arguments as the struct has fields
    nfields = len(re.findall(r"(\w+)::", JL[JL.index("struct KtnParams"):JL.index("\nend", JL.index("struct KtnParams"))]))
    assert nfields == len(L.KtnParams._fields_)


# ---- esh_ref against closed forms and mpmath ------------------------------------------------------------------
def _quad_row(rng, k, lin=True):
    cols = np.arange(k)
    kinds = [esh_ref.QUAD] * k + ([esh_ref.LIN] if lin else [])
    if lin:
        cols = np.append(cols, k)
    p0 = list(rng.uniform(0.5, 2.0, k)) + ([rng.uniform(-1, 1)] if lin else [])
    p1 = list(rng.uniform(-1, 1, k)) + ([0.0] if lin else [])
    return esh_ref.SepRow(cols, kinds, p0, p1, 0.0)


@pytest.mark.parametrize("seed", range(5))
def test_search_on_quadratic_rows_meets_the_closed_form_root(seed):
    rng = np.random.default_rng(seed)
    row = _quad_row(rng, 6)
    n = len(row.cols)
    xi = np.array([row.p1[j] for j in range(6)] + [0.0])           # the minimiser of the quadratic part
    g0 = row.eval(xi)[0]
    bound = g0 + 1.0
    xs = xi + rng.normal(size=n) * 3.0
    assert esh_ref.phi(row, xi, xs, 1, bound, 1.0)[0] > 1e-6
    lam, passes = esh_ref.root_search(row, xi, xs, 1, bound, 1e-7)
    exact = esh_ref.quad_root(row, xi, xs, 1, bound)
    assert lam is not None and passes <= 20
    assert 0.0 <= esh_ref.phi(row, xi, xs, 1, bound, lam)[0] <= 1e-7
    assert lam >= float(exact) - 1e-15 and lam - float(exact) <= 1e-6
    assert abs(esh_ref.exact_root(row, xi, xs, 1, bound) - exact) <= mp.mpf(10) ** -40


@pytest.mark.parametrize("kind", [esh_ref.LIN, esh_ref.QUAD, esh_ref.EXP, esh_ref.NEGLOG])
@pytest.mark.parametrize("side", [1, -1])
def test_search_for_every_atom_kind_against_the_mpmath_root(kind, side):
    rng = np.random.default_rng(kind * 7 + (side > 0))
    k = 5
    cols = np.arange(k)
    if kind == esh_ref.NEGLOG:
        p0, p1 = rng.uniform(0.5, 2, k), rng.uniform(1.0, 2.0, k)
    elif kind == esh_ref.EXP:
        p0, p1 = rng.uniform(0.5, 2, k), rng.uniform(-1, 1, k)
    else:
        p0, p1 = rng.uniform(0.5, 2, k), rng.uniform(-1, 1, k)
    # convex rows on the upper side, concave (negated) rows on the lower side
    row = esh_ref.SepRow(cols, [kind] * k, list(side * p0), list(p1), 0.0)
    if kind == esh_ref.LIN:
        row = esh_ref.SepRow(np.arange(k + 1), [esh_ref.LIN] * k + [esh_ref.QUAD], list(side * p0) + [side * 1.0],
                             list(p1) + [0.0], 0.0)
    n = len(row.cols)
    xi = np.zeros(n)
    xs = rng.uniform(0.2, 0.9, n)
    g0, g1 = row.eval(xi)[0], row.eval(xs)[0]
    if side * (g1 - g0) < 0:
        xi, xs, g0, g1 = xs, xi, g1, g0
    bound = g0 + 0.3 * (g1 - g0)                                 # x_int inside, x* beyond
    assert side * (g0 - bound) < -1e-5 and side * (g1 - bound) > 1e-6
    lam, _ = esh_ref.root_search(row, xi, xs, side, bound, 1e-7)
    exact = float(esh_ref.exact_root(row, xi, xs, side, bound))
    assert lam is not None and lam >= exact - 1e-14
    f = esh_ref.phi(row, xi, xs, side, bound, lam)[0]
    assert 0.0 <= f <= 1e-7
    # the cut at x_b: valid for the row (convexity), cuts x* off, keeps x_int
    coef, const = esh_ref.cut_at(row, xi, xs, side, bound, lam)
    assert side * (coef @ xs + const - bound) > 0 and side * (coef @ xi + const - bound) < 0
    for t in np.linspace(0, 1, 7):
        y = rng.uniform(0.0, 1.0, n)
        gy = row.eval(y)[0]
        assert side * (coef @ y + const) <= side * gy + 1e-12 * (1 + abs(gy))


def test_search_on_an_expression_row_matches_its_separable_twin():
    rng = np.random.default_rng(11)
    row = _quad_row(rng, 3, lin=False)
    expr = ["+"] + [["*", float(row.p0[j]), ["^", ["-", ["var", j], float(row.p1[j])], 2]] for j in range(3)]
    srow = esh_ref.SexprRow(expr, row.cols)
    xi = np.array(row.p1, dtype=float)
    xs = xi + np.array([1.0, -2.0, 0.5])
    bound = row.eval(xi)[0] + 0.5
    lam_a, _ = esh_ref.root_search(row, xi, xs, 1, bound, 1e-7)
    lam_b, _ = esh_ref.root_search(srow, xi, xs, 1, bound, 1e-7)
    assert abs(lam_a - lam_b) <= 1e-12
    assert abs(lam_a - float(esh_ref.quad_root(row, xi, xs, 1, bound))) <= 1e-6


def test_a_row_whose_search_finds_no_point_below_one_keeps_kelley():
    row = esh_ref.SepRow([0], [esh_ref.QUAD], [1.0], [0.0], 0.0)
    lam, passes = esh_ref.root_search(row, np.array([0.0]), np.array([1.0]), 1, 0.99999995, 1e-7)
    # phi(1) = 5e-8 <= tol: the point x* already lies within the tolerance band -> Kelley's cut
    assert lam is None and passes == 1


def test_lambda_is_recovered_from_a_coefficient():
    for kind, p0, p1 in ((esh_ref.QUAD, 1.5, 0.2), (esh_ref.EXP, 0.7, 0.9), (esh_ref.NEGLOG, 1.2, 1.5)):
        x0, x1, lam = 0.1, 0.8, 0.37
        _, der = esh_ref.atom(kind, p0, p1, x0 + lam * (x1 - x0))
        assert abs(esh_ref.lambda_from_coefficient(kind, p0, p1, der, x0, x1) - lam) <= 1e-12
