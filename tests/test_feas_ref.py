"""CPU tier: the cases of tests/feas_cases.py say what they are meant to say, so that the device tests (tests/test_gpu_feasible_point.py)
cannot hide behind a tie or a row that was never searched, and the float64 reference search of tests/feas_ref.py does what
include/katana_hip.h states."""
import math

import numpy as np
import pytest
from mpmath import mp, mpf

import feas_cases as FC
import feas_ref as FR


def _cases():
    out = [("sep%d" % G, lambda G=G: FC.sep_case(G)) for G in FC.GROUPS]
    out += [("tape1", lambda: FC.tape_case(1)), ("tape65", lambda: FC.tape_case(65)), ("quad", FC.quad_case),
            ("indefinite", lambda: FC.quad_fallback_case("indefinite"))]
    return out


def _searched(C):
    """the float64 reference search of every taking-part row: {row: (lambda, converged, passes)}"""
    return {i: FR.search(FR.phi_f64(C.d, i, C.xi, C.xs, C.sig[i], C.bnd[i]), FC.TAU, FC.ITERS) for i in C.part}


@pytest.mark.parametrize("name,make", _cases(), ids=[c[0] for c in _cases()])
def test_cases_are_unambiguous_and_the_reference_search_converges(name, make):
    C = FC.classify(make())
    assert C.part and C.search, name
    S = _searched(C)
    with mp.workprec(FR.PREC):
        for i in C.part:
            f0, e0 = FR.phi_exact(C.d, i, C.xi, C.xs, C.sig[i], C.bnd[i], 0.0)
            assert f0 < -10 * FC.F_TOL - e0, (name, i, float(f0))               # x_in is well inside every row
            lam, conv, passes = S[i]
            f, e = FR.phi_exact(C.d, i, C.xi, C.xs, C.sig[i], C.bnd[i], lam)
            assert f <= e, (name, i, lam, float(f))                             # valid whether converged or not
            if i in C.onepass:
                assert lam == 1.0 and conv and passes == 1, (name, i)
            elif i not in C.loose:
                assert conv and passes <= FC.ITERS and 0.0 < lam < 1.0, (name, i, lam, conv, passes)
                assert f >= -FC.TAU - e, (name, i, float(f))
            else:
                assert 0.0 <= lam < 1.0 and math.isfinite(lam), (name, i, lam)
        # the blocking row: its exact boundary point lies below every other row's by more than 10 tau / phi'
        order = sorted(C.part, key=lambda i: S[i][0])
        first = order[0]
        assert first in C.search
        lb0 = FR.lambda_bar(C.d, first, C.xi, C.xs, C.sig[first], C.bnd[first])
        dphi = FR.phi_f64(C.d, first, C.xi, C.xs, C.sig[first], C.bnd[first])(float(lb0))[1]
        assert dphi > 0
        if len(order) > 1:
            second = order[1]
            lb1 = FR.lambda_bar(C.d, second, C.xi, C.xs, C.sig[second], C.bnd[second])
            assert lb1 - lb0 > 10 * FC.TAU / dphi, (name, first, second, float(lb0), float(lb1))
        assert abs(mpf(S[first][0]) - lb0) <= 2 * FC.TAU / dphi                  # the search ends within the window's width of it
    if name.startswith("sep"):
        G = int(name[3:])
        assert C.onepass and set(C.loose) <= set(C.search)
        if G < 64:                                                              # a wavefront (64 / G rows) holds both kinds
            per = 64 // G
            assert any({"s", "o"} <= {("s" if i in C.search else "o") for i in range(w, min(w + per, len(C.sig))) if C.sig[i]}
                       for w in range(0, len(C.sig), per))
        lens = {int(C.d.rowptr[i + 1] - C.d.rowptr[i]) for i in C.part}
        assert {1, G - 1, G, G + 1, 2 * G + 1} <= lens
        for side in (1, -1):
            kinds = {int(k) for i in C.part if C.sig[i] == side for k in C.d.atom_kind[C.d.rowptr[i]:C.d.rowptr[i + 1]]}
            assert kinds == {FC.LIN, FC.QUAD, FC.EXP, FC.NEGLOG}, (side, kinds)


def test_the_domain_edge_row_is_infinite_at_x_star_and_ends_below_one():
    C = FC.sep_case(8)
    (i,) = C.loose
    row = FR.sep_row(C.d, i)
    assert C.xs[row.cols[1]] + row.p1[1] == 0.0                                 # log(0): +inf in float64 on the device
    fn = FR.phi_f64(C.d, i, C.xi, C.xs, C.sig[i], C.bnd[i])
    assert fn(1.0)[2] is False
    lam, conv, _ = FR.search(fn, FC.TAU, FC.ITERS)
    assert 0.0 < lam < 1.0 and fn(lam)[0] <= 0.0


def test_the_long_row_and_the_fallback_rows():
    C = FC.long_case()
    lens = np.diff(C.d.rowptr)
    assert lens[0] == FC.K_LONG + 1 and C.sig[0] == 1
    S = _searched(C)
    assert all(conv and 0.0 < lam < 1.0 for lam, conv, _ in S.values())
    order = sorted(C.part, key=lambda i: S[i][0])
    assert order[0] == 0 and S[order[1]][0] - S[0][0] > 1e-3                    # the long row blocks, far from the others
    E = FC.quad_fallback_case("edge")
    fn = FR.phi_f64(E.d, 0, E.xi, E.xs, 1, 1.0)
    assert fn(0.0)[0] == 0.0 and all(fn(t)[0] > 0.0 for t in (1e-9, 0.5, 1.0))   # only lambda = 0 is feasible
    assert FR.search(fn, FC.TAU, FC.ITERS)[:2] == (0.0, False)
    I = FC.quad_fallback_case("indefinite")
    fn = FR.phi_f64(I.d, 0, I.xi, I.xs, 1, 0.7)
    assert fn(1.0)[0] > 0 and fn(1.0)[1] < 0                                    # phi'(1) < 0: the closed form's condition fails
    lam, conv, _ = FR.search(fn, FC.TAU, FC.ITERS)
    assert conv and abs(lam - (1.8 - math.sqrt(0.44)) / 2) < 1e-6


@pytest.mark.parametrize("m_nl", FC.REDUCE_SIZES)
def test_reduction_cases(m_nl):
    for where in ("first", "middle", "last"):
        C = FC.reduce_case(m_nl, where)
        assert np.count_nonzero(C.b == 0.25) == 1 and C.b[C.blocking] == 0.25
        T = FC.reduce_case(m_nl, where, tie=True)
        twins = np.flatnonzero(T.b == 0.25)
        assert T.blocking == twins[0]
        if m_nl > 64:
            assert len(twins) == 2 and T.d.col[twins[0]] == T.d.col[twins[1]]
    lam, row = FR.reduce_lambdas([1.0, 0.5, 0.5, 0.25], [1, 1, 1, 0])
    assert (lam, row) == (0.5, 1)
    assert FR.reduce_lambdas([1.0, 1.0], [1, 1]) == (1.0, -1)


def test_point_and_sides():
    xi, xs = np.array([0.1, 0.2]), np.array([0.7, -0.4])
    assert np.array_equal(FR.device_point(xi, xs, 1.0), xs)
    assert np.array_equal(FR.device_point(xi, xs, 0.0), xi)
    assert np.array_equal(FR.x_feas(xi, xs, 0.5, np.array([0.0, 0.0]), np.array([0.3, 1.0])), [0.3, 0.0])
    C = FC.ball()
    assert list(C.sig) == [1]
    with pytest.raises(ValueError):
        FR.sides(C.d, np.array([0.0]), np.array([1.0]))
    assert list(FR.sides(C.d, np.array([-math.inf]), np.array([math.inf]))) == [0]      # a free row has nothing to satisfy
