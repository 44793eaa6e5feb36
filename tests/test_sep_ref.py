"""CPU tier: the separable-row reference (tests/sep_ref.py) and the case generator (tests/sep_cases.py) that
tests/test_gpu_sep_kernels.py relies on."""
import math

import numpy as np
import pytest

import sep_cases as sc
import sep_ref
from oracle.evaluators import SeparableNLPEvaluator
from oracle.katana import KatanaFirstOrderSeparator, linear_oa_cut, round_coefs
from sep_ref import EXP, F_TOL, LIN, NEGLOG, QUAD, mpf

INF = float("inf")


def _small_case(edges):
    return sc.make_case(5, 400, 120, [0, 1, 2, 5, 9, 17, 33, 70], [300], edges=edges, n_linear=3)


@pytest.mark.parametrize("edges", [0, 1, 2])
def test_reference_agrees_with_the_oracle_evaluator_and_cuts(edges):
    C = _small_case(edges)
    R, E = sc.check_conditions(C)
    d = SeparableNLPEvaluator(C.n, C.rowptr, C.col, C.kind, C.p0, C.p1, C.rconst, C.obj_col, C.obj_kind, C.obj_p0, C.obj_p1)
    osep = KatanaFirstOrderSeparator()
    osep.initialize(None, C.n, C.m, d)
    with np.errstate(all="ignore"):
        osep.precompute(C.x)
    assert np.array_equal(osep.csr_ptr, C.rowptr) and np.array_equal(osep.csr_col, C.col)
    rows = np.arange(C.m)
    sep_ref.check_rows_f64(R, rows, osep.g, what="oracle g")
    sep_ref.check_jac_f64(R, np.arange(len(C.col)), osep.jac[osep.csr_ind], what="oracle jac")
    viol = [int(r) for r in C.nl_rows if not osep.isconstrsat(r, C.lb[r], C.ub[r], F_TOL)]
    assert viol == [int(r) for r in E.viol_rows]
    for kcut, r in enumerate(viol):
        M = sc.row_mp(C, r)
        with np.errstate(all="ignore"):
            cut = linear_oa_cut(osep, C.x, None, r)
            M.check_g(osep.g[r]); M.check_b(cut.constant); M.check_der(cut.coeffs)
            round_coefs(cut, C.cut_coef_rng)
        a, b = E.cut_rowptr[kcut], E.cut_rowptr[kcut + 1]
        assert list(cut.vars) == list(E.col[a:b])
        if all(math.isfinite(c) for c in cut.coeffs):
            assert [c == 0.0 for c in cut.coeffs] == list(E.zeroed[a:b])
            assert np.all(np.abs(np.asarray(cut.coeffs) - E.coef[a:b]) <= E.coef_tol[a:b])


def _orders(val, rconst):
    """g in float64 under several summation orders: sequential, reversed, numpy pairwise, lane-strided partial sums with an
    xor butterfly for G = 8 .. 64, and the long-row kernel's shape (1 024 strided sums, 64-lane butterflies, 16 in order)"""
    out = {}
    s = 0.0
    for v in val:
        s += v
    out["sequential"] = s + rconst
    s = 0.0
    for v in val[::-1]:
        s += v
    out["reversed"] = s + rconst
    out["pairwise"] = float(np.sum(val)) + rconst

    def strided(G):
        acc = [0.0] * G
        for e, v in enumerate(val):
            acc[e % G] += v
        return acc

    def butterfly(acc):
        acc = list(acc)
        off = len(acc) // 2
        while off:
            acc = [acc[i] + acc[i ^ off] for i in range(len(acc))]
            off //= 2
        return acc[0]
    for G in (8, 16, 32, 64):
        out["G%d" % G] = butterfly(strided(G)) + rconst
    acc = strided(1024)
    s = 0.0
    for w in range(16):
        p = butterfly(acc[64 * w:64 * w + 64])
        s = p if w == 0 else s + p
    out["long"] = s + rconst
    return out


@pytest.mark.parametrize("k", [1, 7, 8, 9, 31, 33, 64, 65, 129, 700, 9001])
def test_bounds_hold_for_float64_in_every_summation_order(k):
    rng = np.random.default_rng(k)
    n = 12000
    x = np.where(rng.random(n) < 0.5, -1.0, 1.0) * rng.uniform(0.1, 1.0, n)
    col = np.sort(rng.choice(n, k, replace=False))
    kind = rng.integers(0, 4, k)
    p0, p1 = sc._params(rng, kind, x[col])
    M = sep_ref.row_ref_mp(col, kind, p0, p1, 0.75, x)
    Ml = sep_ref.row_ref_mp(col, kind, p0, p1, 0.75, x, depth=sep_ref.long_row_depth(k))
    assert Ml.e_g <= M.e_g or k < 30
    val, der = sep_ref.atoms_f64(kind, p0, p1, x[col])
    worst = 0.0
    for name, g in _orders(val.tolist(), 0.75).items():
        (Ml if name == "long" else M).check_g(g, name)
        worst = max(worst, float(abs(mpf(g) - M.g) / M.e_g))
    M.check_der(der)
    dots = _orders((x[col] * der).tolist(), 0.0)
    for name in ("sequential", "G8", "G64", "long"):
        (Ml if name == "long" else M).check_b(_orders(val.tolist(), 0.75)[name] - dots[name], name)
    # the bound is far below one term: a dropped entry cannot pass
    assert float(M.e_g) * 1e3 <= np.min(np.abs(val))
    g_drop = float(np.sum(val[1:])) + 0.75
    with pytest.raises(AssertionError):
        M.check_g(g_drop)
    assert worst < 1.0
    # the float64 bulk reference agrees with the mpmath one on value and bound
    R = sep_ref.rows_ref_f64([0, k], col, kind, p0, p1, [0.75], x)
    assert abs(mpf(float(R.g[0])) - M.g) <= M.e_g and abs(R.e_g[0] - float(M.e_g)) <= 1e-6 * float(M.e_g)
    assert abs(R.e_b[0] - float(M.e_b)) <= 1e-6 * float(M.e_b)


def test_subnormal_underflow_of_exp_is_not_rejected():
    # 1.5 * exp(-750): the exact value is 1e-326, a correctly rounded float64 result is 0
    M = sep_ref.row_ref_mp([0], [EXP], [1.5], [-750.0], 0.0, np.array([1.0]))
    assert M.g > 0 and M.g_f64 == 0.0
    M.check_g(0.0); M.check_der([0.0]); M.check_b(0.0)
    with pytest.raises(AssertionError):
        M.check_g(1e-300)


def test_classes_at_the_edges():
    x = np.array([0.5, -0.25, 2.0])
    # NEGLOG at s = 0: value +inf, partial -inf; the cut constant inf - x * (-inf): +inf for x > 0, NaN for x < 0
    M = sep_ref.row_ref_mp([0, 2], [NEGLOG, LIN], [1.0, 1.0], [-0.5, 0.0], 0.0, x)
    assert M.g is None and M.g_f64 == INF and M.der[0] is None and M.der_f64[0] == -INF and M.der[1] == 1 and M.b_f64 == INF
    M.check_g(INF); M.check_der([-INF, 1.0]); M.check_b(INF)
    for wrong in (-INF, float("nan"), 1e308):
        with pytest.raises(AssertionError):
            M.check_g(wrong)
    M = sep_ref.row_ref_mp([1], [NEGLOG], [1.0], [0.25], 0.0, x)
    assert M.b_f64 != M.b_f64
    M.check_b(float("nan"))
    # log of a negative: NaN value, finite partial -a / s
    M = sep_ref.row_ref_mp([0, 2], [NEGLOG, QUAD], [1.0, 1.0], [-2.5, 0.0], 0.0, x)
    assert M.g is None and M.g_f64 != M.g_f64 and M.der[0] == mpf("0.5") and M.b is None
    M.check_g(float("nan")); M.check_der([0.5, 4.0]); M.check_b(float("nan"))
    with pytest.raises(AssertionError):
        M.check_g(INF)
    with pytest.raises(AssertionError):
        M.check_der([0.5000001, 4.0])
    # exp overflow: +inf value, partial b * inf with the sign of b
    M = sep_ref.row_ref_mp([2], [EXP], [1.0], [-400.0], 0.0, -x)
    assert M.g_f64 == INF and M.der_f64[0] == -INF
    M.check_g(INF); M.check_der([-INF])
    R = sep_ref.rows_ref_f64([0, 1, 2], [0, 0], [NEGLOG, NEGLOG], [1.0, 1.0], [-0.5, -2.5], [0.0, 0.0], x)
    assert R.g[0] == INF and np.isnan(R.g[1]) and R.jac[0] == -INF and R.jac[1] == 0.5
    sep_ref.check_rows_f64(R, [0, 1], np.array([INF, float("nan")]))
    with pytest.raises(AssertionError):
        sep_ref.check_rows_f64(R, [0, 1], np.array([INF, INF]))


def _pick_group(avg):
    g = 4
    while g < 64 and 2 * g <= avg:
        g <<= 1
    return max(g, 8)


def _gpu_cases():
    for G in (8, 16, 32, 64):
        for rem in (1, 2, 3):
            for edges in (0, 1, 2):
                yield "row G%d rem%d e%d" % (G, rem, edges), (lambda G=G, rem=rem, edges=edges: sc.row_kernel_case(G, rem, edges)), G
    for edges in (0, 1, 2):
        yield "long e%d" % edges, (lambda edges=edges: sc.long_case(edges)), 64
        for n, bc in ((16384, 8192), (20000, 8192), (24577, 8192), (32768, 16384), (40000, 16384), (49153, 16384)):
            yield "blocked n%d bc%d e%d" % (n, bc, edges), (lambda n=n, bc=bc, edges=edges: sc.blocked_case(n, bc, edges)), 64
        for m_nl, n in sc.BATCH_SHAPES:
            yield "batch m%d n%d e%d" % (m_nl, n, edges), (lambda m_nl=m_nl, n=n, edges=edges: sc.batch_case(m_nl, n, edges)), None
    yield "unsorted", (lambda: sc.blocked_case(20000, unsorted=True)), 64
    for only in [(src, pos, True) for src in ("log0", "ovf") for pos in ("first", "mid", "last")] + [("log0", "last", False), ("ovf", "mid", False)]:
        yield "flag row %s" % (only,), (lambda only=only: sc.row_kernel_case(8, 1, 2, only)), 8
        yield "flag long %s" % (only,), (lambda only=only: sc.long_case(2, only)), 64
        yield "flag blocked %s" % (only,), (lambda only=only: sc.blocked_case(24577, 8192, 2, only=only)), 64
        yield "flag batch %s" % (only,), (lambda only=only: sc.batch_case(2047, 8192, 2, only)), None
    yield "mat 256 CUs", (lambda: sc.mat_case(256)), 8


def test_input_conditions_hold_on_every_gpu_case():
    """the two conditions the GPU file's exact assertions rest on (terms >= 1e3 x the value bound, rows >= 10 x the bound away
    from the thresholds; and unambiguous round_coefs decisions), the lane-group width each case means to select, and the
    coverage the generator promises: all 15 kind subsets, all sides, violated above and below"""
    for name, make, G in _gpu_cases():
        C = make()
        R, E = sc.check_conditions(C, sc.reference(C, sc.long_depth(C)) if "long" in name else None)
        lens = np.diff(C.e_rowptr)
        avg = lens[C.nl_rows].sum() / C.m_nl
        if G is not None:
            assert _pick_group(avg) == G, (name, avg)
        if name.startswith("flag"):                             # exactly one row with a non-finite coefficient
            assert len(np.unique(R.rows[~np.isfinite(R.jac)])) == 1 and E.nonfinite == ("True" in name), name
            continue
        assert E.nviol > 0 and (C.edges < 2) == (not E.nonfinite), name
        assert np.isfinite(E.maxviol) == (C.edges == 0), name
        if name.startswith("long"):                             # four more threshold rows beyond 8 192 entries
            assert sum(1 for r in np.flatnonzero(C.e_threshold) if lens[r] > 8192) == 4
        bulk = np.flatnonzero(np.asarray([t == "bulk" for t in C.e_tags]) & (lens >= 4))
        subsets = set()
        for r in bulk[:4000]:
            subsets.add(frozenset(C.e_kind[C.e_rowptr[r]:C.e_rowptr[r + 1]].tolist()))
        assert len(subsets) == 15, (name, len(subsets))
        lbf, ubf = np.isfinite(C.e_lb[bulk]), np.isfinite(C.e_ub[bulk])
        g = R.g[bulk]
        for what, msk in (("upper", ~lbf & ubf), ("lower", lbf & ~ubf), ("two-sided", lbf & ubf & (C.e_lb[bulk] < C.e_ub[bulk])),
                          ("equality", lbf & (C.e_lb[bulk] == C.e_ub[bulk]))):
            assert msk.any(), (name, what)
            above, below = g[msk] > C.e_ub[bulk][msk] + F_TOL, g[msk] < C.e_lb[bulk][msk] - F_TOL
            assert (~above & ~below).any() and (above | below).any(), (name, what)
        if C.edges == 0:                                        # the deepest violation is a lower-sided one
            r = E.viol_rows[int(np.argmax(np.where(np.isfinite(R.g[E.viol_rows]), np.fmax(R.g[E.viol_rows] - C.e_ub[E.viol_rows],
                                                                                          C.e_lb[E.viol_rows] - R.g[E.viol_rows]), 0)))]
            assert C.e_lb[r] - R.g[r] == E.maxviol, name
        tags = set(C.e_tags)
        assert {"thr_at_ub", "thr_above_ub", "thr_at_lb", "thr_below_lb", "round_coefs"} <= tags
        vr = set(int(r) for r in E.viol_rows)
        for r in np.flatnonzero(C.e_threshold):
            assert (int(r) in vr) == (C.e_tags[r] in ("thr_above_ub", "thr_below_lb")), (name, C.e_tags[r])
        if C.edges >= 1:
            assert {"edge_nan_first", "edge_nan_mid", "edge_nan_last"} <= tags
        if C.edges == 2:
            assert {"edge_log0_first", "edge_log0_mid", "edge_log0_last", "edge_ovf_first", "edge_ovf_mid", "edge_ovf_last"} <= tags
        # the round_coefs row loses every coefficient but the large one
        rr = C.e_tags.index("round_coefs")
        if not E.nonfinite:
            kc = int(np.flatnonzero(E.viol_rows == rr)[0])
            z = E.zeroed[E.cut_rowptr[kc]:E.cut_rowptr[kc + 1]]
            assert z.sum() == len(z) - 1
        if not C.obj_linear and C.e_pad[-1] and C.e_tags[-1] == "epigraph" and name.startswith(("row", "long")) and not E.nonfinite:
            kc = int(np.flatnonzero(E.viol_rows == C.m)[0])     # pad_zero: only the implicit zeros drop the negative partials
            z = E.zeroed[E.cut_rowptr[kc]:E.cut_rowptr[kc + 1]]
            assert z[:-1].all() and not z[-1]
