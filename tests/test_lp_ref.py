"""CPU tier: the LP reference (tests/lp_ref.py) and the cases the GPU tests use (tests/lp_cases.py).  The float64 twin must sit
within the derived bounds of the mpmath values on every case, every compared quantity must be finite, the step must agree with
the dense numpy recurrences of test_gpu_lp.py and the scaling with oracle/pdlp_mirror.py."""
import numpy as np
import pytest
import scipy.sparse as sp

import lp_cases
import lp_ref
from oracle import pdlp_mirror

CASES = {"ragged": lp_cases.ragged, "ragged_max": lambda: lp_cases.ragged("Max"), "long_rows": lp_cases.long_rows,
         "long_cols": lp_cases.long_cols, "long_both": lambda: lp_cases.long_cols(True), "tiled": lp_cases.tiled,
         "tiled_long": lambda: lp_cases.tiled(True), "degenerate": lp_cases.degenerate_scaling}


def _halpern_numpy(A, c, l, u, lo, hi, x, y, x0, y0, eta, omega, k0, iters):
    """test_gpu_lp._halpern_numpy with given anchors and first counter"""
    tau, sigma = eta / omega, eta * omega
    for k in range(k0, k0 + iters):
        xt = np.clip(x - tau * (c - A.T @ y), l, u)
        v = y - sigma * (A @ (2 * xt - x))
        yt = v + sigma * np.clip(-v / sigma, lo, hi)
        w = (k + 1) / (k + 2)
        x = w * (2 * xt - x) + (1 - w) * x0
        y = w * (2 * yt - y) + (1 - w) * y0
    return x, y


@pytest.mark.parametrize("k", [0, 5])
@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_within_the_bounds_of_the_exact_values_and_everything_finite(name, k):
    c = CASES[name]()
    lp = c["lp"]
    if name in ("ragged_max", "long_both", "degenerate"):         # the cases that also run under the solve's own scaling
        dr, dc, _, _ = lp_ref.ruiz(lp, 8, lp_ref.F64)
    else:
        dr, dc = np.ones(lp.m), np.ones(lp.n)
    C = lp_ref.case(lp, dr, dc, c["x"], c["y"], c["x0"], c["y0"], c["eta"], c["omega"], k)
    for q in lp_ref.NAMES:
        assert np.all(np.isfinite(C.x[q])) and np.all(np.isfinite(C.f[q])) and np.all(np.isfinite(C.b[q])), q
        ratio = lp_ref.compare(C, q, C.f[q])
        assert ratio <= 1.0, (q, ratio)
    # the case moves: a step that changes nothing would compare equal to anything
    assert np.max(np.abs(C.x["xn"] - C.x["xh"])) > 0.1 and np.max(np.abs(C.x["yn"] - C.x["yh"])) > 0.1
    qx = C.x["q"]
    used = [0, 1, 2, 3, 4, 10, 12, 21, 22, 23, 24, 25, 26, 27, 29, 30]
    assert np.all(qx[used] != 0.0) and np.all(np.delete(qx, used) == 0.0)
    assert qx[26] != qx[23]                                       # the Farkas value is not the dual objective's bound part


def test_case_ingredients():
    c = lp_cases.ragged()
    lp = c["lp"]
    assert (lp.m, lp.n) == (517, 389)
    a = np.abs(lp.val)
    assert a.min() < 0.02 and a.max() > 50.0                      # four decades
    flo, fhi = np.isfinite(lp.lo), np.isfinite(lp.hi)
    assert np.any(flo & fhi & (lp.lo < lp.hi)) and np.any(lp.lo == lp.hi) and np.any(~flo & ~fhi) and np.any(~flo & fhi) and np.any(flo & ~fhi)
    assert np.any(np.isnan(lp.lo_raw))
    fl_, fu_ = np.isfinite(lp.l), np.isfinite(lp.u)
    assert np.any(fl_ & fu_ & (lp.l < lp.u)) and np.any(lp.l == lp.u) and np.any(~fl_ & ~fu_) and np.any(fl_ & ~fu_) and np.any(~fl_ & fu_)
    y = c["y"]
    assert np.any((y > 0) & ~flo) and np.any((y < 0) & ~fhi)      # sign-infeasible duals
    assert np.any(c["x"] < lp.l) and np.any(c["x"] > lp.u) and not np.array_equal(c["x"], c["x0"])
    assert lp_cases.ragged("Max")["lp"].sense == "Max"
    lr = lp_cases.long_rows()["lp"]
    assert sorted(lr.rlen[lr.rlen >= 2048].tolist()) == [2048, 2049, 3100, 4101] and lr.n == 4200
    lc = lp_cases.long_cols()["lp"]
    assert lc.m == 2100 and np.all(lc.rlen == 3) and lc.clen[0] == 2100 and lc.clen[1] == 2048 and np.sum(lc.clen > 2048) == 1
    lb = lp_cases.long_cols(True)["lp"]
    assert np.sum(lb.rlen > 2048) == 2 and np.sum(lb.clen > 2048) == 1
    t = lp_cases.tiled()["lp"]
    assert (t.m, t.n) == (8200, 8200) and set(t.rlen.tolist()) == {3, 64} and np.all(t.col[t.row >= 8192] < 8192)
    assert np.sum(lp_cases.tiled(True)["lp"].rlen > 2048) == 1


@pytest.mark.parametrize("name", ["ragged", "ragged_max", "long_cols"])
def test_step_agrees_with_the_dense_numpy_recurrences(name):
    c = CASES[name]()
    lp = c["lp"]
    A = lp.dense()
    s = -1.0 if lp.sense == "Max" else 1.0
    x, x0 = np.clip(c["x"], lp.l, lp.u), np.clip(c["x0"], lp.l, lp.u)
    C = lp_ref.case(lp, np.ones(lp.m), np.ones(lp.n), c["x"], c["y"], c["x0"], c["y0"], c["eta"], c["omega"], 5, exact=False)
    xn, yn = _halpern_numpy(A, s * lp.c, lp.l, lp.u, lp.lo, lp.hi, x, c["y"], x0, c["y0"], c["eta"], c["omega"], 5, 1)
    assert lp_ref.compare(C, "xn", xn) <= 1.0 and lp_ref.compare(C, "yn", yn) <= 1.0
    # ... and the step after a restart: from (xt, yt), anchored there, counter 0
    xr, yr = _halpern_numpy(A, s * lp.c, lp.l, lp.u, lp.lo, lp.hi, C.f["xt"], C.f["yt"], C.f["xt"], C.f["yt"], c["eta"], c["omega"], 0, 1)
    assert lp_ref.compare(C, "xr", xr) <= 1.0 and lp_ref.compare(C, "yr", yr) <= 1.0


def test_check_sums_agree_with_a_dense_statement():
    """the sums once more, from dense matrix products and the definitions"""
    c = lp_cases.ragged()
    lp = c["lp"]
    A = lp.dense()
    C = lp_ref.case(lp, np.ones(lp.m), np.ones(lp.n), c["x"], c["y"], c["x0"], c["y0"], c["eta"], c["omega"], 5, exact=False)
    f = C.f
    xt, yt, x, y = f["xt"], f["yt"], f["xh"], f["yh"]
    q = np.zeros(32)
    q[0] = (yt - y) @ (A @ (xt - x)); q[1] = np.sum((yt - y) ** 2); q[3] = np.sum((yt - f["y0h"]) ** 2); q[4] = yt @ yt
    terms = np.array([lp.lo[i] * yt[i] if yt[i] > 0 and np.isfinite(lp.lo[i]) else lp.hi[i] * yt[i] if yt[i] < 0 and np.isfinite(lp.hi[i]) else 0.0
                      for i in range(lp.m)])
    q[2], q[10] = terms.sum(), np.abs(terms).sum()
    ax = A @ xt
    q[12] = max(0.0, np.max(np.maximum(np.where(np.isfinite(lp.lo), lp.lo - ax, 0), np.where(np.isfinite(lp.hi), ax - lp.hi, 0))))
    q[21] = np.sum((xt - x) ** 2); q[22] = lp.c @ xt; q[24] = np.sum((xt - f["x0h"]) ** 2); q[25] = xt @ xt
    for r, qs, qa, qm in ((lp.c - A.T @ yt, 23, None, 29), (-(A.T @ yt), 26, 27, 30)):
        t = np.array([lp.l[j] * r[j] if r[j] > 0 and np.isfinite(lp.l[j]) else lp.u[j] * r[j] if r[j] < 0 and np.isfinite(lp.u[j]) else 0.0
                      for j in range(lp.n)])
        bad = np.array([abs(r[j]) if (r[j] > 0 and not np.isfinite(lp.l[j])) or (r[j] < 0 and not np.isfinite(lp.u[j])) else 0.0 for j in range(lp.n)])
        q[qs] = t.sum(); q[qm] = bad.max()
        if qa:
            q[qa] = np.abs(t).sum()
    assert lp_ref.compare(C, "q", q) <= 1.0


@pytest.mark.parametrize("name", ["ragged", "long_cols"])
def test_scaling_agrees_with_the_pdlp_mirror_and_bounds_the_norm(name):
    """no empty row or column: the mirror's algorithm (factors accumulated, matrix rescaled in place) is the same mathematics"""
    lp = CASES[name]()["lp"]
    assert lp.rlen.min() > 0 or name == "ragged"
    passes = 8
    dr, dc, dr_r, dc_r = lp_ref.ruiz(lp, passes, lp_ref.F64)
    A = sp.csr_matrix((lp.val, lp.col, lp.rowptr), shape=(lp.m, lp.n))
    mr, mc = pdlp_mirror.scale_matrix(A, passes)
    E = lp_ref.scale_bound(lp, passes)
    assert np.max(np.abs(dr - mr) / dr) <= 2 * E and np.max(np.abs(dc - mc) / dc) <= 2 * E
    xr = lp_ref.ruiz(lp, passes, lp_ref.MP)
    for a, b, last in zip((dr, dc, dr_r, dc_r), xr, (True, True, False, False)):
        assert np.max(np.abs(a - lp_ref.MP.f64(b)) / a) <= lp_ref.scale_bound(lp, passes, last)
    nrm = np.linalg.norm(dr[:, None] * lp.dense() * dc[None, :], 2)
    assert nrm <= (1 + E) ** 2 + (lp.m + lp.n) * lp_ref.U


def test_scaling_keeps_the_factor_where_the_statistic_is_zero():
    lp = lp_cases.degenerate_scaling()["lp"]
    for ar in (lp_ref.F64, lp_ref.MP):
        dr, dc, dr_r, dc_r = lp_ref.ruiz(lp, 8, ar)
        assert dr[3] == 1 and dc[0] == 1 and dr_r[3] == 1 and dc_r[0] == 1
        assert all(np.isfinite(float(v)) and v > 0 for v in list(dr) + list(dc))
    assert float(dr[9]) > 1e100                                   # the row of the single 1e-300 entry is scaled up, finitely
