"""GPU tier: a handle made with profile=1 sends its timed kernels through the launch path that carries the kernel's own start /
stop events; no other test constructs such a handle.  The events must change nothing: the same kernels run on the same data, so
every result is equal BIT FOR BIT to the profile=0 handle's, and the event records count the launches that were made."""
import ctypes

import numpy as np
import pytest

import katana_jl_amd as ktn
import lp_cases
import sep_cases as sc
from sep_ref import F_TOL

pytestmark = pytest.mark.gpu

ITERS = 20
LP_ENV = ("KTN_GRP_ROWS", "KTN_GRP_COLS", "KTN_PACKED_TRIPS", "KTN_TILED", "KTN_NO_PACKED")
LP_CASES = [("ragged", lp_cases.ragged, dict(KTN_GRP_ROWS=4, KTN_GRP_COLS=4)),
            ("ragged", lp_cases.ragged, dict(KTN_GRP_ROWS=64, KTN_GRP_COLS=64)),
            ("long_rows", lp_cases.long_rows, {}),
            ("long_both", lambda: lp_cases.long_cols(True), {}),
            ("tiled", lp_cases.tiled, dict(KTN_TILED=1))]


@pytest.mark.parametrize("name,make,env", LP_CASES, ids=["ragged-G4", "ragged-G64", "long_rows", "long_both", "tiled"])
def test_lp_iterations_with_events_give_the_plain_bits(name, make, env, monkeypatch):
    """20 raw PDHG iterations from the case's state: x and y of the profile=1 handle equal the profile=0 handle's, and the
    profile=1 handle recorded one x-step and one y-step per iteration"""
    for k in LP_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    c = make()
    out = []
    for profile in (0, 1):
        m = lp_cases.load(ktn, c, profile=profile)
        out.append(m.lp_pdhg_raw(c["x"], c["y"], c["eta"], c["omega"], ITERS) + (m.stat("kx_launches"), m.stat("ky_launches")))
    (x0, y0, kx0, ky0), (x1, y1, kx1, ky1) = out
    print("   %s: kx_launches %g / %g  ky_launches %g / %g (profile 0 / 1)" % (name, kx0, kx1, ky0, ky1))
    assert np.isfinite(x0).all() and np.isfinite(y0).all() and np.any(x0 != c["x"]) and np.any(y0 != c["y"])
    assert np.array_equal(x0, x1) and np.array_equal(y0, y1)
    assert kx0 == 0 and ky0 == 0
    assert kx1 == ITERS
    assert c["lp"].m > 0 and ky1 == ITERS


@pytest.fixture(scope="module")
def sep_case():
    """64 NL rows of the G = 8 length profile (0 ... 5 G + 3 entries) over 2 000 columns, threshold and round_coefs rows included"""
    return sc.make_case(4242, 2000, 64, sc.row_profile(8))


def _sweep(C, profile):
    m = sc.load(ktn, C, profile=profile)
    sep = ktn.KatanaHipSeparator(m); sep.initialize()
    sep.precompute(C.x)
    m0 = m.lp_num_rows()
    nv, mv = sep.sweep(F_TOL)
    g, jac = np.zeros(sep.num_constr), np.zeros(sep.nnz)
    ktn._lib.check(m._h, m._lib.ktn_sep_get_g(m._h, g.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(g)))
    ktn._lib.check(m._h, m._lib.ktn_sep_get_jac(m._h, jac.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(jac)))
    cuts = tuple(np.array(a) for a in m.lp_rows_from(m0))
    stats = {k: m.stat(k) for k in ("sweep_rows_per_group", "sweep_batched", "sweep_blocked", "sweep_eval_launches")}
    return nv, mv, g, jac, cuts, stats


@pytest.mark.parametrize("env,form", [(dict(KTN_SWEEP_ROWS=1, KTN_SWEEP_BATCHED=0), dict(sweep_rows_per_group=1, sweep_batched=0)),
                                      (dict(KTN_SWEEP_ROWS=2, KTN_SWEEP_BATCHED=0), dict(sweep_rows_per_group=2, sweep_batched=0)),
                                      (dict(KTN_SWEEP_ROWS=4, KTN_SWEEP_BATCHED=0), dict(sweep_rows_per_group=4, sweep_batched=0)),
                                      (dict(KTN_SWEEP_BATCHED=1), dict(sweep_batched=1))],
                         ids=["rows1", "rows2", "rows4", "batched"])
def test_sweep_with_events_gives_the_plain_bits(env, form, sep_case, monkeypatch):
    """one sweep of the small separable case under each form of the row sweep: row values, Jacobian and the appended cuts of the
    profile=1 handle equal the profile=0 handle's; the profile=1 handle recorded the one sweep"""
    for k in ("KTN_SWEEP_ROWS", "KTN_SWEEP_BATCHED", "KTN_SWEEP_BLOCKED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    nv0, mv0, g0, jac0, cuts0, st0 = _sweep(sep_case, 0)
    nv1, mv1, g1, jac1, cuts1, st1 = _sweep(sep_case, 1)
    print("   sweep_eval_launches %g / %g (profile 0 / 1), %d violated rows" % (st0["sweep_eval_launches"], st1["sweep_eval_launches"], nv0))
    for st in (st0, st1):
        assert st["sweep_blocked"] == 0 and all(st[k] == v for k, v in form.items()), st
    assert nv0 > 0 and len(cuts0[3]) == nv0                     # (edges = 0: every violated row is cut)
    assert nv0 == nv1 and mv0 == mv1
    assert np.array_equal(g0, g1, equal_nan=True) and np.array_equal(jac0, jac1, equal_nan=True)
    assert all(np.array_equal(a, b, equal_nan=(a.dtype == float)) for a, b in zip(cuts0, cuts1))
    assert st0["sweep_eval_launches"] == 0 and st1["sweep_eval_launches"] == 1
