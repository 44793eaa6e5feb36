"""GPU tier: the batched lane-strided gather-dot (kernels.hpp, lane_dot) in every LP step and check kernel that uses it, on the
one LP of tests/lp_lane_dot_cases.py -- a row and a column of every length at which a lane takes no entry, part of a batch, a
whole batch, or several, for every lane-group width.  One step and one check from a prescribed state against tests/lp_ref.py (mpmath
at 200 bits) within the bounds that module derives, as tests/test_gpu_lp_kernels.py does; every test asserts through the engine's
statistics that the form it names is the one that ran.  Between forms that do the same arithmetic (packed / plain, 1 / 2 / 4 outputs
per lane group) the comparison is exact.

k_spmv / k_spmv_skip (the power iteration, A'y of the long-column check) use the same helper, but no lp_script op reaches the power
iteration: they are covered by the whole solves of tests/tools/lp_bits.py, compared bit for bit between two builds
(profiles/step_loads_bits.txt)."""
import functools

import numpy as np
import pytest

import katana_jl_amd as ktn
from katana_jl_amd import _lib as L
import lp_cases
import lp_lane_dot_cases
import lp_ref

pytestmark = pytest.mark.gpu

STEP, CHECK = L.LPOP_STEP, L.LPOP_CHECK
ENV = ("KTN_GRP_ROWS", "KTN_GRP_COLS", "KTN_PACKED_TRIPS", "KTN_TILED", "KTN_NO_TILED_CHECK", "KTN_NO_PINNED_CHECK", "KTN_NO_PACKED")
GROUPS = lp_lane_dot_cases.GROUPS
TRIPS = (1, 2, 4)


def handle(monkeypatch, G, T):
    """a fresh handle on the case under the given development switches (read once, when the handle is made)"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(KTN_GRP_ROWS=G, KTN_GRP_COLS=G, KTN_PACKED_TRIPS=T).items():
        monkeypatch.setenv(k, str(v))
    return lp_cases.load(ktn, lp_lane_dot_cases.batches(), lp_ruiz_iters=8, lp_ruiz_warm=1)


@functools.lru_cache(maxsize=None)
def reference(k):
    """the mpmath reference of the case at Halpern counter k (identity scaling), computed once for all forms"""
    c = lp_lane_dot_cases.batches()
    lp = c["lp"]
    return lp_ref.case(lp, np.ones(lp.m), np.ones(lp.n), c["x"], c["y"], c["x0"], c["y0"], c["eta"], c["omega"], k)


def script(m, k, ops, packed):
    c = lp_lane_dot_cases.batches()
    return m.lp_script(c["x"], c["y"], c["x0"], c["y0"], c["eta"], c["omega"], k, ops, packed=packed)


def within(C, **dev):
    """every named device quantity within the derived bound of the reference; the figures are printed before they are judged"""
    ratios = {k: lp_ref.compare(C, k, v) for k, v in dev.items()}
    print("   |device - reference| / bound:", "  ".join("%s %.3g" % kv for kv in ratios.items()))
    bad = {k: r for k, r in ratios.items() if not r <= 1.0}
    assert not bad, bad


def forms(m, G, T, packed):
    assert m.stat("lp_long_rows") == 0 and m.stat("lp_long_cols") == 0 and m.stat("lp_tiled") == 0
    assert m.stat("lp_grp_rows") == G and m.stat("lp_grp_cols") == G
    assert m.stat("lp_packed") == (1 if packed else 0) and m.stat("lp_packed_trips") == T


@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
@pytest.mark.parametrize("T", TRIPS)
@pytest.mark.parametrize("G", GROUPS)
def test_step_and_check_at_every_batch_edge(monkeypatch, G, T, packed):
    """640 x 640, lengths 0 ... 515: k_pdhg_x / k_pdhg_y or the packed pair in the step, k_pdhg_x<G, false>, k_pdhg_y_chk and
    k_chk_cols in the check, from Halpern counters 0 and 5"""
    m = handle(monkeypatch, G, T)
    for k in (0, 5):
        C = reference(k)
        o = script(m, k, [STEP], packed)
        forms(m, G, T, packed)
        within(C, xn=o["x"], yn=o["y"], x0h=o["x0"], y0h=o["y0"])
        o = script(m, k, [CHECK], packed)
        forms(m, G, T, packed)
        within(C, xh=o["x"], yh=o["y"], xt=o["xt"], yt=o["yt"], q=o["q"])


@pytest.mark.parametrize("G", GROUPS)
def test_packed_and_plain_and_every_trip_count_give_the_same_bits(monkeypatch, G):
    """the plain kernels and the packed ones at 1, 2 and 4 outputs per lane group add the same products in the same order: x, y after
    two steps and xt, yt, q of the check that follows are identical bit for bit"""
    out = {}
    for T in TRIPS:
        m = handle(monkeypatch, G, T)
        for packed in (False, True):
            out[T, packed] = script(m, 5, [STEP, STEP, CHECK], packed)
            forms(m, G, T, packed)
    base = out[1, False]
    assert all(np.all(np.isfinite(base[k])) for k in ("x", "y", "xt", "yt"))
    for key, o in out.items():
        for k in ("x", "y", "xt", "yt", "q"):
            assert np.array_equal(base[k], o[k]), (key, k)
