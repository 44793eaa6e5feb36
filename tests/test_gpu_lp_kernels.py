"""GPU tier: the LP step, check and scaling kernels, one or two ops from a prescribed state, against tests/lp_ref.py (mpmath at
200 bits) within the error bounds that module derives.  Every test asserts through the engine's statistics that the form it
names is the one that ran.  Device-against-device comparisons are exact where the arithmetic is the same, and use the suite's
1e-11 rule (test_gpu_lp.test_raw_pdhg_iterations_match_numpy) over many iterations."""
import functools

import numpy as np
import pytest

import katana_jl_amd as ktn
from katana_jl_amd import _lib as L
import lp_cases
import lp_ref

pytestmark = pytest.mark.gpu

STEP, CHECK, ADVANCE, RESTART = L.LPOP_STEP, L.LPOP_CHECK, L.LPOP_ADVANCE, L.LPOP_RESTART
PASSES = 8                                         # lp_ruiz_iters of the handles below
ENV = ("KTN_GRP_ROWS", "KTN_GRP_COLS", "KTN_PACKED_TRIPS", "KTN_TILED", "KTN_NO_TILED_CHECK", "KTN_NO_PINNED_CHECK", "KTN_NO_PACKED")
CASES = {"ragged": lp_cases.ragged, "ragged_max": lambda: lp_cases.ragged("Max"), "long_rows": lp_cases.long_rows,
         "long_cols": lp_cases.long_cols, "long_both": lambda: lp_cases.long_cols(True), "tiled": lp_cases.tiled,
         "tiled_long": lambda: lp_cases.tiled(True), "degenerate": lp_cases.degenerate_scaling}


def handle(monkeypatch, name, **env):
    """a fresh handle on the case under the given development switches (read once, when the handle is made)"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    return lp_cases.load(ktn, CASES[name](), lp_ruiz_iters=PASSES, lp_ruiz_warm=1)


@functools.lru_cache(maxsize=None)
def reference(name, k, scaling=None):
    """the mpmath reference of a case at Halpern counter k; scaling = (dr bytes, dc bytes) or None for the identity"""
    c = CASES[name]()
    lp = c["lp"]
    dr, dc = (np.ones(lp.m), np.ones(lp.n)) if scaling is None else (np.frombuffer(scaling[0]), np.frombuffer(scaling[1]))
    return lp_ref.case(lp, dr, dc, c["x"], c["y"], c["x0"], c["y0"], c["eta"], c["omega"], k)


def script(m, name, k, ops, **kw):
    c = CASES[name]()
    return m.lp_script(c["x"], c["y"], c["x0"], c["y0"], c["eta"], c["omega"], k, ops, **kw)


def within(C, **dev):
    """every named device quantity within the derived bound of the reference; the figures are printed before they are judged"""
    ratios = {k: lp_ref.compare(C, k, v) for k, v in dev.items()}
    print("   |device - reference| / bound:", "  ".join("%s %.3g" % kv for kv in ratios.items()))
    bad = {k: r for k, r in ratios.items() if not r <= 1.0}
    assert not bad, bad


def step_and_check(m, name, k, **kw):
    """one plain step and one check from the case's state at counter k, both against the reference"""
    o = script(m, name, k, [STEP], **kw)
    sc = None if kw.get("identity", True) else (o["dr"].tobytes(), o["dc"].tobytes())
    C = reference(name, k, sc)
    within(C, xn=o["x"], yn=o["y"], x0h=o["x0"], y0h=o["y0"])
    o = script(m, name, k, [CHECK], **kw)
    within(C, xh=o["x"], yh=o["y"], xt=o["xt"], yt=o["yt"], q=o["q"])
    return o


def forms(m, packed, G=None, T=None, long_rows=0, long_cols=0, tiled=0):
    assert m.stat("lp_packed") == (1 if packed else 0) and m.stat("lp_tiled") == tiled
    assert m.stat("lp_long_rows") == long_rows and m.stat("lp_long_cols") == long_cols
    if G is not None:
        assert m.stat("lp_grp_rows") == G and m.stat("lp_grp_cols") == G
    if T is not None:
        assert m.stat("lp_packed_trips") == T


# ---------------------------------------------------------------------------------------------- lane groups and trips
@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
@pytest.mark.parametrize("T", [1, 2, 4])
@pytest.mark.parametrize("G", [4, 8, 16, 32, 64])
def test_ragged_step_and_check_every_lane_group_and_trip_count(monkeypatch, G, T, packed):
    """517 x 389 with every edge length on both sides: fewer outputs than groups x T at G = 64, T = 4"""
    m = handle(monkeypatch, "ragged", KTN_GRP_ROWS=G, KTN_GRP_COLS=G, KTN_PACKED_TRIPS=T)
    o = script(m, "ragged", 0, [STEP], packed=packed)
    within(reference("ragged", 0), xn=o["x"], yn=o["y"])
    o = step_and_check(m, "ragged", 5, packed=packed)
    forms(m, packed, G, T)
    assert o["spec"] and m.stat("lp_check_pinned") == 1


def test_check_sums_through_the_device_buffer(monkeypatch):
    m = handle(monkeypatch, "ragged", KTN_NO_PINNED_CHECK=1)
    step_and_check(m, "ragged", 5)
    assert m.stat("lp_check_pinned") == 0


# ---------------------------------------------------------------------------------------------- long rows, long columns
@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
@pytest.mark.parametrize("T", [1, 2, 4])
def test_long_rows_step_and_check(monkeypatch, T, packed):
    """rows of 2048 (lane groups), 2049, 3100 and 4101 entries: the trailing workgroups of the packed kernel at T = 1 (4-way body,
    one pass of the 16-way body, tails), k_pdhg_y_long<false> otherwise, k_pdhg_y_long<true> in the check"""
    m = handle(monkeypatch, "long_rows", KTN_PACKED_TRIPS=T)
    step_and_check(m, "long_rows", 5, packed=packed)
    forms(m, packed, T=T, long_rows=3)


@pytest.mark.parametrize("name,nrows", [("long_cols", 0), ("long_both", 2)])
@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
def test_long_columns_step_and_check(monkeypatch, packed, name, nrows):
    """a column of 2100 entries and one of exactly 2048: k_pdhg_x_skip + k_pdhg_x_long, spmv_cols + k_chk_cols_vec in the check"""
    m = handle(monkeypatch, name)
    o = step_and_check(m, name, 5, packed=packed)
    forms(m, packed, long_rows=nrows, long_cols=1)
    assert not o["spec"]


# ---------------------------------------------------------------------------------------------- tiled
@pytest.mark.parametrize("name,nrows", [("tiled", 0), ("tiled_long", 1)])
def test_tiled_step_and_both_check_forms(monkeypatch, name, nrows):
    m = handle(monkeypatch, name, KTN_TILED=1)
    step_and_check(m, name, 5)
    forms(m, False, long_rows=nrows, tiled=1)
    assert m.stat("lp_tiled_builds") >= 1 and m.stat("lp_tiled_overflows") == 0 and m.stat("lp_tiled_check") == 1
    assert m.stat("lp_tiled_pieces") > 1                 # an output's sum is put together from several workgroups' pieces
    m = handle(monkeypatch, name, KTN_TILED=1, KTN_NO_TILED_CHECK=1)
    o = script(m, name, 5, [CHECK])
    within(reference(name, 5), xt=o["xt"], yt=o["yt"], q=o["q"])
    assert m.stat("lp_tiled") == 1 and m.stat("lp_tiled_check") == 0


# ---------------------------------------------------------------------------------------------- speculative update, restart
@pytest.mark.parametrize("G", [4, 64])
def test_speculative_update_of_the_check_has_the_bits_of_the_halpern_kernel(monkeypatch, G):
    m = handle(monkeypatch, "ragged", KTN_GRP_ROWS=G, KTN_GRP_COLS=G)
    a = script(m, "ragged", 5, [CHECK, ADVANCE])
    assert a["spec"] and m.stat("lp_check_spec") == 1
    b = script(m, "ragged", 5, [CHECK, ADVANCE], no_spec=True)
    assert not b["spec"] and m.stat("lp_check_spec") == 0
    assert np.array_equal(a["xnext"], b["x"]) and np.array_equal(a["ynext"], b["y"])
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["y"], b["y"])
    assert np.array_equal(a["xt"], b["xt"]) and np.array_equal(a["yt"], b["yt"]) and np.array_equal(a["q"], b["q"])
    C = reference("ragged", 5)
    within(C, xn=a["x"], yn=a["y"])


@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
def test_step_after_a_restart_starts_from_the_check_point_with_the_check_point_as_anchor(monkeypatch, packed):
    m = handle(monkeypatch, "ragged")
    o = script(m, "ragged", 5, [CHECK, RESTART, STEP], packed=packed)
    forms(m, packed)
    within(reference("ragged", 5), xr=o["x"], yr=o["y"], xt=o["x0"], yt=o["y0"])
    assert np.array_equal(o["x0"], o["xt"]) and np.array_equal(o["y0"], o["yt"])


# ---------------------------------------------------------------------------------------------- many iterations, device vs device
@pytest.mark.parametrize("name", ["ragged", "long_rows"])
def test_packed_and_plain_steps_agree_over_50_iterations(monkeypatch, name):
    m = handle(monkeypatch, name)
    a = script(m, name, 0, [STEP] * 50, packed=False)
    assert m.stat("lp_packed") == 0
    b = script(m, name, 0, [STEP] * 50, packed=True)
    assert m.stat("lp_packed") == 1
    for k in ("x", "y"):
        assert np.all(np.isfinite(a[k]))
        assert np.max(np.abs(a[k] - b[k])) <= 1e-11 * (1 + np.max(np.abs(a[k])))


# ---------------------------------------------------------------------------------------------- the solve's own scaling
@pytest.mark.parametrize("name", ["ragged_max", "long_both"])
@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
def test_step_and_check_under_the_equilibration_of_a_solve(monkeypatch, packed, name):
    """prep (scaled cost, bounds, state), the scaled values of both copies and the unscaled maxima: the reference takes the
    device's dr, dc and scales the problem itself"""
    m = handle(monkeypatch, name)
    o = step_and_check(m, name, 5, packed=packed, identity=False)
    assert m.stat("lp_packed") == (1 if packed else 0)
    assert np.ptp(o["dr"]) > 0 and np.ptp(o["dc"]) > 0
    dr, dc, _, _ = m.lp_scaling()
    assert np.array_equal(dr, o["dr"]) and np.array_equal(dc, o["dc"])


@functools.lru_cache(maxsize=None)
def scaling_reference(name):
    lp = CASES[name]()["lp"]
    return tuple(lp_ref.MP.f64(a) for a in lp_ref.ruiz(lp, PASSES, lp_ref.MP))


@pytest.mark.parametrize("name,fused,long_rows,long_cols", [("ragged", True, 0, 0), ("long_rows", False, 3, 0), ("long_cols", False, 0, 1),
                                                            ("long_both", False, 2, 1), ("degenerate", True, 0, 0)])
def test_equilibration_against_the_reference(monkeypatch, name, fused, long_rows, long_cols):
    m = handle(monkeypatch, name)
    lp = CASES[name]()["lp"]
    dev = m.lp_scaling()
    assert m.stat("lp_scale_fused_passes") == (PASSES + 1 if fused else 0) and m.stat("lp_scale_split_passes") == (0 if fused else PASSES + 1)
    assert m.stat("lp_long_rows") == long_rows and m.stat("lp_long_cols") == long_cols
    ref = scaling_reference(name)
    for label, d, r, last in (("dr", dev[0], ref[0], True), ("dc", dev[1], ref[1], True), ("dr_r", dev[2], ref[2], False), ("dc_r", dev[3], ref[3], False)):
        bound = lp_ref.scale_bound(lp, PASSES, last)
        err = np.max(np.abs(d - r) / r)
        print("   %s: relative error %.3g, bound %.3g" % (label, err, bound))
        assert np.all(np.isfinite(d)) and err <= bound, (label, err, bound)
    if name == "degenerate":                            # statistic 0: the factor stays put
        assert dev[0][3] == 1.0 and dev[1][0] == 1.0 and dev[2][3] == 1.0 and dev[3][0] == 1.0
    # Pock-Chambolle: ||diag(dr) A diag(dc)||_2 <= 1 in exact arithmetic; factors within E of the exact ones: (1 + E)^2, and numpy's
    # own backward-stable singular value: (m + n) u
    nrm = np.linalg.norm(dev[0][:, None] * lp.dense() * dev[1][None, :], 2)
    E = lp_ref.scale_bound(lp, PASSES, True)
    print("   ||A^||_2 = %.17g" % nrm)
    assert nrm <= (1 + E) ** 2 + (lp.m + lp.n) * lp_ref.U
