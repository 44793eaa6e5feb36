"""GPU tier: every hand-written form of the separable-row evaluation (kernels.hpp k_sep_eval, k_sep_sweep<G, R>, its MAT form,
k_sep_eval_long, k_sep_eval_blk + k_sep_combine, k_sep_sweep_batch, the passes inside k_ecp_blocks) and k_emit on mixed-atom rows against the
high-precision reference of tests/sep_ref.py, on the cases of tests/sep_cases.py (whose input conditions
tests/test_sep_ref.py asserts).  Every case asserts the load-time statistics that name the form it means to run.
Tolerances come from sep_ref alone; the only literal is f_tol = 2^-20 (sep_ref.F_TOL).
The passes inside k_ecp_blocks are covered here by whole solves only; their cuts are compared entry by entry with the reference
in tests/test_gpu_blocks_kelley.py.

Per case, three models: edges = 0 (maxviol finite, from a lower-sided row), edges = 1 (rows whose value is NaN with finite
partials: cut rows with NaN bounds) and edges = 2 (a non-finite coefficient in a violated row: status Error, nothing appended).
"""
import ctypes

import numpy as np
import pytest

import katana_jl_amd as ktn
import sep_cases as sc
import sep_ref
from sep_ref import F_TOL

pytestmark = pytest.mark.gpu


def _cus():
    """the device's CU count, asked in a child process: this one already holds the engine's HIP runtime"""
    import subprocess, sys
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         check=True, capture_output=True, text=True, timeout=300).stdout
    return int(out.split()[-1])


def _mp_sample(C, budget):
    """rows for the mpmath comparison: every special row, then bulk rows of every length, within `budget` entries"""
    lens = np.diff(C.e_rowptr)
    sep = C.e_row_kind == sc.ROW_SEP
    rows = [r for r in range(len(lens)) if sep[r] and C.e_tags[r] != "bulk" and C.e_tags[r] != "linear"]
    longest = int(np.argmax(np.where(sep, lens, -1)))          # (the row of 8 192 entries of the row-kernel cases)
    if longest not in rows and lens[longest] <= budget // 2:
        rows.append(longest)
    used = int(sum(lens[r] for r in rows))
    seen = {int(lens[longest]): 2}
    for r in np.flatnonzero(sep):
        if C.e_tags[r] != "bulk" or seen.get(int(lens[r]), 0) >= 2 or used + lens[r] > budget:
            continue
        seen[int(lens[r])] = seen.get(int(lens[r]), 0) + 1
        rows.append(int(r)); used += int(lens[r])
    return rows


def check_case(C, stats, depth=None, mp_budget=15000, mp_rows=None, twice=False, sweep=True):
    """load C, assert the statistics, then precompute!, gencut / isconstrsat and a sweep against the reference"""
    R = sc.reference(C, depth)
    E = sc.expected_sweep(C, R)
    m = sc.load(ktn, C)
    for k, v in stats.items():
        assert m.stat(k) == v, ("statistic", k, m.stat(k), v)
    sep = ktn.KatanaHipSeparator(m); sep.initialize()
    assert np.array_equal(sep.rowptr, C.e_rowptr) and np.array_equal(sep.col, C.e_col)
    sep.precompute(C.x)
    # ---- precompute!: g and the Jacobian of every separable row, in bulk against float64
    seprows = np.flatnonzero(C.e_row_kind == sc.ROW_SEP)
    sep_ref.check_rows_f64(R, seprows, sep.g, what="precompute g")
    ent = np.flatnonzero((C.e_row_kind == sc.ROW_SEP)[R.rows])
    sep_ref.check_jac_f64(R, ent, sep.jac[ent], what="precompute jac")
    thr = np.flatnonzero(C.e_threshold)
    assert np.array_equal(sep.g[thr], R.g[thr])                 # dyadic rows: exact in every order
    # ---- a sample against mpmath, with gencut and isconstrsat
    dep = (lambda r: None) if depth is None else (lambda r: int(depth[r]))
    sample = _mp_sample(C, mp_budget) if mp_rows is None else mp_rows
    refs = {}
    for r in sample:
        M = refs[r] = sc.row_mp(C, r, dep(r))
        a, b = C.e_rowptr[r], C.e_rowptr[r + 1]
        M.check_g(sep.g[r], (C.e_tags[r], r))
        M.check_der(sep.jac[a:b], (C.e_tags[r], r))
        cols, coefs, const = sep.gencut(C.x, (C.e_lb[r], C.e_ub[r]), r)
        assert np.array_equal(cols, C.e_col[a:b]) and np.array_equal(coefs, sep.jac[a:b], equal_nan=True)
        M.check_b(const, (C.e_tags[r], r))
        want = (M.g is not None) and (M.g >= C.e_lb[r] - F_TOL) and (M.g <= C.e_ub[r] + F_TOL)
        assert sep.isconstrsat(r, C.e_lb[r], C.e_ub[r], F_TOL) == want, ("isconstrsat", C.e_tags[r], r)
    if not sweep:
        return m, sep, R, E
    # ---- sweep: the exact violated set, maxviol, the appended rows
    out = []
    for rep in range(2 if twice else 1):
        m0 = m.lp_num_rows()
        nv, mv = sep.sweep(F_TOL)
        out.append((nv, mv) + tuple(np.array(a) for a in m.lp_rows_from(m0)))
        if twice and rep == 0:
            m.reset(); sep.precompute(C.x)
    nv, mv, rowptr, col, val, lo, hi = out[0]
    # g as the sweep's own kernels left it (precompute! above ran the row kernel whatever form the sweep takes)
    g_sw = np.zeros(len(sep.g))
    ktn._lib.check(m._h, m._lib.ktn_sep_get_g(m._h, g_sw.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(g_sw)))
    nlsep = C.nl_rows[C.e_row_kind[C.nl_rows] == sc.ROW_SEP]
    sep_ref.check_rows_f64(R, nlsep, g_sw, what="sweep g")
    assert np.array_equal(g_sw[thr], R.g[thr])
    in_sweep = set(nlsep.tolist())
    for r, M in refs.items():
        if r in in_sweep:
            M.check_g(g_sw[r], ("sweep", C.e_tags[r], r))
    if twice:                                                   # the batch-blocked sweep claims bitwise reproducibility
        assert out[1][0] == nv and out[1][1] == mv
        assert all(np.array_equal(p, q, equal_nan=(p.dtype == float)) for p, q in zip(out[0][2:], out[1][2:]))
    assert nv == E.nviol > 0, ("nviol", nv, E.nviol)
    if np.isfinite(E.maxviol):
        assert abs(mv - E.maxviol) <= E.maxviol_tol, ("maxviol", mv, E.maxviol, E.maxviol_tol)
    else:
        assert mv == E.maxviol
    if E.nonfinite:
        assert m.status() == "Error" and len(lo) == 0 and m.lp_num_rows() == m0
        return m, sep, R, E
    assert m.status() != "Error"
    assert len(lo) == E.nviol and np.array_equal(rowptr, E.cut_rowptr)
    assert np.array_equal(col, E.col), "cut columns / order"
    assert E.round_margin_ok.all()
    zero = E.zeroed
    assert np.all(val[zero] == 0.0), ("round_coefs kept a coefficient", np.flatnonzero(zero & (val != 0.0))[:5])
    assert np.all(val[~zero] != 0.0), ("round_coefs dropped a coefficient", np.flatnonzero(~zero & (val == 0.0))[:5])
    bad = ~(np.abs(val - E.coef) <= E.coef_tol)
    assert not bad.any(), ("cut coefficient", np.flatnonzero(bad)[:5], val[bad][:5], E.coef[bad][:5])
    for name, dv, want, tol in (("lo", lo, E.lo, E.lo_tol), ("hi", hi, E.hi, E.hi_tol)):
        fin = np.isfinite(want)
        with np.errstate(invalid="ignore"):
            bad = fin & ~(np.abs(dv - want) <= tol)
        assert not bad.any(), ("cut bound " + name, E.viol_rows[bad][:5], dv[bad][:5], want[bad][:5], tol[bad][:5])
        nf = ~fin
        okc = (np.isnan(dv[nf]) & np.isnan(want[nf])) | (dv[nf] == want[nf])
        assert okc.all(), ("cut bound class " + name, E.viol_rows[nf][~okc][:5], dv[nf][~okc][:5], want[nf][~okc][:5])
    # the sampled rows' cut bounds against the exact cut constant
    pos = {int(r): i for i, r in enumerate(E.viol_rows)}
    for r, M in refs.items():
        if r not in pos or M.b is None:
            continue
        for dv, bnd in ((lo[pos[r]], C.e_lb[r]), (hi[pos[r]], C.e_ub[r])):
            if np.isfinite(bnd):
                assert abs(sep_ref.mpf(float(dv)) - (sep_ref.mpf(float(bnd)) - M.b)) <= M.bound_tol(bnd), ("cut bound", r, dv)
            else:
                assert dv == bnd
    return m, sep, R, E


# ---------------------------------------------------------------------------------------------------- row kernels
@pytest.mark.parametrize("rem", [1, 2, 3])
@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("G", [8, 16, 32, 64])
def test_row_kernel_ragged_mixed_rows(G, R, rem, monkeypatch):
    """k_sep_eval (R = 1) and k_sep_sweep<G, R> on ragged mixed rows at the trip boundaries, tape and linear rows inside the
    R-groups, m_nl = 4q + rem, the pad_zero epigraph row as the last slot"""
    monkeypatch.setenv("KTN_SWEEP_ROWS", str(R))
    monkeypatch.setenv("KTN_SWEEP_BATCHED", "0")
    for edges in (0, 1, 2):
        C = sc.row_kernel_case(G, rem, edges)
        assert C.m_nl % 4 == rem
        stats = dict(sweep_group=G, sweep_rows_per_group=R, sweep_blocked=0, sweep_batched=0, precompute_multirow=0, sep_long_rows=0)
        check_case(C, stats, mp_budget=12000 if edges == 0 else 3000)


def test_precompute_multirow_form_at_size(monkeypatch):
    """enough short mixed rows that precompute! takes k_sep_sweep<8, 4, true>: all rows against float64, a stratified sample
    (the first and last 256 rows, every 1000th, every special row) against mpmath; the sweep (four rows per group by size)
    meets the non-finite edge rows: Error, nothing appended"""
    monkeypatch.setenv("KTN_SWEEP_BATCHED", "0")
    C = sc.mat_case(_cus())
    lens = np.diff(C.e_rowptr)
    m = len(lens)
    rows = set(range(256)) | set(range(m - 256, m)) | set(range(0, m, 1000)) | {r for r in range(m) if C.e_tags[r] != "bulk"}
    rows = sorted(r for r in rows if C.e_row_kind[r] == sc.ROW_SEP)
    stats = dict(sweep_group=8, sweep_rows_per_group=4, precompute_multirow=1, sweep_blocked=0, sweep_batched=0)
    check_case(C, stats, mp_rows=rows)


# ---------------------------------------------------------------------------------------------------- long rows
@pytest.mark.parametrize("edges", [0, 1, 2])
def test_long_rows(edges):
    """rows of 8 193, 9 000 and 9 217 entries through k_sep_eval_long: mixed kinds, all sides, the pad_zero epigraph row
    (8 501 entries), non-finite sources at the first, a middle and the LAST entry; the sum bound follows the kernel's shape
    (sep_ref.long_row_depth) instead of k u mag"""
    C = sc.long_case(edges)
    lens = np.diff(C.e_rowptr)
    nlong = int(np.sum(lens > 8192))
    assert nlong >= len(sc.LONG_LENS) + 2 and lens[-1] == 8501 and C.e_pad[-1]
    long_nl = [r for r in C.nl_rows if lens[r] > 8192]
    assert any(np.isfinite(C.e_lb[r]) for r in long_nl)
    rows = [r for r in range(len(lens)) if lens[r] > 8192 or C.e_tags[r] != "bulk"]
    rows = rows if edges == 0 else [r for r in rows if C.e_tags[r] != "bulk"][:8]
    check_case(C, dict(sep_long_rows=nlong, sweep_blocked=0, sweep_batched=0), depth=sc.long_depth(C), mp_rows=rows)


# ---------------------------------------------------------------------------------------------------- column-blocked
@pytest.mark.parametrize("cfg,n", [(None, 16384), (None, 20000), (None, 24577), (1, 16384), (1, 20000), (1, 24577),
                                   (2, 32768), (2, 40000), (2, 49153)])
def test_column_blocked_sweep(cfg, n, monkeypatch):
    """k_sep_eval_blk + k_sep_combine (KTN_BLK_CFG default, 1, 2) on sorted mixed rows of 300 - 700 entries: entries on the
    block edges and on column n - 1, rows inside one block, rows that skip the middle block, threshold rows over the first and
    the last block, m_nl = 131"""
    if cfg is not None:
        monkeypatch.setenv("KTN_BLK_CFG", str(cfg))
    bc = 16384 if cfg == 2 else 8192
    for edges in (0, 1, 2):
        C = sc.blocked_case(n, bc, edges)
        assert C.m_nl % 64 != 0
        check_case(C, dict(sweep_blocked=1, sweep_batched=0, sweep_rows_per_group=0, sep_long_rows=0), mp_budget=12000 if edges == 0 else 3000)


def test_one_unsorted_row_sends_the_sweep_to_the_row_kernel():
    C = sc.blocked_case(20000, unsorted=True)
    r = int(np.flatnonzero(C.bulk_of == 11)[0])
    cols = C.e_col[C.e_rowptr[r]:C.e_rowptr[r + 1]]
    assert np.any(np.diff(cols) < 0)
    check_case(C, dict(sweep_blocked=0, sweep_batched=0, sweep_group=64, sweep_rows_per_group=1), mp_rows=[r] + _mp_sample(C, 4000))


# ---------------------------------------------------------------------------------------------------- batch-blocked
@pytest.mark.parametrize("m_nl,n", sc.BATCH_SHAPES)
def test_batch_blocked_sweep(m_nl, n, monkeypatch):
    """k_sep_sweep_batch (KTN_SWEEP_BATCHED=1): mixed kinds, empty rows inside a batch, a run of one kind and block beyond a
    chunk, repeated columns, unsorted rows, all sides, threshold rows; the pad_zero epigraph row of a nonlinear objective is a
    short row for n = 8 192 and a long one beyond (the batch kernel skips the slot, k_sep_eval_long fills it); two sweeps give
    the same bits"""
    monkeypatch.setenv("KTN_SWEEP_BATCHED", "1")
    for edges in (0, 1, 2):
        C = sc.batch_case(m_nl, n, edges)
        assert C.m_nl == m_nl
        lens = np.diff(C.e_rowptr)
        big = int(np.argmax(lens[:C.m]))
        a, b = C.e_rowptr[big], C.e_rowptr[big + 1]
        assert max(np.bincount(C.e_kind[a:b][C.e_col[a:b] < 8192], minlength=4)) > 1024
        nlong = 1 if n > 8192 else 0
        assert (lens[-1] > 8192) == bool(nlong) and C.e_pad[-1]
        rows = _mp_sample(C, 6000 if edges == 0 else 2000) + ([big, len(lens) - 1] if edges == 0 else [])
        check_case(C, dict(sweep_batched=1, sweep_blocked=0, sweep_rows_per_group=0, sep_long_rows=nlong),
                   depth=sc.long_depth(C), mp_rows=rows, twice=True)



# ---------------------------------------------------------------------------------------------------- the non-finite flag
# one model per (source, position) with exactly ONE row that has a non-finite coefficient: the flag has to travel from that
# entry -- the last one, another wavefront of a long row, another column block -- to the sweep's Error; and two controls in
# which the same kind of row is lower-sided, so its value +inf satisfies it: the flag is set, the row is not cut, no Error
FLAG_ROWS = [(src, pos, True) for src in ("log0", "ovf") for pos in ("first", "mid", "last")] + \
            [("log0", "last", False), ("ovf", "mid", False)]


def check_flag(make, stats, depth=None):
    for only in FLAG_ROWS:
        C = make(only)
        R = sc.reference(C, None if depth is None else depth(C))
        E = sc.expected_sweep(C, R)
        bad_rows = np.unique(R.rows[~np.isfinite(R.jac)])
        assert len(bad_rows) == 1 and E.nonfinite == only[2], only
        r = int(bad_rows[0])
        m = sc.load(ktn, C)
        for k, v in stats.items():
            assert m.stat(k) == v, ("statistic", k, m.stat(k), v)
        sep = ktn.KatanaHipSeparator(m); sep.initialize()
        sep.precompute(C.x)
        a, b = C.e_rowptr[r], C.e_rowptr[r + 1]
        sep_ref.check_jac_f64(R, np.arange(a, b), sep.jac[a:b], what=only)
        m0 = m.lp_num_rows()
        nv, mv = sep.sweep(F_TOL)
        assert nv == E.nviol, (only, nv, E.nviol)
        if only[2]:
            assert m.status() == "Error" and m.lp_num_rows() == m0, (only, m.status())
        else:
            assert m.status() != "Error" and m.lp_num_rows() == m0 + E.nviol, (only, m.status())
            assert abs(mv - E.maxviol) <= E.maxviol_tol


@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("G", [8, 64])
def test_non_finite_flag_row_kernel(G, R, monkeypatch):
    monkeypatch.setenv("KTN_SWEEP_ROWS", str(R))
    monkeypatch.setenv("KTN_SWEEP_BATCHED", "0")
    check_flag(lambda only: sc.row_kernel_case(G, 1, 2, only), dict(sweep_group=G, sweep_rows_per_group=R, sweep_blocked=0, sweep_batched=0))


def test_non_finite_flag_long_rows():
    """the source sits at entry 0 (wavefront 0), 4 423 (wavefront 5) and 8 692 (wavefront 7) of a row of 8 693 entries"""
    check_flag(lambda only: sc.long_case(2, only), dict(sweep_blocked=0, sweep_batched=0), depth=sc.long_depth)


@pytest.mark.parametrize("cfg,n", [(None, 24577), (1, 24577), (2, 40000)])
def test_non_finite_flag_column_blocked(cfg, n, monkeypatch):
    if cfg is not None:
        monkeypatch.setenv("KTN_BLK_CFG", str(cfg))
    check_flag(lambda only: sc.blocked_case(n, 16384 if cfg == 2 else 8192, 2, only=only), dict(sweep_blocked=1))


@pytest.mark.parametrize("m_nl,n", [(2047, 8192), (5000, 30000)])
def test_non_finite_flag_batch_blocked(m_nl, n, monkeypatch):
    monkeypatch.setenv("KTN_SWEEP_BATCHED", "1")
    check_flag(lambda only: sc.batch_case(m_nl, n, 2, only), dict(sweep_batched=1), depth=sc.long_depth)


# ---------------------------------------------------------------------------------------------------- device-side batch loop
CUT_CAPACITY = 128      # cuts per NL row an instance's arena holds: these smooth models cut every active row once per round for up to
                        # about 70 rounds, and the default room for 12 sends the batch to the host-driven loop (ecp_blocks_fallbacks)


def _solver():
    return ktn.KatanaSolver(log_level=0, f_tol=F_TOL, lp_max_iter=400000, iter_cap=400)


def _rows_within_f_tol(inst, x):
    R = sep_ref.rows_ref_f64(inst.rowptr, inst.col, inst.kind, inst.p0, inst.p1, inst.rconst, x)
    tol = F_TOL + R.slack * R.e_g
    return bool(np.all(R.g - inst.u_constr <= tol) and np.all(inst.l_constr - R.g <= tol))


def test_device_side_batch_loop_on_convex_mixed_atom_models():
    """k_ecp_blocks (the sweep and emit passes inside the per-instance loop) on 16 small convex models with all four atom kinds
    and upper- and lower-sided rows: one launch, no fallback; status, objective (within sep_cases.convex_objective_bound of the
    CPU oracle, of the host-driven fused loop and of the per-instance host loops) and every NL row within f_tol under the
    reference"""
    from helpers import oracle_solve_instance
    from katana_jl_amd.batch import FusedBatch
    insts = [sc.convex_instance(900 + s) for s in range(16)]
    res = FusedBatch(_solver(), insts, False, True).solve(cut_capacity=CUT_CAPACITY)
    assert res[0]["ecp_blocks_launches"] == 1 and res[0]["ecp_blocks_fallbacks"] == 0
    ref = FusedBatch(_solver(), insts, False, False).solve()
    one, _ = ktn.solve_batch(_solver(), insts, threads=1)
    for r, f, o, inst in zip(res, ref, one, insts):
        assert set(inst.kind.tolist()) == {0, 1, 2, 3} and np.isfinite(inst.l_constr).any() and np.isfinite(inst.u_constr).any()
        om = oracle_solve_instance(inst, f_tol=F_TOL)
        bound = sc.convex_objective_bound(inst, F_TOL)
        assert r["status"] == "Optimal" and f["status"] == "Optimal" and o["status"] == "Optimal" and om.status == "Optimal"
        for other in (om.getobjval(), f["objval"], o["objval"]):
            assert abs(r["objval"] - other) <= bound, (r["objval"], other, bound)
        assert _rows_within_f_tol(inst, r["x"])
        assert np.all(np.abs(r["x"]) <= 1.0)


def test_device_side_batch_loop_non_finite_row_ends_in_error():
    """one instance of the batch has a row whose value and derivative are +inf at the first LP point (a coefficient round_coefs
    keeps, so the oracle ends Error as well): the device loop ends Error, like the host-driven loop on the same batch.  The
    handle has ONE status for a batch, so 'that instance Error, the others Optimal' is asserted on the per-instance host loops
    and the oracle."""
    from helpers import oracle_solve_instance
    from katana_jl_amd.batch import FusedBatch
    insts = [sc.convex_instance(900 + s, bad=(s == 5)) for s in range(16)]
    res = FusedBatch(_solver(), insts, False, True).solve(cut_capacity=CUT_CAPACITY)
    assert res[0]["ecp_blocks_launches"] == 1 and res[0]["status"] == "Error"
    ref = FusedBatch(_solver(), insts, False, False).solve()
    assert ref[0]["status"] == "Error"
    one, _ = ktn.solve_batch(_solver(), insts, threads=1)
    want = ["Error" if s == 5 else "Optimal" for s in range(16)]
    assert [o["status"] for o in one] == want
    with np.errstate(all="ignore"):
        assert [oracle_solve_instance(i, f_tol=F_TOL).status for i in insts] == want
