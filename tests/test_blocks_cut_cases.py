"""CPU tier: the input conditions of tests/blocks_cut_cases.py, on which tests/test_gpu_blocks_kelley.py relies."""
import numpy as np
import pytest

import blocks_cut_cases as bc
import katana_jl_amd as ktn
import sep_cases as sc
import sep_ref
from sep_ref import LIN, QUAD, EXP, NEGLOG, F_TOL

L = ktn._lib


@pytest.fixture(scope="module", params=[0, 1])
def batch(request):
    return request.param, bc.pinned_batch(request.param)


def test_pinned_batches_have_the_shapes_the_gpu_test_is_about(batch):
    edges, cases = batch
    assert 6 <= len(cases) <= 8
    assert len({C.n for C in cases}) == len(cases) and len({C.m_nl for C in cases}) == len(cases)   # arena offsets differ
    lens, subsets, sides, tags = set(), set(), set(), []
    for C in cases:
        assert C.obj_linear and np.all(C.cost != 0.0) and len(C.cost) == C.n == len(C.x)
        assert C.m_nl == C.m and np.all(C.row_linear == 0) and np.all(C.row_kind == sc.ROW_SEP)     # no linear row: the first LP has no rows
        assert not C.e_pad.any() and np.all(np.diff(C.e_rowptr) > 0)                                 # no pad_zero row, no empty row
        p = bc.pinned_problem(C)
        assert np.array_equal(p.l_var, C.x) and np.array_equal(p.u_var, C.x) and np.all(np.isfinite(C.x))
        R, E = sc.check_conditions(C)                            # margins 1 - 3 of sep_cases; threshold rows exact
        for r in range(C.m):
            a, b = C.e_rowptr[r], C.e_rowptr[r + 1]
            lens.add(int(b - a))
            subsets.add(frozenset(C.e_kind[a:b].tolist()))
            g, lb, ub = R.g[r], C.e_lb[r], C.e_ub[r]
            if np.isfinite(g):
                form = "eq" if lb == ub else ("two" if np.isfinite(lb) and np.isfinite(ub) else ("up" if np.isfinite(ub) else "lo"))
                sides.add((form, "above" if g > ub + F_TOL else ("below" if g < lb - F_TOL else "sat")))
        tags += list(C.e_tags)
        # no row undecided: every non-threshold row is farther from ub + f_tol / lb - f_tol than TWICE the reference bound (the float64
        # reference passes within slack = 2 bounds), and every round_coefs decision has its margin
        with np.errstate(all="ignore"):
            du, dl = np.abs(R.g - (C.e_ub + F_TOL)), np.abs(R.g - (C.e_lb - F_TOL))
        chk = np.isfinite(R.g) & ~C.e_threshold
        assert np.all((np.isinf(C.e_ub) | (du > R.slack * R.e_g))[chk]) and np.all((np.isinf(C.e_lb) | (dl > R.slack * R.e_g))[chk])
        assert E.round_margin_ok.all() and not E.nonfinite
        zr = np.unique(np.repeat(np.arange(E.nviol), np.diff(E.cut_rowptr))[E.zeroed])
        assert "round_coefs" in [C.e_tags[r] for r in E.viol_rows[zr]]                               # round_coefs drops something there
    assert lens >= set(bc.A_LENS), sorted(lens)
    assert len({s for s in subsets if s <= {LIN, QUAD, EXP, NEGLOG}}) == 15
    want = {(f, v) for f in ("up", "lo", "two", "eq") for v in ("sat",)} | {("up", "above"), ("lo", "below"), ("two", "above"), ("two", "below")}
    assert sides >= want and (("eq", "above") in sides or ("eq", "below") in sides), sides
    for t in ("thr_at_ub", "thr_above_ub", "thr_at_lb", "thr_below_lb", "round_coefs"):
        assert tags.count(t) == len(cases)
    assert (sum(t.startswith("edge_nan") for t in tags) > 0) == bool(edges)
    m_nl = [C.m_nl for C in cases]
    if not edges:
        assert 150 in m_nl and min(m_nl) < 16                    # three trips of the 64-group row loop, the last ragged; less than one
        big = cases[m_nl.index(150)]
        rep = unsorted = 0
        for r in range(big.m):
            cols = big.e_col[big.e_rowptr[r]:big.e_rowptr[r + 1]]
            rep += len(set(cols.tolist())) < len(cols)
            unsorted += bool(np.any(np.diff(cols) < 0))
        assert rep > 0 and unsorted > 0
        E = sc.expected_sweep(big, sc.reference(big))
        assert E.viol_slots.min() < 64 and E.viol_slots.max() >= 128                                 # cuts from the first and the third trip
    else:
        for C in cases:
            E = sc.expected_sweep(C, sc.reference(C))
            assert np.isinf(E.maxviol) == (C.edges == 1)
            assert bool(np.isnan(E.hi).any() or np.isnan(E.lo).any()) == (C.edges == 1)


def test_every_batch_qualifies_for_the_device_loop():
    for edges in (0, 1):
        assert bc.device_loop_lds([bc.pinned_problem(C) for C in bc.pinned_batch(edges)]) <= bc.LDS_BUDGET
    for items in (bc.sep_items(), bc.tape_items(), bc.quad_items(), bc.quad_items(many_rows=True), bc.mixed_items(),
                  bc.quad_items(4), bc.quad_items(16), bc.quad_items(64)):
        assert bc.device_loop_lds(items) <= bc.LDS_BUDGET
    many = bc.many_tape_rows()
    assert bc.device_loop_lds(many, bc.MANY_TAPE_CAPACITY) <= bc.LDS_BUDGET < bc.device_loop_lds(many)


def test_part_b_items_have_the_rows_the_gpu_test_is_about():
    kinds = lambda items: [[r.kind for r in bc.nl_rows_of(p)] for p in items]
    assert all(set(k) == {L.ROW_SEP} for k in kinds(bc.sep_items()))
    assert all(set(k) == {L.ROW_TAPE} for k in kinds(bc.tape_items()))
    assert all(set(k) == {L.ROW_TAPE, L.ROW_QUAD} for k in kinds(bc.mixed_items()))
    for items in (bc.sep_items(), bc.tape_items()):
        rows = [r for p in items for r in bc.nl_rows_of(p)]
        assert {len(r.cols) for r in rows} >= {3, 16, 40}                                            # below, at and beyond one 16-lane trip
        forms = {(np.isfinite(r.lb), np.isfinite(r.ub)) for r in rows}
        assert forms == {(False, True), (True, False), (True, True)}
        assert all(len(set(r.cols.tolist())) == len(r.cols) for r in rows)
    for G in (4, 16, 64):
        items = bc.quad_items(G)
        rows = bc.nl_rows_of(items[0])
        assert set(np.diff(rows[0].seg_ptr)) >= {1, G - 1, G, G + 1, 2 * G + 1} and len(rows[0].cols) == 2 * G + 7
        assert all(set(k) == {L.ROW_QUAD} for k in kinds(items))
    k = kinds(bc.quad_items(many_rows=True))
    assert len(k[0]) == 70 > 64 and set(k[0]) == {L.ROW_QUAD}    # a second trip of the 16-lanes-per-row value pass
    many = bc.many_tape_rows()
    rows = bc.nl_rows_of(many[0])
    assert len(rows) == bc.MANY_TAPE_ROWS > 1024 and many[0].num_var == bc.MANY_TAPE_COLS and {r.kind for r in rows} == {L.ROW_TAPE}
    assert all(len(r.cols) == 3 and len(r.ops) <= 20 for r in rows)                      # short tape rows


def test_row_ref_is_the_three_references_behind_one_interface():
    """value, partials and cut constant agree with a plain float64 evaluation of the same rows within the bounds"""
    import fuse_quad_cases as FQ
    rng = np.random.default_rng(3)
    for items in (bc.sep_items()[:1], bc.tape_items()[:1], bc.quad_items()[:1], bc.mixed_items()[:1]):
        p = items[0]
        x = np.clip(rng.uniform(-0.9, 0.9, p.num_var), p.l_var, p.u_var)
        qv = FQ.quad_row_values(p.d, x) if p.d.quad_ptr is not None else {}
        for r in bc.nl_rows_of(p)[:4]:
            R = bc.row_ref(r, x)
            assert len(R.der) == len(R.e_der) == len(r.cols)
            if r.kind == L.ROW_SEP:
                val, der = sep_ref.atoms_f64(r.akind, r.p0, r.p1, x[r.cols])
                g = float(np.sum(val) + r.rconst)
            elif r.kind == L.ROW_QUAD:
                g = qv[r.index]
                der = [float(r.a[e] + np.sum(r.seg_val[r.seg_ptr[e]:r.seg_ptr[e + 1]] * x[r.seg_col[r.seg_ptr[e]:r.seg_ptr[e + 1]]])) for e in range(len(r.cols))]
            else:
                from oracle import sexpr
                import tape_ref
                g, gr = sexpr.eval_grad(tape_ref.tape_to_sexpr(r.ops, r.args), x)
                g, der = g + r.rconst, [gr.get(int(c), 0.0) for c in r.cols]
            b = g - float(np.dot(x[r.cols], der))
            assert abs(sep_ref.mpf(g) - R.g) <= R.e_g and abs(sep_ref.mpf(b) - R.b) <= R.e_b, (r.kind, r.index)
            for e in range(len(r.cols)):
                assert abs(sep_ref.mpf(float(der[e])) - R.der[e]) <= R.e_der[e], (r.kind, r.index, e)
            dec, v = bc.verdict(r, R)
            fin = [t for t in (r.lb, r.ub) if np.isfinite(t)]
            assert dec in (-1, 0, 1) and abs(v - sep_ref.mpf(max(g - r.ub, r.lb - g))) <= R.e_g + 2 * sep_ref.U * (abs(g) + max(abs(t) for t in fin))
