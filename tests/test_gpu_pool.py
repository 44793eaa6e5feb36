"""GPU tier: the cut pool of the engine -- csrc/pool.hip with k_compact / k_append_link, k_purge_mark, k_dedupe_mark, k_purge_copy,
k_purge_relink, k_list_clip, the deepest-cut selection and the append-only column mirror -- against the plain-Python model
tests/pool_ref.py, on the scripts of tests/pool_cases.py (tests/test_pool_ref.py runs the same scripts on the CPU).

After EVERY step the engine's pool is compared with the model's exactly: structure, values, bounds, multipliers (bit patterns)
and the purge counters.  Ages and links are not exported; they show in the call at which a row disappears and in where the
multiplier of the next cut of an id comes from.  A point (x, y) is set with lp_pdhg_raw(x, y, 1, 1, 0): zero iterations leave lp_x
and lp_y at the given values."""
import numpy as np
import pytest

import katana_jl_amd as ktn
from helpers import hip_load_instance
import pool_cases as PC
import pool_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scripts():
    return {S.name: S for S in PC.all_scripts()}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def compare(m, model, what):
    rowptr, col, val, lo, hi = m.lp_rows()
    rp, c, v, l, h = model.csr()
    assert rowptr.tolist() == rp, (what, "rowptr", rowptr.tolist()[-5:], rp[-5:])
    assert col.tolist() == c, (what, "col")
    for name, dev, ref in (("val", val, v), ("lo", lo, l), ("hi", hi, h), ("y", m.lp_duals(), model.y)):
        if bits(dev) != bits(ref):
            k = next(i for i, (a, b) in enumerate(zip(np.asarray(dev).tolist(), ref)) if bits([a]) != bits([b]))
            raise AssertionError((what, name, "first difference at", k, float(np.asarray(dev)[k]), ref[k]))
    for name in ("purges", "purged_rows", "deduped_rows"):
        assert m.stat(name) == model.stats[name], (what, name, m.stat(name), model.stats[name])


def csr_of(rows):
    rowptr = np.cumsum([0] + [len(r[0]) for r in rows]).astype(np.int64)
    col = np.asarray([j for r in rows for j in r[0]], dtype=np.int32)
    val = np.asarray([a for r in rows for a in r[1]], dtype=np.float64)
    return rowptr, col, val, np.asarray([r[2] for r in rows], dtype=np.float64), np.asarray([r[3] for r in rows], dtype=np.float64)


def run_script(S):
    """the script on the engine and on a fresh model, side by side"""
    m = hip_load_instance(ktn, S.inst, **S.params)
    assert m.num_var == S.n
    if S.n_lists:
        m.lp_enable_global_lists(S.n_lists)
    model = S.new_model()
    compare(m, model, (S.name, "loaded"))
    steps = 0
    for i, step in enumerate(S.steps):
        what = (S.name, i, step[0])
        want = PC.apply_step(model, step, S.params)
        if step[0] == "append":
            m.lp_append_rows(*csr_of(step[1]), nl_id=step[2] if S.n_lists else None)
        elif step[0] == "point":
            m.lp_pdhg_raw(step[1], step[2], 1.0, 1.0, 0)
        elif step[0] == "purge":
            got = m.lp_purge()
            assert got == want, (what, got, want)
        elif step[0] == "truncate":
            m.lp_truncate(step[1])
        elif step[0] == "step":
            # one identity-scaled plain step from x with tau = 1 (the Halpern weight 1/2 against the anchor x0 = x gives back
            # the prox point): x_j - (c_j - (A'y)_j), the column sum in row order with the lanes per column the step picks
            c, _ = m.lp_objective()
            x, _ = m.lp_pdhg_raw(model.x, model.y, 1.0, 1.0, 1)
            aty = pool_ref.mirror_aty(model, model.y, pool_ref.pick_group(model.nnz / S.n))
            aty += [0.0] * (S.n - len(aty))
            ref = [xj - 1.0 * (cj - a) for xj, cj, a in zip(model.x, c.tolist(), aty)]
            assert x.tolist() == ref, (what, [(j, a, b) for j, (a, b) in enumerate(zip(x.tolist(), ref)) if a != b])
            assert (m.stat("lp_csc_sorts"), m.stat("lp_csc_merges")) == S.csc[steps], (what, S.csc[steps])
            steps += 1
        compare(m, model, what)
    return m, model


AGEING = ["ageing/p1/plain", "ageing/p2/plain", "ageing/p3/plain", "ageing/p2/min_frac", "ageing/p2/min_rows"]


@pytest.mark.parametrize("name", AGEING)
def test_ageing(scripts, name):
    """script A: a row goes at the call at which its age reaches purge_age; a tight call resets the age; y != 0, a slack inside
    the margin or exactly on it (`>` is strict), a close second side keep a row; a NaN bound and an empty row are idle; base
    rows stay; a call below purge_min_frac leaves the pool alone but the ages stand; below purge_min_rows nothing happens"""
    S = scripts[name]
    m, model = run_script(S)
    assert m.lp_num_rows() == len(S.after[-1])


@pytest.mark.parametrize("name", ["dedupe/eps%g" % PC.EPS, "dedupe/eps0", "relink"])
def test_dedupe_and_relink(scripts, name):
    """script B: exact multiples and rows within eps / 2 of the kept head go and their multiplier moves, scaled by nr / nh; 2 eps in
    one coefficient or in the bound, the other side, another length, a zero or NaN head, a head that went by age: no dedupe;
    the cuts appended afterwards inherit from the model's heads (k_purge_relink).  "relink": a list's tail ends the list"""
    run_script(scripts[name])


@pytest.mark.parametrize("G", PC.GROUPS)
def test_lane_groups_and_workgroup_edges(scripts, G):
    """script C: the same rules with G lanes per row, rows of 0, 1, G - 1, G, G + 1, 2 G + 1 entries, two workgroups"""
    run_script(scripts["groups/G%d" % G])


def test_truncate_then_append_of_the_same_id(scripts):
    """append g -> truncate -> append g: the row index comes back, the new row's link must not be itself; heads above the cut
    move down their links (k_list_clip); purge, dedupe and inheritance then work on the clipped lists"""
    run_script(scripts["truncate"])


def test_column_mirror(scripts):
    """script F: A'y through the mirror after a fresh sort, three appends (merge), a purge, a truncate (sort) and an append that
    gives one column 130 entries (merge: the few-per-column rule reads the NLP's structure, and this LP has no NL row)"""
    run_script(scripts["mirror"])


# ---- script D: the lists the engine's own sweep threads ------------------------------------------------------------------
@pytest.mark.parametrize("inherit", [0, 1])
def test_engine_lists(inherit):
    C, sweeps, _, removed = PC.engine_lists_plan(inherit)
    inst = C.inst
    m = hip_load_instance(ktn, inst, lp_dual_inherit=inherit, **PC.ENGINE_PARAMS)
    assert m.num_var == inst.n
    rowptr, col, val, lo, hi = m.lp_rows()
    M0 = len(lo)
    model = pool_ref.PoolRef([(col[rowptr[i]:rowptr[i + 1]].tolist(), val[rowptr[i]:rowptr[i + 1]].tolist(), lo[i], hi[i]) for i in range(M0)],
                             inst.m_nl)
    assert M0 == inst.m_lin

    def point(x):
        model.x, model.y = x.tolist(), [PC.engine_y(i, M0) for i in range(model.M)]
        m.lp_pdhg_raw(model.x, model.y, 1.0, 1.0, 0)

    def sweep(x, want, what):
        point(x)
        before = m.lp_num_rows()
        nv, _ = m.sweep_lp_point(1e-6)
        slots = m.last_sweep_slots().tolist()
        assert nv == len(want) and slots == want, (what, nv, slots, want)
        rp, c, v, l, h = m.lp_rows_from(before)
        rows = [(c[rp[i]:rp[i + 1]].tolist(), v[rp[i]:rp[i + 1]].tolist(), l[i], h[i]) for i in range(len(l))]
        model.append(rows, slots, inherit)
        ref, R = C.cut_rows(x, slots)
        for s, (rc, rv, rl, rh), (dc, dv, dl, dh) in zip(slots, ref, rows):              # lb - b, ub - b against the reference's b
            r = C.nl[s]
            assert dc == rc and dl == rl == -np.inf and abs(dh - rh) <= 2 * R.e_b[r], (what, s, dh, rh, R.e_b[r])
        compare(m, model, what)

    sweep(C.x1, sweeps[0], "sweep 1")
    sweep(C.x2, sweeps[1], "sweep 2")
    point(C.x3)
    model.trace = []
    got = m.lp_purge()
    want = model.lp_purge(model.x, 1, PC.MARGIN, PC.ENGINE_EPS, 0.0, 1)
    PC.check_trace_gaps(model.trace, PC.MARGIN, "engine lists")           # (the engine's own cuts: the gaps hold for them too)
    model.trace = None
    assert got == want == removed, (got, want, removed)
    compare(m, model, "purge")
    sweep(C.x1, sweeps[2], "sweep 3")
    assert (np.count_nonzero(m.lp_duals()[-30:]) > 0) == bool(inherit)


# ---- script E: the deepest-cut selection ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [8, 1000])
def test_deepest_cut_selection(cap):
    """cap 8 with 32 rows flagged: the eighth largest depth is shared by three equal rows, which all stay; the row flagged inside
    its bound (depth <= 0, negative f_tol) has the smallest key and goes.  cap 1000: no selection"""
    C, d, flagged, kept, selected = PC.selection_plan(cap)
    inst = C.inst
    m = hip_load_instance(ktn, inst, purge_age=0, cut_cap_factor=1e-9, cut_cap_min=cap)
    M0 = m.lp_num_rows()
    m.lp_pdhg_raw(C.x1, np.zeros(M0), 1.0, 1.0, 0)
    nv, _ = m.sweep_lp_point(PC.F_TOL_E)
    slots = m.last_sweep_slots().tolist()
    print("flagged", int(flagged.sum()), "kept", slots)
    assert nv == int(flagged.sum()) == 32
    assert slots == kept and selected == (cap == 8)
    assert m.stat("cut_selections") == (1 if selected else 0) and m.stat("cuts_skipped") == nv - len(kept)
    rp, c, v, l, h = m.lp_rows_from(M0)
    ref, R = C.cut_rows(C.x1, slots)
    assert len(h) == len(kept)
    for i, (s, (rc, rv, rl, rh)) in enumerate(zip(slots, ref)):                           # exactly those slots, in slot order
        assert c[rp[i]:rp[i + 1]].tolist() == rc and abs(h[i] - rh) <= 2 * R.e_b[C.nl[s]], (s, h[i], rh)
