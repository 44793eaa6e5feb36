"""GPU tier: the kernels of ktn_set_row_bounds alone (csrc/rebound.hpp k_rebase_cuts, k_row_owners, k_lin_bounds; DESIGN.md section
14 "Row bounds").  A solved pool gets new constraint bounds; every cut row must then hold the NumPy float64 value of the rule
    hi + (ub' - ub),  lo + (lb' - lb),  an equal side untouched
bit for bit, the linear rows the bounds of a fresh load, and everything else of the pool -- coefficients, multipliers, counts -- what
it held.  Owners are checked against the column lists: a cut has the columns of its row."""
import copy
import math

import numpy as np
import pytest

import katana_jl_amd as ktn
import kat_util
from helpers import hip_load_instance, hip_model_from_kat, oracle_solve_instance, pool_bits

pytestmark = pytest.mark.gpu
L = ktn._lib
INF = math.inf
COEF = (0, 1, 2, 5, 6, 7)             # of helpers.pool_bits: rowptr, col, val | duals, row count, cut count  (3, 4: lo, hi)


TIGHT_UB = [0.0, -0.953125, -0.734375, -1.015625, -0.59375, -0.859375]


def inst40(name="inst40"):
    """inst40; at its optimum only the first NL row is active, and only that row is ever cut.  "inst40_tight" is the same instance
    with the five slack NL rows' bounds pulled to just below their values at that optimum (dyadic; the CPU oracle reports
    "Optimal"), so that several lists hold cuts."""
    inst = ktn.instances.make_instance(n=40, m_nl=6, k=8, family="explog", seed=11)
    if name == "inst40_tight":
        u = np.array(inst.u_constr, dtype=np.float64)
        u[inst.m_lin:] = TIGHT_UB
        inst.u_constr = u
    return inst


def row_columns(inst):
    return [tuple(sorted(int(j) for j in inst.col[inst.rowptr[i]:inst.rowptr[i + 1]])) for i in range(inst.num_constr)]


def owners_from_columns(m, cols_of, n_lin):
    """per LP row: the one entry of cols_of {column tuple: owner} with the row's columns; -1 for the first n_lin rows"""
    rp, col, _, lo, _ = m.lp_rows()
    out = []
    for k in range(len(lo)):
        c = tuple(sorted(int(j) for j in col[rp[k]:rp[k + 1]]))
        out.append(-1 if k < n_lin else cols_of[c])
    return np.array(out, dtype=np.int64)


def rule(v, old, new, owner):
    """the NumPy float64 value of the rule for every row with an owner among the caller's rows"""
    out = v.copy()
    for k, o in enumerate(owner):
        if 0 <= o < len(old) and not (old[o] == new[o]):
            out[k] = v[k] + (new[o] - old[o])
    return out


@pytest.fixture(scope="module", params=["inst40", "inst40_tight"])
def solved(request):
    inst = inst40(request.param)
    if request.param == "inst40_tight":
        assert oracle_solve_instance(inst).status == "Optimal"                    # precondition of the variant
    m = hip_load_instance(ktn, inst)
    assert m.optimize() == "Optimal"
    return inst, m


def test_owners_are_the_rows_with_the_same_columns(solved):
    inst, m = solved
    cols = row_columns(inst)
    nl = range(inst.m_lin, inst.num_constr)
    assert len({cols[i] for i in nl}) == inst.m_nl                                # precondition: pairwise distinct column lists
    want = owners_from_columns(m, {cols[i]: i for i in nl}, inst.m_lin)
    got = m.lp_row_owners()
    assert got.dtype == np.int64 and np.array_equal(got, want), (got, want)
    assert np.all(got[:inst.m_lin] == -1)
    counts = np.bincount(got[got >= 0], minlength=inst.num_constr)
    print("cuts per NL row:", counts[inst.m_lin:])
    assert counts[inst.m_lin:].max() >= 2                                          # precondition: a list with several cuts
    if tuple(inst.u_constr[inst.m_lin:]) == tuple(TIGHT_UB):
        assert (counts[inst.m_lin:] > 0).sum() >= 3                                # ... and in the variant several lists with cuts
    assert set(np.flatnonzero(counts)) == set(int(o) for o in want if o >= 0)     # every NL row with a cut appears


@pytest.mark.parametrize("name", ["inst40", "inst40_tight"])
def test_shift_is_the_rule_bit_for_bit_and_the_rest_of_the_pool_stays(name):
    inst = inst40(name)
    m = hip_load_instance(ktn, inst)
    assert m.optimize() == "Optimal"
    ml, mc = inst.m_lin, inst.num_constr
    lb0, ub0 = np.array(inst.l_constr, dtype=np.float64), np.array(inst.u_constr, dtype=np.float64)
    lb1, ub1 = lb0.copy(), ub0.copy()
    ub1[ml:] += np.array([0.5, 0.0, -0.25, 0.125, 0.0, -0.0625])                   # a dyadic delta per NL row, two rows unchanged
    lb1[3] = ub0[3] - 8.0                                                          # a linear row gains a side
    ub1[5] = INF                                                                   # one loses its only side
    ub1[7] += 0.5                                                                  # one moves
    owner = m.lp_row_owners()
    before = pool_bits(m)
    _, _, _, lo, hi = m.lp_rows()
    m.setconstrbounds(lb1, ub1)
    after = pool_bits(m)
    _, _, _, lo2, hi2 = m.lp_rows()
    for k in COEF:
        assert after[k] == before[k], k
    cut = owner >= 0
    assert np.array_equal(owner, m.lp_row_owners())
    assert hi2[cut].tobytes() == rule(hi, ub0, ub1, owner)[cut].tobytes()
    assert lo2[cut].tobytes() == rule(lo, lb0, lb1, owner)[cut].tobytes()
    moved = np.isin(owner, [ml + 0, ml + 2, ml + 3, ml + 5])
    assert m.stat("rebase_rows") == moved.sum() and moved.sum() >= 2 and m.stat("rebase_kernel_s") >= 0.0
    assert np.all(hi2[moved] != hi[moved])
    same = cut & ~moved                                                            # every row of an unchanged constraint: bit-identical
    assert hi2[same].tobytes() == hi[same].tobytes() and lo2[same].tobytes() == lo[same].tobytes()
    # the linear rows: those of a fresh handle loaded with the new bounds
    fresh_inst = copy.copy(inst)
    fresh_inst.l_constr, fresh_inst.u_constr = lb1, ub1
    f = hip_load_instance(ktn, fresh_inst)
    _, _, _, flo, fhi = f.lp_rows()
    assert len(flo) == ml and lo2[:ml].tobytes() == flo.tobytes() and hi2[:ml].tobytes() == fhi.tobytes()
    assert hi2[5] == INF and math.isfinite(lo2[3]) and m.stat("screen_crossed_rows") == 0
    assert m.status() == "None" and m.numiters() == 0
    # the bounds in force once more: nothing moves; then the loaded ones: the linear rows are the loaded handle's again
    snap = pool_bits(m)
    m.setconstrbounds(lb1, ub1)
    assert pool_bits(m) == snap and m.stat("rebase_rows") == 0
    m.setconstrbounds(None, None)
    assert pool_bits(m) == snap
    m.setconstrbounds(lb0, ub0)
    back = pool_bits(m)
    _, _, _, lo3, hi3 = m.lp_rows()
    assert lo3[:ml].tobytes() == lo[:ml].tobytes() and hi3[:ml].tobytes() == hi[:ml].tobytes()
    assert hi3[cut].tobytes() == rule(hi2, ub1, ub0, owner)[cut].tobytes()        # (dyadic deltas on these magnitudes: exact both ways)
    for k in COEF:
        assert back[k] == before[k], k


def test_setter_with_the_loaded_bounds_leaves_the_pool_bit_for_bit(solved):
    inst, m = solved
    before = pool_bits(m)
    m.setconstrbounds(inst.l_constr, inst.u_constr)
    assert pool_bits(m) == before and m.stat("rebase_rows") == 0
    assert m.optimize() == "Optimal"                                               # (the fixture stays a solved handle)


def test_refusals_change_nothing(solved):
    inst, m = solved
    ml = inst.m_lin
    lb0, ub0 = np.array(inst.l_constr, dtype=np.float64), np.array(inst.u_constr, dtype=np.float64)
    before = pool_bits(m)
    st = m.status()

    def refused(lb, ub, code):
        with pytest.raises(L.KatanaHipError) as e:
            m.setconstrbounds(lb, ub)
        assert e.value.code == code
        assert pool_bits(m) == before and m.status() == st

    gain = lb0.copy(); gain[ml + 1] = -1.0                                         # a nonlinear row gains a lower side
    refused(gain, ub0, L.E_INVALID)
    lose = ub0.copy(); lose[ml + 2] = INF; lose[2] += 1.0                          # one loses its side (the linear change with it is not made)
    refused(lb0, lose, L.E_INVALID)
    flip = lb0.copy(); flip[ml] = INF                                              # -inf -> +inf is not "the same side"
    refused(flip, None, L.E_INVALID)
    nan = ub0.copy(); nan[0] = np.nan
    refused(None, nan, L.E_INVALID)
    with pytest.raises(ValueError):
        m.setconstrbounds(lb0[:-1], None)
    _, _, _, lo, hi = m.lp_rows()
    f = hip_load_instance(ktn, inst)
    assert f.lp_rows()[4].tobytes() == hi[:ml].tobytes()                           # the linear rows are still the loaded ones
    # handles whose cuts cannot be attributed: global lists, a cut exchange
    g = hip_load_instance(ktn, inst)
    g.lp_enable_global_lists(inst.m_nl)
    for call in (lambda: g.setconstrbounds(lb0, ub0), g.lp_row_owners):
        with pytest.raises(L.KatanaHipError) as e:
            call()
        assert e.value.code == L.E_UNSUPPORTED
    keep = L.EXCHANGE_CB(lambda *a: 0)
    g.set_cut_exchange(keep, 0)
    with pytest.raises(L.KatanaHipError) as e:
        g.setconstrbounds(lb0, ub0)
    assert e.value.code == L.E_UNSUPPORTED


@pytest.mark.parametrize("kid", ["102_04", "107_02"])
def test_epigraph_cuts_own_num_constr_and_do_not_move(kid):
    """102_04: nonlinear objective, one NL row, one linear row -- its NL row is never violated on the way (the objective minimises the
    row's own function), so its pool holds epigraph cuts only; 107_02 (nonlinear objective, an active NL row) has both kinds."""
    model = next(k for k in kat_util.load_kats() if k["id"] == kid)
    P = hip_model_from_kat(ktn, model).problem()
    m = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))
    m.loadproblem(*P)
    assert m.optimize() == "Optimal"
    sep = ktn.KatanaHipSeparator(m)
    sep.initialize()
    mc = int(P.num_constr)
    assert sep.num_constr == mc + 1                                                # the extended structure: the epigraph row last
    cols = [tuple(sorted(int(j) for j in c)) for c in sep.sp_cols]
    n_lin = sum(1 for c in model["constraints"] if c["linear"])
    assert cols[0] != cols[mc] and not model["constraints"][0]["linear"]
    got = m.lp_row_owners()
    print(kid, "owners:", got)
    # the linear rows and the rows the engine made itself while bounding the LP come first and are in no list; every row from the
    # first cut on has the columns of its owner
    n_base = int(np.flatnonzero(got >= 0)[0])
    assert n_base >= n_lin and np.all(got[:n_base] == -1)
    want = owners_from_columns(m, {cols[0]: 0, cols[mc]: mc}, n_base)
    assert np.array_equal(got, want)
    assert (got == mc).sum() >= 1                                                  # precondition: epigraph cuts
    if kid == "107_02":
        assert (got == 0).sum() >= 1                                               # precondition: cuts of the NL row next to them
    lb0, ub0 = np.array(P.l_constr, dtype=np.float64), np.array(P.u_constr, dtype=np.float64)
    lb1, ub1 = lb0.copy(), ub0.copy()
    ub1[0] += 0.5
    if n_lin:
        lb1[1] -= 0.25
    before = pool_bits(m)
    _, _, _, lo, hi = m.lp_rows()
    m.setconstrbounds(lb1, ub1)
    after = pool_bits(m)
    _, _, _, lo2, hi2 = m.lp_rows()
    for k in COEF:
        assert after[k] == before[k], k
    epi, nl = got == mc, got == 0
    assert hi2[epi].tobytes() == hi[epi].tobytes() and lo2[epi].tobytes() == lo[epi].tobytes()
    assert hi2[nl].tobytes() == (hi[nl] + (ub1[0] - ub0[0])).tobytes() and lo2[nl].tobytes() == lo[nl].tobytes()
    assert m.stat("rebase_rows") == nl.sum()
    f = ktn.NonlinearModel(ktn.KatanaSolver(log_level=0))
    f.loadproblem(*P._replace(l_constr=lb1, u_constr=ub1))
    _, _, _, flo, fhi = f.lp_rows()
    assert lo2[:n_lin].tobytes() == flo[:n_lin].tobytes() and hi2[:n_lin].tobytes() == fhi[:n_lin].tobytes()
    base = slice(n_lin, n_base)                                                    # the engine-made rows stay as they are
    assert lo2[base].tobytes() == lo[base].tobytes() and hi2[base].tobytes() == hi[base].tobytes()
