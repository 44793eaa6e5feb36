"""GPU tier: FusedBatch.set_row_bounds (ktn_set_row_bounds on a fused batch; csrc/batch_warm.hpp k_blocks_rebase; DESIGN.md section 14
"Row bounds") on the ten instances of tests/blocks_warm_cases.py plus one expression-built instance whose quadratic objective fusion
turns into an epigraph row.

Cold: after set_row_bounds, solve() equals a fresh batch fused from instances that carry the new bounds, bit for bit.  Arena shift:
with a device launch standing, the setter moves every cut row of the resident arenas by its row's change -- the NumPy float64 value
of  hi + (ub' - ub), lo + (lb' - lb), an equal side untouched -- and leaves everything else of the arenas as it was; the arenas'
linear rows are not readable through the ABI, so they are checked through k_blocks_rewarm, which screens them: a linear row made
impossible over the box is reported by its arena index.  Warm: solve(warm=True) after the change is "Optimal" everywhere and agrees
with the fresh cold batch.

The changes: nonlinear rows loosened by 0.25 (instances 0, 2, 7, 10), tightened by 0.0625 (1, 3, 4, 8: the CPU oracle reports
"Optimal" for each of these instances with every nonlinear row tightened by that much), the rows of the LP (6) loosened, one linear
row of instance 0 loosened; instances 5 and 9 are left alone (None)."""
import copy
import math

import numpy as np
import pytest

import katana_jl_amd as ktn
from katana_jl_amd import _lib as L
from katana_jl_amd.batch import FusedBatch
import blocks_warm_cases as BC
import fuse_quad_cases as FQ
import kat_util
from helpers import max_nl_violation, oracle_solve_instance

pytestmark = pytest.mark.gpu
LP_MAX_ITER = 30000
CAP = 48
F_TOL = 1e-6
LOOSEN, TIGHTEN, NONE = (0, 2, 7, 10), (1, 3, 4, 8), (5, 9)


def solver():
    return ktn.KatanaSolver(log_level=0, lp_max_iter=LP_MAX_ITER)


@pytest.fixture(scope="module")
def world():
    items, viol, _, _ = BC.batch()
    qinst = ktn.instances.make_instance(n=24, m_nl=4, k=6, family="explog", objective="quad", seed=50)
    items = items + [FQ.quad_objective_problem(qinst, ncross=6)]
    insts = items[:9] + [None, qinst]                                             # the SeparableInstance behind an item (9: the mixed Problem)
    lb, ub = [], []
    for k, it in enumerate(items):
        p = ktn.batch._as_problem(it)
        lb.append(np.array(p.l_constr, dtype=np.float64)); ub.append(np.array(p.u_constr, dtype=np.float64))
    nub = [None] * len(items)
    for k in LOOSEN + TIGHTEN:
        i, u = insts[k], ub[k].copy()
        u[i.m_lin:] += 0.25 if k in LOOSEN else -0.0625
        nub[k] = u
    nub[0][3] += 0.5                                                               # a linear row of instance 0
    nub[6] = np.where(np.isfinite(ub[6]), ub[6] + 0.25, ub[6])                     # the LP: every finite upper side
    return dict(items=items, insts=insts, viol=viol, lb=lb, ub=ub, nub=nub)


def precondition_oracle(world):
    for k in TIGHTEN:
        i = copy.copy(world["insts"][k])
        i.u_constr = world["nub"][k]
        assert oracle_solve_instance(i).status == "Optimal", k


def with_rows(item, ub):
    if ub is None:
        return item
    if isinstance(item, ktn.Problem):
        return item._replace(u_constr=np.asarray(ub, dtype=np.float64))
    c = copy.copy(item)
    c.u_constr = np.asarray(ub, dtype=np.float64)
    return c


def cuts_bits(fb, k):
    c = fb.m.blocks_cuts(k)
    return {name: np.asarray(v).tobytes() for name, v in c.items()}


def violation(world, k, x):
    if world["insts"][k] is None:
        return world["viol"][k](x)
    i = copy.copy(world["insts"][k])
    if world["nub"][k] is not None:
        i.u_constr = world["nub"][k]
    return max_nl_violation(i, x)


def test_cold_solve_after_the_setter_equals_a_fresh_batch(world):
    precondition_oracle(world)
    items = world["items"]
    fb = FusedBatch(solver(), items)
    out0 = fb.solve(cut_capacity=CAP)
    assert all(o["status"] == "Optimal" for o in out0) and fb.m.stat("ecp_blocks_fallbacks") == 0
    cur = fb.set_row_bounds(None, world["nub"])
    ranges = fb._row_ranges()
    assert len(cur[1]) == int(fb.big.num_constr) and len(cur[1]) == sum(len(r) for r, _ in ranges) + 1       # (+1: instance 10's epigraph row)
    out1 = fb.solve(cut_capacity=CAP)
    fresh = FusedBatch(solver(), [with_rows(it, u) for it, u in zip(items, world["nub"])])
    out2 = fresh.solve(cut_capacity=CAP)
    assert fb.m.stat("ecp_blocks_fallbacks") == 0 and fresh.m.stat("ecp_blocks_fallbacks") == 0
    assert np.array_equal(np.asarray(fresh.big.u_constr, dtype=np.float64), cur[1])
    assert fb.m.blocks_results().tobytes() == fresh.m.blocks_results().tobytes()
    for k, (a, b) in enumerate(zip(out1, out2)):
        assert a["status"] == b["status"] == "Optimal" and a["x"].tobytes() == b["x"].tobytes() and a["objval"] == b["objval"], k
        assert cuts_bits(fb, k) == cuts_bits(fresh, k), k
    for k in NONE:
        assert out1[k]["x"].tobytes() == out0[k]["x"].tobytes()


def test_arena_shift_and_warm_solve(world):
    items, nub = world["items"], world["nub"]
    fb = FusedBatch(solver(), items)
    out0 = fb.solve(cut_capacity=CAP)
    assert all(o["status"] == "Optimal" for o in out0) and fb.m.stat("ecp_blocks_launches") == 1
    m, nb = fb.m, len(items)
    d = fb.big.d
    nlrows = np.flatnonzero(np.asarray(d.row_linear) == 0)                         # the engine's NL row list: slot -> fused row
    fcols = lambda r: sorted(int(j) for j in d.col[d.rowptr[r]:d.rowptr[r + 1]])
    lb0, ub0 = np.array(fb.big.l_constr, dtype=np.float64), np.array(fb.big.u_constr, dtype=np.float64)
    before = [m.blocks_cuts(k) for k in range(nb)]
    duals = [m.blocks_duals(k).tobytes() for k in range(nb)]
    lb1, ub1 = fb.set_row_bounds(None, nub)
    after = [m.blocks_cuts(k) for k in range(nb)]
    assert m.status() == "None" and [m.blocks_duals(k).tobytes() for k in range(nb)] == duals
    moved = 0
    for k in range(nb):
        c0, c1 = before[k], after[k]
        for name in ("rowptr", "col", "val", "slot", "lam"):
            assert c0[name].tobytes() == c1[name].tobytes(), (k, name)
        if len(c0["lo"]) == 0:
            continue
        owner = nlrows[c0["slot"]]
        for q, o in enumerate(owner):                                              # owners by the column lists: a cut has the columns of its row
            assert sorted(int(j) for j in c0["col"][c0["rowptr"][q]:c0["rowptr"][q + 1]]) == fcols(o), (k, q)
        ch = ub1[owner] != ub0[owner]
        want_hi = np.where(ch, c0["hi"] + (ub1[owner] - ub0[owner]), c0["hi"])
        assert c1["hi"].tobytes() == want_hi.tobytes() and c1["lo"].tobytes() == c0["lo"].tobytes(), k
        if k == 10:                                                                # its own rows moved; the cuts of the fusion-made epigraph row stay
            epi = int(fb._row_ranges()[k][0][-1]) + 1
            assert np.array_equal(ch, owner != epi) and (owner == epi).any() and ch.any()
        else:
            assert ch.all() if k in LOOSEN + TIGHTEN else not ch.any(), k
        moved += int(ch.sum())
        if k in NONE or k == 6:
            assert c1["hi"].tobytes() == c0["hi"].tobytes()
    assert moved >= 8 and m.stat("rebase_rows") == moved and m.stat("rebase_kernel_s") >= 0.0
    # ---- warm: every instance from its own shifted cuts, against the fresh cold batch
    outw = fb.solve(cut_capacity=CAP, warm=True, fallback=False)
    assert m.stat("ecp_blocks_warm_launches") == 1 and m.stat("ecp_blocks_fallbacks") == 0
    recw = m.blocks_results().copy()
    fresh = FusedBatch(solver(), [with_rows(it, u) for it, u in zip(items, nub)])
    outc = fresh.solve(cut_capacity=CAP, fallback=False)
    recc = fresh.m.blocks_results().copy()
    for k in range(nb):
        print("instance %2d: warm status %d rounds %d obj %.9f | cold status %d rounds %d obj %.9f" % (
            k, recw[k, 0], recw[k, 1], outw[k]["objval"], recc[k, 0], recc[k, 1], outc[k]["objval"]))
    print("rounds summed over the instances: cold %d, warm %d" % (recc[:, 1].sum(), recw[:, 1].sum()))
    for k in range(nb):
        assert int(recw[k, 0]) == L.STATUS_OPTIMAL == int(recc[k, 0]), k
        assert kat_util.isapprox(outw[k]["objval"], outc[k]["objval"], 1e-6, 1e-6), (k, outw[k]["objval"], outc[k]["objval"])
        v = violation(world, k, outw[k]["x"])
        assert v <= F_TOL, (k, v)
    # ---- the arenas' linear rows follow the setter: one made impossible over the box is found by the screen of k_blocks_rewarm
    k, r = 5, 2                                                                    # instance 5, its linear row 2
    idx = fb._row_ranges()[k][0]
    rp, col, val, lo, hi = m.lp_rows()
    lin_rows = np.flatnonzero(np.asarray(d.row_linear) != 0)                       # the LP's first rows: the fused linear rows in order
    lp_row = int(np.searchsorted(lin_rows, idx[r]))
    assert lin_rows[lp_row] == idx[r] and sorted(int(j) for j in col[rp[lp_row]:rp[lp_row + 1]]) == fcols(idx[r])
    first = int(np.searchsorted(lin_rows, idx[0]))                                 # instance 5's first linear row: its arena row 0
    assert lp_row - first == r
    amin, _ = m.lp_row_activity()
    assert math.isfinite(amin[lp_row]) and math.isfinite(hi[lp_row]) and amin[lp_row] < hi[lp_row]
    ub5 = world["ub"][k].copy()
    ub5[r] -= (hi[lp_row] - amin[lp_row]) + 1.0
    lst = [None] * nb
    lst[k] = ub5
    fb.set_row_bounds(None, lst)
    rec = m.blocks_rewarm()
    assert rec[k, 0] == 2 and rec[k, 5] == r, list(rec[k])
    assert [int(s) for b, s in enumerate(rec[:, 0]) if b != k] == [1] * (nb - 1)
