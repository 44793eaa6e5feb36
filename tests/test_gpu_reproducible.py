"""GPU tier: a solve on the same inputs, by the same build, gives the same bits -- and reads no device memory that nobody wrote
(DESIGN.md "Reproducibility").

Every case of tests/repro_cases.py is solved on five fresh handles in the order  nan, unset, zero, unset, unset  of KTN_POISON
(csrc/common.hpp: every new device allocation filled, floating-point buffers with NaN or everything with 0); the order is
deliberate: the memory a destroyed `nan` handle frees is what the next unfilled handle is likely to be given.  The five
fingerprints -- everything a caller can read that is not a time -- must be equal, and `poison_fills` says the switch was live on
exactly the two filled handles.

The purging solve of test_gpu_kkt.test_report_after_a_solve_that_purged is also driven round by round: its state after every
round is compared between two unfilled handles and a `nan` handle (a mismatch names the first round and field), and the KKT
report is asserted after every round, not only after the last."""
import contextlib
import gc
import os
import time

import numpy as np
import pytest

import katana_jl_amd as ktn
import repro_cases as RC
from helpers import hip_load_instance
from test_gpu_kkt import check_against_sep_ref

pytestmark = pytest.mark.gpu

ORDER = ("nan", None, "zero", None, None)


@contextlib.contextmanager
def poison(value):
    """KTN_POISON for the handles made inside (the switch is read when a handle is made)"""
    old = os.environ.pop("KTN_POISON", None)
    if value is not None:
        os.environ["KTN_POISON"] = value
    try:
        yield
    finally:
        os.environ.pop("KTN_POISON", None)
        if old is not None:
            os.environ["KTN_POISON"] = old


def label(k, value):
    return "handle %d (KTN_POISON %s)" % (k, value or "unset")


def solved_fingerprint(name, value):
    """(fingerprint, poison_fills) of a fresh handle of the case; the handle is destroyed before the next one is made"""
    with poison(value):
        s = RC.CASES[name]()
    fp, fills = RC.fingerprint(s), s.m.stat("poison_fills")
    del s
    gc.collect()
    return fp, fills


@pytest.mark.parametrize("name", list(RC.CASES))
def test_five_handles_give_the_same_bits(name):
    fps, fills = [], []
    t0 = time.perf_counter()
    for value in ORDER:
        fp, nf = solved_fingerprint(name, value)
        fps.append(fp)
        fills.append(nf)
    print("%s: five handles in %.2f s, %d fields, poison_fills %r" % (name, time.perf_counter() - t0, len(fps[0]), fills))
    for k, value in enumerate(ORDER):
        assert (fills[k] > 0) == (value is not None), (name, label(k, value), fills[k])
    for k in range(1, len(ORDER)):
        for j in range(k):
            diff = RC.first_difference(fps[j], fps[k])
            assert diff is None, "%s: %s against %s: %s" % (name, label(j, ORDER[j]), label(k, ORDER[k]), diff)


# ---- the purging solve round by round ------------------------------------------------------------------------------------------
def stepped(value, after_round=None, case="purge_mid"):
    """the solve of case purge_mid (or purge_pdhg) driven by optimize_begin / ecp_step / optimize_end on a fresh handle: the state
    after every round, then the state after optimize_end with the status it returned (the form of fingerprint(..., report=False))"""
    inst = RC.purge_mid_instance()
    with poison(value):
        m = hip_load_instance(ktn, inst, **RC.STEPPED_KW[case])
    m.optimize_begin()
    rounds, done = [], False
    while not done:
        done = m.ecp_step()
        rounds.append(RC.state_fields(m))
        if after_round is not None:
            after_round(inst, m, len(rounds))
    st = m.optimize_end()
    rounds.append([("optimize", st)] + RC.state_fields(m))
    return rounds


@pytest.fixture(scope="module")
def plain_solves():
    """case -> fingerprint without the report fields of a plain optimize() of the case, on a handle that never called a report
    getter; computed once per case"""
    cache = {}

    def get(case):
        if case not in cache:
            s = RC.CASES[case]()
            cache[case] = RC.fingerprint(s, report=False)
            del s
            gc.collect()
        return cache[case]
    return get


def compare_traces(a, b, la, lb):
    for r in range(min(len(a), len(b))):
        diff = RC.first_difference(a[r], b[r])
        what = "round %d" % (r + 1) if r + 1 < len(a) else "after optimize_end"
        assert diff is None, "%s against %s: first difference in %s: %s" % (la, lb, what, diff)
    assert len(a) == len(b), "%s made %d rounds, %s %d" % (la, len(a) - 1, lb, len(b) - 1)


@pytest.mark.parametrize("case", list(RC.STEPPED_KW))
def test_trace_of_the_purging_solve(plain_solves, case):
    values = (None, None, "nan")
    traces = [stepped(v, case=case) for v in values]
    assert len(traces[0]) >= 3
    for k in (1, 2):
        compare_traces(traces[0], traces[k], label(0, values[0]), label(k, values[k]))
    # reading lp_rows / lp_duals between the steps changes nothing: the end state is that of a plain optimize()
    diff = RC.first_difference(traces[0][-1], plain_solves(case))
    assert diff is None, "stepped solve against optimize(): %s" % diff


def test_report_after_every_round_of_the_purging_solve(plain_solves):
    """the assertions of test_gpu_kkt.test_report_after_a_solve_that_purged after EVERY round whose LP solve ended Optimal, and the
    report computes into buffers of its own: the solve's state equals that of a handle that never called a
    getter"""
    checked, clamped = [], []

    def after_round(inst, m, r):
        if m.status() not in ("None", "Optimal"):                 # the round's LP solve did not end Optimal: the loop leaves
            return
        x, d, z, lb, gap, R = check_against_sep_ref(inst, m, "round %d" % r)
        # the report's rule for a multiplier on a side the row does not have (k_row_duals).  A linear row's d is its own LP
        # multiplier: unchanged bit for bit on the side the row has, 0 on the other.  What was zeroed is no larger than the
        # residue of prox_y can be: yt = v + sigma (-v / sigma) is off by at most 2 u |v|, u = 2^-53, and |v| <= |y| + sigma |a'x|
        # stays below 1e4 (1 + max|d|) here (rows of 8 entries of size <= 3 on a box of +-10, steps and row scales below 10)
        y = m.lp_duals()[:inst.m_lin]
        assert np.array_equal(d[:inst.m_lin], np.where(y > 0.0, 0.0, y)), (r, np.flatnonzero(d[:inst.m_lin] != np.where(y > 0.0, 0.0, y))[:5])
        nclamp, cmax = m.stat("kkt_clamped_duals"), m.stat("kkt_clamped_max")
        assert nclamp >= np.count_nonzero(y > 0.0) and cmax <= 2.0 ** -52 * 1e4 * (1.0 + np.max(np.abs(d))), (r, nclamp, cmax)
        clamped.append((r, int(nclamp), cmax))
        assert np.all(d <= 0.0), (r, np.flatnonzero(d > 0.0)[:5], d[d > 0.0][:5])
        assert np.isfinite(lb), (r, lb)
        assert lb <= inst.opt_obj + R.e_LB + 1e-12 * (1.0 + abs(inst.opt_obj)), (r, lb, inst.opt_obj, R.e_LB)
        checked.append(r)

    rounds = stepped(None, after_round)
    assert len(checked) >= len(rounds) - 2 > 0, (len(checked), len(rounds))
    print("multipliers zeroed on an infinite side (round, count, largest):", [c for c in clamped if c[1]])
    assert any(c[1] for c in clamped)                             # the rule was exercised: round 2 leaves +1.8e-18 on an NL row
    diff = RC.first_difference(rounds[-1], plain_solves("purge_mid"))
    assert diff is None, "solve with a report after every round against a solve without: %s" % diff
