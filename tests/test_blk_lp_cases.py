"""CPU tier of the block-LP tests: the generator of tests/blk_lp_cases.py is checked on its own -- block-diagonal structure, the
shapes each case is there for, and the planted pair of every block against the exact-rational KKT certificate
(tests/exact_lp_ref.py) and HiGHS -- so that a failure of tests/test_gpu_blk_lp.py is a finding about the kernels, not the cases."""
import functools

import numpy as np
import pytest

import blk_lp_cases as bc
from exact_lp_cases import highs_solve
from exact_lp_ref import certify, failures

ALL = bc.FEASIBLE + bc.INFEASIBLE


def _lens(case, b):
    """(row lengths, column lengths, columns) of block b"""
    sub, idx = bc.block_lp(case, b)
    return np.diff(sub.rowptr), np.bincount(sub.col, minlength=sub.n), sub.n


@pytest.mark.parametrize("mixed", bc.ORDERS, ids=("mixed", "blockwise"))
@pytest.mark.parametrize("name", ALL)
def test_case_is_block_diagonal_under_its_offsets(name, mixed):
    case = bc.case(name, mixed)
    assert case.offsets[0] == 0 and case.offsets[-1] == case.n and np.all(np.diff(case.offsets) >= 0)
    blk_of_col = np.searchsorted(case.offsets[1:], case.col.astype(np.int64), side="right")
    rows = np.repeat(np.arange(case.m), np.diff(case.rowptr))
    assert np.array_equal(blk_of_col, case.row_block[rows])                  # no row has entries in two blocks
    assert np.array_equal(case.row_block, bc.row_blocks(case.rowptr, case.col, case.offsets))
    for i in range(case.m):                                                  # sorted, distinct columns in every row
        assert np.all(np.diff(case.col[case.rowptr[i]:case.rowptr[i + 1]].astype(np.int64)) > 0)
    nonempty = np.diff(case.rowptr) > 0
    assert np.array_equal(case.row_block[nonempty], case.info["owner"][nonempty])
    if name != "one_block":
        assert case.n > bc.MID_MAX_VAR
    rb = case.row_block[nonempty]
    if mixed and len(np.unique(rb)) > 1:                                     # (`shifted`: one block alone owns rows)
        # consecutive rows belong to different blocks about as often as in a random order (1 - sum of the squared shares)
        share = np.bincount(rb) / len(rb)
        assert np.count_nonzero(np.diff(rb) != 0) >= 0.5 * (1.0 - float(share @ share)) * len(rb) and np.count_nonzero(np.diff(rb) < 0) >= 3
    else:
        assert np.all(np.diff(rb) >= 0)
    # the two orders hold the same rows
    other = bc.case(name, not mixed)
    assert np.array_equal(other.offsets, case.offsets) and np.array_equal(other.c, case.c)
    assert sorted(np.diff(other.rowptr).tolist()) == sorted(np.diff(case.rowptr).tolist())
    assert np.array_equal(np.sort(other.val), np.sort(case.val))


def test_the_listed_lengths_and_counts_occur():
    e = bc.case("edges")
    assert np.diff(e.offsets).tolist() == [1, 3, 255, 257, 1023, 1024] == np.diff(bc.case("max_sense").offsets).tolist()
    assert bc.X_PASS == 1024 and bc.Y_PASS == 1280
    rows_of = lambda case: np.bincount(case.info["owner"], minlength=case.nblocks).tolist()
    assert [r < 256 for r in rows_of(e)] == [True, True, True, False, False, False]      # fewer outputs than lane groups
    t = bc.case("two_trips")
    assert np.diff(t.offsets).tolist()[:2] == [bc.X_PASS + 1, 2 * bc.X_PASS + 1 + 5]
    assert rows_of(t)[:4] == [bc.Y_PASS - 1, bc.Y_PASS, bc.Y_PASS + 1, 2 * bc.Y_PASS + 1]
    assert np.diff(t.offsets)[2] < bc.X_PASS < np.diff(t.offsets)[0] and rows_of(t)[4] < bc.Y_PASS     # crossing independently
    r = bc.case("ranges")
    for b in range(r.nblocks):
        rl, cl, n = _lens(r, b)
        drawn = np.diff(r.rowptr)[r.info["owner"] == b]                      # (the rows without entries count as block 0's on the device)
        assert set(bc.RANGE_LENGTHS) <= set(drawn.tolist()) and set(bc.RANGE_LENGTHS) - {0} <= set(rl.tolist())
        assert set(bc.RANGE_LENGTHS) <= set(cl[:40].tolist())
    p = bc.case("empties")
    sizes, nrows = np.diff(p.offsets), np.bincount(p.row_block, minlength=p.nblocks)
    assert sizes[0] == 0 and sizes[2] == sizes[3] == 0 and sizes[1] > 0 and sizes[4] > 0 and sizes[-1] == 0
    assert sizes[5] > 0 and nrows[5] == 0                                    # columns and no rows
    empty = np.flatnonzero(np.diff(p.rowptr) == 0)
    assert len(empty) == 2 and nrows[0] == 2                                 # the rows without entries are block 0's, which has no column
    for i in empty:
        assert not p.hi[i] < 0.0 and not p.lo[i] > 0.0                       # sides that contain 0
    assert bc.case("one_block").nblocks == 1
    big = bc.case("too_big")
    nmax, mmax = int(np.max(np.diff(big.offsets))), int(np.max(rows_of(big)))
    assert 3 * (nmax + mmax) * 8 > bc.LDS_LIMIT and min(np.diff(big.offsets)) < 100
    small = max(3 * (int(n) + m) * 8 + 4 * m + 2048 for c in (e, t, r, p) for n, m in zip(np.diff(c.offsets), rows_of(c)))
    assert small < bc.LDS_LIMIT                                              # every other case fits
    lr = bc.case("long_row")
    assert np.max(np.diff(lr.rowptr)) > bc.K_LONG and np.count_nonzero(np.diff(lr.rowptr) > bc.K_LONG) == 1
    assert np.diff(lr.offsets)[1] >= 2100
    # every row and variable kind occurs in every block of >= 6 rows / 5 columns
    for b in range(e.nblocks):
        sub, idx = bc.block_lp(e, b)
        if sub.m >= 6:
            kinds = {(bool(np.isfinite(a)), bool(np.isfinite(h)), bool(np.isnan(a)), bool(a == h)) for a, h in zip(sub.lo, sub.hi)}
            assert {(False, True, False, False), (True, True, False, False), (True, True, False, True), (False, False, False, False),
                    (False, True, True, False), (True, False, False, False)} <= kinds
        if sub.n >= 5:
            fl, fu = np.isfinite(sub.l), np.isfinite(sub.u)
            assert np.any(fl & fu & (sub.l < sub.u)) and np.any(fl & ~fu) and np.any(~fl & fu) and np.any(~fl & ~fu) and np.any(sub.l == sub.u)


@functools.lru_cache(maxsize=None)
def _planted(name):
    """per block: (sub-LP, certificate of the planted pair)"""
    case = bc.case(name)
    out = []
    for b in range(case.nblocks):
        sub, idx = bc.block_lp(case, b)
        c0, c1 = case.offsets[b], case.offsets[b + 1]
        if case.block_status[b] != "Optimal":
            out.append((sub, None))
            continue
        out.append((sub, certify(sub.csr(), sub.lo, sub.hi, sub.l, sub.u, sub.c, sub.sense, case.x[c0:c1], case.y[idx])))
    return out


@pytest.mark.parametrize("name", ALL)
def test_planted_pair_is_an_exact_kkt_pair_of_every_block(name):
    case = bc.case(name)
    tight = 0
    for b, (sub, cert) in enumerate(_planted(name)):
        if cert is None:
            continue
        print(name, b, "n", sub.n, "m", sub.m, cert)
        assert failures(cert) == [], (b, failures(cert))
        assert abs(cert.gap) <= 1e-12 * max(1.0, abs(cert.pobj)), (b, cert.gap, cert.pobj)
        assert cert.row_viol <= 1e-12 and cert.bound_viol <= 0.0
        tight += np.count_nonzero(case.y[case.row_block == b])
    assert tight >= 0.15 * np.count_nonzero(np.diff(case.rowptr))                # a share of the rows carries multipliers


@pytest.mark.parametrize("name", ALL)
def test_highs_returns_the_planted_objective_of_every_block(name):
    """(a planted vertex may be degenerate: nothing is asserted about HiGHS's x)"""
    for b, (sub, cert) in enumerate(_planted(name)):
        if sub.n == 0:                                                       # no column (HiGHS takes no such model): rows without entries only
            assert cert.pobj == 0.0 and len(sub.col) == 0
            continue
        st, obj, _, _ = highs_solve(sub)
        if cert is None:
            assert st == "Infeasible", (b, st)
            continue
        assert st == "Optimal", (b, st)
        s = -1.0 if sub.sense == "Max" else 1.0
        assert abs(s * obj - cert.pobj) <= 1e-9 * max(1.0, abs(cert.pobj)), (b, obj, cert.pobj)


@pytest.mark.parametrize("name", bc.INFEASIBLE)
def test_infeasible_cases_have_exactly_one_infeasible_block(name):
    case = bc.case(name)
    assert case.status == "Infeasible" and list(case.block_status).count("Infeasible") == 1
    bad = list(case.block_status).index("Infeasible")
    assert np.diff(case.offsets)[bad] == 8
    if name == "infeasible_empty_row":
        i = np.flatnonzero(np.diff(case.rowptr) == 0)
        assert len(i) == 1 and case.hi[i[0]] < 0.0 and bad == 0 == case.row_block[i[0]]


def test_cut_rows_cut_the_point_off_inside_their_blocks():
    case = bc.case("edges")
    rowptr, col, val, lo, hi = bc.cut_rows(case, case.x, (3, 5))
    assert len(lo) == 4
    rb = bc.row_blocks(rowptr, col, case.offsets)
    assert rb.tolist() == [3, 5, 3, 5]
    for i in range(4):
        cols = col[rowptr[i]:rowptr[i + 1]]
        assert np.all((cols >= case.offsets[rb[i]]) & (cols < case.offsets[rb[i] + 1]))
        assert float(val[rowptr[i]:rowptr[i + 1]] @ case.x[cols]) > hi[i] + 0.05
    # the touched blocks stay feasible and their objectives rise
    grown = (np.concatenate([case.rowptr, case.rowptr[-1] + rowptr[1:]]), np.concatenate([case.col, col]), np.concatenate([case.val, val]),
             np.concatenate([case.lo, lo]), np.concatenate([case.hi, hi]))
    for b in (3, 5):
        sub, idx = bc.block_lp(case, b, grown)
        st, obj, _, _ = highs_solve(sub)
        c0, c1 = case.offsets[b], case.offsets[b + 1]
        assert st == "Optimal" and len(idx) == np.count_nonzero(case.row_block == b) + 2
        assert obj > float(case.c[c0:c1] @ case.x[c0:c1]) + 0.1
