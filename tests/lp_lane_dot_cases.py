"""The LP of tests/test_gpu_lp_lane_dot.py: every length at which the batched lane-strided gather-dot of the LP step and check kernels
(kernels.hpp, lane_dot: U = 4 entries per lane and batch, G lanes per output) takes another path.

For each G in {4, 8, 16, 32, 64}: no entry, one, a group short by one lane / full / one over (G - 1, G, G + 1), a batch short by one
entry / full / one over (U G - 1, U G, U G + 1), and two batches plus a ragged third (2 U G + 3).  The longest is 515 entries, below
Engine::kLongRow, so that every output is served by a lane group.  Values, bounds and state as lp_cases.ragged (lp_cases._finish)."""
import functools

import numpy as np

import lp_cases

U = 4                                            # kLaneU
GROUPS = (4, 8, 16, 32, 64)
LENGTHS = sorted({v for g in GROUPS for v in (0, 1, g - 1, g, g + 1, U * g - 1, U * g, U * g + 1, 2 * U * g + 3)})
M = N = 640
R0 = C0 = 100                                    # rows [0, R0) and columns [0, C0) carry the prescribed lengths


@functools.lru_cache(maxsize=None)
def batches():
    """640 x 640: rows [0, 100) take every length from columns [100, 640); columns [0, 100) take every length from rows [100, 640),
    which also hold up to three entries of their own"""
    rng = np.random.default_rng(21)
    assert LENGTHS[-1] == 515 < lp_cases.K_LONG and LENGTHS[-1] <= N - C0 and len(LENGTHS) <= R0
    rows = [lp_cases._pick(rng, C0, N, LENGTHS[i % len(LENGTHS)]) for i in range(R0)]
    low = [[] for _ in range(M - R0)]
    for j in range(C0):
        for i in lp_cases._pick(rng, 0, M - R0, LENGTHS[j % len(LENGTHS)]):
            low[i].append(j)
    for i in range(M - R0):
        rows.append(np.array(sorted(low[i]) + list(lp_cases._pick(rng, C0, N, i % 4)), dtype=np.int64))
    case = lp_cases._finish(rng, rows, N, "Min")
    lp = case["lp"]
    assert set(LENGTHS) <= set(lp.rlen[:R0].tolist()) and set(LENGTHS) <= set(lp.clen[:C0].tolist())
    assert lp.rlen.max() == 515 and lp.clen.max() == 515
    return case
