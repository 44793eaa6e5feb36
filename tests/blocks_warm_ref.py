"""What k_blocks_rewarm (csrc/batch_warm.hpp) does to ONE instance's arena between two device launches, as plain Python over lists
and floats (DESIGN.md section 14 "In the device-side loop"; the style of tests/pool_ref.py).  No GPU, no numpy.

An Arena is the instance's LP as the device loop left it: m_lin linear rows first, then its cut rows; per row the local columns,
the coefficients, lo / hi, the multiplier y, lambda (None unless the supporting variant allocated it) and, for a cut row, the link
to the previous cut of the same NL slot (a LOWER row index, or -1); per NL slot the head of its list (its newest cut, or -1).

rewarm() follows the kernel step by step: (a) eligibility, (b) crossed columns, (c) clamp, (d) screen, (e) compaction, (f) record.
Sums run in the kernel's order -- LANES lanes per row, lane k takes the entries k, k + LANES, ... in order, then the butterfly --
and every other operation is a single IEEE operation written as the kernel writes it, so the records and the moved data can be
compared bit for bit.

`mut` names one deliberate defect (MUTATIONS): the CPU tier shows that its checks tell each of them from the model."""
import math

from pool_ref import lane_group_sum

LANES = 4                       # kWarmG
STATUS_OPTIMAL = 1              # KTN_STATUS_OPTIMAL
INF = math.inf
MUTATIONS = ("compact_at_half", "idle_ge", "drops_linear", "relink_skips", "relink_no_tail", "idle_ignores_y","screen_no_tau", "order_lost")
RECORD_FIELDS = ("state", "lp_rows", "nnz", "dropped_rows", "clamped_cols", "first_proving_row", "crossed_cols", "redundant_rows")


class Arena:
    def __init__(self, m_lin, cap_rows, cols, vals, lo, hi, y, prev, last, lam=None, status=STATUS_OPTIMAL, overflow=0):
        self.m_lin, self.cap_rows = int(m_lin), int(cap_rows)
        self.cols, self.vals = [list(map(int, c)) for c in cols], [list(map(float, v)) for v in vals]
        self.lo, self.hi, self.y = list(map(float, lo)), list(map(float, hi)), list(map(float, y))
        self.prev = [int(p) for p in prev]                  # per row; linear rows: -1 (in no list)
        self.last = [int(p) for p in last]                  # per NL slot
        self.lam = None if lam is None else list(map(float, lam))
        self.status, self.overflow = int(status), int(overflow)
        assert len(self.cols) == len(self.vals) == len(self.lo) == len(self.hi) == len(self.y) == len(self.prev)

    @property
    def M(self):
        return len(self.lo)

    @property
    def nnz(self):
        return sum(len(c) for c in self.cols)

    def copy(self):
        return Arena(self.m_lin, self.cap_rows, self.cols, self.vals, self.lo, self.hi, self.y, self.prev, self.last, self.lam,
                     self.status, self.overflow)

    def lists(self):
        """per NL slot the rows of its list, newest first; a link that does not strictly descend ends the walk"""
        out = []
        for head in self.last:
            rows, r = [], head
            while 0 <= r < self.M:
                rows.append(r)
                p = self.prev[r]
                r = p if p < r else -1
            out.append(rows)
        return out

    def list_y_sums(self):
        """per NL slot the multipliers of its list, newest first (their sum in this order is what the certificate adds up)"""
        return [[self.y[r] for r in rows] for rows in self.lists()]

    def slots(self):
        """per row the NL slot whose list reaches it (-1: none), as ktn_blocks_get_cuts reports it"""
        s = [-1] * self.M
        for i, rows in enumerate(self.lists()):
            for r in rows:
                s[r] = i
        return s


def screen_row(cols, vals, lo, hi, l, u, tol0):
    """(proving, redundant, amin, amax) of one row over the box: csrc/rebound.hpp's test with LANES lanes"""
    tmin_t, tmax_t, abs_t = [], [], []
    inf_min = inf_max = False
    for c, v in zip(cols, vals):
        if v == 0.0:
            tmin_t.append(0.0); tmax_t.append(0.0); abs_t.append(0.0)      # (adding +0.0 to a lane sum changes nothing)
            continue
        tl, tu = v * l[c], v * u[c]
        tmin, tmax = (tl, tu) if v > 0.0 else (tu, tl)
        fmin, fmax = abs(tmin) < INF, abs(tmax) < INF                   # (False for NaN too)
        tmin_t.append(tmin if fmin else 0.0)
        tmax_t.append(tmax if fmax else 0.0)
        inf_min, inf_max = inf_min or not fmin, inf_max or not fmax
        a0, a1 = (abs(tmin) if fmin else 0.0), (abs(tmax) if fmax else 0.0)
        abs_t.append(a0 if a0 > a1 else a1)
    smin, smax, sabs = lane_group_sum(tmin_t, LANES), lane_group_sum(tmax_t, LANES), lane_group_sum(abs_t, LANES)
    amin, amax = (-INF if inf_min else smin), (INF if inf_max else smax)
    n = len(cols)

    def proves(excess, bound, mut_no_tau=False):
        tau = tol0 + (float(n + 2) * 2.0 ** -52) * (sabs + abs(bound))
        return excess > (0.0 if mut_no_tau else tau)
    return proves, amin, amax


def idle_row(cols, vals, lo, hi, y, x, margin, ge=False, ignore_y=False):
    """the pool's idle rule without ageing (Purge (a)) at x"""
    ax = lane_group_sum([v * x[c] for c, v in zip(cols, vals)], LANES)
    slack, scale = INF, 1.0
    if math.isfinite(hi):
        slack, scale = min(slack, hi - ax), max(scale, abs(hi))
    if math.isfinite(lo):
        slack, scale = min(slack, ax - lo), max(scale, abs(lo))
    if ge:
        return y == 0.0 and slack >= margin * scale
    return (ignore_y or y == 0.0) and slack > margin * scale


def rewarm(arena, l, u, x, tol0, purge_margin, mut=None):
    """-> (record: the eight numbers of RECORD_FIELDS, arena after, x after).  The inputs are not modified."""
    assert mut is None or mut in MUTATIONS
    a, x = arena.copy(), list(map(float, x))
    M, m_lin = a.M, a.m_lin
    rec = dict(state=0, lp_rows=M, nnz=a.nnz, dropped_rows=0, clamped_cols=0, first_proving_row=-1, crossed_cols=0, redundant_rows=0)

    def done():
        return [rec[k] for k in RECORD_FIELDS], a, x
    # (a) eligibility
    if not (a.status == STATUS_OPTIMAL and a.overflow == 0):
        return done()
    # (b) crossed columns
    crossed = sum(1 for lj, uj in zip(l, u) if lj > uj)
    if crossed:
        rec.update(state=2, crossed_cols=crossed)
        return done()
    # (c) clamp
    for j, (lj, uj) in enumerate(zip(l, u)):
        xj = x[j]
        nx = lj if xj < lj else (uj if xj > uj else xj)
        if not nx == xj:
            x[j] = nx
            rec["clamped_cols"] += 1
    # (d) screen
    proving = []
    for r in range(M):
        proves, amin, amax = screen_row(a.cols[r], a.vals[r], a.lo[r], a.hi[r], l, u, tol0)
        nt = mut == "screen_no_tau"
        if proves(amin - a.hi[r], a.hi[r], nt) or proves(a.lo[r] - amax, a.lo[r], nt):
            proving.append(r)
        if amax <= a.hi[r] and amin >= a.lo[r]:
            rec["redundant_rows"] += 1
    if proving:
        rec.update(state=2, first_proving_row=min(proving))
        return done()
    rec["state"] = 1
    # (e) compaction
    room = a.cap_rows - m_lin
    over_half = (M - m_lin >= room // 2) if mut == "compact_at_half" else (M - m_lin > room // 2)
    if not over_half:
        return done()
    first = 0 if mut == "drops_linear" else m_lin
    keep = [True] * M
    for r in range(first, M):
        keep[r] = not idle_row(a.cols[r], a.vals[r], a.lo[r], a.hi[r], a.y[r], x, purge_margin, ge=mut == "idle_ge", ignore_y=mut == "idle_ignores_y")
    if all(keep):
        return done()
    dst, n = [-1] * M, 0
    for r in range(M):
        if keep[r]:
            dst[r] = n
            n += 1

    def relink(p):                                          # the first kept row at or below p along the old links, in new indices
        while p >= m_lin and not keep[p]:
            if mut == "relink_skips":
                return -1
            q = a.prev[p]
            p = q if q < p else -1
        return dst[p] if p >= m_lin else -1
    new_prev = [-1] * n
    for r in range(m_lin, M):
        if keep[r]:
            p = a.prev[r]
            new_prev[dst[r]] = relink(p if p < r else -1)
            if mut == "relink_no_tail" and new_prev[dst[r]] < 0 and p >= 0:
                new_prev[dst[r]] = dst[r]
    a.last = [relink(p if p < M else -1) for p in a.last]
    order = [r for r in range(M) if keep[r]]
    if mut == "order_lost" and len(order) - m_lin >= 2:
        order[-1], order[-2] = order[-2], order[-1]
    a.cols, a.vals = [a.cols[r] for r in order], [a.vals[r] for r in order]
    a.lo, a.hi, a.y = [a.lo[r] for r in order], [a.hi[r] for r in order], [a.y[r] for r in order]
    if a.lam is not None:
        a.lam = [a.lam[r] for r in order]
    a.prev = [-1] * m_lin + new_prev[m_lin:] if mut != "drops_linear" else new_prev
    rec.update(lp_rows=n, nnz=a.nnz, dropped_rows=M - n)
    return done()


# ---- invariants of a compaction, checked by the CPU tier on the model and by the GPU tier on the engine's arenas ----
def check_invariants(before, after, rec):
    """raises AssertionError when `after` is not what a compaction of `before` may leave"""
    m_lin = before.m_lin
    assert after.m_lin == m_lin and after.M == rec[1] and after.nnz == rec[2] and before.M - after.M == rec[3]
    # linear rows never move
    for r in range(m_lin):
        assert (after.cols[r], after.vals[r], after.lo[r], after.hi[r], after.y[r]) == (before.cols[r], before.vals[r], before.lo[r], before.hi[r], before.y[r]), r
    # links strictly descend, stay among the cut rows, and every cut row is in exactly one list
    seen = [0] * after.M
    for rows in after.lists():
        for r in rows:
            assert r >= m_lin
            seen[r] += 1
    for r in range(m_lin, after.M):
        assert after.prev[r] < r and (after.prev[r] == -1 or after.prev[r] >= m_lin), (r, after.prev[r])
        assert seen[r] == 1, (r, seen[r])
    # every list's multipliers are conserved: the same non-zero values in the same order, only zeros may have gone
    for i, (yb, ya) in enumerate(zip(before.list_y_sums(), after.list_y_sums())):
        assert [v for v in yb if v != 0.0] == [v for v in ya if v != 0.0], i
        assert math.fsum(yb) == math.fsum(ya), i
    # nothing moves at or below half fill
    if before.M - m_lin <= (before.cap_rows - m_lin) // 2:
        assert rec[3] == 0 and after.M == before.M
    # the survivors keep their order: the rows of `after` are a subsequence of the rows of `before`
    it = iter(range(before.M))
    for r in range(after.M):
        row = (after.cols[r], after.vals[r], after.lo[r], after.hi[r], after.y[r])
        for q in it:
            if (before.cols[q], before.vals[q], before.lo[q], before.hi[q], before.y[q]) == row:
                break
        else:
            raise AssertionError("row %d of the compacted arena is not a row of the old one in order" % r)
