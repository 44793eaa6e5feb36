"""The cut pool as plain Python: what csrc/pool.hip and its kernels (k_append_link / k_compact's bookkeeping, k_purge_mark,
k_dedupe_mark, k_purge_copy, k_purge_relink, k_list_clip, k_depth_keys / k_depth_reflag) are documented to do, one loop each over
Python lists and floats ("The pool's rules").  No GPU, no numpy.

A x of the idle test is summed in fractions.Fraction from the float inputs, so the model does not depend on a summation order; the
case builders (tests/pool_cases.py) keep every threshold decision away from rounding.  Dedupe's arithmetic is a handful of single
IEEE operations (a maximum, a division, a difference) and is restated with the same float expressions.

`mut` names one deliberate defect (MUTATIONS); the CPU tier shows that the scripts tell every one of them from the model."""
import math
import struct
from fractions import Fraction

MUTATIONS = ("keep_le", "age_no_reset", "idle_ge", "dedupe_no_scale", "dedupe_vs_previous", "relink_no_tail", "reflag_le",
             "copy_short", "clip_keeps_head")
INF = math.inf


def pick_group(avg_len):
    """lanes per row (csrc/engine.hpp): the power of two in 4 .. 64 nearest below the mean row length"""
    g = 4
    while g < 64 and 2 * g <= avg_len:
        g <<= 1
    return g


def depth_key(depth):
    """bit pattern of a non-negative double: orders like the double itself"""
    return struct.unpack("<Q", struct.pack("<d", depth))[0]


def lane_group_sum(terms, G):
    """the engine's sum of one row or column with G lanes: lane l adds the terms l, l + G, ... in order, then the lanes are
    combined by a butterfly (lane i takes lane i ^ off for off = G / 2 ... 1); lane 0 holds the result"""
    lanes = [0.0] * G
    for k, t in enumerate(terms):
        lanes[k % G] += t
    off = G // 2
    while off:
        lanes = [lanes[i] + lanes[i ^ off] for i in range(G)]
        off //= 2
    return lanes[0]


def mirror_aty(model, y, G, arrival=None):
    """A'y column by column as the column mirror sums it: the entries of a column in ROW order (the order k_cscm_order and the
    radix sort both leave), every product rounded, G lanes.  arrival: {column: [row, ...]} puts those rows' entries last in the
    given order instead (what the append-only update would leave without its ordering pass)."""
    ncol = 1 + max([j for c in model.cols for j in c], default=-1)
    cols = [[] for _ in range(ncol)]
    for r in range(model.M):
        for j, a in zip(model.cols[r], model.vals[r]):
            cols[j].append((r, a * y[r]))
    out = []
    for j, ent in enumerate(cols):
        late = (arrival or {}).get(j, [])
        terms = [t for r, t in ent if r not in late] + [t for q in late for r, t in ent if r == q]
        out.append(lane_group_sum(terms, G))
    return out


class PoolRef:
    def __init__(self, base_rows, n_lists, mut=None):
        """base_rows: [(cols, vals, lo, hi)], the LP's own rows (never aged, never moved); n_lists: list heads (NL ids)"""
        assert mut is None or mut in MUTATIONS
        self.mut = mut
        self.cols, self.vals, self.lo, self.hi, self.y, self.age, self.prev = [], [], [], [], [], [], []
        for c, v, lo, hi in base_rows:
            self._push(c, v, lo, hi)
        self.M_base = len(self.lo)
        self.heads = [-1] * n_lists
        self.stats = dict(purges=0, purged_rows=0, deduped_rows=0)
        self._older = []
        self.tag = []                 # a name per row, riding along (the case builders' bookkeeping; no rule reads it)
        self.trace = None             # a list: every threshold decision of a purge is recorded there (for the builders' gap check)

    def _push(self, c, v, lo, hi):
        assert len(c) == len(v)
        self.cols.append([int(j) for j in c]); self.vals.append([float(a) for a in v])
        self.lo.append(float(lo)); self.hi.append(float(hi))
        self.y.append(0.0); self.age.append(0); self.prev.append(-1)

    @property
    def M(self):
        return len(self.lo)

    @property
    def nnz(self):
        return sum(len(c) for c in self.cols)

    def list_rows(self, s):
        """rows of list s, newest first; asserts what every walker relies on: the links strictly descend"""
        out, r = [], self.heads[s]
        while r >= 0:
            assert r < self.M and (not out or r < out[-1]), ("list %d does not descend" % s, out, r)
            out.append(r)
            r = self.prev[r]
        return out

    # ---- append -----------------------------------------------------------------------------------------------------------
    def append(self, rows, nl_ids, inherit):
        """rows [(cols, vals, lo, hi)] with the list id of each (outside [0, n_lists): none).  The new cut becomes the head of
        its list; with `inherit` it takes over the previous head's y, which becomes 0.  One cut per id and call."""
        ids = [g for g in nl_ids if 0 <= g < len(self.heads)]
        assert len(ids) == len(set(ids)) and len(rows) == len(nl_ids)
        for (c, v, lo, hi), g in zip(rows, nl_ids):
            R = self.M
            self._push(c, v, lo, hi)
            if 0 <= g < len(self.heads):
                p = self.heads[g]
                if inherit and p >= 0:
                    self.y[R], self.y[p] = self.y[p], 0.0
                self.prev[R] = p
                self.heads[g] = R

    # ---- purge ------------------------------------------------------------------------------------------------------------
    def slack_scale(self, r, x):
        """(slack, scale, ax) of row r at x from the finite sides only; slack as a Fraction or +inf, ax None when it is NaN"""
        ax, nan = Fraction(0), False
        for j, a in zip(self.cols[r], self.vals[r]):
            if math.isnan(a) or math.isnan(x[j]):
                nan = True
            else:
                ax += Fraction(a) * Fraction(x[j])
        slack, scale = INF, 1.0
        for b, side in ((self.hi[r], 1), (self.lo[r], -1)):
            if math.isfinite(b):
                scale = max(scale, abs(b))
                if not nan:                                           # (fmin passes over a NaN operand)
                    s = (Fraction(b) - ax) * side
                    slack = s if slack == INF else min(slack, s)
        return slack, scale, (None if nan else ax)

    def row_norm(self, r):
        """largest |coefficient|; None when the row holds a NaN (such a row never matches)"""
        if any(math.isnan(a) for a in self.vals[r]):
            return None
        return max([abs(a) for a in self.vals[r]], default=0.0)

    def purge(self, x, margin, max_age, dedupe_eps, min_frac):
        """one purge in the engine's order: (a) ageing, (b) dedupe against each list's kept head, (c) the min_frac decision,
        (d) compaction and re-threading.  Returns (self, rows removed)."""
        m, mut = self.M, self.mut
        keep = [True] * m
        for r in range(self.M_base, m):                                                   # (a)
            slack, scale, _ = self.slack_scale(r, x)
            if self.trace is not None:
                self.trace.append(("idle", self.tag[r] if self.tag else r, self.cols[r], self.vals[r], self.lo[r], self.hi[r], x, slack, scale))
            thr = Fraction(margin) * Fraction(scale)
            far = (slack == INF) or (slack >= thr if mut == "idle_ge" else slack > thr)
            idle = self.y[r] == 0.0 and far
            if idle:
                self.age[r] += 1
            elif mut != "age_no_reset":
                self.age[r] = 0
            keep[r] = (self.age[r] <= max_age) if mut == "keep_le" else (self.age[r] < max_age)
        nd = 0
        if dedupe_eps > 0.0:                                                               # (b)
            for s in range(len(self.heads)):
                head = self.heads[s]
                if head < 0 or not keep[head]:
                    continue
                ref = head
                for r in self.list_rows(s)[1:]:
                    if not keep[r]:
                        continue
                    if self._duplicate(r, ref, dedupe_eps):
                        nr, nh = self.row_norm(r), self.row_norm(head)
                        nh = math.nan if nh is None else nh            # (only a mutant gets here with a NaN head)
                        keep[r] = False
                        self.y[head] += self.y[r] if mut == "dedupe_no_scale" else self.y[r] * (nr / nh)
                        self.y[r] = 0.0
                        nd += 1
                    elif mut == "dedupe_vs_previous":
                        ref = r
        self.stats["deduped_rows"] += nd
        removed = keep.count(False)
        if removed < int(min_frac * m) or removed == 0:                                   # (c)
            return self, 0
        new = [-1] * m                                                                     # (d)
        k = 0
        for r in range(m):
            if keep[r]:
                new[r] = k
                k += 1
        lists = [[new[r] for r in self.list_rows(s) if keep[r]] for s in range(len(self.heads))]
        G = pick_group(self.nnz / max(m, 1))
        for name in ("cols", "vals", "lo", "hi", "y", "age") + (("tag",) if self.tag else ()):
            setattr(self, name, [v for r, v in enumerate(getattr(self, name)) if keep[r]])
        if mut == "copy_short":
            for r in range(self.M):
                if len(self.cols[r]) % G == 1:
                    self.cols[r][-1], self.vals[r][-1] = 0, 0.0
        self.prev, self._spare = [-1] * k, self.prev                  # (the engine swaps two link buffers at every compaction)
        for s, rows in enumerate(lists):
            self.heads[s] = rows[0] if rows else -1
            for a, b in zip(rows, rows[1:]):
                self.prev[a] = b
            if rows and mut == "relink_no_tail":                      # the slot keeps what the buffer held two compactions ago
                t = rows[-1]
                self.prev[t] = self._older[t] if t < len(self._older) and self._older[t] < t else -1
        self._older = self._spare
        assert self.M_base <= k
        self.stats["purges"] += 1
        self.stats["purged_rows"] += removed
        return self, removed

    def _duplicate(self, r, head, eps):
        nh = self.row_norm(head)
        if nh is None or not (nh > 0.0) or not math.isfinite(nh):
            return False
        up = math.isfinite(self.hi[head])
        bh = (self.hi[head] if up else self.lo[head]) / nh
        if not math.isfinite(bh):
            return False
        if len(self.vals[r]) != len(self.vals[head]) or math.isfinite(self.hi[r]) != up:
            return False
        nr = self.row_norm(r)
        if nr is None or not (nr > 0.0) or not math.isfinite(nr):
            return False
        br = (self.hi[r] if up else self.lo[r]) / nr
        if self.trace is not None:
            self.trace.append(("bound", self.tag[r] if self.tag else r, abs(br - bh), eps * (1.0 + abs(bh))))
        if not (abs(br - bh) <= eps * (1.0 + abs(bh))):
            return False
        diff = max([abs(a / nr - b / nh) for a, b in zip(self.vals[r], self.vals[head])], default=0.0)
        if self.trace is not None:
            self.trace.append(("coef", self.tag[r] if self.tag else r, diff, eps))
        return diff <= eps

    def lp_purge(self, x, purge_age, purge_margin, dedupe_eps, purge_min_frac, purge_min_rows):
        """ktn_lp_purge: nothing at all -- not even ageing -- with purge_age = 0 or fewer than purge_min_rows cuts"""
        if purge_age <= 0 or self.M - self.M_base < max(purge_min_rows, 1):
            return 0
        return self.purge(x, purge_margin, purge_age, dedupe_eps, purge_min_frac)[1]

    # ---- truncate ---------------------------------------------------------------------------------------------------------
    def truncate(self, nrows):
        """rows >= nrows go; every list head among them moves down its links to the first surviving row (-1: none).  The
        surviving rows keep y, age and their links."""
        assert self.M_base <= nrows <= self.M
        if self.mut != "clip_keeps_head":
            for s in range(len(self.heads)):
                r = self.heads[s]
                while r >= nrows:
                    r = self.prev[r]
                self.heads[s] = r
        for name in ("cols", "vals", "lo", "hi", "y", "age", "prev", "tag"):
            del getattr(self, name)[nrows:]

    # ---- deepest-cut selection --------------------------------------------------------------------------------------------
    def select_deepest(self, depths, flagged, cap):
        """slots that keep their flag: all when no more than `cap` are flagged (no selection), else those whose key is at least
        the cap-th largest -- ties at the threshold all stay.  key = bits of the depth, 1 for a flagged row of depth <= 0."""
        if cap <= 0 or sum(1 for f in flagged if f) <= cap:
            return [s for s, f in enumerate(flagged) if f], False
        keys = [(depth_key(d) if d > 0.0 else 1) if f else 0 for d, f in zip(depths, flagged)]
        thr = sorted(keys, reverse=True)[cap - 1]
        if self.mut == "reflag_le":
            return [s for s, k in enumerate(keys) if flagged[s] and k > thr], True
        return [s for s, k in enumerate(keys) if flagged[s] and k >= thr], True

    # ---- what the device shows --------------------------------------------------------------------------------------------
    def csr(self):
        rowptr = [0]
        for c in self.cols:
            rowptr.append(rowptr[-1] + len(c))
        return (rowptr, [j for c in self.cols for j in c], [a for v in self.vals for a in v], list(self.lo), list(self.hi))

    def list_sums(self):
        return [math.fsum(self.y[r] for r in self.list_rows(s)) for s in range(len(self.heads))]
