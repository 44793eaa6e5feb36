"""Scripts for the cut pool (test code): lists of steps -- append | set point | purge | truncate -- with all their data, built
once and run through tests/pool_ref.py on the CPU (tests/test_pool_ref.py) and through the engine next to the model on the GPU
(tests/test_gpu_pool.py).

Every threshold decision of a script is kept away from rounding, and the builder asserts it for every row of every purge:
  * idle test  slack > margin * scale:  either the row is exact by construction (coefficients, x, bounds and the margin on the
    dyadic grid 2^-10 Z, so the engine's lane-group sum is exact in any order -- slack == margin * scale is then allowed, and is
    used: `>` is strict), or |slack - margin * scale| >= 1e-6 (sum |a_j x_j| + |bound| + margin * scale);
  * dedupe tests  |br - bh| <= eps (1 + |bh|),  max |delta| <= eps:  the left side is at most eps / 2 or at least 2 eps.
No row is excluded from a comparison."""
import math
from fractions import Fraction

import numpy as np

from katana_jl_amd import instances
import pool_ref

INF = math.inf
MARGIN = 0.25
EPS = 2.0 ** -10
GRID = 1024
IDLE_REL = 1e-6
GROUPS = (4, 8, 16, 32, 64)
GROUP_MEAN = {4: 5, 8: 10, 16: 20, 32: 40, 64: 70}


def base_lp(n, m, seed, nnz_row, integer=False):
    """instances.make_lp and its rows as the pool's base rows.  integer: coefficients, bounds and cost rounded to small integers
    and the variable box opened wide (script F: one exact PDHG step)"""
    inst = instances.make_lp(n=n, m=m, seed=seed, nnz_row=nnz_row)
    if integer:
        p0 = np.rint(inst.p0 * 2.0)
        inst.p0 = np.where(p0 == 0.0, 1.0, p0)
        inst.u_constr = np.rint(inst.u_constr * 4.0)
        inst.obj_p0 = np.rint(inst.obj_p0 * 2.0)
        inst.l_var, inst.u_var = np.full(n, -2.0 ** 20), np.full(n, 2.0 ** 20)
    rp = inst.rowptr
    rows = [(inst.col[rp[i]:rp[i + 1]].tolist(), inst.p0[rp[i]:rp[i + 1]].tolist(), float(inst.l_constr[i]), float(inst.u_constr[i]))
            for i in range(inst.num_constr)]
    return inst, rows


def on_grid(v):
    return math.isfinite(v) and abs(v) <= 4096.0 and float(v * GRID).is_integer()


class Script:
    """steps: ("append", rows, ids, tags) | ("point", x, y) | ("purge",) | ("truncate", nrows).  `after[i]`: tags of the rows left
    after step i (model).  `groups`: lanes per row of every purge that ran (from the mean row length at that call)."""

    def __init__(self, name, inst_kw, n_lists, **params):
        self.name, self.inst_kw, self.n_lists = name, inst_kw, n_lists
        self.params = dict(purge_age=1, purge_margin=MARGIN, dedupe_eps=EPS, purge_min_frac=0.0, purge_min_rows=1, lp_dual_inherit=1)
        self.params.update(params)
        self.inst, self.base = base_lp(**inst_kw)
        self.n = self.inst.n
        self.steps, self.after, self.groups, self.removed = [], [], [], []
        self.model = self.new_model()
        self.ytab = {}
        self.exact_ties = 0

    def new_model(self, mut=None):
        m = pool_ref.PoolRef(self.base, self.n_lists, mut=mut)
        m.tag = ["base%d" % i for i in range(m.M)]
        return m

    # ---- building (the model runs along: the builder knows the pool at every step) ----
    def append(self, rows, ids=None, y=None):
        """rows: [(tag, cols, vals, lo, hi)]; y: the multiplier every later set point gives the row (by tag)"""
        ids = [-1] * len(rows) if ids is None else list(ids)
        tags = [r[0] for r in rows]
        assert not set(tags) & set(self.model.tag), "tags are unique"
        body = [tuple(r[1:]) for r in rows]
        self.steps.append(("append", body, ids, tags))
        apply_step(self.model, self.steps[-1], self.params)
        for t, v in zip(tags, y if y is not None else [0.0] * len(rows)):
            self.ytab[t] = float(v)
        self._done()

    def point(self, x, y_over=None):
        y = [dict(self.ytab, **(y_over or {})).get(t, 0.0) for t in self.model.tag]
        self.steps.append(("point", [float(v) for v in x], y))
        apply_step(self.model, self.steps[-1], self.params)
        self._done()

    def purge(self):
        m = self.model
        ran = self.params["purge_age"] > 0 and m.M - m.M_base >= max(self.params["purge_min_rows"], 1)
        if ran:
            self.groups.append(pool_ref.pick_group(m.nnz / max(m.M, 1)))
        m.trace = []
        self.steps.append(("purge",))
        self.removed.append(apply_step(m, self.steps[-1], self.params))
        self._check_gaps(m.trace)
        m.trace = None
        self._done()

    def truncate(self, nrows):
        self.steps.append(("truncate", int(nrows)))
        apply_step(self.model, self.steps[-1], self.params)
        self._done()

    def _done(self):
        self.after.append(list(self.model.tag))

    def _check_gaps(self, trace):
        """the condition on the inputs: every decision of this purge is exact by construction or away from its threshold"""
        margin, eps = self.params["purge_margin"], self.params["dedupe_eps"]
        for rec in trace:
            if rec[0] == "idle":
                _, tag, cols, vals, lo, hi, x, slack, scale = rec
                if slack == INF:
                    continue
                thr = Fraction(margin) * Fraction(scale)
                exact = (len(cols) <= 512 and on_grid(margin) and all(on_grid(a) for a in vals) and all(on_grid(x[j]) for j in cols)
                         and all(on_grid(b) for b in (lo, hi) if math.isfinite(b)))
                if exact:
                    self.exact_ties += slack == thr
                    continue
                mag = sum(abs(Fraction(a) * Fraction(x[j])) for j, a in zip(cols, vals)) + max(abs(b) for b in (lo, hi) if math.isfinite(b)) + thr
                assert abs(slack - thr) >= Fraction(IDLE_REL) * mag, (self.name, tag, float(slack), float(thr))
            else:
                _, tag, q, bound = rec
                assert q <= 0.5 * bound * (1 + 1e-6) or q >= 2.0 * bound * (1 - 1e-6), (self.name, rec)


def apply_step(model, step, params):
    """one step on a model (a PoolRef with a `tag` list riding along); returns what the engine's call returns"""
    kind = step[0]
    if kind == "append":
        _, rows, ids, tags = step
        model.append(rows, ids, params["lp_dual_inherit"])
        model.tag.extend(tags)
        return None
    if kind == "point":
        model.x, model.y = list(step[1]), list(step[2])
        assert len(model.y) == model.M
        return None
    if kind == "purge":
        return model.lp_purge(model.x, params["purge_age"], params["purge_margin"], params["dedupe_eps"], params["purge_min_frac"],
                              params["purge_min_rows"])
    if kind == "truncate":
        model.truncate(step[1])
        return None
    if kind == "step":                                                     # one PDHG step: the pool does not change
        return None
    raise ValueError(kind)


def run_model(script, mut=None):
    """the script through a fresh model: yields (step index, step, model, returned) after every step"""
    m = script.new_model(mut)
    for i, step in enumerate(script.steps):
        out = apply_step(m, step, script.params)
        yield i, step, m, out


def snapshot(m):
    """everything the engine shows of the pool: rows, bounds, multipliers (bit patterns), counters"""
    bits = lambda v: [np.float64(a).tobytes() for a in v]
    rowptr, col, val, lo, hi = m.csr()
    return (rowptr, col, bits(val), bits(lo), bits(hi), bits(m.y), sorted(m.stats.items()))


# ---- row helpers -------------------------------------------------------------------------------------------------------------
def grid_x(n, shift=0):
    return [((3 * j + shift) % 9 - 4) / 4.0 for j in range(n)]


def ax_exact(cols, vals, x):
    return sum(Fraction(a) * Fraction(x[j]) for j, a in zip(cols, vals))


def upper_row(tag, cols, vals, x, slack):
    """a'x <= a'x + slack at x (all on the grid)"""
    return (tag, list(cols), list(vals), -INF, float(ax_exact(cols, vals, x) + Fraction(slack)))


def idle_slack(cols, vals, x):
    """a power of two s with s > MARGIN * max(1, |a'x + s|): the row  a'x <= a'x + s  is idle at x"""
    s = 8.0
    while s < abs(ax_exact(cols, vals, x)):
        s *= 2.0
    return s


PATTERN = (4.0, 2.0, -1.0, 3.0, 1.0, -2.0, 2.0, -3.0)


def pattern_row(length, start, n):
    """`length` entries on the columns start, start + 1, ... (mod n: a long row visits a column more than once); |a| <= 4, a_0 = 4"""
    return [(start + e) % n for e in range(length)], [PATTERN[e % len(PATTERN)] for e in range(length)]


# ---- script A: ageing --------------------------------------------------------------------------------------------------------
def script_ageing(purge_age, variant="plain"):
    """idle rows, a row made tight once, y != 0, inside the margin, exactly on the margin, two finite sides, a NaN bound, an empty
    row, rows with arbitrary floats away from the threshold.  variant "min_frac": a call declines to compact; "min_rows": every
    call is a no-op."""
    p = purge_age
    kw = dict(plain={}, min_frac=dict(purge_min_frac=0.4), min_rows=dict(purge_min_rows=1000))[variant]
    S = Script("ageing/p%d/%s" % (p, variant), dict(n=12, m=6, seed=5, nnz_row=4), 2, purge_age=p, **kw)
    n, x = S.n, grid_x(12)
    rng = np.random.default_rng(17)
    rows, y = [], []

    def add(row, yv=0.0):
        rows.append(row); y.append(yv)

    for i in range(3):
        c, v = pattern_row(3 + i, i, 10)
        add(upper_row("idle%d" % i, c, v, x, idle_slack(c, v, x)))
    c, v = [11, 2, 5], [1.0, 2.0, -1.0]                                  # column 11 belongs to this row alone
    add(upper_row("reset", c, v, x, 8.0))
    c, v = pattern_row(4, 3, 10)
    add(upper_row("has_y", c, v, x, idle_slack(c, v, x)), -0.75)
    c, v = [0, 3], [-4.0, 1.0]                                            # a'x = 3, hi = 4: slack 1 == MARGIN * scale (scale 4)
    assert ax_exact(c, v, x) == 3
    add(("on_margin", c, v, -INF, 4.0))
    c2, v2 = pattern_row(5, 2, 10)
    add(upper_row("in_margin", c2, v2, x, 0.125))
    c3, v3 = pattern_row(3, 6, 10)
    a3 = ax_exact(c3, v3, x)
    add(("both_idle", c3, v3, float(a3 - 16), float(a3 + 16)))
    add(("both_tight", c3, v3, float(a3 - Fraction(1, 8)), float(a3 + 16)))
    add(("nan_bound", [1, 4], [1.0, 1.0], -INF, math.nan))
    add(("empty_idle", [], [], -INF, 8.0))
    add(("empty_tight", [], [], -INF, 0.0))
    for i, rel in enumerate((1e-3, -1e-3, 0.5, -0.5)):                    # arbitrary floats: slack = thr (1 + rel)
        c = sorted(rng.choice(10, size=4, replace=False).tolist())
        v = rng.standard_normal(4).tolist()
        xs = float(sum(a * x[j] for j, a in zip(c, v)))
        hi = xs + 3.0
        hi = xs + MARGIN * max(1.0, abs(hi)) * (1.0 + rel)
        hi = xs + MARGIN * max(1.0, abs(hi)) * (1.0 + rel)
        add(("float%d" % i, c, v, -INF, hi))
    ids = [-1] * len(rows)
    ids[0], ids[4] = 0, 1
    S.append(rows, ids, y)
    t = max(p - 1, 1)                                                      # the call at which "reset" is tight
    x_tight = list(x)
    x_tight[11] += 8.0
    calls = t + p + 1
    S.expect = dict(reset_tight_at=t, reset_gone_at=t + p, calls=calls)
    for call in range(1, calls + 1):
        if variant == "min_frac" and call == 2:                            # a second batch, one call younger than the first
            late = []
            for i in range(3):
                c, v = pattern_row(2 + i, 4 + i, 10)
                late.append(upper_row("late%d" % i, c, v, x, idle_slack(c, v, x)))
            S.append(late)
        S.point(x_tight if call == t else x)
        S.purge()
    if variant == "min_frac":                                              # call 2 declines (8 of 25 rows < 0.4 * 25), call 3 takes 12
        assert S.removed == [0, 0, 12, 0], S.removed
    return S


# ---- script B: dedupe --------------------------------------------------------------------------------------------------------
HEAD = ([1, 3, 4, 6], [4.0, 2.0, -1.0, 3.0], 8.0)                          # normalised by 4: bound 2


def script_dedupe(eps=EPS):
    """two lists of five around the same head geometry, a list whose head goes by age, an all-zero head, a NaN head; multipliers
    on every duplicate; then one new cut per id (dual inheritance through the re-threaded lists)"""
    S = Script("dedupe/eps%g" % eps, dict(n=10, m=6, seed=9, nnz_row=4), 5, dedupe_eps=eps)
    x = grid_x(10)
    hc, hv, hb = HEAD
    e = EPS
    up = lambda tag, v, b, c=hc: (tag, list(c), list(v), -INF, float(b))
    scaled = lambda f: [f * a for a in hv]
    coef2 = [hv[0], hv[1] + 4.0 * 2 * e, hv[2], hv[3]]
    # list 0, oldest first: the 2 eps coefficient row twice (only the head is the yardstick), within eps / 2, x3, the head
    l0 = [up("l0_coef2_older", coef2, hb), up("l0_coef2", coef2, hb), up("l0_within", [hv[0], hv[1], hv[2] - 4.0 * e / 2, hv[3]], hb),
          up("l0_times3", scaled(3.0), 3.0 * hb), up("l0_head", hv, hb)]
    # list 1: a shorter row, the opposite side, the bound at 2 eps (1 + |bh|), x0.5, the head
    l1 = [up("l1_short", hv[:3], hb, hc[:3]), ("l1_opposite", list(hc), list(hv), hb, INF), up("l1_bound2", hv, hb + 4.0 * 2 * e * 3.0),
          up("l1_half", scaled(0.5), 0.5 * hb), up("l1_head", hv, hb)]
    # list 2: exact duplicates under a head that is idle and goes by age; list 3: all-zero rows; list 4: a NaN in the head
    z = [0.0, 0.0, 0.0]
    l2 = [up("l2_dup_a", hv, hb), up("l2_dup_b", scaled(3.0), 3.0 * hb), None, None, upper_row("l2_head_idle", hc, hv, x, idle_slack(hc, hv, x))]
    l3 = [up("l3_zero_old", z, 1.0, [0, 1, 2]), None, None, None, up("l3_zero_head", z, 1.0, [0, 1, 2])]
    l4 = [up("l4_dup", hv, hb), None, None, up("l4_half", scaled(0.5), 0.5 * hb), up("l4_nan_head", [hv[0], math.nan, hv[2], hv[3]], hb)]
    yv = -0.25
    for depth in range(5):                                                 # one append per depth: one cut per id and call
        rows, ids, y = [], [], []
        for s, lst in enumerate((l0, l1, l2, l3, l4)):
            if lst[depth] is not None:
                rows.append(lst[depth]); ids.append(s)
                y.append(0.0 if lst[depth][0] == "l2_head_idle" else yv)
                yv -= 0.25
        S.append(rows, ids, y)
    S.point(x)
    S.purge()
    tail = [up("new%d" % s, [1.0, 1.0], 5.0, [0, 2]) for s in range(5)]
    S.append(tail, list(range(5)))
    return S


def script_relink():
    """three compactions: a list tail whose link slot, two link buffers back, pointed at a row that now duplicates the list's
    head but belongs to another list -- only a tail written as -1 keeps that row out of the list (k_purge_relink).  List 2 is
    one cut, twice base row 0: a tail whose slot was left holding 0 would draw that base row into the list, and dedupe drops it"""
    S = Script("relink", dict(n=10, m=6, seed=9, nnz_row=4), 3)
    x = grid_x(10)
    hc, hv, hb = HEAD
    up = lambda tag, v, b, c=hc: (tag, list(c), list(v), -INF, float(b))
    junk = lambda tag: upper_row(tag, [0, 2], [1.0, 1.0], x, 8.0)
    other = [1.0, -4.0, 2.0, 1.0]
    bc, bv, _, bhi = S.base[0]
    S.append([up("c", other, 3.0), ("twice_base0", list(bc), [2.0 * a for a in bv], -INF, 2.0 * bhi)], [1, 2], [-0.5, -0.5])
    S.append([up("d", [3.0 * a for a in hv], 3.0 * hb)], [1], [-1.5])      # 3 x the head of list 0, in list 1
    S.append([junk("junk0")])
    S.append([up("e", [2.0, 1.0, 4.0, -1.0], 6.0)], [1], [-0.75])
    S.append([junk("junk1")])
    S.append([up("a", hv, hb)], [0], [-0.25])
    for k in range(3):
        S.point(x)
        S.purge()
        assert S.removed[-1] >= 1
        S.append([junk("junk%d" % (k + 2))])
    S.append([up("new%d" % s, [1.0, 1.0], 5.0, [0, 2]) for s in range(3)], [0, 1, 2])
    assert "d" in S.model.tag
    return S


# ---- script C: lane groups and workgroup edges -------------------------------------------------------------------------------
def script_groups(G):
    """ageing and dedupe material with row lengths 0, 1, G - 1, G, G + 1, 2 G + 1 at a mean row length that selects G lanes per
    row, more rows than one workgroup holds, kept and dropped rows alternating across the workgroup boundary"""
    nbase = 2 if G == 64 else 6
    S = Script("groups/G%d" % G, dict(n=80, m=nbase, seed=G, nnz_row=min(8, G)), 6)
    n, x = S.n, grid_x(80)
    lens = (0, 1, G - 1, G, G + 1, 2 * G + 1)
    per_wg = 256 // G
    cycles = max(3, -(-(2 * per_wg + 4) // 6))
    cut = 0

    def fated(tag, L, keep):
        c, v = pattern_row(L, 7 * cut, n)
        return upper_row(tag, c, v, x, idle_slack(c, v, x)), (-(1 + cut % 5) / 4.0 if keep else 0.0)

    for k in range(cycles):                                                # kept (y != 0) and idle rows in turn
        rows, y = [], []
        for L in lens:
            r, yv = fated("c%d_len%d" % (k, L), L, (cut // 6 + cut) % 2 == 1)
            rows.append(r); y.append(yv); cut += 1
        S.append(rows, None, y)
    e = EPS
    for k, kind in enumerate(("times3", "near", "head")):                  # three cuts per list: x3 of the head, 2 eps off, the head
        rows, y = [], []
        for L in lens:
            c, v = pattern_row(L, 3 + L, n)
            b = 8.0
            if kind == "times3":
                v, b = [3.0 * a for a in v], 24.0
            elif kind == "near" and L >= 2:
                v[-1] += (-1.0 if v[-1] >= 4.0 else 1.0) * 4.0 * 2 * e     # the LAST entry: the lane (L - 1) mod G (norm stays 4)
            elif kind == "near":
                b += 4.0 * 2 * e * 3.0
            rows.append(("%s_len%d" % (kind, L), c, v, -INF, b)); y.append(-0.25 * (k + 1) - L / 256.0)
        S.append(rows, list(range(6)), y)
    # fillers bring the mean row length (base rows included) to GROUP_MEAN[G]
    target, fill, M, nnz = GROUP_MEAN[G], [], S.model.M, S.model.nnz
    while True:
        need = target * (M + 1) - nnz
        L = min(2 * G, need)
        assert L >= 0
        c, v = pattern_row(L, 11 * len(fill), n)
        fill.append(upper_row("fill%d" % len(fill), c, v, x, idle_slack(c, v, x)))
        M, nnz = M + 1, nnz + L
        if L == need:
            break
    S.append(fill, None, [-0.5] * len(fill))
    assert S.model.nnz == target * S.model.M and S.model.M * G > 256
    S.point(x)
    S.purge()
    assert S.groups == [G], (S.groups, G)
    b = per_wg - nbase                                                     # first cut row of the second workgroup
    if b >= 1:
        kept = set(S.after[-1])
        t0, t1 = S.after[-3][per_wg - 1], S.after[-3][per_wg]
        assert (t0 in kept) != (t1 in kept), (G, t0, t1)
    tail = [("new_len%d" % L, [0, 2], [1.0, 1.0], -INF, 5.0) for L in lens]
    S.append(tail, list(range(6)))
    S.point(x)
    S.purge()
    return S


# ---- script T: truncate ------------------------------------------------------------------------------------------------------
def script_truncate():
    """append g -> truncate -> append g again (the row index comes back); a head two links above the cut; then dedupe, relink
    and inheritance over the clipped lists"""
    S = Script("truncate", dict(n=10, m=6, seed=9, nnz_row=4), 3)
    x = grid_x(10)
    hc, hv, hb = HEAD
    up = lambda tag, v, b, c=hc: (tag, list(c), list(v), -INF, float(b))
    R = S.model.M
    S.append([up("g0", hv, hb)], [0], [-0.5])                              # lands at R
    S.truncate(R)
    assert S.model.heads == [-1, -1, -1]
    S.append([up("g1", hv, hb)], [0], [-0.5])                              # R again: its link must be -1, not R
    assert S.model.prev[R] == -1
    S.append([up("h0", [1.0, 4.0, 2.0, -1.0], 3.0)], [1], [-1.0])
    S.append([up("g2", [3.0 * a for a in hv], 3.0 * hb), up("h1", [2.0, 4.0, 2.0, -1.0], 3.0)], [0, 1], [-0.25, -2.0])
    S.append([up("g3", hv, hb), up("h2", [3.0, 4.0, 2.0, -1.0], 3.0), up("k0", [1.0, 1.0], 2.0, [0, 1])], [0, 1, 2], [-0.125, -3.0, -0.5])
    S.point(x)
    S.truncate(R + 2)                                                      # g2, h1, g3, h2, k0 go: heads g1 (two links down), h0, none
    assert S.model.heads == [R, R + 1, -1]
    S.append([up("g4", [0.5 * a for a in hv], 0.5 * hb), up("h3", [5.0, 4.0, 2.0, -1.0], 3.0), up("k1", [1.0, 1.0], 2.0, [0, 1])], [0, 1, 2])
    S.append([upper_row("junk", [0, 2], [1.0, 1.0], x, 8.0)])
    S.point(x, dict(g4=-0.375, h3=-0.625, k1=-0.875))
    S.purge()                                                              # g1 duplicates g4: dropped, its multiplier moves
    assert S.removed[-1] == 2 and "g1" not in S.model.tag
    S.append([up("g5", [1.0, 1.0], 5.0, [0, 2]), up("h4", [1.0, 1.0], 5.0, [0, 2]), up("k2", [1.0, 1.0], 5.0, [0, 2])], [0, 1, 2])
    return S


# ---- script F: the column mirror ---------------------------------------------------------------------------------------------
BIG = 2.0 ** 53


def script_mirror(J=None):
    """integer rows, multipliers and cost, a wide variable box, x = 0: one plain step with tau = 1 leaves x_j = (A'y)_j - c_j,
    exact in any order -- except in column `order_col`, whose three newest entries (1, 2^53, -2^53) sum differently in row order and
    in the order the append-only update receives them (the first of the two new rows holds the column in its LAST entry, which
    its lane group reaches one trip later than the second row reaches its first).  ("step",) steps: after a fresh sort, after each of three appends, after a purge, after a
    truncate, after one append that gives column 0 130 entries."""
    if J is None:                                                          # the first column whose sum tells the orders apart
        return next(S for S in (script_mirror(j) for j in range(1, 12)) if S is not None)
    S = Script("mirror", dict(n=12, m=6, seed=3, nnz_row=4, integer=True), 0)
    rng = np.random.default_rng(4)
    S.order_col = J
    count = [0]

    def block(nrows, tag, first_col=None):
        rows, y = [], []
        for i in range(nrows):
            c = sorted(rng.choice(12, size=3, replace=False).tolist())
            if first_col is not None and first_col not in c:
                c = [first_col] + c[1:]
            v = rng.integers(1, 4, size=len(c)).astype(float).tolist()
            rows.append(("%s%d" % (tag, i), c, v, -INF, float(rng.integers(4, 9))))
            count[0] += 1
            y.append(0.0 if J in c else float((count[0] * 7) % 5 - 2))
        return rows, y

    for i, (c, v, lo, hi) in enumerate(S.base):
        S.ytab["base%d" % i] = 0.0 if J in c else float(i % 3 - 1)
    x = [0.0] * S.n
    S.csc = []                                                             # (sorts, merges) after every ("step",)

    def step(sorts, merges):
        S.point(x)
        S.steps.append(("step",)); S._done()
        prev = S.csc[-1] if S.csc else (0, 0)
        S.csc.append((prev[0] + sorts, prev[1] + merges))

    step(1, 0)
    S.append(block(5, "a")[0])
    step(0, 1)
    S.ytab.update({t: (0.0 if J in S.model.cols[i] else float((i * 7) % 5 - 2)) for i, t in enumerate(S.model.tag) if t[0] == "a"})
    others = [c for c in range(12) if c != J]
    S.append([("one", [J] + others[8:10], [1.0, 1.0, 2.0], -INF, 8.0)], None, [1.0])   # the column's last old entry: product 1
    step(0, 1)
    order = [("ordA", others[:4] + [J], [1.0, 2.0, 1.0, 3.0, BIG], -INF, 8.0),
             ("ordB", [J] + others[4:8], [-BIG, 1.0, 2.0, 1.0, 1.0], -INF, 8.0)]
    S.append(order, None, [1.0, 1.0])
    step(0, 1)
    m, y = S.model, S.steps[-2][2]
    G = pool_ref.pick_group(m.nnz / S.n)
    rowwise = pool_ref.mirror_aty(m, y, G)[J]
    if pool_ref.mirror_aty(m, y, G, {J: [m.M - 1, m.M - 2]})[J] == rowwise:   # this column's lane layout hides the order
        return None
    S.purge()
    assert S.removed[-1] >= 1 and "ordA" in S.model.tag
    step(1, 0)
    S.truncate(S.model.M - 2)
    step(1, 0)
    wide = block(130, "wide", first_col=0)[0]
    S.append(wide, None, [float(i % 3 - 1) for i in range(130)])
    step(0, 1)
    return S


ALL_BUILDERS = ([lambda p=p: script_ageing(p) for p in (1, 2, 3)]
                + [lambda: script_ageing(2, "min_frac"), lambda: script_ageing(2, "min_rows")]
                + [lambda: script_dedupe(EPS), lambda: script_dedupe(0.0), script_relink, script_truncate, script_mirror]
                + [lambda G=G: script_groups(G) for G in GROUPS])
_cache = []


def all_scripts():
    """every script, built once (the reference the tiers share; nothing changes a built script)"""
    if not _cache:
        _cache.extend(b() for b in ALL_BUILDERS)
    return _cache


# ---- scripts D and E: the engine's own lists and the deepest-cut selection ---------------------------------------------------
F_TOL_E = -0.25                       # script E sweeps with a NEGATIVE f_tol: a row inside its bound by less than 0.25 is flagged


class EngineCase:
    """a small separable NLP (40 NL rows of 4 atoms) whose upper bounds are set from the reference's g at x1, so that every
    row's violation depth there is a designed number: rows 0 .. 29 violated by 0.05 (1 + i), the rest satisfied by 1"""

    def __init__(self, ties=False):
        import sep_ref
        self.sep_ref = sep_ref
        inst = instances.make_instance(n=24, m_nl=40, k=4, m_lin=6, family="explog", seed=11)
        self.x1 = np.clip(inst.xhat + 0.5, inst.l_var, inst.u_var)
        self.x2 = self.x1.copy()
        self.x2[:6] -= 0.2
        self.x3 = inst.xhat - 2.0         # (only the LP rows are evaluated there: a point at which some cuts are slack)
        nl = inst.m_lin + np.arange(inst.m_nl)
        if ties:                      # rows 25 and 33 become copies of row 22: three equal rows
            rp = inst.rowptr
            for dst in (25, 33):
                for name in ("col", "kind", "p0", "p1"):
                    getattr(inst, name)[rp[nl[dst]]:rp[nl[dst] + 1]] = getattr(inst, name)[rp[nl[22]]:rp[nl[22] + 1]]
                inst.rconst[nl[dst]] = inst.rconst[nl[22]]
        g = self.ref(inst, self.x1).g[nl]
        depth = np.where(np.arange(inst.m_nl) < 30, 0.05 * (1 + np.arange(inst.m_nl)), -1.0)
        if ties:
            depth[[25, 33]] = depth[22]
            depth[35] = -0.1          # inside its bound, but by less than |F_TOL_E|: flagged, depth <= 0
        inst.u_constr[nl] = g - depth
        inst.l_constr[nl] = -np.inf
        self.inst, self.nl = inst, nl

    def ref(self, inst, x):
        return self.sep_ref.rows_ref_f64(inst.rowptr, inst.col, inst.kind, inst.p0, inst.p1, inst.rconst, x)

    def depths(self, x, f_tol):
        """(depth per NL slot, flagged, error bound) from the reference; asserts that no verdict is within the error of f_tol"""
        R = self.ref(self.inst, x)
        g, e = R.g[self.nl], R.e_g[self.nl]
        d = np.maximum(g - self.inst.u_constr[self.nl], self.inst.l_constr[self.nl] - g)
        assert np.all(np.abs(d - f_tol) > 1e-6 + 4 * e), "a verdict too close to f_tol"
        return d, d > f_tol, e, R

    def cut_rows(self, x, slots):
        """the cuts of the NL slots `slots` at x as the reference gives them (for the builders' gap check; the GPU tier feeds the
        model the rows the engine returned)"""
        inst, rp, R = self.inst, self.inst.rowptr, self.ref(self.inst, x)
        out = []
        for s in slots:
            r = self.nl[s]
            out.append((inst.col[rp[r]:rp[r + 1]].tolist(), R.jac[rp[r]:rp[r + 1]].tolist(), float(inst.l_constr[r] - R.b[r]), float(inst.u_constr[r] - R.b[r])))
        return out, R


def engine_y(i, m_base):
    """the multiplier the set points of script D give LP row i"""
    return 0.0 if i < m_base or i % 3 == 1 else -(1 + i % 4) / 4.0


ENGINE_EPS = 2.0 ** -20               # (the cuts of two nearby points differ by O(1e-3): far outside, exact repeats far inside)
ENGINE_PARAMS = dict(purge_age=1, purge_margin=MARGIN, dedupe_eps=ENGINE_EPS, purge_min_frac=0.0, purge_min_rows=1, cut_cap_factor=0.0)


def check_trace_gaps(trace, margin, what):
    """the gap conditions of Script._check_gaps for rows with arbitrary floats (script D's cuts)"""
    for rec in trace:
        if rec[0] == "idle":
            _, tag, cols, vals, lo, hi, x, slack, scale = rec
            if slack == INF:
                continue
            thr = Fraction(margin) * Fraction(scale)
            mag = sum(abs(Fraction(a) * Fraction(x[j])) for j, a in zip(cols, vals)) + max(abs(b) for b in (lo, hi) if math.isfinite(b)) + thr
            assert abs(slack - thr) >= Fraction(IDLE_REL) * mag, (what, tag, float(slack), float(thr))
        else:
            _, tag, q, bound = rec
            assert q <= 0.5 * bound * (1 + 1e-6) or q >= 2.0 * bound * (1 - 1e-6), (what, rec)


def engine_lists_plan(inherit):
    """script D on the CPU with the reference's cuts: the slots every sweep must cut, and the gap conditions of the purge.
    Returns (case, [slots of sweep 1, 2, 3], model)."""
    C = EngineCase()
    inst = C.inst
    rp = inst.rowptr
    base = [(inst.col[rp[i]:rp[i + 1]].tolist(), inst.p0[rp[i]:rp[i + 1]].tolist(), float(inst.l_constr[i] - inst.rconst[i]),
             float(inst.u_constr[i] - inst.rconst[i])) for i in range(inst.m_lin)]
    m = pool_ref.PoolRef(base, inst.m_nl)
    sweeps = []
    for x in (C.x1, C.x2):
        slots = np.flatnonzero(C.depths(x, 1e-6)[1]).tolist()
        m.append(C.cut_rows(x, slots)[0], slots, inherit)
        sweeps.append(slots)
    m.y = [engine_y(i, m.M_base) for i in range(m.M)]
    m.trace = []
    removed = m.purge(C.x3.tolist(), MARGIN, 1, ENGINE_EPS, 0.0)[1]
    check_trace_gaps(m.trace, MARGIN, "engine lists")
    m.trace = None
    slots = np.flatnonzero(C.depths(C.x1, 1e-6)[1]).tolist()
    m.append(C.cut_rows(C.x1, slots)[0], slots, inherit)
    sweeps.append(slots)
    return C, sweeps, m, removed


def selection_plan(cap=8):
    """script E on the CPU: (case, depths, flagged, kept slots, selected?) at x1 with f_tol = F_TOL_E; three rows tie at the
    threshold, one flagged row has depth <= 0; every other depth is away from the threshold by far more than the reference's
    error"""
    C = EngineCase(ties=True)
    d, flagged, e, _ = C.depths(C.x1, F_TOL_E)
    kept, selected = pool_ref.PoolRef([], 0).select_deepest(d.tolist(), flagged.tolist(), cap)
    if selected:
        thr = sorted(d[flagged], reverse=True)[cap - 1]
        tied = np.flatnonzero(flagged & (d == thr))
        assert tied.tolist() == [22, 25, 33], tied
        others = flagged & (d != thr)
        assert np.all(np.abs(d[others] - thr) > 1e-3), "a depth too close to the threshold"
        assert np.count_nonzero(flagged & (d <= 0.0)) == 1
    return C, d, flagged, kept, selected
