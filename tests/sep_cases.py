"""Seeded builders of separable-row test models with mixed atom kinds (test code; reference: tests/sep_ref.py).

`make_case` returns a SepCase: the arrays of an NLPDescription, the box, the evaluation point x and what the reference
needs to know about every row.  Rows, in this order: a third of the special rows, half of the bulk rows, a third of the
specials, the other half, the rest of the specials.

* Bulk rows draw their atoms from all four kinds in random storage order.  Row i uses the kinds of subset 1 + (i mod 15) of
  {LIN, QUAD, EXP, NEGLOG} -- every non-empty subset, LIN-only included (the description is built directly with
  row_linear = 0 for it) -- each kind of the subset at least once where the row is long enough.  Columns are sorted and
  distinct by default (one per stratum of the row's column range), may be confined to a range, skip a gap, be forced onto
  given columns, repeated, or stored unsorted.  Weights p0 have either sign (these cases evaluate and cut: no convexity).
* Sides cycle through (-inf, ub], [lb, +inf), [lb, ub] and equality; satisfied, violated above, violated below.
* Threshold rows: two dyadic atoms (a LIN and a QUAD, each worth 1 at x = 1.0 and x = 0.5) plus a dyadic rconst with f_tol = 2^-20, so g is exact
  in every summation order: exactly at ub + f_tol, one ulp above it, exactly at lb - f_tol, one ulp below it.
* Edge rows: one non-finite source each, at the first, a middle and the last entry: NEGLOG at s < 0 (a NaN value with all
  partials finite: the cut is appended with NaN bounds, maxviol is +inf) with edges >= 1; with edges = 2 also NEGLOG at
  s = 0 and EXP overflow (a non-finite coefficient of a violated row: status Error, nothing appended).  edges = 0 has
  neither, so maxviol is finite there -- and comes from a lower-sided row, whose offsets are three times the others'.
* A round_coefs row whose largest coefficient exceeds the others by more than cut_coef_rng; a pad_zero row (nonlinear
  separable objective over fewer than n columns: the epigraph row) whose partials are all negative, so that only the
  implicit zero coefficients make round_coefs drop them.

Input conditions, asserted by `check_conditions` (tests/test_sep_ref.py runs it on every case the GPU file uses):
  1. every finite term of a row is at least 1e3 x the row's value bound E_g (sep_ref): a dropped, doubled or misplaced entry
     cannot hide inside the tolerance;
  2. every row that is not a threshold row has |g - (ub + f_tol)| and |g - (lb - f_tol)| >= 10 x E_g: the violated set is
     unambiguous;
  3. every round_coefs decision `der + cut_coef_rng < max` has a margin of 1e3 x the bounds of the two partials.
"""
import numpy as np

import sep_ref
from sep_ref import LIN, QUAD, EXP, NEGLOG, F_TOL, U

INF = float("inf")
ROW_SEP, ROW_TAPE = 0, 1
OP_CONST, OP_VAR, OP_ADD, OP_SUB, OP_MUL = 0, 1, 2, 3, 4
_SUBSETS = [[k for k in range(4) if (s >> k) & 1] for s in range(1, 16)]


class SepCase:
    pass


def _bulk(rng, lens, rlo, rhi, gap_lo, gap_len):
    """vectorised mixed rows: (rowptr, col, kind), sorted distinct columns, kinds in random storage order"""
    m = len(lens)
    lens = np.asarray(lens, dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    nnz = int(rowptr[-1])
    rows = np.repeat(np.arange(m), lens)
    j = np.arange(nnz) - rowptr[:-1][rows]                      # position inside the row
    k = lens[rows]
    width = (rhi - rlo - gap_len)[rows]
    assert np.all(width >= k), "a row longer than its column range"
    lo = (j * width) // k
    hi = ((j + 1) * width) // k
    v = lo + np.floor(rng.random(nnz) * (hi - lo)).astype(np.int64)
    v = np.minimum(v, hi - 1) + rlo[rows]
    col = v + np.where(v >= gap_lo[rows], gap_len[rows], 0)
    # kinds: position j takes member j of the row's subset while j < |subset|, then a random member; then shuffled inside the row
    sub = np.arange(m) % 15
    size = np.array([len(s) for s in _SUBSETS])[sub]
    table = np.array([[s[t % len(s)] for t in range(4)] for s in _SUBSETS])
    pick = np.where(j < size[rows], j % 4, rng.integers(0, 4, nnz))
    kp = table[sub[rows], pick % 4]
    perm = np.lexsort((rng.random(nnz), rows))
    kind = kp[perm]
    return rowptr, col, kind


def _params(rng, kind, xv):
    nnz = len(kind)
    sgn = np.where(rng.random(nnz) < 0.3, -1.0, 1.0)
    p0 = sgn * rng.uniform(0.5, 2.0, nnz)
    p1 = np.zeros(nnz)
    m = kind == QUAD
    p1[m] = xv[m] + np.where(rng.random(m.sum()) < 0.5, -1.0, 1.0) * rng.uniform(0.3, 1.5, m.sum())
    m = kind == EXP
    p1[m] = np.where(rng.random(m.sum()) < 0.5, -1.0, 1.0) * rng.uniform(0.3, 1.5, m.sum())
    m = kind == NEGLOG
    p1[m] = rng.uniform(2.5, 3.5, m.sum())                      # the shift lies beyond the box [-1, 1]
    return p0, p1


def _row(col, kind, p0, p1, rconst=0.0, lb=-INF, ub=INF, tag="", thr=False, row_kind=ROW_SEP, linear=0, tape=None):
    return dict(col=np.asarray(col, dtype=np.int64), kind=np.asarray(kind, dtype=np.int64), p0=np.asarray(p0, dtype=float),
                p1=np.asarray(p1, dtype=float), rconst=float(rconst), lb=float(lb), ub=float(ub), tag=tag, thr=thr,
                row_kind=row_kind, linear=linear, tape=tape)


def _g64(r, x):
    val, _ = sep_ref.atoms_f64(r["kind"], r["p0"], r["p1"], x[r["col"]])
    with np.errstate(all="ignore"):
        return float(np.sum(val) + r["rconst"])


def _mixed_row(rng, x, cols, sub=14):
    cols = np.sort(np.asarray(cols, dtype=np.int64))
    s = _SUBSETS[sub]
    kind = np.array([s[t % len(s)] for t in range(len(cols))])
    kind = kind[rng.permutation(len(cols))]
    p0, p1 = _params(rng, kind, x[cols])
    return cols, kind, p0, p1


def _specials(rng, x, cA, cB, edges, edge_len, edge_cols, only=None):
    """threshold, edge and round_coefs rows.  only = (source, position, violated): that single non-finite row instead of the
    edge rows of `edges`; violated=False makes it lower-sided, so its value +inf satisfies it (the flag is set, no Error)"""
    out = []
    e = 2.0 ** -51                                              # one ulp in [2, 4)
    for tag, rc, lb, ub in (("thr_at_ub", 0.5 + F_TOL, -INF, 2.5), ("thr_above_ub", 0.5 + F_TOL + e, -INF, 2.5),
                            ("thr_at_lb", 0.5 - F_TOL, 2.5, INF), ("thr_below_lb", 0.5 - F_TOL - e, 2.5, 4.0)):
        # (columns ascending; either kind first: 1 * 1.0 + 4 * 0.5^2 or 1 * 1.0^2 + 2 * 0.5)
        kinds, w = ([LIN, QUAD], [1.0, 4.0]) if rng.random() < 0.5 else ([QUAD, LIN], [1.0, 2.0])
        out.append(_row([cA, cB], kinds, w, [0.0, 0.0], rc, lb, ub, tag, thr=True))
    sources = ([("nan", NEGLOG)] if edges >= 1 else []) + ([("log0", NEGLOG), ("ovf", EXP)] if edges >= 2 else [])
    sides = [(-INF, 1.0), (0.0, INF), (-1.0, 1.0)]
    kd_of = dict(nan=NEGLOG, log0=NEGLOG, ovf=EXP)
    todo = [(src, pi, pos) for src, _ in sources for pi, pos in enumerate(("first", "mid", "last"))]
    if only is not None:
        todo = [(only[0], 0, only[1])]
    for src, pi, pos in todo:
        kd = kd_of[src]
        cols, kind, p0, p1 = _mixed_row(rng, x, edge_cols(edge_len))
        # (mid: off the multiples of 1 024, so that a long row's source sits in another wavefront than its first entry)
        at = {"first": 0, "mid": len(cols) // 2 + (77 if len(cols) > 200 else 0), "last": len(cols) - 1}[pos]
        kind[at] = kd
        p0[at] = 1.25
        xc = x[cols[at]]
        p1[at] = {"nan": -xc - 1.0, "log0": -xc, "ovf": 800.0 / xc}[src]
        lb, ub = sides[pi] if src == "nan" else (-INF, 1.0)
        if only is not None and not only[2]:
            lb, ub = 0.0, INF
        out.append(_row(cols, kind, p0, p1, 0.5, lb, ub, "edge_%s_%s" % (src, pos)))
    # round_coefs: one LIN coefficient of 64 next to O(1) partials, violated from above
    cols, kind, p0, p1 = _mixed_row(rng, x, edge_cols(edge_len))
    kind[1] = LIN; p0[1] = 64.0; p1[1] = 0.0
    r = _row(cols, kind, p0, p1, 0.25, -INF, 0.0, "round_coefs")
    r["ub"] = _g64(r, x) - 0.75
    out.append(r)
    return out


def _long_thresholds(rng, x, n, k):
    """threshold rows of k LIN atoms with weights +-2^-j (j = 0, 1, 2) on dyadic x (multiples of 2^-10): every partial sum is a
    multiple of 2^-12 below 2^14, hence exact in any order; the signs keep the total S within 1, so rconst = target - S and
    S + rconst = target are exact as well"""
    out = []
    e = 2.0 ** -51
    for tag, target, lb, ub in (("thr_at_ub", 2.5 + F_TOL, -INF, 2.5), ("thr_above_ub", 2.5 + F_TOL + e, -INF, 2.5),
                                ("thr_at_lb", 2.5 - F_TOL, 2.5, INF), ("thr_below_lb", 2.5 - F_TOL - e, 2.5, 4.0)):
        cols = np.sort(rng.choice(n, k, replace=False))
        w = 2.0 ** -rng.integers(0, 3, k)
        S = 0.0
        for t in range(k):                                      # greedy signs: the running sum stays within the largest term
            if (S > 0) == (w[t] * x[cols[t]] > 0):
                w[t] = -w[t]
            S += w[t] * x[cols[t]]
        assert abs(S) <= 1.0 and S + (target - S) == target
        out.append(_row(cols, [LIN] * k, w, [0.0] * k, target - S, lb, ub, tag, thr=True))
    return out


def make_case(seed, n, m_nl, profile, extra_lens=(), *, edges=0, n_tape=0, n_linear=0, objective=None, obj_len=None,
              col_ranges=None, forced=(), repeat_rows=(), unsorted_rows=(), unsorted_all=False, empty_every=0,
              cut_coef_rng=4.0, special_cols=(3, 5), edge_len=9, edge_range=None, only=None, long_thr=0):
    """m_nl: number of nonlinear rows (the epigraph row of a nonlinear objective included); profile: row lengths, tiled over
    the bulk rows and shuffled; extra_lens: lengths that appear once.  col_ranges(i, k) -> (lo, hi, gap_lo, gap_len) confines
    bulk row i (index among the bulk rows, length k) to columns [lo, hi) minus [gap_lo, gap_lo + gap_len).  forced:
    (bulk row, column) pairs; repeat_rows / unsorted_rows: bulk row indices.  only: see _specials.  long_thr: length of four more
    threshold rows of dyadic LIN atoms (x is then dyadic everywhere: multiples of 2^-10), exact in every summation order."""
    rng = np.random.default_rng(seed)
    cA, cB = special_cols
    nx = n + (0 if objective is None else 1)
    x = np.where(rng.random(nx) < 0.5, -1.0, 1.0) * rng.uniform(0.1, 1.0, nx)
    if long_thr:
        x = np.where(rng.random(nx) < 0.5, -1.0, 1.0) * rng.integers(128, 1025, nx) / 1024.0
    x[cA], x[cB] = 1.0, 0.5
    elo, ehi = edge_range if edge_range is not None else (0, n)
    edge_cols = lambda k: elo + rng.choice(ehi - elo, k, replace=False)
    spec = _specials(rng, x, cA, cB, edges, edge_len, edge_cols, only)
    if long_thr:
        spec += _long_thresholds(rng, x, n, long_thr)
    for t in range(n_tape):                                     # x_a * x_b <= 100: a tape row inside the R-groups, never violated
        a, b = sorted(rng.choice(n, 2, replace=False))
        spec.append(_row([a, b], [0, 0], [0.0, 0.0], [0.0, 0.0], 0.0, -INF, 100.0, "tape", row_kind=ROW_TAPE,
                         tape=([OP_VAR, OP_VAR, OP_MUL], [float(a), float(b), 0.0])))
    for t in range(n_linear):                                   # a declared-linear row: it is no NL slot
        cols = np.sort(rng.choice(n, 4, replace=False))
        spec.append(_row(cols, [LIN] * 4, rng.uniform(0.5, 2, 4), [0.0] * 4, 0.0, -INF, 50.0, "linear", linear=1))
    n_spec_nl = sum(1 for r in spec if not r["linear"])
    nb = m_nl - n_spec_nl - (0 if objective is None else 1)
    assert nb >= len(extra_lens) and nb > 0
    lens = np.concatenate([np.resize(np.asarray(profile, dtype=np.int64), nb - len(extra_lens)),
                           np.asarray(extra_lens, dtype=np.int64)])
    lens = lens[rng.permutation(nb)]
    if empty_every:
        lens[::empty_every] = 0
    rlo, rhi = np.zeros(nb, dtype=np.int64), np.full(nb, n, dtype=np.int64)
    glo, glen = np.full(nb, n, dtype=np.int64), np.zeros(nb, dtype=np.int64)
    if col_ranges is not None:
        for i in range(nb):
            rr = col_ranges(i, int(lens[i]))
            if rr is not None:
                rlo[i], rhi[i], glo[i], glen[i] = rr
    browptr, bcol, bkind = _bulk(rng, lens, rlo, rhi, glo, glen)
    for i, c in forced:                                         # the entry of the stratum that holds column c moves onto c
        a, b = browptr[i], browptr[i + 1]
        if b - a == 0:
            continue
        assert rlo[i] <= c < rhi[i] and not (glo[i] <= c < glo[i] + glen[i])
        t = a + int(np.searchsorted(bcol[a:b], c, side="right")) - 1
        t = max(t, a)
        ok = (t == a or bcol[t - 1] < c) and (t == b - 1 or bcol[t + 1] > c)
        if ok:
            bcol[t] = c
    for i in repeat_rows:
        a, b = browptr[i], browptr[i + 1]
        if b - a >= 2:
            bcol[a + 1] = bcol[a]
    urows = range(nb) if unsorted_all else unsorted_rows
    for i in urows:
        a, b = browptr[i], browptr[i + 1]
        p = a + rng.permutation(b - a)
        bcol[a:b], bkind[a:b] = bcol[p], bkind[p]
    bp0, bp1 = _params(rng, bkind, x[bcol])                     # (after the columns are final: QUAD centres depend on x[col])
    brconst = np.where(rng.random(nb) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 2.0, nb)
    # sides from the float64 value
    val, _ = sep_ref.atoms_f64(bkind, bp0, bp1, x[bcol])
    brows = np.repeat(np.arange(nb), lens)
    g = np.bincount(brows, weights=val, minlength=nb) + brconst
    side = (np.arange(nb) + int(rng.integers(0, 9))) % 9
    d1, d2 = rng.uniform(0.05, 0.5, nb), rng.uniform(0.05, 0.5, nb)
    d1 = np.where((side == 3) | (side == 6), 3 * d1 + 1.0, d1)   # the deepest violation is a lower-sided one (lb - g)
    blb, bub = np.full(nb, -INF), np.full(nb, INF)
    sd = lambda s: side == s
    bub[sd(0)] = (g + d1)[sd(0)]                                # (-inf, ub] satisfied
    bub[sd(1)] = (g - d1)[sd(1)]                                # (-inf, ub] violated above
    blb[sd(2)] = (g - d1)[sd(2)]                                # [lb, +inf) satisfied
    blb[sd(3)] = (g + d1)[sd(3)]                                # [lb, +inf) violated below
    blb[sd(4)] = (g - d1)[sd(4)]; bub[sd(4)] = (g + d2)[sd(4)]  # [lb, ub] satisfied
    bub[sd(5)] = (g - d1)[sd(5)]; blb[sd(5)] = (g - d1 - d2)[sd(5)]   # [lb, ub] violated above
    blb[sd(6)] = (g + d1)[sd(6)]; bub[sd(6)] = (g + d1 + d2)[sd(6)]   # [lb, ub] violated below
    blb[sd(7)] = g[sd(7)]; bub[sd(7)] = g[sd(7)]                # equality, satisfied
    blb[sd(8)] = (g + d1)[sd(8)]; bub[sd(8)] = (g + d1)[sd(8)]  # equality, violated
    # assemble
    third = (len(spec) + 2) // 3
    rng.shuffle(spec)
    # threshold and edge rows spread over the three places; keep an edge row first and one last
    h = nb // 2
    C = SepCase()
    parts = [("s", spec[:third]), ("b", (0, h)), ("s", spec[third:2 * third]), ("b", (h, nb)), ("s", spec[2 * third:])]
    lens_all, cols, kinds, p0s, p1s, rcs, lbs, ubs, tags, thr, rk, lin, tptr, top, targ, bulk_of = ([] for _ in range(16))
    tptr.append(0)
    for what, p in parts:
        if what == "s":
            for r in p:
                lens_all.append(len(r["col"])); cols.append(r["col"]); kinds.append(r["kind"]); p0s.append(r["p0"]); p1s.append(r["p1"])
                rcs.append(r["rconst"]); lbs.append(r["lb"]); ubs.append(r["ub"]); tags.append(r["tag"]); thr.append(r["thr"])
                rk.append(r["row_kind"]); lin.append(r["linear"]); bulk_of.append(-1)
                if r["tape"] is not None:
                    top.extend(r["tape"][0]); targ.extend(r["tape"][1])
                tptr.append(len(top))
        else:
            a, b = p
            lens_all.extend(lens[a:b].tolist())
            sl = slice(browptr[a], browptr[b])
            cols.append(bcol[sl]); kinds.append(bkind[sl]); p0s.append(bp0[sl]); p1s.append(bp1[sl])
            rcs.extend(brconst[a:b].tolist()); lbs.extend(blb[a:b].tolist()); ubs.extend(bub[a:b].tolist())
            tags.extend(["bulk"] * (b - a)); thr.extend([False] * (b - a)); rk.extend([ROW_SEP] * (b - a)); lin.extend([0] * (b - a))
            bulk_of.extend(range(a, b)); tptr.extend([len(top)] * (b - a))
    m = len(lens_all)
    C.n, C.m = n, m
    C.rowptr = np.concatenate([[0], np.cumsum(lens_all)]).astype(np.int64)
    C.col = np.concatenate(cols).astype(np.int32); C.kind = np.concatenate(kinds).astype(np.uint8)
    C.p0 = np.concatenate(p0s); C.p1 = np.concatenate(p1s)
    C.rconst = np.array(rcs); C.lb = np.array(lbs); C.ub = np.array(ubs)
    C.tags = tags; C.threshold = np.array(thr, dtype=bool)
    C.row_kind = np.array(rk, dtype=np.uint8); C.row_linear = np.array(lin, dtype=np.uint8)
    C.tape_ptr, C.tape_op, C.tape_arg = np.array(tptr, dtype=np.int64), np.array(top, dtype=np.int32), np.array(targ, dtype=float)
    C.bulk_of = np.array(bulk_of)
    C.l_var, C.u_var = np.full(n, -1.0), np.full(n, 1.0)
    C.x, C.f_tol, C.cut_coef_rng, C.sense = x, F_TOL, cut_coef_rng, "Min"
    C.edges = edges
    # objective
    if objective is None:
        C.obj_linear = True
        C.obj_col, C.obj_kind, C.obj_p0, C.obj_p1, C.obj_const = np.array([0]), np.array([LIN]), np.array([1.0]), np.array([0.0]), 0.0
    else:
        C.obj_linear = False
        k = obj_len
        assert k < n
        oc = np.sort(rng.choice(n, k, replace=False))
        ok = rng.integers(0, 4, k)
        xv = x[oc]
        if objective == "pad":                                  # every partial in (-4.9, -4.1): see the module docstring
            d = -rng.uniform(4.1, 4.9, k)
            op0, op1 = np.zeros(k), np.zeros(k)
            mk = ok == LIN; op0[mk] = d[mk]
            mk = ok == QUAD; op0[mk] = 1.0; op1[mk] = xv[mk] - d[mk] / 2
            mk = ok == EXP; op1[mk] = -1.0; op0[mk] = -d[mk] * np.exp(xv[mk])
            mk = ok == NEGLOG; op1[mk] = 3.0; op0[mk] = -d[mk] * (xv[mk] + 3.0)
        else:
            op0, op1 = _params(rng, ok, xv)
        C.obj_col, C.obj_kind, C.obj_p0, C.obj_p1, C.obj_const = oc, ok, op0, op1, 0.75
        val, _ = sep_ref.atoms_f64(ok, op0, op1, xv)
        C.x[n] = float(np.sum(val) + 0.75) - 1.0               # f(x) - t = 1: the epigraph row is violated
    _extend(C)
    return C


def _extend(C):
    """the extended structure the engine evaluates: the rows plus, for a nonlinear objective, the epigraph row f(x) - t <= 0
    over n + 1 columns (src/nlpeval.jl:42-63) -- stored with its structural non-zeros only, pad_zero remembers the rest"""
    if C.obj_linear:
        C.e_rowptr, C.e_col, C.e_kind, C.e_p0, C.e_p1 = C.rowptr, C.col.astype(np.int64), C.kind.astype(np.int64), C.p0, C.p1
        C.e_rconst, C.e_lb, C.e_ub, C.e_row_kind = C.rconst, C.lb, C.ub, C.row_kind
        C.e_pad = np.zeros(C.m, dtype=bool)
        C.e_threshold, C.e_tags = C.threshold, C.tags
    else:
        k = len(C.obj_col)
        C.e_rowptr = np.concatenate([C.rowptr, [C.rowptr[-1] + k + 1]])
        C.e_col = np.concatenate([C.col, C.obj_col, [C.n]]).astype(np.int64)
        C.e_kind = np.concatenate([C.kind, C.obj_kind, [LIN]]).astype(np.int64)
        C.e_p0 = np.concatenate([C.p0, C.obj_p0, [-1.0]]); C.e_p1 = np.concatenate([C.p1, C.obj_p1, [0.0]])
        C.e_rconst = np.concatenate([C.rconst, [C.obj_const]])
        C.e_lb = np.concatenate([C.lb, [-INF]]); C.e_ub = np.concatenate([C.ub, [0.0]])
        C.e_row_kind = np.concatenate([C.row_kind, [ROW_SEP]])
        C.e_pad = np.concatenate([np.zeros(C.m, dtype=bool), [k + 1 < C.n + 1]])
        C.e_threshold = np.concatenate([C.threshold, [False]]); C.e_tags = C.tags + ["epigraph"]
    nl = np.flatnonzero(C.row_linear == 0)
    C.nl_rows = nl if C.obj_linear else np.concatenate([nl, [C.m]])
    C.m_nl = len(C.nl_rows)


def description(ktn, C):
    return ktn.NLPDescription(C.n, C.rowptr, C.col, C.row_kind, C.row_linear, C.rconst, C.kind, C.p0, C.p1,
                              C.tape_ptr, C.tape_op, C.tape_arg, obj_linear=C.obj_linear, obj_col=C.obj_col,
                              obj_atom_kind=C.obj_kind, obj_p0=C.obj_p0, obj_p1=C.obj_p1, obj_const=C.obj_const)


def load(ktn, C, **solver_kw):
    kw = dict(log_level=0, cut_coef_rng=C.cut_coef_rng, cut_cap_factor=0.0, purge_age=0)
    kw.update(solver_kw)
    m = ktn.NonlinearModel(ktn.KatanaSolver(**kw))
    m.loadproblem(C.n, C.m, C.l_var, C.u_var, C.lb, C.ub, C.sense, description(ktn, C))
    return m


def reference(C, depth=None):
    """float64 reference of every row of the extended structure (tape rows: zeros that nobody reads)"""
    return sep_ref.rows_ref_f64(C.e_rowptr, C.e_col, C.e_kind, C.e_p0, C.e_p1, C.e_rconst, C.x, depth=depth)


def row_mp(C, r, depth=None):
    a, b = C.e_rowptr[r], C.e_rowptr[r + 1]
    return sep_ref.row_ref_mp(C.e_col[a:b], C.e_kind[a:b], C.e_p0[a:b], C.e_p1[a:b], C.e_rconst[r], C.x, depth=depth)


class Expected:
    pass


def expected_sweep(C, R):
    """what a sweep at C.x must find, from the float64 reference R (valid under the input conditions): the violated NL
    slots in order, maxviol and its tolerance, whether a violated row has a non-finite coefficient, and the cuts"""
    E = Expected()
    nl = C.nl_rows
    sep = C.e_row_kind[nl] == ROW_SEP
    g, lb, ub = R.g[nl], C.e_lb[nl], C.e_ub[nl]
    with np.errstate(all="ignore"):
        sat = (g >= lb - C.f_tol) & (g <= ub + C.f_tol)
        sat |= ~sep                                             # tape rows of these cases are satisfied by construction
        v = np.fmax(g - ub, lb - g)
        v = np.where(np.isnan(v), INF, v)
    E.viol_slots = np.flatnonzero(~sat)
    E.viol_rows = nl[E.viol_slots]
    E.nviol = len(E.viol_rows)
    vv = v[E.viol_slots]
    E.maxviol = float(vv.max()) if E.nviol else 0.0
    E.maxviol_tol = 0.0
    if E.nviol and np.isfinite(E.maxviol):                      # the bound of the row that attains the maximum
        rmax = E.viol_rows[int(np.argmax(vv))]
        E.maxviol_tol = float(R.slack * (R.e_g[rmax] + 2 * U * E.maxviol))
    # entries of the violated rows, in order
    lens = np.diff(C.e_rowptr)[E.viol_rows]
    E.cut_rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.repeat(C.e_rowptr[E.viol_rows] - E.cut_rowptr[:-1], lens) + np.arange(int(E.cut_rowptr[-1]))
    E.idx = idx
    der = R.jac[idx]
    E.nonfinite = bool((~np.isfinite(der)).any())
    # round_coefs (src/model.jl:200-207): signed maximum, implicit zeros of a pad_zero row included
    crow = np.repeat(np.arange(E.nviol), lens)
    mx = np.full(E.nviol, -INF)
    np.maximum.at(mx, crow, der)
    mx = np.where(C.e_pad[E.viol_rows], np.maximum(mx, 0.0), mx)
    amax_err = np.zeros(E.nviol)
    np.maximum.at(amax_err, crow, R.e_der[idx])
    with np.errstate(all="ignore"):
        lhs = der + C.cut_coef_rng
        E.zeroed = lhs < mx[crow]
        E.round_margin_ok = np.abs(lhs - mx[crow]) >= 1e3 * R.slack * 2 * (R.e_der[idx] + amax_err[crow]) + 1e3 * U * np.abs(mx[crow])
        E.round_margin_ok |= lhs == mx[crow] + C.cut_coef_rng   # the maximum itself
    E.col = C.e_col[idx]
    E.coef = np.where(E.zeroed, 0.0, der)
    E.coef_tol = np.where(E.zeroed, 0.0, R.slack * 2 * R.e_der[idx])
    b = R.b[E.viol_rows]
    with np.errstate(all="ignore"):
        E.lo, E.hi = C.e_lb[E.viol_rows] - b, C.e_ub[E.viol_rows] - b
        E.lo_tol = R.slack * (R.e_b[E.viol_rows] + 2 * U * np.abs(E.lo))
        E.hi_tol = R.slack * (R.e_b[E.viol_rows] + 2 * U * np.abs(E.hi))
    return E


def check_conditions(C, R=None):
    """the input conditions of the module docstring; returns the reference"""
    R = reference(C) if R is None else R
    sep = C.e_row_kind == ROW_SEP
    nlmask = np.zeros(len(sep), dtype=bool); nlmask[C.nl_rows] = True
    rows = R.rows
    fin_row = np.isfinite(R.g)
    # 1. terms against the row's value bound
    term_ok = ~np.isfinite(R.val) | ~fin_row[rows] | ~sep[rows] | (np.abs(R.val) >= 1e3 * R.e_g[rows])
    assert term_ok.all(), ("a term below 1e3 x the value bound", rows[~term_ok][:5], R.val[~term_ok][:5], R.e_g[rows[~term_ok]][:5])
    rc_ok = ~fin_row | ~sep | (C.e_rconst == 0.0) | (np.abs(C.e_rconst) >= 1e3 * R.e_g)
    assert rc_ok.all(), ("rconst below 1e3 x the value bound", np.flatnonzero(~rc_ok)[:5])
    # 2. distance from the thresholds
    with np.errstate(all="ignore"):
        du = np.abs(R.g - (C.e_ub + C.f_tol)); dl = np.abs(R.g - (C.e_lb - C.f_tol))
        far = (np.isinf(C.e_ub) | (du >= 10 * R.e_g)) & (np.isinf(C.e_lb) | (dl >= 10 * R.e_g))
    chk = sep & nlmask & fin_row & ~C.e_threshold
    assert far[chk].all(), ("a row within 10 x its value bound of a threshold", np.flatnonzero(chk & ~far)[:5])
    # threshold rows: g is what the module docstring says, exactly
    for r in np.flatnonzero(C.e_threshold):
        want = {"thr_at_ub": C.e_ub[r] + C.f_tol, "thr_above_ub": np.nextafter(C.e_ub[r] + C.f_tol, INF),
                "thr_at_lb": C.e_lb[r] - C.f_tol, "thr_below_lb": np.nextafter(C.e_lb[r] - C.f_tol, -INF)}[C.e_tags[r]]
        assert R.g[r] == want, (C.e_tags[r], R.g[r], want)
    # 3. round_coefs margins on the rows a sweep cuts
    E = expected_sweep(C, R)
    if not E.nonfinite:
        assert E.round_margin_ok.all(), ("an ambiguous round_coefs decision", E.col[~E.round_margin_ok][:5])
    return R, E


# ---- the cases of tests/test_gpu_sep_kernels.py (tests/test_sep_ref.py asserts the input conditions on each) -------------
ROW_M = {8: 4000, 16: 2000, 32: 2000, 64: 2000}                # enough rows that the one 8 192-entry row leaves the average (hence G) alone


def row_profile(G):
    return [0, 1, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, 5 * G + 3]


def row_kernel_case(G, rem, edges=0, only=None):
    """ragged rows around the trip boundaries of the G-lane row kernels, one row of 8 192 entries (the largest that is still a
    row-kernel row), tape rows and declared-linear rows in between; m_nl = 4q + rem"""
    return make_case(1000 + 10 * G + rem, 9000, ROW_M[G] + rem, row_profile(G), [8192], edges=edges, n_tape=3, n_linear=2,
                     objective="pad", obj_len=3 * G + 1, only=only)


def mat_rows(cus):
    """rows from which precompute! takes four rows per lane group at G = 8: m_ext * 8 / 64 >= 16 * 32 * CUs"""
    return 4096 * cus + 1003


def mat_case(cus):
    return make_case(77, 100000, mat_rows(cus), [0, 1, 2, 3, 5, 7, 8, 9, 11, 13, 15, 15, 14], edges=2)


LONG_LENS = [8193, 9000, 1024 * 9 + 1] * 3


def long_case(edges=0, only=None):
    """rows beyond 8 192 entries (k_sep_eval_long), among them the edge rows (a non-finite source at the last entry) and the
    pad_zero epigraph row of a nonlinear objective over 8 500 of 12 000 columns"""
    return make_case(31, 12000, 64, [20, 40, 64], LONG_LENS, edges=edges, objective="pad", obj_len=8500, edge_len=8693,
                     only=only, long_thr=8500)


def long_depth(C):
    """longest chain of additions per row: k_sep_eval_long's shape beyond 8 192 entries, else the row length"""
    lens = np.diff(C.e_rowptr)
    return np.where(lens > 8192, sep_ref.long_row_depth(lens), lens)


def blocked_case(n, bc=8192, edges=0, unsorted=False, only=None):
    """long sorted rows for the column-blocked sweep (blocks of bc columns): rows confined to one block, rows with no entry in
    the middle block, entries forced onto the block edges, threshold rows that span the first and the last block"""
    nb_blocks = -(-n // bc)
    m_nl = 131

    def ranges(i, k):
        if i % 5 == 0:
            b = (i // 5) % nb_blocks
            lo, hi = b * bc, min((b + 1) * bc, n)
            return (lo, hi, n, 0) if hi - lo >= k else None
        if i % 5 == 1 and nb_blocks >= 3:
            return (0, n, bc, bc)
        return None
    edge_cols = [bc - 1, bc, 2 * bc - 1, 2 * bc, n - 1]
    forced = []
    for i in range(m_nl):
        if i % 10 == 2:
            forced += [(i, bc - 1), (i, 2 * bc - 1), (i, n - 1)]
        if i % 10 == 7:
            forced += [(i, bc), (i, 2 * bc)] if 2 * bc < n else [(i, bc)]
    forced = [(i, c) for i, c in forced if i < m_nl - 20 and c < n]
    C = make_case(500 + n % 97 + (1 if unsorted else 0), n, m_nl, [300, 500, 700, 400], edges=edges, col_ranges=ranges, forced=forced,
                  unsorted_rows=[11] if unsorted else (), special_cols=(3, n - 2), only=only)
    for c in edge_cols:
        assert c >= n or (C.col == c).any(), ("edge column unused", c)
    return C


BATCH_SHAPES = [(m_nl, n) for m_nl in (2047, 2049, 5000) for n in (8192, 8193, 30000)]


def batch_case(m_nl, n, edges=0, only=None):
    """many short rows for the batch-blocked sweep: empty rows inside a batch, one row of 5 000 entries confined to the first
    column block (a run of one kind and block beyond a chunk of 1 024), repeated columns, unsorted rows, and a nonlinear
    objective: over more than 8 192 columns for n > 8 192 (the batch kernel next to k_sep_eval_long), else over 50"""
    ranges = lambda i, k: (0, 8192, n, 0) if k == 5000 else None
    # n = 8 192: a short pad_zero epigraph row, which the batch kernel itself evaluates (t is the only column of block 1)
    obj = dict(objective="mixed", obj_len=(n - 1 if n == 8193 else 9000)) if n > 8192 else dict(objective="pad", obj_len=50)
    return make_case(7000 + m_nl + n % 13, n, m_nl, [0, 1, 3, 8, 16, 31, 33, 64], [5000], edges=edges, col_ranges=ranges,
                     repeat_rows=[4, 5, 300, 301], unsorted_rows=[6, 7, 8, 302, 303, 1500], empty_every=37, only=only, **obj)



# ---- small convex mixed-atom models for the device-side batch loop (k_ecp_blocks) -----------------------------------------
CONVEX_SLACK = 0.3


def convex_instance(seed, n=12, m_nl=4, k=4, bad=False):
    """min c.x over the box [-1, 1]^n under m_nl convex mixed-atom rows: upper-sided rows g(x) <= ub with positive weights on
    QUAD / EXP / NEGLOG atoms (NEGLOG shifts beyond the box), lower-sided rows g(x) >= lb with negative weights, LIN atoms of
    either sign; every row has slack CONVEX_SLACK at an interior point x0.  bad: the first row gets exp(800 x_j) on a column
    with c_j < 0 and x0_j = -0.5, so the first LP point (x_j = +1) makes its value and its derivative +inf -- a coefficient
    that round_coefs keeps, so the reference ends Error too."""
    from katana_jl_amd.instances import SeparableInstance
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(-0.5, 0.5, n)
    c = np.where(rng.random(n) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 2.0, n)
    rows = np.repeat(np.arange(m_nl), k)
    col = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for _ in range(m_nl)])
    kind = np.concatenate([rng.permutation(np.resize([QUAD, EXP, NEGLOG, LIN], k)) for _ in range(m_nl)])
    p0, p1 = _params(rng, kind, x0[col])
    lower = (np.arange(m_nl) % 2 == 1)
    nl = kind != LIN
    p0[nl] = np.abs(p0[nl]) * np.where(lower[rows][nl], -1.0, 1.0)
    if bad:
        j = int(np.flatnonzero(c < 0)[0])
        x0[j] = -0.5
        col[0], kind[0], p0[0], p1[0] = j, EXP, 1.0, 800.0     # (row 0 may now repeat a column or be unsorted: allowed)
    val, _ = sep_ref.atoms_f64(kind, p0, p1, x0[col])
    g0 = np.bincount(rows, weights=val, minlength=m_nl)
    lb = np.where(lower, g0 - CONVEX_SLACK, -INF)
    ub = np.where(lower, INF, g0 + CONVEX_SLACK)
    return SeparableInstance(n=n, l_var=np.full(n, -1.0), u_var=np.full(n, 1.0), sense="Min",
                             rowptr=np.arange(0, m_nl * k + 1, k).astype(np.int64), col=col.astype(np.int32), kind=kind.astype(np.uint8),
                             p0=p0, p1=p1, rconst=np.zeros(m_nl), l_constr=lb, u_constr=ub, obj_col=np.arange(n, dtype=np.int32),
                             obj_kind=np.zeros(n, dtype=np.uint8), obj_p0=c, obj_p1=np.zeros(n), obj_const=0.0, xhat=x0,
                             opt_obj=float("nan"), m_lin=0, m_nl=m_nl, meta=dict(lam_sum=0.0, mu_sum=0.0))


def convex_objective_bound(inst, f_tol):
    """Two points that both minimise c.x over an outer approximation of F = {g <= ub, g >= lb} and lie in the relaxed set
    F_eps (every row within eps) have objectives in [min over F_eps, min over F].  For y in F_eps and the interior point x0
    with slack s on every row, z = (1 - t) y + t x0 with t = eps / (eps + s) lies in F by convexity, and
    c.z - c.y = t c.(x0 - y) <= t sum_j |c_j| (u_j - l_j).  So the two objectives differ by at most that; eps = 2 f_tol leaves
    room for the LP tolerances, which are fractions of f_tol."""
    eps = 2 * f_tol
    return eps / (eps + CONVEX_SLACK) * float(np.sum(np.abs(inst.obj_p0) * (inst.u_var - inst.l_var)))
