"""The case list of the exact-LP tests (tests/test_exact_lp_ref.py on the CPU, tests/test_gpu_exact_lp.py on the GPU): small LPs
at the edges of csrc/mid_lp.hpp (33 .. lp_mid_max_var columns) and csrc/dense_lp.hpp (<= 32 columns), each with the status it
must end in.  Deterministic generators on top of `instances.make_lp` and of the `_random_small_lp` recipe of
tests/test_gpu_lp.py.  Every variable is boxed unless the case says otherwise; a case with free columns has at most 8 of them.

The trip lengths the sizes are chosen around are read from the code: k_mid_price covers 4 096 rows per pass (128 blocks x 256
threads / 8 lanes), k_mid_select / k_mid_ratio / k_mid_final / k_mid_resid_norm stride by 256 over the columns (k_mid_select also
over the entering row's entries), k_mid_apply takes 4 columns per block and 64 lanes per column, k_dense_lp walks rows by 256."""
from dataclasses import dataclass, field

import numpy as np

from katana_jl_amd import instances

INF = np.inf


@dataclass
class LpCase:
    name: str
    n: int
    rowptr: np.ndarray
    col: np.ndarray
    val: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    l: np.ndarray
    u: np.ndarray
    c: np.ndarray
    sense: str = "Min"
    status: str = "Optimal"
    tags: tuple = ()
    info: dict = field(default_factory=dict)      # what the CPU tier checks the case for (row indices, expected values)

    @property
    def m(self):
        return len(self.lo)

    def csr(self):
        return self.rowptr, self.col, self.val

    def instance(self):
        """the LP as a SeparableInstance of LIN atoms (helpers.hip_load_instance loads it as is: rconst = 0)"""
        nz = np.flatnonzero(self.c)
        z = np.zeros(len(self.col))
        return instances.SeparableInstance(
            n=self.n, l_var=self.l.copy(), u_var=self.u.copy(), sense=self.sense, rowptr=self.rowptr.astype(np.int64),
            col=self.col.astype(np.int32), kind=np.zeros(len(self.col), dtype=np.uint8), p0=self.val.copy(), p1=z,
            rconst=np.zeros(self.m), l_constr=self.lo.copy(), u_constr=self.hi.copy(), obj_col=nz.astype(np.int32),
            obj_kind=np.zeros(len(nz), dtype=np.uint8), obj_p0=self.c[nz].copy(), obj_p1=np.zeros(len(nz)), obj_const=0.0,
            xhat=np.zeros(self.n), opt_obj=0.0, m_lin=self.m, m_nl=0, meta=dict(lp=True))


def highs_solve(case, extra=None):
    """(status, objective, x, y) of HiGHS (oracle.lp.LinearModel) on the case, plus the rows of `extra` = (rowptr, col, val, lo, hi);
    y in the engine's convention: > 0 lower side, < 0 upper side, for the problem min s c'x"""
    from oracle.lp import LinearModel
    lm = LinearModel()
    lm.add_variables(case.l, case.u)
    lm.set_objective(case.sense, np.arange(case.n), case.c, 0.0)
    lm.add_rows(case.rowptr, case.col, case.val, case.lo, case.hi)
    if extra is not None:
        lm.add_rows(*extra)
    st = lm.solve()
    if st != "Optimal":
        return st, None, None, None
    s = -1.0 if case.sense == "Max" else 1.0
    y = s * np.array(lm.h.getSolution().row_dual, dtype=np.float64)
    # HiGHS's duals are sign feasible to ITS dual tolerance (1e-9, oracle.lp): a multiplier within it that points at an absent side is
    # that rounding, not a multiplier (the engine's own y never has one: it is written as +-max(lambda, 0))
    lo, hi = np.asarray(lm.row_lo), np.asarray(lm.row_hi)
    y[(np.abs(y) <= 1e-9) & (((y > 0) & ~np.isfinite(lo)) | ((y < 0) & ~np.isfinite(hi)))] = 0.0
    return st, lm.getobjval(), lm.getsolution(), y


# ---- building blocks ------------------------------------------------------------------------------------------------------

def _base(name, n, m, seed, tags=(), **kw):
    inst = instances.make_lp(n=n, m=m, seed=seed, **kw)
    c = np.zeros(n)
    c[inst.obj_col] = inst.obj_p0
    case = LpCase(name, n, inst.rowptr.astype(np.int64), inst.col.astype(np.int32), inst.p0.copy(), inst.l_constr.copy(),
                  inst.u_constr.copy(), inst.l_var.copy(), inst.u_var.copy(), c, tags=tuple(tags))
    case.info["xhat"] = inst.xhat.copy()
    return case


def _add_rows(case, rows):
    """rows: list of (cols, vals, lo, hi); returns the index of the first one"""
    first = case.m
    for cols, vals, lo, hi in rows:
        case.col = np.concatenate([case.col, np.asarray(cols, dtype=np.int32)])
        case.val = np.concatenate([case.val, np.asarray(vals, dtype=np.float64)])
        case.rowptr = np.concatenate([case.rowptr, [case.rowptr[-1] + len(cols)]]).astype(np.int64)
        case.lo = np.concatenate([case.lo, [lo]])
        case.hi = np.concatenate([case.hi, [hi]])
    return first


def _cut_row(rng, case, length, depth, cols=None):
    """a random row  g'x <= g'xhat - depth ||g||  that cuts the planted point off"""
    xhat = case.info["xhat"]
    if cols is None:
        cols = np.sort(rng.choice(case.n, size=length, replace=False))
    g = rng.standard_normal(len(cols))
    g[np.abs(g) < 0.1] = 0.5
    return cols, g, -INF, float(g @ xhat[cols] - depth * np.linalg.norm(g))


def _as_max(case, name):
    return LpCase(name, case.n, case.rowptr.copy(), case.col.copy(), case.val.copy(), case.lo.copy(), case.hi.copy(), case.l.copy(),
                  case.u.copy(), -case.c, sense="Max", status=case.status, tags=case.tags + ("max",), info=dict(case.info))


# ---- the mid-size solver (n >= 33) -------------------------------------------------------------------------------------------

def _mid_sizes():
    return [_base("mid_n%d" % n, n, 3 * n, 100 + n, tags=("size",)) for n in (33, 34, 63, 65, 255, 257, 511, 512)]


def _mid_price_second_trip():
    """m = 4 100 > 4 096: the pricing loop's second trip.  With active_frac = 0 every column is pinned to a bound by a positive
    reduced cost and the 4 096 random rows are slack: the bound vertex the solver starts from is their optimum.  The last 4 rows
    push lower-pinned columns up by a little, which costs: the optimum has multipliers on them (checked on the CPU), and only a
    pricing pass that reaches row 4 096 and beyond sees that the start is infeasible."""
    case = _base("mid_price_4100", 64, 4096, 7, tags=("price2",), active_frac=0.0)
    rng = np.random.default_rng(70)
    xhat = case.info["xhat"]
    lower = np.flatnonzero(case.l > -10.0)
    rows = []
    for _ in range(4):
        cols = np.sort(rng.choice(lower, size=8, replace=False))
        g = -rng.uniform(0.5, 1.5, 8)
        rows.append((cols, g, -INF, float(g @ xhat[cols] - 0.02)))
    first = _add_rows(case, rows)
    case.info["active_among"] = list(range(first, first + 4))
    return case


def _mid_long_entering_row():
    """n = 512 with one active row of 300 entries: k_mid_select's 256-stride loop over the entering row makes a second trip"""
    case = _base("mid_long_row_300", 512, 3 * 512, 8, tags=("longrow",))
    rng = np.random.default_rng(80)
    first = _add_rows(case, [_cut_row(rng, case, 300, 0.5)])
    case.info["active_among"] = [first]
    return case


def _mid_row_shapes():
    """rows of 1, 7, 8, 9 and 17 entries (the 8-lane groups of k_mid_price), a row that repeats a column, an empty row with
    hi = 0, a row with hi = NaN and lo = -inf (vacuous)"""
    case = _base("mid_row_shapes", 48, 144, 9, tags=("shapes",))
    rng = np.random.default_rng(90)
    rows = [_cut_row(rng, case, k, 0.2) for k in (1, 7, 8, 9, 17)]
    cols, g, lo, hi = _cut_row(rng, case, 6, 0.2)
    xhat = case.info["xhat"]
    rep = (np.concatenate([cols, cols[2:3]]), np.concatenate([g, [0.75]]), lo, float(hi + 0.75 * xhat[cols[2]]))     # column cols[2] twice
    first = _add_rows(case, rows + [rep, ([], [], -INF, 0.0), (cols, g, -INF, np.nan)])
    case.info.update(active_among=list(range(first, first + 6)), repeated_row=first + 5, empty_row=first + 6, nan_row=first + 7)
    return case


def _mid_eq_range():
    """two equality rows and three range rows over columns that the planted optimum pins to a bound with a positive reduced cost
    (moving them costs, so the rows carry multipliers): the equalities and the second range row push lower-pinned columns UP
    (lower side, y > 0), the first range row pushes upper-pinned columns DOWN (upper side, y < 0), the third is slack"""
    case = _base("mid_eq_range", 72, 216, 10, tags=("eqrange",), active_frac=0.03)
    rng = np.random.default_rng(100)
    xhat = case.info["xhat"]
    lower = rng.permutation(np.flatnonzero(case.l > -10.0))
    upper = rng.permutation(np.flatnonzero(case.u < 10.0))
    assert len(lower) >= 12 and len(upper) >= 3

    def row(cols, a, b):
        cols = np.sort(cols)
        g = rng.uniform(0.5, 1.5, len(cols))
        ax = float(g @ xhat[cols])
        return cols, g, ax + a, ax + b
    first = _add_rows(case, [row(lower[0:3], 0.1, 0.1), row(lower[3:6], 0.1, 0.1), row(upper[0:3], -1.0, -0.2), row(lower[6:9], 0.2, 1.0),
                             row(lower[9:12], -0.5, 0.5)])
    case.info.update(eq_rows=[first, first + 1], range_rows=[first + 2, first + 3, first + 4], upper_active=first + 2, lower_active=first + 3)
    return case


def _mid_free(name, flip):
    """dual degenerate, with (at most 8) FREE columns: make_lp's `free_frac` columns -- in no multiplier-carrying row, zero cost,
    strictly inside a wide box -- lose both bounds (the rows they are in keep the LP bounded: checked on the CPU).
    flip: every free column that HiGHS's optimum has below zero is replaced by its negative (x_j -> -x_j: column j of the rows
    changes sign), so that no free column has to cross the artificial side at 0 that mid_lp.hpp starts it on."""
    case = _base(name, 96, 288, 11, tags=("free",), active_frac=0.05, free_frac=0.5, degenerate_frac=0.1)
    free = np.flatnonzero((case.l == -10.0) & (case.u == 10.0) & (case.c == 0.0))[:8]
    assert len(free) >= 4
    case.l[free] = -INF
    case.u[free] = INF
    case.info["free_cols"] = free.tolist()
    if flip:
        x = highs_solve(case)[2]
        neg = [j for j in free if x[j] < 0.0]
        case.val = np.where(np.isin(case.col, neg), -case.val, case.val)
        case.info["xhat"][neg] *= -1.0
        case.info["flipped"] = neg
    return case


def _mid_swap():
    """column 0 occurs in ONE row R only, R is active and x0 is basic (strictly inside its box) at the optimum (checked on the CPU
    from HiGHS's solution): column 0 of the working matrix B then has a single non-zero, in whichever slot R sits in.  Which slot
    that is the solver decides (a side that enters takes the slot of the one that leaves), so this case does not PROVE a row swap
    at column 0; it does not have to: k_mid_gj_pivot pivots on the largest magnitude, so row swaps are routine in every case here."""
    case = _base("mid_swap", 65, 195, 12, tags=("swap",))
    keep = case.col != 0                                                  # column 0 leaves every row ...
    rows = np.repeat(np.arange(case.m), np.diff(case.rowptr))
    case.rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=case.m))]).astype(np.int64)
    case.col, case.val = case.col[keep], case.val[keep]
    xhat = case.info["xhat"]
    case.l[0], case.u[0] = -10.0, 10.0
    rng = np.random.default_rng(120)
    cols = np.concatenate([[0], np.sort(rng.choice(np.arange(1, case.n), size=7, replace=False))])
    g = rng.standard_normal(8)
    g[0] = -1.5
    R = _add_rows(case, [(cols, g, -INF, float(g @ xhat[cols] - 0.5))])    # ... and enters R alone
    case.c[0] = 1.5                                                       # the cost pushes x0 down, R alone holds it up
    case.info.update(swap_row=R)
    return case


def _mid_infeasible(n, seed):
    """a contradictory pair of parallel rows inside an otherwise feasible boxed LP:  g'x <= t  and  2 g'x >= 2 t + 2"""
    case = _base("mid_infeasible_n%d" % n, n, 3 * n, seed, tags=("infeasible",))
    rng = np.random.default_rng(seed + 1000)
    cols, g, _, _ = _cut_row(rng, case, 8, 0.0)
    t = float(g @ case.info["xhat"][cols])
    _add_rows(case, [(cols, g, -INF, t), (cols, 2.0 * g, 2.0 * t + 2.0, INF)])
    case.status = "Infeasible"
    return case


def _mid_infeasible_empty_row():
    case = _base("mid_infeasible_empty_row", 40, 120, 15, tags=("infeasible",))
    _add_rows(case, [([], [], -INF, -1.0)])
    case.status = "Infeasible"
    return case


def _big_bound(n_base, seed, row_lo, name, dense=False):
    """x0 in [0, 2e7] (a FINITE bound beyond kDenseBig = 1e7) and one row  x0 >= row_lo; the other columns are a boxed LP of their
    own.  row_lo = 2.5e7: infeasible.  row_lo = 1.5e7 with cost +x0: optimal at x0 = 1.5e7."""
    if dense:
        base = LpCase("", n_base, np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), np.array([1.0]), np.array([-INF]),
                      np.array([0.5]), np.array([-1.0]), np.array([1.0]), np.array([-1.0]))
    else:
        base = _base("", n_base, 3 * n_base, seed)
    n = n_base + 1
    case = LpCase(name, n, base.rowptr.copy(), (base.col + 1).astype(np.int32), base.val.copy(), base.lo.copy(), base.hi.copy(),
                  np.concatenate([[0.0], base.l]), np.concatenate([[2e7], base.u]), np.concatenate([[1.0], base.c]), tags=("bigbound",))
    _add_rows(case, [([0], [1.0], row_lo, INF)])
    case.status = "Infeasible" if row_lo > 2e7 else "Optimal"
    case.info["x0"] = row_lo
    return case


def mid_cases():
    sizes = _mid_sizes()
    shapes = _mid_row_shapes()
    cases = sizes + [_mid_price_second_trip(), _mid_long_entering_row(), shapes, _mid_eq_range(),
                     _as_max(sizes[3], "mid_n65_max"), _as_max(shapes, "mid_row_shapes_max"),
                     _base("mid_degenerate", 100, 300, 13, tags=("degenerate",), degenerate_frac=0.4), _mid_free("mid_free8", False), _mid_free("mid_free8_nonneg", True),
                     _base("mid_bad_scale", 80, 240, 14, tags=("badscale",), bad_scale_decades=3), _mid_swap(),
                     _mid_infeasible(40, 16), _mid_infeasible(300, 17), _mid_infeasible_empty_row(),
                     _big_bound(39, 18, 2.5e7, "mid_big_bound_infeasible"), _big_bound(39, 18, 1.5e7, "mid_big_bound_optimal")]
    assert all(c.n >= 33 for c in cases)
    return cases


# ---- the dense kernel (n <= 32) ------------------------------------------------------------------------------------------------

def _small(name, n, m_in, seed, boxed=False, tags=()):
    """the `_random_small_lp` recipe of tests/test_gpu_lp.py with the number of inequality rows as a parameter: a bounded polytope
    around the origin, m_in inequality rows, a few range / equality rows (when m_in >= 8), mixed variable bounds"""
    rng = np.random.default_rng(seed)
    m_rg, m_eq = (3, min(2, n - 1)) if m_in >= 8 else (0, 0)
    m_in -= m_rg + m_eq
    A = rng.normal(size=(m_in + m_rg + m_eq, n))
    A[rng.random(A.shape) < 0.3] = 0.0
    if len(A):
        A[:, 0] += 0.1                                # no empty row
    xf = rng.normal(size=n) * 0.3                     # a feasible point
    ax = A @ xf
    lo = np.full(len(A), -INF)
    hi = ax + rng.uniform(0.5, 2.0, len(A))
    lo[m_in:m_in + m_rg] = ax[m_in:m_in + m_rg] - rng.uniform(0.5, 2.0, m_rg)
    lo[m_in + m_rg:] = hi[m_in + m_rg:] = ax[m_in + m_rg:]
    l, u = np.full(n, -INF), np.full(n, INF)
    kind = np.full(n, 3) if boxed else rng.integers(0, 4, n)      # 0 free, 1 lower only, 2 upper only, 3 boxed
    kind[np.flatnonzero(kind == 0)[8:]] = 3           # at most 8 free columns
    l[(kind == 1) | (kind == 3)] = xf[(kind == 1) | (kind == 3)] - 1.0
    u[(kind == 2) | (kind == 3)] = xf[(kind == 2) | (kind == 3)] + 1.0
    r, q = np.nonzero(A)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=len(A)))]).astype(np.int64)
    case = LpCase(name, n, rowptr, q.astype(np.int32), A[r, q], lo, hi, l, u, rng.normal(size=n), tags=tuple(tags))
    case.info["xhat"] = xf
    return case


def _dense_row_shapes():
    case = _small("dense_row_shapes", 12, 60, 31, tags=("shapes",))
    rng = np.random.default_rng(310)
    cols, g, _, hi = _cut_row(rng, case, 5, -0.3)                     # (depth < 0: the row passes the feasible point by)
    xf = case.info["xhat"]
    rep = (np.concatenate([cols, cols[1:2]]), np.concatenate([g, [-0.6]]), -INF, float(hi - 0.6 * xf[cols[1]]))
    first = _add_rows(case, [rep, ([], [], -INF, 0.0), (cols, g, -INF, np.nan)])
    case.info.update(repeated_row=first, empty_row=first + 1, nan_row=first + 2)
    return case


def _dense_unbounded_face():
    """a FREE column whose optimal face is unbounded in a zero-cost direction:  min x0,  x0 in [-1, 1],  x1 free with cost 0,
    one row  x0 - x1 <= -3: the optimum is x0 = -1 with any x1 >= 2.  The artificial side x1 >= 0 the kernel starts on has to
    leave; no multiplier is left on an artificial side, so the kernel answers itself (lp_solve_dense hands over only when an
    artificial side still CARRIES a multiplier and nothing stops the move along it, i.e. the LP is unbounded)"""
    return LpCase("dense_unbounded_face", 2, np.array([0, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32), np.array([1.0, -1.0]),
                  np.array([-INF]), np.array([-3.0]), np.array([-1.0, -INF]), np.array([1.0, INF]), np.array([1.0, 0.0]),
                  tags=("unbounded_face",))


def _dense_artificial_stays():
    """the other half: the same LP with the row  x0 - x1 <= 3, which the start vertex (-1, 0) satisfies.  Nothing enters, the
    artificial side x1 >= 0 STAYS in the working set with a zero multiplier, and the point is optimal for the LP as it is"""
    case = _dense_unbounded_face()
    case.name, case.hi, case.tags = "dense_artificial_stays", np.array([3.0]), ("start_optimal",)
    return case


def dense_cases():
    cases = [_small("dense_n%d_m%d" % (n, m), n, m, 20 + i, boxed=(m <= 1), tags=("size",))      # (one row cannot bound a free column)
             for i, (n, m) in enumerate(((1, 1), (1, 257), (2, 0), (2, 255), (31, 257), (31, 600), (32, 0), (32, 1), (32, 255), (32, 600)))]
    cases += [_as_max(cases[4], "dense_n31_m257_max"), _as_max(cases[8], "dense_n32_m255_max"), _dense_row_shapes(),
              _dense_unbounded_face(), _dense_artificial_stays(),
              _big_bound(1, 0, 2.5e7, "dense_big_bound_infeasible", dense=True), _big_bound(1, 0, 1.5e7, "dense_big_bound_optimal", dense=True)]
    assert all(c.n <= 32 for c in cases)
    return cases


# ---- warm re-solves -------------------------------------------------------------------------------------------------------------

def start_vertex(case):
    """the bound vertex both solvers start from on a boxed LP: every column on the bound its cost pushes it to"""
    s = -1.0 if case.sense == "Max" else 1.0
    return np.where(s * case.c >= 0.0, case.l, case.u)


def max_row_violation(case, x):
    ax = np.bincount(np.repeat(np.arange(case.m), np.diff(case.rowptr)), weights=case.val * x[case.col], minlength=case.m)
    with np.errstate(invalid="ignore"):
        v = np.fmax(ax - case.hi, case.lo - ax)                      # (fmax: a NaN side is vacuous)
    return float(np.max(v)) if case.m else -INF


def warm_rows(case, x_star, seed, n_slack=20, n_cut=5):
    """(rowptr, col, val, lo, hi) of n_slack rows that are slack by >= 1 at x_star, followed by n_cut rows  g'x <= g'x* - 0.1  with
    random sparse g that cut x_star off.  Every second cut is written as a lower-side row (odd side ids in the working set: what a
    purge has to carry over to the row's new index)"""
    rng = np.random.default_rng(seed)
    k = min(6, case.n)
    rowptr, col, val, lo, hi = [0], [], [], [], []
    for i in range(n_slack + n_cut):
        cols = np.sort(rng.choice(case.n, size=k, replace=False))
        g = rng.standard_normal(k)
        gx = float(g @ x_star[cols])
        b = gx + rng.uniform(1.0, 2.0) if i < n_slack else gx - 0.1
        if i >= n_slack and (i - n_slack) % 2 == 1:
            g, lo_i, hi_i = -g, -b, INF               # the same inequality stated on the row's LOWER side: (-g)'x >= -(g'x* - 0.1)
        else:
            lo_i, hi_i = -INF, b
        col.extend(cols.tolist()); val.extend(g.tolist()); rowptr.append(len(col))
        lo.append(lo_i); hi.append(hi_i)
    return (np.array(rowptr, dtype=np.int64), np.array(col, dtype=np.int32), np.array(val), np.array(lo), np.array(hi))


def warm_cases():
    """(solver, case) of the warm re-solve tests: the mid-size solver at n = 64 and n = 300, the dense kernel at n = 12"""
    return [("mid", _base("warm_n64", 64, 192, 40)), ("mid", _base("warm_n300", 300, 900, 41)), ("dense", _small("warm_n12", 12, 72, 43, boxed=True))]


WARM_SEED = 5
