"""Host mirror of Katana's plugin surface over the C ABI (src/solver.jl, src/model.jl,
src/separators.jl, src/util.jl).  Names, argument meaning and status vocabulary follow the
reference; indices are 0-based."""
import collections
import ctypes as C
import os

import numpy as np

from . import _lib as L

STATUS_SYMBOLS = {L.STATUS_NONE: "None", L.STATUS_OPTIMAL: "Optimal", L.STATUS_UNBOUNDED: "Unbounded",
                  L.STATUS_INFEASIBLE: "Infeasible", L.STATUS_USERLIMIT: "UserLimit", L.STATUS_ERROR: "Error"}
_SUPPORTED_FEATURES = ("VisData",)   # src/solver.jl:31-32
# the cut generator of KatanaFirstOrderSeparator(algo) (src/separators.jl:73-76): ktn_params.cut_algo
CUT_ALGOS = {"kelley": L.CUT_KELLEY, "linear_oa_cut": L.CUT_KELLEY,
             "supporting_hyperplane": L.CUT_SUPPORTING, "supporting_hyperplane_cut": L.CUT_SUPPORTING,
             "supporting_hyperplane_quad": L.CUT_SUPPORTING_QUAD, "supporting_hyperplane_quad_cut": L.CUT_SUPPORTING_QUAD}


# the answer of feasible_point() (ktn_get_feasible_point: x and info[0..7])
FeasiblePoint = collections.namedtuple("FeasiblePoint", "found x lam objval nl_margin lin_viol blocking_row unconverged backoffs")


def _cut_algo_code(cut_algo):
    if isinstance(cut_algo, str):
        if cut_algo not in CUT_ALGOS:
            raise ValueError("unknown cut_algo %r (one of %s)" % (cut_algo, ", ".join(sorted(CUT_ALGOS))))
        return CUT_ALGOS[cut_algo]
    return int(cut_algo)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


class KatanaSolver:
    """KatanaSolver(lp_solver; separator, features, f_tol=1e-6, cut_coef_rng=1e9, log_level=10,
    iter_cap=10000, obj_eps=-1.0)  -- src/solver.jl:34-43.

    `lp_solver` is accepted for call-site compatibility (`KatanaSolver(GLPKSolverLP(), ...)`,
    test/runtests.jl:24) and ignored: the LP is solved on the GPU.  Extra keywords `lp_*`,
    `device`, `profile` reach the GPU LP (ktn_params).

    `cut_algo` picks the separator's cut generator: "kelley" (the reference's linear_oa_cut, the default) or
    "supporting_hyperplane" (cut at the boundary point between an interior point and x*), "supporting_hyperplane_quad" (the same
    with the declared-quadratic rows taking part, their boundary point in closed form), or the ktn_params code."""

    def __init__(self, lp_solver=None, separator=None, features=(), f_tol=1e-6, cut_coef_rng=1e9, log_level=10,
                 iter_cap=10000, obj_eps=-1.0, cut_algo="kelley", **gpu_options):
        self.lp_solver = lp_solver
        self.features = list(features)
        for f in self.features:
            if f not in _SUPPORTED_FEATURES:
                raise ValueError("type KatanaFeatures has no field %s" % f)   # setfield! error, src/model.jl:50-52
        self.separator = separator
        self.model_params = dict(f_tol=float(f_tol), cut_coef_rng=float(cut_coef_rng), log_level=int(log_level),
                                 iter_cap=int(iter_cap), obj_eps=float(obj_eps))
        self.gpu_options = dict(gpu_options)
        self.gpu_options["cut_algo"] = _cut_algo_code(cut_algo)


def NonlinearModel(s):
    """MathProgBase.NonlinearModel(s::KatanaSolver)  src/model.jl:63-65"""
    return KatanaNonlinearModel(s)


def quad_triplets_to_engine(rowidx, colidx, vals, convention):
    """MathProgBase's two ways of stating a quadratic form -> the engine's: symmetric Q of  1/2 x'Qx  as triplets stored in
    full, both (r, c) and (c, r) (duplicates are summed downstream, nlp.QuadNLP).  T = the matrix the given triplets sum to.

      convention "objective"  (setquadobj!):    the form is  1/2 x'Qx  with Q symmetric and an off-diagonal pair given ONCE standing
                                                for both entries:  Q = T + T' - diag(T),  i.e.  1/2 sum_r T_rr x_r^2 + sum_{r != c} T_rc x_r x_c
      convention "constraint" (addquadconstr!): the form is  sum T_rc x_r x_c  with no 1/2:  Q = T + T'  (diagonal doubled)

    so an off-diagonal triplet becomes the two mirrored entries in both, and only the diagonal differs: as given, or doubled."""
    if convention not in ("objective", "constraint"):
        raise ValueError("convention must be 'objective' or 'constraint'")
    r = np.asarray(rowidx, dtype=np.int64).reshape(-1)
    c = np.asarray(colidx, dtype=np.int64).reshape(-1)
    v = np.asarray(vals, dtype=np.float64).reshape(-1)
    if not (len(r) == len(c) == len(v)):
        raise ValueError("quadratic triplets: index and value arrays differ in length")
    off = r != c
    dv = v[~off] * (2.0 if convention == "constraint" else 1.0)
    return (np.concatenate([r[off], c[off], r[~off]]), np.concatenate([c[off], r[off], c[~off]]),
            np.concatenate([v[off], v[off], dv]))



class KatanaNonlinearModel:
    def __init__(self, solver):
        self.solver = solver
        lib = L.lib()
        p = L.KtnParams()
        lib.ktn_default_params(C.byref(p))
        for k, v in solver.model_params.items():
            setattr(p, k, v)
        p.vis_data = 1 if "VisData" in solver.features else 0
        for k, v in solver.gpu_options.items():
            if not hasattr(p, k):
                raise TypeError("unknown KatanaSolver option %r" % k)
            setattr(p, k, v)
        self.params = p
        self._h = C.c_void_p()
        code = lib.ktn_create(C.byref(p), C.byref(self._h))
        if code != L.KTN_OK:
            raise L.KatanaHipError(code, "ktn_create failed (no MI355X visible? the engine has no CPU path)")
        self._lib = lib
        self._pid = os.getpid()          # a handle belongs to the process that made it (a forked child must not touch the GPU state)
        self._desc = None
        self.num_var = 0
        self.num_constr = 0
        self._n0 = 0
        self._m0 = 0

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value and getattr(self, "_pid", None) == os.getpid():
                self._lib.ktn_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    # ---- MathProgBase.loadproblem!  src/model.jl:81-173 -----------------------------------
    def loadproblem(self, num_var, num_constr, l_var, u_var, l_constr, u_constr, sense, d):
        l_var, u_var, l_constr, u_constr = _f64(l_var), _f64(u_var), _f64(l_constr), _f64(u_constr)
        assert len(l_var) == num_var and len(u_var) == num_var
        assert len(l_constr) == num_constr and len(u_constr) == num_constr
        sense_code = {"Min": L.MIN, "Max": L.MAX}[sense]
        self._desc = d
        cd = d.c_struct()
        L.check(self._h, self._lib.ktn_loadproblem(self._h, num_var, num_constr, _p(l_var), _p(u_var), _p(l_constr),
                                                   _p(u_constr), sense_code, C.byref(cd)))
        self.num_var = int(self._lib.ktn_get_num_var(self._h))
        self.num_constr = int(self._lib.ktn_sep_num_constr(self._h))
        self._n0 = int(num_var)
        self._m0 = int(num_constr)

    # ---- MathProgBase.optimize!  src/model.jl:219-319 ---------------------------------------
    def optimize(self):
        return STATUS_SYMBOLS[L.check(self._h, self._lib.ktn_optimize(self._h))]

    def optimize_begin(self):
        L.check(self._h, self._lib.ktn_optimize_begin(self._h))

    def ecp_step(self):
        done = C.c_int32(0)
        L.check(self._h, self._lib.ktn_ecp_step(self._h, C.byref(done)))
        return bool(done.value)

    def optimize_end(self):
        return STATUS_SYMBOLS[L.check(self._h, self._lib.ktn_optimize_end(self._h))]

    def reset(self):
        L.check(self._h, self._lib.ktn_reset(self._h))

    # ---- re-solve from the kept cut pool (MathProgBase.setvarLB! / setvarUB! / setobj!) ----------------
    def setvarbounds(self, l, u):
        """New variable bounds in place (None keeps that side); the cuts, their multipliers and x stay, the next optimize()
        runs from them.  Crossed bounds are accepted and end that solve "Infeasible" through the screen."""
        l = None if l is None else _f64(l)
        u = None if u is None else _f64(u)
        for v in (l, u):
            if v is not None and len(v) != self._n0:
                raise ValueError("setvarbounds: %d entries for %d variables" % (len(v), self._n0))
        null = C.POINTER(C.c_double)()
        L.check(self._h, self._lib.ktn_set_var_bounds(self._h, null if l is None else _p(l), null if u is None else _p(u), self._n0))

    def setvarLB(self, l):
        self.setvarbounds(l, None)

    def setvarUB(self, u):
        self.setvarbounds(None, u)

    def setobj(self, c, c0=0.0):
        """A new linear cost c'x + c0 in place, for a loaded objective that is linear (separable of linear atoms, or a QuadNLP
        without obj_Q); non-zeros must stay inside the loaded objective's pattern."""
        c = _f64(c)
        if len(c) != self._n0:
            raise ValueError("setobj: %d entries for %d variables" % (len(c), self._n0))
        L.check(self._h, self._lib.ktn_set_linear_objective(self._h, _p(c), self._n0, float(c0)))

    def setconstrbounds(self, lb, ub):
        """New constraint bounds in place (MathProgBase.setconstrLB! / setconstrUB!; None keeps that side): every cut of a
        nonlinear row moves with its row's bound, linear rows are worked out again, the multipliers and x stay.  A nonlinear row
        may move its finite bound(s) but not gain or lose a side (E_INVALID, nothing changed).  lb_i > ub_i is accepted and ends
        the next solve "Infeasible" (stat "screen_crossed_rows")."""
        lb = None if lb is None else _f64(lb)
        ub = None if ub is None else _f64(ub)
        for v in (lb, ub):
            if v is not None and len(v) != self._m0:
                raise ValueError("setconstrbounds: %d entries for %d constraints" % (len(v), self._m0))
        null = C.POINTER(C.c_double)()
        L.check(self._h, self._lib.ktn_set_row_bounds(self._h, null if lb is None else _p(lb), null if ub is None else _p(ub), self._m0))

    def setconstrLB(self, lb):
        self.setconstrbounds(lb, None)

    def setconstrUB(self, ub):
        self.setconstrbounds(None, ub)

    def lp_row_owners(self):
        """per LP row the constraint row whose cut list holds it; num_constr for a cut of the epigraph row, -1 for a row in no
        list: linear rows, engine-made rows, rows appended without an id (ktn_lp_get_row_owners)"""
        m = int(self._lib.ktn_lp_num_rows(self._h))
        owner = np.full(max(m, 1), -1, dtype=np.int64)
        L.check(self._h, self._lib.ktn_lp_get_row_owners(self._h, _p(owner, C.c_int64), m))
        return owner[:m]

    def lp_row_activity(self):
        """(amin, amax): the smallest and largest value of every LP row over the current variable bounds."""
        m = int(self._lib.ktn_lp_num_rows(self._h))
        amin, amax = np.zeros(max(m, 1)), np.zeros(max(m, 1))
        L.check(self._h, self._lib.ktn_lp_row_activity(self._h, _p(amin), _p(amax), m))
        return amin[:m], amax[:m]

    # ---- getters  src/model.jl:326-343 ---------------------------------------------------
    def status(self):
        return STATUS_SYMBOLS[self._lib.ktn_get_status(self._h)]

    def getobjval(self):
        return float(self._lib.ktn_get_objval(self._h))

    def getsolution(self):
        x = np.empty(self.num_var)
        L.check(self._h, self._lib.ktn_get_solution(self._h, _p(x), len(x)))
        return x

    def getsolvetime(self):
        return float(self._lib.ktn_get_solvetime(self._h))

    # ---- Lagrange multipliers, reduced costs, dual bound (include/katana_hip.h) ----
    def getconstrduals(self):
        """MathProgBase.getconstrduals: d[num_constr] in the caller's row order, d_i > 0 lower side active, < 0 upper side
        (ktn_get_constr_duals; the epigraph row is not reported)"""
        d = np.zeros(max(self._m0, 1))
        L.check(self._h, self._lib.ktn_get_constr_duals(self._h, _p(d), len(d)))
        return d[:self._m0]

    def getreducedcosts(self):
        """MathProgBase.getreducedcosts: z = grad f(x*) - J(x*)' d over the caller's variables (ktn_get_reduced_costs)"""
        z = np.zeros(max(self._n0, 1))
        L.check(self._h, self._lib.ktn_get_reduced_costs(self._h, _p(z), len(z)))
        return z[:self._n0]

    def _dual_bound(self):
        b, g = C.c_double(0.0), C.c_double(0.0)
        L.check(self._h, self._lib.ktn_get_dual_bound(self._h, C.byref(b), C.byref(g)))
        return float(b.value), float(g.value)

    def getobjbound(self):
        """MathProgBase.getobjbound: the bound on the optimum that (d, z) certify at x* -- a lower bound for Min, an upper bound
        for Max (ktn_get_dual_bound)"""
        return self._dual_bound()[0]

    def getobjgap(self):
        """f(x*) - bound (Min) / bound - f(x*) (Max)"""
        return self._dual_bound()[1]

    # ---- a feasible point and the primal bound it certifies (include/katana_hip.h) ----
    def feasible_point(self):
        """x_feas on the segment from the reference point (set_interior_point, or the engine's own under the supporting-hyperplane
        modes) to getsolution(), with every taking-part nonlinear row satisfied (ktn_get_feasible_point).  found: 1 found, 0 no
        reference point, -1 the reference point is not feasible, -2 verification failed; x is NaN unless found == 1."""
        x, info = np.zeros(max(self._n0, 1)), np.zeros(L.FEAS_INFO_LEN)
        L.check(self._h, self._lib.ktn_get_feasible_point(self._h, _p(x), len(x), _p(info), len(info)))
        return FeasiblePoint(int(info[0]), x[:self._n0].copy(), float(info[1]), float(info[2]), float(info[3]), float(info[4]), int(info[5]),
                             int(info[6]), int(info[7]))

    def feasible_row_lambdas(self):
        """lambda_i of feasible_point() by caller row; 1 for a row that does not take part (ktn_get_feasible_row_lambdas)"""
        lam = np.ones(max(self._m0, 1))
        L.check(self._h, self._lib.ktn_get_feasible_row_lambdas(self._h, _p(lam), len(lam)))
        return lam[:self._m0]

    def blocks_feasible_points(self):
        """(x [num_var], info [n_blocks, 8]) of a fused batch: every instance's segment of x_feas (NaN where its found != 1) and its
        record (ktn_blocks_get_feasible_points; needs set_blocks)"""
        n = C.c_int64(0)
        null = C.POINTER(C.c_double)()
        L.check(self._h, self._lib.ktn_blocks_get_feasible_points(self._h, null, 0, null, 0, C.byref(n)))
        x, info = np.zeros(max(self._n0, 1)), np.zeros(max(n.value, 1))
        L.check(self._h, self._lib.ktn_blocks_get_feasible_points(self._h, _p(x), len(x), _p(info), len(info), C.byref(n)))
        return x[:self._n0], info[:n.value].reshape(-1, L.FEAS_INFO_LEN)

    def getfeasiblesolution(self):
        """x_feas, or None when there is none (feasible_point().found != 1)"""
        fp = self.feasible_point()
        return fp.x if fp.found == 1 else None

    def getprimalbound(self):
        """f(x_feas): an upper bound of the optimum for Min, a lower bound for Max; NaN when no feasible point was found"""
        fp = self.feasible_point()
        return fp.objval if fp.found == 1 else float("nan")

    def getcertifiedgap(self):
        """|f(x_feas) - getobjbound()|: for a convex problem the optimum lies between the two"""
        return abs(self.getprimalbound() - self.getobjbound())

    def blocks_duals(self, block):
        """the unscaled multiplier of each cut row of instance `block` after the last device launch, row for row as in
        blocks_cuts(block) (ktn_blocks_get_duals)"""
        n = C.c_int64(0)
        L.check(self._h, self._lib.ktn_blocks_get_duals(self._h, int(block), C.POINTER(C.c_double)(), 0, C.byref(n)))
        y = np.zeros(max(n.value, 1))
        L.check(self._h, self._lib.ktn_blocks_get_duals(self._h, int(block), _p(y), len(y), C.byref(n)))
        return y[:n.value]

    def blocks_dual_bounds(self):
        """[n_blocks, 2] (bound, gap) per instance of a fused batch, each without the loaded problem's objective constant
        (ktn_blocks_get_dual_bounds; needs set_blocks)"""
        n = C.c_int64(0)
        L.check(self._h, self._lib.ktn_blocks_get_dual_bounds(self._h, C.POINTER(C.c_double)(), 0, C.byref(n)))
        out = np.zeros(max(n.value, 1))
        L.check(self._h, self._lib.ktn_blocks_get_dual_bounds(self._h, _p(out), len(out), C.byref(n)))
        return out[:n.value].reshape(-1, 2)

    def numiters(self):
        return int(self._lib.ktn_numiters(self._h))

    def numcuts(self):
        return int(self._lib.ktn_numcuts(self._h))

    def setwarmstart(self, x):            # src/model.jl:335 -- ignores its input
        x = _f64(x)
        self._lib.ktn_setwarmstart(self._h, _p(x), len(x))
        return np.zeros(len(x))

    # ---- supporting-hyperplane cuts: the interior point (ktn_set_interior_point / ktn_get_interior_point) ----
    def set_interior_point(self, x):
        """hand the engine an interior point x_int (the problem's own num_var entries); None clears it"""
        if x is None:
            L.check(self._h, self._lib.ktn_set_interior_point(self._h, C.POINTER(C.c_double)(), 0))
            return
        x = _f64(x)
        L.check(self._h, self._lib.ktn_set_interior_point(self._h, _p(x), len(x)))

    def interior_point(self):
        """the interior point in use (found by the engine or the caller's), or None when there is none"""
        n = self._n0
        x = np.zeros(max(n, 1))
        found = C.c_int32(0)
        L.check(self._h, self._lib.ktn_get_interior_point(self._h, _p(x), len(x), C.byref(found)))
        return x[:n].copy() if found.value else None

    def set_blocks(self, col_offsets):
        """throughput mode: the loaded problem is block-diagonal with these column offsets (ktn_set_blocks)"""
        off = np.ascontiguousarray(col_offsets, dtype=np.int64)
        L.check(self._h, self._lib.ktn_set_blocks(self._h, len(off) - 1, _p(off, C.c_int64)))

    def optimize_blocks(self, cut_capacity=0, supporting=False, fallback=True, warm=False):
        """optimize! of a block-diagonal batch with every instance's whole loop in its own workgroup (ktn_optimize_blocks).
        supporting: cut_algo "supporting_hyperplane[_quad]" runs inside the device-side loop (KTN_BLOCKS_SUPPORTING; tape rows keep
        Kelley's cut there); without it such a handle is refused.  fallback=False (KTN_BLOCKS_NO_FALLBACK): return after the device
        launch with the first status that is not "Optimal" instead of running the ordinary loop.  warm=True (KTN_BLOCKS_WARM): every
        instance starts from its arena of the last device launch -- its cuts, multipliers and x, screened against the bounds in
        force --; do not reset() in between (that drops the warm state, and the call is then the cold launch).  With all keywords
        at their defaults the call is ktn_optimize_blocks itself, otherwise ktn_optimize_blocks_ex.  last_sweep_lambdas() keeps
        describing the sweeps of the host-driven loop only; the lambdas of a device launch come from blocks_cuts()."""
        if not supporting and fallback and not warm:
            return STATUS_SYMBOLS[L.check(self._h, self._lib.ktn_optimize_blocks(self._h, int(cut_capacity)))]
        flags = (L.BLOCKS_SUPPORTING if supporting else 0) | (0 if fallback else L.BLOCKS_NO_FALLBACK) | (L.BLOCKS_WARM if warm else 0)
        return STATUS_SYMBOLS[L.check(self._h, self._lib.ktn_optimize_blocks_ex(self._h, int(cut_capacity), flags))]

    BLOCKS_REWARM_FIELDS = ("state", "lp_rows", "nnz", "dropped_rows", "clamped_cols", "first_proving_row", "crossed_cols", "redundant_rows")

    def blocks_rewarm(self):
        """[n_blocks, 8] records of k_blocks_rewarm on the arenas of the last device launch (ktn_blocks_rewarm; columns:
        BLOCKS_REWARM_FIELDS, state 0 cold / 1 warm / 2 infeasible): the screen against the bounds in force, the clamp of x and the
        compaction that a warm optimize_blocks() would run first.  Idempotent until the next setter or launch."""
        n = C.c_int64(0)
        L.check(self._h, self._lib.ktn_blocks_rewarm(self._h, C.POINTER(C.c_double)(), 0, C.byref(n)))
        out = np.zeros(max(n.value, 1))
        L.check(self._h, self._lib.ktn_blocks_rewarm(self._h, _p(out), len(out), C.byref(n)))
        return out[:n.value].reshape(-1, 8)

    BLOCKS_RESULT_FIELDS = ("status", "iters", "objval", "numcuts", "pdhg_iters", "max_viol", "lp_rows", "overflow")

    def blocks_results(self):
        """[n_blocks, 8] records of the last device launch (ktn_blocks_get_results; columns: BLOCKS_RESULT_FIELDS, the status as its
        KTN_STATUS_* code)"""
        n = C.c_int64(0)
        L.check(self._h, self._lib.ktn_blocks_get_results(self._h, C.POINTER(C.c_double)(), 0, C.byref(n)))
        out = np.zeros(max(n.value, 1))
        L.check(self._h, self._lib.ktn_blocks_get_results(self._h, _p(out), len(out), C.byref(n)))
        return out[:n.value].reshape(-1, 8)

    def blocks_cuts(self, block):
        """the cut rows of instance `block` in its arena after the last device launch (ktn_blocks_get_cuts): dict(rowptr, col --
        global columns --, val, lo, hi, slot -- position in the engine's NL row list --, lam -- 1 for a cut at x* itself)"""
        nr, nz = C.c_int64(0), C.c_int64(0)
        null = lambda t: C.POINTER(t)()
        L.check(self._h, self._lib.ktn_blocks_get_cuts(self._h, int(block), null(C.c_int64), null(C.c_int32), null(C.c_double), null(C.c_double),
                                                       null(C.c_double), null(C.c_int64), null(C.c_double), 0, 0, C.byref(nr), C.byref(nz)))
        rows, nnz = nr.value, nz.value
        rowptr, col, val = np.zeros(rows + 1, dtype=np.int64), np.zeros(max(nnz, 1), dtype=np.int32), np.zeros(max(nnz, 1))
        lo, hi, lam = np.zeros(max(rows, 1)), np.zeros(max(rows, 1)), np.zeros(max(rows, 1))
        slot = np.zeros(max(rows, 1), dtype=np.int64)
        L.check(self._h, self._lib.ktn_blocks_get_cuts(self._h, int(block), _p(rowptr, C.c_int64), _p(col, C.c_int32), _p(val), _p(lo), _p(hi),
                                                       _p(slot, C.c_int64), _p(lam), rows, nnz, C.byref(nr), C.byref(nz)))
        return dict(rowptr=rowptr, col=col[:nnz], val=val[:nnz], lo=lo[:rows], hi=hi[:rows], slot=slot[:rows], lam=lam[:rows])

    def stat(self, name):
        return float(self._lib.ktn_get_stat(self._h, name.encode()))

    # ---- LP introspection ---------------------------------------------------------------
    def lp_rows(self):
        m, nnz = int(self._lib.ktn_lp_num_rows(self._h)), int(self._lib.ktn_lp_nnz(self._h))
        rowptr, col = np.zeros(m + 1, dtype=np.int64), np.zeros(max(nnz, 1), dtype=np.int32)
        val, lo, hi = np.zeros(max(nnz, 1)), np.zeros(max(m, 1)), np.zeros(max(m, 1))
        L.check(self._h, self._lib.ktn_lp_get_rows(self._h, _p(rowptr, C.c_int64), _p(col, C.c_int32), _p(val), _p(lo),
                                                   _p(hi)))
        return rowptr, col[:nnz], val[:nnz], lo[:m], hi[:m]

    def lp_objective(self):
        c = np.zeros(self.num_var)
        c0 = C.c_double(0.0)
        L.check(self._h, self._lib.ktn_lp_get_objective(self._h, _p(c), len(c), C.byref(c0)))
        return c, c0.value

    def lp_duals(self):
        m = int(self._lib.ktn_lp_num_rows(self._h))
        y = np.zeros(max(m, 1))
        L.check(self._h, self._lib.ktn_lp_get_duals(self._h, _p(y), len(y)))
        return y[:m]

    def lp_solve(self, row_tol=1e-7, gap_tol=1e-7):
        st, it = C.c_int32(0), C.c_int64(0)
        L.check(self._h, self._lib.ktn_lp_solve(self._h, row_tol, gap_tol, C.byref(st), C.byref(it)))
        return STATUS_SYMBOLS[st.value], int(it.value)

    # ---- multi-GPU building blocks (include/katana_hip.h "multi-GPU building blocks") ------
    def lp_num_rows(self):
        return int(self._lib.ktn_lp_num_rows(self._h))

    def sweep_lp_point(self, f_tol):
        nv, mv = C.c_int64(0), C.c_double(0.0)
        L.check(self._h, self._lib.ktn_sweep_lp_point(self._h, f_tol, C.byref(nv), C.byref(mv)))
        return int(nv.value), float(mv.value)

    def objective_certificate(self, id_offset=0):
        """this handle's share of sum_i lambda_i * (signed residual of NL row i) at the last sweep's point (signed; the caller
        adds the shares of all handles and clamps at zero)"""
        v = C.c_double(0.0)
        L.check(self._h, self._lib.ktn_objective_certificate(self._h, int(id_offset), C.byref(v)))
        return float(v.value)

    def lp_rows_from(self, first_row):
        nr = self.lp_num_rows() - first_row
        nz = int(self._lib.ktn_lp_nnz_from(self._h, first_row))
        rowptr, col = np.zeros(nr + 1, dtype=np.int64), np.zeros(max(nz, 1), dtype=np.int32)
        val, lo, hi = np.zeros(max(nz, 1)), np.zeros(max(nr, 1)), np.zeros(max(nr, 1))
        L.check(self._h, self._lib.ktn_lp_get_rows_from(self._h, first_row, _p(rowptr, C.c_int64), _p(col, C.c_int32),
                                                        _p(val), _p(lo), _p(hi)))
        return rowptr, col[:nz], val[:nz], lo[:nr], hi[:nr]

    def lp_pack_rows_dev(self, first_row, id_offset, dev_ptr=0, cap=0):
        """(nrows, nnz) of the rows [first_row, M); with a device pointer the packed f64 block of those rows is written there
        (ktn_lp_pack_rows_dev: the device-resident half of the cut exchange)"""
        nr, nz = C.c_int64(0), C.c_int64(0)
        L.check(self._h, self._lib.ktn_lp_pack_rows_dev(self._h, first_row, id_offset, C.c_void_p(dev_ptr or None), cap,
                                                        C.byref(nr), C.byref(nz)))
        return int(nr.value), int(nz.value)

    def lp_append_packed_dev(self, nrows, nnz, dev_ptr):
        L.check(self._h, self._lib.ktn_lp_append_packed_dev(self._h, nrows, nnz, C.c_void_p(dev_ptr or None)))

    def lp_truncate(self, nrows):
        L.check(self._h, self._lib.ktn_lp_truncate(self._h, nrows))

    def lp_purge(self):
        """cut-pool purge between the LP solve and the sweep (as ktn_ecp_step does); returns the number of rows dropped"""
        n = C.c_int64(0)
        L.check(self._h, self._lib.ktn_lp_purge(self._h, C.byref(n)))
        return int(n.value)

    def lp_append_rows(self, rowptr, col, val, lo, hi, nl_id=None):
        """append rows; `nl_id` = global NL-row id of the row each cut belongs to (after lp_enable_global_lists)"""
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
        nr = len(rowptr) - 1
        if nr <= 0:
            return
        col = np.ascontiguousarray(col, dtype=np.int32)
        val, lo, hi = _f64(val), _f64(lo), _f64(hi)
        colp = col if len(col) else np.zeros(1, dtype=np.int32)
        valp = val if len(val) else np.zeros(1)
        if nl_id is None:
            idp = C.POINTER(C.c_int64)()
        else:
            nl_id = np.ascontiguousarray(nl_id, dtype=np.int64)
            assert len(nl_id) == nr
            idp = _p(nl_id, C.c_int64)
        L.check(self._h, self._lib.ktn_lp_append_rows_nl(self._h, nr, _p(rowptr, C.c_int64), _p(colp, C.c_int32), _p(valp),
                                                         _p(lo), _p(hi), idp))

    def set_cut_exchange(self, cb, first_nl_id):
        """ktn_set_cut_exchange: `cb` is an _lib.EXCHANGE_CB instance the caller keeps alive (None removes it)"""
        ptr = C.cast(cb, C.c_void_p) if cb is not None else None
        L.check(self._h, self._lib.ktn_set_cut_exchange(self._h, ptr, None, int(first_nl_id)))

    def lp_enable_global_lists(self, nl_total):
        L.check(self._h, self._lib.ktn_lp_enable_global_lists(self._h, int(nl_total)))

    def last_sweep_slots(self):
        """local NL slots of the cuts the last sweep appended, in row order"""
        n = C.c_int64(0)
        L.check(self._h, self._lib.ktn_last_sweep_slots(self._h, C.POINTER(C.c_int64)(), 0, C.byref(n)))
        out = np.zeros(max(int(n.value), 1), dtype=np.int64)
        if n.value:
            L.check(self._h, self._lib.ktn_last_sweep_slots(self._h, _p(out, C.c_int64), len(out), C.byref(n)))
        return out[:int(n.value)]

    def last_sweep_lambdas(self):
        """lambda of each cut the last sweep appended (order of last_sweep_slots): the cut was taken at
        x_int + lambda (x* - x_int); 1 = Kelley's cut at x*"""
        n = C.c_int64(0)
        L.check(self._h, self._lib.ktn_last_sweep_lambdas(self._h, C.POINTER(C.c_double)(), 0, C.byref(n)))
        out = np.ones(max(int(n.value), 1))
        if n.value:
            L.check(self._h, self._lib.ktn_last_sweep_lambdas(self._h, _p(out), len(out), C.byref(n)))
        return out[:int(n.value)]

    def lp_pdhg_raw(self, x0, y0, eta, omega, iters):
        x0, y0 = _f64(x0), _f64(y0)
        m = int(self._lib.ktn_lp_num_rows(self._h))
        xo, yo = np.zeros(self.num_var), np.zeros(max(m, 1))
        y0p = y0 if len(y0) else np.zeros(1)
        L.check(self._h, self._lib.ktn_lp_pdhg_raw(self._h, _p(x0), _p(y0p), eta, omega, iters, _p(xo), _p(yo)))
        return xo, yo[:m]

    def lp_script(self, x, y, x0, y0, eta, omega, k, ops, identity=True, packed=False, no_spec=False):
        """ktn_lp_script: ops (L.LPOP_*) from the state (x, y) with anchors (x0, y0), all given in the stored LP's space.
        Returns a dict of the SCALED x, y, x0, y0, xt, yt, the 32 check sums q, xnext / ynext (None unless the last check left
        them), and the scaling dr, dc."""
        n, m = self.num_var, int(self._lib.ktn_lp_num_rows(self._h))
        pad = lambda a: a if len(a) else np.zeros(1)
        ins = [pad(_f64(a)) for a in (x, y, x0, y0)]
        assert len(ins[0]) == len(ins[2]) == n and (m == 0 or len(ins[1]) == len(ins[3]) == m)
        ops = np.ascontiguousarray(ops, dtype=np.int32)
        flags = (L.LPS_IDENTITY if identity else 0) | (L.LPS_PACKED if packed else 0) | (L.LPS_NO_SPEC if no_spec else 0)
        o = {k_: np.zeros(n) for k_ in ("x", "x0", "xt", "xnext", "dc")}
        o.update({k_: np.zeros(max(m, 1)) for k_ in ("y", "y0", "yt", "ynext", "dr")})
        o["q"] = np.zeros(32)
        spec = C.c_int32(0)
        L.check(self._h, self._lib.ktn_lp_script(
            self._h, _p(ins[0]), _p(ins[1]), _p(ins[2]), _p(ins[3]), eta, omega, int(k), flags,
            _p(ops if len(ops) else np.zeros(1, dtype=np.int32), C.c_int32), len(ops), _p(o["x"]), _p(o["y"]), _p(o["x0"]),
            _p(o["y0"]), _p(o["xt"]), _p(o["yt"]), _p(o["q"]), _p(o["xnext"]), _p(o["ynext"]), C.byref(spec), _p(o["dr"]),
            _p(o["dc"])))
        for k_ in ("y", "y0", "yt", "ynext", "dr"):
            o[k_] = o[k_][:m]
        o["spec"] = bool(spec.value)
        if not o["spec"]:
            o["xnext"] = o["ynext"] = None
        return o

    def lp_scaling(self):
        """ktn_lp_scaling: (dr, dc, dr_r, dc_r) of a fresh equilibration of the current LP (needs lp_ruiz_warm > 0)"""
        n, m = self.num_var, int(self._lib.ktn_lp_num_rows(self._h))
        dr, drr, dc, dcr = np.zeros(max(m, 1)), np.zeros(max(m, 1)), np.zeros(n), np.zeros(n)
        L.check(self._h, self._lib.ktn_lp_scaling(self._h, _p(dr), _p(dc), _p(drr), _p(dcr)))
        return dr[:m], dc, drr[:m], dcr


class KatanaHipSeparator:
    """The first-order separator (KatanaFirstOrderSeparator, src/separators.jl:58-120) in batched,
    device-resident form.  precompute!/isconstrsat/gencut keep the reference's per-row meaning;
    `sweep` is the whole loop body of src/model.jl:272-283 in one call."""

    def __init__(self, model):
        self.m = model
        self.xstar = None

    def initialize(self):                         # src/separators.jl:81-107
        lib, h = self.m._lib, self.m._h
        mrows, nnz = int(lib.ktn_sep_num_constr(h)), int(lib.ktn_sep_jac_nnz(h))
        self.rowptr, self.col = np.zeros(mrows + 1, dtype=np.int64), np.zeros(max(nnz, 1), dtype=np.int32)
        L.check(h, lib.ktn_sep_get_structure(h, _p(self.rowptr, C.c_int64), _p(self.col, C.c_int32)))
        self.col = self.col[:nnz]
        self.num_constr, self.nnz = mrows, nnz
        self.sp_cols = [self.col[self.rowptr[i]:self.rowptr[i + 1]] for i in range(mrows)]

    def precompute(self, xstar):                  # src/separators.jl:111-116
        x = _f64(xstar)
        L.check(self.m._h, self.m._lib.ktn_sep_precompute(self.m._h, _p(x), len(x)))
        self.xstar = x
        self.g = np.zeros(max(self.num_constr, 1))
        self.jac = np.zeros(max(self.nnz, 1))
        L.check(self.m._h, self.m._lib.ktn_sep_get_g(self.m._h, _p(self.g), self.num_constr))
        L.check(self.m._h, self.m._lib.ktn_sep_get_jac(self.m._h, _p(self.jac), self.nnz))
        self.g, self.jac = self.g[:self.num_constr], self.jac[:self.nnz]

    def isconstrsat(self, i, lb, ub, f_tol):      # src/separators.jl:120
        return bool(L.check(self.m._h, self.m._lib.ktn_sep_isconstrsat(self.m._h, i, lb, ub, f_tol)))

    def gencut(self, xstar, bounds, i):           # src/separators.jl:118 -> (cols, coefs, constant)
        cap = int(self.rowptr[i + 1] - self.rowptr[i])
        cols, coefs = np.zeros(max(cap, 1), dtype=np.int32), np.zeros(max(cap, 1))
        nnz, const = C.c_int64(cap), C.c_double(0.0)
        L.check(self.m._h, self.m._lib.ktn_sep_gencut(self.m._h, i, _p(cols, C.c_int32), _p(coefs), C.byref(nnz),
                                                      C.byref(const)))
        return cols[:nnz.value], coefs[:nnz.value], const.value

    def sweep(self, f_tol):
        nv, mv = C.c_int64(0), C.c_double(0.0)
        L.check(self.m._h, self.m._lib.ktn_sep_sweep(self.m._h, f_tol, C.byref(nv), C.byref(mv)))
        return int(nv.value), float(mv.value)


# ---- src/util.jl ---------------------------------------------------------------------------
def getKatanaModel(m):                            # src/util.jl:3-5
    return m.internal_model if hasattr(m, "internal_model") else m


def getKatanaCuts(m):
    """src/util.jl:16-34: table M x (N+2): coefficients, constant, direction (-1 '<=', +1 '>=')
    of every LP row (the reference lists the rows recorded under :VisData)."""
    m = getKatanaModel(m)
    rowptr, col, val, lo, hi = m.lp_rows()
    M, N = len(lo), m.num_var
    table = np.zeros((M, N + 2))
    for i in range(M):
        for e in range(rowptr[i], rowptr[i + 1]):
            table[i, col[e]] += val[e]
        if np.isfinite(hi[i]) and not np.isfinite(lo[i]):
            table[i, N], table[i, N + 1] = hi[i], -1
        elif np.isfinite(lo[i]) and not np.isfinite(hi[i]):
            table[i, N], table[i, N + 1] = lo[i], 1
        else:
            raise AssertionError("range or free row: not an inequality (src/util.jl:27-29)")
    return table


def getKatanaSols(m):                             # src/util.jl:36
    m = getKatanaModel(m)
    k = int(m._lib.ktn_num_lp_sols(m._h))
    out = []
    for i in range(k):
        x = np.zeros(m.num_var)
        L.check(m._h, m._lib.ktn_get_lp_sol(m._h, i, _p(x), len(x)))
        out.append(x)
    return out


class LinearQuadraticModel(KatanaNonlinearModel):
    """MathProgBase.LinearQuadraticModel(s::KatanaSolver)  src/solver.jl:46 -- the LP / QP / QCQP surface the reference presents
    through NonlinearToLPQPBridge, stated natively: the rows go to the engine as KTN_ROW_QUAD rows (nlp.QuadNLP), not as
    expressions.  Indices are 0-based.

        loadproblem(A, collb, colub, obj, rowlb, rowub, sense)    A dense or scipy-sparse, sense "Min" / "Max"
        setquadobj(rowidx, colidx, vals)                          objective + 1/2 x'Qx, an off-diagonal pair given once
        addquadconstr(linidx, linval, quadrowidx, quadcolidx, quadval, sense, rhs)     sum linval x + sum quadval x_r x_c {'<', '>'} rhs
        optimize()                                                assembles the QuadNLP, loads it and solves

    (quad_triplets_to_engine holds both conversions.)  The 8-argument loadproblem(num_var, num_constr, ..., d) of
    NonlinearModel keeps working on it, and the getters are inherited.

    The engine sees the problem only inside optimize() and forgets its interior point at every load, so set_interior_point(x) on
    the 7-argument path keeps x on this object and hands it over after each such load; set_interior_point(None) clears it."""

    def __init__(self, solver):
        super().__init__(solver)
        self._lq = None
        self._xint_pending = None

    def loadproblem(self, *args):
        if len(args) == 8:
            self._lq = None
            self._xint_pending = None
            return super().loadproblem(*args)
        if len(args) != 7:
            raise TypeError("loadproblem(A, collb, colub, obj, rowlb, rowub, sense) or loadproblem(num_var, num_constr, l_var, "
                            "u_var, l_constr, u_constr, sense, d)")
        A, collb, colub, obj, rowlb, rowub, sense = args
        if sense not in ("Min", "Max"):
            raise ValueError("sense must be 'Min' or 'Max'")
        if hasattr(A, "tocsr"):
            A = A.tocsr()
            A.sum_duplicates()
            m, n = A.shape
            rp, ci, av = np.asarray(A.indptr, dtype=np.int64), np.asarray(A.indices, dtype=np.int64), _f64(A.data)
        else:
            A = np.asarray(A, dtype=np.float64)
            if A.ndim != 2:
                A = A.reshape(0, len(np.atleast_1d(collb)))
            m, n = A.shape
            nz = A != 0.0
            rp = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int64)
            ci, av = np.nonzero(nz)[1].astype(np.int64), A[nz]
        collb, colub, obj, rowlb, rowub = _f64(collb), _f64(colub), _f64(obj), _f64(rowlb), _f64(rowub)
        if not (len(collb) == len(colub) == len(obj) == n and len(rowlb) == len(rowub) == m):
            raise ValueError("loadproblem: array lengths do not match A (%d x %d)" % (m, n))
        rows = [(ci[rp[i]:rp[i + 1]], av[rp[i]:rp[i + 1]], [], [], [], 0.0) for i in range(m)]
        self._lq = dict(n=n, collb=collb, colub=colub, obj=obj, sense=sense, rows=rows, lb=list(rowlb), ub=list(rowub),
                        objq=None, dirty=True)
        self._xint_pending = None

    def set_interior_point(self, x):
        q = self._lq
        if q is None:                                    # the 8-argument path: the problem is loaded, the engine keeps the point
            return super().set_interior_point(x)
        if x is not None:
            x = _f64(x).copy()
            if len(x) != q["n"]:
                raise ValueError("set_interior_point: %d entries for %d variables" % (len(x), q["n"]))
        self._xint_pending = x
        if not q["dirty"]:                               # already loaded and unchanged since: the engine can take it now
            super().set_interior_point(x)

    # the 7-argument path keeps the problem on this object: a change before the load (or while it is dirty) goes into it alone,
    # a change after the load also goes to the engine, which keeps its cuts (setobj: as long as the new cost's non-zeros lie where
    # the loaded cost's did; otherwise the LP is loaded again at the next optimize())
    def setvarbounds(self, l, u):
        q = self._lq
        if q is None:
            return super().setvarbounds(l, u)
        l = None if l is None else _f64(l).copy()
        u = None if u is None else _f64(u).copy()
        for v in (l, u):
            if v is not None and len(v) != q["n"]:
                raise ValueError("setvarbounds: %d entries for %d variables" % (len(v), q["n"]))
        if not q["dirty"]:
            super().setvarbounds(l, u)
        if l is not None:
            q["collb"] = l
        if u is not None:
            q["colub"] = u

    def setconstrbounds(self, lb, ub):
        q = self._lq
        if q is None:
            return super().setconstrbounds(lb, ub)
        lb = None if lb is None else _f64(lb).copy()
        ub = None if ub is None else _f64(ub).copy()
        m = len(q["lb"])                                 # (the rows of loadproblem and those of addquadconstr after them)
        for v in (lb, ub):
            if v is not None and len(v) != m:
                raise ValueError("setconstrbounds: %d entries for %d constraints" % (len(v), m))
        if not q["dirty"]:
            super().setconstrbounds(lb, ub)              # (refused: the kept state below stays as it is)
        if lb is not None:
            q["lb"] = list(lb)
        if ub is not None:
            q["ub"] = list(ub)

    def setobj(self, c, c0=0.0):
        q = self._lq
        if q is None:
            return super().setobj(c, c0)
        c = _f64(c).copy()
        if len(c) != q["n"]:
            raise ValueError("setobj: %d entries for %d variables" % (len(c), q["n"]))
        if c0 != 0.0:
            raise ValueError("setobj: the 7-argument loadproblem has no objective constant")
        if np.any(np.isnan(c)):
            raise ValueError("setobj: a coefficient is NaN")
        if not q["dirty"]:
            # The engine keeps the loaded cost's sparsity pattern (QuadNLP stores the non-zeros of obj) and refuses a non-zero
            # outside it.  This object holds the whole LP, so such a cost is not an error here: the problem is marked for a
            # re-load, and the next optimize() solves it cold with the new cost.
            try:
                super().setobj(c, 0.0)
            except L.KatanaHipError as e:
                if e.code != L.E_INVALID:
                    raise
                q["dirty"] = True
        q["obj"] = c

    def _need_lq(self):
        if self._lq is None:
            raise RuntimeError("no LP loaded: call loadproblem(A, collb, colub, obj, rowlb, rowub, sense) first")
        return self._lq

    def setquadobj(self, rowidx, colidx, vals):
        q = self._need_lq()
        q["objq"] = quad_triplets_to_engine(rowidx, colidx, vals, "objective")
        q["dirty"] = True

    def addquadconstr(self, linidx, linval, quadrowidx, quadcolidx, quadval, sense, rhs):
        q = self._need_lq()
        if sense not in ("<", ">", "="):
            raise ValueError("addquadconstr: sense must be '<', '>' or '='")
        qr, qc, qv = quad_triplets_to_engine(quadrowidx, quadcolidx, quadval, "constraint")
        q["rows"].append((np.asarray(linidx, dtype=np.int64), _f64(linval), qr, qc, qv, 0.0))
        q["lb"].append(-np.inf if sense == "<" else float(rhs))
        q["ub"].append(np.inf if sense == ">" else float(rhs))
        q["dirty"] = True

    def optimize(self):
        q = self._lq
        if q is not None and q["dirty"]:
            from .nlp import QuadNLP
            d = QuadNLP(q["n"], q["obj"], 0.0, q["objq"], q["rows"])
            KatanaNonlinearModel.loadproblem(self, q["n"], len(q["rows"]), q["collb"], q["colub"], q["lb"], q["ub"], q["sense"], d)
            q["dirty"] = False
            if self._xint_pending is not None:
                KatanaNonlinearModel.set_interior_point(self, self._xint_pending)
        return super().optimize()
