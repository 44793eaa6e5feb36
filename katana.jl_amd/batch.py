"""Throughput mode: a batch of independent convex NLPs (BASELINE.json configs[4]; SURVEY.md section 8e
"replicas only": no communication).

Every instance gets its own engine handle, hence its own HIP stream; `threads` host threads drive
the handles concurrently (ctypes releases the GIL for the duration of every ktn_* call), so the GPU
sees up to `threads` independent kernel streams at once -- small instances (n ~ 1e3) occupy a few
workgroups each and many of them fit on the 256 CUs side by side."""
import time
from concurrent.futures import ThreadPoolExecutor

from .nlp import SeparableNLP, Problem, fuse_problems
from .solver import NonlinearModel


def _as_problem(item):
    """a Problem of a jump_like.Model (Model.problem()), a SeparableInstance (SeparableNLP) or a Problem"""
    if isinstance(item, Problem):
        return item
    if hasattr(item, "problem"):
        return item.problem()
    return Problem(item.n, item.num_constr, item.l_var, item.u_var, item.l_constr, item.u_constr, item.sense, SeparableNLP(item))


def _all_instances(items):
    from .instances import SeparableInstance
    return all(isinstance(i, SeparableInstance) for i in items)


def solve_batch(solver, instances, threads=16, describe=SeparableNLP, fused=False, per_instance_lp=False, device_loop=None):
    """Solve every instance; returns (results, wall_seconds).  results[i] = dict(status, objval, iters,
    numcuts, x) in the order of `instances`.  The items are SeparableInstances or -- expression-built and declared-quadratic
    models, tape and KTN_ROW_QUAD rows included -- Problems (katana_jl_amd.Problem: the arguments of loadproblem!) or
    jump_like.Models; a fused batch of the latter is the block-diagonal union of nlp.fuse_problems (a quadratic objective
    becomes the instance's own epigraph row there), and each instance's objective is reported in its own sense.

    fused=True solves the block-diagonal union of the instances as ONE problem (instances.fuse_instances): the
    cutting-plane loop, the sweep and every PDHG launch then serve the whole batch at once, and the stop rule --
    every nonlinear row of every instance within f_tol -- is the conjunction of the per-instance stop rules.
    Iteration counts are then those of the union (the slowest instance), objectives are split per instance.
    With per_instance_lp every LP re-solve of the fused problem is ONE launch with one workgroup per instance
    (ktn_set_blocks, csrc/batch_lp.hpp: iterates in LDS, restarts and termination per instance) instead of the global
    first-order loop.  Measured on 512 x cfg5: 2.5x fewer instance-iterations in total, but every
    cutting-plane round still waits for its slowest instance, so the batch takes 0.26 s against 0.22 s -- hence off by default.
    With device_loop (the default for fused batches) the WHOLE cutting-plane loop of every instance runs inside its own
    workgroup (ktn_optimize_blocks, csrc/batch_ecp.hpp): no instance waits for another; 0.10 s for 512 x cfg5.  Batches it does
    not cover (host rows, nonlinear objective, free variables) fall back to the host-driven loop inside the call."""
    if device_loop is None:
        device_loop = fused and not per_instance_lp
    if fused:
        return _solve_fused(solver, instances, per_instance_lp, device_loop)
    def work(inst):
        m = NonlinearModel(solver)
        if isinstance(inst, Problem) or hasattr(inst, "problem"):
            m.loadproblem(*_as_problem(inst))
        else:
            m.loadproblem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr, inst.u_constr, inst.sense,
                          describe(inst))
        status = m.optimize()
        return dict(status=status, objval=m.getobjval(), iters=m.numiters(), numcuts=m.numcuts(), x=m.getsolution(),
                    pdhg_iters=m.stat("pdhg_iters"))

    t0 = time.perf_counter()
    if threads <= 1:
        out = [work(i) for i in instances]
    else:
        with ThreadPoolExecutor(max_workers=threads) as ex:
            out = list(ex.map(work, instances))
    return out, time.perf_counter() - t0


def fuse_points(points, offs, nvar=None):
    """Per-instance vectors -> one vector in the fused column layout of instances.fuse_instances / nlp.fuse_problems: instance k's
    entries start at offs[k].  nvar[k] = the instance's own number of variables where fusion appended a column to it (the epigraph
    variable of a quadratic objective), which is padded with 0; None: every instance fills its whole range."""
    import numpy as np
    if len(points) != len(offs) - 1:
        raise ValueError("one point per instance: %d points for %d instances" % (len(points), len(offs) - 1))
    out = np.zeros(int(offs[-1]))
    for k, pt in enumerate(points):
        pt = np.asarray(pt, dtype=np.float64).reshape(-1)
        own = int(nvar[k]) if nvar is not None else int(offs[k + 1] - offs[k])
        if len(pt) != own or own > int(offs[k + 1] - offs[k]):
            raise ValueError("instance %d has %d variables, its point %d entries" % (k, own, len(pt)))
        out[int(offs[k]):int(offs[k]) + own] = pt
    return out


class FusedBatch:
    """A batch loaded ONCE as one block-diagonal problem (instances.fuse_instances + ktn_loadproblem [+ ktn_set_blocks]); solve()
    can then be called repeatedly -- every call after the first starts from the loaded state (ktn_reset) -- with the batch's
    data resident in HBM.  bench.py --workload cfg5 times solve() alone; solve_batch(fused=True) is load + one solve()."""

    def __init__(self, solver, instances, per_instance_lp=False, device_loop=True):
        self.device_loop = device_loop
        self.per_instance_lp = per_instance_lp
        self.m = NonlinearModel(solver)
        self.load(instances)

    def load(self, instances):
        """(re)load a batch on this handle: a process that serves batch after batch keeps its handle -- and with it the
        engine's device buffers -- instead of making a new one per batch (512 x cfg5: 0.14 s per batch against 0.20 s)"""
        import numpy as np
        from .instances import fuse_instances
        self.instances = instances
        self._bounds = None                                         # (set_var_bounds: the fused bounds in force, once they differ from the loaded ones)
        self._row_bounds = None                                     # (set_row_bounds: the same for the constraint bounds)
        if not _all_instances(instances):                         # Problems / Models, tape and QUAD rows allowed (nlp.fuse_problems)
            probs = [_as_problem(i) for i in instances]
            self.big, self.offs, self._objinfo = fuse_problems(probs, allow_quad=True)
            self._nvar = [int(p.num_var) for p in probs]            # (a quadratic objective adds its epigraph variable behind them)
            self.m.loadproblem(*self.big)
            if self.per_instance_lp or self.device_loop:
                self.m.set_blocks(self.offs)
            self._solved = False
            return self
        self._objinfo = None
        self.big, self.offs = fuse_instances(instances)
        big = self.big
        self.m.loadproblem(big.n, big.num_constr, big.l_var, big.u_var, big.l_constr, big.u_constr, big.sense, SeparableNLP(big))
        if self.per_instance_lp or self.device_loop:
            self.m.set_blocks(self.offs)
        self._obj = (np.asarray(big.obj_kind), np.asarray(big.obj_p0), np.asarray(big.obj_p1), np.asarray(big.obj_col))
        self._solved = False
        return self

    def set_interior_points(self, points):
        """Interior points of the instances, one per instance (each with the instance's own num_var entries), concatenated into
        the fused layout and handed to the engine (ktn_set_interior_point).  Where fusion gave an instance an epigraph variable
        (a quadratic objective, nlp.fuse_problems) that column is padded with 0: no row that takes part reads it.  None clears
        the point: the engine then solves the auxiliary problem of the fused batch -- ONE problem over every instance, by the
        host-driven loop -- when it next needs a point."""
        if points is None:
            self.m.set_interior_point(None)
            return None
        xi = fuse_points(points, self.offs, self._nvar if self._objinfo is not None else None)
        self.m.set_interior_point(xi)
        return xi

    # ---- new bounds or costs on the loaded batch (ktn_set_var_bounds / ktn_set_linear_objective) ----
    def _own_nvar(self):
        return self._nvar if self._objinfo is not None else [int(self.offs[k + 1] - self.offs[k]) for k in range(len(self.instances))]

    def set_var_bounds(self, l_list, u_list):
        """New variable bounds per instance, each vector in the instance's own variables; None (for a side, or for one instance
        of a side) keeps what is loaded.  The vectors are concatenated in the fused column order and set in place; the next
        solve() runs every instance with them.  Where fusion gave an instance an epigraph variable (a quadratic objective), its
        interval [-R, R] is worked out again for the new box (nlp.quad_objective_bound)."""
        import numpy as np
        from .nlp import quad_objective_bound
        nv, offs = self._own_nvar(), self.offs
        cur = [np.array(self.big.l_var, dtype=np.float64).reshape(-1), np.array(self.big.u_var, dtype=np.float64).reshape(-1)]
        if getattr(self, "_bounds", None) is not None:
            cur = [self._bounds[0].copy(), self._bounds[1].copy()]
        touched = set()
        for side, lst in enumerate((l_list, u_list)):
            if lst is None:
                continue
            if len(lst) != len(self.instances):
                raise ValueError("one bound vector per instance: %d for %d instances" % (len(lst), len(self.instances)))
            for k, v in enumerate(lst):
                if v is None:
                    continue
                v = np.asarray(v, dtype=np.float64).reshape(-1)
                if len(v) != int(nv[k]):
                    raise ValueError("instance %d has %d variables, its bound vector %d entries" % (k, int(nv[k]), len(v)))
                cur[side][int(offs[k]):int(offs[k]) + int(nv[k])] = v
                touched.add(k)
        for k in sorted(touched):
            o, n_k = int(offs[k]), int(nv[k])
            if self._objinfo is not None and int(offs[k + 1]) - o > n_k:          # the instance's own epigraph variable
                R = quad_objective_bound(_as_problem(self.instances[k]).d, cur[0][o:o + n_k], cur[1][o:o + n_k], k)
                cur[0][o + n_k], cur[1][o + n_k] = -R, R
        self.m.setvarbounds(cur[0], cur[1])
        self._bounds = cur
        return cur

    def set_row_bounds(self, lb_list, ub_list):
        """New constraint bounds per instance (ktn_set_row_bounds), each vector over the instance's own rows in its own row order;
        None (for a side, or for one instance of a side) keeps what is in force.  The vectors are placed at the instance's rows of
        the fused problem (_row_ranges) and set in place.  The epigraph row that fusion gave a quadratic objective keeps its
        bounds.  Fusion negates the objective of a "Max" instance, never its rows: the bounds go in as given.  With a device
        launch standing the resident arenas are updated by the same call, so solve(warm=True) continues from each instance's own
        cuts; solve() starts from the loaded rows with the new bounds."""
        import numpy as np
        cur = [np.array(self.big.l_constr, dtype=np.float64).reshape(-1), np.array(self.big.u_constr, dtype=np.float64).reshape(-1)]
        if getattr(self, "_row_bounds", None) is not None:
            cur = [self._row_bounds[0].copy(), self._row_bounds[1].copy()]
        ranges = self._row_ranges()
        for side, lst in enumerate((lb_list, ub_list)):
            if lst is None:
                continue
            if len(lst) != len(self.instances):
                raise ValueError("one bound vector per instance: %d for %d instances" % (len(lst), len(self.instances)))
            for k, v in enumerate(lst):
                if v is None:
                    continue
                v = np.asarray(v, dtype=np.float64).reshape(-1)
                idx = ranges[k][0]
                if len(v) != len(idx):
                    raise ValueError("instance %d has %d constraints, its bound vector %d entries" % (k, len(idx), len(v)))
                cur[side][idx] = v
        self.m.setconstrbounds(cur[0], cur[1])
        self._row_bounds = cur
        return cur

    def set_costs(self, c_list):
        """New linear cost vectors per instance, each dense over the instance's own variables and in its own sense (None keeps an
        instance's cost); constants stay.  The fused objective is separable of linear atoms, so the engine's cost setter applies;
        an instance whose quadratic objective became an epigraph row at fusion keeps its objective (ValueError)."""
        import numpy as np
        nv, offs, m = self._own_nvar(), self.offs, self.m
        if len(c_list) != len(self.instances):
            raise ValueError("one cost vector per instance: %d for %d instances" % (len(c_list), len(self.instances)))
        c, c0 = m.lp_objective()
        c = np.array(c[:int(offs[-1])], dtype=np.float64)
        own = {}
        for k, ck in enumerate(c_list):
            if ck is None:
                continue
            ck = np.asarray(ck, dtype=np.float64).reshape(-1)
            o, n_k = int(offs[k]), int(nv[k])
            if len(ck) != n_k:
                raise ValueError("instance %d has %d variables, its cost vector %d entries" % (k, n_k, len(ck)))
            if int(offs[k + 1]) - o > n_k:
                raise ValueError("instance %d: its quadratic objective is an epigraph row of the fused problem, not a cost vector" % k)
            sgn = -1.0 if (self._objinfo is not None and _as_problem(self.instances[k]).sense == "Max") else 1.0
            c[o:o + n_k] = sgn * ck
            own[k] = ck
        m.setobj(c, c0)
        if self._objinfo is not None:
            for k, ck in own.items():
                cols, _, c0k = self._objinfo[k]
                self._objinfo[k] = (cols, ck[cols].copy(), c0k)
        else:
            kind, _, p1, col = self._obj
            self._obj = (kind, c[col], p1, col)
        return c

    def solve(self, cut_capacity=0, supporting=None, warm=False, fallback=True):
        """cut_capacity: cuts per NL row an instance's arena has room for in the device-side loop (0: the engine's default, 12);
        an instance that outgrows it sends the batch to the host-driven loop (stat ecp_blocks_fallbacks).
        supporting: supporting-hyperplane cuts inside the device-side loop (ktn_optimize_blocks_ex, KTN_BLOCKS_SUPPORTING); None =
        on when the solver's cut_algo is not Kelley's and device_loop is set.  (m.last_sweep_lambdas() describes host-loop sweeps
        only; the cuts of a device launch and their lambdas are m.blocks_cuts(k).)
        warm: every instance starts from its own cuts, multipliers and x of the last device launch on this handle (KTN_BLOCKS_WARM;
        after set_var_bounds / set_costs, or with unchanged data); the handle is NOT reset in between.  An instance whose new box is
        empty ends "Infeasible" alone: the statuses per instance are column 0 of m.blocks_results(), the status returned is the
        first that is not "Optimal".
        fallback=False: KTN_BLOCKS_NO_FALLBACK."""
        import numpy as np
        from .instances import atom_value_deriv
        m, big, offs = self.m, self.big, self.offs
        if supporting is None:
            supporting = bool(self.device_loop) and int(m.params.cut_algo) != 0
        warm = bool(warm) and bool(self.device_loop)
        if self._solved and not warm:
            m.reset()
        self._solved = True
        if self.device_loop:
            status = m.optimize_blocks(cut_capacity, supporting=bool(supporting), fallback=bool(fallback), warm=warm)
        else:
            status = m.optimize()
        x = m.getsolution()
        common = dict(status=status, iters=m.numiters(), numcuts=None, pdhg_iters=m.stat("pdhg_iters"),
                      blk_lp_launches=m.stat("blk_lp_launches"), blk_lp_fallbacks=m.stat("blk_lp_fallbacks"),
                      blk_pdhg_iters_sum=m.stat("blk_pdhg_iters_sum"), ecp_blocks_launches=m.stat("ecp_blocks_launches"),
                      ecp_blocks_fallbacks=m.stat("ecp_blocks_fallbacks"), ecp_blocks_pdhg_sum=m.stat("ecp_blocks_pdhg_sum"),
                      ecp_blocks_esh_rows=m.stat("ecp_blocks_esh_rows"))
        if self._objinfo is not None:
            # each instance's objective in its own sense, from its own LIN coefficients and constant on its slice of x
            common["ecp_blocks_tape_rows"] = m.stat("ecp_blocks_tape_rows")
            common["ecp_blocks_quad_rows"] = m.stat("ecp_blocks_quad_rows")
            out = []
            for k, (cols, coefs, c0) in enumerate(self._objinfo):
                xk = x[offs[k]:offs[k + 1]]
                out.append(dict(common, objval=float(np.sum(coefs * xk[cols]) + c0), x=xk[:self._nvar[k]]))
            return out
        # per-instance objectives: all atoms of the fused objective at once, then sums by instance
        kind, p0, p1, col = self._obj
        val, _ = atom_value_deriv(kind, p0, p1, x[col])
        optr = big.meta["obj_ptr"]
        seg = np.zeros(len(self.instances))
        nz = np.flatnonzero(np.diff(optr) > 0)                    # (instances with an empty objective are not reduceat starts)
        if len(nz):
            seg[nz] = np.add.reduceat(val, optr[:-1][nz])
        return [dict(common, objval=float(seg[k] + inst.obj_const), x=x[offs[k]:offs[k + 1]]) for k, inst in enumerate(self.instances)]


    # ---- Lagrange multipliers, reduced costs, dual bounds per instance ----
    def _row_ranges(self):
        """per instance: the index arrays of its rows in the fused problem, in the instance's own row order (the epigraph row
        that fusion gave a quadratic objective left out), and its sign (+1 Min, -1 Max: fusion negates a Max objective)"""
        import numpy as np
        if self._objinfo is None:                                  # fuse_instances: linear rows of every instance, then the NL rows
            lo = np.concatenate([[0], np.cumsum([i.m_lin for i in self.instances])])
            no = np.concatenate([[0], np.cumsum([i.m_nl for i in self.instances])]) + lo[-1]
            return [(np.concatenate([np.arange(lo[k], lo[k + 1]), np.arange(no[k], no[k + 1])]), 1.0) for k in range(len(self.instances))]
        probs = [_as_problem(i) for i in self.instances]           # fuse_problems: rows instance after instance
        epi = [int(self.offs[k + 1] - self.offs[k]) - self._nvar[k] for k in range(len(probs))]
        ro = np.concatenate([[0], np.cumsum([int(p.num_constr) + e for p, e in zip(probs, epi)])])
        return [(np.arange(ro[k], ro[k] + int(p.num_constr)), -1.0 if p.sense == "Max" else 1.0) for k, p in enumerate(probs)]

    def constr_duals(self):
        """one array per instance: its constraint duals in its own row order and sense (KatanaNonlinearModel.getconstrduals)"""
        d = self.m.getconstrduals()
        return [sgn * d[idx] for idx, sgn in self._row_ranges()]

    def reduced_costs(self):
        """one array per instance: the reduced costs of its own variables, in its own sense"""
        z = self.m.getreducedcosts()
        nv = self._nvar if self._objinfo is not None else [int(self.offs[k + 1] - self.offs[k]) for k in range(len(self.instances))]
        return [sgn * z[int(self.offs[k]):int(self.offs[k]) + int(nv[k])] for k, (_, sgn) in enumerate(self._row_ranges())]

    def dual_bounds(self):
        """[(bound, gap)] per instance, in its own sense and with its own objective constant: instance k's share of the fused
        bound from its rows and columns alone (k_dual_bound, one workgroup per instance).  A batch solved by the host loop has no
        blocks set: they are set for the call and cleared again."""
        m = self.m
        temp = not (self.per_instance_lp or self.device_loop)
        if temp:
            m.set_blocks(self.offs)
        try:
            bg = m.blocks_dual_bounds()
        finally:
            if temp:
                m.set_blocks([0])
        out = []
        for k, (_, sgn) in enumerate(self._row_ranges()):
            c0 = float(self._objinfo[k][2]) if self._objinfo is not None else float(self.instances[k].obj_const)
            out.append((sgn * float(bg[k, 0]) + c0, float(bg[k, 1])))
        return out


    # ---- a feasible point per instance ----
    def feasible_points(self):
        """one FeasiblePoint per instance (KatanaNonlinearModel.feasible_point), in the instance's own variables -- the epigraph
        variable that fusion gave a quadratic objective left out --, rows and sense: x_feas on the segment from the instance's
        reference point (set_interior_points) to its part of the solution, lambda_b over the instance's own rows (1 for an
        instance without nonlinear rows), objval its share of the fused objective in its own sense with its own constant.  An
        instance whose reference point fails gets found = -1 and a NaN x; the others are not affected.  A batch solved by the host
        loop has no blocks set: they are set for the call and cleared again.
        (The epigraph column of a quadratic objective is padded with 0 in the reference point, so such an instance has a usable
        reference point only where its objective is <= 0 there; its objval is the epigraph variable at x_feas, an upper estimate.)"""
        import numpy as np
        from .solver import FeasiblePoint
        m = self.m
        temp = not (self.per_instance_lp or self.device_loop)
        if temp:
            m.set_blocks(self.offs)
        try:
            x, info = m.blocks_feasible_points()
        finally:
            if temp:
                m.set_blocks([0])
        nv = self._nvar if self._objinfo is not None else [int(self.offs[k + 1] - self.offs[k]) for k in range(len(self.instances))]
        out = []
        for k, (idx, sgn) in enumerate(self._row_ranges()):
            r = info[k]
            c0 = float(self._objinfo[k][2]) if self._objinfo is not None else float(self.instances[k].obj_const)
            row = int(r[5])
            if row >= 0:                                            # a row of the fused problem -> the instance's own row index
                own = np.flatnonzero(idx == row)
                row = int(own[0]) if len(own) else -1
            out.append(FeasiblePoint(int(r[0]), x[int(self.offs[k]):int(self.offs[k]) + int(nv[k])].copy(), float(r[1]), sgn * float(r[2]) + c0,
                                     float(r[3]), float(r[4]), row, int(r[6]), int(r[7])))
        return out


def _solve_fused(solver, instances, per_instance_lp=False, device_loop=False):
    t0 = time.perf_counter()
    out = FusedBatch(solver, instances, per_instance_lp, device_loop).solve()
    return out, time.perf_counter() - t0


def shard_range(count, rank, world):
    """contiguous block of `count` items owned by `rank` (sizes differ by at most one)"""
    return (count * rank) // world, (count * (rank + 1)) // world


def solve_batch_sharded(solver, instances, rank, world, dist=None, gather=True, **kw):
    """Throughput mode over several GPUs (SURVEY.md section 8e "batch mode: replicas only, no communication"): rank r solves
    the contiguous block shard_range(len(instances), r, world) of the batch on ITS device as one fused batch (solve_batch,
    fused=True by default: every instance's loop inside its own workgroup).  The data path has no collective.  With
    gather=True the per-instance results are exchanged afterwards through `dist.all_gather_object` (host objects: statuses,
    objectives, solutions) so that every rank returns the results of the whole batch, in the order of `instances`; with
    gather=False a rank returns only its own block.  Returns (results, wall_seconds of this rank's solve)."""
    lo, hi = shard_range(len(instances), rank, world)
    kw.setdefault("fused", True)
    mine, wall = solve_batch(solver, instances[lo:hi], **kw) if hi > lo else ([], 0.0)
    if not gather or dist is None or world == 1:
        return mine, wall
    parts = [None] * world
    dist.all_gather_object(parts, mine)
    return [r for part in parts for r in part], wall
