"""Multi-GPU ECP: NL rows sharded by contiguous blocks, replicated LP, one exchange of the
generated cuts per ECP iteration (no counterpart in the serial reference).

One process per GPU (torch.distributed; backend "nccl" is RCCL over xGMI on ROCm, "gloo" on
CPU for the tests).  Given x*, every nonlinear row is evaluated and cut independently
(`for i in m.nlconstr_ixs`, src/model.jl:272-283), so rank r sweeps only its block of rows.
The cuts are then all-gathered -- two collectives per iteration: the (rows, nnz) counts together with the
status flags and the largest violation, then the cut blocks padded to the largest -- and appended on every rank in RANK ORDER, so that all
ranks hold the identical LP and the deterministic GPU LP gives them the identical x*.

The loop below is the host-level statement of Engine::step (csrc/ecp.hip) with the exchange
between sweep and append; it drives the same kernels through the C ABI.
"""
import numpy as np

from .instances import SeparableInstance
from .nlp import SeparableNLP
from .solver import NonlinearModel


def shard_bounds(m_nl, rank, world):
    """contiguous block [lo, hi) of the NL rows owned by `rank`"""
    return (m_nl * rank) // world, (m_nl * (rank + 1)) // world


def shard_instance(inst, rank, world):
    """all linear rows + this rank's block of NL rows (same variables, same objective)"""
    lo, hi = shard_bounds(inst.m_nl, rank, world)
    rp = np.asarray(inst.rowptr)
    ml = inst.m_lin
    a, b = rp[ml + lo], rp[ml + hi]
    keep = np.concatenate([np.arange(0, rp[ml]), np.arange(a, b)])
    rows = np.concatenate([np.arange(0, ml), np.arange(ml + lo, ml + hi)])
    new_rp = np.concatenate([rp[:ml + 1], rp[ml] + (rp[ml + lo + 1:ml + hi + 1] - a)])
    return SeparableInstance(
        n=inst.n, l_var=inst.l_var, u_var=inst.u_var, sense=inst.sense, rowptr=new_rp.astype(np.int64),
        col=np.asarray(inst.col)[keep], kind=np.asarray(inst.kind)[keep], p0=np.asarray(inst.p0)[keep],
        p1=np.asarray(inst.p1)[keep], rconst=np.asarray(inst.rconst)[rows], l_constr=np.asarray(inst.l_constr)[rows],
        u_constr=np.asarray(inst.u_constr)[rows], obj_col=inst.obj_col, obj_kind=inst.obj_kind, obj_p0=inst.obj_p0,
        obj_p1=inst.obj_p1, obj_const=inst.obj_const, xhat=inst.xhat, opt_obj=inst.opt_obj, m_lin=ml, m_nl=hi - lo,
        meta=dict(inst.meta, shard=(rank, world)))


def pack_block(rowptr, col, val, lo, hi, ids=None):
    """one f64 buffer: [rowptr[1:], col, val, lo, hi(, global NL-row ids)]  (integers are exact in f64)"""
    parts = [np.asarray(rowptr[1:], dtype=np.float64), np.asarray(col, dtype=np.float64),
             np.asarray(val, dtype=np.float64), np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)]
    if ids is not None:
        parts.append(np.asarray(ids, dtype=np.float64))
    return np.concatenate(parts)


def unpack_block(buf, nrows, nnz, with_ids=False):
    o = 0
    rp = np.concatenate([[0], buf[o:o + nrows].astype(np.int64)]); o += nrows
    col = buf[o:o + nnz].astype(np.int32); o += nnz
    val = buf[o:o + nnz].copy(); o += nnz
    lo = buf[o:o + nrows].copy(); o += nrows
    hi = buf[o:o + nrows].copy(); o += nrows
    if with_ids:
        return rp, col, val, lo, hi, buf[o:o + nrows].astype(np.int64)
    return rp, col, val, lo, hi


def exchange_cuts(dist, block, device="cpu", scalars=None):
    """All-gather one cut block per rank.  `block` = (rowptr, col, val, lo, hi[, ids]) of the local cuts.
    Returns the list of blocks in rank order.  With dist=None (single process) it is the identity.
    `scalars` = (a, b, ...): floats that ride along with the size exchange; the call then returns
    (blocks, max over ranks of a, max over ranks of b, ...) -- the loop's status flags need no collective of their own."""
    import torch
    with_ids = len(block) == 6
    rowptr, col, val, lo, hi = block[:5]
    ids = block[5] if with_ids else None
    nrows, nnz = len(lo), len(col)
    import os
    if dist is None or (dist.get_world_size() == 1 and not os.environ.get("KTN_FORCE_COLLECTIVE")):
        return [block] if scalars is None else ([block],) + tuple(float(v) for v in scalars)
    world = dist.get_world_size()
    sc = () if scalars is None else tuple(float(v) for v in scalars)
    counts = torch.tensor([float(nrows), float(nnz)] + list(sc), dtype=torch.float64, device=device)
    all_counts = [torch.zeros_like(counts) for _ in range(world)]
    dist.all_gather(all_counts, counts)                       # collective 1: sizes (+ the scalars)
    all_counts = [c.cpu() for c in all_counts]
    maxima = tuple(max(float(c[2 + k]) for c in all_counts) for k in range(len(sc)))
    all_counts = [(int(c[0]), int(c[1])) for c in all_counts]
    blocks = _gather_blocks(dist, device, world, all_counts, with_ids, rowptr, col, val, lo, hi, ids)
    return blocks if scalars is None else (blocks,) + maxima


def _gather_blocks(dist, device, world, all_counts, with_ids, rowptr, col, val, lo, hi, ids):
    import torch
    width = max((4 if with_ids else 3) * r + 2 * z for r, z in all_counts)
    if width == 0:
        empty = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0), np.zeros(0))
        return [empty + ((np.zeros(0, dtype=np.int64),) if with_ids else ()) for _ in range(world)]
    send = torch.zeros(width, dtype=torch.float64, device=device)
    payload = pack_block(rowptr, col, val, lo, hi, ids)
    send[:len(payload)] = torch.from_numpy(payload).to(device)
    recv = [torch.empty(width, dtype=torch.float64, device=device) for _ in range(world)]
    dist.all_gather(recv, send)                               # collective 2: padded cut blocks
    return [unpack_block(recv[r].cpu().numpy(), *all_counts[r], with_ids=with_ids) for r in range(world)]


def exchange_cuts_dev(dist, model, first_row, id_offset, scalars):
    """The same exchange with the cut blocks resident in device memory from the sweep that generated them to the LP that
    receives them (the north star's "RCCL all-gather of generated cuts over xGMI"): the engine packs the rows [first_row, M)
    into a torch CUDA tensor (ktn_lp_pack_rows_dev), `dist.all_gather` moves the padded blocks between the GPUs -- RCCL when
    the process group is "nccl"; a gloo group (tests: ranks sharing one GPU) cannot gather CUDA tensors and stages that one
    call through the host -- and every rank's block is appended from the receive buffer (ktn_lp_append_packed_dev).  Only
    the sizes / flags per rank cross to the host.  Returns (rows appended, max over ranks of scalars[0], of scalars[1], ...);
    the model's own rows >= first_row are replaced by the gathered ones, in rank order.  scalars[1] is the status flag: with
    any rank at >= 2 nothing is moved."""
    import torch
    world = dist.get_world_size()
    nccl = dist.get_backend() == "nccl"
    nr, nz = model.lp_pack_rows_dev(first_row, id_offset)
    sc = [float(v) for v in scalars]
    counts = torch.tensor([float(nr), float(nz)] + sc, dtype=torch.float64, device="cuda" if nccl else "cpu")
    all_counts = [torch.zeros_like(counts) for _ in range(world)]
    dist.all_gather(all_counts, counts)                       # collective 1: sizes (+ the scalars)
    all_counts = [c.cpu() for c in all_counts]
    maxima = tuple(max(float(c[2 + k]) for c in all_counts) for k in range(len(sc)))
    sizes = [(int(c[0]), int(c[1])) for c in all_counts]
    width = max(4 * r + 2 * z for r, z in sizes)
    if width == 0 or maxima[1] >= 2.0:                        # nothing to move, or some rank's LP failed: the caller leaves the loop
        model.lp_truncate(first_row)
        return (0,) + maxima
    # (torch.empty, not zeros: a fill kernel on torch's stream would race with the engine's pack kernel on ITS stream; the
    #  padding behind a rank's 4 r + 2 z doubles is never read)
    send = torch.empty(width, dtype=torch.float64, device="cuda")
    model.lp_pack_rows_dev(first_row, id_offset, send.data_ptr(), width)
    model.lp_truncate(first_row)
    recv = [torch.empty(width, dtype=torch.float64, device="cuda") for _ in range(world)]
    if nccl:
        dist.all_gather(recv, send)                           # collective 2: padded cut blocks, device to device
    else:
        host = [torch.empty(width, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(host, send.cpu())
        for r in range(world):
            recv[r].copy_(host[r])
    torch.cuda.current_stream().synchronize()                 # the engine reads the buffers on its own stream
    total = 0
    for r, (rows, nnz) in enumerate(sizes):                   # rank order => identical LP everywhere
        model.lp_append_packed_dev(rows, nnz, recv[r].data_ptr())
        total += rows
    return (total,) + maxima


class ShardedKatanaModel:
    """KatanaNonlinearModel over `world` GPUs: same getters, same stepping interface."""

    def __init__(self, solver, inst, rank, world, dist=None, exchange_device=None):
        self.rank, self.world, self.dist = rank, world, dist
        solver.gpu_options = dict(solver.gpu_options)
        if world > 1 and "cut_cap_factor" not in solver.gpu_options:
            # deepest-cut selection works per shard: split the cap so that the gathered LP gets what one GPU would add
            import ctypes as C
            from . import _lib as L
            dp = L.KtnParams()
            L.lib().ktn_default_params(C.byref(dp))
            solver.gpu_options["cut_cap_factor"] = dp.cut_cap_factor / world
            solver.gpu_options.setdefault("cut_cap_min", max(1, dp.cut_cap_min // world))
        self.p = dict(solver.model_params)
        self.inst = inst
        self.local = shard_instance(inst, rank, world)
        self.m = NonlinearModel(solver)
        self.m.loadproblem(self.local.n, self.local.num_constr, self.local.l_var, self.local.u_var,
                           self.local.l_constr, self.local.u_constr, self.local.sense, SeparableNLP(self.local))
        # cuts carry the global id of their NL row, so that every rank's engine threads them into the per-row cut lists
        # (dual inheritance, stall consolidation, purging) exactly as the single-GPU sweep does for its own cuts
        self.shard_lo = shard_bounds(inst.m_nl, rank, world)[0]
        self.m.lp_enable_global_lists(inst.m_nl)
        prm = self.m.params
        self.tol = dict(scale=prm.lp_tol_scale, floor=prm.lp_tol_floor, cap=prm.lp_tol_cap, gfloor=prm.lp_gap_floor,
                        gcap=prm.lp_gap_cap)
        # "cuda": the cut blocks stay in device memory end to end (exchange_cuts_dev; the default over RCCL); "cpu": blocks are
        # downloaded, gathered as host tensors and uploaded again (exchange_cuts; gloo groups, world 1)
        if exchange_device is None:
            exchange_device = "cpu" if (dist is None or dist.get_backend() == "gloo") else "cuda"
        self.exchange_device = exchange_device
        self.num_var = self.m.num_var
        self._reset_state()
        from . import _lib as L
        import weakref
        me = weakref.ref(self)                                     # (no reference cycle model -> callback -> model: the engine
                                                                   #  handle is destroyed when the last user reference goes)

        def trampoline(user, what, first_new_row, scalars, nscalars):
            obj = me()
            return obj._exchange(user, what, first_new_row, scalars, nscalars) if obj is not None else 1
        self._cb = L.EXCHANGE_CB(trampoline)                       # kept alive with the model
        self.m.set_cut_exchange(self._cb, self.shard_lo)

    def _reset_state(self):
        self.exchanged_rows = 0

    def reset(self):
        self.m.reset()
        self._reset_state()

    # ---- the exchange step of one cutting-plane round: what Engine::step calls where the single-GPU loop sweeps ------------
    def _exchange(self, user, what, first_new_row, scalars, nscalars):
        """ktn_exchange_cb (include/katana_hip.h).  what = 0: this rank's engine has just swept its block of NL rows; its new LP
        rows are the rows from `first_new_row` on.  Every rank's new rows are appended to every rank's LP in rank order; scalars[0]
        <- rows appended in total, scalars[1:] <- the maximum over the ranks of what was there (largest violation, status flags,
        the two values the loop's decisions ride on).  what = 1: scalars <- their sum over the ranks (certificate shares).
        The loop itself -- tolerance schedule, floor rule, purge, refinement -- is Engine::step on every rank (round 4: one
        implementation; until round 3 this class re-stated those rules on top of the building blocks)."""
        try:
            import os
            n = int(nscalars)
            vals = [float(scalars[k]) for k in range(n)]
            collective = self.dist is not None and (self.world > 1 or bool(os.environ.get("KTN_FORCE_COLLECTIVE")))
            if what == 1:
                if collective:
                    import torch
                    t = torch.tensor(vals, dtype=torch.float64, device="cuda" if self.dist.get_backend() == "nccl" else "cpu")
                    self.dist.all_reduce(t)
                    vals = [float(v) for v in t.tolist()]
                for k in range(n):
                    scalars[k] = vals[k]
                return 0
            m0 = int(first_new_row)
            sc = tuple(vals[1:])                                   # (largest violation, flag, extra0, extra1)
            if self.exchange_device == "cuda" and collective:
                total, *maxima = exchange_cuts_dev(self.dist, self.m, m0, self.shard_lo, sc)
            else:
                if vals[2] < 2.0:
                    block = tuple(self.m.lp_rows_from(m0)) + (self.shard_lo + self.m.last_sweep_slots(),)
                else:                                              # this rank's LP failed: an empty block, the flag does the rest
                    block = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0), np.zeros(0),
                             np.zeros(0, dtype=np.int64))
                self.m.lp_truncate(m0)
                blocks, *maxima = exchange_cuts(self.dist, block, self.exchange_device, scalars=sc)
                total = 0
                if maxima[1] < 2.0:
                    for rp, col, val, lo, hi, ids in blocks:       # rank order => identical LP everywhere
                        self.m.lp_append_rows(rp, col, val, lo, hi, ids)
                        total += len(lo)
            self.exchanged_rows += total
            scalars[0] = float(total)
            for k, v in enumerate(maxima):
                scalars[1 + k] = float(v)
            return 0
        except Exception as e:                                     # never raise across the C ABI
            import sys
            print("cut-exchange callback failed: %r" % (e,), file=sys.stderr, flush=True)
            return 1

    def optimize_begin(self):
        self.m.optimize_begin()          # box-bounded shards: no presolve work, starts the solve timer

    def ecp_step(self):
        """one pass of src/model.jl:258-308 across all ranks (Engine::step on every rank, the exchange through _exchange);
        returns True when the loop ends"""
        return self.m.ecp_step()

    def optimize_end(self):
        return self.m.optimize_end()

    def optimize(self):
        self.optimize_begin()
        while not self.ecp_step():
            pass
        return self.optimize_end()

    # getters of the plugin surface
    def status(self): return self.m.status()
    def getobjval(self): return self.m.getobjval()
    def getsolution(self): return self.m.getsolution()
    def getsolvetime(self): return self.m.getsolvetime()
    def numiters(self): return self.m.numiters()
    def numcuts(self): return self.m.numcuts()
    def lp_num_rows(self): return self.m.lp_num_rows()
    @property
    def iter(self): return self.m.numiters()
    @property
    def purged_rows(self): return int(self.m.stat("purged_rows"))
    @property
    def cert_refinements(self): return int(self.m.stat("cert_refinements"))
    @property
    def polish_iters(self): return int(self.m.stat("polish_iters"))
    def stat(self, name):
        return float(getattr(self, name)) if name == "exchanged_rows" else self.m.stat(name)


# =====================================================================================================================
# Row-sharded LP: every rank keeps the cuts it generates, x is replicated, A'y is a local
# partial plus ONE all-reduce of an n-vector per PDHG iteration -- inside the engine, on its own stream (include/
# katana_hip.h "row-sharded LP").  No cut exchange, no host loop: ktn_optimize itself is the collective call.
# =====================================================================================================================
def shard_rows(inst, rank, world):
    """rank's shard for the row-sharded LP: all variables and the objective, the block [m_lin r / w, m_lin (r+1) / w) of the
    linear rows and the block of the NL rows given by shard_bounds"""
    if getattr(inst, "quad_ptr", None) is not None or np.any(np.asarray(getattr(inst, "row_kind", ())) == 3):
        raise ValueError("shard_rows: KTN_ROW_QUAD rows cannot be row-sharded (their Q segments are not split)")
    ml = inst.m_lin
    l0, l1 = (ml * rank) // world, (ml * (rank + 1)) // world
    n0, n1 = shard_bounds(inst.m_nl, rank, world)
    rp = np.asarray(inst.rowptr)
    rows = np.concatenate([np.arange(l0, l1), np.arange(ml + n0, ml + n1)])
    keep = np.concatenate([np.arange(rp[l0], rp[l1]), np.arange(rp[ml + n0], rp[ml + n1])])
    lens = np.diff(rp)[rows]
    new_rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return SeparableInstance(
        n=inst.n, l_var=inst.l_var, u_var=inst.u_var, sense=inst.sense, rowptr=new_rp,
        col=np.asarray(inst.col)[keep], kind=np.asarray(inst.kind)[keep], p0=np.asarray(inst.p0)[keep],
        p1=np.asarray(inst.p1)[keep], rconst=np.asarray(inst.rconst)[rows], l_constr=np.asarray(inst.l_constr)[rows],
        u_constr=np.asarray(inst.u_constr)[rows], obj_col=inst.obj_col, obj_kind=inst.obj_kind, obj_p0=inst.obj_p0,
        obj_p1=inst.obj_p1, obj_const=inst.obj_const, xhat=inst.xhat, opt_obj=inst.opt_obj, m_lin=l1 - l0, m_nl=n1 - n0,
        meta=dict(inst.meta, row_shard=(rank, world)))


def make_allreduce_callback(dist):
    """ktn_allreduce_cb over torch.distributed (any backend that reduces CPU tensors, i.e. gloo): the engine hands over a host
    buffer, the reduction happens in place."""
    import ctypes as C
    import torch
    from . import _lib as L

    def cb(_user, buf, count, op):
        try:
            t = torch.from_numpy(np.ctypeslib.as_array(buf, (int(count),)))
            dist.all_reduce(t, op=dist.ReduceOp.MAX if op else dist.ReduceOp.SUM)
            return 0
        except Exception:                       # never unwind through the C ABI
            return 1
    return L.ALLREDUCE_CB(cb)


class RowShardedKatanaModel:
    """KatanaNonlinearModel over `world` GPUs with the LP itself sharded by rows.  Same getters and stepping interface as the
    single-GPU model; optimize / ecp_step / lp_solve are collective calls (every rank must make them)."""

    def __init__(self, solver, inst, rank, world, dist=None, transport="auto"):
        import ctypes as C
        from . import _lib as L
        self.rank, self.world, self.dist = rank, world, dist
        self.inst = shard_rows(inst, rank, world) if world > 1 else inst
        self.m = NonlinearModel(solver)
        lib, h = self.m._lib, self.m._h
        self._cb = None
        import os
        forced = world == 1 and dist is not None and bool(os.environ.get("KTN_FORCE_COLLECTIVE"))   # one-rank RCCL test
        if world > 1 or forced:
            fallback = "rccl" if dist.get_backend() == "nccl" else "callback"
            if transport == "auto":
                # over RCCL's backend with several GPUs: PROBE -- the peer-buffer transport (an n-vector all-reduce in ~12 us instead
                # of a 2 (w - 1)-hop ring) where its self-test passes on every rank of this box, RCCL otherwise
                transport = os.environ.get("KTN_DIST_TRANSPORT") or ("probe" if (dist.get_backend() == "nccl" and world > 1) else fallback)
            if transport == "probe":
                transport = "ipc" if self._probe_ipc(C, L, lib, h, inst, rank, world, dist) else fallback
                self.probe_verdict = transport
            elif transport == "ipc":
                # peer-buffer transport (include/katana_hip.h): export this rank's buffers, gather everybody's handles, map them
                import torch
                cap = int(inst.n) + 64                       # (+ epigraph column; the scalar reductions need far less)
                mine = C.create_string_buffer(128)
                L.check(h, lib.ktn_dist_ipc_export(h, rank, world, cap, mine))
                dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
                t = torch.tensor(list(mine.raw), dtype=torch.uint8, device=dev)
                got = [torch.zeros_like(t) for _ in range(world)]
                dist.all_gather(got, t)
                raw = b"".join(bytes(g.cpu().tolist()) for g in got)
                L.check(h, lib.ktn_dist_init_ipc(h, rank, world, raw))
                # self-test before any solve rests on it: a sum and a max every rank can check for itself
                _, err = self.allreduce_probe(min(cap, 1 << 16), 2)
                if not err <= 1e-9:
                    raise RuntimeError("peer-buffer transport failed its self-test on rank %d: deviation %g" % (rank, err))
            if transport == "ipc":
                pass
            elif transport == "rccl":
                import torch
                uid = C.create_string_buffer(128)
                if rank == 0:
                    L.check(h, lib.ktn_dist_unique_id(uid))
                dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
                t = torch.tensor(list(uid.raw), dtype=torch.uint8, device=dev)
                dist.broadcast(t, src=0)
                raw = bytes(t.cpu().tolist())
                L.check(h, lib.ktn_dist_init_rccl(h, raw, rank, world))
            else:
                self._cb = make_allreduce_callback(dist)
                L.check(h, lib.ktn_dist_init_callback(h, rank, world, C.cast(self._cb, C.c_void_p), None))
        self.transport = transport if (world > 1 or forced) else "none"
        s = self.inst
        self.m.loadproblem(s.n, s.num_constr, s.l_var, s.u_var, s.l_constr, s.u_constr, s.sense, SeparableNLP(s))

    def _probe_ipc(self, C, L, lib, h, inst, rank, world, dist):
        """Try the peer-buffer transport and keep it only if EVERY rank could export, map and pass the self-test
        (ktn_dist_allreduce_probe: six rounds of changing contents through both slots, sum and max, against values each rank
        computes itself -- on several GPUs this is the test of the cross-GPU visibility rule the protocol rests on, which one GPU
        cannot exercise).  Every step is followed by a vote (all-reduce MIN), so all ranks take the same branch; a rank that
        failed leaves the transport again (ktn_dist_release_ipc) and the caller falls back to RCCL -- decided once, at init,
        in the same process."""
        import os
        import torch
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"

        def vote(ok):
            t = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            return bool(t.item() > 0.5)

        cap = int(inst.n) + 64
        mine = C.create_string_buffer(128)
        ok = lib.ktn_dist_ipc_export(h, rank, world, cap, mine) == 0 and not (os.environ.get("KTN_DIST_PROBE_FAIL") == str(rank))
        t = torch.tensor(list(mine.raw), dtype=torch.uint8, device=dev)
        got = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(got, t)
        if not vote(ok):
            lib.ktn_dist_release_ipc(h)
            return False
        raw = b"".join(bytes(g.cpu().tolist()) for g in got)
        ok = lib.ktn_dist_init_ipc(h, rank, world, raw) == 0
        if not vote(ok):
            lib.ktn_dist_release_ipc(h)
            return False
        us, err = C.c_double(0.0), C.c_double(1.0)
        ok = lib.ktn_dist_allreduce_probe(h, min(cap, 1 << 16), 2, C.byref(us), C.byref(err)) == 0 and err.value <= 1e-9
        if not vote(ok):
            lib.ktn_dist_release_ipc(h)
            return False
        return True

    def __getattr__(self, name):                # getters, stepping interface, stats: those of the local handle
        return getattr(self.m, name)

    def allreduce_probe(self, n, reps=20):
        """(mean microseconds of one all-reduce of n doubles through this handle's transport, largest deviation of a sum / max
        all-reduce from the value every rank can compute itself).  Collective call."""
        import ctypes as C
        from . import _lib as L
        us, err = C.c_double(0.0), C.c_double(0.0)
        L.check(self.m._h, self.m._lib.ktn_dist_allreduce_probe(self.m._h, int(n), int(reps), C.byref(us), C.byref(err)))
        return us.value, err.value

    def numcuts_global(self):
        """cuts generated on all ranks (numcuts() is this rank's count; the linear rows are counted once, src/model.jl:77)"""
        import torch
        t = torch.tensor([float(self.m.numcuts())], dtype=torch.float64)
        if self.world > 1:
            if self.dist.get_backend() == "nccl":
                t = t.cuda()
            self.dist.all_reduce(t)
        return int(t.item())
