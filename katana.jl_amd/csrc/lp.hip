// lp.hip -- solve(m.linear_model) (src/model.jl:259; GLPK in the reference): restarted reflected-Halpern PDHG and the exact small / mid-size LPs  (struct Engine: engine.hpp)
#include "engine.hpp"
#include "launch.hpp"
#include "kernels.hpp"
#include "pdhg_check.hpp"
#include "dense_lp.hpp"
#include "mid_lp.hpp"
#include "batch_lp.hpp"

namespace ktn {

// --------------------------------------------------------------- reductions ---
double Engine::dev_dot(int64_t n, const double* a, const double* b) {
    launch(k_dot_partial, kRedBlocks, kBlock, 0, stream, n, a, b, partials.p);
    launch(k_sum_final, 1, kRedBlocks, 0, stream, partials.p, kRedBlocks, chkout.p + 2 * kChkQ);
    double v = 0.0;
    KTN_HIP(hipMemcpyAsync(&v, chkout.p + 2 * kChkQ, sizeof(double), hipMemcpyDeviceToHost, stream));
    sync();
    return v;
}

double Engine::dev_finite_sq(int64_t n, const double* a) {
    launch(k_finite_sq_partial, kRedBlocks, kBlock, 0, stream, n, a, partials.p);
    launch(k_sum_final, 1, kRedBlocks, 0, stream, partials.p, kRedBlocks, chkout.p + 2 * kChkQ);
    double v = 0.0;
    KTN_HIP(hipMemcpyAsync(&v, chkout.p + 2 * kChkQ, sizeof(double), hipMemcpyDeviceToHost, stream));
    sync();
    return v;
}

// out = A'v over the mirror: G lanes per column, a 1024-thread workgroup per long column
void Engine::spmv_cols(const SpMat& AT, const double* v, double* out, hipEvent_t e0, hipEvent_t e1) {
    const int64_t n = n_lp;
    if (n_longc > 0) {
        // (timed as a pair: the first kernel's start, the second one's stop)
        with_group(grp_cols, [&](auto g) { launch_timed(k_spmv_skip<g()>, group_grid(n, g()), kBlock, 0, stream, e0, nullptr, n, AT, v, out, kLongRow); });
        launch_timed(k_spmv_long, (unsigned)n_longc, 1024, 0, stream, nullptr, e1, d_longcols.p, AT, v, out);
    } else {
        with_group(grp_cols, [&](auto g) { launch_timed(k_spmv<g()>, group_grid(n, g()), kBlock, 0, stream, e0, e1, n, AT, v, out); });
    }
}

void Engine::compute_scaling(bool identity) {
    dr.resize((size_t)std::max<int64_t>(M, 1), stream);
    dc.resize((size_t)n_lp, stream);
    statr.resize((size_t)std::max<int64_t>(M, 1), stream);
    statc.resize((size_t)n_lp, stream);
    // Warm start (lp_ruiz_warm > 0): rows are only ever appended, so the Ruiz (max-norm) equilibration of the previous solve
    // -- kept in dr_r / dc_r as it was BEFORE that solve's Pock-Chambolle pass -- already fits all but the new rows.  Those
    // start at 1 and lp_ruiz_warm passes replace the lp_ruiz_iters passes from scratch; the Pock-Chambolle pass (which
    // carries the ||A^||_2 <= 1 guarantee) is applied afresh.  (Warm-starting from the FINAL scaling instead compounds the
    // Pock-Chambolle passes of all earlier solves: cfg3 then needs 3.5x the PDHG iterations.)
    const bool warm = !identity && prm.lp_ruiz_warm > 0 && scal_rows > 0 && scal_rows <= M && scal_cols == n_lp;
    dr_r.resize((size_t)std::max<int64_t>(M, 1), stream);
    dc_r.resize((size_t)n_lp, stream);
    if (warm) {
        KTN_HIP(hipMemcpyAsync(dr.p, dr_r.p, (size_t)scal_rows * sizeof(double), hipMemcpyDeviceToDevice, stream));
        KTN_HIP(hipMemcpyAsync(dc.p, dc_r.p, (size_t)n_lp * sizeof(double), hipMemcpyDeviceToDevice, stream));
        launch_n(k_fill, M - scal_rows, stream, M - scal_rows, dr.p + scal_rows, 1.0);
        stats["lp_scaling_warm"] += 1.0;
    } else {
        launch_n(k_fill, M, stream, M, dr.p, 1.0);
        launch_n(k_fill, n_lp, stream, n_lp, dc.p, 1.0);
    }
    const int gr = pick_group((double)NNZ / (double)std::max<int64_t>(M, 1));
    const int gc = pick_group((double)NNZ / (double)std::max<int64_t>(n_lp, 1));
    const double cap_c = w_shift ? 1e3 : kInf;          // (kernels.hpp k_scale_apply2)
    if (!identity && (M > 0 || row_sharded())) {
        const int passes = warm ? prm.lp_ruiz_warm : prm.lp_ruiz_iters;
        for (int it = 0; it <= passes; ++it) {
            const int mode = (it == passes) ? 1 : 0;   // last pass: Pock-Chambolle (alpha = 1)
            if (mode == 1 && prm.lp_ruiz_warm > 0) {
                KTN_HIP(hipMemcpyAsync(dr_r.p, dr.p, (size_t)M * sizeof(double), hipMemcpyDeviceToDevice, stream));
                KTN_HIP(hipMemcpyAsync(dc_r.p, dc.p, (size_t)n_lp * sizeof(double), hipMemcpyDeviceToDevice, stream));
            }
            if (n_long == 0 && n_longc == 0 && !row_sharded() && M > 0) {
                // statistic + update of BOTH sides in one launch, into new arrays that are swapped in (9 launches; round 1: 33, round 2: 22)
                dr2.resize((size_t)M, stream); dc2.resize((size_t)n_lp, stream);
                const unsigned br = group_grid(M, gr), bc = group_grid(n_lp, gc);
                launch(k_scale_stat_upd_both, br + bc, kBlock, 0, stream, M, lp_rowptr.p, lp_col.p, Wval(), n_lp, c_ptr.p, c_row.p, c_val.p, dr.p, dc.p, mode,
                       dr2.p, dc2.p, cap_c, gr, gc, br);
                dr.swap(dr2); dc.swap(dc2);
                stats["lp_scale_fused_passes"] += 1.0;
                continue;
            }
            if (n_long > 0) {
                with_group(gr, [&](auto g) {
                    launch(k_scale_stat_skip<g()>, group_grid(M, g()), kBlock, 0, stream, M, lp_rowptr.p, lp_col.p, Wval(), dr.p, dc.p, mode, statr.p, kLongRow);
                });
                launch(k_scale_stat_long, (unsigned)n_long, 1024, 0, stream, d_longrows.p, lp_rowptr.p, lp_col.p, Wval(), dr.p, dc.p, mode, statr.p);
            } else {
                with_group(gr, [&](auto g) {
                    launch(k_scale_stat<g()>, group_grid(M, g()), kBlock, 0, stream, M, lp_rowptr.p, lp_col.p, Wval(), dr.p, dc.p, mode, statr.p);
                });
            }
            if (n_longc > 0) {
                with_group(gc, [&](auto g) {
                    launch(k_scale_stat_skip<g()>, group_grid(n_lp, g()), kBlock, 0, stream, n_lp, c_ptr.p, c_row.p, c_val.p, dc.p, dr.p, mode, statc.p,
                           kLongRow);
                });
                launch(k_scale_stat_long, (unsigned)n_longc, 1024, 0, stream, d_longcols.p, c_ptr.p, c_row.p, c_val.p, dc.p, dr.p, mode, statc.p);
            } else {
                with_group(gc, [&](auto g) {
                    launch(k_scale_stat<g()>, group_grid(n_lp, g()), kBlock, 0, stream, n_lp, c_ptr.p, c_row.p, c_val.p, dc.p, dr.p, mode, statc.p);
                });
            }
            if (row_sharded()) {                       // a column's max / sum runs over the rows of every rank
                if (M == 0) launch_n(k_fill, n_lp, stream, n_lp, statc.p, 0.0);
                allreduce(statc.p, (size_t)n_lp, mode ? 0 : 1);
            }
            launch_n(k_scale_apply2, std::max(M, n_lp), stream, M, dr.p, statr.p, n_lp, dc.p, statc.p, cap_c);
            stats["lp_scale_split_passes"] += 1.0;
        }
    }
    scal_rows = identity ? 0 : M;
    scal_cols = n_lp;
    r_sval.resize((size_t)NNZ + 1, stream);
    c_sval.resize((size_t)NNZ + 1, stream);
    // (long columns: the mirror's scaled values are gathered entry-parallel from the row copy instead of walked column by column)
    if (n_longc > 0 || M == 0) {
        with_group(gr, [&](auto g) { launch(k_scale_vals<g()>, group_grid(M, g()), kBlock, 0, stream, M, lp_rowptr.p, lp_col.p, Wval(), dr.p, dc.p, r_sval.p); });
        if (n_longc > 0) launch_n(k_csc_vals, NNZ, stream, NNZ, c_perm.p, r_sval.p, c_sval.p);
        else with_group(gc, [&](auto g) { launch(k_scale_vals<g()>, group_grid(n_lp, g()), kBlock, 0, stream, n_lp, c_ptr.p, c_row.p, c_val.p, dc.p, dr.p, c_sval.p); });
    } else {                                            // both copies in one launch
        const unsigned br = group_grid(M, gr), bc = group_grid(n_lp, gc);
        launch(k_scale_vals_both, br + bc, kBlock, 0, stream, M, lp_rowptr.p, lp_col.p, Wval(), n_lp, c_ptr.p, c_row.p, c_val.p, dr.p, dc.p, r_sval.p, c_sval.p,
               gr, gc, br);
    }
    check_launch();
}

void Engine::launch_tiled(const TiledBuf& T, int64_t n_out, int64_t n_in, const double* in, hipEvent_t e0) {
    launch_ev(k_spmv_tiled, (unsigned)T.grid, kTileThreads, 0, stream, e0, nullptr, n_out, n_in, T.tiles, T.view(), in, tpart.p);
}

// Tiled copy of a sparse matrix given by (ptr, idx, val) over n_out outputs and n_in inputs; outputs longer than
// skip_longer are left out (long rows have their own kernel).  Returns false when a (tile, block) segment does not fit
// the 16-bit offsets (then the CSR kernels serve this solve).
bool Engine::build_tiled(TiledBuf& T, int64_t n_out, int64_t n_in, const int64_t* ptr, const int32_t* idx, const double* val,
                         int64_t skip_longer) {
    T.tiles = ceil_div(n_out, kTileOut);
    T.nb_in = ceil_div(n_in, kTileIn);
    const size_t cells = (size_t)T.tiles * (size_t)T.nb_in;
    T.bptr.resize(cells * (kTileOut + 1), stream);
    T.segtot.resize(cells + 1, stream);
    T.segstart.resize(cells + 1, stream);
    T.idx.resize((size_t)NNZ + 1, stream);
    T.val.resize((size_t)NNZ + 1, stream);
    int32_t ovf = 0;
    const bool no_sorted = dev.tiled_general_build;             // (tests: the general kernels)
    // first the run-based kernels (entries of an output in ascending input order: what the LP's rows and the mirror's columns
    // are); an output that is not ascending makes them give up (bit 1) and the general kernels build the copy
    for (int pass = no_sorted ? 1 : 0; pass < 2; ++pass) {
        T.bptr.zero(stream);
        T.segtot.zero(stream);
        KTN_HIP(hipMemsetAsync(d_anynf.p + 1, 0, sizeof(int32_t), stream));
        if (pass == 0) {
            launch_n(k_tile_count_sorted, n_out, stream, n_out, ptr, idx, T.nb_in, skip_longer, T.bptr.p, d_anynf.p + 1);
        } else {
            T.cur.resize(cells * (kTileOut + 1), stream);
            T.cur.zero(stream);
            launch_n(k_tile_count, n_out, stream, n_out, ptr, idx, T.nb_in, skip_longer, T.bptr.p, d_anynf.p + 1);
        }
        launch(k_tile_scan, (unsigned)cells, kTileThreads, 0, stream, T.bptr.p, T.segtot.p, d_anynf.p + 1);
        check_launch();
        exclusive_scan(T.segtot.p, T.segstart.p, cells + 1);
        if (pass == 0) launch_n(k_tile_fill_sorted, n_out, stream, n_out, ptr, idx, val, T.nb_in, skip_longer, T.bptr.p, T.segstart.p, d_anynf.p + 1, T.idx.p, T.val.p);
        else launch_n(k_tile_fill, n_out, stream, n_out, ptr, idx, val, T.nb_in, skip_longer, T.bptr.p, T.cur.p, T.segstart.p, T.idx.p, T.val.p);
        check_launch();
        KTN_HIP(hipMemcpyAsync(&ovf, d_anynf.p + 1, 4, hipMemcpyDeviceToHost, stream));
        sync();
        if (pass == 0 && (ovf & 2)) { stats["lp_tiled_general_builds"] += 1.0; continue; }
        break;
    }
    // two 1024-thread workgroups per CU (80 KB of LDS each): a persistent grid over the (tile, block) units
    const int64_t U = T.tiles * T.nb_in;
    const int wg_per_cu = dev.tiled_wg;
    T.grid = std::max<int64_t>(std::min<int64_t>((int64_t)wg_per_cu * num_cus, U), 1);
    {
        std::vector<int32_t> pc((size_t)T.tiles);
        T.pieces = 1;
        for (int64_t tl = 0; tl < T.tiles; ++tl) {       // owner(u) = ((u + 1) G - 1) / U, as in the kernel
            const int64_t p0 = ((tl * T.nb_in + 1) * T.grid - 1) / U, p1 = (((tl + 1) * T.nb_in) * T.grid - 1) / U;
            pc[(size_t)tl] = (int32_t)(p1 - p0 + 1);
            T.pieces = std::max<int64_t>(T.pieces, p1 - p0 + 1);
        }
        T.pcnt.upload(pc, stream);
        sync();
    }
    return ovf == 0;
}

// Throughput mode: rows -> blocks (by the first column), block row lists in row order, local row positions of the CSC mirror.
void Engine::build_blocks() {
    const int nb = (int)n_blocks;
    d_blkrowptr.resize((size_t)nb + 1, stream);
    d_blkrows.resize((size_t)std::max<int64_t>(M, 1), stream);
    d_rowloc.resize((size_t)std::max<int64_t>(M, 1), stream);
    d_crowl.resize((size_t)NNZ + 1, stream);
    k_in.resize((size_t)std::max<int64_t>(M, 1), stream); k_out.resize((size_t)std::max<int64_t>(M, 1), stream);
    p_in.resize((size_t)std::max<int64_t>(M, 1), stream); p_out.resize((size_t)std::max<int64_t>(M, 1), stream);
    launch_n(k_row_block, M, stream, M, lp_rowptr.p, lp_col.p, d_blkcol.p, nb, k_in.p, p_in.p);
    int bits = 1;
    while ((1 << bits) < nb + 1 && bits < 30) ++bits;
    const size_t need = sort_pairs_temp_bytes((size_t)M);
    d_sorttmp.resize(need + 16, stream);
    KTN_HIP(sort_pairs_u64_u32(d_sorttmp.p, need, k_in.p, k_out.p, p_in.p, p_out.p, (size_t)M, 0, bits, stream));   // stable: rows ascending
    launch_n(k_block_rows, M, stream, M, k_out.p, p_out.p, nb, d_blkrowptr.p, d_blkrows.p, d_rowloc.p);
    launch_n(k_row_local, M, stream, M, k_out.p, p_out.p, d_blkrowptr.p, d_rowloc.p);
    launch_n(k_localize_rows, NNZ, stream, NNZ, c_row.p, d_rowloc.p, d_crowl.p);
    check_launch();
    std::vector<int32_t> rp = d_blkrowptr.to_host(stream);
    blk_mmax = 1;
    for (int b = 0; b < nb; ++b) blk_mmax = std::max(blk_mmax, rp[(size_t)b + 1] - rp[(size_t)b]);
    blocks_built_rows = M;
}

// One launch: every block's LP to the given tolerances.  Returns false when some block could not finish here (the caller
// then runs the ordinary loop).
bool Engine::lp_solve_blocks(double tol_p, double tol_g, double eta, LpResult* R, int64_t max_it) {
    const int nb = (int)n_blocks;
    const size_t lds = (size_t)(3 * blk_nmax + 3 * blk_mmax + (kBlkThreads / 64) * kBlkQ + kBlkQ + 8) * sizeof(double) +
                       (size_t)(blk_mmax + 2) * sizeof(int32_t);
    if (lds > 150 * 1024) return false;
    if (lds > lds_set_lp) {        // (per handle: handles live on different devices and host threads)
        KTN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pdhg_blocks), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        lds_set_lp = lds;
    }
    d_blkres.resize((size_t)nb * 8, stream);
    BlkLp P;
    P.blk_col = d_blkcol.p; P.blk_rowptr = d_blkrowptr.p; P.blk_rows = d_blkrows.p;
    P.rptr = lp_rowptr.p; P.rcol = lp_col.p; P.rval = r_sval.p;
    P.cptr = c_ptr.p; P.crowl = d_crowl.p; P.cval = c_sval.p;
    P.c = ch.p; P.l = lh.p; P.u = uh.p; P.lo = loh.p; P.hi = hih.p; P.dr = dr.p; P.dc = dc.p;
    P.x = xh.p; P.y = yh.p; P.xt = xth.p; P.yt = yth.p; P.omega = d_blkomega.p; P.res = d_blkres.p;
    P.tol_p = tol_p; P.tol_g = tol_g; P.eta0 = eta; P.eta_safe = 0.998; P.stag_factor = prm.lp_stag_factor;
    P.stall_accept = (tol_p > prm.lp_tol_floor * prm.f_tol * (1.0 + 1e-9)) ? 10.0 : 3.0;
    P.check_every = std::max(2, prm.lp_check_every); P.first_chunk = 31; P.near_chunk = prm.lp_near_check;
    P.max_iter = (int)std::min<int64_t>(max_it, 2000000000);
    P.nmax = blk_nmax; P.mmax = blk_mmax;
    launch(k_pdhg_blocks, (unsigned)nb, kBlkThreads, lds, stream, P);
    check_launch();
    std::vector<double> res = d_blkres.to_host(stream);
    bool all_ok = true;
    double pobj = 0.0, dobj = 0.0, pviol = 0.0, gap = 0.0, it_max = 0.0, it_sum = 0.0;
    for (int b = 0; b < nb; ++b) {
        const double* o = res.data() + (size_t)b * 8;
        if ((int)o[0] != KTN_STATUS_OPTIMAL) all_ok = false;
        pobj += o[2]; dobj += o[3]; pviol = std::max(pviol, o[4]); gap = std::max(gap, o[5]);
        it_max = std::max(it_max, o[1]); it_sum += o[1];
    }
    stats["blk_lp_launches"] += 1.0;
    stats["blk_pdhg_iters_sum"] += it_sum;
    stats["blk_pdhg_iters_max"] += it_max;
    if (!all_ok) { stats["blk_lp_fallbacks"] += 1.0; return false; }
    R->status = KTN_STATUS_OPTIMAL; R->iters = (int64_t)it_max; R->pobj = pobj; R->dobj = dobj; R->row_viol = pviol; R->gap = gap;
    return true;
}

// y-step over all rows: G lanes per row for ordinary rows, a workgroup per row for the long ones.  Step sizes and the
// Halpern weight travel as kernel arguments (eager launches: at ~6 us per kernel the host stays ahead of the GPU, and a
// hipGraph of the chunk bought nothing measurable while its capture + instantiation cost every LP solve).
void Engine::launch_y(const SpMat& A, double sigma, double w, double rho, hipEvent_t e0, hipEvent_t e1) {
    const int64_t m = M;
    if (m == 0) return;                                 // (first LP of a model with NL rows only: no dual step, no zero-size grid)
    const int64_t thr = n_long > 0 ? kLongRow : (int64_t)1 << 62;
    if (tiled_on && m > 0) {
        launch_tiled(tA, m, n_lp, xbar.p, e0);
        launch_ev(k_y_epilogue, grid_n(m), kBlock, 0, stream, nullptr, e1, m, tA.pcnt.p, tpart.p, (n_long > 0 ? A.ptr : (const int64_t*)nullptr), thr, yh.p,
                  y0h.p, loh.p, hih.p, sigma, w, rho);
    } else if (packed_on) {
        // T rows per lane group; T = 1 is one launch for all rows: the regular lane groups plus one trailing workgroup per long row
        const int thr32 = n_long > 0 ? (int)kLongRow : 0x7fffffff;
        const bool with_long = packed_trips != 2 && packed_trips != 4;
        with_value<2, 4, 1>(packed_trips, [&](auto t) {
            with_group(grp_rows, [&](auto g) {
                constexpr int G = g(), T = t();
                launch_ev(k_pdhg_y_packed<G, T>, T == 1 ? group_grid_long(m, G, n_long) : group_grid(m, G, T), kBlock, 0, stream, e0, e1, m, A.idx, A.val,
                          xbar.p, yh.p, d_rrec.p, sigma, w, rho, thr32, T == 1 ? (const int32_t*)d_longrows.p : nullptr, T == 1 ? (int)n_long : 0);
            });
        });
        if (with_long) return;
    } else {
        with_group(grp_rows, [&](auto g) {
            launch_timed(k_pdhg_y<g()>, group_grid(m, g()), kBlock, 0, stream, e0, e1, m, A, xbar.p, yh.p, y0h.p, loh.p, hih.p, sigma, w, rho, thr);
        });
    }
    if (n_long > 0)
        launch(k_pdhg_y_long<false>, (unsigned)n_long, kLongBlock, 0, stream, d_longrows.p, A, xbar.p, (const double*)nullptr, yh.p, y0h.p, yth.p, loh.p, hih.p,
               dr.p, sigma, w, rho, (double*)nullptr);
}

void Engine::launch_x(const SpMat& AT, double tau, double w, double rho, bool update, hipEvent_t e0, hipEvent_t e1) {
    const int64_t n = n_lp;
    if (row_sharded()) {
        // local partial of A'y, summed over the ranks, then the element-wise primal step on the replicated x
        // (peer-buffer transport: the partial is written straight into the exposed slot, and the primal step adds up the
        //  ranks' slots itself -- spmv, one single-workgroup barrier kernel, prox: no reduction pass, no copy)
        const bool ipc = dist.ipc.on && n <= dist.ipc.cap;
        double* part = ipc ? ipc_slot() : pv.p;
        if (M == 0) launch_n(k_fill, n, stream, n, part, 0.0);
        if (tiled_on && M > 0) {                          // this rank's block is large: its partial A_r'y_r from the tiled copy
            launch_tiled(tAT, n, M, yh.p, e0);
            launch_ev(k_tile_vec, grid_n(n), kBlock, 0, stream, nullptr, e1, n, tAT.pcnt.p, tpart.p, part);
        }
        else spmv_cols(AT, yh.p, part, e0, e1);
        if (ipc) {
            stats["allreduce_calls"] += 1.0;
            stats["allreduce_bytes"] += 8.0 * (double)n;
            const int64_t off = ipc_barrier();
            with_bool(update, [&](auto u) {
                launch_n(k_x_prox_ipc<u()>, n, stream, n, dist.ipc.P, dist.world, off, xh.p, x0h.p, xth.p, xbar.p, ch.p, lh.p, uh.p, tau, w, rho);
            });
            return;
        }
        allreduce(pv.p, (size_t)n, 0);
        with_bool(update, [&](auto u) { launch_n(k_x_prox<u()>, n, stream, n, pv.p, xh.p, x0h.p, xth.p, xbar.p, ch.p, lh.p, uh.p, tau, w, rho); });
        return;
    }
    if (n_longc > 0 && !(tiled_on && M > 0)) {
        // long columns: lane groups for the ordinary columns, a workgroup per long one -- the primal step fused into both
        // (timed as a pair: the first kernel's start, the second one's stop)
        with_bool(update, [&](auto u) {
            constexpr bool U = u();
            with_group(grp_cols, [&](auto g) {
                launch_timed(k_pdhg_x_skip<g(), U>, group_grid(n, g()), kBlock, 0, stream, e0, nullptr, n, AT, yh.p, xh.p, x0h.p, xth.p, xbar.p, ch.p,
                             lh.p, uh.p, tau, w, rho, kLongRow);
            });
            launch_timed(k_pdhg_x_long<U>, (unsigned)n_longc, 1024, 0, stream, nullptr, e1, d_longcols.p, AT, yh.p, xh.p, x0h.p, xth.p, xbar.p, ch.p,
                         lh.p, uh.p, tau, w, rho);
        });
        return;
    }
    if (update && tiled_on && M > 0) {
        launch_tiled(tAT, n, M, yh.p, e0);
        launch_ev(k_x_epilogue, grid_n(n), kBlock, 0, stream, nullptr, e1, n, tAT.pcnt.p, tpart.p, xh.p, x0h.p, xbar.p, ch.p, lh.p, uh.p, tau, w, rho);
    } else if (update && packed_on) {
        with_value<2, 4, 1>(packed_trips, [&](auto t) {
            with_group(grp_cols, [&](auto g) {
                constexpr int G = g(), T = t();
                launch_ev(k_pdhg_x_packed<G, T>, group_grid(n, G, T), kBlock, 0, stream, e0, e1, n, d_cbl.p, AT.idx, AT.val, yh.p, xh.p, xbar.p, d_crec.p, tau, w, rho);
            });
        });
    } else {
        // plain CSC; without update (the check) xbar is not written and the launch is never timed
        with_bool(update, [&](auto u) {
            constexpr bool U = u();
            with_group(grp_cols, [&](auto g) {
                launch_timed(k_pdhg_x<g(), U>, group_grid(n, g()), kBlock, 0, stream, U ? e0 : nullptr, U ? e1 : nullptr, n, AT, yh.p, xh.p, x0h.p, xth.p,
                             U ? xbar.p : nullptr, ch.p, lh.p, uh.p, tau, w, rho);
            });
        });
    }
}

// One plain (update) iteration: the x-step, then the y-step.  profile: each step's kernels carry their own start / stop events
// (bytes moved per step: DESIGN.md section 4).
void Engine::pdhg_iteration(const SpMat& A, const SpMat& AT, double tau, double sigma, double w, double rho) {
    if (!prm.profile) {
        launch_x(AT, tau, w, rho, true, nullptr, nullptr);
        launch_y(A, sigma, w, rho, nullptr, nullptr);
        return;
    }
    const int64_t n = n_lp, m = M;
    const size_t e0 = ev_get(), e1 = ev_get(), e2 = ev_get(), e3 = ev_get();
    launch_x(AT, tau, w, rho, true, ev_pool[e0], ev_pool[e1]);
    launch_y(A, sigma, w, rho, ev_pool[e2], ev_pool[e3]);
    ev_recs.push_back({0, e0, e1, (double)NNZ * 12 + 8.0 * (n + 1) + 8.0 * 7 * n + 8.0 * m});
    if (m > 0) ev_recs.push_back({1, e2, e3, (double)NNZ * 12 + 8.0 * (m + 1) + 8.0 * 5 * m + 8.0 * n});
}

// Check iteration: the PDHG step without update (xt, yt stored) and the KKT / fixed-point sums.  The row side rides on the
// y-step (k_pdhg_y_chk gathers xt and x anyway); the column side needs A'yt and is one G-lanes-per-column pass.
bool Engine::launch_check(const SpMat& A, const SpMat& AT, double tau, double sigma, double w_next, double rho) {
    const int64_t n = n_lp, m = M;
    const int64_t thr = n_long > 0 ? kLongRow : (int64_t)1 << 62;
    const int64_t brow = group_grid(std::max<int64_t>(m, 1), grp_rows), bcol = group_grid(n, grp_cols);
    chk_part.resize((size_t)(brow + n_long + bcol) * kChkQ, stream);
    double* prow = chk_part.p;
    double* pcol = chk_part.p + (size_t)(brow + n_long) * kChkQ;
    const bool tiled_chk_off = dev.no_tiled_check;
    if (tiled_on && m > 0 && !tiled_chk_off) {
        // the four SpMV passes of a check through the tiled copy (kernels.hpp "check iteration on the tiled copy"); row-sharded:
        // the two column-side vectors are this rank's partials and are summed over the ranks -- the same sequence of
        // collectives as the CSR form below, so ranks may differ in which form they run
        const int64_t brow_t = grid_n(m), bcol_t = grid_n(n);      // <= brow, bcol
        launch_tiled(tAT, n, m, yh.p, nullptr);
        if (row_sharded()) {
            launch_n(k_tile_vec, n, stream, n, tAT.pcnt.p, tpart.p, pv.p);
            allreduce(pv.p, (size_t)n, 0);
            launch_n(k_x_prox<false>, n, stream, n, pv.p, xh.p, x0h.p, xth.p, xbar.p, ch.p, lh.p, uh.p, tau, 0.0, 1.0);
        } else {
            launch_n(k_x_epilogue_chk, n, stream, n, tAT.pcnt.p, tpart.p, xh.p, xth.p, ch.p, lh.p, uh.p, tau);
        }
        launch_tiled(tA, m, n, xth.p, nullptr);
        launch_n(k_tile_vec, m, stream, m, tA.pcnt.p, tpart.p, pw.p);
        launch_tiled(tA, m, n, xh.p, nullptr);
        launch_n(k_y_epilogue_chk, m, stream, m, tA.pcnt.p, tpart.p, pw.p, (n_long > 0 ? A.ptr : (const int64_t*)nullptr), thr, yh.p, y0h.p, yth.p, loh.p,
                 hih.p, dr.p, sigma, prow);
        if (n_long > 0)
            launch(k_pdhg_y_long<true>, (unsigned)n_long, kLongBlock, 0, stream, d_longrows.p, A, xth.p, xh.p, yh.p, y0h.p, yth.p, loh.p, hih.p, dr.p, sigma,
                   0.0, 1.0, prow + (size_t)brow_t * kChkQ);
        chk_nrow = (int)(brow_t + n_long);
        launch_tiled(tAT, n, m, yth.p, nullptr);
        launch_n(k_tile_vec, n, stream, n, tAT.pcnt.p, tpart.p, pv.p);
        if (row_sharded()) allreduce(pv.p, (size_t)n, 0);
        launch_n(k_chk_cols_vec, n, stream, n, pv.p, xh.p, xth.p, x0h.p, ch.p, lh.p, uh.p, dc.p, pcol);
        chk_ncol = (int)bcol_t;
        launch(k_chk_final, 2 * kChkQ, kRedBlocks, 0, stream, prow, chk_nrow, pcol, chk_ncol, chk_target());
        if (row_sharded()) {                            // row sums: every rank's rows; column sums are identical already
            allreduce(chkout.p, 12, 0);
            allreduce(chkout.p + 12, 4, 1);
        }
        return false;
    }
    // the plain CSR form on one GPU: the two step kernels of the check also leave the Halpern update in xnext / ynext
    const bool spec = w_next >= 0.0 && m > 0 && !row_sharded() && n_long == 0 && n_longc == 0;
    if (spec) {
        xnext.resize((size_t)n, stream); ynext.resize((size_t)m, stream);
        with_group(grp_cols, [&](auto g) {
            launch(k_pdhg_x<g(), false>, group_grid(n, g()), kBlock, 0, stream, n, AT, yh.p, xh.p, x0h.p, xth.p, xnext.p, ch.p, lh.p, uh.p, tau, w_next, rho);
        });
    } else {
        launch_x(AT, tau, 0.0, 1.0, false, nullptr, nullptr);
    }
    if (m > 0) {
        with_group(grp_rows, [&](auto g) {
            launch(k_pdhg_y_chk<g()>, group_grid(m, g()), kBlock, 0, stream, m, A, xth.p, xh.p, yh.p, y0h.p, yth.p, loh.p, hih.p, dr.p, sigma, thr, prow,
                   spec ? ynext.p : (double*)nullptr, w_next, rho);
        });
        if (n_long > 0)
            launch(k_pdhg_y_long<true>, (unsigned)n_long, kLongBlock, 0, stream, d_longrows.p, A, xth.p, xh.p, yh.p, y0h.p, yth.p, loh.p, hih.p, dr.p, sigma,
                   0.0, 1.0, prow + (size_t)brow * kChkQ);
    }
    chk_nrow = (m > 0) ? (int)(brow + n_long) : 0;
    if (row_sharded() || n_longc > 0) {
        if (m == 0) launch_n(k_fill, n, stream, n, pv.p, 0.0);
        spmv_cols(AT, yth.p, pv.p);
        allreduce(pv.p, (size_t)n, 0);
        chk_ncol = (int)grid_n(n);               // <= bcol: the column partials fit the same region
        launch_n(k_chk_cols_vec, n, stream, n, pv.p, xh.p, xth.p, x0h.p, ch.p, lh.p, uh.p, dc.p, pcol);
    } else {
        with_group(grp_cols, [&](auto g) {
            launch(k_chk_cols<g()>, group_grid(n, g()), kBlock, 0, stream, n, AT, xh.p, xth.p, x0h.p, yth.p, ch.p, lh.p, uh.p, dc.p, pcol);
        });
        chk_ncol = (int)bcol;
    }
    launch(k_chk_final, 2 * kChkQ, kRedBlocks, 0, stream, prow, chk_nrow, pcol, chk_ncol, chk_target());   // (rows | columns) x quantity
    if (row_sharded()) {                            // row sums: every rank's rows; column sums are identical already
        allreduce(chkout.p, 12, 0);
        allreduce(chkout.p + 12, 4, 1);
    }
    return spec;
}

// LP dispatch.  The first-order method is the default: on the large sparse LPs of the hot path it is the only
// option, and on small ones its solutions sit in the middle of the optimal face, which Kelley's method likes
// (test/misc.jl 501: tens of iterations instead of thousands from simplex vertices).  Where it STALLS -- several
// nearly parallel cuts active at a curved optimum, DESIGN.md section 5 -- and the LP has at most kDenseMaxN
// columns, the exact kernel finishes the solve; each stall doubles the number of following solves that go to
// the exact kernel directly.
LpResult Engine::lp_solve(double tol_p, double tol_g, int mode, bool identity_scaling) {
    md_y_version = 0;                                    // (set again by an exact mid-size solve that ends optimal)
    ++kkt_solves; kkt_solved = mode == 0; kkt_arena = false;      // (KKT report: lp_y is this solve's from here on)
    const bool dense_ok = mode == 0 && !identity_scaling && !row_sharded() && prm.lp_dense_after != 0 && n_lp >= 1 && n_lp <= kDenseMaxN &&
                          M * n_lp <= 8000000;
    // ... and LPs of 33 .. lp_mid_max_var columns by the exact mid-size solver (mid_lp.hpp), under the same hand-over rule
    const bool mid_ok = mode == 0 && !identity_scaling && !row_sharded() && prm.lp_dense_after != 0 && n_lp > kDenseMaxN &&
                        n_lp <= std::min<int64_t>(prm.lp_mid_max_var, kMidMaxN) && n_blocks == 0 && M < ((int64_t)1 << 29);
    if (mid_ok && mid_backoff > 0) {
        --mid_backoff;                                   // (a recent exact solve failed: cold starts cost ~n pivots each, do not repeat them at once)
    } else if (mid_ok) {
        auto failed = [&]() {
            stats["mid_lp_fallbacks"] += 1.0;
            mid_credit = 0;
            mid_backoff_len = std::min<int64_t>(2 * std::max<int64_t>(mid_backoff_len, 4), 256);
            mid_backoff = mid_backoff_len;
        };
        if (prm.lp_dense_after < 0 || mid_credit > 0) {
            if (mid_credit > 0) --mid_credit;
            LpResult R;
            if (lp_solve_mid(&R)) return R;
            failed();
            return lp_solve_core(tol_p, tol_g, mode, identity_scaling);
        }
        lp_iter_budget = prm.lp_dense_after;
        LpResult R = lp_solve_core(tol_p, tol_g, mode, identity_scaling);
        lp_iter_budget = 0;
        if (R.status != KTN_STATUS_USERLIMIT) return R;
        stats["lp_stalls"] += 1.0;
        LpResult D;
        if (lp_solve_mid(&D)) {
            mid_run = std::min<int64_t>(2 * std::max<int64_t>(mid_run, 1), 1 << 20);
            mid_credit = mid_run;
            mid_backoff_len = 0;
            return D;
        }
        failed();
        return lp_solve_core(tol_p, tol_g, mode, identity_scaling);
    }
    if (!dense_ok) return lp_solve_core(tol_p, tol_g, mode, identity_scaling);
    // (KTN_CUT_SUPPORTING_QUAD with an interior point: every LP the exact kernel can take goes to it.  A supporting cut taken on the
    //  segment to a loosely solved LP point lands next to the previous one, where Kelley's cut at that point would still be a new
    //  tangent: measured on the ellipsoid of DESIGN.md section 11, 100 / 231 rounds at n = 4 / 8 with the tolerance schedule against
    //  49 / 162 from vertices)
    const bool esh_vertices = esh_quad_mode() && xint_found != 0;
    if (prm.lp_dense_after < 0 || esh_vertices || dense_credit > 0) {
        if (dense_credit > 0 && !esh_vertices) --dense_credit;
        LpResult R;
        if (lp_solve_dense(&R)) return R;
        stats["dense_lp_fallbacks"] += 1.0;
        return lp_solve_core(tol_p, tol_g, mode, identity_scaling);
    }
    lp_iter_budget = prm.lp_dense_after;
    LpResult R = lp_solve_core(tol_p, tol_g, mode, identity_scaling);
    lp_iter_budget = 0;
    if (R.status != KTN_STATUS_USERLIMIT) return R;
    stats["lp_stalls"] += 1.0;
    LpResult D;
    if (lp_solve_dense(&D)) {
        dense_run = std::min<int64_t>(2 * std::max<int64_t>(dense_run, 1), 1 << 20);
        dense_credit = dense_run;
        return D;
    }
    stats["dense_lp_fallbacks"] += 1.0;
    return lp_solve_core(tol_p, tol_g, mode, identity_scaling);
}

// Exact solve of a small LP by the dual active-set kernel (dense_lp.hpp).  Returns false when the kernel
// gives up (singular working set, pivot limit, an artificial side that still carries a multiplier with no real side to stop
// at -- the LP is unbounded along it; an artificial side left with a ZERO multiplier, i.e. an optimal face unbounded in a
// zero-cost direction, is no failure --, or an optimum that breaks a finite bound beyond kDenseBig): the caller then runs
// the first-order method.
bool Engine::lp_solve_dense(LpResult* R) {
    auto t0 = std::chrono::steady_clock::now();
    const int n = (int)n_lp;
    const int64_t m = M;
    ds_dense.resize((size_t)std::max<int64_t>(m, 1) * n, stream);
    ds_out.resize(4, stream);
    if (ds_W.n != (size_t)n) {
        ds_W.resize(n, stream);
        ds_valid.resize(1, stream);
        ds_valid.zero(stream);
    }
    lp_y.resize((size_t)std::max<int64_t>(m, 1), stream);
    lp_y.n = (size_t)m;
    DenseLpIO P;
    P.n = n; P.m = m; P.rowptr = lp_rowptr.p; P.col = lp_col.p; P.val = lp_val.p; P.lo = lp_lo.p; P.hi = lp_hi.p;
    P.l = lp_l.p; P.u = lp_u.p; P.c = lp_c.p; P.sgn = (sense == KTN_MAX) ? -1.0 : 1.0;
    P.dense = ds_dense.p; P.W = ds_W.p; P.Wvalid = ds_valid.p; P.x = lp_x.p; P.y = lp_y.p; P.out = ds_out.p;
    P.max_pivots = 200 + 20 * n + (int)std::min<int64_t>(m, 100000);
    P.tol = 1e-9;
    launch(k_dense_lp, 1, 256, 0, stream, P);
    check_launch();
    double out[4];
    KTN_HIP(hipMemcpyAsync(out, ds_out.p, sizeof(out), hipMemcpyDeviceToHost, stream));
    sync();
    stats["dense_lp_solves"] += 1.0;
    stats["dense_lp_pivots"] += out[1];
    stats["lp_solves"] += 1.0;
    stats["lp_time_s"] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const int st = (int)out[0];
    if (st == 0 && !big_bounds_hold()) {                 // optimal for the LP without its bounds beyond kDenseBig only
        ds_valid.zero(stream);
        return false;
    }
    if (st == 0) {
        R->status = KTN_STATUS_OPTIMAL;
        R->iters = (int64_t)out[1];
        R->pobj = R->dobj = out[2];
        R->row_viol = 0.0; R->gap = 0.0;
        R->exact = true;
        objval = P.sgn * out[2] + c0;
        return true;
    }
    if (st == 1) {
        R->status = KTN_STATUS_INFEASIBLE;
        R->iters = (int64_t)out[1];
        return true;
    }
    return false;
}

// The finite variable bounds beyond kDenseBig, which the exact solvers treat as absent (dense_lp.hpp), at the point in lp_x.
bool Engine::big_bounds_hold() {
    if (!has_big_bound) return true;
    int32_t bad = 0;
    KTN_HIP(hipMemsetAsync(d_anynf.p + 3, 0, sizeof(int32_t), stream));
    launch(k_big_bounds_check, (unsigned)ceil_div(n_lp, 256), 256, 0, stream, (int)n_lp, lp_x.p, lp_l.p, lp_u.p, d_anynf.p + 3);
    check_launch();
    KTN_HIP(hipMemcpyAsync(&bad, d_anynf.p + 3, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    sync();
    if (bad) stats["lp_big_bound_rejects"] += 1.0;
    return bad == 0;
}

// the solver's view of the LP and of its own persistent state
static MidLpIO mid_io(Engine* e) {
    MidLpIO P;
    P.n = (int)e->n_lp; P.m = e->M; P.rowptr = e->lp_rowptr.p; P.col = e->lp_col.p; P.val = e->lp_val.p; P.lo = e->lp_lo.p; P.hi = e->lp_hi.p;
    P.l = e->lp_l.p; P.u = e->lp_u.p; P.c = e->lp_c.p; P.sgn = (e->sense == KTN_MAX) ? -1.0 : 1.0;
    P.Binv = e->md_Binv.p; P.W = e->md_W.p; P.hW = e->md_hW.p; P.x = e->md_x.p; P.lam = e->md_lam.p; P.uvec = e->md_u.p; P.dvec = e->md_d.p; P.rvec = e->md_r.p;
    P.part_val = e->md_pv.p; P.part_idx = e->md_pi.p; P.st = e->md_st.p; P.ctil = e->md_c.p;
    P.tol = 1e-9; P.max_pivots = 0;
    return P;
}

// ktn_lp_get_duals after an exact mid-size solve whose rows and working set still stand: the multipliers of the LP's own cost
// (mid_lp.hpp k_mid_true_duals), not those of the perturbed cost that lp_y holds for the loop.  false: nothing to add to lp_y.
bool Engine::mid_true_duals(double* y_out) {
    if (!md_valid || md_y_version == 0 || md_y_version != lp_version || md_W.n != (size_t)n_lp) return false;
    MidLpIO P = mid_io(this);
    const size_t mm = (size_t)std::max<int64_t>(M, 1);
    md_y.resize(mm, stream);
    KTN_HIP(hipMemsetAsync(md_y.p, 0, mm * sizeof(double), stream));
    const unsigned g_n = (unsigned)ceil_div(P.n, 256);
    launch(k_mid_lambda, g_n, 256, 0, stream, P, 1);
    launch(k_mid_true_duals, g_n, 256, 0, stream, P, md_y.p);
    check_launch();
    if (y_out) md_y.download(y_out, (size_t)M, stream);      // (null: the caller reads md_y on the device)
    return true;
}

// Exact solve of a mid-size LP (mid_lp.hpp): batches of pivots enqueued without a host synchronisation, the device-resident
// state read back once per batch.  Returns false when the solver gives up (an artificial side of a free variable is still
// needed, pivot limit, a basis inverse that a cold restart does not repair): the caller then runs the first-order method.
bool Engine::lp_solve_mid(LpResult* R) {
    auto t0 = std::chrono::steady_clock::now();
    const int n = (int)n_lp;
    const int64_t m = M;
    if (md_W.n != (size_t)n) {
        md_Binv.resize((size_t)n * n, stream);
        md_W.resize(n, stream); md_hW.resize(n, stream); md_x.resize(n, stream); md_lam.resize(n, stream);
        md_u.resize(n, stream); md_d.resize(n, stream); md_r.resize(n, stream); md_c.resize(n, stream);
        md_pv.resize(kMidPriceBlocks, stream); md_pi.resize(kMidPriceBlocks, stream); md_st.resize(1, stream); md_lost.resize(1, stream);
        md_valid = false;
    }
    lp_y.resize((size_t)std::max<int64_t>(m, 1), stream);
    lp_y.n = (size_t)m;
    MidLpIO P = mid_io(this);
    P.tol = 1e-9;
    // (a cold start from the bound vertex of a cutting-plane LP that the first-order method has already grown to a few thousand
    //  rows takes tens of pivots per column -- every variable leaves its box corner, many of them more than once; the warm
    //  re-solves that follow take tens to hundreds in total)
    P.max_pivots = 5000 + 200 * n + (int)std::min<int64_t>(20 * m, 4000000);
    const unsigned g_nn = (unsigned)ceil_div((int64_t)n * n, 256), g_n = (unsigned)ceil_div(n, 256);
    auto refine = [&]() {                               // x = B^-1 h_W + one step of iterative refinement; lambda = -B^-T c
        launch(k_mid_resid, g_n, 256, 0, stream, P, 0);
        launch(k_mid_apply, (unsigned)ceil_div(n, 4), 256, 0, stream, P, 0);
        launch(k_mid_resid, g_n, 256, 0, stream, P, 1);
        launch(k_mid_apply, (unsigned)ceil_div(n, 4), 256, 0, stream, P, 1);
        launch(k_mid_resid, g_n, 256, 0, stream, P, 1);
        launch(k_mid_resid_norm, 1, 256, 0, stream, P, 1);
        launch(k_mid_lambda, g_n, 256, 0, stream, P, 0);
    };
    // B^-1 afresh from the working set (mid_lp.hpp "refactorisation"), then x and lambda from their definitions
    auto refactor = [&]() {
        md_aug.resize((size_t)n * 2 * n, stream); md_prow.resize((size_t)2 * n, stream); md_fcol.resize((size_t)n, stream);
        launch(k_mid_gj_build, (unsigned)n, 256, 0, stream, P, md_aug.p);
        const unsigned g_2n = (unsigned)ceil_div(2 * n, 256), g_aug = (unsigned)ceil_div((int64_t)n * 2 * n, 256);
        for (int col = 0; col < n; ++col) {
            launch(k_mid_gj_pivot, 1, 256, 0, stream, P, (const double*)md_aug.p, col);
            launch(k_mid_gj_swap, g_2n, 256, 0, stream, P, md_aug.p, col, md_prow.p);
            launch(k_mid_gj_col, g_n, 256, 0, stream, P, (const double*)md_aug.p, col, md_fcol.p);
            launch(k_mid_gj_elim, g_aug, 256, 0, stream, P, md_aug.p, col, (const double*)md_prow.p, (const double*)md_fcol.p);
        }
        launch(k_mid_gj_store, g_nn, 256, 0, stream, P, (const double*)md_aug.p);
        refine();
        md_since_refactor = 0;
        stats["mid_lp_refactors"] += 1.0;
    };
    const int64_t refactor_every = dev.mid_refactor > 0 ? dev.mid_refactor : kMidRefactor;      // (KTN_MID_REFACTOR: tests reach the refactorisation on small LPs)
    MidState hs;
    int total_pivots = 0, status = 4;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (!md_valid) {
            launch(k_mid_init, g_nn, 256, 0, stream, P);
            stats["mid_lp_cold_starts"] += 1.0;
            md_since_refactor = 0;
        } else {
            launch(k_mid_rearm, 1, 1, 0, stream, md_st.p);
            if (md_since_refactor >= refactor_every) refactor();
        }
        int refined_at = -1, refinements = 0, pivots_seen = 0;
        bool bad_inverse = false;
        status = 4;
        for (;;) {
            for (int b = 0; b < 8; ++b) {
                launch(k_mid_price, kMidPriceBlocks, 256, 0, stream, P);
                launch(k_mid_select, 1, 256, 0, stream, P);
                launch(k_mid_u, g_n, 256, 0, stream, P);
                launch(k_mid_ratio, 1, 256, 0, stream, P);
                launch(k_mid_rank1, g_nn, 256, 0, stream, P);
            }
            check_launch();
            KTN_HIP(hipMemcpyAsync(&hs, md_st.p, sizeof(hs), hipMemcpyDeviceToHost, stream));
            sync();
            md_since_refactor += hs.pivots - pivots_seen;
            pivots_seen = hs.pivots;
            if (hs.gj_singular) { bad_inverse = true; break; }            // the working set itself is (numerically) dependent: cold start
            if (hs.status == 0) {
                if (md_since_refactor >= refactor_every) refactor();
                continue;
            }
            if (hs.status == 1) {
                if (refined_at == hs.pivots) {          // the confirming price after the refinement found nothing either
                    if (!(hs.resid <= 1e-7 * hs.scale)) { bad_inverse = true; break; }
                    status = 0;
                    break;
                }
                if (++refinements > 50) break;
                refine();
                refined_at = hs.pivots;
                continue;
            }
            status = hs.status;                          // 3 infeasible, 4 failed
            break;
        }
        total_pivots += hs.pivots;
        if (status == 0 || status == 3) break;
        md_valid = false;                                // failed on a warm start (or a decayed inverse): once more from the bound vertex
        if (!bad_inverse && attempt == 0 && hs.pivots >= P.max_pivots) break;      // (a pivot limit is not repaired by a restart)
    }
    stats["mid_lp_solves"] += 1.0;
    stats["mid_lp_pivots"] += (double)total_pivots;
    stats["lp_solves"] += 1.0;
    bool ok = false;
    if (status == 0) {
        KTN_HIP(hipMemsetAsync(lp_y.p, 0, (size_t)std::max<int64_t>(m, 1) * sizeof(double), stream));
        launch(k_mid_final, 1, 256, 0, stream, P, lp_y.p);
        KTN_HIP(hipMemcpyAsync(lp_x.p, md_x.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));
        KTN_HIP(hipMemcpyAsync(&hs, md_st.p, sizeof(hs), hipMemcpyDeviceToHost, stream));
        check_launch();
        sync();
        stats["mid_lp_dup_sides"] += (double)hs.dup_sides;      // positions of the working set that repeated a side (k_mid_final sums them)
        if (hs.art_left == 0 && big_bounds_hold()) {
            R->status = KTN_STATUS_OPTIMAL;
            R->iters = total_pivots;
            R->pobj = R->dobj = hs.obj;
            R->row_viol = 0.0; R->gap = 0.0;
            R->exact = true;
            objval = P.sgn * hs.obj + c0;
            md_valid = true;
            md_y_version = lp_version;
            ok = true;
        } else {
            md_valid = false;
        }
    } else if (status == 3) {
        R->status = KTN_STATUS_INFEASIBLE;
        R->iters = total_pivots;
        md_valid = false;
        ok = true;
    }
    stats["lp_time_s"] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return ok;
}

// ---- pieces of a first-order solve that lp_solve_core and the scripted test hook (lp_script) share ----
// lanes per row / column: by the average length, then the development overrides
void Engine::lp_pick_groups() {
    const int64_t n = n_lp, m = M;
    const double avg_r = m ? (double)NNZ / (double)m : 1.0, avg_c = n ? (double)NNZ / (double)n : 1.0;
    grp_rows = pick_group(avg_r);
    grp_cols = pick_group(avg_c);
    if (dev.grp_rows > 0) grp_rows = dev.grp_rows;
    if (dev.grp_cols > 0) grp_cols = dev.grp_cols;
}

// LPs beyond the caches: tiled copies of A^ and A^' (kernels.hpp "tiled SpMV") serve the plain steps and the check
// iterations; the power iteration keeps the CSR / CSC kernels
void Engine::lp_choose_tiled(bool same_matrix) {
    {
        const bool tenv = dev.tiled >= 0;
        // ... and dense enough: every (tile, block) unit stages a 64 KB block of the input vector, so a matrix with few entries
        // per unit pays more for the staging than for its entries (n = 1e6, 5.8e6 entries: 350 per unit, 1.31 s tiled against
        // 0.49 s with the CSR kernels; cfg4: 9 500 per unit)
        const int64_t units_t = ceil_div(M, (int64_t)kTileOut) * ceil_div(n_lp, (int64_t)kTileIn);
        const int64_t units_tt = ceil_div(n_lp, (int64_t)kTileOut) * ceil_div(M, (int64_t)kTileIn);
        tiled_on = prm.lp_tiled_nnz > 0 && NNZ >= prm.lp_tiled_nnz && n_lp >= 2 * kTileIn && M >= 2 * kTileIn &&
                   NNZ >= 4096 * std::max(units_t, units_tt);
        if (tenv) tiled_on = dev.tiled != 0 && M > 0 && NNZ > 0;
        if (same_matrix) tiled_on = tiled_built;            // the copies of the previous solve (or their absence) still fit
        else if (tiled_on) {
            auto tt = std::chrono::steady_clock::now();
            tiled_on = build_tiled(tA, M, n_lp, lp_rowptr.p, lp_col.p, r_sval.p, kLongRow) &&
                       build_tiled(tAT, n_lp, M, c_ptr.p, c_row.p, c_sval.p, (int64_t)1 << 62);
            tpart.resize((size_t)std::max<int64_t>(tA.pieces * M, tAT.pieces * n_lp), stream);
            stats["lp_tiled_builds"] += 1.0;
            stats["lp_tiled_build_time_s"] += std::chrono::duration<double>(std::chrono::steady_clock::now() - tt).count();
            if (!tiled_on) stats["lp_tiled_overflows"] += 1.0;
        }
        tiled_built = tiled_on;
    }
}

// the scaled problem vectors and the PDHG iterates (xbar, pv, pw: work vectors of the steps and of the power iteration)
void Engine::lp_resize_iterates() {
    const size_t n = (size_t)n_lp, mm = (size_t)std::max<int64_t>(M, 1);
    ch.resize(n, stream); lh.resize(n, stream); uh.resize(n, stream); xh.resize(n, stream);
    x0h.resize(n, stream); xth.resize(n, stream); xbar.resize(n, stream); pv.resize(n, stream);
    loh.resize(mm, stream); hih.resize(mm, stream); yh.resize(mm, stream); y0h.resize(mm, stream);
    yth.resize(mm, stream); pw.resize(mm, stream);
}

// anchors z0 = z; with the packed records of the plain steps when asked for (not for the tiled / row-sharded forms, whose
// steps are split into SpMV + element-wise kernels)
void Engine::lp_set_anchors(bool want_packed) {
    const int64_t n = n_lp, m = M;
    const size_t mm = (size_t)std::max<int64_t>(m, 1);
    packed_on = want_packed && !tiled_on && !row_sharded() && NNZ < ((int64_t)1 << 31) && !dev.no_packed;
    if (dev.packed_trips > 0) packed_trips = dev.packed_trips;
    if (packed_on) {
        d_crec.resize((size_t)n, stream); d_cbl.resize((size_t)n, stream); d_rrec.resize(mm, stream);
        launch_n(k_pack_both, std::max(n, m), stream, n, c_ptr.p, ch.p, lh.p, uh.p, xh.p, x0h.p, d_crec.p, d_cbl.p, m, lp_rowptr.p, loh.p, hih.p, yh.p, y0h.p,
                 d_rrec.p);
    } else {
        KTN_HIP(hipMemcpyAsync(x0h.p, xh.p, n * sizeof(double), hipMemcpyDeviceToDevice, stream));
        if (m > 0) KTN_HIP(hipMemcpyAsync(y0h.p, yh.p, m * sizeof(double), hipMemcpyDeviceToDevice, stream));
    }
}

// the 2 kChkQ sums of the last check: q[0 .. kChkQ) rows, q[kChkQ ..) columns
void Engine::lp_read_check(double* q) {
    if (chk_pinned()) {
        sync();
        std::memcpy(q, h_chk, 2 * kChkQ * sizeof(double));
    } else {
        KTN_HIP(hipMemcpyAsync(q, chkout.p, 2 * kChkQ * sizeof(double), hipMemcpyDeviceToHost, stream));
        sync();
        ipc_check();
    }
}

// restart from the point of the last check: z <- T(z), z0 <- T(z), in the arrays and in the packed records
void Engine::lp_restart() {
    const int64_t n = n_lp, m = M;
    launch_n(k_restart_set, std::max(n, m), stream, n, m, xth.p, xh.p, x0h.p, yth.p, yh.p, y0h.p, packed_on ? d_crec.p : (ColRec*)nullptr,
             packed_on ? d_rrec.p : (RowRec*)nullptr);
}

// the Halpern update after a check that neither ended nor restarted the solve
void Engine::lp_advance(bool spec, int64_t k, double rho) {
    const int64_t n = n_lp, m = M;
    if (spec) {                                       // the check kernels left the update in xnext / ynext
        xh.swap(xnext); yh.swap(ynext);
    } else {
        const double w = (double)(k + 1) / (double)(k + 2);
        launch_n(k_halpern2, std::max(n, m), stream, n, m, xh.p, xth.p, x0h.p, yh.p, yth.p, y0h.p, w, rho);
    }
}

LpResult Engine::lp_solve_core(double tol_p, double tol_g, int mode, bool identity_scaling) {
    auto t0 = std::chrono::steady_clock::now();
    LpResult R;
    auto lap = [&](const char* key, std::chrono::steady_clock::time_point& tp) {     // setup breakdown (profile runs only)
        if (!prm.profile) return;
        sync();
        const auto now = std::chrono::steady_clock::now();
        stats[key] += std::chrono::duration<double>(now - tp).count();
        tp = now;
    };
    auto tp = t0;
    ensure_matrix(want_shift(mode));
    lap("lp_csc_time_s", tp);
    // (row-sharded: the versions are per rank while the scaling is a collective -- no reuse there)
    const bool no_reuse = dev.no_setup_reuse;
    const bool same_matrix = !no_reuse && !row_sharded() && scaled_version == lp_version && scaled_identity == identity_scaling;
    find_long_rows();                                   // (before the scaling: its row passes treat long rows separately)
    if (!same_matrix) compute_scaling(identity_scaling);
    else stats["lp_setup_reuses"] += 1.0;
    lap("lp_scaling_time_s", tp);
    const int64_t n = n_lp, m = M;
    lp_resize_iterates();
    const double sgn = (sense == KTN_MAX) ? -1.0 : 1.0;
    launch_n(k_prep_both, std::max(n, m), stream,
             PrepCols{n, Wc(), lp_l.p, lp_u.p, dc.p, lp_x.p, (mode == 1 ? box.p : (const double*)nullptr), sgn, mode, ch.p, lh.p, uh.p, xh.p},
             PrepRows{m, Wlo(), Whi(), dr.p, lp_y.p, mode, loh.p, hih.p, yh.p});
    if (w_shift) {                                      // the epigraph variable of the start: s = t - a_ref'x - b_ref
        epi_dot(lp_x.p);
        launch(k_epi_var, 1, 1, 0, stream, xh.p, (int32_t)n0, epi_scal.p, (const double*)dc.p, -1, have_omega ? 0 : 1, sgn, epi_newest.p);
    }
    check_launch();
    lp_pick_groups();
    SpMat A{lp_rowptr.p, lp_col.p, r_sval.p};
    SpMat AT{c_ptr.p, c_row.p, c_sval.p};
    lp_choose_tiled(same_matrix);
    scaled_version = lp_version; scaled_identity = identity_scaling;

    // Step size eta = 0.998 / sigma_max(A^).  sigma_max comes from 8 power iterations (round 1: 20; hashed start
    // vector: a constant one can be orthogonal to every row).  The power iteration approaches sigma_max
    // from BELOW, and an estimate a few percent low makes PDHG stall in a limit cycle (seen on dense
    // epigraph cuts: constant fixed-point residual, 8e-6 row violation), so the main loop watches for
    // that stall and backs eta off towards eta_safe.  With the Pock-Chambolle (alpha = 1) pass applied
    // last ||A^||_2 <= 1 is guaranteed (Pock & Chambolle 2011, Lemma 2): eta_safe = 0.998; always using
    // it costs 40 % (cfg3) to 170 % (cfg2) more PDHG iterations than the estimate.
    double smax = 0.0;
    bool have_power = false;
    // sigma_max of the previous solve is reused while the matrix has grown by less than KTN_SMAX_REUSE (a fraction of its
    // rows) since the estimate was made (development switch, default off)
    const double smax_reuse = dev.smax_reuse;
    const bool reuse_smax = mode == 0 && smax_reuse > 0.0 && smax_rows > 0 && m >= smax_rows && !row_sharded() &&
                            (double)(m - smax_rows) <= smax_reuse * (double)smax_rows && smax_prev > 0.0;
    if (same_matrix && smax_version == lp_version && smax_prev > 0.0) smax = smax_prev;       // same matrix, same estimate
    else if (reuse_smax) { smax = smax_prev; stats["lp_smax_reused"] += 1.0; }
    else if ((m > 0 && NNZ > 0) || row_sharded()) {
        // 8 passes from a hashed start vector (a looser estimate is a larger step: 20 -> 8 passes saves 6 % on cfg3 and 8 %
        // on cfg4 beyond the passes themselves; the back-off safeguards of the main loop catch an estimate that is too low).  Norms stay on the device (k_normalize reads them): one host
        // round trip at the end instead of one per pass.  (Measured: warm-starting v from the previous LP makes
        // the estimate tighter and the step therefore smaller -- cfg3 then needs 14 700 instead of 7 800 PDHG
        // iterations; boosting eta by 5 % over the tight estimate stalls the method.  The slightly generous
        // cold estimate plus the back-off safeguard is the better operating point.)
        double* nrm = (chk_pinned() ? h_chk_dev : chkout.p) + 2 * kChkQ + 1;
        auto dot_dev = [&](const double* a, double* out) {
            launch(k_dot_partial, kRedBlocks, kBlock, 0, stream, n, a, a, partials.p);
            launch(k_sum_final, 1, kRedBlocks, 0, stream, partials.p, kRedBlocks, out);
        };
        auto normalize_into = [&](const double* a, double* out) {        // out = a / ||a||: partial sums, then k_normalize_sum adds them up itself
            launch(k_dot_partial, kRedBlocks, kBlock, 0, stream, n, a, a, partials.p);
            launch(k_normalize_sum, (unsigned)ceil_div(n, kRedBlocks), kRedBlocks, 0, stream, n, a, partials.p, out);
        };
        // the start vector -- hashed, normalised -- depends on n alone: made once per handle (and size), read by the first pass in place
        if (power_v0_n != n) {
            power_v.resize(n, stream); power_v0.resize(n, stream);
            launch_n(k_hash_fill, n, stream, n, power_v.p);
            normalize_into(power_v.p, power_v0.p);
            power_v0_n = n;
        }
        const int passes_env = dev.power_passes;
        const int iters = passes_env > 0 ? passes_env : 8;
        // The iterate is re-normalised only every fourth pass (and before the last, whose ||A'A v|| with ||v|| = 1 is the
        // estimate): with ||A^||_2 <= 1 after the Pock-Chambolle pass the un-normalised vector only shrinks slowly, and the
        // Rayleigh quotient does not depend on the scale -- 6 instead of 20 (dot, final sum, normalise) triples per LP solve.
        for (int it = 0; it < iters; ++it) {
            const double* vin = (it == 0) ? power_v0.p : pv.p;
            if (n_long > 0) {
                with_group(grp_rows, [&](auto g) { launch(k_spmv_skip<g()>, group_grid(m, g()), kBlock, 0, stream, m, A, vin, pw.p, kLongRow); });
                launch(k_spmv_long, (unsigned)n_long, 1024, 0, stream, d_longrows.p, A, vin, pw.p);
            } else {
                with_group(grp_rows, [&](auto g) { launch(k_spmv<g()>, group_grid(m, g()), kBlock, 0, stream, m, A, vin, pw.p); });
            }
            const bool norm_now = (it % 4 == 3) || it >= iters - 2;
            if (norm_now) {
                spmv_cols(AT, pw.p, xbar.p);
                allreduce(xbar.p, (size_t)n, 0);            // row-sharded: A'A v = sum over the ranks of A_r'(A_r v)
                if (it == iters - 1) dot_dev(xbar.p, nrm);  // the last pass: ||A'A v||^2 with ||v|| = 1 is the estimate; the vector is not needed again
                else normalize_into(xbar.p, pv.p);
            } else {
                spmv_cols(AT, pw.p, pv.p);
                allreduce(pv.p, (size_t)n, 0);
            }
        }
        have_power = true;
    }
    // The scalars the loop needs -- the power iteration's ||A'A v||, ||A^||_F^2, ||c^||^2 and the finite parts of ||lo^||^2, ||hi^||^2 --
    // are all queued into slots behind chkout's check sums and come back with ONE copy and ONE host synchronisation (they
    // were five round trips, each idling the GPU for ~30 us).
    // (one-GPU solves: the final sums are written straight into the pinned, device-mapped block the check sums use -- no copy kernel,
    //  the host reads them after the synchronisation)
    const bool pin_slots = chk_pinned();
    double* slots = (pin_slots ? h_chk_dev : chkout.p) + 2 * kChkQ;           // [1] power, [2] fro2, [3] nc2, [4] |lo|^2, [5] |hi|^2
    // slots 2..5 (||A^||_F^2, ||c^||^2, finite ||lo^||^2, ||hi^||^2) by one fused pair of launches
    launch(k_setup_norms_partial, kRedBlocks, kBlock, 0, stream, NNZ, r_sval.p, n, ch.p, m, loh.p, hih.p, partials.p);
    launch(k_sum_final_multi, 4, kRedBlocks, 0, stream, partials.p, kRedBlocks, slots + 2);
    if (w_shift) {                                      // ||c|| of the STORED cost vector: the scale of the (unscaled) dual-residual tolerance
        launch(k_dot_partial, kRedBlocks, kBlock, 0, stream, n, lp_c.p, lp_c.p, partials.p);
        launch(k_sum_final, 1, kRedBlocks, 0, stream, partials.p, kRedBlocks, slots + 6);
    }
    // Initial primal weight of a solve that has none to inherit: ||c^|| / ||b^|| with each norm taken as sqrt(count) x geometric
    // mean of the magnitudes (KTN_OMEGA_ROBUST=0: the plain 2-norms).  A few columns whose only entries are ~1e-6 get column
    // factors of 1e5-1e6 and with them c^_j ~ 1e6: three such columns among 1e5 make ||c^||_2 a thousand times the typical
    // magnitude -- cfg3's first LP started at a weight of 2 686, settled at 2.7 six restarts later and took 744 iterations; with
    // this statistic it starts at 3.2 and takes 220.  64 / 48 / 16 seeds: cfg3 -5.5 %, cfg2 -10 %, cfg4 +4 % (-3 % iterations).
    const int omega_robust = dev.omega_robust;
    const bool robust = omega_robust && mode == 0 && !have_omega && !row_sharded() && m > 0;
    if (robust) {                                       // log-magnitude statistics of c^ and of the finite row bounds: slots 8..11
        auto logstat = [&](int64_t cnt, const double* a, const double* b, int slot) {
            launch(k_logabs_partial, kRedBlocks, kBlock, 0, stream, cnt, a, b, partials.p);
            launch(k_sum_final, 1, kRedBlocks, 0, stream, partials.p, kRedBlocks, slots + slot);
            launch(k_sum_final, 1, kRedBlocks, 0, stream, partials.p + kRedBlocks, kRedBlocks, slots + slot + 1);
        };
        logstat(n, ch.p, nullptr, 8);
        logstat(m, loh.p, hih.p, 10);
    }
    double hs[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (!pin_slots) KTN_HIP(hipMemcpyAsync(hs, slots, sizeof(hs), hipMemcpyDeviceToHost, stream));
    double epi_b = 0.0;                                 // b_ref of the working form: the objective constant it carries
    if (w_shift) KTN_HIP(hipMemcpyAsync(&epi_b, epi_scal.p, sizeof(double), hipMemcpyDeviceToHost, stream));
    sync();
    if (pin_slots) std::memcpy(hs, h_chk + 2 * kChkQ, sizeof(hs));
    const double obj_shift = sgn * epi_b;               // internal objective of the stored LP = working objective + obj_shift
    if (have_power) {
        const double nv2 = hs[1];
        smax = (nv2 > 0.0) ? std::sqrt(std::sqrt(nv2)) : 0.0;     // sigma_max^2 ~ ||A'A v||
        if (mode == 0) { smax_prev = smax; smax_rows = m; smax_version = lp_version; }
    }
    lap("lp_power_time_s", tp);
    double fro2 = (NNZ > 0) ? hs[2] : 0.0;                                              // ||A||_2 <= ||A||_F
    allreduce_host(&fro2, 1, 0);
    const double fro = std::sqrt(fro2);
    if (!(smax > 0.0)) smax = fro;
    const double eta_safe = 0.998 / std::max(identity_scaling ? fro : std::min(1.0, fro), 1e-12);
    double eta = std::max(0.998 / std::max(smax, 1e-12), eta_safe);
    int infeas_hits = 0;
    PdhgCtl pc = pdhg_start();
    stats["lp_setup_time_s"] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const double nc2 = hs[3];
    const double nc2_tol = w_shift ? hs[6] : nc2;       // (the working cost carries a_ref: not the scale the dual residual is judged on)
    double nb2 = (m > 0) ? hs[4] + hs[5] : 0.0;
    allreduce_host(&nb2, 1, 0);
    double omega_ref = (nc2 > 0.0 && nb2 > 0.0) ? std::sqrt(nc2 / nb2) : 1.0;
    if (robust && hs[9] > 0.0 && hs[11] > 0.0) {
        omega_ref = std::sqrt(hs[9] / hs[11]) * std::exp(hs[8] / hs[9] - hs[10] / hs[11]);
        stats["lp_omega_robust"] += 1.0;
    }
    double om = (have_omega && mode == 0) ? omega : omega_ref;
    const double om_start = om;
    const double rho = 1.0;
    // The rules of this loop's checks (pdhg_check.hpp; DESIGN.md section 5 sets them beside the device-side loops').
    PdhgRules rules{};
    rules.tol_p = tol_p; rules.tol_g = tol_g;
    rules.dres_scale = 1.0 + std::sqrt(nc2_tol);
    // Primal-stagnation exit (lp_stag_factor).  On LPs with degenerate duals the primal part converges within a few hundred
    // iterations while the duality gap crawls for 10 000 more.  "Flat" is within 0.4 tol_g over the last TWO
    // checks (KTN_FLAT_FACTOR, KTN_STAG_CHECKS; 0.1 and three until round 3: -12 % and -5 ... -7 % PDHG iterations on the BASELINE
    // shapes, objective errors, reference models, fuzz set and shape matrix unchanged).
    // A model with free variables runs inside the box the presolve put around it (boundroutine, model.jl:175-197): a loosely solved
    // LP can then sit ANYWHERE in that box, and cuts taken at |x| ~ 1e13 have constants of 1e31 that no first-order LP survives (fuzz
    // model 2/109: primal weight 1e-30, objective 6e26, :Error).  Such models keep the conservative rules of round 2 and 3: three
    // flat checks within 0.1 of the gap tolerance, gap certified to 100 tolerances, the undamped weight update.
    rules.stag_factor = mode != 0 ? 0.0 : (has_inf_bound ? std::min(prm.lp_stag_factor, 100.0) : prm.lp_stag_factor);
    rules.flat_factor = has_inf_bound ? std::min(dev.flat_factor, 0.1) : dev.flat_factor;
    rules.flat_checks = has_inf_bound ? 3 : dev.stag_checks;
    // Stalled-row allowance.  tol_p's floor is 0.3 f_tol -- a safety factor, the stop rule itself is the sweep at f_tol -- so a
    // violation that has not moved by 2 % over three checks is accepted up to 3 tol_p (0.9 f_tol; seen: 3.47e-7 against 3.0e-7 for
    // 2.1e6 iterations).  An INTERMEDIATE solve (tol_p above its floor: its x* only has to be a useful separation point, cuts are
    // valid anywhere) accepts up to 10 tol_p -- the new cuts of the next sweep are what ends such a stall.
    rules.stall_accept = (tol_p > prm.lp_tol_floor * prm.f_tol * (1.0 + 1e-9)) ? 10.0 : 3.0;
    rules.eta_safe = eta_safe;
    rules.nan_exit = true;
    rules.grow_backoff = true;          // (seen on cfg3 seeds 28/29: r0 = 6 -> 87 -> 530 -> 1e5 until the flat-residual rule fired)
    // (row-sharded: the decision to consolidate must not depend on what THIS rank holds -- a rank that consolidated while another did
    //  not would leave the sequence of collectives -- so the local conditions are dropped; k_consolidate on a rank without cuts is a no-op)
    rules.consolidate = mode == 0 && (row_sharded() ? (prm.lp_dual_inherit != 0) : (prm.lp_dual_inherit && lists_ok() && list_count() > 0 && m > M_base));
    rules.omega_ref = omega_ref;
    // Unearned restarts carry little information about the weight (round 4; profiles/r04_omega_ab.txt).  A solve's first restarts
    // come "by the clock" (k >= 0.36 it), whether or not the residual has moved; after a warm start whose primal part is already
    // converged x moves by 1e-6 of its norm in such a period, and the ratio of that movement to the dual's sent the weight
    // 603 -> 0.16 in four restarts (cfg2 seed 92: 44 000 iterations to earn it back).  So the weight of the new ratio in the geometric
    // mean grows with the length of the period it was measured over: theta = 0.5 min(1, k / K), K = KTN_OMEGA_ART_K.
    rules.om_art = dev.omega_art != 0;
    rules.om_art_k = has_inf_bound ? 0.0 : dev.omega_art_k;
    rules.om_art_clamp = dev.omega_art_clamp;
    rules.om_clamp = dev.omega_clamp;
    rules.om_clamp_down = dev.omega_clamp_down;
    if (dev.debug_lp)
        std::fprintf(stderr, "[lp setup mode %d] m %lld n %lld nnz %lld smax %.4g fro %.4g nc2 %.4g nc2_tol %.4g nb2 %.4g omega_ref %.4g om0 %.4g shift %d b_ref %.9g n_long %lld tol_p %.3g tol_g %.3g\n",
                     mode, (long long)m, (long long)n, (long long)NNZ, smax, fro, nc2, nc2_tol, nb2, omega_ref, om, (int)w_shift, epi_b, (long long)n_long, tol_p, tol_g);

    // anchors z0 = z; with the packed records of the plain steps (not for the tiled / row-sharded forms, whose steps are
    // split into SpMV + element-wise kernels)
    lp_set_anchors(true);

    int64_t k = 0, it = 0;
    const bool dbg_lp = dev.debug_lp;
    R.status = KTN_STATUS_USERLIMIT;
    const int64_t max_it = lp_iter_budget > 0 ? std::min<int64_t>(lp_iter_budget, prm.lp_max_iter) : prm.lp_max_iter;
    const int chk = std::max(1, prm.lp_check_every);
    const int plain_len = std::min(chk - 1, (int)kMaxChunk);
    const int first_chunk = dev.first_chunk;
    bool plain_next = false, near_conv = false, primal_ok = false;
    const int stag_chunk = dev.stag_chunk;
    // throughput mode: one workgroup per block runs its LP to the end (batch_lp.hpp); the ordinary loop below only serves
    // as the fall-back when a block reports that it could not finish
    bool blocks_done = false;
    if (n_blocks > 0 && mode == 0 && !row_sharded() && n_long == 0 && m > 0 && !prm.profile) {
        if (blocks_built_rows != M) build_blocks();
        // (the block kernel has no growing-residual back-off: next to columns without a bound it starts with the safe step)
        blocks_done = lp_solve_blocks(tol_p, tol_g, has_inf_bound ? eta_safe : eta, &R, max_it);
        if (blocks_done) it = R.iters;
    }
    const int near_env = dev.near_chunk;
    const int near_chunk = near_env >= 0 ? near_env : prm.lp_near_check;
    while (!blocks_done && it < max_it) {
        const double tau = eta / om, sigma = eta * om;
        if (plain_next) {
            // ---- a chunk of plain (update) iterations between two checks
            plain_next = false;
            // the first chunk after a restart is shorter: the restarted iteration moves fastest there and an
            // early check catches the next restart / termination sooner
            int want = (k <= 1 && first_chunk > 0) ? std::min(first_chunk, plain_len) : plain_len;
            // close to the tolerances the next check comes sooner: a solve ends on average half a chunk after it converged
            if (near_conv && near_chunk > 0) want = std::min(want, near_chunk);
            if (primal_ok && stag_chunk > 0 && mode == 0) want = std::min(want, stag_chunk);
            const int np = (int)std::min<int64_t>(want, max_it - it);
            if (np <= 0) continue;
            for (int j = 0; j < np; ++j) {
                const double w = (double)(k + j + 1) / (double)(k + j + 2);
                pdhg_iteration(A, AT, tau, sigma, w, rho);
            }
            k += np; it += np;
            continue;
        }
        // ---- check iteration: PDHG step without update, KKT + fixed-point residual
        const bool spec_next = launch_check(A, AT, tau, sigma, (double)(k + 1) / (double)(k + 2), rho);
        check_launch();
        double q[2 * kChkQ];
        lp_read_check(q);
        if (prm.profile) ev_flush();
        const double dobj_rows = q[2], yt2 = q[4];
        const PdhgSums S{q[0], q[1], q[3], q[kChkQ + 5], q[kChkQ + 8], q[kChkQ + 9], yt2,
                         q[kChkQ + 6] + obj_shift, dobj_rows + q[kChkQ + 7] + obj_shift, q[12], q[kChkQ + 13]};
        const PdhgStop t = pdhg_stop(S, rules, pc, om, eta, k);
        if (dbg_lp) std::fprintf(stderr, "[lp mode %d] it %7lld k %6lld r %.3e pviol %.3e dres %.3e gap %.3e pobj %.10g dobj %.10g om %.3g eta %.3g\n",
                                 mode, (long long)it, (long long)k, t.r, S.pviol, S.dres, t.gap, S.pobj, S.dobj, om, eta);
        R.pobj = S.pobj; R.dobj = S.dobj; R.row_viol = S.pviol; R.gap = t.gap;
        R.dres_rel = S.dres / rules.dres_scale;
        near_conv = t.near; primal_ok = t.primal_ok;
        if (t.exit != PDHG_EXIT_NONE) {
            if (t.exit == PDHG_EXIT_STAGNATION) { R.stag_exit = true; stats["lp_stagnation_exits"] += 1.0; }
            if (t.exit == PDHG_EXIT_STALLED_ROW) stats["lp_stalled_row_exits"] += 1.0;
            R.status = t.exit == PDHG_EXIT_NAN ? KTN_STATUS_ERROR : KTN_STATUS_OPTIMAL;
            ++it;
            break;
        }
        // primal infeasibility: yt is a Farkas certificate when the dual objective of the c = 0 problem is
        // positive (weak duality makes it <= 0 for every sign-valid y of a feasible LP).  Two checks in a row.
        // (after the exits: the plateau exits accept a row violation above tol_p, which the certificate requires)
        if (mode == 0 && (m > 0 || row_sharded())) {     // (row-sharded: every quantity below is all-reduced, so all ranks agree)
            const double farkas = dobj_rows + q[kChkQ + 10];
            const double mag = q[10] + q[kChkQ + 11] + 1e-300;
            const bool cert = farkas > 1e-6 * mag && q[kChkQ + 14] <= 1e-9 * (1.0 + std::sqrt(yt2)) && S.pviol > tol_p;
            infeas_hits = cert ? infeas_hits + 1 : 0;
            if (infeas_hits >= 2 && it >= 2 * chk) {
                R.status = KTN_STATUS_INFEASIBLE;
                ++it;
                break;
            }
        }
        const PdhgNext nx = pdhg_next(S, rules, pc, t, om, eta, k, it);
        if (nx.backoff != PDHG_BACKOFF_NONE) stats["lp_eta_backoffs"] += 1.0;
        if (nx.backoff == PDHG_BACKOFF_GROW) stats["lp_divergence_backoffs"] += 1.0;
        eta = nx.eta;
        if (nx.action == PDHG_CONSOLIDATE) {
            // PDHG is idling between near-parallel cuts of one NL row (k_consolidate): move the multiplier mass onto the
            // tightest cut at the current point and restart from there
            stats["lp_consolidations"] += 1.0;
            launch_n(k_unscale, n, stream, n, xth.p, dc.p, pv.p);
            SpMat Au{lp_rowptr.p, lp_col.p, Wval()};
            with_group(grp_rows, [&](auto g) { launch(k_spmv<g()>, group_grid(m, g()), kBlock, 0, stream, m, Au, pv.p, pw.p); });
            KTN_HIP(hipMemsetAsync(d_anynf.p + 1, 0, sizeof(int32_t), stream));
            launch_n(k_consolidate, list_count(), stream, list_count(), list_heads(), d_cutprev.p, pw.p, Wlo(), Whi(), dr.p, tol_p, yth.p, d_anynf.p + 1);
        }
        if (nx.action != PDHG_ADVANCE) {
            if (nx.action == PDHG_RESTART) {
                if (dbg_lp) std::fprintf(stderr, "[lp restart] it %lld k %lld decayed %d dx %.3e dy %.3e |xt| %.3e |yt| %.3e om %.4g\n", (long long)it, (long long)k, (int)(t.r <= 0.8 * pc.r0), std::sqrt(S.dx0sq), std::sqrt(S.dy0sq), std::sqrt(S.xt2), std::sqrt(S.yt2), om);
                stats["lp_restarts"] += 1.0;
            }
            om = nx.om;
            if (nx.backoff == PDHG_BACKOFF_GROW && has_inf_bound) {
                // The residual grew check after check: the power iteration gave a sigma_max below the true one (a block-diagonal
                // matrix has one near-largest singular value per block, which 8 passes do not separate) and the iterates ran
                // away.  A box clamps them back once the step is safe; a column without a bound keeps what it picked up
                // (seen: |x| 1e13 after 65 iterations at eta sigma_max = 1.08, not back after 400 000).  Such a solve starts
                // again, from the point of the box nearest to 0, with the safe step and the weight it began with.
                launch_n(k_cold_point, std::max(n, m), stream, n, m, lh.p, uh.p, xth.p, yth.p);
                eta = eta_safe;
                om = om_start;
                stats["lp_cold_restarts"] += 1.0;
            }
            lp_restart();
            k = 0;
            ++it;
            continue;
        }
        lp_advance(spec_next, k, rho);
        ++k; ++it;
        plain_next = true;       // (after a restart k == 0 and the next pass is a check again: it needs r0)
    }
    R.iters = it;
    // un-scale the last PDHG point (xt, yt)
    if (mode == 0) {
        launch_n(k_unscale2, std::max(n, m), stream, n, xth.p, dc.p, lp_x.p, m, yth.p, dr.p, lp_y.p);
        if (w_shift) {                                  // back to the epigraph variable of the stored LP: t = s + a_ref'x + b_ref
            epi_dot(lp_x.p);
            launch(k_epi_var, 1, 1, 0, stream, lp_x.p, (int32_t)n0, epi_scal.p, (const double*)nullptr, 1, 0, sgn, epi_newest.p);
        }
        omega = om;
        have_omega = true;
        objval = sgn * R.pobj + c0;
    } else {
        launch_n(k_unscale, n, stream, n, xth.p, dc.p, d_ray.p);
    }
    check_launch();
    sync();
    if (prm.profile) ev_flush();
    stats["pdhg_iters"] += (double)it;
    stats["lp_solves"] += 1.0;
    // (the quantities Engine::step's floor rule reads: a host-driven loop over the same entry points -- distributed.py -- needs them too)
    stats["lp_last_row_viol"] = R.row_viol; stats["lp_last_gap"] = R.gap; stats["lp_last_dres_rel"] = R.dres_rel;
    stats["lp_last_stag_exit"] = R.stag_exit ? 1.0 : 0.0;
    stats["lp_time_s"] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return R;
}

void Engine::pdhg_raw(const double* x0, const double* y0, double eta, double omega_, int64_t iters, double* x_out,
                      double* y_out) {
    ensure_matrix(false);
    compute_scaling(true);
    scaled_version = 0;                                  // (lp_solve_core must not take this identity scaling for its own)
    const int64_t n = n_lp, m = M;
    lp_resize_iterates();
    const double sgn = (sense == KTN_MAX) ? -1.0 : 1.0;
    KTN_HIP(hipMemcpyAsync(lp_x.p, x0, n * sizeof(double), hipMemcpyHostToDevice, stream));
    if (m > 0) KTN_HIP(hipMemcpyAsync(lp_y.p, y0, m * sizeof(double), hipMemcpyHostToDevice, stream));
    launch_n(k_prep_cols, n, stream, n, lp_c.p, lp_l.p, lp_u.p, dc.p, lp_x.p, (double*)nullptr, sgn, 0, ch.p, lh.p, uh.p, xh.p);
    launch_n(k_prep_rows, m, stream, m, lp_lo.p, lp_hi.p, dr.p, lp_y.p, 0, loh.p, hih.p, yh.p);
    grp_rows = pick_group(m ? (double)NNZ / (double)m : 1.0);
    grp_cols = pick_group(n ? (double)NNZ / (double)n : 1.0);
    SpMat A{lp_rowptr.p, lp_col.p, r_sval.p};
    SpMat AT{c_ptr.p, c_row.p, c_sval.p};
    packed_on = false;
    KTN_HIP(hipMemcpyAsync(x0h.p, xh.p, n * sizeof(double), hipMemcpyDeviceToDevice, stream));
    if (m > 0) KTN_HIP(hipMemcpyAsync(y0h.p, yh.p, m * sizeof(double), hipMemcpyDeviceToDevice, stream));
    find_long_rows();
    lp_choose_tiled(false);                              // (scaled_version = 0 above: the next solve never reads tiled_built)
    const double tau = eta / omega_, sigma = eta * omega_;
    for (int64_t k = 0; k < iters; ++k) {
        const double w = (double)(k + 1) / (double)(k + 2);
        pdhg_iteration(A, AT, tau, sigma, w, 1.0);
        if ((k & 255) == 255) { sync(); if (prm.profile) ev_flush(); }
    }
    sync();
    if (prm.profile) ev_flush();
    check_launch();
    KTN_HIP(hipMemcpyAsync(x_out, xh.p, n * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (m > 0) KTN_HIP(hipMemcpyAsync(y_out, yh.p, m * sizeof(double), hipMemcpyDeviceToHost, stream));
    sync();
}

// Scripted test hook: the state (x, y) with anchors (x0, y0), given in the stored LP's space and scaled by k_prep_both as a
// solve scales its start, then a short list of ops through the member functions lp_solve_core itself runs.  k is the
// Halpern counter of the first op.  flags: KTN_LPS_IDENTITY (dr = dc = 1), KTN_LPS_PACKED (packed records for the plain
// steps), KTN_LPS_NO_SPEC (the check does not leave the update in xnext / ynext: the advance is k_halpern2).
void Engine::lp_script(const LpScriptIO& io) {
    const bool identity = (io.flags & KTN_LPS_IDENTITY) != 0;
    ensure_matrix(false);
    find_long_rows();
    scal_rows = 0;                                       // (a cold equilibration, whatever ran on this handle before)
    compute_scaling(identity);
    scaled_version = 0;                                  // (lp_solve_core must not take this setup for its own)
    const int64_t n = n_lp, m = M;
    lp_resize_iterates();
    const double sgn = (sense == KTN_MAX) ? -1.0 : 1.0;
    auto prep = [&](const double* xs, const double* ys) {
        KTN_HIP(hipMemcpyAsync(lp_x.p, xs, n * sizeof(double), hipMemcpyHostToDevice, stream));
        if (m > 0) KTN_HIP(hipMemcpyAsync(lp_y.p, ys, m * sizeof(double), hipMemcpyHostToDevice, stream));
        launch_n(k_prep_both, std::max(n, m), stream, PrepCols{n, Wc(), lp_l.p, lp_u.p, dc.p, lp_x.p, (const double*)nullptr, sgn, 0, ch.p, lh.p, uh.p, xh.p},
                 PrepRows{m, Wlo(), Whi(), dr.p, lp_y.p, 0, loh.p, hih.p, yh.p});
    };
    lp_pick_groups();
    SpMat A{lp_rowptr.p, lp_col.p, r_sval.p};
    SpMat AT{c_ptr.p, c_row.p, c_sval.p};
    lp_choose_tiled(false);
    prep(io.x0, io.y0);                                  // the anchors first: lp_set_anchors takes them from xh / yh ...
    lp_set_anchors((io.flags & KTN_LPS_PACKED) != 0);
    prep(io.x, io.y);                                    // ... then the state itself
    check_launch();
    stats["lp_long_rows"] = (double)n_long; stats["lp_long_cols"] = (double)n_longc;
    stats["lp_packed"] = packed_on ? 1.0 : 0.0; stats["lp_packed_trips"] = (double)packed_trips;
    stats["lp_grp_rows"] = (double)grp_rows; stats["lp_grp_cols"] = (double)grp_cols;
    stats["lp_tiled"] = tiled_on ? 1.0 : 0.0;
    stats["lp_tiled_check"] = (tiled_on && m > 0 && !dev.no_tiled_check) ? 1.0 : 0.0;
    stats["lp_tiled_pieces"] = tiled_on ? (double)std::max(tA.pieces, tAT.pieces) : 0.0;
    stats["lp_check_pinned"] = chk_pinned() ? 1.0 : 0.0;
    const double tau = io.eta / io.omega, sigma = io.eta * io.omega, rho = 1.0;
    int64_t k = io.k;
    bool checked = false, spec = false;
    double q[2 * kChkQ];
    for (int q_ = 0; q_ < 2 * kChkQ; ++q_) q[q_] = 0.0;
    for (int64_t o = 0; o < io.nops; ++o) {
        const double w = (double)(k + 1) / (double)(k + 2);
        switch (io.ops[o]) {
            case KTN_LPOP_STEP:
                launch_x(AT, tau, w, rho, true, nullptr, nullptr);
                launch_y(A, sigma, w, rho, nullptr, nullptr);
                ++k; checked = false;
                break;
            case KTN_LPOP_CHECK:
                spec = launch_check(A, AT, tau, sigma, (io.flags & KTN_LPS_NO_SPEC) ? -1.0 : w, rho);
                check_launch();
                lp_read_check(q);
                if (spec && io.xnext_out) xnext.download(io.xnext_out, (size_t)n, stream);
                if (spec && io.ynext_out && m > 0) ynext.download(io.ynext_out, (size_t)m, stream);
                checked = true;
                break;
            case KTN_LPOP_ADVANCE:
                KTN_REQUIRE(checked, "lp_script: advance without a check before it");
                lp_advance(spec, k, rho);
                ++k; checked = false;
                break;
            case KTN_LPOP_RESTART:
                KTN_REQUIRE(checked, "lp_script: restart without a check before it");
                lp_restart();
                k = 0; checked = false;
                break;
            default:
                KTN_REQUIRE(false, "lp_script: unknown op");
        }
        if ((o & 255) == 255) sync();
    }
    check_launch();
    sync();
    stats["lp_check_spec"] = spec ? 1.0 : 0.0;
    if (io.spec_out) *io.spec_out = spec ? 1 : 0;
    if (io.q_out) std::memcpy(io.q_out, q, sizeof(q));
    auto out = [&](DBuf<double>& b, double* dst, int64_t cnt) { if (dst && cnt > 0) b.download(dst, (size_t)cnt, stream); };
    out(xh, io.x_out, n); out(x0h, io.x0_out, n); out(xth, io.xt_out, n); out(dc, io.dc_out, n);
    out(yh, io.y_out, m); out(y0h, io.y0_out, m); out(yth, io.yt_out, m); out(dr, io.dr_out, m);
    sync();
}

// Scaling hook: a cold compute_scaling(false) on the current LP; dr, dc and the factors before the Pock-Chambolle pass
// (dr_r, dc_r: kept when lp_ruiz_warm > 0)
void Engine::lp_scaling(double* dr_out, double* dc_out, double* drr_out, double* dcr_out) {
    ensure_matrix(false);
    find_long_rows();
    scal_rows = 0;
    compute_scaling(false);
    scaled_version = 0;
    stats["lp_long_rows"] = (double)n_long; stats["lp_long_cols"] = (double)n_longc;
    if (M > 0) { dr.download(dr_out, (size_t)M, stream); dr_r.download(drr_out, (size_t)M, stream); }
    dc.download(dc_out, (size_t)n_lp, stream); dc_r.download(dcr_out, (size_t)n_lp, stream);
    sync();
}

// ------------------------------------------------------------------------------------
// ECP driver
// ------------------------------------------------------------------------------------
// "status == :Unbounded" + getunboundedray: solve the recession-cone LP (oracle/lp.py).
bool Engine::recession_ray() {
    box.resize((size_t)n_lp, stream);
    launch_n(k_fill, n_lp, stream, n_lp, box.p, 1.0);
    if (!obj_linear) {
        KTN_HIP(hipMemsetAsync(d_scal.p + 1, 0, sizeof(double), stream));
        launch_n(k_aux_box, M, stream, M, lp_rowptr.p, lp_col.p, lp_val.p, (int32_t)n0, d_scal.p + 1);
        double w = 0.0;
        KTN_HIP(hipMemcpyAsync(&w, d_scal.p + 1, 8, hipMemcpyDeviceToHost, stream));
        sync();
        allreduce_host(&w, 1, 1);
        launch_n(k_fill, 1, stream, (int64_t)1, box.p + n0, 1.0 + w);
    }
    // Small models (the reference's own tests: a handful of free variables): the recession LP by the exact kernel.  It is a
    // degenerate LP with tolerances of 1e-9 -- the first-order method can need more than its iteration limit for six rows and
    // five columns (fuzz model 13/142: 2e6 iterations, limit reached, "no ray" reported, and the main LP then ran along the ray
    // it had missed until ITS limit: :UserLimit where the oracle ends :Optimal) -- and the simplex ray is what the reference
    // hands to boundroutine (src/model.jl:233-236).
    if (n_lp <= kDenseMaxN && !row_sharded() && prm.lp_dense_after != 0 && M * n_lp <= 8000000) {
        bool unb = false;
        if (recession_ray_dense(&unb)) return unb;
    }
    LpResult R = lp_solve(1e-9, 1e-7, 1);
    return R.status == KTN_STATUS_OPTIMAL && R.pobj < -1e-6;
}

// min c'd over the recession cone of the LP's rows inside the box: variables with a finite bound keep that side at 0, free sides
// get -/+ box; finite row sides become 0 (k_prep_cols / k_prep_rows, mode 1, with unit scaling).  d -> d_ray.  Returns false when
// the exact kernel gives up (the caller falls back to the first-order solve).
bool Engine::recession_ray_dense(bool* unbounded) {
    const int n = (int)n_lp;
    const int64_t m = M;
    const size_t mm = (size_t)std::max<int64_t>(m, 1);
    const double sgn = (sense == KTN_MAX) ? -1.0 : 1.0;
    DBuf<double> ones, rl, ru, rc, rx, rlo, rhi, ry, out;
    DBuf<int32_t> W, Wv;
    ones.resize(std::max<size_t>(mm, (size_t)n), stream);
    launch_n(k_fill, (int64_t)ones.n, stream, (int64_t)ones.n, ones.p, 1.0);
    rl.resize(n, stream); ru.resize(n, stream); rc.resize(n, stream); rx.resize(n, stream);
    rlo.resize(mm, stream); rhi.resize(mm, stream); ry.resize(mm, stream); out.resize(4, stream);
    W.resize(n, stream); Wv.resize(1, stream); Wv.zero(stream);
    lp_x.resize((size_t)n, stream);
    launch_n(k_prep_cols, n, stream, (int64_t)n, lp_c.p, lp_l.p, lp_u.p, ones.p, lp_x.p, box.p, 1.0, 1, rc.p, rl.p, ru.p, rx.p);
    launch_n(k_prep_rows, m, stream, m, lp_lo.p, lp_hi.p, ones.p, ones.p, 1, rlo.p, rhi.p, ry.p);
    ds_dense.resize(mm * (size_t)n, stream);
    d_ray.resize((size_t)n, stream);
    DenseLpIO P;
    P.n = n; P.m = m; P.rowptr = lp_rowptr.p; P.col = lp_col.p; P.val = lp_val.p; P.lo = rlo.p; P.hi = rhi.p;
    P.l = rl.p; P.u = ru.p; P.c = lp_c.p; P.sgn = sgn;
    P.dense = ds_dense.p; P.W = W.p; P.Wvalid = Wv.p; P.x = d_ray.p; P.y = ry.p; P.out = out.p;
    P.max_pivots = 200 + 20 * n + (int)std::min<int64_t>(m, 100000);
    P.tol = 1e-9;
    launch(k_dense_lp, 1, 256, 0, stream, P);
    check_launch();
    double o[4];
    KTN_HIP(hipMemcpyAsync(o, out.p, sizeof(o), hipMemcpyDeviceToHost, stream));
    sync();
    stats["dense_recession_solves"] += 1.0;
    if ((int)o[0] != 0) { stats["dense_recession_fallbacks"] += 1.0; return false; }
    *unbounded = o[2] < -1e-6;
    return true;
}

}  // namespace ktn
