// ecp.hip -- optimize! (src/model.jl:219-319): presolve, the cutting-plane loop, the terminal refinement, the device-side batch loop  (struct Engine: engine.hpp)
#include "engine.hpp"
#include "launch.hpp"
#include "kernels.hpp"
#include "batch_lp.hpp"
#include "batch_ecp.hpp"
#include "batch_warm.hpp"

namespace ktn {

// k_blocks_rewarm over the resident arenas (batch_warm.hpp): screen, clamp, compaction; the records into h_rewarm.  Runs once per
// state of the data: a second call before the next setter or launch returns with h_rewarm as it is.
void Engine::blocks_rewarm() {
    if (blocks_rewarmed) return;
    const int nb = (int)n_blocks;
    e_rewarm.resize((size_t)nb * 8, stream);
    WarmBatch W;
    W.blk_col = d_blkcol.p; W.blk_lin = d_blklin.p; W.blk_nl = d_blknl.p; W.arena = d_ar.p;
    W.rptr = e_rptr.p; W.rcol = e_rcol.p; W.rval = e_rval.p; W.lo = e_lo.p; W.hi = e_hi.p; W.y = e_y.p;
    W.lam = blocks_last_esh ? e_lam.p : nullptr;
    W.last_cut = e_last.p; W.cut_prev = e_prev.p;
    W.crow = e_crow.p; W.cval = e_cval.p; W.dr = e_dr.p; W.loh = e_loh.p; W.hih = e_hih.p;
    W.l = lp_l.p; W.u = lp_u.p; W.x = lp_x.p; W.res = e_res.p; W.out = e_rewarm.p;
    W.tol0 = prm.lp_tol_floor * prm.f_tol; W.purge_margin = prm.purge_margin;
    for (hipEvent_t& e : ev_rewarm)                      // the kernel's own begin / end timestamps ("ecp_blocks_rewarm_kernel_s")
        if (!e) KTN_HIP(hipEventCreate(&e));
    launch_ev(k_blocks_rewarm, (unsigned)nb, kEcpThreads, 0, stream, ev_rewarm[0], ev_rewarm[1], W);
    check_launch();
    h_rewarm = e_rewarm.to_host(stream);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev_rewarm[0], ev_rewarm[1]) != hipSuccess) { (void)hipGetLastError(); ms = 0.f; }
    stats["ecp_blocks_rewarm_kernel_s"] = (double)ms * 1e-3;
    double cnt[3] = {0.0, 0.0, 0.0}, dropped = 0.0, clamped = 0.0;
    for (int bb = 0; bb < nb; ++bb) {
        const double* r = h_rewarm.data() + (size_t)bb * 8;
        cnt[(int)r[0]] += 1.0; dropped += r[3]; clamped += r[4];
        if ((int)r[0] == 1) h_blkres[(size_t)bb * 8 + 6] = r[1];       // (ktn_blocks_get_cuts / _duals read the compacted arena)
    }
    stats["ecp_blocks_warm_instances"] = cnt[1]; stats["ecp_blocks_warm_cold_instances"] = cnt[0]; stats["ecp_blocks_warm_infeasible"] = cnt[2];
    stats["ecp_blocks_warm_dropped_rows"] = dropped; stats["ecp_blocks_warm_clamped_cols"] = clamped;
    kkt_cached = false;                                  // (rows moved: the report is built again from the re-threaded lists)
    blocks_rewarmed = true;
}

// ktn_set_row_bounds with a device launch standing: k_blocks_rebase over the resident arenas (batch_warm.hpp), the old row bounds
// still in d_lb / d_ub, the new ones in d_lb_new / d_ub_new, lp_lo / lp_hi already those of the new linear rows.  *cnt += rows moved.
void Engine::blocks_rebase(unsigned long long* cnt, hipEvent_t e0, hipEvent_t e1) {
    RebaseBatch W;
    W.blk_lin = d_blklin.p; W.blk_nl = d_blknl.p; W.arena = d_ar.p; W.nl_rows = d_nlrows.p;
    W.lp_lo = lp_lo.p; W.lp_hi = lp_hi.p;
    W.lb_old = d_lb.p; W.ub_old = d_ub.p; W.lb_new = d_lb_new.p; W.ub_new = d_ub_new.p;
    W.lo = e_lo.p; W.hi = e_hi.p; W.last_cut = e_last.p; W.cut_prev = e_prev.p;
    W.res = e_res.p; W.cnt = cnt;
    launch_ev(k_blocks_rebase, (unsigned)n_blocks, kEcpThreads, 0, stream, e0, e1, W);
    check_launch();
    kkt_cached = false;                                  // (the report reads the arenas' row bounds)
}

// Throughput mode, device-side loop (batch_ecp.hpp).  Returns kBlocksUnfit when the problem does not qualify (nothing launched),
// kBlocksOpen when an instance could not finish (arena overflow, LP status) -- the caller then runs the ordinary loop, or with
// KTN_BLOCKS_NO_FALLBACK reports the first such instance's status -- and kBlocksDone when every instance ended :Optimal.
// KTN_BLOCKS_SUPPORTING with an interior point in hand launches k_ecp_blocks<1> (the root search inside the emit pass), everything
// else k_ecp_blocks<0>.
// KTN_BLOCKS_WARM with the arenas of the last device launch still standing (blocks_warm_ok, the same cap_mul): nothing is uploaded
// or resized, k_blocks_rewarm screens, clamps and compacts every arena, and the instantiation with the trailing EcpWarm starts each
// instance from what is left (batch_warm.hpp).  Instances the screen ends :Infeasible do not send the batch to the host loop, which
// could not help them: when they are the only ones not :Optimal the return is kBlocksScreened, status the first of them.  Without
// such a previous launch the flag changes nothing: the cold launch, and "ecp_blocks_warm_launches" does not move.
int Engine::optimize_blocks_device(int cap_mul, int flags) {
    const bool keep = (flags & KTN_BLOCKS_NO_FALLBACK) != 0;
    const bool want_warm = (flags & KTN_BLOCKS_WARM) != 0 && blocks_warm_ok && blocks_launched && cap_mul == blocks_cap_mul &&
                      (int64_t)h_ar_rows.size() == n_blocks;
    const bool esh = (flags & KTN_BLOCKS_SUPPORTING) != 0 && esh_mode() && xint_found != 0;
    // (rows: separable, tape or QUAD, linear or not; k_ecp_blocks evaluates tape rows with the interpreter of k_tape_eval and QUAD
    //  rows with the two passes of quad_rows.hpp.  A handle whose OBJECTIVE row is KTN_ROW_QUAD -- a hand-fused QuadNLP; nlp.fuse_problems
    //  always emits a separable objective of LIN atoms -- keeps the ordinary loop: include/katana_hip.h, ktn_optimize_blocks)
    if (n_blocks <= 0 || !obj_linear || sense != KTN_MIN || has_inf_bound || n_host > 0 || prm.vis_data) return kBlocksUnfit;
    if (h_rowkind[(size_t)(m_ext - 1)] == KTN_ROW_QUAD) return kBlocksUnfit;
    for (int64_t i = 0; i < m_ext - 1; ++i)
        if (h_rowkind[(size_t)i] != KTN_ROW_SEP && h_rowkind[(size_t)i] != KTN_ROW_TAPE && h_rowkind[(size_t)i] != KTN_ROW_QUAD) return kBlocksUnfit;
    const int nb = (int)n_blocks;
    auto block_of_col = [&](int64_t c) { return (int)(std::upper_bound(h_blkcol.begin(), h_blkcol.end(), c) - h_blkcol.begin()) - 1; };
    // linear rows of the loaded LP (in original row order) and NL slots must be grouped by instance, instance after instance
    std::vector<int64_t> lin_rows, blk_lin((size_t)nb + 1, 0), blk_nl((size_t)nb + 1, 0), nnz_lin((size_t)nb, 0), nnz_nl((size_t)nb, 0);
    // the instances' ranges of the QUAD NL launch list (build_quad_rows: rows and entry positions in ascending row order)
    std::vector<int64_t> blk_qrow((size_t)nb + 1, 0), blk_qent((size_t)nb + 1, 0);
    {
        std::vector<char> is_nl((size_t)m0, 0);
        for (auto r : h_nlrows) if (r < m0) is_nl[(size_t)r] = 1;
        for (int64_t i = 0; i < m0; ++i) if (!is_nl[(size_t)i]) lin_rows.push_back(i);
    }
    if ((int64_t)lin_rows.size() != M_base) return kBlocksUnfit;
    int prev = 0;
    for (size_t k = 0; k < lin_rows.size(); ++k) {
        const int64_t r = lin_rows[k];
        if (h_rowptr[r + 1] == h_rowptr[r]) return kBlocksUnfit;
        const int bb = block_of_col(h_col[(size_t)h_rowptr[r]]);
        if (bb < prev || bb >= nb) return kBlocksUnfit;
        for (int64_t e = h_rowptr[r]; e < h_rowptr[r + 1]; ++e) if (block_of_col(h_col[(size_t)e]) != bb) return kBlocksUnfit;
        prev = bb;
        blk_lin[(size_t)bb + 1] += 1;
        nnz_lin[(size_t)bb] += h_rowptr[r + 1] - h_rowptr[r];
    }
    prev = 0;
    for (size_t k = 0; k < h_nlrows.size(); ++k) {
        const int64_t r = h_nlrows[k];
        if (h_rowptr[r + 1] == h_rowptr[r]) return kBlocksUnfit;
        const int bb = block_of_col(h_col[(size_t)h_rowptr[r]]);
        if (bb < prev || bb >= nb) return kBlocksUnfit;
        for (int64_t e = h_rowptr[r]; e < h_rowptr[r + 1]; ++e) if (block_of_col(h_col[(size_t)e]) != bb) return kBlocksUnfit;
        prev = bb;
        blk_nl[(size_t)bb + 1] += 1;
        nnz_nl[(size_t)bb] += h_rowptr[r + 1] - h_rowptr[r];
        if (h_rowkind[(size_t)r] == KTN_ROW_QUAD) {
            if (k > 0 && h_nlrows[k - 1] >= r) return kBlocksUnfit;           // (the launch list is in row order: so must the slots be)
            blk_qrow[(size_t)bb + 1] += 1;
            blk_qent[(size_t)bb + 1] += h_rowptr[r + 1] - h_rowptr[r];
        }
    }
    for (int bb = 0; bb < nb; ++bb) {
        blk_lin[(size_t)bb + 1] += blk_lin[(size_t)bb]; blk_nl[(size_t)bb + 1] += blk_nl[(size_t)bb];
        blk_qrow[(size_t)bb + 1] += blk_qrow[(size_t)bb]; blk_qent[(size_t)bb + 1] += blk_qent[(size_t)bb];
    }
    if (blk_qrow[(size_t)nb] != n_quad_nl || blk_qent[(size_t)nb] != n_quad_ent_nl) return kBlocksUnfit;
    // arenas
    std::vector<EcpArena> ar((size_t)nb);
    int64_t row_tot = 0, nnz_tot = 0;
    int mmax = 1;
    for (int bb = 0; bb < nb; ++bb) {
        const int64_t ml = blk_lin[(size_t)bb + 1] - blk_lin[(size_t)bb], mn = blk_nl[(size_t)bb + 1] - blk_nl[(size_t)bb];
        EcpArena a;
        a.row0 = row_tot; a.nnz0 = nnz_tot;
        a.cap_rows = (int32_t)(ml + (int64_t)cap_mul * mn);
        a.cap_nnz = (int32_t)(nnz_lin[(size_t)bb] + (int64_t)cap_mul * nnz_nl[(size_t)bb]);
        row_tot += a.cap_rows; nnz_tot += a.cap_nnz;
        mmax = std::max<int>(mmax, std::max<int>(a.cap_rows, (int)mn));
        ar[(size_t)bb] = a;
    }
    const size_t lds = (size_t)(3 * blk_nmax + 3 * mmax + (kEcpThreads / 64) * kEcpQ + kEcpQ + 8 + 16) * sizeof(double) +
                       (size_t)(std::max(blk_nmax, mmax) + 4) * sizeof(int32_t);
    if (lds > 158 * 1024 || blk_nmax > 65535 || mmax > 65535) return kBlocksUnfit;      // 16-bit local indices in the arenas
    t_start = std::chrono::steady_clock::now();
    // (a supporting launch needs a lambda per kept row: after a Kelley launch there is none, and the launch is the cold one)
    bool warm = want_warm && !(esh && !blocks_last_esh);
    for (int bb = 0; warm && bb < nb; ++bb)                 // the geometry the resident arenas were laid out with
        warm = ar[(size_t)bb].row0 == h_ar_row0[(size_t)bb] && ar[(size_t)bb].nnz0 == h_ar_nnz0[(size_t)bb] && ar[(size_t)bb].cap_rows == h_ar_rows[(size_t)bb];
    if (!warm) {
        d_ar.upload(ar, stream); d_blklin.upload(blk_lin, stream); d_blknl.upload(blk_nl, stream);
        e_rptr.resize((size_t)row_tot + nb + 1, stream);
        e_rcol.resize((size_t)nnz_tot + 1, stream); e_rval.resize((size_t)nnz_tot + 1, stream); e_rsval.resize((size_t)nnz_tot + 1, stream);
        e_crow.resize((size_t)nnz_tot + 1, stream); e_cval.resize((size_t)nnz_tot + 1, stream); e_csval.resize((size_t)nnz_tot + 1, stream);
        for (DBuf<double>* v : {&e_lo, &e_hi, &e_y, &e_dr, &e_loh, &e_hih}) v->resize((size_t)row_tot + 1, stream);
        e_cptr.resize((size_t)n_lp + nb + 1, stream);
        for (DBuf<double>* v : {&e_dc, &e_ch, &e_lh, &e_uh}) v->resize((size_t)n_lp + 1, stream);
        e_last.resize((size_t)std::max<int64_t>(m_nl, 1), stream);
        e_prev.resize((size_t)row_tot + 1, stream); e_ax.resize((size_t)row_tot + 1, stream);
        e_res.resize((size_t)nb * 8, stream);
        h_ar_row0.resize((size_t)nb); h_ar_nnz0.resize((size_t)nb); h_ar_rows.resize((size_t)nb);      // (ktn_blocks_get_cuts reads the arenas of this launch)
        for (int bb = 0; bb < nb; ++bb) { h_ar_row0[(size_t)bb] = ar[(size_t)bb].row0; h_ar_nnz0[(size_t)bb] = ar[(size_t)bb].nnz0; h_ar_rows[(size_t)bb] = ar[(size_t)bb].cap_rows; }
        h_blklin = blk_lin; h_blknl = blk_nl;
    }
    EcpWarm Wm{nullptr};
    if (warm) {
        blocks_rewarm();
        Wm.rec = e_rewarm.p;
    }
    const std::vector<double> rewarm_rec = warm ? h_rewarm : std::vector<double>();
    blocks_launched = false; blocks_last_esh = esh; blocks_warm_ok = false; blocks_rewarmed = false; blocks_cap_mul = cap_mul;
    EcpEsh E{};
    if (esh) {
        e_lam.resize((size_t)row_tot + 1, stream);
        e_res2.resize((size_t)nb * 4, stream);
        E.xint = d_xint.p; E.sig = d_esh_sig.p; E.jint = esh_n_quad_part > 0 ? d_jint.p : nullptr;
        E.lam = e_lam.p; E.res = e_res2.p;
        E.root_tol = prm.esh_root_tol; E.iters = prm.esh_root_iters;
    }
    EcpBatch B;
    B.blk_col = d_blkcol.p; B.blk_lin = d_blklin.p; B.blk_nl = d_blknl.p;
    B.lp_rowptr = lp_rowptr.p; B.lp_col = lp_col.p; B.lp_val = lp_val.p; B.lp_lo = lp_lo.p; B.lp_hi = lp_hi.p;
    B.c = lp_c.p; B.l = lp_l.p; B.u = lp_u.p;
    B.P = nlp_view(); B.nl_rows = d_nlrows.p;
    B.jac = d_jac.p; B.has_tape = n_tape_nl > 0 ? 1 : 0;      // every row owns its entries of the Jacobian buffer
    B.has_quad = n_quad_nl > 0 ? 1 : 0;
    B.quad_group = (dev.ecp_quad_group == 4 || dev.ecp_quad_group == 8 || dev.ecp_quad_group == 16 || dev.ecp_quad_group == 32 ||
                    dev.ecp_quad_group == 64) ? dev.ecp_quad_group : grp_quad;
    B.Q = QuadDev{d_qcol.p, d_qval.p, d_qptr.p, d_qjidx.p, d_qvterm.p};
    B.q_rows = d_qrows_nl.p; B.q_slots = d_qslots_nl.p; B.q_tbase = d_qtbase_nl.p;
    B.q_ent = n_quad_nl != n_quad ? d_qent_nl.p : nullptr;
    B.blk_qrow = nullptr; B.blk_qent = nullptr;
    if (B.has_quad) {
        d_blkqrow.upload(blk_qrow, stream); d_blkqent.upload(blk_qent, stream);
        B.blk_qrow = d_blkqrow.p; B.blk_qent = d_blkqent.p;
    }
    B.arena = d_ar.p;
    B.rptr = e_rptr.p; B.rcol = e_rcol.p; B.rval = e_rval.p; B.rsval = e_rsval.p; B.lo = e_lo.p; B.hi = e_hi.p; B.y = e_y.p; B.dr = e_dr.p;
    B.loh = e_loh.p; B.hih = e_hih.p;
    B.cptr = e_cptr.p; B.crow = e_crow.p; B.cval = e_cval.p; B.csval = e_csval.p;
    B.dc = e_dc.p; B.ch = e_ch.p; B.lh = e_lh.p; B.uh = e_uh.p;
    e_xbest.resize((size_t)n_lp + 1, stream);
    B.last_cut = e_last.p; B.cut_prev = e_prev.p; B.ax = e_ax.p; B.x = lp_x.p; B.xbest = e_xbest.p; B.res = e_res.p;
    B.cert_tol = prm.obj_cert_tol; B.polish_max_iter = prm.polish_max_iter;
    B.f_tol = prm.f_tol; B.cut_coef_rng = prm.cut_coef_rng; B.tol_scale = prm.lp_tol_scale; B.tol_floor = prm.lp_tol_floor;
    B.tol_cap = prm.lp_tol_cap; B.gap_floor = prm.lp_gap_floor; B.gap_cap = prm.lp_gap_cap; B.stag_factor = prm.lp_stag_factor;
    B.iter_cap = prm.iter_cap; B.lp_max_iter = prm.lp_max_iter; B.check_every = std::max(2, prm.lp_check_every);
    // (a lone workgroup's check is cheap and every instance stops on its own: a period of 24 halves the iterations of the
    //  slowest instance against 64 -- 512 x cfg5: max 15 842 -> 5 008, the launch 0.131 -> 0.097 s)
    B.check_every = std::min(B.check_every, 24);
    B.near_chunk = prm.lp_near_check; B.ruiz_iters = prm.lp_ruiz_iters; B.nmax = blk_nmax; B.mmax = mmax;
    B.power_passes = dev.ecp_power;
    // the loaded state: M == M_base rows (the linear rows), as after reset()
    if (warm) {
        // (the warm instantiations ask for their dynamic LDS at every launch: two more high-water marks would save a call per solve)
        if (esh) {
            KTN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ecp_blocks<1, EcpEsh, EcpWarm>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            launch(k_ecp_blocks<1, EcpEsh, EcpWarm>, (unsigned)nb, kEcpThreads, lds, stream, B, E, Wm);
        } else {
            KTN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ecp_blocks<0, EcpWarm>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            launch(k_ecp_blocks<0, EcpWarm>, (unsigned)nb, kEcpThreads, lds, stream, B, Wm);
        }
    } else if (esh) {
        if (lds > lds_set_ecp_esh) {
            KTN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ecp_blocks<1, EcpEsh>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            lds_set_ecp_esh = lds;
        }
        launch(k_ecp_blocks<1, EcpEsh>, (unsigned)nb, kEcpThreads, lds, stream, B, E);
    } else {
        if (lds > lds_set_ecp) {
            KTN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ecp_blocks<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            lds_set_ecp = lds;
        }
        launch(k_ecp_blocks<0>, (unsigned)nb, kEcpThreads, lds, stream, B);
    }
    check_launch();
    std::vector<double> res = e_res.to_host(stream);
    blocks_launched = true; blocks_warm_ok = true;
    h_blkres = res;
    ++kkt_solves; kkt_solved = true; kkt_arena = true; kkt_cached = false;      // (KKT report: multipliers and lists are the arenas' now)
    stats["ecp_blocks_esh_rows"] = 0.0;
    if (esh) {                                                  // the instances' counters: rows moved, fallback rows, passes, QUAD rows moved
        const std::vector<double> r2 = e_res2.to_host(stream);
        double c[4] = {0.0, 0.0, 0.0, 0.0};
        for (int bb = 0; bb < nb; ++bb) for (int k = 0; k < 4; ++k) c[k] += r2[(size_t)bb * 4 + k];
        stats["esh_rows"] += c[0]; stats["esh_fallback_rows"] += c[1]; stats["esh_newton_steps"] += c[2]; stats["esh_quad_rows"] += c[3];
        stats["ecp_blocks_esh_rows"] = c[0];
    }
    bool ok = true, screened_only = warm;                    // (screened_only: every instance that is not :Optimal was ended by the screen)
    int first_open = KTN_STATUS_OPTIMAL;
    double obj = 0.0, it_max = 0.0, cuts = 0.0, pd = 0.0, rows = 0.0;
    for (int bb = 0; bb < nb; ++bb) {
        const double* o = res.data() + (size_t)bb * 8;
        if ((int)o[0] != KTN_STATUS_OPTIMAL) {
            if (ok) first_open = (int)o[0];
            ok = false;
            if (!(warm && (int)rewarm_rec[(size_t)bb * 8] == 2)) screened_only = false;
        }
        obj += o[2]; it_max = std::max(it_max, o[1]); cuts += o[3]; pd += o[4]; rows += o[6];
    }
    if (dev.debug_blocks) {
        std::vector<std::pair<double, int>> v;
        for (int bb = 0; bb < nb; ++bb) v.push_back({res[(size_t)bb * 8 + 4], bb});
        std::sort(v.begin(), v.end());
        std::fprintf(stderr, "[ecp blocks] pdhg per instance: min %.0f median %.0f p90 %.0f p99 %.0f max %.0f (instance %d, %g ecp iterations, %g rows)\n",
                     v.front().first, v[v.size() / 2].first, v[v.size() * 9 / 10].first, v[v.size() * 99 / 100].first, v.back().first, v.back().second,
                     res[(size_t)v.back().second * 8 + 1], res[(size_t)v.back().second * 8 + 6]);
        for (int bb = 0; bb < nb; ++bb) {                       // what sends the batch to the host-driven loop
            const double* o = res.data() + (size_t)bb * 8;
            if ((int)o[0] != KTN_STATUS_OPTIMAL)
                std::fprintf(stderr, "[ecp blocks] instance %d not optimal: status %d, %g ecp iterations, %g pdhg iterations, %g rows, max violation %g%s\n",
                             bb, (int)o[0], o[1], o[4], o[6], o[5], o[7] != 0.0 ? ", arena overflow" : "");
        }
    }
    stats["ecp_blocks_launches"] += 1.0;
    if (warm) stats["ecp_blocks_warm_launches"] += 1.0;
    stats["ecp_blocks_pdhg_sum"] += pd;
    stats["ecp_blocks_rows"] = rows;
    stats["ecp_blocks_tape_rows"] = (double)n_tape_nl;
    stats["ecp_blocks_quad_rows"] = (double)n_quad_nl;
    screened_only = screened_only && !ok;
    if (!ok && !keep && !screened_only) { stats["ecp_blocks_fallbacks"] += 1.0; return kBlocksOpen; }
    status = ok ? KTN_STATUS_OPTIMAL : first_open; lp_status = KTN_STATUS_OPTIMAL;
    iter = (int64_t)it_max; numcuts = (int64_t)cuts; objval = obj + c0; allsat = ok;
    soltime = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    return ok ? kBlocksDone : (screened_only ? kBlocksScreened : kBlocksOpen);
}

// ktn_blocks_get_cuts: the cut rows of instance `block` in the arenas of the last device launch
void Engine::blocks_cuts(int64_t block, std::vector<int64_t>& rowptr, std::vector<int32_t>& col, std::vector<double>& val,
                         std::vector<double>& lo, std::vector<double>& hi, std::vector<int64_t>& slot, std::vector<double>& lam) {
    struct { int64_t row0, nnz0, cap_rows; } a{h_ar_row0[(size_t)block], h_ar_nnz0[(size_t)block], h_ar_rows[(size_t)block]};
    const int64_t c0 = h_blkcol[(size_t)block];
    const int64_t m_lin = h_blklin[(size_t)block + 1] - h_blklin[(size_t)block];
    const int64_t nl0 = h_blknl[(size_t)block], m_nl = h_blknl[(size_t)block + 1] - nl0;
    const int64_t Mb = std::min<int64_t>((int64_t)h_blkres[(size_t)block * 8 + 6], a.cap_rows);
    const int64_t nc = std::max<int64_t>(Mb - m_lin, 0);
    rowptr.assign((size_t)nc + 1, 0); lo.assign((size_t)nc, 0.0); hi.assign((size_t)nc, 0.0); slot.assign((size_t)nc, -1); lam.assign((size_t)nc, 1.0);
    col.clear(); val.clear();
    if (nc == 0) return;
    std::vector<int32_t> rp((size_t)nc + 1), prev((size_t)nc), last((size_t)std::max<int64_t>(m_nl, 1), -1);
    auto fetch = [&](auto* host, const auto* devp, size_t count) {
        if (count) KTN_HIP(hipMemcpyAsync(host, devp, count * sizeof(*host), hipMemcpyDeviceToHost, stream));
    };
    fetch(rp.data(), e_rptr.p + (a.row0 + block + m_lin), rp.size());
    fetch(lo.data(), e_lo.p + (a.row0 + m_lin), (size_t)nc);
    fetch(hi.data(), e_hi.p + (a.row0 + m_lin), (size_t)nc);
    fetch(prev.data(), e_prev.p + (a.row0 + m_lin), (size_t)nc);
    if (m_nl > 0) fetch(last.data(), e_last.p + nl0, (size_t)m_nl);
    if (blocks_last_esh) fetch(lam.data(), e_lam.p + (a.row0 + m_lin), (size_t)nc);
    sync();
    const int64_t e0 = rp[0], ne = rp[(size_t)nc] - e0;
    std::vector<uint16_t> lc((size_t)std::max<int64_t>(ne, 1));
    val.assign((size_t)ne, 0.0); col.assign((size_t)ne, 0);
    if (ne > 0) {
        fetch(lc.data(), e_rcol.p + (a.nnz0 + e0), (size_t)ne);
        fetch(val.data(), e_rval.p + (a.nnz0 + e0), (size_t)ne);
        sync();
    }
    for (int64_t k = 0; k <= nc; ++k) rowptr[(size_t)k] = rp[(size_t)k] - e0;
    for (int64_t k = 0; k < ne; ++k) col[(size_t)k] = (int32_t)(c0 + lc[(size_t)k]);
    // the NL slot of every cut: walk each slot's list (newest first) through last_cut / cut_prev
    for (int64_t i = 0; i < m_nl; ++i)
        for (int32_t r = last[(size_t)i]; r >= m_lin && r < Mb; r = prev[(size_t)(r - m_lin)]) slot[(size_t)(r - m_lin)] = nl0 + i;
}

// boundroutine  src/model.jl:175-197 with the ray in d_ray
void Engine::boundroutine() {
    for (int nn = 2; nn <= 1023; ++nn) {
        const double s = std::ldexp(1.0, nn);
        launch_n(k_axpy_scaled, n_lp, stream, n_lp, d_ray.p, s, d_xs.p);
        int64_t nviol = 0;
        double mv = 0.0;
        bool nonfin = false;
        global_sweep(d_xs.p, prm.f_tol, &nviol, &mv, &nonfin);
        if (nonfin) { status = KTN_STATUS_ERROR; return; }
        if (nviol > 0) break;   // !allsat -> stop searching in this direction
    }
}

void Engine::begin() {
    KTN_REQUIRE(loaded, "optimize! before loadproblem!");
    blocks_drop_warm();               // (x is the host loop's from here on: a later KTN_BLOCKS_WARM launch starts cold)
    t_start = std::chrono::steady_clock::now();
    begun = true;
    lp_status = KTN_STATUS_OPTIMAL;
    if (status == KTN_STATUS_ERROR) return;
    screened_out = false;
    if (screen_pending) {      // once per ktn_set_var_bounds: the pool's rows against the new box (rebound.hip)
        screen_pending = false;
        screened_out = screen();
        if (screened_out) { lp_status = KTN_STATUS_INFEASIBLE; status = KTN_STATUS_INFEASIBLE; return; }
    }
    if (reopened) stats["warm_solves"] += 1.0;
    if (esh_mode() && !esh_ready) esh_prepare();      // x_int, once per loaded problem (esh.hip)
    if (has_inf_bound) {       // presolve: resolve an initially-unbounded LP  model.jl:228-247
        int64_t i = 0;
        bool unb = recession_ray();
        if (unb) std::fprintf(stderr, "WARNING: Automatically bounding unbounded LP\n");     // model.jl:229-231
        while (unb && i < n_lp) {
            if (prm.log_level > 0) {                                                          // model.jl:237
                std::vector<double> ray = d_ray.to_host(stream);
                std::printf("Unbounded ray along: [");
                for (int64_t j = 0; j < n_lp; ++j) std::printf(j ? ",%g" : "%g", ray[(size_t)j]);
                std::printf("]\n");
            }
            boundroutine();
            if (status == KTN_STATUS_ERROR) return;
            unb = recession_ray();
            ++i;
        }
        if (unb) {
            std::fprintf(stderr, "WARNING: Katana could not resolve unbounded LP\n");         // model.jl:244-247
            lp_status = KTN_STATUS_UNBOUNDED; status = KTN_STATUS_UNBOUNDED;
            return;
        }
    }
    if (logging()) { print_header(); std::fflush(stdout); }                                   // model.jl:249-251
}

void Engine::step(int32_t* done) {
    KTN_REQUIRE(begun, "ktn_ecp_step before ktn_optimize_begin");
    *done = 1;
    if (status == KTN_STATUS_ERROR || status == KTN_STATUS_UNBOUNDED || screened_out) return;
    if (polishing) { polish_step(done); return; }
    if (allsat || iter >= prm.iter_cap) return;          // while !allsat && m.iter < iter_cap  model.jl:257
    iter += 1;
    const double floor_p = prm.lp_tol_floor * prm.f_tol;
    double tol_p = std::min(std::max(prm.lp_tol_scale * last_maxviol, floor_p), prm.lp_tol_cap);
    if (m_nl_global == 0) tol_p = floor_p;      // pure LP: one exact solve, like the reference (row-sharded: NL rows of ALL ranks)
    double tol_g = std::min(std::max(tol_p, prm.lp_gap_floor), prm.lp_gap_cap);
    LpResult R = lp_solve(tol_p, tol_g, 0);
    lp_status = R.status;
    int64_t nviol = 0;
    double mv = 0.0, ex_not_floor = 0.0, ex_obj = objval;
    if (R.status != KTN_STATUS_OPTIMAL) {                                // model.jl:261-263
        // (NL-row blocks: a rank whose LP failed still takes part in this iteration's exchange -- its flag makes every rank leave)
        if (exchanging()) (void)sweep_all(lp_x.p, prm.f_tol, false, R.status, &nviol, &mv, &ex_not_floor, &ex_obj);
        status = R.status;
        return;
    }
    if (prm.vis_data) lp_sols.push_back(lp_x.to_host(stream));          // model.jl:267
    // (NL-row blocks: every rank holds the identical LP, so the purge is identical too)
    if (prm.purge_age > 0 && !prm.vis_data && (!sharded_rows || exchanging()) && M - M_base >= std::max<int64_t>(prm.purge_min_rows, 1)) purge_cuts();
    const double floor_p0 = prm.lp_tol_floor * prm.f_tol, floor_g0 = std::min(std::max(floor_p0, prm.lp_gap_floor), prm.lp_gap_cap);
    ex_not_floor = (R.row_viol <= floor_p0 && R.dres_rel <= floor_g0 &&
                    (R.gap <= floor_g0 || (R.stag_exit && prm.lp_stag_factor > 0.0 && R.gap <= prm.lp_stag_factor * floor_g0))) ? 0.0 : 1.0;
    if (sweep_all(lp_x.p, prm.f_tol, true, R.status, &nviol, &mv, &ex_not_floor, &ex_obj)) return;      // model.jl:268-283 (true: status set, leave)
    last_maxviol = mv;
    stats["last_maxviol"] = mv; stats["last_nviol"] = (double)nviol;
    const bool sat_now = (nviol == 0);
    // inexact-LP rule (DESIGN.md "LP tolerance schedule"): all rows satisfied only counts once
    // the LP itself was solved to the floor tolerance -- by request, or because the last check of a looser solve
    // happens to meet the floor tolerances already (then the re-solve would return this very point)
    const double floor_g = std::min(std::max(floor_p, prm.lp_gap_floor), prm.lp_gap_cap);
    // (... or ended through the stagnation exit with a gap the floor-tolerance solve would accept through that same exit: it
    //  would return after its first two checks with this very point -- 34 iterations and a setup on cfg3)
    (void)floor_g;
    const bool at_floor = ex_not_floor == 0.0;          // (NL-row blocks: the ranks' verdicts agree; taken from the exchange all the same)
    if (sat_now && !R.exact && tol_p > floor_p * (1.0 + 1e-12) && !at_floor) last_maxviol = 0.0;
    else { allsat = sat_now; if (sat_now && tol_p > floor_p * (1.0 + 1e-12) && !R.exact) stats["floor_resolves_skipped"] += 1.0; }
    const double obj = objval;                                           // model.jl:287-289
    const double obj_delta = std::fabs((obj_prev - obj) / obj);
    obj_prev = obj;
    log_max_viol = std::max(log_max_viol, nviol);                        // model.jl:284-285
    log_cuts_lastprnt += last_sweep_cuts;
    if (logging()) {                                                     // model.jl:291-303
        const int64_t r = iter % prm.log_level;
        if (r == 0) {
            if (iter % ((int64_t)prm.log_level * 50) == 0) print_header();
            print_stats(prm.log_level);
            log_cuts_lastprnt = 0;
            log_max_viol = 0;
        } else if (allsat) {
            print_stats(r);                                              // print on last iteration also
        } else if (obj_delta <= prm.obj_eps) {
            print_stats(iter);
        }
    }
    const bool eps_stop = obj_delta <= prm.obj_eps;
    if (eps_stop) { allsat = true; }                                     // model.jl:306-308 (break)
    *done = (allsat || iter >= prm.iter_cap) ? 1 : 0;
    // Terminal refinement of small problems: the reference's simplex vertices end Kelley's method with the last
    // violation far below f_tol (its tests ask the objective to 1e-6 / 1e-7); a first-order LP ends AT f_tol.
    bool refine = false;
    // (row-sharded LP: every rank holds the cut lists of its own NL rows, so the certificate is the all-reduced sum of the ranks'
    //  shares and every decision below is taken from all-reduced numbers: all ranks refine, or none)
    if (allsat && !eps_stop && !polish_done && (!sharded_rows || exchanging()) && prm.polish_max_iter > 0 && (m_nl_global > 0 || exchanging())) {
        if (n_lp <= prm.polish_max_var && !row_sharded()) {
            refine = prm.polish_factor > 0.0 && prm.polish_factor < 1.0;
            polish_phi = prm.polish_factor;
            cert_target = 0.0;
        } else if (prm.obj_cert_tol > 0.0 && lists_ok()) {
            // Larger problems: refine only while the multiplier-weighted residual of the NL rows (the part of  f* - objective  the
            // stop rule leaves open; the LP's own accuracy is its gap tolerance) exceeds half the objective tolerance.
            // (A fused batch -- ktn_set_blocks -- owes the tolerance to EVERY instance: D is then the largest per-instance
            //  certificate in units of that instance's target, and the target is 1.)
            const double target = n_blocks > 0 ? 1.0 : prm.obj_cert_tol * std::max(1.0, std::fabs(ex_obj));
            cert_gap = 0.25 * target / (1.0 + 2.0 * std::fabs(ex_obj));
            const double D = n_blocks > 0 ? certificate_blocks(&cert_gap) : certificate_all_ranks();
            stats["cert_evals"] += 1.0;
            stats["cert_last"] = D;
            if (D > 0.5 * target) {
                refine = true;
                cert_target = target;
                polish_phi = std::min(std::max(0.25 * target / D, 0.05), 0.5);
                stats["cert_refinements"] += 1.0;
            }
        }
    }
    if (refine) {
        polishing = true;
        polish_count = 0;
        best_viol = kInf;
        d_xbest.resize((size_t)n_lp, stream);
        // The point that met the stop rule is a candidate for the answer; its largest violation among ALL rows (the
        // sweep above only measured rows beyond f_tol, i.e. none) comes from a sweep at the polish tolerance below.
        *done = 0;
    }
}

// One pass of the terminal refinement: LP at the polish tolerance, cuts for every row beyond polish_factor * f_tol.
// Ends when no such row is left, or after polish_max_iter passes; the answer is then the point with the smallest violation
// among those that satisfy the reference's stop rule (every row within f_tol).
void Engine::polish_step(int32_t* done) {
    const double f_eff = polish_phi * prm.f_tol;
    int64_t nviol = 0;
    double mv = 0.0;
    auto consider = [&](double viol) {           // lp_x / objval hold a point whose largest violation is `viol` (<= f_tol)
        if (viol <= prm.f_tol && viol < best_viol) {
            best_viol = viol;
            best_obj = objval;
            KTN_HIP(hipMemcpyAsync(d_xbest.p, lp_x.p, (size_t)n_lp * sizeof(double), hipMemcpyDeviceToDevice, stream));
        }
    };
    auto finish = [&]() {
        if (best_viol < kInf) {
            KTN_HIP(hipMemcpyAsync(lp_x.p, d_xbest.p, (size_t)n_lp * sizeof(double), hipMemcpyDeviceToDevice, stream));
            objval = best_obj;
            sync();
        }
        polishing = false;
        polish_done = true;
        *done = 1;
    };
    *done = 0;
    double ex0 = 0.0, ex1 = 0.0;
    if (polish_count == 0) {
        // first pass: measure (and cut at) the point that met the stop rule
        if (sweep_all(lp_x.p, f_eff, true, KTN_STATUS_OPTIMAL, &nviol, &mv, &ex0, &ex1)) { polishing = false; *done = 1; return; }
        consider(mv);
        polish_count = 1;
        if (nviol == 0 && cert_target <= 0.0) finish();     // (certificate mode: the LP itself may be what is short -- solve it tighter)
        return;
    }
    if (polish_count > prm.polish_max_iter) { finish(); return; }
    ++polish_count;
    stats["polish_iters"] += 1.0;
    const double tol_p = prm.lp_tol_floor * f_eff;
    // gap tolerance of a refinement solve: scaled with the cut tolerance (small problems); in certificate mode a quarter of the
    // objective tolerance, as a relative gap
    const double tol_g = cert_target > 0.0 ? std::min(std::min(std::max(tol_p, prm.lp_gap_floor), prm.lp_gap_cap), cert_gap)
                                           : std::max(prm.lp_gap_floor * polish_phi, 1e-12);
    LpResult R = lp_solve(tol_p, tol_g, 0);
    if (R.status != KTN_STATUS_OPTIMAL) {                                // keep the point that met the stop rule
        // (NL-row blocks: the exchange of this pass still takes place, so that no rank waits in a collective the others left)
        if (exchanging()) { const int keep = status; (void)sweep_all(lp_x.p, f_eff, false, R.status, &nviol, &mv, &ex0, &ex1); status = keep; }
        finish();
        return;
    }
    { const int keep = status; if (sweep_all(lp_x.p, f_eff, true, KTN_STATUS_OPTIMAL, &nviol, &mv, &ex0, &ex1)) { status = keep; finish(); return; } }
    consider(mv);
    if (cert_target > 0.0 && mv <= prm.f_tol) {                          // certificate mode: done as soon as the bound holds
        double gap_now = 0.0;
        const double D = n_blocks > 0 ? certificate_blocks(&gap_now) : certificate_all_ranks();
        stats["cert_evals"] += 1.0;
        stats["cert_last"] = D;
        if (D <= 0.5 * cert_target) { finish(); return; }
    }
    if (nviol == 0) finish();
}

// max(sum_i lambda_i res_i, 0) over the NL rows at (lp_x, lp_y), with g of the last sweep (kernels.hpp "objective certificate")
// (id_offset: the global id of this handle's first NL row when the cut lists are global -- NL-row blocks over several GPUs;
//  raw: the signed sum, for the caller to add up over the ranks before clamping)
double Engine::objective_certificate(int64_t id_offset, bool raw) {
    if (m_nl <= 0) return 0.0;
    d_cert.resize((size_t)m_nl, stream);
    launch_n(k_cert_nl, m_nl, stream, m_nl, d_nlrows.p, list_heads() + id_offset, d_cutprev.p, lp_y.p, d_g.p, d_lb.p, d_ub.p, prm.f_tol, d_cert.p);
    launch(k_sum_partial, kRedBlocks, kBlock, 0, stream, m_nl, d_cert.p, partials.p);
    launch(k_sum_final, 1, kRedBlocks, 0, stream, partials.p, kRedBlocks, d_scal.p);
    check_launch();
    double D = 0.0;
    KTN_HIP(hipMemcpyAsync(&D, d_scal.p, sizeof(double), hipMemcpyDeviceToHost, stream));
    sync();
    if (raw) return D;
    return (D == D) ? std::max(D, 0.0) : kInf;
}

// Fused batch: the largest per-instance certificate over that instance's own target (k_cert_blocks); *gap_tol = a quarter of the
// smallest per-instance (target / (1 + 2 |objective|)): the relative gap the refinement's LP solves are asked for
double Engine::certificate_blocks(double* gap_tol) {
    if (m_nl <= 0 || n_blocks <= 0) return 0.0;
    d_cert.resize((size_t)m_nl, stream);
    launch_n(k_cert_nl, m_nl, stream, m_nl, d_nlrows.p, list_heads(), d_cutprev.p, lp_y.p, d_g.p, d_lb.p, d_ub.p, prm.f_tol, d_cert.p);
    d_certblk.resize((size_t)(2 * n_blocks), stream);
    launch(k_cert_blocks, (unsigned)n_blocks, kBlock, 0, stream, m_nl, d_nlrows.p, d_rowptr.p, d_col.p, d_cert.p, d_blkcol.p, n_blocks, lp_c.p, lp_x.p,
           prm.obj_cert_tol, d_certblk.p);
    check_launch();
    std::vector<double> h = d_certblk.to_host(stream);
    double worst = 0.0, gap = kInf;
    for (int64_t b = 0; b < n_blocks; ++b) {
        const double r = h[(size_t)b];
        worst = (r == r) ? std::max(worst, r) : kInf;
        gap = std::min(gap, h[(size_t)(n_blocks + b)]);
    }
    if (gap_tol) *gap_tol = 0.25 * gap;
    return worst;
}

// The certificate of a solve whose NL rows (and their cut lists) are spread over the ranks of a row-sharded LP: the signed shares
// add up, the sum is clamped -- every rank gets the same number
// The stop rule's sweep in whichever form the handle runs: alone (sweep), row-sharded LP (all-reduced counts), or NL-row blocks
// with a replicated LP -- then this rank sweeps its block, the callback moves every rank's new rows into every rank's LP in rank
// order and returns the totals and the maxima of the flags.  Returns true when the loop has to end (status is set).
bool Engine::sweep_all(const double* d_x, double f_cut, bool lp_ok, int lp_stat, int64_t* nviol, double* maxviol, double* extra0, double* extra1) {
    bool nonfin = false;
    if (!exchanging()) {
        global_sweep(d_x, f_cut, nviol, maxviol, &nonfin);
        if (nonfin) { status = KTN_STATUS_ERROR; return true; }
        return false;
    }
    const int64_t m0 = M;
    int64_t nv = 0;
    double mv = 0.0;
    if (lp_ok) sweep(d_x, f_cut, &nv, &mv, &nonfin);
    double sc[5] = {0.0, mv, (lp_ok ? 0.0 : 2.0) + (nonfin ? 1.0 : 0.0), *extra0, *extra1};
    if (exch_cb(exch_user, 0, m0, sc, 5) != 0) throw Error(KTN_E_CALLBACK, "cut-exchange callback failed");
    *nviol = (int64_t)(sc[0] + 0.5);
    *maxviol = sc[1];
    *extra0 = sc[3]; *extra1 = sc[4];
    if (sc[2] >= 2.0) { status = lp_ok ? KTN_STATUS_ERROR : lp_stat; return true; }     // some rank's LP failed
    if (sc[2] >= 1.0) { status = KTN_STATUS_ERROR; return true; }                        // some rank's sweep met a non-finite cut
    return false;
}

double Engine::certificate_all_ranks() {
    if (exchanging()) {                                  // NL-row blocks: the ranks' shares through the callback (sum)
        double D = objective_certificate(exch_lo, true);
        if (!(D == D)) D = kInf;
        if (exch_cb(exch_user, 1, 0, &D, 1) != 0) throw Error(KTN_E_CALLBACK, "cut-exchange callback failed");
        return (D == D) ? std::max(D, 0.0) : kInf;
    }
    if (!row_sharded()) return objective_certificate();
    double D = objective_certificate(0, true);
    if (!(D == D)) D = kInf;
    allreduce_host(&D, 1, 0);
    return (D == D) ? std::max(D, 0.0) : kInf;
}

void Engine::end() {
    soltime = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();   // model.jl:311
    if (status == KTN_STATUS_ERROR || status == KTN_STATUS_UNBOUNDED) return;
    if (lp_status != KTN_STATUS_OPTIMAL) { status = lp_status; return; }
    status = (iter >= prm.iter_cap) ? KTN_STATUS_USERLIMIT : KTN_STATUS_OPTIMAL;                   // model.jl:313-317
}

}  // namespace ktn
