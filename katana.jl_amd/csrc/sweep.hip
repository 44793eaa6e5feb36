// sweep.hip -- the separator sweep (src/separators.jl:85-135, src/model.jl:272-283), the host-evaluator rows and the KKT report  (struct Engine: engine.hpp)
#include "engine.hpp"
#include "launch.hpp"
#include "kernels.hpp"
#include "tape_classes.hpp"
#include "quad_rows.hpp"
#include "kkt.hpp"

namespace ktn {

// KTN_ROW_HOST: the caller's evaluator computes g and J of those rows at x (one call per sweep, like the reference's
// precompute!, src/separators.jl:111-116); the values are staged to the device, everything downstream is unchanged.
void Engine::host_eval(const double* d_x) {
    const int64_t nx = std::min<int64_t>(n_lp > 0 ? n_lp : n0, n0 + 1);
    KTN_HIP(hipMemcpyAsync(h_xh.data(), d_x, (size_t)nx * sizeof(double), hipMemcpyDeviceToHost, stream));
    sync();
    if (host_constr_rows) {
        const int rc = cb_rows(cb_user, h_xh.data(), h_gh.data(), h_jh.data());
        if (rc != 0) throw Error(KTN_E_CALLBACK, "eval_rows callback failed (" + std::to_string(rc) + ")");
    }
    if (host_obj) {
        double f = 0.0;
        double* grad = h_jh.data() + h_rowptr[m0];
        const int rc = cb_obj(cb_user, h_xh.data(), &f, grad);
        if (rc != 0) throw Error(KTN_E_CALLBACK, "eval_obj callback failed (" + std::to_string(rc) + ")");
        const double t = (nx > n0) ? h_xh[(size_t)n0] : 0.0;
        h_gh[(size_t)m0] = f - t;                       // f(x) - t, src/nlpeval.jl:45
        grad[n0] = -1.0;                                // src/nlpeval.jl:62
    }
    d_gh.upload(h_gh.data(), (size_t)m_ext, stream);
    d_jh.upload(h_jh.data(), (size_t)nnz_ext, stream);
    NlpDev P = nlp_view();
    SweepOut O = sweep_view();
    launch_n(k_host_scatter, n_host, stream, P, d_hostrows.p, n_host, d_gh.p, d_jh.p, O);
    check_launch();
    stats["host_evals"] += 1.0;
}

// k_tape_classed over the classes of NL rows (the sweep; mslot: NL slots) or over all classes (precompute_all; mslot: rows)
void Engine::launch_tape_classed(bool nl_only, const int32_t* mslot, const double* d_x, double f_tol) {
    if (tc_launches.empty()) return;
    if (!tc_lds_set) {
        KTN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tape_classed), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(kTapeClassMaxCells * kTapeClassWave * sizeof(double))));
        tc_lds_set = true;
    }
    NlpDev P = nlp_view();
    SweepOut O = sweep_view();
    for (const TcLaunch& q : tc_launches) {
        if (nl_only && !q.nl) continue;
        TapeClassDev T = tape_class_view();
        T.wave_cls += q.wave0; T.wave_first += q.wave0;
        launch(k_tape_classed, (unsigned)q.nwaves, kTapeClassWave, q.lds, stream, P, T, mslot, d_x, f_tol, O);
    }
}

TapeClassDev Engine::tape_class_view() {
    TapeClassDev T;
    T.wave_cls = d_tc_wavecls.p; T.wave_first = d_tc_wavefirst.p; T.meta = d_tc_meta.p;
    T.prog_op = d_tc_op.p; T.prog_a = d_tc_a.p; T.prog_b = d_tc_b.p; T.prog_c = d_tc_c.p;
    T.cst = d_tc_cst.p; T.scol = d_tc_scol.p; T.mrow = d_tc_mrow.p;
    return T;
}

// k_quad_jac + k_quad_stats over the QUAD rows among the NL rows (the sweep: flags by NL slot) or over all of them (precompute_all)
void Engine::launch_quad(bool nl_only, const double* d_x, double f_tol) {
    const int64_t nr = nl_only ? n_quad_nl : n_quad, ne = nl_only ? n_quad_ent_nl : n_quad_ent;
    if (nr == 0) return;
    NlpDev P = nlp_view();
    SweepOut O = sweep_view();
    QuadDev Q{d_qcol.p, d_qval.p, d_qptr.p, d_qjidx.p, d_qvterm.p};
    QuadList L;
    L.rows = nl_only ? d_qrows_nl.p : d_qrows_all.p;
    L.slots = nl_only ? d_qslots_nl.p : d_qslots_all.p;
    L.tbase = nl_only ? d_qtbase_nl.p : d_qtbase_all.p;
    L.ent = (nl_only && n_quad_nl != n_quad) ? d_qent_nl.p : nullptr;
    L.n_rows = nr; L.n_ent = ne;
    size_t ta = 0, tb = 0;
    const bool ev = prm.profile && nl_only;
    if (ev) { ta = ev_get(); tb = ev_get(); KTN_HIP(hipEventRecord(ev_pool[ta], stream)); }
    with_group(grp_quad, [&](auto g) { launch(k_quad_jac<g()>, group_grid(ne, g()), kBlock, 0, stream, P, Q, L, d_x, O); });
    with_group(grp_quad_rows, [&](auto g) { launch(k_quad_stats<g()>, group_grid(nr, g()), kBlock, 0, stream, P, Q, L, d_x, f_tol, nl_only ? 1 : 0, O); });
    if (ev) { KTN_HIP(hipEventRecord(ev_pool[tb], stream)); ev_recs.push_back({5, ta, tb, quad_bytes}); }
}

NlpDev Engine::nlp_view() {
    NlpDev P;
    P.rowptr = d_rowptr.p; P.col = d_col.p; P.colk = d_colk.p; P.pp = d_pp.p;
    P.rconst = d_rconst.p; P.row_kind = d_rowkind.p; P.pad_zero = d_padzero.p; P.lb = d_lb.p; P.ub = d_ub.p;
    P.node_ptr = d_nodeptr.p; P.node_op = d_nodeop.p; P.node_a = d_nodea.p; P.node_b = d_nodeb.p;
    P.node_c = d_nodec.p; P.node_val = d_nodeval.p; P.node_adj = d_nodeadj.p;
    return P;
}

SweepOut Engine::sweep_view() {
    SweepOut O;
    O.g = d_g.p; O.jac = d_jac.p; O.bconst = d_bconst.p; O.maxc = d_maxc.p; O.nonfin = d_nonfin.p;
    O.flag = d_flag.p; O.cnt = d_cnt.p; O.maxviol = d_scal.p; O.any_nonfin = d_anynf.p;
    return O;
}

// ================================================================ separator =====
// precompute! for every row of the extended structure (jac materialised)
void Engine::precompute_all(const double* d_x) {
    NlpDev P = nlp_view();
    SweepOut O = sweep_view();
    // many short rows: the R-rows-per-lane-group form of the sweep with the Jacobian store (same sums, same bits); the
    // selection is the sweep's, made once in loadproblem (pre_multirow)
    if (pre_multirow) {
        with_value<8, 16, 32, 64>(grp_sweep, [&](auto g) {            // (grp_sweep >= 8: loadproblem)
            launch(k_sep_sweep<g(), 4, true>, group_grid(m_ext, g(), 4), kBlock, 0, stream, P, d_allrows.p, m_ext, d_x, 0.0, O);
        });
    } else {
        with_group(grp_sweep, [&](auto g) { launch(k_sep_eval<g()>, group_grid(m_ext, g()), kBlock, 0, stream, P, d_allrows.p, m_ext, d_x, 0.0, 1, 0, O); });
    }
    if (n_longev > 0)
        launch(k_sep_eval_long, (unsigned)n_longev, 1024, 0, stream, P, d_longev_rows.p, d_longev_slots.p, d_x, 0.0, 0, O);
    launch_quad(false, d_x, 0.0);
    launch_n(k_tape_eval, (int64_t)d_tapeint_all.n, stream, P, d_tapeint_all.p, (int64_t)d_tapeint_all.n, d_x, O);
    if (n_host > 0) host_eval(d_x);
    // cut constants / maxima of tape rows from the materialised Jacobian (flags unused here)
    KTN_HIP(hipMemsetAsync(d_scal.p, 0, sizeof(double), stream));
    KTN_HIP(hipMemsetAsync(d_anynf.p, 0, sizeof(int32_t), stream));
    // rows of the classed shapes: value, Jacobian and those constants / maxima in one pass (flags by row, as k_gj_stats' here)
    launch_tape_classed(false, d_tc_mrow.p, d_x, 0.0);
    if (tc_rows == 0 || d_tapeint_all.n > 0 || n_host > 0)
        launch_n(k_gj_stats, m_ext, stream, P, d_allrows.p, m_ext, d_x, 0.0, (int)KTN_ROW_TAPE, (const uint8_t*)(tc_rows > 0 ? d_tc_rowflag.p : nullptr), O);
    check_launch();
}

// ================================================================ KKT report (kkt.hpp) =====
// Column mirror of the extended structure (rows 0 .. m0, the objective row last; columns 0 .. n0), by the radix sort the LP's
// mirror uses: keys (col << 32 | row) in CSR order (k_kkt_keys: a thread per entry), a stable sort on the column bits gives row-ordered columns.  Built on the
// first getter after ktn_loadproblem, never changed until the next one.
void Engine::kkt_build_mirror() {
    if (kkt_mirror) return;
    if (nnz_ext >= ((int64_t)1 << 32)) throw Error(KTN_E_UNSUPPORTED, "KKT report: 2^32 Jacobian entries and more are not mirrored");
    const int64_t nc = n0 + 1;
    d_kkt_cptr.resize((size_t)nc + 1, stream);
    d_kkt_crow.resize((size_t)nnz_ext + 1, stream); d_kkt_cperm.resize((size_t)nnz_ext + 1, stream);
    DBuf<int64_t> cnt;
    DBuf<uint64_t> kin, kout;
    DBuf<uint32_t> pin, pout;
    DBuf<char> tmp;
    cnt.resize((size_t)nc + 1, stream); cnt.zero(stream);
    if (nnz_ext > 0) {
        kin.resize((size_t)nnz_ext, stream); kout.resize((size_t)nnz_ext, stream);
        pin.resize((size_t)nnz_ext, stream); pout.resize((size_t)nnz_ext, stream);
        launch_n(k_kkt_keys, nnz_ext, stream, nnz_ext, m_ext, d_rowptr.p, d_col.p, kin.p, pin.p, cnt.p);
        check_launch();
    }
    exclusive_scan(cnt.p, d_kkt_cptr.p, (size_t)nc + 1);
    if (nnz_ext > 0) {
        int bits = 1;
        while (((int64_t)1 << bits) < nc + 1 && bits < 31) ++bits;
        const size_t need = sort_pairs_temp_bytes((size_t)nnz_ext);
        tmp.resize(need + 16, stream);
        KTN_HIP(sort_pairs_u64_u32(tmp.p, need, kin.p, kout.p, pin.p, pout.p, (size_t)nnz_ext, 32, 32 + bits, stream));
        launch_n(k_csc_rows_perm, nnz_ext, stream, nnz_ext, kout.p, pout.p, d_kkt_crow.p, d_kkt_cperm.p);
        check_launch();
    }
    sync();                                             // the temporaries are freed on leaving the scope
    kkt_mirror = true;
    stats["kkt_mirror_bytes"] = 8.0 * (double)(nc + 1) + 8.0 * (double)nnz_ext;
}

void Engine::kkt_compute() {
    KTN_REQUIRE(loaded, "KKT report: no problem loaded");
    if (kkt_foreign())
        throw Error(KTN_E_UNSUPPORTED, "KKT report: a row-sharded handle or one with a cut exchange owns only a part of the cut lists");
    KTN_REQUIRE(kkt_solved, "KKT report: no LP solve since the problem was loaded or reset, or since rows were appended, truncated or purged");
    if (!kkt_arena && !lists_ok())
        throw Error(KTN_E_UNSUPPORTED, "KKT report: rows were appended from the host without cut lists (ktn_lp_enable_global_lists)");
    if (kkt_cached && kkt_key_version == lp_version && kkt_key_solves == kkt_solves) return;
    kkt_cached = false;
    kkt_build_mirror();
    const double sgn = (sense == KTN_MAX) ? -1.0 : 1.0;
    const size_t mm = (size_t)std::max<int64_t>(m_ext, 1);
    d_kkt_d.resize(mm, stream); d_kkt_z.resize((size_t)n0 + 1, stream); d_kkt_t.resize((size_t)(m0 + n0) + 1, stream);
    d_kkt_out.resize(8, stream);
    // ---- 1. constraint duals
    KktSrc S{};
    KTN_HIP(hipMemsetAsync(d_kkt_out.p + 4, 0, 2 * sizeof(double), stream));      // k_row_duals: entries zeroed on an infinite side, their largest
    const bool epi = !obj_linear && !kkt_arena;
    if (kkt_arena) {
        S.y = e_y.p; S.a_last = e_last.p; S.a_prev = e_prev.p; S.arena = d_ar.p;
        S.blk_lin = d_blklin.p; S.blk_nl = d_blknl.p; S.nb = (int64_t)h_ar_row0.size();
        launch_n(k_row_duals<true>, m0, stream, m0, d_kkt_rowmap.p, S, sgn, (int64_t)0, (int64_t)0, (int64_t)-1, (double*)nullptr, (const double*)d_lb.p, (const double*)d_ub.p, (double*)nullptr, d_kkt_d.p);
    } else {
        // what ktn_lp_get_duals returns: the true-cost multipliers of an exact mid-size solve while they stand, lp_y otherwise
        S.y = (!dev.raw_duals && mid_true_duals(nullptr)) ? md_y.p : lp_y.p;
        S.heads = list_heads(); S.prev = d_cutprev.p; S.n_heads = list_count(); S.n_rows = M;
        launch_n(k_row_duals<false>, std::max<int64_t>(m0, 1), stream, m0, d_kkt_rowmap.p, S, sgn, M_lin, M_base, epi ? m_nl - 1 : (int64_t)-1,
                 epi ? d_kkt_out.p + 2 : (double*)nullptr, (const double*)d_lb.p, (const double*)d_ub.p, d_kkt_out.p + 4, d_kkt_d.p);
    }
    check_launch();
    // ---- 2. g and J of every row at x* = lp_x, into buffers of the report's own: what ktn_sep_* and the certificate read stays
    d_kkt_x.resize((size_t)n0 + 1, stream); d_kkt_x.zero(stream);
    KTN_HIP(hipMemcpyAsync(d_kkt_x.p, lp_x.p, (size_t)std::min<int64_t>(n_lp, n0 + 1) * sizeof(double), hipMemcpyDeviceToDevice, stream));
    d_kkt_g.resize(mm, stream); d_kkt_bconst.resize(mm, stream); d_kkt_maxc.resize(mm, stream); d_kkt_nonfin.resize(mm, stream);
    d_kkt_jac.resize((size_t)nnz_ext + 1, stream); d_kkt_jac.zero(stream);
    auto swap_bufs = [&]() { d_g.swap(d_kkt_g); d_jac.swap(d_kkt_jac); d_bconst.swap(d_kkt_bconst); d_maxc.swap(d_kkt_maxc); d_nonfin.swap(d_kkt_nonfin); };
    swap_bufs();
    try {
        precompute_all(d_kkt_x.p);
    } catch (...) {
        swap_bufs();
        throw;
    }
    swap_bufs();
    // ---- 3. reduced costs
    int G = dev.kkt_group;
    if (!(G == 4 || G == 8 || G == 16 || G == 32 || G == 64)) G = pick_group((double)nnz_ext / (double)(n0 + 1));
    with_group(G, [&](auto g) {
        launch(k_lagr_grad<g()>, group_grid(n0, g()), kBlock, 0, stream, n0, (int32_t)m0, d_kkt_cptr.p, d_kkt_crow.p, d_kkt_cperm.p, d_kkt_jac.p, d_kkt_d.p,
               d_kkt_z.p);
    });
    // ---- 4. the bound
    launch_n(k_dual_terms, m0 + n0, stream, m0, n0, sgn, d_kkt_rowmap.p, kkt_n_lin, d_kkt_d.p, d_kkt_z.p, d_kkt_g.p, d_lb.p, d_ub.p, d_kkt_x.p, lp_l.p, lp_u.p,
             d_kkt_t.p);
    if (m0 + n0 > 0) launch(k_sum_partial, kRedBlocks, kBlock, 0, stream, m0 + n0, d_kkt_t.p, partials.p);
    else KTN_HIP(hipMemsetAsync(partials.p, 0, kRedBlocks * sizeof(double), stream));
    launch(k_dual_final, 1, 64, 0, stream, partials.p, (int)kRedBlocks, d_kkt_g.p, d_kkt_x.p, m0, n0, d_kkt_out.p);
    check_launch();
    h_kkt_d.assign((size_t)m0, 0.0); h_kkt_z.assign((size_t)n0, 0.0);
    std::vector<double> out(d_kkt_out.n, 0.0);
    if (m0 > 0) KTN_HIP(hipMemcpyAsync(h_kkt_d.data(), d_kkt_d.p, (size_t)m0 * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (n0 > 0) KTN_HIP(hipMemcpyAsync(h_kkt_z.data(), d_kkt_z.p, (size_t)n0 * sizeof(double), hipMemcpyDeviceToHost, stream));
    d_kkt_out.download(out.data(), out.size(), stream);
    // Min form: LB = f_min - T with f_min = sgn f; mirrored back: bound = sgn LB, gap = T in both senses
    const double T = out[0], f = out[1];
    kkt_bound = sgn * (sgn * f - T);
    kkt_gap = T;
    h_kkt_blk.clear();                                  // (per instance: kkt_blocks, on ktn_blocks_get_dual_bounds only)
    stats["kkt_evals"] += 1.0;
    stats["kkt_epi_dual"] = epi ? out[2] : std::numeric_limits<double>::quiet_NaN();
    stats["kkt_group"] = (double)G;
    stats["kkt_clamped_duals"] = out[4]; stats["kkt_clamped_max"] = out[5];      // (0, 0 after a device launch of the batch loop: the arenas are not clamped)
    kkt_key_version = lp_version; kkt_key_solves = kkt_solves; kkt_cached = true;
}

// The instances' ranges of a fused batch -- linear rows, NL slots, columns, each grouped by instance, instance after instance -- and
// the caller rows of each instance, found once per ktn_set_blocks (kkt_seg_ok); shared by kkt_blocks and the feasible points per
// instance (feas.hip).
void Engine::kkt_build_seg() {
    const int64_t nb = n_blocks;
    if (kkt_seg_ok) return;
    std::vector<int64_t> seg((size_t)nb * 6), bl((size_t)nb + 1, 0), bn((size_t)nb + 1, 0), bptr((size_t)nb + 1, 0);
    std::vector<int32_t> blk_of((size_t)std::max<int64_t>(m0, 1), 0);
    auto block_of_col = [&](int64_t c) { return (int64_t)(std::upper_bound(h_blkcol.begin(), h_blkcol.end(), c) - h_blkcol.begin()) - 1; };
    std::vector<char> is_nl((size_t)std::max<int64_t>(m0, 1), 0);
    for (auto r : h_nlrows) if (r < m0) is_nl[(size_t)r] = 1;
    int64_t prev_l = 0, prev_n = 0;
    bool grouped = true;
    for (int64_t i = 0; i < m0; ++i) {
        if (h_rowptr[i + 1] == h_rowptr[i]) { grouped = false; break; }
        const int64_t b = std::min<int64_t>(std::max<int64_t>(block_of_col(h_col[(size_t)h_rowptr[i]]), 0), nb - 1);
        int64_t& prev = is_nl[(size_t)i] ? prev_n : prev_l;
        if (b < prev) { grouped = false; break; }
        prev = b;
        (is_nl[(size_t)i] ? bn : bl)[(size_t)b + 1] += 1;
        blk_of[(size_t)i] = (int32_t)b; bptr[(size_t)b + 1] += 1;
    }
    if (!grouped) throw Error(KTN_E_UNSUPPORTED, "KKT report: the rows of the fused batch are not grouped by instance");
    for (int64_t b = 0; b < nb; ++b) { bl[(size_t)b + 1] += bl[(size_t)b]; bn[(size_t)b + 1] += bn[(size_t)b]; bptr[(size_t)b + 1] += bptr[(size_t)b]; }
    for (int64_t b = 0; b < nb; ++b) {
        int64_t* s = seg.data() + 6 * b;
        s[0] = bl[(size_t)b]; s[1] = bl[(size_t)b + 1];
        s[2] = kkt_n_lin + bn[(size_t)b]; s[3] = kkt_n_lin + bn[(size_t)b + 1];
        s[4] = m0 + h_blkcol[(size_t)b]; s[5] = m0 + std::min<int64_t>(h_blkcol[(size_t)b + 1], n0);
    }
    // the caller rows of each instance, ascending (the feasible point's per-instance verification, feas.hpp)
    std::vector<int32_t> brows((size_t)std::max<int64_t>(m0, 1), 0);
    {
        std::vector<int64_t> cur(bptr.begin(), bptr.end() - 1);
        for (int64_t i = 0; i < m0; ++i) brows[(size_t)cur[(size_t)blk_of[(size_t)i]]++] = (int32_t)i;
    }
    d_kkt_seg.upload(seg, stream);
    d_kkt_browptr.upload(bptr, stream);
    d_kkt_brows.upload(brows, stream);
    sync();
    h_kkt_seg = seg;
    kkt_seg_ok = true;
}

// The bound per instance of a fused batch (ktn_blocks_get_dual_bounds) from the terms the last evaluation left in d_kkt_t: one
// launch of k_dual_bound, no re-evaluation.
void Engine::kkt_blocks() {
    kkt_compute();
    const int64_t nb = n_blocks;
    KTN_REQUIRE(nb > 0, "KKT report: no blocks set (ktn_set_blocks)");
    if ((int64_t)h_kkt_blk.size() == 2 * nb) return;
    const double sgn = (sense == KTN_MAX) ? -1.0 : 1.0;
    kkt_build_seg();
    d_kkt_blk.resize((size_t)(2 * nb), stream);
    launch(k_dual_bound, (unsigned)nb, kBlock, 0, stream, d_kkt_seg.p, d_kkt_t.p, lp_c.p, d_kkt_x.p, m0, d_kkt_blk.p);
    check_launch();
    const std::vector<double> out = d_kkt_blk.to_host(stream);
    h_kkt_blk.assign((size_t)(2 * nb), 0.0);
    for (int64_t b = 0; b < nb; ++b) {
        const double Tb = out[(size_t)(2 * b)], fb = out[(size_t)(2 * b + 1)];
        h_kkt_blk[(size_t)(2 * b)] = sgn * (sgn * fb - Tb);
        h_kkt_blk[(size_t)(2 * b + 1)] = Tb;
    }
}

// the batched {isconstrsat, gencut, round_coefs, _addcut} over the NL rows
void Engine::sweep(const double* d_x, double f_tol, int64_t* nviol_out, double* maxviol_out, bool* nonfinite_out) {
    auto t0 = std::chrono::steady_clock::now();
    *nviol_out = 0;
    *maxviol_out = 0.0;
    *nonfinite_out = false;
    last_sweep_cuts = 0;
    stats["sweeps"] += 1.0;
    if (m_nl == 0) return;
    if (esh_mode() && !esh_ready) esh_prepare();
    NlpDev P = nlp_view();
    SweepOut O = sweep_view();
    KTN_HIP(hipMemsetAsync(d_scal.p, 0, sizeof(double), stream));
    KTN_HIP(hipMemsetAsync(d_anynf.p, 0, sizeof(int32_t), stream));
    hipEvent_t e0 = nullptr, e1 = nullptr;         // profile: the separable evaluation carries its own start / stop events
    if (prm.profile) {
        const size_t ea = ev_get(), eb = ev_get();
        e0 = ev_pool[ea]; e1 = ev_pool[eb];
        ev_recs.push_back({2, ea, eb, sweep_bytes});
    }
    if (blk_on) {
        // long rows: column-blocked evaluation through LDS, then the block-order combination
        with_value<1, 2, 0>(blk_cfg, [&](auto c) {       // KTN_BLK_CFG: tuning variants kept for the next round's experiments
            constexpr int G = c() == 0 ? 8 : 16, BC = c() == 2 ? 16384 : 8192, BS = c() == 2 ? 1024 : 512;
            launch_ev(k_sep_eval_blk<G, BC, BS, 4>, (unsigned)(num_cus * blk_wg_per_cu), BS, 0, stream, e0, nullptr, d_bcolk.p, d_bpp.p, d_bseg.p, d_bkind.p,
                      m_nl, blk_nb, d_x, n_lp, d_part.p);
        });
        launch_ev(k_sep_combine, grid_n(m_nl), kBlock, 0, stream, nullptr, e1, d_slots.p, m_nl, blk_nb, d_part.p, f_tol, O);
    } else if (sb_on) {
        if (!sb_lds_set) {
            KTN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sep_sweep_batch), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSbLds));
            sb_lds_set = true;
        }
        SbView V{d_sbck.p, d_sbrow.p, d_sbpp.p, d_sbseg.p, sb_nb};
        launch_ev(k_sep_sweep_batch, (unsigned)sb_batches, kSbThreads, kSbLds, stream, e0, e1, V, P, d_nlrows.p, m_nl, d_x, n_lp, f_tol, O);
    } else {
        // many short rows: several rows per lane group (k_sep_sweep) once one row per group would make more wavefronts
        // than the chip holds several times over; small sweeps keep one row per group and all the parallelism (the
        // choice is made once in loadproblem)
        const int R = sweep_rows_per_group;
        with_value<4, 2, 1>(R >= 4 ? 4 : R >= 2 ? 2 : 1, [&](auto r) {
            with_group(grp_sweep, [&](auto g) {
                constexpr int G = g(), RR = r();
                if constexpr (RR == 1) launch_ev(k_sep_eval<G>, group_grid(m_nl, G), kBlock, 0, stream, e0, e1, P, d_nlrows.p, m_nl, d_x, f_tol, 0, 1, O);
                else launch_ev(k_sep_sweep<G, RR>, group_grid(m_nl, G, RR), kBlock, 0, stream, e0, e1, P, d_nlrows.p, m_nl, d_x, f_tol, O);
            });
        });
    }
    if (n_longev_nl > 0)
        launch(k_sep_eval_long, (unsigned)n_longev_nl, 1024, 0, stream, P, d_longev_nlrows.p, d_longev_nlslots.p, d_x, f_tol, 1, O);
    launch_quad(true, d_x, f_tol);
    if (n_tape_nl > 0 || n_host_nl > 0) {
        // tape rows: the classed shapes in one launch (k_tape_classed, statistics folded in), the others through the interpreter
        // and k_gj_stats.  profile: the tape part has an event record of its own (tape_eval_*; sweep_eval_* stays the separable kernel)
        size_t ta = 0, tb = 0;
        const bool ev = prm.profile && n_tape_nl > 0;
        if (ev) { ta = ev_get(); tb = ev_get(); KTN_HIP(hipEventRecord(ev_pool[ta], stream)); }
        const int64_t n_int = (int64_t)d_tapeint_nl.n;
        launch_n(k_tape_eval, n_int, stream, P, d_tapeint_nl.p, n_int, d_x, O);
        if (n_host_nl > 0) host_eval(d_x);
        launch_tape_classed(true, d_tc_mslot.p, d_x, f_tol);
        if (n_int > 0 || n_host_nl > 0)
            launch_n(k_gj_stats, m_nl, stream, P, d_nlrows.p, m_nl, d_x, f_tol, (int)KTN_ROW_TAPE, (const uint8_t*)(tc_rows_nl > 0 ? d_tc_rowflag.p : nullptr),
                     O);
        if (ev) { KTN_HIP(hipEventRecord(ev_pool[tb], stream)); ev_recs.push_back({4, ta, tb, tape_bytes}); }
    }
    check_launch();
    exclusive_scan(d_flag.p, d_rank.p, (size_t)m_nl);
    exclusive_scan(d_cnt.p, d_cntscan.p, (size_t)m_nl);
    int64_t tail[4];
    double mv = 0.0;
    int32_t anynf = 0;
    if (h_chk_dev) {                               // one thread gathers the six scalars into pinned host memory
        double* ht = h_chk + 2 * kChkQ;
        launch(k_host_tail, 1, 1, 0, stream, h_chk_dev + 2 * kChkQ, d_flag.p + (m_nl - 1), d_rank.p + (m_nl - 1), d_cnt.p + (m_nl - 1),
               d_cntscan.p + (m_nl - 1), (const double*)d_scal.p, (const int32_t*)d_anynf.p, (const int32_t*)nullptr);
        sync();
        for (int k = 0; k < 4; ++k) tail[k] = (int64_t)ht[k];
        mv = ht[4]; anynf = (int32_t)ht[5];
    } else {
        KTN_HIP(hipMemcpyAsync(&tail[0], d_flag.p + (m_nl - 1), 8, hipMemcpyDeviceToHost, stream));
        KTN_HIP(hipMemcpyAsync(&tail[1], d_rank.p + (m_nl - 1), 8, hipMemcpyDeviceToHost, stream));
        KTN_HIP(hipMemcpyAsync(&tail[2], d_cnt.p + (m_nl - 1), 8, hipMemcpyDeviceToHost, stream));
        KTN_HIP(hipMemcpyAsync(&tail[3], d_cntscan.p + (m_nl - 1), 8, hipMemcpyDeviceToHost, stream));
        KTN_HIP(hipMemcpyAsync(&mv, d_scal.p, 8, hipMemcpyDeviceToHost, stream));
        KTN_HIP(hipMemcpyAsync(&anynf, d_anynf.p, 4, hipMemcpyDeviceToHost, stream));
        sync();
    }
    if (prm.profile) ev_flush();
    int64_t V = tail[0] + tail[1], nnzV = tail[2] + tail[3];
    *nviol_out = V;                // the stop rule counts EVERY violated row (model.jl:273-283)
    *maxviol_out = mv;
    // Deepest-cut selection: an LP vertex is supported by at most n_lp rows, so when far more rows than that are
    // violated only the cut_cap_factor * n_lp deepest get a cut this iteration (the reference cuts every violated
    // row; with 1e6 NL rows over 1e5 variables that makes the LP 10x larger than it needs to be).  Ties at the
    // threshold are all kept.  Never triggers on the reference's own test models.
    int64_t cap = (prm.cut_cap_factor > 0.0) ? std::max<int64_t>((int64_t)(prm.cut_cap_factor * (double)n_lp), prm.cut_cap_min) : 0;
    if (cap > 0 && row_sharded()) cap = std::max<int64_t>(cap / dist.world, 1);      // every rank selects among ITS rows
    if (cap > 0 && V > cap && !anynf) {
        d_dkeys.resize((size_t)m_nl, stream); d_dsorted.resize((size_t)m_nl, stream);
        launch_n(k_depth_keys, m_nl, stream, P, d_nlrows.p, m_nl, d_g.p, d_flag.p, d_dkeys.p);
        const size_t need = sort_keys_desc_temp_bytes((size_t)m_nl);
        d_sorttmp.resize(need + 16, stream);
        KTN_HIP(sort_keys_desc_u64(d_sorttmp.p, need, d_dkeys.p, d_dsorted.p, (size_t)m_nl, stream));
        launch_n(k_depth_reflag, m_nl, stream, m_nl, d_dkeys.p, d_dsorted.p, cap, d_flag.p, d_cnt.p);
        check_launch();
        exclusive_scan(d_flag.p, d_rank.p, (size_t)m_nl);
        exclusive_scan(d_cnt.p, d_cntscan.p, (size_t)m_nl);
        KTN_HIP(hipMemcpyAsync(&tail[0], d_flag.p + (m_nl - 1), 8, hipMemcpyDeviceToHost, stream));
        KTN_HIP(hipMemcpyAsync(&tail[1], d_rank.p + (m_nl - 1), 8, hipMemcpyDeviceToHost, stream));
        KTN_HIP(hipMemcpyAsync(&tail[2], d_cnt.p + (m_nl - 1), 8, hipMemcpyDeviceToHost, stream));
        KTN_HIP(hipMemcpyAsync(&tail[3], d_cntscan.p + (m_nl - 1), 8, hipMemcpyDeviceToHost, stream));
        sync();
        V = tail[0] + tail[1];
        nnzV = tail[2] + tail[3];
        stats["cut_selections"] += 1.0;
        stats["cuts_skipped"] += (double)(*nviol_out - V);
    }
    if (anynf) {   // model.jl:69-73: "Nonlinear constraint or objective likely undefined within domain"
        std::fprintf(stderr, "WARNING: Nonlinear constraint or objective likely undefined within domain\n");
        *nonfinite_out = true;
        return;
    }
    if (V > 0) {
        if (esh_mode()) esh_search(d_x, f_tol);     // (esh.hip: moves the selected rows' cuts to x_b)
        lp_rowptr.resize((size_t)(M + V + 1), stream);
        lp_lo.resize((size_t)(M + V), stream);
        lp_hi.resize((size_t)(M + V), stream);
        lp_y.resize((size_t)(M + V), stream);
        d_cutprev.resize((size_t)(M + V), stream);
        d_age.resize((size_t)(M + V), stream);
        KTN_HIP(hipMemsetAsync(d_age.p + M, 0, (size_t)V * sizeof(int32_t), stream));
        lp_col.resize((size_t)(NNZ + nnzV), stream);
        lp_val.resize((size_t)(NNZ + nnzV), stream);
        d_violslots.resize((size_t)V, stream);
        LpRows L = lp_view();
        launch_n(k_compact, m_nl, stream, P, d_nlrows.p, m_nl, d_flag.p, d_rank.p, d_cntscan.p, d_bconst.p, M, NNZ, L, d_violslots.p, d_lastcut.p, d_cutprev.p,
                 (int)(prm.lp_dual_inherit && !glists));
        if (esh_mode()) esh_emit(d_x, V);
        else with_group(grp_sweep, [&](auto g) {
            launch(k_emit<g()>, group_grid(V, g()), kBlock, 0, stream, P, d_nlrows.p, d_violslots.p, V, d_x, d_jac.p, d_maxc.p, prm.cut_coef_rng, 1, M, L);
        });
        check_launch();
        M += V;
        NNZ += nnzV;
        numcuts += V;
        last_sweep_cuts = V;
        lp_dirty = true; ++lp_version;
    }
    sync();
    stats["sep_time_s"] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// sweep + (row-sharded) the stop rule's quantities over all ranks: number of violated rows, largest violation, error flag
void Engine::global_sweep(const double* d_x, double f_tol, int64_t* nviol, double* maxviol, bool* nonfinite) {
    sweep(d_x, f_tol, nviol, maxviol, nonfinite);
    if (!row_sharded()) return;
    double v[2] = {(double)*nviol, *nonfinite ? 1.0 : 0.0};
    allreduce_host(v, 2, 0);
    double mv = *maxviol;
    allreduce_host(&mv, 1, 1);
    *nviol = (int64_t)(v[0] + 0.5);
    *nonfinite = v[1] > 0.0;
    *maxviol = mv;
}

}  // namespace ktn
