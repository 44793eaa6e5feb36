// rebound.hip -- re-solve after a change of variable bounds, of constraint bounds or of a linear cost, from the kept cut pool:
// the host side of rebound.hpp (struct Engine: engine.hpp)
#include "engine.hpp"
#include "launch.hpp"
#include "kernels.hpp"
#include "dense_lp.hpp"
#include "rebound.hpp"

namespace ktn {

// Everything reset() does except the items that make up the pool.  Kept: M, NNZ, numcuts, purged_total (numcuts - purged_total is
// the number of cuts in the LP), the row arrays, lp_x, lp_y, the cut lists and ages (d_lastcut, d_cutprev, d_glast, d_age,
// sharded_rows), lp_version, lp_epoch, lp_dirty, the column mirror with its long-column scan, the scaling (scal_rows; compute_scaling
// reads the matrix only, neither c nor l nor u) and the sigma_max estimate, omega / have_omega.
void Engine::reopen() {
    const bool was_optimal = status == KTN_STATUS_OPTIMAL;
    have_precompute = false;
    blocks_built_rows = -1;
    kkt_solved = false; kkt_arena = false; kkt_cached = false; feas_cached = false; feas_blk_cached = false;
    if (d_blkomega.n) d_blkomega.zero(stream);
    if (ds_valid.n) ds_valid.zero(stream);               // the exact solvers restart cold
    dense_credit = dense_run = 0;
    md_valid = false; md_y_version = 0; mid_credit = mid_run = 0; mid_backoff = mid_backoff_len = 0;
    last_sweep_cuts = 0;
    status = KTN_STATUS_NONE; lp_status = KTN_STATUS_OPTIMAL;
    iter = 0; soltime = 0.0; objval = std::numeric_limits<double>::quiet_NaN();
    // after an :Optimal solve the first LP of the re-solve runs at the tolerance that solve ended with (its floor): at lp_tol_cap
    // the warm, clamped point would pass the first check and the round would sweep at the old optimum
    if (begun && !was_optimal) last_maxviol = 1e300;      // (begun: a solve ran since the load or the last setter)
    obj_prev = kInf; allsat = false; begun = false; tight_done = false;
    log_cuts_lastprnt = 0; log_max_viol = 0;
    polishing = false; polish_done = false; polish_count = 0; best_viol = kInf; best_obj = 0.0; cert_target = 0.0;
    lp_sols.clear();
    screened_out = false;
    reopened = true;
    blocks_rewarmed = false;          // (the arenas of a device launch, blocks_launched and x stay: a warm launch screens them again)
    sync();
}

static void require_own_lp(const Engine* e, const char* who) {
    if (e->kkt_foreign())
        throw Error(KTN_E_UNSUPPORTED, std::string(who) + ": not available on a row-sharded handle or one with a cut exchange or a transport installed");
}

void Engine::set_var_bounds(const double* l, const double* u, int64_t n) {
    KTN_REQUIRE(loaded, "ktn_set_var_bounds: after ktn_loadproblem");
    KTN_REQUIRE(n == n0, "ktn_set_var_bounds: n must be the problem's num_var");
    KTN_REQUIRE(status != KTN_STATUS_ERROR, "ktn_set_var_bounds: the handle's status is :Error (ktn_reset or ktn_loadproblem first)");
    require_own_lp(this, "ktn_set_var_bounds");
    for (int64_t j = 0; j < n0; ++j)
        KTN_REQUIRE(!(l && l[j] != l[j]) && !(u && u[j] != u[j]), "ktn_set_var_bounds: a bound is NaN");
    std::vector<double> lv = lp_l.to_host(stream), uv = lp_u.to_host(stream);      // (a NULL side keeps what is there; the epigraph variable keeps +-inf)
    if (l) std::copy(l, l + n0, lv.begin());
    if (u) std::copy(u, u + n0, uv.begin());
    lp_l.upload(lv, stream); lp_u.upload(uv, stream);
    has_inf_bound = false; has_big_bound = false; crossed_cols = 0;
    for (int64_t j = 0; j < n_lp; ++j) {
        if (!std::isfinite(lv[(size_t)j]) || !std::isfinite(uv[(size_t)j])) has_inf_bound = true;
        if ((std::isfinite(uv[(size_t)j]) && uv[(size_t)j] >= kDenseBig) || (std::isfinite(lv[(size_t)j]) && -lv[(size_t)j] >= kDenseBig)) has_big_bound = true;
        if (lv[(size_t)j] > uv[(size_t)j]) ++crossed_cols;
    }
    // the box of the supporting-hyperplane auxiliary problem; the engine's own interior point belongs to the old box
    if (aux.n > 0) {
        std::copy(lv.begin(), lv.begin() + n0, aux.lv.begin());
        std::copy(uv.begin(), uv.begin() + n0, aux.uv.begin());
    }
    delete child;                                        // (esh_find_interior never leaves one behind: it builds its own from aux)
    child = nullptr;
    if (!xint_given) { xint_found = 0; esh_ready = false; h_xint.clear(); }
    d_act_cnt.resize(4, stream);
    d_act_cnt.zero(stream);
    launch_n(k_rebound, n_lp, stream, n_lp, (const double*)lp_l.p, (const double*)lp_u.p, lp_x.p, d_act_cnt.p);
    check_launch();
    unsigned long long cnt[2] = {0, 0};
    KTN_HIP(hipMemcpyAsync(cnt, d_act_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, stream));
    sync();
    stats["warm_clamped_cols"] = (double)cnt[0];
    screen_pending = true;
    reopen();
}

void Engine::set_linear_objective(const double* c, int64_t n, double c0_new) {
    KTN_REQUIRE(loaded, "ktn_set_linear_objective: after ktn_loadproblem");
    KTN_REQUIRE(c != nullptr && n == n0, "ktn_set_linear_objective: c must hold the problem's num_var coefficients");
    KTN_REQUIRE(status != KTN_STATUS_ERROR, "ktn_set_linear_objective: the handle's status is :Error (ktn_reset or ktn_loadproblem first)");
    require_own_lp(this, "ktn_set_linear_objective");
    if (!obj_settable)
        throw Error(KTN_E_UNSUPPORTED, "ktn_set_linear_objective: the loaded objective is not a linear row of KTN_ATOM_LIN atoms or a KTN_ROW_QUAD row without Q");
    KTN_REQUIRE(c0_new == c0_new, "ktn_set_linear_objective: c0 is NaN");
    // the objective row's own entries: all but its last one, -t
    const int64_t ob = h_rowptr[(size_t)m0], ne = h_rowptr[(size_t)m0 + 1] - ob - 1;
    std::vector<uint8_t> seen((size_t)n0, 0);
    std::vector<double> p0((size_t)std::max<int64_t>(ne, 1), 0.0), cvec((size_t)n_lp, 0.0);
    for (int64_t k = 0; k < ne; ++k) {
        const int32_t j = h_col[(size_t)(ob + k)];
        if (!seen[(size_t)j]) p0[(size_t)k] = c[j];      // (a column the row names twice carries its coefficient on the first entry)
        seen[(size_t)j] = 1;
    }
    for (int64_t j = 0; j < n0; ++j) {
        KTN_REQUIRE(c[j] == c[j], "ktn_set_linear_objective: a coefficient is NaN");
        KTN_REQUIRE(c[j] == 0.0 || seen[(size_t)j], "ktn_set_linear_objective: a non-zero coefficient on a column outside the objective row's structure");
        cvec[(size_t)j] = seen[(size_t)j] ? c[j] : 0.0;
    }
    lp_c.upload(cvec, stream);
    c0 = c0_new;
    DBuf<double> t_p0;
    t_p0.upload(p0, stream);
    launch_n(k_obj_coefs, std::max<int64_t>(ne, 1), stream, ne, ob, (const double*)t_p0.p, d_pp.p, d_rconst.p + m0, c0_new);
    check_launch();
    sync();                                              // (the temporary is freed on leaving the scope)
    reopen();
}

// New constraint bounds in place (rebound.hpp "row bounds").  Nothing is changed before every refusal has been decided.
void Engine::set_row_bounds(const double* lb, const double* ub, int64_t m) {
    KTN_REQUIRE(loaded, "ktn_set_row_bounds: after ktn_loadproblem");
    KTN_REQUIRE(m == m0, "ktn_set_row_bounds: m must be the problem's num_constr");
    KTN_REQUIRE(status != KTN_STATUS_ERROR, "ktn_set_row_bounds: the handle's status is :Error (ktn_reset or ktn_loadproblem first)");
    require_own_lp(this, "ktn_set_row_bounds");
    if (!lists_ok() || glists)
        throw Error(KTN_E_UNSUPPORTED, "ktn_set_row_bounds: the cuts cannot be attributed to their rows (rows appended from the host, or global cut lists)");
    for (int64_t i = 0; i < m0; ++i)
        KTN_REQUIRE(!(lb && lb[i] != lb[i]) && !(ub && ub[i] != ub[i]), "ktn_set_row_bounds: a bound is NaN");
    std::vector<double> nlb(h_lb), nub(h_ub);            // per extended row; a NULL side keeps what is loaded, the epigraph row its own
    if (lb) std::copy(lb, lb + m0, nlb.begin());
    if (ub) std::copy(ub, ub + m0, nub.begin());
    std::vector<char> is_nl((size_t)std::max<int64_t>(m0, 1), 0);
    for (int32_t r : h_nlrows) if (r < m0) is_nl[(size_t)r] = 1;
    // a nonlinear row keeps its pattern of finite sides (an infinite side stays the infinity it is): the finite side defines the
    // convex level set the cuts were taken for
    auto same_side = [](double a, double b) { return std::isfinite(a) ? std::isfinite(b) : a == b; };
    bool lin_changed = false;
    int64_t crossed = 0;
    for (int64_t i = 0; i < m0; ++i) {
        const size_t k = (size_t)i;
        if (is_nl[k])
            KTN_REQUIRE(same_side(h_lb[k], nlb[k]) && same_side(h_ub[k], nub[k]),
                        "ktn_set_row_bounds: a nonlinear row may move its finite bounds but not gain or lose a side");
        else if (std::memcmp(&h_lb[k], &nlb[k], sizeof(double)) != 0 || std::memcmp(&h_ub[k], &nub[k], sizeof(double)) != 0)
            lin_changed = true;
        if (nlb[k] > nub[k]) ++crossed;
    }
    crossed_rows = crossed;
    stats["screen_crossed_rows"] = (double)crossed;
    d_lb_new.upload(nlb, stream); d_ub_new.upload(nub, stream);
    // linear rows: the tangent at the origin again, as the load takes it; their LP rows then equal a fresh load's bit for bit
    if (lin_changed && kkt_n_lin > 0) {
        d_xs.zero(stream);
        precompute_all(d_xs.p);
        launch_n(k_lin_bounds, m0, stream, m0, (const int32_t*)d_kkt_rowmap.p, (const int64_t*)d_rowptr.p, (const double*)d_jac.p, (const double*)d_g.p,
                 (const double*)d_lb_new.p, (const double*)d_ub_new.p, std::min<int64_t>(M, M_lin), lp_lo.p, lp_hi.p);
        check_launch();
    }
    // cuts: every list row moves with its slot's bounds; the old ones are still in d_lb / d_ub
    for (hipEvent_t& e : ev_rebase)                      // the kernels' own begin / end timestamps ("rebase_kernel_s")
        if (!e) KTN_HIP(hipEventCreate(&e));
    d_act_cnt.resize(4, stream);
    d_act_cnt.zero(stream);
    const bool pool_cuts = m_nl > 0 && M > M_base;
    if (pool_cuts) {
        launch_ev(k_rebase_cuts, grid_n(m_nl), kBlock, 0, stream, ev_rebase[0], ev_rebase[1], m_nl, (const int32_t*)d_nlrows.p, (const int64_t*)d_lastcut.p,
                  (const int64_t*)d_cutprev.p, M, (const double*)d_lb.p, (const double*)d_ub.p, (const double*)d_lb_new.p, (const double*)d_ub_new.p,
                  lp_lo.p, lp_hi.p, d_act_cnt.p);
        check_launch();
    }
    // the resident arenas of a device launch hold their own row bounds (batch_warm.hpp k_blocks_rebase)
    const bool arenas = blocks_launched && n_blocks > 0 && (int64_t)h_ar_rows.size() == n_blocks;
    if (arenas) blocks_rebase(d_act_cnt.p + 1, ev_rebase[2], ev_rebase[3]);
    unsigned long long cnt[2] = {0, 0};
    KTN_HIP(hipMemcpyAsync(cnt, d_act_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, stream));
    sync();
    float ms = 0.f, ms_pool = 0.f, ms_blk = 0.f;
    if (pool_cuts && hipEventElapsedTime(&ms_pool, ev_rebase[0], ev_rebase[1]) != hipSuccess) { (void)hipGetLastError(); ms_pool = 0.f; }
    if (arenas && hipEventElapsedTime(&ms_blk, ev_rebase[2], ev_rebase[3]) != hipSuccess) { (void)hipGetLastError(); ms_blk = 0.f; }
    ms = ms_pool + ms_blk;
    stats["rebase_rows"] = (double)(cnt[0] + cnt[1]);
    stats["rebase_kernel_s"] = (double)ms * 1e-3;
    // the bounds themselves, and their two other copies
    h_lb = nlb; h_ub = nub;
    d_lb.upload(h_lb, stream); d_ub.upload(h_ub, stream);
    if (blk_on && d_slots.n == (size_t)m_nl) {           // the column-blocked sweep reads them from its slot records
        std::vector<SepSlot> slots = d_slots.to_host(stream);
        for (int64_t si = 0; si < m_nl; ++si) {
            const size_t r = (size_t)h_nlrows[(size_t)si];
            slots[(size_t)si].lb = h_lb[r]; slots[(size_t)si].ub = h_ub[r];
        }
        d_slots.upload(slots, stream);
        sync();                                          // (the temporary is freed on leaving the scope)
    }
    for (size_t k = 0; k < aux.rows.size(); ++k) {       // the supporting-hyperplane auxiliary problem, in its own row numbering
        aux.lc[k] = h_lb[(size_t)aux.rows[k]]; aux.uc[k] = h_ub[(size_t)aux.rows[k]];
    }
    // the engine's own interior point belongs to the old bounds; the caller's stays, and which rows it is interior to is
    // evaluated again (esh_prepare): a row for which it no longer is stores Kelley's cut
    delete child;
    child = nullptr;
    if (!xint_given) { xint_found = 0; h_xint.clear(); }
    esh_ready = false;
    lp_dirty = true;                                     // the working form (wlo / whi) is a copy of lp_lo / lp_hi made when this is set
    screen_pending = true;                               // a moved row bound can make a row impossible over the unchanged box
    reopen();
}

void Engine::row_owners(int64_t* owner_out) {
    if (!lists_ok() || glists)
        throw Error(KTN_E_UNSUPPORTED, "ktn_lp_get_row_owners: no per-row cut lists (rows appended from the host, or global cut lists)");
    if (M == 0) return;
    DBuf<int64_t> t_owner;
    t_owner.resize((size_t)M, stream);
    KTN_HIP(hipMemsetAsync(t_owner.p, 0xFF, (size_t)M * sizeof(int64_t), stream));
    if (m_nl > 0 && M > M_base) {
        launch_n(k_row_owners, m_nl, stream, m_nl, (const int32_t*)d_nlrows.p, (const int64_t*)d_lastcut.p, (const int64_t*)d_cutprev.p, M, t_owner.p);
        check_launch();
    }
    t_owner.download(owner_out, (size_t)M, stream);      // (synchronises: the temporary is free to go)
    sync();
}

void Engine::row_activity(hipEvent_t e0, hipEvent_t e1) {
    const size_t mm = (size_t)std::max<int64_t>(M, 1);
    d_act_min.resize(mm, stream); d_act_max.resize(mm, stream);
    d_act_cnt.resize(4, stream);
    static const unsigned long long init[4] = {0ull, ~0ull, 0ull, 0ull};      // (static: the copy is read after this function returns)
    KTN_HIP(hipMemcpyAsync(d_act_cnt.p, init, sizeof(init), hipMemcpyHostToDevice, stream));
    const ScreenOut O{d_act_min.p, d_act_max.p, d_act_cnt.p};
    const int G = pick_group(M ? (double)NNZ / (double)M : 1.0);       // as k_spmv<G>: by the mean row length
    with_group(G, [&](auto g) {
        launch_timed(k_row_activity<g()>, group_grid(M, g()), kBlock, 0, stream, e0, e1, M, (const int64_t*)lp_rowptr.p, (const int32_t*)lp_col.p,
                     (const double*)lp_val.p, (const double*)lp_lo.p, (const double*)lp_hi.p, (const double*)lp_l.p, (const double*)lp_u.p,
                     prm.lp_tol_floor * prm.f_tol, O);
    });
    check_launch();
    stats["screen_group"] = (double)G;
}

bool Engine::screen() {
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long long cnt[4] = {0ull, ~0ull, 0ull, 0ull};
    float ms = 0.f;
    if (M > 0) {
        for (hipEvent_t& e : ev_screen)                  // the kernel's own begin / end timestamps ("screen_kernel_s")
            if (!e) KTN_HIP(hipEventCreate(&e));
        row_activity(ev_screen[0], ev_screen[1]);
        KTN_HIP(hipMemcpyAsync(cnt, d_act_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, stream));
        sync();
        if (hipEventElapsedTime(&ms, ev_screen[0], ev_screen[1]) != hipSuccess) { (void)hipGetLastError(); ms = 0.f; }
    }
    stats["screen_runs"] += 1.0;
    stats["screen_infeasible_rows"] = (double)cnt[0];
    stats["screen_first_row"] = cnt[0] ? (double)cnt[1] : -1.0;
    stats["screen_redundant_rows"] = (double)cnt[2];
    stats["screen_crossed_cols"] = (double)crossed_cols;
    stats["screen_crossed_rows"] = (double)crossed_rows;
    stats["screen_kernel_s"] = (double)ms * 1e-3;
    stats["screen_time_s"] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return cnt[0] > 0 || crossed_cols > 0 || crossed_rows > 0;
}

}  // namespace ktn
