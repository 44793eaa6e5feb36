// feas.hip -- a feasible point and a primal bound after a solve: the host side of feas.hpp
// (struct Engine: engine.hpp)
#include "engine.hpp"
#include "launch.hpp"
#include "kernels.hpp"
#include "esh.hpp"
#include "quad_rows.hpp"
#include "feas.hpp"

namespace ktn {

// Once per loaded problem, under every cut_algo (h_esh_side is all zero under Kelley): the rows that take part -- a caller row not
// declared linear, separable, tape or QUAD, with exactly one finite side; never the epigraph row, never a free row -- and the NL slot
// of every tape NL row.
void Engine::feas_sides() {
    if (feas_sides_ok) return;
    std::vector<int8_t> sig((size_t)std::max<int64_t>(m_ext, 1), 0);
    std::vector<int32_t> tslots;
    feas_n_part = 0; feas_two_sided = -1;
    for (size_t si = 0; si < h_nlrows.size(); ++si) {
        const int64_t i = h_nlrows[si];
        const uint8_t kind = h_rowkind[(size_t)i];
        if (kind == KTN_ROW_TAPE) tslots.push_back((int32_t)si);
        if (i >= m0 || (kind != KTN_ROW_SEP && kind != KTN_ROW_TAPE && kind != KTN_ROW_QUAD)) continue;
        const bool lf = std::isfinite(h_lb[(size_t)i]), uf = std::isfinite(h_ub[(size_t)i]);
        if (lf && uf) { if (feas_two_sided < 0) feas_two_sided = i; continue; }
        if (!lf && !uf) continue;                                // a free row has nothing to satisfy
        sig[(size_t)i] = uf ? 1 : -1;
        ++feas_n_part;
    }
    d_feas_sig.upload(sig, stream);
    d_feas_tslots.upload(tslots, stream);
    sync();
    feas_sides_ok = true;
}

// g and J of every row at d_x into (g, jac): the sweep's buffers are swapped out for the call, as in kkt_compute, so what
// ktn_sep_*, the certificate and a following ktn_ecp_step read stays
void Engine::feas_eval(const double* d_x, DBuf<double>& g, DBuf<double>& jac) {
    auto swap_bufs = [&]() { d_g.swap(g); d_jac.swap(jac); d_bconst.swap(d_feas_bconst); d_maxc.swap(d_feas_maxc); d_nonfin.swap(d_feas_nonfin); };
    swap_bufs();
    try {
        precompute_all(d_x);
    } catch (...) {
        swap_bufs();
        throw;
    }
    swap_bufs();
}

// blocks: the per-instance form of a fused batch (ktn_blocks_get_feasible_points) -- the same evaluations and the same search over
// all NL slots, then lambda_b, the point and the verification per instance, one workgroup each.
void Engine::feas_run(bool blocks) {
    KTN_REQUIRE(loaded, "feasible point: no problem loaded");
    if (kkt_foreign())
        throw Error(KTN_E_UNSUPPORTED, "feasible point: a row-sharded handle or one with a cut exchange sees only a part of the rows");
    if (n_host > 0 || host_obj)
        throw Error(KTN_E_UNSUPPORTED, "feasible point: KTN_ROW_HOST rows and objectives are not searched");
    feas_sides();
    if (feas_two_sided >= 0)
        throw Error(KTN_E_UNSUPPORTED, "feasible point: nonlinear row " + std::to_string(feas_two_sided) + " has two finite sides (equality or ranged)");
    const int64_t nb = blocks ? n_blocks : 1;
    KTN_REQUIRE(nb > 0, "feasible points: no blocks set (ktn_set_blocks)");
    KTN_REQUIRE(kkt_solved, "feasible point: no LP solve since the problem was loaded or reset, or since rows were appended, truncated or purged");
    KTN_REQUIRE(!dev.feas_xstar_pre || have_precompute, "feasible point: KTN_FEAS_XSTAR_PRECOMPUTE is set and no ktn_sep_precompute has run");
    if (blocks) {
        kkt_build_seg();                                 // (refuses a batch whose rows are not grouped by instance)
        if (feas_blk_cached && feas_blk_key_version == lp_version && feas_blk_key_solves == kkt_solves) return;
        feas_blk_cached = false;
    } else {
        if (feas_cached && feas_key_version == lp_version && feas_key_solves == kkt_solves) return;
        feas_cached = false;
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double>& hx = blocks ? h_feas_blk_x : h_feas_x;
    std::vector<double> info((size_t)(8 * nb), 0.0);
    hx.assign((size_t)n0, nan);
    if (!blocks) h_feas_lam.assign((size_t)m0, 1.0);
    auto done = [&]() {
        if (blocks) { h_feas_blk_info = info; feas_blk_key_version = lp_version; feas_blk_key_solves = kkt_solves; feas_blk_cached = true; }
        else { std::copy(info.begin(), info.begin() + 8, feas_info); feas_key_version = lp_version; feas_key_solves = kkt_solves; feas_cached = true; }
    };
    auto answer = [&](int64_t b, double found, double lam, double f, double margin, double lin, double row, double unconv, double backoffs) {
        const double v[8] = {found, lam, f, margin, lin, row, unconv, backoffs};
        std::copy(v, v + 8, info.begin() + 8 * b);
    };
    // ---- the reference point: the caller's under every cut_algo, the engine's own under the supporting-hyperplane modes
    if (!xint_given && esh_mode() && !esh_ready) esh_prepare();
    const bool have = xint_given || (esh_mode() && xint_found != 0);
    if (!have || (int64_t)h_xint.size() != n0) {
        for (int64_t b = 0; b < nb; ++b) answer(b, 0.0, nan, nan, nan, nan, -1.0, 0.0, 0.0);
        done();
        return;
    }
    stats["feas_evals"] += 1.0;
    const size_t mm = (size_t)std::max<int64_t>(m_ext, 1), nx = (size_t)n0 + 1, ms = (size_t)std::max<int64_t>(m_nl, 1);
    {
        std::vector<double> xi(h_xint);
        xi.push_back(0.0);
        d_feas_xin.upload(xi, stream);
        sync();
    }
    if (!xint_given) launch_n(k_feas_clamp, n0, stream, n0, d_feas_xin.p, (const double*)lp_l.p, (const double*)lp_u.p);      // (the engine's own point)
    d_feas_xs.resize(nx, stream); d_feas_xs.zero(stream);
    KTN_HIP(hipMemcpyAsync(d_feas_xs.p, dev.feas_xstar_pre ? d_xs.p : lp_x.p, (size_t)std::min<int64_t>(n_lp, n0 + 1) * sizeof(double),
                           hipMemcpyDeviceToDevice, stream));
    d_feas_x.resize(nx, stream);
    for (DBuf<double>* b : {&d_feas_g0, &d_feas_g1, &d_feas_bconst, &d_feas_maxc}) b->resize(mm, stream);
    d_feas_nonfin.resize(mm, stream);
    for (DBuf<double>* b : {&d_feas_j0, &d_feas_j1}) { b->resize((size_t)nnz_ext + 1, stream); b->zero(stream); }
    d_feas_lam.resize(ms, stream); d_feas_unc.resize(ms, stream); d_feas_unc.zero(stream);
    d_feas_part.resize((size_t)kRedBlocks * 4, stream);
    d_feas_res.resize((size_t)(4 * nb), stream); d_feas_out.resize((size_t)(16 * nb), stream);
    d_feas_cnt.resize(1, stream); d_feas_cnt.zero(stream);
    // ---- 1. every row at x_in (the check of the reference point; J0 of the QUAD rows) and at x* (g*, J* of the QUAD rows)
    auto verify = [&](const double* d_x, const double* g, double* out) {
        const FeasVerify V{d_feas_sig.p, d_kkt_rowmap.p, g, d_lb.p, d_ub.p, d_x, lp_l.p, lp_u.p};
        if (blocks) {
            launch(k_feas_verify_blocks, (unsigned)nb, kBlock, 0, stream, (const int64_t*)d_kkt_seg.p, m0, (const int64_t*)d_kkt_browptr.p,
                   (const int32_t*)d_kkt_brows.p, V, (const double*)lp_c.p, out);
        } else {
            launch(k_feas_verify_partial, kRedBlocks, kBlock, 0, stream, m0, n0, V, d_feas_part.p);
            launch(k_feas_verify_final, 1, 64, 0, stream, (const double*)d_feas_part.p, (int)kRedBlocks, g, d_x, m0, n0, out);
        }
    };
    feas_eval(d_feas_xin.p, d_feas_g0, d_feas_j0);
    verify(d_feas_xin.p, d_feas_g0.p, d_feas_out.p);
    feas_eval(d_feas_xs.p, d_feas_g1, d_feas_j1);
    // ---- 2. lambda_i per NL slot
    NlpDev P = nlp_view();
    const double tau = prm.esh_root_tol * prm.f_tol;
    const FeasArgs A{d_feas_xs.p, d_feas_xin.p, d_feas_sig.p, d_feas_lam.p, d_feas_unc.p, d_feas_cnt.p, tau, prm.esh_root_iters};
    const bool pinned = dev.feas_group == 4 || dev.feas_group == 8 || dev.feas_group == 16 || dev.feas_group == 32 || dev.feas_group == 64;
    const int G = pinned ? dev.feas_group : grp_sweep, G2 = pinned ? dev.feas_group : grp_quad_rows;
    launch_n(k_fill, (int64_t)ms, stream, (int64_t)ms, d_feas_lam.p, 1.0);
    with_group(G, [&](auto g) { launch(k_feas_sep<g()>, group_grid(m_nl, g()), kBlock, 0, stream, P, d_nlrows.p, m_nl, A); });
    if (n_longev_nl > 0) launch(k_feas_long, (unsigned)n_longev_nl, 1024, 0, stream, P, d_longev_nlrows.p, d_longev_nlslots.p, A);
    // (the tape kernel's Jacobian scratch: J1, whose tape entries nothing reads afterwards -- the QUAD rows' entries are not touched)
    launch_n(k_feas_tape, n_tape_nl, stream, P, d_taperows_nl.p, d_feas_tslots.p, n_tape_nl, A, d_feas_j1.p);
    if (n_quad_nl > 0) {
        const QuadList QL{d_qrows_nl.p, d_qslots_nl.p, d_qtbase_nl.p, nullptr, n_quad_nl, n_quad_ent_nl};
        with_group(G2, [&](auto g) {
            launch(k_feas_quad<g()>, group_grid(n_quad_nl, g()), kBlock, 0, stream, P, QL, (const double*)d_feas_g1.p, (const double*)d_feas_j1.p,
                   (const double*)d_feas_j0.p, A);
        });
    }
    // ---- 3. lambda* and the blocking row, then the point: no host round trip in between
    if (blocks) {
        launch(k_feas_min_blocks, (unsigned)nb, kBlock, 0, stream, (const int64_t*)d_kkt_seg.p, kkt_n_lin, (const double*)d_feas_lam.p,
               (const int32_t*)d_feas_unc.p, (const int32_t*)d_nlrows.p, d_feas_res.p);
    } else {
        FeasMin* part = reinterpret_cast<FeasMin*>(d_feas_part.p);
        launch(k_feas_min_partial, kRedBlocks, kBlock, 0, stream, m_nl, (const double*)d_feas_lam.p, (const int32_t*)d_feas_unc.p,
               (const int32_t*)d_nlrows.p, part);
        launch(k_feas_min_final, 1, kBlock, 0, stream, (const FeasMin*)part, (int)kRedBlocks, d_feas_res.p);
    }
    // ---- 4. the point, verified; a failed verification (rounding, the clamp) moves lambda towards 0 and verifies again:
    //         back-off k = 1 .. 8 takes lambda* (1 - 2^(6 k - 48)), so the eighth lands on x_in itself.  Per instance in the blocks form.
    std::vector<double> out((size_t)(16 * nb)), shrink((size_t)nb, 1.0);
    std::vector<int> backoffs((size_t)nb, 0);
    double* const out1 = d_feas_out.p + 8 * nb;          // (the verification of x_feas behind that of x_in)
    auto ref_ok = [&](int64_t b) { return out[(size_t)(8 * b + 2)] < 0.0 && out[(size_t)(8 * b + 3)] == 0.0; };      // x_in: no offending row, inside [l, u]
    auto feas_ok = [&](int64_t b) { return out[(size_t)(8 * (nb + b) + 2)] < 0.0; };
    for (;;) {
        if (blocks) {
            d_feas_shrink.upload(shrink, stream);
            launch_n(k_feas_point_blocks, n0, stream, n0, (const int64_t*)d_blkcol.p, nb, (const double*)d_feas_xs.p, (const double*)d_feas_xin.p,
                     (const double*)lp_l.p, (const double*)lp_u.p, (const double*)d_feas_shrink.p, d_feas_res.p, d_feas_x.p);
        } else {
            launch_n(k_feas_point, std::max<int64_t>(n0, 1), stream, n0, (const double*)d_feas_xs.p, (const double*)d_feas_xin.p, (const double*)lp_l.p,
                     (const double*)lp_u.p, shrink[0], d_feas_res.p, d_feas_x.p);
        }
        feas_eval(d_feas_x.p, d_feas_g1, d_feas_j1);
        verify(d_feas_x.p, d_feas_g1.p, out1);
        check_launch();
        d_feas_out.download(out.data(), out.size(), stream);
        bool again = false;
        for (int64_t b = 0; b < nb; ++b)
            if (ref_ok(b) && !feas_ok(b) && backoffs[(size_t)b] < 8) {
                ++backoffs[(size_t)b];
                shrink[(size_t)b] = 1.0 - std::ldexp(1.0, 6 * backoffs[(size_t)b] - 48);
                again = true;
            }
        if (!again) break;
    }
    const std::vector<double> res = d_feas_res.to_host(stream);
    if (!blocks) {
        const std::vector<double> lam = d_feas_lam.to_host(stream);
        for (int64_t s = 0; s < m_nl; ++s)
            if (h_nlrows[(size_t)s] < m0) h_feas_lam[(size_t)h_nlrows[(size_t)s]] = lam[(size_t)s];
    }
    unsigned long long cnt = 0ull;
    KTN_HIP(hipMemcpyAsync(&cnt, d_feas_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, stream));
    std::vector<double> xf((size_t)n0 + 1);
    d_feas_x.download(xf.data(), xf.size(), stream);       // (synchronises: cnt is here too)
    stats["feas_group"] = (double)G;
    stats["feas_quad_group"] = (double)G2;
    stats["feas_passes"] = (double)cnt;
    for (int64_t b = 0; b < nb; ++b) {
        const double* o0 = out.data() + 8 * b;
        const double* o1 = out.data() + 8 * (nb + b);
        const double* r = res.data() + 4 * b;
        if (!ref_ok(b)) {                            // the reference point is outside [l, u], violates a row, or a row is not finite there
            answer(b, -1.0, nan, nan, o0[0], o0[1], o0[2], r[2], 0.0);
        } else if (!feas_ok(b)) {
            answer(b, -2.0, r[3], nan, o1[0], o1[1], o1[2], r[2], (double)backoffs[(size_t)b]);
        } else {
            answer(b, 1.0, r[3], o1[4], o1[0], o1[1], r[1], r[2], (double)backoffs[(size_t)b]);
            const int64_t c0 = blocks ? h_blkcol[(size_t)b] : 0, c1 = blocks ? std::min<int64_t>(h_blkcol[(size_t)b + 1], n0) : n0;
            std::copy(xf.begin() + c0, xf.begin() + c1, hx.begin() + c0);
        }
    }
    done();
}

}  // namespace ktn
