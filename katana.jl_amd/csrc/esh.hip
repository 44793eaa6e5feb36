// esh.hip -- supporting-hyperplane cuts (cut_algo == KTN_CUT_SUPPORTING / _QUAD): the auxiliary problem that finds
// the interior point, its evaluation, and the host side of the per-row root search in the sweep  (struct Engine: engine.hpp)
#include "engine.hpp"
#include "launch.hpp"
#include "kernels.hpp"
#include "esh.hpp"
#include "esh_quad.hpp"

namespace ktn {

// At load (the caller's description is valid only now): which rows take part, and the auxiliary min-max problem
//     min s   over (x, s), s in [-1, +inf):   linear rows as they are;   g_i(x) - s <= ub_i  /  g_i(x) + s >= lb_i  per taking-part row
// (a separable row gains a LIN atom on s, a tape row VAR s and SUB / ADD, a taking-part QUAD row -- KTN_CUT_SUPPORTING_QUAD -- an
//  entry on s with coefficient -sigma_i and an empty Q segment, as the engine appends t to a quadratic objective; every other
//  nonlinear row is dropped).
void Engine::esh_build_aux(const double* l_var, const double* u_var, const double* l_constr, const double* u_constr,
                           const ktn_nlp_desc* d) {
    delete child;
    child = nullptr;
    xint_given = false; esh_ready = false; xint_found = 0;
    blocks_launched = false;                     // (a new problem: no device launch of the batch loop to read back yet)
    blocks_drop_warm();
    h_xint.clear();
    aux = EshAux();
    h_esh_side.assign((size_t)m_ext, 0);
    esh_n_part = esh_n_quad_part = 0;
    d_jint.release();
    stats["esh_quad_rows"] = 0.0;
    if (!esh_mode()) return;
    if (row_sharded()) throw Error(KTN_E_UNSUPPORTED, "cut_algo = KTN_CUT_SUPPORTING is not available on a row-sharded handle");
    std::vector<int32_t> tslots;
    for (size_t si = 0; si < h_nlrows.size(); ++si) {
        const int64_t i = h_nlrows[si];
        if (h_rowkind[(size_t)i] == KTN_ROW_TAPE) tslots.push_back((int32_t)si);
        const bool quad = esh_quad_mode() && h_rowkind[(size_t)i] == KTN_ROW_QUAD;       // (h_nlrows: not declared linear)
        if (i >= m0 || (h_rowkind[(size_t)i] != KTN_ROW_SEP && h_rowkind[(size_t)i] != KTN_ROW_TAPE && !quad)) continue;
        const bool lf = std::isfinite(h_lb[(size_t)i]), uf = std::isfinite(h_ub[(size_t)i]);
        if (lf == uf) continue;                                  // two-sided rows, equalities, free rows
        h_esh_side[(size_t)i] = uf ? 1 : -1;
        ++esh_n_part;
        if (quad) ++esh_n_quad_part;
    }
    d_tape_nlslots.upload(tslots, stream);
    stats["esh_participating_rows"] = (double)esh_n_part;
    if (esh_n_part == 0) return;
    EshAux& A = aux;
    const int32_t s_col = (int32_t)n0;
    A.n = n0 + 1;
    A.lv.assign(l_var, l_var + n0); A.lv.push_back(-1.0);
    A.uv.assign(u_var, u_var + n0); A.uv.push_back(kInf);
    A.rowptr.assign(1, 0);
    A.tptr.assign(1, 0);
    A.qptr.assign(1, 0);
    for (int64_t i = 0; i < m0; ++i) {
        const uint8_t kind = d->row_kind ? d->row_kind[i] : KTN_ROW_SEP;
        const bool lin = d->row_linear && d->row_linear[i];
        const int side = h_esh_side[(size_t)i];
        // (host-evaluated rows have no program the auxiliary problem can carry and are dropped, and so are the nonlinear QUAD rows
        //  that do not take part; a QUAD row declared linear has an empty Q and goes in as the separable row of LIN atoms it is)
        const bool quad_lin = kind == KTN_ROW_QUAD && lin;
        const bool quad_nl = kind == KTN_ROW_QUAD && !lin && esh_quad_mode();
        if ((kind != KTN_ROW_SEP && kind != KTN_ROW_TAPE && !quad_lin && !quad_nl) || (!lin && side == 0)) continue;
        for (int64_t e = d->rowptr[i]; e < d->rowptr[i + 1]; ++e) {
            A.col.push_back(d->col[e]);
            A.akind.push_back(d->atom_kind && !quad_lin && !quad_nl ? d->atom_kind[e] : 0);
            A.p0.push_back(d->p0 ? d->p0[e] : 0.0);
            A.p1.push_back(d->p1 && !quad_lin && !quad_nl ? d->p1[e] : 0.0);
            if (quad_nl)                                          // the entry's Q segment, re-based
                for (int64_t k = d->quad_ptr[e]; k < d->quad_ptr[e + 1]; ++k) { A.qcol.push_back(d->quad_col[k]); A.qval.push_back(d->quad_val[k]); }
            A.qptr.push_back((int64_t)A.qcol.size());
        }
        if (quad_nl) A.has_quad = true;
        if (kind == KTN_ROW_TAPE) {
            for (int64_t t = d->tape_ptr[i]; t < d->tape_ptr[i + 1]; ++t) { A.top.push_back(d->tape_op[t]); A.targ.push_back(d->tape_arg[t]); }
            A.has_tape = true;
        }
        if (!lin) {                                              // g_i(x) - sigma_i s against the bound
            A.col.push_back(s_col);
            A.akind.push_back(KTN_ATOM_LIN);
            A.p0.push_back(-(double)side);
            A.p1.push_back(0.0);
            A.qptr.push_back((int64_t)A.qcol.size());
            if (kind == KTN_ROW_TAPE) {
                A.top.push_back(KTN_OP_VAR); A.targ.push_back((double)s_col);
                A.top.push_back(side > 0 ? KTN_OP_SUB : KTN_OP_ADD); A.targ.push_back(0.0);
            }
        }
        A.rowptr.push_back((int64_t)A.col.size());
        A.tptr.push_back((int64_t)A.top.size());
        A.kind.push_back(quad_lin ? (uint8_t)KTN_ROW_SEP : kind);
        A.lin.push_back(lin ? 1 : 0);
        A.rconst.push_back(d->rconst ? d->rconst[i] : 0.0);
        A.rows.push_back(i);
        A.lc.push_back(l_constr[i]);
        A.uc.push_back(u_constr[i]);
    }
    A.m = (int64_t)A.kind.size();
    A.ocol.assign(1, s_col); A.okind.assign(1, KTN_ATOM_LIN); A.op0.assign(1, 1.0); A.op1.assign(1, 0.0);
}

// The auxiliary problem on a child engine (cut_algo 0, iter_cap esh_interior_iters, silent).  After round k the child's
// sweep bounds every taking-part row: g_i(x_k) - b_i <= s_k + max(v_k, f_tol) (v_k: its largest violation beyond f_tol); the
// first round with that bound at -10 f_tol or below gives x_int = x_k.
void Engine::esh_find_interior() {
    const auto t0 = std::chrono::steady_clock::now();
    const double delta = 10.0 * prm.f_tol;
    stats["esh_interior_found"] = 0.0;
    stats["esh_interior_rounds"] = 0.0;
    stats["esh_interior_s"] = std::numeric_limits<double>::quiet_NaN();
    const EshAux& A = aux;
    ktn_params cp = prm;
    cp.cut_algo = KTN_CUT_KELLEY; cp.iter_cap = prm.esh_interior_iters; cp.log_level = 0; cp.vis_data = 0; cp.device = device;
    delete child;
    child = nullptr;
    bool ok = false;
    std::vector<double> xk((size_t)A.n, 0.0);
    try {
        child = new Engine(cp, this);
        ktn_nlp_desc dd{};
        dd.num_var = A.n; dd.num_constr = A.m;
        dd.rowptr = A.rowptr.data(); dd.col = A.col.data(); dd.row_kind = A.kind.data(); dd.row_linear = A.lin.data();
        dd.rconst = A.rconst.data(); dd.atom_kind = A.akind.data(); dd.p0 = A.p0.data(); dd.p1 = A.p1.data();
        if (A.has_tape) { dd.tape_ptr = A.tptr.data(); dd.tape_op = A.top.data(); dd.tape_arg = A.targ.data(); }
        if (A.has_quad) { dd.quad_ptr = A.qptr.data(); dd.quad_col = A.qcol.data(); dd.quad_val = A.qval.data(); }
        dd.obj_linear = 1; dd.obj_kind = KTN_ROW_SEP; dd.obj_nnz = 1;
        dd.obj_col = A.ocol.data(); dd.obj_atom_kind = A.okind.data(); dd.obj_p0 = A.op0.data(); dd.obj_p1 = A.op1.data();
        child->loadproblem(A.n, A.m, A.lv.data(), A.uv.data(), A.lc.data(), A.uc.data(), KTN_MIN, &dd);
        child->begin();
        int32_t done = (child->status == KTN_STATUS_ERROR || child->status == KTN_STATUS_UNBOUNDED) ? 1 : 0;
        while (!done && !child->polishing) {
            child->step(&done);
            if (child->lp_status != KTN_STATUS_OPTIMAL || child->status == KTN_STATUS_ERROR || child->status == KTN_STATUS_UNBOUNDED) break;
            double s = 0.0;
            KTN_HIP(hipMemcpyAsync(&s, child->lp_x.p + n0, sizeof(double), hipMemcpyDeviceToHost, child->stream));
            child->sync();
            const double v = child->stats["last_maxviol"];
            stats["esh_interior_rounds"] = (double)child->iter;
            stats["esh_interior_s"] = s;
            if (s + std::max(v, prm.f_tol) <= -delta) {
                child->lp_x.download(xk.data(), (size_t)A.n, child->stream);
                ok = true;
                break;
            }
        }
    } catch (const Error&) {
        ok = false;                               // (no interior point: every row is cut as in Kelley's method)
    }
    delete child;
    child = nullptr;
    if (ok) {
        h_xint.assign(xk.begin(), xk.begin() + n0);
        xint_found = 1;
    }
    stats["esh_interior_found"] = ok ? 1.0 : 0.0;
    stats["esh_interior_time_s"] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// Once per loaded problem (or after ktn_set_interior_point): x_int from the caller or the auxiliary problem, then every row
// evaluated there; a row takes part only where g_i(x_int) is at least 10 f_tol inside its bound.
void Engine::esh_prepare() {
    esh_ready = true;
    xint_found = 0;
    stats["esh_interior_depth"] = std::numeric_limits<double>::quiet_NaN();
    if (esh_n_part == 0 && !xint_given) return;
    if (xint_given) {                                    // the caller's point: used as given
        xint_found = 1;
        stats["esh_interior_found"] = 1.0;
        stats["esh_interior_rounds"] = 0.0;
        stats["esh_interior_s"] = std::numeric_limits<double>::quiet_NaN();
    } else {
        esh_find_interior();
    }
    if (!xint_found) return;
    const double delta = 10.0 * prm.f_tol;
    std::vector<double> xi(h_xint);
    xi.push_back(0.0);
    d_xint.upload(xi, stream);
    precompute_all(d_xint.p);
    const std::vector<double> g = d_g.to_host(stream);
    if (esh_n_quad_part > 0) {                           // the Jacobian at x_int, by Jacobian entry: k_esh_quad interpolates from it
        d_jint.resize((size_t)nnz_ext, stream);
        KTN_HIP(hipMemcpyAsync(d_jint.p, d_jac.p, (size_t)nnz_ext * sizeof(double), hipMemcpyDeviceToDevice, stream));
    }
    std::vector<int8_t> sig((size_t)m_ext, 0);
    double depth = kInf;
    int64_t inside = 0;
    for (int64_t i = 0; i < m0; ++i) {
        const int side = h_esh_side[(size_t)i];
        if (side == 0) continue;
        const double margin = side > 0 ? h_ub[(size_t)i] - g[(size_t)i] : g[(size_t)i] - h_lb[(size_t)i];
        depth = (margin == margin) ? std::min(depth, margin) : -kInf;
        if (margin >= delta) { sig[(size_t)i] = (int8_t)side; ++inside; }
    }
    d_esh_sig.upload(sig, stream);
    d_lam.resize((size_t)m_ext, stream);
    d_esh_cnt.resize(3, stream);
    stats["esh_interior_depth"] = esh_n_part ? depth : kInf;
    stats["esh_interior_rows"] = (double)inside;
    if (have_precompute) precompute_all(d_xs.p);        // (ktn_sep_*: the state of the caller's last precompute)
    sync();
}

// In the sweep, after the selection: the root search of every selected violated row that takes part
void Engine::esh_search(const double* d_x, double f_tol) {
    esh_on = false;
    if (!xint_found) return;
    const auto t0 = std::chrono::steady_clock::now();
    NlpDev P = nlp_view();
    SweepOut O = sweep_view();
    d_esh_cnt.zero(stream);
    launch_n(k_fill, m_ext, stream, m_ext, d_lam.p, 1.0);            // (rows the search leaves alone keep Kelley's cut: lambda 1)
    const EshArgs A{d_x, d_xint.p, d_esh_sig.p, d_lam.p, d_esh_cnt.p, prm.esh_root_tol * f_tol, prm.esh_root_iters, 0};
    with_group(grp_sweep, [&](auto g) { launch(k_esh_sep<g()>, group_grid(m_nl, g()), kBlock, 0, stream, P, d_nlrows.p, m_nl, (const int64_t*)d_flag.p, A, O); });
    if (n_longev_nl > 0)
        launch(k_esh_long, (unsigned)n_longev_nl, 1024, 0, stream, P, d_longev_nlrows.p, d_longev_nlslots.p, (const int64_t*)d_flag.p, A, O);
    launch_n(k_esh_tape, n_tape_nl, stream, P, d_taperows_nl.p, d_tape_nlslots.p, n_tape_nl, (const int64_t*)d_flag.p, A, O);
    if (esh_n_quad_part > 0 && n_quad_nl > 0) {         // (KTN_CUT_SUPPORTING_QUAD; d_jint stands)
        const QuadList QL{d_qrows_nl.p, d_qslots_nl.p, d_qtbase_nl.p, nullptr, n_quad_nl, n_quad_ent_nl};
        with_group(esh_quad_group(), [&](auto g) {
            launch(k_esh_quad<g()>, group_grid(n_quad_nl, g()), kBlock, 0, stream, P, QL, (const int64_t*)d_flag.p, (const double*)d_jint.p, A, O);
        });
    }
    check_launch();
    unsigned long long c[3] = {0ull, 0ull, 0ull};
    KTN_HIP(hipMemcpyAsync(c, d_esh_cnt.p, sizeof(c), hipMemcpyDeviceToHost, stream));
    sync();
    esh_on = true;
    esh_last_rows = (int64_t)c[0];
    stats["esh_rows"] += (double)c[0];
    stats["esh_quad_rows"] += (double)c[2];
    stats["esh_newton_steps"] += (double)c[1];
    stats["esh_root_time_s"] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

void Engine::esh_emit(const double* d_x, int64_t V) {
    NlpDev P = nlp_view();
    LpRows L = lp_view();
    stats["esh_fallback_rows"] += (double)(V - (esh_on ? esh_last_rows : 0));
    if (esh_on)
        with_group(grp_sweep, [&](auto g) {
            launch(k_emit_esh<g()>, group_grid(V, g()), kBlock, 0, stream, P, d_nlrows.p, d_violslots.p, V, d_x, (const double*)d_xint.p,
                   (const double*)d_lam.p, d_jac.p, (const double*)(esh_n_quad_part > 0 ? d_jint.p : nullptr), d_maxc.p, prm.cut_coef_rng, 1, M, L);
        });
    else
        with_group(grp_sweep, [&](auto g) {
            launch(k_emit<g()>, group_grid(V, g()), kBlock, 0, stream, P, d_nlrows.p, d_violslots.p, V, d_x, d_jac.p, d_maxc.p, prm.cut_coef_rng, 1, M, L);
        });
}

// ktn_sep_gencut: row i's cut at the point of the last precompute (d_xs).  Returns true when the row was cut at x_b and writes that
// cut into (coefs, constant); the row's Jacobian entries and cut statistics are put back as the precompute left them, so a
// separator loop pays O(row) per call.
bool Engine::esh_gencut_row(int64_t i, double* coefs, double* constant) {
    if (!esh_ready) esh_prepare();
    if (!xint_found || i < 0 || i >= m0 || h_esh_side[(size_t)i] == 0) return false;
    const uint8_t kind = h_rowkind[(size_t)i];
    if (kind != KTN_ROW_SEP && kind != KTN_ROW_TAPE && !(kind == KTN_ROW_QUAD && esh_quad_mode())) return false;
    const int64_t beg = h_rowptr[(size_t)i], len = h_rowptr[(size_t)i + 1] - beg;
    const bool longrow = !blk_on && kind == KTN_ROW_SEP && len > kLongEval;      // (device kind kRowSepLong: k_sep_eval_long's rows)
    // what the precompute left for row i
    std::vector<double> jac0((size_t)std::max<int64_t>(len, 1));
    double b0 = 0.0, m0v = 0.0;
    int32_t nf0 = 0;
    if (len) KTN_HIP(hipMemcpyAsync(jac0.data(), d_jac.p + beg, (size_t)len * sizeof(double), hipMemcpyDeviceToHost, stream));
    KTN_HIP(hipMemcpyAsync(&b0, d_bconst.p + i, sizeof(double), hipMemcpyDeviceToHost, stream));
    KTN_HIP(hipMemcpyAsync(&m0v, d_maxc.p + i, sizeof(double), hipMemcpyDeviceToHost, stream));
    KTN_HIP(hipMemcpyAsync(&nf0, d_nonfin.p + i, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    NlpDev P = nlp_view();
    SweepOut O = sweep_view();
    d_esh_one.resize(1, stream);
    d_esh_slot.resize(1, stream);
    const int32_t r = (int32_t)i;
    const int64_t sl = 0;
    KTN_HIP(hipMemcpyAsync(d_esh_one.p, &r, sizeof(r), hipMemcpyHostToDevice, stream));
    KTN_HIP(hipMemcpyAsync(d_esh_slot.p, &sl, sizeof(sl), hipMemcpyHostToDevice, stream));
    d_esh_cnt.zero(stream);
    const EshArgs A{d_xs.p, d_xint.p, d_esh_sig.p, d_lam.p, d_esh_cnt.p, prm.esh_root_tol * prm.f_tol, prm.esh_root_iters, 1};
    if (longrow)
        launch(k_esh_long, 1, 1024, 0, stream, P, d_esh_one.p, d_esh_slot.p, (const int64_t*)nullptr, A, O);
    else if (kind == KTN_ROW_TAPE)
        launch_n(k_esh_tape, 1, stream, P, d_esh_one.p, d_esh_one.p, (int64_t)1, (const int64_t*)nullptr, A, O);
    else if (kind == KTN_ROW_QUAD) {
        const QuadList QL{d_esh_one.p, d_esh_slot.p, nullptr, nullptr, 1, len};
        with_group(esh_quad_group(), [&](auto g) {
            launch(k_esh_quad<g()>, group_grid(1, g()), kBlock, 0, stream, P, QL, (const int64_t*)nullptr, (const double*)d_jint.p, A, O);
        });
    }
    else
        with_group(grp_sweep, [&](auto g) { launch(k_esh_sep<g()>, group_grid(1, g()), kBlock, 0, stream, P, d_esh_one.p, (int64_t)1, (const int64_t*)nullptr, A, O); });
    check_launch();
    unsigned long long c[3] = {0ull, 0ull, 0ull};
    KTN_HIP(hipMemcpyAsync(c, d_esh_cnt.p, sizeof(c), hipMemcpyDeviceToHost, stream));
    sync();
    stats["esh_newton_steps"] += (double)c[1];
    const bool moved = c[0] > 0;
    if (moved) {
        if (len) KTN_HIP(hipMemcpyAsync(coefs, d_jac.p + beg, (size_t)len * sizeof(double), hipMemcpyDeviceToHost, stream));
        KTN_HIP(hipMemcpyAsync(constant, d_bconst.p + i, sizeof(double), hipMemcpyDeviceToHost, stream));
    }
    if (len) KTN_HIP(hipMemcpyAsync(d_jac.p + beg, jac0.data(), (size_t)len * sizeof(double), hipMemcpyHostToDevice, stream));
    KTN_HIP(hipMemcpyAsync(d_bconst.p + i, &b0, sizeof(double), hipMemcpyHostToDevice, stream));
    KTN_HIP(hipMemcpyAsync(d_maxc.p + i, &m0v, sizeof(double), hipMemcpyHostToDevice, stream));
    KTN_HIP(hipMemcpyAsync(d_nonfin.p + i, &nf0, sizeof(int32_t), hipMemcpyHostToDevice, stream));
    sync();
    return moved;
}

// lambda of each cut the last sweep appended, in row order (1: Kelley's cut at x*)
void Engine::esh_last_lambdas(double* out) {
    const int64_t V = last_sweep_cuts;
    if (V <= 0) return;
    if (!esh_on) { for (int64_t v = 0; v < V; ++v) out[v] = 1.0; return; }
    std::vector<int32_t> slots((size_t)V);
    d_violslots.download(slots.data(), slots.size(), stream);
    const std::vector<double> lam = d_lam.to_host(stream);
    for (int64_t v = 0; v < V; ++v) out[v] = lam[(size_t)h_nlrows[(size_t)slots[(size_t)v]]];
}

}  // namespace ktn
