// esh.hpp -- supporting-hyperplane cuts (cut_algo == KTN_CUT_SUPPORTING / _QUAD): the per-row root search on the
// segment from the interior point x_int to the LP point x*, and the cut emission at the point found.
//
// Row i with side sigma_i (+1: g_i <= ub_i, -1: g_i >= lb_i) and bound b_i:
//     phi_i(lambda) = sigma_i (g_i(x_int + lambda (x* - x_int)) - b_i),   phi_i(0) <= -10 f_tol,   phi_i(1) > f_tol (violated)
// phi_i is convex in lambda, so Newton steps from lambda = 1 stay at or beyond the root; a bracket [lo, hi] catches what rounding
// or a non-finite value does.  The cut is taken at hi, the last point with a finite phi >= 0: a gradient cut there is valid for
// the convex row and cuts x* off strictly, whether the search converged or not.  A row that never reached such a point below
// lambda = 1 keeps its Kelley cut, bit for bit (its cut constant, maximum and Jacobian entries are left as the sweep wrote them).
//
//   k_esh_sep<G>   separable rows, G lanes per row (the k_sep_eval layout); the wavefront loops until all of its rows are done
//   k_esh_long     rows of k_sep_eval_long, one 1 024-thread workgroup per row
//   k_esh_tape     tape rows, one lane per row through tape_row_eval
//   k_emit_esh<G>  k_emit with the separable derivatives taken at x_b (tape and long rows: their Jacobian, written at x_b; QUAD rows
//                  that k_esh_quad of esh_quad.hpp moved: the Jacobian interpolated between x_int and x*)
#pragma once
#include "kernels.hpp"

namespace ktn {

struct EshArgs {
    const double* x;               // x* (the LP point of the sweep)
    const double* xi;              // x_int
    const int8_t* sig;             // per extended row: sigma_i when row i takes part (x_int at least 10 f_tol inside), else 0
    double* lam;                   // per extended row: lambda of the row's cut (1: Kelley's cut at x*; set to 1 before a sweep's search)
    unsigned long long* cnt;       // [0] rows cut at x_b, [1] evaluation passes, [2] QUAD rows among [0] (k_esh_quad)
    double tol;                    // stop once 0 <= phi <= tol
    int iters;                     // passes per row at most
    int materialize;               // separable rows: also write the Jacobian at x_b (ktn_sep_gencut)
};

// Bracketed Newton on phi (identical in the three kernels; every lane / thread that holds a row runs it on the same numbers)
struct EshState {
    double lo, hi, lam, best;
    bool have, done;
};
__device__ __forceinline__ void esh_init(EshState& s) { s.lo = 0.0; s.hi = 1.0; s.lam = 1.0; s.best = 1.0; s.have = false; s.done = false; }
// phi, dphi at s.lam; fin: phi and every derivative of the row finite.  Returns true when s.lam became the cut point.
__device__ __forceinline__ bool esh_step(EshState& s, double phi, double dphi, bool fin, double tol) {
    bool acc = false;
    if (!(phi < 0.0)) {                        // phi >= 0, +inf or NaN: the root lies below lambda
        s.hi = s.lam;
        if (fin && s.lam < 1.0) { s.best = s.lam; s.have = true; acc = true; }
        if (fin && phi <= tol) { s.done = true; return acc; }
    } else {
        s.lo = s.lam;
    }
    double nl = s.lam - phi / dphi;
    if (!(fin && dphi > 0.0 && isfinite(nl) && nl > s.lo && nl < s.hi)) nl = 0.5 * (s.lo + s.hi);
    s.lam = nl;
    return acc;
}
// the point on the segment; lambda == 1 reads x* itself
__device__ __forceinline__ double esh_point(double xs, double x0, double lam) { return (lam == 1.0) ? xs : x0 + lam * (xs - x0); }

// A QUAD row's gradient is affine in x, so at x_b it is the interpolation of the Jacobians at x_int (j0) and x* (js).  k_esh_quad
// (maximum, cut constant, ktn_sep_gencut) and k_emit_esh (the LP row) both take a coefficient from here: the same bits.
__device__ __forceinline__ double esh_quad_coef(double lam, double js, double j0) { return fma(lam, js - j0, j0); }

// separable rows: G lanes per row.  rows[k] is NL slot k's row; flag == nullptr: every listed row is a candidate.
template <int G>
__global__ __launch_bounds__(kBlock) void k_esh_sep(NlpDev P, const int32_t* __restrict__ rows, int64_t n,
                                                    const int64_t* __restrict__ flag, EshArgs A, SweepOut O) {
    const int64_t gid = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    const int lane = threadIdx.x & (G - 1);
    // (no early return: every lane of the wavefront takes part in the butterflies and the ballot)
    const int32_t r = gid < n ? rows[gid] : 0;
    const bool sep = gid < n && (flag == nullptr || flag[gid] != 0) && P.row_kind[r] == KTN_ROW_SEP;
    const int sg = sep ? (int)A.sig[r] : 0;
    bool active = sg != 0;
    const int64_t beg = active ? P.rowptr[r] : 0, end = active ? P.rowptr[r + 1] : 0;
    const double bound = sg > 0 ? P.ub[r] : (sg < 0 ? P.lb[r] : 0.0);
    const double rc = active ? P.rconst[r] : 0.0;
    EshState S;
    esh_init(S);
    double gb = 0.0, dotb = 0.0, mxb = 0.0;
    unsigned long long passes = 0;
    for (int it = 0; it < A.iters; ++it) {
        if (__ballot(active) == 0ull) break;          // uniform trip count per wavefront; finished groups sit predicated off
        const double lam = S.lam;
        RowAcc acc;
        double acc_d = 0.0;                            // the directional derivative sum der_c (x*_c - x_int_c), beside the row's statistics
        for (int64_t e = beg + lane; active && e < end; e += G) {
            const int ck = P.colk[e];
            const double2 q = P.pp[e];
            const int c = ck & kColMask;
            const double xs = A.x[c], x0 = A.xi[c];
            const double xv = esh_point(xs, x0, lam);
            double val, der;
            atom_eval((unsigned)ck >> kKindShift, q.x, q.y, xv, val, der);
            acc.add(val, der, xv);
            acc_d += der * (xs - x0);
        }
        acc.template reduce<G>();
        acc_d = group_sum<G>(acc_d);
        if (active) {
            const double g = acc.g + rc;
            const double phi = sg * (g - bound), dphi = sg * acc_d;
            ++passes;
            if (esh_step(S, phi, dphi, !acc.nf && isfinite(phi), A.tol)) { gb = g; dotb = acc.dot; mxb = acc.mx; }
            if (S.done) active = false;
        }
    }
    if (A.materialize && S.have) {
        for (int64_t e = P.rowptr[r] + lane; e < P.rowptr[r + 1]; e += G) {
            const int ck = P.colk[e];
            const double2 q = P.pp[e];
            const int c = ck & kColMask;
            double val, der;
            atom_eval((unsigned)ck >> kKindShift, q.x, q.y, esh_point(A.x[c], A.xi[c], S.best), val, der);
            O.jac[e] = der;
        }
    }
    if (lane == 0 && sep) {
        if (S.have) {
            A.lam[r] = S.best;
            row_store_cut(O, r, gb - dotb, mxb, 0, P.pad_zero[r]);
            atomicAdd(&A.cnt[0], 1ull);
        } else {
            A.lam[r] = 1.0;
        }
        if (passes) atomicAdd(&A.cnt[1], passes);
    }
}

// rows of k_sep_eval_long (device kind kRowSepLong): one workgroup per row, the Jacobian written at x_b
static __global__ __launch_bounds__(1024) void k_esh_long(NlpDev P, const int32_t* __restrict__ rows, const int64_t* __restrict__ slots,
                                                   const int64_t* __restrict__ flag, EshArgs A, SweepOut O) {
    __shared__ double sh[16][4];
    __shared__ int shn[16];
    const int32_t r = rows[blockIdx.x];
    const int64_t slot = slots[blockIdx.x];
    const int sg = (int)A.sig[r];
    if (sg == 0 || (flag != nullptr && (slot < 0 || flag[slot] == 0))) return;      // (uniform over the workgroup)
    const int64_t beg = P.rowptr[r], end = P.rowptr[r + 1];
    const double bound = sg > 0 ? P.ub[r] : P.lb[r];
    const int wv = threadIdx.x >> 6;
    // one pass at lambda: every thread ends with the same totals (partials combined in wavefront order)
    auto pass = [&](double lam, bool write, RowAcc& t, double& d) {
        RowAcc a;
        double ad = 0.0;
        for (int64_t e = beg + threadIdx.x; e < end; e += 1024) {
            const int ck = P.colk[e];
            const double2 q = P.pp[e];
            const int c = ck & kColMask;
            const double xs = A.x[c], x0 = A.xi[c];
            const double xv = esh_point(xs, x0, lam);
            double val, der;
            atom_eval((unsigned)ck >> kKindShift, q.x, q.y, xv, val, der);
            a.add(val, der, xv); ad += der * (xs - x0);
            if (write) O.jac[e] = der;
        }
        a.reduce<64>(); ad = group_sum<64>(ad);
        if ((threadIdx.x & 63) == 0) { sh[wv][0] = a.g; sh[wv][1] = ad; sh[wv][2] = a.dot; sh[wv][3] = a.mx; shn[wv] = a.nf; }
        __syncthreads();
        t = RowAcc{sh[0][0], sh[0][2], sh[0][3], shn[0]}; d = sh[0][1];
        for (int k = 1; k < 16; ++k) { t.merge(RowAcc{sh[k][0], sh[k][2], sh[k][3], shn[k]}); d += sh[k][1]; }
        t.g += P.rconst[r];
        __syncthreads();                             // (the cells are reused by the next pass)
    };
    EshState S;
    esh_init(S);
    unsigned long long passes = 0;
    for (int it = 0; it < A.iters && !S.done; ++it) {
        RowAcc t;
        double d;
        pass(S.lam, false, t, d);
        ++passes;
        esh_step(S, sg * (t.g - bound), sg * d, !t.nf && isfinite(t.g), A.tol);
    }
    if (S.have) {
        RowAcc t;
        double d;
        pass(S.best, true, t, d);
        if (threadIdx.x == 0) {
            A.lam[r] = S.best;
            row_store_cut(O, r, t.g - t.dot, t.mx, t.nf, P.pad_zero[r]);
            atomicAdd(&A.cnt[0], 1ull);
        }
    }
    if (threadIdx.x == 0) atomicAdd(&A.cnt[1], passes);
}

// tape rows: one lane per row; the Jacobian is left at x_b (a cut) or re-evaluated at x* (no cut: Kelley's entries again)
static __global__ __launch_bounds__(kBlock) void k_esh_tape(NlpDev P, const int32_t* __restrict__ rows, const int32_t* __restrict__ slots,
                                                     int64_t n, const int64_t* __restrict__ flag, EshArgs A, SweepOut O) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const int32_t r = rows[t];
    if (flag != nullptr && flag[slots[t]] == 0) return;
    const int sg = (int)A.sig[r];
    if (sg == 0 || P.row_kind[r] != KTN_ROW_TAPE) return;
    const double bound = sg > 0 ? P.ub[r] : P.lb[r];
    const int64_t beg = P.rowptr[r], end = P.rowptr[r + 1];
    EshState S;
    esh_init(S);
    unsigned long long passes = 0;
    for (int it = 0; it < A.iters && !S.done; ++it) {
        const double lam = S.lam;
        const double g = tape_row_eval(P, r, [&](int32_t c) { return esh_point(A.x[c], A.xi[c], lam); }, O.jac);
        double d = 0.0;
        int nf = 0;
        for (int64_t e = beg; e < end; ++e) {
            const int c = P.col[e];
            const double der = O.jac[e];
            d += der * (A.x[c] - A.xi[c]);
            nf |= !isfinite(der);
        }
        ++passes;
        esh_step(S, sg * (g - bound), sg * d, !nf && isfinite(g), A.tol);
    }
    if (passes) atomicAdd(&A.cnt[1], passes);
    if (!S.have) {
        if (passes) (void)tape_row_eval(P, r, [&](int32_t c) { return A.x[c]; }, O.jac);
        return;
    }
    const double lb = S.best;
    const double g = tape_row_eval(P, r, [&](int32_t c) { return esh_point(A.x[c], A.xi[c], lb); }, O.jac);
    const RowJacStats st = row_jac_stats(g, beg, end, [&](int64_t e) { return O.jac[e]; },
                                         [&](int64_t e) { return esh_point(A.x[P.col[e]], A.xi[P.col[e]], lb); });
    A.lam[r] = lb;
    row_store_cut(O, r, st.bconst, st.mx, st.nf, P.pad_zero[r]);
    atomicAdd(&A.cnt[0], 1ull);
}

// emit_rows (as k_emit) with the separable derivatives at x_b = x_int + lam[r] (x* - x_int); jint (the Jacobian
// at x_int by Jacobian entry) is NULL unless QUAD rows take part
template <int G>
__global__ __launch_bounds__(kBlock) void k_emit_esh(NlpDev P, const int32_t* __restrict__ nl_rows,
                                                     const int32_t* __restrict__ viol_slots, int64_t n_viol,
                                                     const double* __restrict__ x, const double* __restrict__ xi,
                                                     const double* __restrict__ lam, const double* __restrict__ jac,
                                                     const double* __restrict__ jint, const double* __restrict__ maxc, double cut_coef_rng, int round_coefs,
                                                     int64_t base_row, LpRows L) {
    emit_rows<G>(P, nl_rows, viol_slots, n_viol, maxc, cut_coef_rng, round_coefs, base_row, L, [&](int32_t r) {
        const bool sep = P.row_kind[r] == KTN_ROW_SEP;
        const bool quad = jint != nullptr && P.row_kind[r] == KTN_ROW_QUAD && lam[r] < 1.0;
        const double lr = (sep || quad) ? lam[r] : 1.0;
        return [&P, x, xi, jac, jint, sep, quad, lr](int64_t e, int c) {
            return sep ? sep_entry_der(P, e, esh_point(x[c], xi[c], lr)) : quad ? esh_quad_coef(lr, jac[e], jint[e]) : jac[e];
        };
    });
}

}  // namespace ktn
