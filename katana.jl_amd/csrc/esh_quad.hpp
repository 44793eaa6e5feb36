// esh_quad.hpp -- supporting-hyperplane cuts of KTN_ROW_QUAD rows (cut_algo == KTN_CUT_SUPPORTING_QUAD): the
// boundary point in closed form.
//
// Along x(lambda) = x_int + lambda (x* - x_int) a quadratic row is a scalar quadratic in lambda and its gradient is affine in lambda.
// With d = x* - x_int, mu = 1 - lambda, the Jacobians J* (at x*, in O.jac as the sweep or precompute! wrote it) and J0 (at x_int, kept
// by esh_prepare in `jint`), P1 = sum_e J*_e d_e, P0 = sum_e J0_e d_e and q = P1 - P0 (= d'Qd, as J* - J0 = Q d):
//     phi(lambda) = phi1 - mu sigma P1 + 1/2 mu^2 sigma q,        phi1 = sigma (g* - bound)
// The cut point is where phi = tol / 2, the middle of the window [0, tol] the root searches of esh.hpp accept, so that the rounding
// of the formulas cannot carry the true phi out of it.  With c = phi1 - tol / 2 the smaller root, free of cancellation, is
//     mu = 2 c / (sigma P1 + sqrt((sigma P1)^2 - 2 sigma q c)),    lambda = 1 - mu
// A row moves only when every number is finite, sigma q >= 0 (convex along the segment), sigma P1 > 0, the discriminant is >= 0,
// c > 0 and 0 < lambda < 1; otherwise lam[r] = 1 and nothing else of the row is written: Kelley's cut, bit for bit.  At x_b
//     J_b = esh_quad_coef(lambda, J*, J0),   g_b = g* - mu' P1 + 1/2 mu'^2 q  (mu' = 1 - lambda from the stored lambda),
//     bconst = g_b - sum_e x_b,e J_b,e
// No Q entry is read: 2 x (8 + 8 + 4 + 8 + 8) B per Jacobian entry of a moved row (J*, J0, column, x*, x_int; two passes) and the
// per-row record.  FP64 throughout, no atomics on values, the summation order fixed by G.
//
//   k_esh_quad<G>  G lanes per row over a QuadList (the k_quad_stats layout).  flag == nullptr: every listed row is a candidate.
//                  O.jac keeps J* unless A.materialize (ktn_sep_gencut), so isconstrsat, the certificate and :VisData see x*.
#pragma once
#include "esh.hpp"
#include "quad_rows.hpp"

namespace ktn {

// The scalar part, shared by k_esh_quad and the device-side batch loop (k_ecp_blocks<1> of batch_ecp.hpp): the root from the row's
// two directional derivatives, the move conditions, and g at the cut point.  Every lane of a row's group runs it on the same numbers.
struct EshQuadRoot { double lam, q; bool moved; };
__device__ __forceinline__ EshQuadRoot esh_quad_root(bool live, int sg, double gs, double bound, double tol, double p1, double p0, int nf) {
    const double q = p1 - p0;
    const double phi1 = sg * (gs - bound);
    const double c = phi1 - 0.5 * tol;
    const double sp1 = sg * p1, sq = sg * q;
    const double disc = sp1 * sp1 - 2.0 * sq * c;
    const double mu = 2.0 * c / (sp1 + sqrt(disc));
    const double lam = 1.0 - mu;
    const bool fin = !nf && isfinite(p1) && isfinite(p0) && isfinite(gs) && isfinite(c) && isfinite(disc) && isfinite(mu);
    const bool moved = live && fin && sq >= 0.0 && sp1 > 0.0 && disc >= 0.0 && c > 0.0 && lam > 0.0 && lam < 1.0;
    return EshQuadRoot{lam, q, moved};
}
__device__ __forceinline__ double esh_quad_gb(double gs, double lam, double p1, double q) {
    const double m2 = 1.0 - lam;
    return gs - m2 * p1 + 0.5 * (m2 * m2) * q;
}

template <int G>
__global__ __launch_bounds__(kBlock) void k_esh_quad(NlpDev P, QuadList L, const int64_t* __restrict__ flag,
                                                     const double* __restrict__ jint, EshArgs A, SweepOut O) {
    const int64_t gid = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    const int lane = threadIdx.x & (G - 1);
    // (no early return: every lane takes part in the butterflies of both passes and in the barriers of the counters)
    const bool listed = gid < L.n_rows;
    const int32_t r = listed ? L.rows[gid] : 0;
    const bool cand = listed && (flag == nullptr || flag[L.slots[gid]] != 0);
    const int sg = cand ? (int)A.sig[r] : 0;
    const bool live = sg != 0;
    const int64_t beg = live ? P.rowptr[r] : 0, end = live ? P.rowptr[r + 1] : 0;
    // pass 1: the two directional derivatives
    double p1 = 0.0, p0 = 0.0;
    int nf = 0;
    for (int64_t e = beg + lane; e < end; e += G) {
        const int c = P.col[e];
        const double js = O.jac[e], j0 = jint[e];
        const double d = A.x[c] - A.xi[c];
        p1 += js * d;
        p0 += j0 * d;
        nf |= !(isfinite(js) && isfinite(j0) && isfinite(d));
    }
    p1 = group_sum<G>(p1);
    p0 = group_sum<G>(p0);
    nf = group_or<G>(nf);
    // the root, in registers (every lane of the group on the same numbers)
    const double gs = live ? O.g[r] : 0.0;
    const double bound = sg > 0 ? P.ub[r] : (sg < 0 ? P.lb[r] : 0.0);
    const EshQuadRoot R = esh_quad_root(live, sg, gs, bound, A.tol, p1, p0, nf);
    const double lam = R.lam;
    const bool moved = R.moved;
    // pass 2 (moved rows; the others run an empty range): the cut at x_b
    const int64_t beg2 = moved ? beg : 0, end2 = moved ? end : 0;
    double dot = 0.0, mx = -__builtin_inf();
    for (int64_t e = beg2 + lane; e < end2; e += G) {
        const int cj = P.col[e];
        const double jb = esh_quad_coef(lam, O.jac[e], jint[e]);
        const double xb = esh_point(A.x[cj], A.xi[cj], lam);
        dot += xb * jb;
        mx = nanmax(mx, jb);
        if (A.materialize) O.jac[e] = jb;
    }
    dot = group_sum<G>(dot);
    mx = group_nanmax<G>(mx);
    if (lane == 0 && live) {
        if (moved) {
            const double gb = esh_quad_gb(gs, lam, p1, R.q);
            A.lam[r] = lam;
            O.bconst[r] = gb - dot;
            O.maxc[r] = P.pad_zero[r] ? nanmax(mx, 0.0) : mx;
            O.nonfin[r] = 0;
        } else {
            A.lam[r] = 1.0;
        }
    }
    // the counters, one atomic each per workgroup (one per row puts every row of the launch on the same cache line)
    const int n_moved = __syncthreads_count(lane == 0 && moved), n_live = __syncthreads_count(lane == 0 && live);
    if (threadIdx.x == 0 && n_live > 0) {
        if (n_moved > 0) { atomicAdd(&A.cnt[0], (unsigned long long)n_moved); atomicAdd(&A.cnt[2], (unsigned long long)n_moved); }
        atomicAdd(&A.cnt[1], (unsigned long long)n_live);
    }
}

}  // namespace ktn
