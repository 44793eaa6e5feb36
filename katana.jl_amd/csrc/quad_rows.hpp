// quad_rows.hpp -- KTN_ROW_QUAD rows: g_i(x) = rconst_i + sum_e a_e x_e + 1/2 sum_e x_e s_e,  s_e = sum_{k in seg(e)} q_k x[qcol_k]
// (include/katana_hip.h).  The gradient of such a row is a sparse matrix-vector product, J_e = a_e + s_e (Q_i symmetric, stored in
// full), so the work is laid out over the Jacobian ENTRIES of all QUAD rows, not over the rows: one row of 40 000 entries and
// 1e5 rows of three entries are the same launch.
//
// Device layout (built by Engine::build_quad_rows at load), entries of the QUAD rows numbered t = 0 .. N-1 in row order:
//   qcol i32 [qnnz]   global column of the second factor   } 12 B per Q entry, two coalesced streams; the column itself is stored
//   qval f64 [qnnz]   q_k                                  } (not the Jacobian slot): x is gathered with ONE dependent load
//   qptr i64 [N + 1]  segment of entry t
//   jidx i64 [N]      Jacobian index e of entry t (a_e = pp[e].x, x_e = x[col[e]], jac[e])
//   vterm f64 [N]     scratch: the entry's value term x_e (a_e + 1/2 s_e)
// and per launch list (all QUAD rows for precompute!, the QUAD rows among the NL rows for the sweep):
//   rows i32 [R], slots i64 [R] (NL slot of the row, -1: none), tbase i64 [R] (t of the row's first entry),
//   ent i64 [n_ent] (the t's of the list's rows; NULL: the list is all entries, t = position)
//
//   k_quad_jac<G>     G lanes per entry: lane-strided partial sums over the segment (consecutive lanes, consecutive Q entries),
//                     xor-butterfly, lane 0 writes jac[e] = a_e + s_e and vterm[t].  An empty segment gives jac[e] = a_e.
//   k_quad_stats<G2>  G2 lanes per row: the row tail of kernels.hpp -- a RowAcc over (vterm, jac), g = rconst + sum vterm,
//                     row_store; with flags on also row_verdict by NL slot.
// No atomics on values and a summation order fixed by (G, G2): run-to-run identical.  Rows beyond 8 192 structure entries are
// correct (a lane group just loops) but not specially optimised.
#pragma once
#include "kernels.hpp"

namespace ktn {

struct QuadDev {
    const int32_t* qcol;
    const double* qval;
    const int64_t* qptr;
    const int64_t* jidx;
    double* vterm;
};

struct QuadList {
    const int32_t* rows;
    const int64_t* slots;
    const int64_t* tbase;
    const int64_t* ent;
    int64_t n_rows, n_ent;
};

// What one Jacobian entry contributes, from its linear coefficient a, its segment sum s and x_e: the coefficient J_e = a + s
// and the value term x_e (a + 1/2 s).  Defined once: k_quad_jac and the device-side batch loop (batch_ecp.hpp) both end here.
struct QuadEntry { double jac, vterm; };
__device__ __forceinline__ QuadEntry quad_entry(double a, double s, double xe) { return QuadEntry{a + s, xe * (a + 0.5 * s)}; }

template <int G>
__global__ __launch_bounds__(kBlock) void k_quad_jac(NlpDev P, QuadDev Q, QuadList L, const double* __restrict__ x, SweepOut O) {
    const int64_t gid = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    const int lane = threadIdx.x & (G - 1);
    // (no early return before the butterfly: an inactive group has an empty segment)
    const bool live = gid < L.n_ent;
    const int64_t t = live ? (L.ent ? L.ent[gid] : gid) : 0;
    const int64_t beg = live ? Q.qptr[t] : 0, end = live ? Q.qptr[t + 1] : 0;
    double s = 0.0;
    constexpr int kU = 2;                                  // two trips' loads and gathers in flight, as k_sep_eval
    for (int64_t k = beg + lane; k < end; k += kU * G) {
        int32_t c[kU];
        double q[kU], xv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int64_t ku = k + (int64_t)u * G;
            const bool on = ku < end;
            c[u] = on ? Q.qcol[ku] : -1;
            q[u] = on ? Q.qval[ku] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) xv[u] = c[u] >= 0 ? x[c[u]] : 0.0;
#pragma unroll
        for (int u = 0; u < kU; ++u)
            if (c[u] >= 0) s += q[u] * xv[u];
    }
    s = group_sum<G>(s);
    if (lane == 0 && live) {
        const int64_t e = Q.jidx[t];
        const double a = P.pp[e].x;
        const double xe = x[P.col[e]];
        const QuadEntry qe = quad_entry(a, s, xe);
        O.jac[e] = qe.jac;
        Q.vterm[t] = qe.vterm;
    }
}

template <int G>
__global__ __launch_bounds__(kBlock) void k_quad_stats(NlpDev P, QuadDev Q, QuadList L, const double* __restrict__ x, double f_tol,
                                                       int flags_on, SweepOut O) {
    const int64_t gid = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    const int lane = threadIdx.x & (G - 1);
    // (no early return: every thread takes part in block_max_nonneg at the end)
    const bool live = gid < L.n_rows;
    const int32_t r = live ? L.rows[gid] : 0;
    const int64_t beg = live ? P.rowptr[r] : 0, end = live ? P.rowptr[r + 1] : 0;
    const int64_t tb = live ? L.tbase[gid] : 0;
    RowAcc acc;
    for (int64_t e = beg + lane; e < end; e += G) {
        const double der = O.jac[e];
        const double xv = x[P.col[e]];
        acc.add(Q.vterm[tb + (e - beg)], der, xv);
    }
    acc.template reduce<G>();
    double viol = 0.0;
    if (lane == 0 && live) {
        const double g = acc.g + P.rconst[r];
        row_store(O, r, g, g - acc.dot, acc.mx, acc.nf, P.pad_zero[r]);
        if (flags_on) viol = row_verdict(O, L.slots[gid], end - beg, g, P.lb[r], P.ub[r], f_tol, acc.nf);
    }
    if (flags_on) block_max_nonneg(O.maxviol, viol);
}

}  // namespace ktn
