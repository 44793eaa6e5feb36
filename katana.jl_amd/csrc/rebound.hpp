// rebound.hpp -- kernels of the re-solve after a change of variable bounds or of a linear cost.
//
//   k_row_activity<G>  the screen: the smallest and the largest value every stored LP row (lp_val, lp_lo, lp_hi: the reference's
//                      form, not the epigraph-shifted working form) can take over the box [l, u], and whether that proves the
//                      row impossible.  G lanes per row as k_spmv<G>; a row beyond kLongRow entries is just more trips of its
//                      lane group's loop (the screen runs once per change of bounds, not once per PDHG iteration).
//   k_rebound          a thread per column: x_j into [l_j, u_j] (a crossed column goes to l_j), moved and crossed columns counted
//   k_obj_coefs        a thread per entry of the objective row: the entry's p0 in the packed atom records
//   k_rebase_cuts      a thread per NL slot: the cuts of the slot's list shifted by the change of its row bounds ("row bounds" below)
//   k_row_owners       a thread per NL slot: the constraint row that owns each cut, by the same walk
//   k_lin_bounds       a thread per caller's row: a linear row's LP bounds from the tangent at the origin
//
// The screen of row k, entries e with coefficient v_e on column c:
//   amin_k = sum_e (v_e > 0 ? v_e l_c : v_e < 0 ? v_e u_c : 0)         amax_k = sum_e (v_e > 0 ? v_e u_c : v_e < 0 ? v_e l_c : 0)
// A zero coefficient contributes 0 whatever the bound; an infinite term makes amin_k = -inf (amax_k = +inf) and stays out of the
// finite sum.  S_k = sum_e of the larger of the entry's two absolute terms that is finite (so S_k bounds the absolute sum of
// either side), and
//   tau_k = tol0 + ((len_k + 2) 2^-52) (S_k + |bound|),        tol0 = lp_tol_floor f_tol,
// each operation rounded once, in this order.  The row proves infeasibility when amin_k - hi_k > tau_k(hi_k) or
// lo_k - amax_k > tau_k(lo_k); it is redundant when amax_k <= hi_k and amin_k >= lo_k.
#pragma once
#include "kernels.hpp"

namespace ktn {

struct ScreenOut {
    double* amin;                 // [m]
    double* amax;                 // [m]
    unsigned long long* cnt;      // [0] proving rows, [1] smallest proving row index (starts at ~0), [2] redundant rows
};

// one side's threshold and decision: `excess` beyond `bound` proves the row impossible
__device__ __forceinline__ bool screen_proves(double excess, double bound, double S, int64_t len, double tol0) {
    const double tau = tol0 + ((double)(len + 2) * 0x1p-52) * (S + fabs(bound));
    return excess > tau;
}

template <int G>
__global__ __launch_bounds__(kBlock) void k_row_activity(int64_t m, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                         const double* __restrict__ val, const double* __restrict__ lo,
                                                         const double* __restrict__ hi, const double* __restrict__ l,
                                                         const double* __restrict__ u, double tol0, ScreenOut O) {
    const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    const int lane = threadIdx.x & (G - 1);
    if (i >= m) return;                                   // (whole lane groups leave: i is the group's)
    const int64_t beg = rowptr[i], end = rowptr[i + 1], len = end - beg;
    double smin = 0.0, smax = 0.0, sabs = 0.0;
    int inf_min = 0, inf_max = 0;
    for (int64_t left = len - lane; left > 0; left -= (int64_t)kLaneU * G) {
        LaneBatch<kLaneU> b;
        lane_load<G, kLaneU>(b, end - left, end, col, val);
        lane_gather2<kLaneU>(b, l, u);
#pragma unroll
        for (int k = 0; k < kLaneU; ++k) {
            const double v = b.v[k];
            if (!b.on[k] || v == 0.0) continue;          // (absent or zero; a NaN coefficient goes on: both terms NaN, both inf flags set, nothing proven)
            const double tl = v * b.g[k], tu = v * b.h[k];
            const double tmin = v > 0.0 ? tl : tu, tmax = v > 0.0 ? tu : tl;
            const bool fmin = fabs(tmin) < __builtin_inf(), fmax = fabs(tmax) < __builtin_inf();
            if (fmin) smin += tmin; else inf_min = 1;
            if (fmax) smax += tmax; else inf_max = 1;
            const double a0 = fmin ? fabs(tmin) : 0.0, a1 = fmax ? fabs(tmax) : 0.0;
            sabs += a0 > a1 ? a0 : a1;
        }
    }
    smin = group_sum<G>(smin); smax = group_sum<G>(smax); sabs = group_sum<G>(sabs);
    inf_min = group_or<G>(inf_min); inf_max = group_or<G>(inf_max);
    if (lane != 0) return;
    const double amin = inf_min ? -__builtin_inf() : smin, amax = inf_max ? __builtin_inf() : smax;
    const double lo_i = lo[i], hi_i = hi[i];
    const bool proving = screen_proves(amin - hi_i, hi_i, sabs, len, tol0) || screen_proves(lo_i - amax, lo_i, sabs, len, tol0);
    const bool redundant = amax <= hi_i && amin >= lo_i;
    O.amin[i] = amin; O.amax[i] = amax;
    if (proving) { atomicAdd(O.cnt, 1ull); atomicMin(O.cnt + 1, (unsigned long long)i); }
    if (redundant) atomicAdd(O.cnt + 2, 1ull);
}

// x_j into [l_j, u_j]; cnt[0] += columns moved, cnt[1] += crossed columns (l_j > u_j: x_j = l_j).  n covers the LP's columns,
// the epigraph variable (bounds -inf, +inf) among them: it never moves.
static __global__ __launch_bounds__(kBlock) void k_rebound(int64_t n, const double* __restrict__ l, const double* __restrict__ u,
                                                           double* __restrict__ x, unsigned long long* __restrict__ cnt) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool moved = false, crossed = false;
    if (j < n) {
        const double lj = l[j], uj = u[j], xj = x[j];
        crossed = lj > uj;
        const double nx = crossed ? lj : (xj < lj ? lj : (xj > uj ? uj : xj));
        moved = !(nx == xj);
        if (moved) x[j] = nx;
    }
    const unsigned long long mv = __ballot(moved), cr = __ballot(crossed);
    if ((threadIdx.x & 63) == 0) {
        if (mv) atomicAdd(cnt, (unsigned long long)__popcll(mv));
        if (cr) atomicAdd(cnt + 1, (unsigned long long)__popcll(cr));
    }
}

// ------------------------------------------------------------------ row bounds (ktn_set_row_bounds) ----
// A cut of NL row i taken at a point with tangent constant b is stored as lo = lb_i - b, hi = ub_i - b (k_compact, k_emit_esh, the
// emit pass of k_ecp_blocks).  The tangent of a convex g_i holds at every level, so the cut for new bounds (lb', ub') is the same
// row with   hi <- hi + (ub' - ub),   lo <- lo + (lb' - lb):   the difference is formed once per NL slot, each operation rounded
// once.  A side whose old and new bound are equal is not written -- two infinite ones included, so no inf - inf is ever formed and
// a zero delta leaves the pool bit for bit.  (An NL row keeps its pattern of finite sides: the setter refuses anything else.)
// Against the bound a fresh cut would get, ub' - b rounded once, the moved one is off by at most 2^-52 (|hi| + |ub' - ub|)
// (tests/test_rowbound_ref.py derives it); every further call adds one rounding of the same size.  That drift is accepted: a
// caller who moves a bound thousands of times and minds the last bits reloads.

// The rows of list s, newest first: every walk of this file goes through here, hence through list_next (kernels.hpp): a link that
// does not strictly descend ends it.  A head at or beyond nrows is not followed (its link slot may not exist).
template <class F>
__device__ __forceinline__ void list_for_each(const int64_t* __restrict__ heads, const int64_t* __restrict__ cut_prev, int64_t s, int64_t nrows, F&& f) {
    for (int64_t r = heads[s]; r >= 0 && r < nrows; r = list_next(cut_prev, r)) f(r);
}

// A thread per NL slot: the cuts of its list move with the slot's row bounds (bounds per extended row, old and new); cnt += rows moved
static __global__ __launch_bounds__(kBlock) void k_rebase_cuts(int64_t m_nl, const int32_t* __restrict__ nl_rows, const int64_t* __restrict__ heads,
                                                               const int64_t* __restrict__ cut_prev, int64_t nrows,
                                                               const double* __restrict__ lb_old, const double* __restrict__ ub_old,
                                                               const double* __restrict__ lb_new, const double* __restrict__ ub_new,
                                                               double* __restrict__ lp_lo, double* __restrict__ lp_hi,
                                                               unsigned long long* __restrict__ cnt) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= m_nl) return;
    const int32_t i = nl_rows[s];
    const double l0 = lb_old[i], l1 = lb_new[i], u0 = ub_old[i], u1 = ub_new[i];
    const bool mlo = !(l0 == l1), mhi = !(u0 == u1);
    if (!mlo && !mhi) return;
    const double dlo = mlo ? l1 - l0 : 0.0, dhi = mhi ? u1 - u0 : 0.0;
    unsigned long long moved = 0;
    list_for_each(heads, cut_prev, s, nrows, [&](int64_t R) {
        if (mlo) lp_lo[R] = lp_lo[R] + dlo;
        if (mhi) lp_hi[R] = lp_hi[R] + dhi;
        ++moved;
    });
    if (moved) atomicAdd(cnt, moved);
}

// A thread per NL slot: owner[R] = the slot's row of the extended structure (the caller's row index; num_constr for the epigraph
// row) for every row R of its list.  The host fills owner with -1 first.
static __global__ __launch_bounds__(kBlock) void k_row_owners(int64_t m_nl, const int32_t* __restrict__ nl_rows, const int64_t* __restrict__ heads,
                                                              const int64_t* __restrict__ cut_prev, int64_t nrows, int64_t* __restrict__ owner) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= m_nl) return;
    const int64_t i = nl_rows[s];
    list_for_each(heads, cut_prev, s, nrows, [&](int64_t R) { owner[R] = i; });
}

// A thread per caller's row: the bounds of a linear row's LP row (rowmap[i] >= 0: that row) from the tangent at the origin in
// (g, jac), b formed as k_lin_rows forms it -- the coefficients are in place since the load and do not depend on the bounds
static __global__ __launch_bounds__(kBlock) void k_lin_bounds(int64_t m0, const int32_t* __restrict__ rowmap, const int64_t* __restrict__ rowptr,
                                                              const double* __restrict__ jac, const double* __restrict__ g,
                                                              const double* __restrict__ lb, const double* __restrict__ ub, int64_t nrows,
                                                              double* __restrict__ lp_lo, double* __restrict__ lp_hi) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m0) return;
    const int64_t r = rowmap[i];
    if (r < 0 || r >= nrows) return;
    const int64_t beg = rowptr[i], len = rowptr[i + 1] - beg;
    double b = g[i];
    for (int64_t e = 0; e < len; ++e) b += -0.0 * jac[beg + e];
    lp_lo[r] = lb[i] - b;
    lp_hi[r] = ub[i] - b;
}

// pp[first + k].x = p0[k] for the ne caller's entries of the objective row (its last entry, -t, stays)
static __global__ __launch_bounds__(kBlock) void k_obj_coefs(int64_t ne, int64_t first, const double* __restrict__ p0, double2* __restrict__ pp,
                                                             double* __restrict__ rconst_row, double rconst) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < ne) pp[first + k].x = p0[k];
    if (k == 0) *rconst_row = rconst;
}

}  // namespace ktn
