// rebound.hpp -- kernels of the re-solve after a change of variable bounds or of a linear cost.
//
//   k_row_activity<G>  the screen: the smallest and the largest value every stored LP row (lp_val, lp_lo, lp_hi: the reference's
//                      form, not the epigraph-shifted working form) can take over the box [l, u], and whether that proves the
//                      row impossible.  G lanes per row as k_spmv<G>; a row beyond kLongRow entries is just more trips of its
//                      lane group's loop (the screen runs once per change of bounds, not once per PDHG iteration).
//   k_rebound          a thread per column: x_j into [l_j, u_j] (a crossed column goes to l_j), moved and crossed columns counted
//   k_obj_coefs        a thread per entry of the objective row: the entry's p0 in the packed atom records
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

// pp[first + k].x = p0[k] for the ne caller's entries of the objective row (its last entry, -t, stays)
static __global__ __launch_bounds__(kBlock) void k_obj_coefs(int64_t ne, int64_t first, const double* __restrict__ p0, double2* __restrict__ pp,
                                                             double* __restrict__ rconst_row, double rconst) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < ne) pp[first + k].x = p0[k];
    if (k == 0) *rconst_row = rconst;
}

}  // namespace ktn
