// kkt.hpp -- the NLP-level report of a solve: constraint duals in the caller's row order, reduced costs
// (the gradient of the Lagrangian at the returned point) and the dual bound they certify.  Launched by Engine::kkt_compute
// (sweep.hip) only, on the first ktn_get_constr_duals / ktn_get_reduced_costs / ktn_get_dual_bound after a solve: a solve that is
// followed by no getter launches none of these kernels.
//
// All FP64, no atomics on values, every sum in a fixed order: the results are bit-reproducible for a given lane-group width.
//
//   d_i  linear row: the multiplier of its own LP row; NL row: the sum of the multipliers of the cuts in its list, newest to
//        oldest (the walk of k_cert_nl); 0 for an empty list.  sgn = -1 (sense Max) mirrors the Min problem the LP solves back.
//   z_j  = grad f_j - sum_i d_i J_ij  over the column mirror of the NLP structure (rows ascending: a fixed order)
//   LB   = f - sum_i [d+_i (g_i - lb_i) - d-_i (g_i - ub_i)] - sum_j [z+_j (x_j - l_j) + z-_j (u_j - x_j)]      (Min form)
#pragma once
#include "kernels.hpp"
#include "batch_ecp.hpp"

namespace ktn {

// where the multipliers and the cut lists live: the ordinary LP state (lp_y / md_y, list heads, d_cutprev: global LP row indices)
// or the arenas of the device-side batch loop (e_y, e_last, e_prev: indices local to the instance's arena)
struct KktSrc {
    const double* y;
    const int64_t* heads; const int64_t* prev; int64_t n_heads, n_rows;          // ordinary (n_rows: LP rows now, see kkt_list_sum)
    const int32_t* a_last; const int32_t* a_prev; const EcpArena* arena;         // arenas
    const int64_t* blk_lin; const int64_t* blk_nl; int64_t nb;
};

// the instance that owns position k of a list grouped by instance (off[0..nb]: ascending offsets)
__device__ __forceinline__ int64_t kkt_block_of(const int64_t* __restrict__ off, int64_t nb, int64_t k) {
    int64_t lo = 0, hi = nb;                                                      // off[lo] <= k < off[hi]
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (off[mid] <= k) lo = mid; else hi = mid; }
    return lo;
}

// Keys of the mirror build, one thread per Jacobian ENTRY (the row of an entry by binary search in rowptr): key = (col << 32 | row)
// in CSR order, value = the entry, and the column counts.  (k_csc_keys, G lanes per ROW, walks the objective row -- 1e5 entries on
// cfg3 -- with one lane group: 3.4 ms of the first call.)
static __global__ __launch_bounds__(kBlock) void k_kkt_keys(int64_t nnz, int64_t m, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                     uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, int64_t* __restrict__ colcount) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= nnz) return;
    int64_t lo = 0, hi = m;                                        // rowptr[lo] <= e < rowptr[hi]
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (rowptr[mid] <= e) lo = mid; else hi = mid; }
    const uint32_t c = (uint32_t)col[e];
    keys[e] = ((uint64_t)c << 32) | (uint64_t)(uint32_t)lo;
    vals[e] = (uint32_t)e;
    atomicAdd(reinterpret_cast<unsigned long long*>(&colcount[c]), 1ULL);
}

// Sum of y over one list of the ordinary state, newest to oldest as k_cert_nl walks it.  ktn_lp_truncate moves every list head
// down to the surviving rows (k_list_clip), so a list starts below n_rows; a head that does not is still passed over, and the
// walk ends should a link ever fail to descend (the rule of every list walker: kernels.hpp list_next).
__device__ __forceinline__ double kkt_list_sum(const KktSrc& S, int64_t s) {
    double a = 0.0;
    if (s < 0 || s >= S.n_heads) return a;
    for (int64_t r = S.heads[s]; r >= 0;) {
        if (r < S.n_rows) a += S.y[r];
        const int64_t nx = S.prev[r];
        if (nx >= r) break;
        r = nx;
    }
    return a;
}

// one thread per original row.  rowmap[i] >= 0: the row's position among the linear rows (its LP row in the ordinary state);
// rowmap[i] = -1 - s: NL slot s.  epi (one entry, may be null): the multiplier mass of the epigraph row -- LP rows
// [epi_lo, epi_hi) (the cut at the bound-box vertex) plus the list of slot epi_slot -- written by thread 0.
template <bool ARENA>
__global__ __launch_bounds__(kBlock) void k_row_duals(int64_t m0, const int32_t* __restrict__ rowmap, KktSrc S, double sgn,
                                                      int64_t epi_lo, int64_t epi_hi, int64_t epi_slot, double* __restrict__ epi,
                                                      const double* __restrict__ lb, const double* __restrict__ ub, double* __restrict__ clamped, double* __restrict__ d) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i == 0 && epi != nullptr && !ARENA) {
        double a = kkt_list_sum(S, epi_slot);
        for (int64_t r = epi_hi - 1; r >= epi_lo; --r) a += S.y[r];
        epi[0] = a;
    }
    if (i >= m0) return;
    const int32_t k = rowmap[i];
    double a = 0.0;
    if (ARENA) {
        if (k >= 0) {
            const int64_t b = kkt_block_of(S.blk_lin, S.nb, k);
            a = S.y[S.arena[b].row0 + (k - S.blk_lin[b])];
        } else {
            const int64_t s = -1 - (int64_t)k, b = kkt_block_of(S.blk_nl, S.nb, s);
            const int64_t r0 = S.arena[b].row0;
            const int32_t cap = S.arena[b].cap_rows;
            for (int32_t r = S.a_last[s]; r >= 0 && r < cap;) {
                a += S.y[r0 + r];
                const int32_t nx = S.a_prev[r0 + r];
                if (nx >= r) break;                               // (a list descends: never followed anywhere else)
                r = nx;
            }
        }
    } else {
        if (k >= 0) a = S.y[k];
        else a = kkt_list_sum(S, -1 - (int64_t)k);
        // The residue of prox_y: yt = v + sigma clip(-v / sigma, lo, hi) is v + sigma (-v / sigma) on a slack row, zero up to a
        // rounding error of either sign (1e-18 ... 1e-15 seen).  With the wrong sign it is a multiplier on a side the row does not
        // have, and times that side's infinite bound it makes the dual bound minus infinity.  A row without that side has no
        // such multiplier: the report gives 0.  (a is the Min-form multiplier, as dm in k_dual_terms; the arenas of the
        // device-side loop keep theirs: their aggregation is compared bit for bit with ktn_blocks_get_duals.)
        // Every magnitude is zeroed, so the rule could hide a real sign error of lp_y or of the lists: clamped[0] counts the
        // entries (an integer sum: exact in any order) and clamped[1] keeps the largest |a| (the bits of a non-negative double
        // order like the number), statistics kkt_clamped_duals / kkt_clamped_max, which the tests bound.
        if ((a > 0.0 && !(lb[i] > -__builtin_inf())) || (a < 0.0 && !(ub[i] < __builtin_inf()))) {
            atomicAdd(&clamped[0], 1.0);
            atomicMax(reinterpret_cast<unsigned long long*>(&clamped[1]), (unsigned long long)__double_as_longlong(fabs(a)));
            a = 0.0;
        }
    }
    d[i] = sgn * a;
}

// z_j = grad f_j - sum_i d_i J_ij, G lanes per column of the mirror (cptr / crow / cperm over the EXTENDED structure: the objective
// row m0 is the last entry of its columns and enters with weight exactly 1, never through d).  Consecutive lanes take consecutive
// mirror entries; the loads of a trip (index pair, then the two gathers) are issued before its arithmetic; a column longer than G
// loops (one path for every length: a column of 64 * 8 entries and more simply makes more trips); xor-butterfly; lane 0 writes.
template <int G>
__global__ __launch_bounds__(kBlock) void k_lagr_grad(int64_t n, int32_t m0, const int64_t* __restrict__ cptr, const int32_t* __restrict__ crow,
                                                      const uint32_t* __restrict__ cperm, const double* __restrict__ jac,
                                                      const double* __restrict__ d, double* __restrict__ z) {
    const int64_t j = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    const int lane = threadIdx.x & (G - 1);
    const bool live = j < n;                                     // (every lane of the wavefront reaches the butterfly)
    const int64_t beg = live ? cptr[j] : 0, end = live ? cptr[j + 1] : 0;
    double acc = 0.0, gf = 0.0;
    for (int64_t e = beg + lane; e < end; e += G) {
        const int32_t r = crow[e];
        const uint32_t p = cperm[e];
        const double a = jac[p];
        const double w = (r < m0) ? d[r] : 0.0;
        if (r < m0) acc += w * a; else gf += a;
    }
    acc = group_sum<G>(acc);
    gf = group_sum<G>(gf);
    if (live && lane == 0) z[j] = gf - acc;
}

// The terms of the dual bound in the Min form (dm = sgn d, zm = sgn z): rows into t[0, m0) -- the linear rows first, then the NL
// rows by slot, the order in which a fused batch groups them by instance --, columns into t[m0, m0 + n).  A term with a zero
// multiplier is 0 whatever the bound (0 * inf counts as 0); an infinite bound under a non-zero multiplier gives +inf, which
// makes the bound -inf.
static __global__ __launch_bounds__(kBlock) void k_dual_terms(int64_t m0, int64_t n, double sgn, const int32_t* __restrict__ rowmap, int64_t n_lin,
                                                       const double* __restrict__ d, const double* __restrict__ z,
                                                       const double* __restrict__ g, const double* __restrict__ lb, const double* __restrict__ ub,
                                                       const double* __restrict__ x, const double* __restrict__ l, const double* __restrict__ u,
                                                       double* __restrict__ t) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < m0) {
        const double dm = sgn * d[i];
        double v = 0.0;
        if (dm > 0.0) v = dm * (g[i] - lb[i]);
        else if (dm < 0.0) v = dm * (g[i] - ub[i]);               // = -d-_i (g_i - ub_i)
        const int32_t k = rowmap[i];
        t[k >= 0 ? (int64_t)k : n_lin + (-1 - (int64_t)k)] = v;
    } else if (i < m0 + n) {
        const int64_t j = i - m0;
        const double zm = sgn * z[j];
        double v = 0.0;
        if (zm > 0.0) v = zm * (x[j] - l[j]);
        else if (zm < 0.0) v = -zm * (u[j] - x[j]);
        t[i] = v;
    }
}

// One workgroup per segment s (an instance of a fused batch, or the whole problem): out[2 s] = the sum of the segment's terms
// -- its linear rows, its NL rows, its columns: three ranges of t, each thread-strided, then block_sum (a fixed shape) --,
// out[2 s + 1] = the segment's objective c'x over its columns (obj_c null: 0).  seg: 6 offsets per segment.
static __global__ __launch_bounds__(kBlock) void k_dual_bound(const int64_t* __restrict__ seg, const double* __restrict__ t,
                                                       const double* __restrict__ obj_c, const double* __restrict__ x, int64_t m0,
                                                       double* __restrict__ out) {
    __shared__ double sh[2][kBlock / 64];
    const int64_t* s = seg + 6 * (int64_t)blockIdx.x;
    double v[2] = {0.0, 0.0};
    for (int q = 0; q < 3; ++q)
        for (int64_t i = s[2 * q] + threadIdx.x; i < s[2 * q + 1]; i += kBlock) v[0] += t[i];
    if (obj_c != nullptr)
        for (int64_t i = s[4] + threadIdx.x; i < s[5]; i += kBlock) v[1] += obj_c[i - m0] * x[i - m0];
    block_sum<kBlock>(v, sh);
    if (threadIdx.x == 0) { out[2 * blockIdx.x] = v[0]; out[2 * blockIdx.x + 1] = v[1]; }
}

// the whole problem as ONE segment would leave 255 CUs idle on 1e5 columns: block partials over t (k_sum_partial), then this
// final block adds them in order and writes  out[0] = sum of the terms, out[1] = f = g[m0] + t (the objective row holds f(x) - t).
static __global__ void k_dual_final(const double* __restrict__ partials, int np, const double* __restrict__ g, const double* __restrict__ x,
                             int64_t m0, int64_t n0, double* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double a = 0.0;
    for (int k = 0; k < np; ++k) a += partials[k];
    out[0] = a;
    out[1] = g[m0] + x[n0];
}

}  // namespace ktn
