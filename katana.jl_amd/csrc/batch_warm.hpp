// batch_warm.hpp -- throughput mode, warm re-solve of a resident batch (DESIGN.md section 14 "In the device-side loop"):
// k_blocks_rewarm does, per instance and inside one workgroup, everything that has to happen between two launches of
// k_ecp_blocks on the same arenas; k_ecp_blocks<ESH, ..., EcpWarm> (batch_ecp.hpp) then starts from what is left there.
//
// For instance b, in this order (tests/blocks_warm_ref.py states the same in plain Python):
//   (a) eligibility   warm only if the last launch's record says :Optimal without overflow; otherwise state 0 (cold), nothing touched
//   (b) crossed box   any l_j > u_j: state 2 (infeasible), nothing else touched
//   (c) clamp         the instance's slice of x into [l, u]; columns moved are counted
//   (d) screen        every arena row, linear rows and cuts, against the box: the test of k_row_activity (rebound.hpp: amin_k,
//                     amax_k, S_k, tau_k), kWarmG lanes per row, each lane its entries in ascending order, then the butterfly.
//                     A proving row: state 2, the smallest one recorded; redundant rows are counted, not removed
//   (e) compaction    only when the cut rows fill more than half of the cut room, M - m_lin > (cap_rows - m_lin) / 2: a cut row
//                     that is idle by the pool's rule (Purge (a), without ageing: y == 0 and
//                     slack > purge_margin * scale at the clamped x) goes, the survivors keep their order (a workgroup prefix scan
//                     over the keep flags), last_cut / cut_prev are re-threaded over them.  Linear rows never move.  A dropped row
//                     has y == 0, so every list's multiplier sum is what it was.
//   (f) record        eight doubles: state, M, NNZ, rows dropped, columns clamped, first proving row (-1), crossed columns,
//                     redundant rows; slot 6 (LP rows) of the instance's launch record follows M, slot 5 (the largest violation
//                     the last solve ended with) stays: the warm entry takes its first LP tolerance from it.
//
// Nothing is moved in place while another lane may still read it: the entries go through crow / cval (the column mirror, rebuilt
// at the top of every cutting-plane round), destinations, new links and new entry offsets are written into dr / loh / hih (per-row
// scalings, rebuilt there too) before any row moves, and the per-row arrays move trip by trip -- all lanes read, barrier, all lanes
// write -- which is safe because a destination is never above its source.
#pragma once
#include "batch_ecp.hpp"
#include "rebound.hpp"

namespace ktn {

constexpr int kWarmG = 4;        // lanes per arena row (the row loops of k_ecp_blocks use the same)

struct WarmBatch {
    const int64_t* blk_col; const int64_t* blk_lin; const int64_t* blk_nl;      // [nb + 1] each, as EcpBatch
    const EcpArena* arena;
    int32_t* rptr; uint16_t* rcol; double* rval; double* lo; double* hi; double* y;
    double* lam;                     // NULL unless the last launch was k_ecp_blocks<1> (or the host filled it with 1)
    int32_t* last_cut; int32_t* cut_prev;
    uint16_t* crow; double* cval;    // staging of the entries
    double* dr; double* loh; double* hih;      // per-row scratch, read as int32: new link, destination, new entry offset
    const double* l; const double* u; double* x;
    double* res;                     // [nb * 8] records of the last launch: read; slot 6 updated
    double* out;                     // [nb * 8] the rewarm records
    double tol0, purge_margin;       // lp_tol_floor * f_tol (the screen's tol0), ktn_params.purge_margin
};

// exclusive prefix sums (pa, pb) of (a, b) over the workgroup in thread order and the totals (ta, tb); sh: 2 * 16 ints
__device__ __forceinline__ void warm_scan2(int a, int b, int& pa, int& pb, int& ta, int& tb, int* sh) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int ia = a, ib = b;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int va = __shfl_up(ia, off, 64), vb = __shfl_up(ib, off, 64);
        if (lane >= off) { ia += va; ib += vb; }
    }
    if (lane == 63) { sh[wv] = ia; sh[16 + wv] = ib; }
    __syncthreads();
    int ba = 0, bb = 0;
    ta = 0; tb = 0;
    for (int k = 0; k < kEcpThreads / 64; ++k) {
        const int sa = sh[k], sb = sh[16 + k];
        if (k < wv) { ba += sa; bb += sb; }
        ta += sa; tb += sb;
    }
    pa = ba + ia - a; pb = bb + ib - b;
    __syncthreads();                 // (sh is free for the next trip)
}

// the first kept row at or below p along the old links (strictly descending, so the walk ends), as its NEW index; -1: none
__device__ __forceinline__ int warm_relink(int p, int m_lin, const int32_t* cut_prev, const int32_t* dst) {
    while (p >= m_lin && dst[p] < 0) {
        const int q = cut_prev[p];
        p = q < p ? q : -1;
    }
    return p >= m_lin ? dst[p] : -1;
}

static __global__ __launch_bounds__(kEcpThreads) void k_blocks_rewarm(WarmBatch W) {
    static_assert(kEcpThreads / 64 <= 16, "warm_scan2 keeps one total per wavefront in 16 cells");
    __shared__ int s_i[8];           // 0 crossed columns, 1 clamped columns, 2 proving rows, 3 smallest proving row, 4 redundant rows
    __shared__ int s_scan[32];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t c0 = W.blk_col[b];
    const int nb = (int)(W.blk_col[b + 1] - c0);
    const int m_lin = (int)(W.blk_lin[b + 1] - W.blk_lin[b]);
    const int64_t nl0 = W.blk_nl[b];
    const int m_nl = (int)(W.blk_nl[b + 1] - nl0);
    const EcpArena A = W.arena[b];
    int32_t* rptr = W.rptr + A.row0 + b;
    uint16_t* rcol = W.rcol + A.nnz0;
    double* rval = W.rval + A.nnz0;
    double* lo = W.lo + A.row0; double* hi = W.hi + A.row0; double* yv = W.y + A.row0;
    double* lam = W.lam ? W.lam + A.row0 : nullptr;
    int32_t* last_cut = W.last_cut + nl0;
    int32_t* cut_prev = W.cut_prev + A.row0;
    uint16_t* crow = W.crow + A.nnz0;
    double* cval = W.cval + A.nnz0;
    int32_t* nprev = reinterpret_cast<int32_t*>(W.dr + A.row0);       // (cap_rows doubles each: room for cap_rows ints)
    int32_t* dst = reinterpret_cast<int32_t*>(W.loh + A.row0);
    int32_t* noff = reinterpret_cast<int32_t*>(W.hih + A.row0);
    const double* ll = W.l + c0; const double* uu = W.u + c0;
    double* xg = W.x + c0;
    double* prev = W.res + (int64_t)b * 8;
    double* o = W.out + (int64_t)b * 8;

    // ---- (a) eligibility
    const int M = (int)prev[6];
    const bool in_range = M >= m_lin && M <= A.cap_rows;
    if (!((int)prev[0] == KTN_STATUS_OPTIMAL && prev[7] == 0.0 && in_range)) {
        if (tid == 0) {
            o[0] = 0.0; o[1] = (double)M; o[2] = in_range ? (double)rptr[M] : 0.0; o[3] = 0.0; o[4] = 0.0; o[5] = -1.0; o[6] = 0.0; o[7] = 0.0;
        }
        return;
    }
    const int NNZ = rptr[M];
    if (tid < 8) s_i[tid] = tid == 3 ? 0x7fffffff : 0;
    __syncthreads();

    // ---- (b) crossed columns
    {
        int cr = 0;
        for (int j = tid; j < nb; j += kEcpThreads) cr += ll[j] > uu[j] ? 1 : 0;
        if (cr) atomicAdd(&s_i[0], cr);
    }
    __syncthreads();
    const int crossed = s_i[0];
    if (crossed > 0) {
        if (tid == 0) {
            o[0] = 2.0; o[1] = (double)M; o[2] = (double)NNZ; o[3] = 0.0; o[4] = 0.0; o[5] = -1.0; o[6] = (double)crossed; o[7] = 0.0;
        }
        return;
    }

    // ---- (c) clamp (k_rebound's rule)
    {
        int mv = 0;
        for (int j = tid; j < nb; j += kEcpThreads) {
            const double lj = ll[j], uj = uu[j], xj = xg[j];
            const double nx = xj < lj ? lj : (xj > uj ? uj : xj);
            if (!(nx == xj)) { xg[j] = nx; ++mv; }
        }
        if (mv) atomicAdd(&s_i[1], mv);
    }

    // ---- (d) screen of every arena row (reads l, u and the rows: not x)
    const int lane = tid & (kWarmG - 1);
    for (int r = tid / kWarmG; r < M; r += kEcpThreads / kWarmG) {
        const int beg = rptr[r], end = rptr[r + 1];
        double smin = 0.0, smax = 0.0, sabs = 0.0;
        int inf_min = 0, inf_max = 0;
        for (int e = beg + lane; e < end; e += kWarmG) {
            const double v = rval[e];
            if (v == 0.0) continue;
            const int cl = rcol[e];
            const double tl = v * ll[cl], tu = v * uu[cl];
            const double tmin = v > 0.0 ? tl : tu, tmax = v > 0.0 ? tu : tl;
            const bool fmin = fabs(tmin) < __builtin_inf(), fmax = fabs(tmax) < __builtin_inf();
            if (fmin) smin += tmin; else inf_min = 1;
            if (fmax) smax += tmax; else inf_max = 1;
            const double a0 = fmin ? fabs(tmin) : 0.0, a1 = fmax ? fabs(tmax) : 0.0;
            sabs += a0 > a1 ? a0 : a1;
        }
        smin = group_sum<kWarmG>(smin); smax = group_sum<kWarmG>(smax); sabs = group_sum<kWarmG>(sabs);
        inf_min = group_or<kWarmG>(inf_min); inf_max = group_or<kWarmG>(inf_max);
        if (lane == 0) {
            const double amin = inf_min ? -__builtin_inf() : smin, amax = inf_max ? __builtin_inf() : smax;
            const double lo_r = lo[r], hi_r = hi[r];
            const int64_t len = end - beg;
            if (screen_proves(amin - hi_r, hi_r, sabs, len, W.tol0) || screen_proves(lo_r - amax, lo_r, sabs, len, W.tol0)) {
                atomicAdd(&s_i[2], 1); atomicMin(&s_i[3], r);
            }
            if (amax <= hi_r && amin >= lo_r) atomicAdd(&s_i[4], 1);
        }
    }
    __syncthreads();                 // (the clamped x is every lane's from here on)
    const int clamped = s_i[1], proving = s_i[2], first = s_i[3], redundant = s_i[4];
    if (proving > 0) {
        if (tid == 0) {
            o[0] = 2.0; o[1] = (double)M; o[2] = (double)NNZ; o[3] = 0.0; o[4] = (double)clamped; o[5] = (double)first; o[6] = 0.0;
            o[7] = (double)redundant;
        }
        return;
    }

    // ---- (e) compaction of the cut rows
    int Mn = M, NNZn = NNZ;
    if (M - m_lin > (A.cap_rows - m_lin) / 2) {
        // keep flags into dst: the pool's idle rule at the clamped x
        for (int r = m_lin + tid / kWarmG; r < M; r += kEcpThreads / kWarmG) {
            double ax = 0.0;
            for (int e = rptr[r] + lane; e < rptr[r + 1]; e += kWarmG) ax += rval[e] * xg[rcol[e]];
            ax = group_sum<kWarmG>(ax);
            if (lane == 0) {
                double slack = __builtin_inf(), scale = 1.0;
                if (isfinite(hi[r])) { slack = fmin(slack, hi[r] - ax); scale = fmax(scale, fabs(hi[r])); }
                if (isfinite(lo[r])) { slack = fmin(slack, ax - lo[r]); scale = fmax(scale, fabs(lo[r])); }
                const bool idle = (yv[r] == 0.0) && (slack > W.purge_margin * scale);
                dst[r] = idle ? 0 : 1;
            }
        }
        __syncthreads();
        // destinations and entry offsets of the survivors: exclusive scan over the cut rows, 1 024 per trip
        int carry_k = 0, carry_n = rptr[m_lin];
        for (int base = m_lin; base < M; base += kEcpThreads) {
            const int r = base + tid;
            const int k = r < M ? dst[r] : 0;
            const int len = k ? rptr[r + 1] - rptr[r] : 0;
            int pk, pl, tk, tl;
            warm_scan2(k, len, pk, pl, tk, tl, s_scan);
            if (r < M) { noff[r] = carry_n + pl; dst[r] = k ? m_lin + carry_k + pk : -1; }
            carry_k += tk; carry_n += tl;
        }
        __syncthreads();
        Mn = m_lin + carry_k; NNZn = carry_n;
        if (Mn < M) {
            // the lists over the survivors, from the old links and in new indices
            for (int r = m_lin + tid; r < M; r += kEcpThreads)
                if (dst[r] >= 0) { const int p = cut_prev[r]; nprev[r] = warm_relink(p < r ? p : -1, m_lin, cut_prev, dst); }
            for (int i = tid; i < m_nl; i += kEcpThreads) { const int p = last_cut[i]; last_cut[i] = warm_relink(p < M ? p : -1, m_lin, cut_prev, dst); }
            // the entries: staged, then written to their new places
            for (int e = rptr[m_lin] + tid; e < NNZ; e += kEcpThreads) { crow[e] = rcol[e]; cval[e] = rval[e]; }
            __syncthreads();
            for (int r = m_lin + tid / kWarmG; r < M; r += kEcpThreads / kWarmG) {
                if (dst[r] < 0) continue;
                const int s = rptr[r], len = rptr[r + 1] - s, d = noff[r];
                for (int e = lane; e < len; e += kWarmG) { rcol[d + e] = crow[s + e]; rval[d + e] = cval[s + e]; }
            }
            __syncthreads();
            // the per-row arrays, trip by trip: a destination is never above its source
            for (int base = m_lin; base < M; base += kEcpThreads) {
                const int r = base + tid;
                const int d = r < M ? dst[r] : -1;
                double v_lo = 0.0, v_hi = 0.0, v_y = 0.0, v_lam = 1.0;
                int v_prev = -1, v_off = 0;
                if (d >= 0) {
                    v_lo = lo[r]; v_hi = hi[r]; v_y = yv[r]; v_prev = nprev[r]; v_off = noff[r];
                    if (lam) v_lam = lam[r];
                }
                __syncthreads();
                if (d >= 0) {
                    lo[d] = v_lo; hi[d] = v_hi; yv[d] = v_y; cut_prev[d] = v_prev; rptr[d] = v_off;
                    if (lam) lam[d] = v_lam;
                }
                __syncthreads();
            }
            if (tid == 0) rptr[Mn] = NNZn;
        }
    }

    // ---- (f) record
    if (tid == 0) {
        o[0] = 1.0; o[1] = (double)Mn; o[2] = (double)NNZn; o[3] = (double)(M - Mn); o[4] = (double)clamped; o[5] = -1.0; o[6] = 0.0;
        o[7] = (double)redundant;
        prev[6] = (double)Mn;
    }
}

// ---- ktn_set_row_bounds on resident arenas (rebound.hpp "row bounds"; Engine::blocks_rebase).  Per instance, one workgroup:
//   linear rows   lo / hi of arena rows [0, m_lin) are copied from the handle's lp_lo / lp_hi, which the setter has just worked out again
//   cut rows      every row of the list of NL slot i moves by the change of that slot's row bounds: hi + (ub' - ub), lo + (lb' - lb),
//                 the difference formed once per slot, a side whose old and new bound are equal not written (k_rebase_cuts' arithmetic)
// M is the row count of the instance's launch record; outside [m_lin, cap_rows] (no launch ended there) the cut rows are left alone --
// k_blocks_rewarm then calls the instance cold.  The walk follows last_cut / cut_prev and ends at a link that does not strictly descend.
struct RebaseBatch {
    const int64_t* blk_lin; const int64_t* blk_nl;      // [nb + 1] each, as EcpBatch
    const EcpArena* arena;
    const int32_t* nl_rows;                              // the engine's NL row list
    const double* lp_lo; const double* lp_hi;            // the loaded LP: the linear rows of every instance
    const double* lb_old; const double* ub_old; const double* lb_new; const double* ub_new;      // per extended row
    double* lo; double* hi;
    const int32_t* last_cut; const int32_t* cut_prev;
    const double* res;                                   // [nb * 8] records of the last launch (slot 6: LP rows)
    unsigned long long* cnt;                             // += cut rows moved
};

static __global__ __launch_bounds__(kEcpThreads) void k_blocks_rebase(RebaseBatch W) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t lin0 = W.blk_lin[b];
    const int m_lin = (int)(W.blk_lin[b + 1] - lin0);
    const int64_t nl0 = W.blk_nl[b];
    const int m_nl = (int)(W.blk_nl[b + 1] - nl0);
    const EcpArena A = W.arena[b];
    double* lo = W.lo + A.row0; double* hi = W.hi + A.row0;
    const int32_t* last_cut = W.last_cut + nl0;
    const int32_t* cut_prev = W.cut_prev + A.row0;
    for (int r = tid; r < m_lin && r < A.cap_rows; r += kEcpThreads) { lo[r] = W.lp_lo[lin0 + r]; hi[r] = W.lp_hi[lin0 + r]; }
    const int M = (int)W.res[(int64_t)b * 8 + 6];
    if (!(M >= m_lin && M <= A.cap_rows)) return;
    unsigned long long moved = 0;
    for (int i = tid; i < m_nl; i += kEcpThreads) {
        const int32_t gr = W.nl_rows[nl0 + i];
        const double l0 = W.lb_old[gr], l1 = W.lb_new[gr], u0 = W.ub_old[gr], u1 = W.ub_new[gr];
        const bool mlo = !(l0 == l1), mhi = !(u0 == u1);
        if (!mlo && !mhi) continue;
        const double dlo = mlo ? l1 - l0 : 0.0, dhi = mhi ? u1 - u0 : 0.0;
        for (int r = last_cut[i]; r >= m_lin && r < M;) {
            if (mlo) lo[r] = lo[r] + dlo;
            if (mhi) hi[r] = hi[r] + dhi;
            ++moved;
            const int nx = cut_prev[r];
            r = nx < r ? nx : -1;
        }
    }
    if (moved) atomicAdd(W.cnt, moved);
}

}  // namespace ktn
