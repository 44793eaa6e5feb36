// batch_ecp.hpp -- throughput mode, second stage (BASELINE.json configs[4] "one instance per CU group"): ONE workgroup runs
// the WHOLE cutting-plane loop of one instance -- src/model.jl:257-309 with everything inside it: LP scaling, step-size
// estimate, the restarted reflected-Halpern PDHG with its checks and restarts, the separator sweep over the instance's
// nonlinear rows (precompute! + isconstrsat + gencut + round_coefs + _addcut), the column mirror of the grown matrix, the
// tolerance schedule and the stop rule -- so that no instance ever waits for another (with a host-driven round per
// cutting-plane iteration every round waits for its slowest instance: csrc/batch_lp.hpp).
//
// The batch is loaded as one block-diagonal problem (instances.fuse_instances, nlp.fuse_problems) of separable, tape or
// KTN_ROW_QUAD rows with a linear objective;
// ktn_loadproblem builds the fused LP of the linear rows as usual.  k_ecp_blocks then works on a per-instance ARENA in
// global memory (the instance's LP in local indices with room for its cuts): CSR rows (unscaled + scaled values), CSC
// mirror (unscaled + scaled), row bounds, duals, diagonal scalings, scaled problem vectors.  The PDHG iterates live in
// LDS; matrix entries stream from L2 / Infinity Cache.  Everything is deterministic: sums have a fixed order, the column
// mirror is sorted by row after the counting-sort scatter.  What a check of the PDHG decides is pdhg_stop / pdhg_next of
// pdhg_check.hpp, the functions the host loop of Engine::lp_solve_core calls, under this loop's own PdhgRules.
//
// k_ecp_blocks<ESH>: ESH = 0 is Kelley's method (every cut at x*).  ESH = 1 (ktn_optimize_blocks_ex with KTN_BLOCKS_SUPPORTING;
// DESIGN.md section 11 "In the device-side loop") moves the cut of every violated row that takes part to the point where the
// segment from the interior point x_int to x* leaves the row: separable rows by the bracketed Newton of esh.hpp (esh_init /
// esh_step / esh_point, 16 lanes per row), KTN_ROW_QUAD rows by the closed form of esh_quad.hpp (esh_quad_root).  TAPE ROWS KEEP
// KELLEY'S CUT, bit for bit, and are counted as fallback rows: a search pass there is a whole interpreter run by a single lane.
// The stop rule, the largest violation, yts[i], the objective certificate and the refinement passes keep the values at x*; a row
// with sig == 0 or without a finite phi >= 0 below lambda = 1 stores exactly what ESH = 0 stores.  The switch is a template
// parameter, not a field of EcpBatch: the kernel is sensitive to register allocation (see the note at the sweep), and
// k_ecp_blocks<0> is the code and the kernel argument that were there before the switch existed.
//
// A trailing EcpWarm argument -- k_ecp_blocks<0, EcpWarm>(EcpBatch, EcpWarm), k_ecp_blocks<1, EcpEsh, EcpWarm>(EcpBatch, EcpEsh, EcpWarm);
// ktn_optimize_blocks_ex with KTN_BLOCKS_WARM, DESIGN.md section 14 "In the device-side loop" -- is the WARM ENTRY: the arenas of the
// last launch are still there, k_blocks_rewarm (batch_warm.hpp) has screened, clamped and compacted them, and per instance its record
// says how to start: 1 from the arena's rows, multipliers, lists and x, with the first LP at the tolerance the last solve ended at;
// 2 an :Infeasible record and nothing else; 0 the initial LP below, as ever.  Like ESH it is decided by the template arguments and
// not by a field of EcpBatch, for the same reason: the cold instantiations <0> and <1, EcpEsh> keep their names, their kernel
// arguments and their code.
#pragma once
#include <type_traits>
#include "kernels.hpp"
#include "pdhg_check.hpp"
#include "quad_rows.hpp"
#include "esh_quad.hpp"

namespace ktn {

constexpr int kEcpThreads = 1024;
constexpr int kEcpQ = 12;

struct EcpArena {            // per-instance offsets into the flat arrays below (all local indices are instance-relative)
    int64_t row0, nnz0;      // first row slot / first entry slot of the instance
    int32_t cap_rows, cap_nnz;
};

struct EcpBatch {
    // ---- fused problem as loaded by the engine
    const int64_t* blk_col;          // [nb + 1] column offsets
    const int64_t* blk_lin;          // [nb + 1] offsets of the instances' linear rows in the fused LP (rows of the loaded LP)
    const int64_t* blk_nl;           // [nb + 1] offsets of the instances' NL slots (positions in nl_rows)
    const int64_t* lp_rowptr; const int32_t* lp_col; const double* lp_val; const double* lp_lo; const double* lp_hi;   // loaded LP
    const double* c; const double* l; const double* u;                                                                // LP columns (unscaled)
    NlpDev P; const int32_t* nl_rows;                                                                                 // NL rows (global ids)
    double* jac;                     // Jacobian scratch indexed like the structure (tape rows: written by the eval pass, read by the emit pass)
    int has_tape;                    // some NL row is a KTN_ROW_TAPE row (0: the sweep is the separable one alone)
    // KTN_ROW_QUAD rows among the NL rows (quad_rows.hpp): the engine's NL launch list; QUAD entries are numbered in row order and
    // NL rows are grouped by instance, so instance b owns rows [blk_qrow[b], blk_qrow[b+1]) and positions [blk_qent[b], blk_qent[b+1])
    int has_quad;                    // some NL row is a KTN_ROW_QUAD row (0: nothing below is read)
    int quad_group;                  // lanes per Jacobian entry of the entry pass (4 .. 64)
    QuadDev Q;
    const int32_t* q_rows; const int64_t* q_slots; const int64_t* q_tbase; const int64_t* q_ent;   // q_ent NULL: t = position
    const int64_t* blk_qrow; const int64_t* blk_qent;                                              // [nb + 1] each
    // ---- arenas
    const EcpArena* arena;
    int32_t* rptr; uint16_t* rcol; double* rval; double* rsval; double* lo; double* hi; double* y; double* dr; double* loh; double* hih;
    int32_t* cptr; uint16_t* crow; double* cval; double* csval;    // cptr: [ncols_total + nb] (instance b at blk_col[b] + b); 16-bit local
                                                                   // indices: 20 instead of 24 bytes per non-zero and PDHG iteration
    double* dc; double* ch; double* lh; double* uh;                // per column (global column indexing)
    int32_t* last_cut;                                             // per NL slot: local row of its newest cut (-1)
    int32_t* cut_prev;                                             // per row: previous cut of the same NL slot (-1): lists for the stall handler
    double* ax;                                                    // per row: scaled activity A^ xt of the last check
    double* x;                                                     // [ncols_total] out: solution (unscaled); in: ignored
    double* xbest;                                                 // [ncols_total] scratch: best point of the certificate refinement
    double* res;                                                   // [nb * 8] out: status, ecp iterations, objective, cuts, pdhg iterations, max violation, lp rows, -
    // ---- parameters
    double f_tol, cut_coef_rng, tol_scale, tol_floor, tol_cap, gap_floor, gap_cap, stag_factor;
    double cert_tol;                 // obj_cert_tol: per-instance objective certificate (below); 0 = stop at the reference's rule alone
    int iter_cap, lp_max_iter, check_every, near_chunk, ruiz_iters, power_passes, nmax, mmax, polish_max_iter;
};
// EcpBatch::res, eight slots per instance: 0 status, 1 cutting-plane iterations, 2 objective, 3 cuts (linear rows counted), 4 PDHG
// iterations, 5 largest violation of the last sweep, 6 LP rows at the end, 7 arena overflow (0 / 1)  (include/katana_hip.h,
// ktn_blocks_get_results)

// What k_ecp_blocks<1> takes beside the batch
struct EcpEsh {
    const double* xint;              // [ncols_total] x_int (global column indexing: the engine's d_xint)
    const int8_t* sig;               // per global row: the side of a row that takes part, else 0 (d_esh_sig)
    const double* jint;              // Jacobian at x_int by Jacobian entry (d_jint); NULL: no QUAD row takes part
    double* lam;                     // arena, per row slot: lambda of the cut row (1: Kelley's cut)
    double* res;                     // [nb * 4] out: rows moved, fallback rows, search passes, QUAD rows moved
    double root_tol;                 // esh_root_tol: a search stops at 0 <= phi <= root_tol * (the sweep's f_tol)
    int iters;                       // esh_root_iters
};
// What the warm entry takes beside them: the records of k_blocks_rewarm (batch_warm.hpp)
struct EcpWarm {
    const double* rec;               // [nb * 8]: state (0 cold, 1 warm, 2 infeasible), M, NNZ, ...
};
template <class... Rest>
__device__ __forceinline__ const EcpEsh& ecp_esh_arg(const EcpEsh& e, const Rest&...) { return e; }
__device__ __forceinline__ const EcpWarm& ecp_warm_arg(const EcpWarm& w) { return w; }
__device__ __forceinline__ const EcpWarm& ecp_warm_arg(const EcpEsh&, const EcpWarm& w) { return w; }

// ---------------------------------------------------------------------------------------------------------------------
// sparse dot products of the block's outputs (rows or columns) with an LDS vector: out(o, acc) called by lane 0 of each
// group.  T outputs per lane group and pass: the entry ranges of all T, then the first two entries per lane of all T, are
// requested before anything is used -- a pass costs two memory latencies instead of two per output (a lone workgroup, the
// tail of the batch, is latency-bound).
struct EcpPre { double a, b, c; };
template <int G, int T, class PF, class F>
__device__ __forceinline__ void ecp_spmv(int count, const int32_t* __restrict__ ptr, const uint16_t* __restrict__ idx,
                                         const double* __restrict__ val, const double* v, PF&& pre, F&& out) {
    constexpr int kGroups = kEcpThreads / G;
    const int lane = threadIdx.x & (G - 1), g0 = threadIdx.x / G;
    static_assert(T <= G, "one output per lane of the group");
    for (int base = 0; base < count; base += T * kGroups) {
        // the scalars the step's element-wise tail needs for the output THIS lane will finish (bounds, cost) are requested
        // first: their latency overlaps the gather chain
        const int omine = base + g0 + lane * kGroups;
        const bool fin = lane < T && omine < count;
        EcpPre pf{0.0, 0.0, 0.0};
        if (fin) pf = pre(omine);
        int beg[T], end[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int o = base + g0 + t * kGroups;
            const bool on = o < count;
            beg[t] = on ? ptr[o] : 0;
            end[t] = on ? ptr[o + 1] : 0;
        }
        double a0[T], a1[T];
        int i0[T], i1[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int e0 = beg[t] + lane, e1 = e0 + G;
            const bool on0 = e0 < end[t], on1 = e1 < end[t];
            a0[t] = on0 ? val[e0] : 0.0; i0[t] = on0 ? idx[e0] : 0;
            a1[t] = on1 ? val[e1] : 0.0; i1[t] = on1 ? idx[e1] : 0;
        }
        // the butterfly leaves every lane of the group with the sum: lane t finishes output t (T <= G), so the element-wise
        // tail of the step (clamps, the Halpern update) runs once per group with all lanes busy instead of T times with one
        // lane in G
        double mine = 0.0;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            double acc = a0[t] * v[i0[t]] + a1[t] * v[i1[t]];
            for (int e = beg[t] + lane + 2 * G; e < end[t]; e += G) acc += val[e] * v[idx[e]];
            acc = group_sum<G>(acc);
            if (lane == t) mine = acc;
        }
        if (fin) out(omine, mine, pf);
    }
}

// one tape row at the instance's LDS copy of x (xs[col - c0]).  Inlined: as a call (__noinline__) the kernel's scratch grows
// from 376 to 1 440 bytes per lane (the live state of the PDHG loop is saved around the call), inlined to 504
// (DESIGN.md section 8).
static __device__ __forceinline__ double ecp_tape_row(const NlpDev& P, int32_t r, const double* xs, int c0, double* jac) {
    return tape_row_eval(P, r, [&](int32_t c) { return xs[c - c0]; }, jac);
}

// Entry pass of the instance's QUAD rows (k_quad_jac inside the workgroup): G lanes per Jacobian entry walk its Q segment,
// consecutive lanes on consecutive Q entries, x from the LDS copy; lane 0 writes jac[e] and vterm[t] (quad_entry).
template <int G>
static __device__ __forceinline__ void ecp_quad_entries(const EcpBatch& B, int64_t p0, int64_t p1, const double* xs, int c0) {
    const int lane = threadIdx.x & (G - 1);
    for (int64_t p = p0 + threadIdx.x / G; p < p1; p += kEcpThreads / G) {
        const int64_t t = B.q_ent ? B.q_ent[p] : p;
        const int64_t beg = B.Q.qptr[t], end = B.Q.qptr[t + 1];
        double s = 0.0;
        for (int64_t k = beg + lane; k < end; k += G) s += B.Q.qval[k] * xs[B.Q.qcol[k] - c0];
        s = group_sum<G>(s);                                   // (p is uniform within a lane group: the butterfly never leaves it)
        if (lane == 0) {
            const int64_t e = B.Q.jidx[t];
            const QuadEntry qe = quad_entry(B.P.pp[e].x, s, xs[(B.P.colk[e] & kColMask) - c0]);
            B.jac[e] = qe.jac;
            B.Q.vterm[t] = qe.vterm;
        }
    }
}

// k_ecp_blocks<0>(EcpBatch) and k_ecp_blocks<1, EcpEsh>(EcpBatch, EcpEsh): the second argument exists only for ESH = 1 (wrapping
// both into one struct changed the code of <0>: 40 bytes and three more SGPR spills; the empty pack leaves it as it was)
template <int ESH, class... EshArg>
__global__ __launch_bounds__(kEcpThreads) void k_ecp_blocks(EcpBatch B, EshArg... esh_arg) {
    constexpr bool WARM = (std::is_same_v<EshArg, EcpWarm> || ...);
    static_assert(sizeof...(EshArg) == (ESH != 0 ? 1 : 0) + (WARM ? 1 : 0),
                  "k_ecp_blocks<0>(EcpBatch) or k_ecp_blocks<1, EcpEsh>(EcpBatch, EcpEsh), each with a trailing EcpWarm for the warm entry");
    extern __shared__ double sm[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t c0 = B.blk_col[b];
    const int nb = (int)(B.blk_col[b + 1] - c0);
    const int64_t lin0 = B.blk_lin[b];
    const int m_lin = (int)(B.blk_lin[b + 1] - lin0);
    const int64_t nl0 = B.blk_nl[b];
    const int m_nl = (int)(B.blk_nl[b + 1] - nl0);
    const EcpArena A = B.arena[b];
    int32_t* rptr = B.rptr + A.row0 + b;          // cap_rows + 1 slots per instance
    uint16_t* rcol = B.rcol + A.nnz0;
    double* rval = B.rval + A.nnz0;
    double* rsval = B.rsval + A.nnz0;
    double* lo = B.lo + A.row0; double* hi = B.hi + A.row0; double* yv = B.y + A.row0; double* dr = B.dr + A.row0;
    double* loh = B.loh + A.row0; double* hih = B.hih + A.row0;
    int32_t* cptr = B.cptr + c0 + b;              // nb + 1 slots per instance
    uint16_t* crow = B.crow + A.nnz0;
    double* cval = B.cval + A.nnz0;
    double* csval = B.csval + A.nnz0;
    double* dc = B.dc + c0; double* ch = B.ch + c0; double* lh = B.lh + c0; double* uh = B.uh + c0;
    const double* cc = B.c + c0; const double* ll = B.l + c0; const double* uu = B.u + c0;
    int32_t* last_cut = B.last_cut + nl0;
    int32_t* cut_prev = B.cut_prev + A.row0;
    double* axv = B.ax + A.row0;
    double* xg = B.x + c0;
    double* xbest = B.xbest + c0;

    double* xs = sm;                   // x (scaled)
    double* x0s = xs + B.nmax;
    double* xts = x0s + B.nmax;        // xbar | xt ; also scratch
    double* ys = xts + B.nmax;
    double* y0s = ys + B.mmax;
    double* yts = y0s + B.mmax;
    double* red = yts + B.mmax;                        // [waves][kEcpQ]
    double* q = red + (kEcpThreads / 64) * kEcpQ;      // [kEcpQ]
    double* ctl = q + kEcpQ;                           // [8]
    double* st = ctl + 8;                              // [16] thread 0's control state of the LP loop (kept out of every thread's registers)
    int32_t* icnt = reinterpret_cast<int32_t*>(st + 16);   // [max(nmax, mmax) + 2] integer scratch (column counts, flags)

    // ================================================================ initial LP: the instance's linear rows =========
    int M = m_lin, NNZ = 0;
    int wstate = 0;                    // (WARM) what k_blocks_rewarm decided for this instance
    if constexpr (WARM) wstate = (int)ecp_warm_arg(esh_arg...).rec[(int64_t)b * 8];
    if (!WARM || wstate == 0) {
        const int64_t e0 = B.lp_rowptr[lin0];
        NNZ = (int)(B.lp_rowptr[lin0 + m_lin] - e0);
        for (int r = tid; r <= m_lin; r += kEcpThreads) rptr[r] = (int32_t)(B.lp_rowptr[lin0 + r] - e0);
        for (int r = tid; r < m_lin; r += kEcpThreads) { lo[r] = B.lp_lo[lin0 + r]; hi[r] = B.lp_hi[lin0 + r]; yv[r] = 0.0; }
        for (int e = tid; e < NNZ; e += kEcpThreads) { rcol[e] = (uint16_t)(B.lp_col[e0 + e] - (int32_t)c0); rval[e] = B.lp_val[e0 + e]; }
        for (int i = tid; i < m_nl; i += kEcpThreads) last_cut[i] = -1;
        for (int j = tid; j < nb; j += kEcpThreads) xg[j] = 0.0;
    }
    [[maybe_unused]] double warm_maxviol = 1e300;
    if constexpr (WARM) {
        if (wstate == 2) {             // the new box is empty or a kept row excludes it: no LP (the arena stays as it is)
            if (tid == 0) {
                double* o = B.res + (int64_t)b * 8;
                const double rows = o[6];
                o[0] = (double)KTN_STATUS_INFEASIBLE; o[1] = 0.0; o[2] = __builtin_nan(""); o[3] = rows; o[4] = 0.0; o[5] = 1e300; o[6] = rows; o[7] = 0.0;
            }
            if constexpr (ESH != 0) { if (tid < 4) ecp_esh_arg(esh_arg...).res[(int64_t)b * 4 + tid] = 0.0; }
            return;
        }
        if (wstate == 1) {             // the arena of the last launch: its rows, yv, last_cut, cut_prev and xg stand
            M = (int)ecp_warm_arg(esh_arg...).rec[(int64_t)b * 8 + 1];
            NNZ = rptr[M];
            warm_maxviol = B.res[(int64_t)b * 8 + 5];      // (read by every lane long before lane 0 writes the new record)
        }
    }
    __syncthreads();
    int status = KTN_STATUS_NONE, iter = 0, numcuts = m_lin;
    if constexpr (WARM) numcuts = M;
    long pdhg_total = 0;
    double last_maxviol = 1e300, objval = 0.0, om_keep = -1.0;
    if constexpr (WARM) last_maxviol = warm_maxviol;
    bool allsat = false, overflow = false;
    // Objective certificate per instance (Engine::objective_certificate / kernels.hpp "objective certificate", round 4): at the
    // point that meets the reference's stop rule the workgroup adds up  D = sum_i lambda_i * (signed residual of NL row i)  with
    // lambda_i the LP duals summed over the cuts of row i -- the part of  f* - objective  the stop rule leaves open -- and while
    // D exceeds half of cert_tol * max(1, |objective|) it keeps cutting at  f_eff = phi * f_tol  with the LP gap tolerance at a
    // quarter of the target (passes not counted in the iteration number, at most polish_max_iter).  The point returned is the
    // one with the smallest violation among those that satisfy the reference's rule.
    double f_eff = B.f_tol, gap_cert = 1e300, best_viol = 1e300, best_obj = 0.0;
    int passes = 0;
    bool refining = false;
    int esh_cnt[4] = {0, 0, 0, 0};                // (ESH) lane 0 of a row's group: rows moved, fallback rows, search passes, QUAD rows moved
  for (;;) {
    const double floor_p = B.tol_floor * f_eff;

    while (!allsat && (refining ? passes <= B.polish_max_iter : iter < B.iter_cap)) {
        if (refining) ++passes; else ++iter;
        double tol_p = fmin(fmax(B.tol_scale * last_maxviol, floor_p), B.tol_cap);
        if (m_nl == 0 || refining) tol_p = floor_p;
        const double tol_g = fmin(fmin(fmax(tol_p, B.gap_floor), B.gap_cap), gap_cert);

        // ============================================================ column mirror of the current rows ================
        // counting sort by column, then every column's entries sorted by row (fixed summation order of A'y)
        for (int j = tid; j <= nb; j += kEcpThreads) icnt[j] = 0;
        __syncthreads();
        for (int e = tid; e < NNZ; e += kEcpThreads) atomicAdd(&icnt[rcol[e] + 1], 1);
        __syncthreads();
        if (tid == 0) { int run = 0; for (int j = 0; j <= nb; ++j) { run += icnt[j]; cptr[j] = run; } }   // nb ~ 1e3: a serial scan is cheap
        __syncthreads();
        for (int j = tid; j < nb; j += kEcpThreads) icnt[j] = cptr[j];                 // cursors
        __syncthreads();
        for (int r = tid; r < M; r += kEcpThreads)
            for (int e = rptr[r]; e < rptr[r + 1]; ++e) {
                const int p = atomicAdd(&icnt[rcol[e]], 1);
                crow[p] = (uint16_t)r; cval[p] = rval[e];
            }
        __syncthreads();
        for (int j = tid; j < nb; j += kEcpThreads) {                                   // insertion sort by row (short lists)
            const int beg = cptr[j], end = cptr[j + 1];
            for (int a = beg + 1; a < end; ++a) {
                const uint16_t rr = crow[a]; const double vv = cval[a];
                int p = a - 1;
                while (p >= beg && crow[p] > rr) { crow[p + 1] = crow[p]; cval[p + 1] = cval[p]; --p; }
                crow[p + 1] = rr; cval[p + 1] = vv;
            }
        }
        __syncthreads();

        // ============================================================ diagonal scaling: Ruiz passes + Pock-Chambolle ===
        for (int r = tid; r < M; r += kEcpThreads) dr[r] = 1.0;
        for (int j = tid; j < nb; j += kEcpThreads) dc[j] = 1.0;
        __syncthreads();
        for (int pass = 0; pass <= B.ruiz_iters; ++pass) {
            const bool pc = pass == B.ruiz_iters;
            // stats with the CURRENT dr, dc (rows into yts, columns into xts), then both applied
            {
                const int lane = tid & 3;
                for (int r = tid / 4; r < M; r += kEcpThreads / 4) {
                    double acc = 0.0;
                    for (int e = rptr[r] + lane; e < rptr[r + 1]; e += 4) { const double v = fabs(rval[e]) * dc[rcol[e]]; acc = pc ? acc + v : fmax(acc, v); }
                    acc = pc ? group_sum<4>(acc) : group_max<4>(acc);
                    if (lane == 0) yts[r] = dr[r] * acc;
                }
                for (int j = tid / 4; j < nb; j += kEcpThreads / 4) {
                    double acc = 0.0;
                    for (int e = cptr[j] + lane; e < cptr[j + 1]; e += 4) { const double v = fabs(cval[e]) * dr[crow[e]]; acc = pc ? acc + v : fmax(acc, v); }
                    acc = pc ? group_sum<4>(acc) : group_max<4>(acc);
                    if (lane == 0) xts[j] = dc[j] * acc;
                }
            }
            __syncthreads();
            for (int r = tid; r < M; r += kEcpThreads) { const double s = yts[r]; if (s > 0.0 && isfinite(s)) dr[r] /= sqrt(s); }
            for (int j = tid; j < nb; j += kEcpThreads) { const double s = xts[j]; if (s > 0.0 && isfinite(s)) dc[j] /= sqrt(s); }
            __syncthreads();
        }
        for (int r = tid; r < M; r += kEcpThreads) {
            const double d = dr[r];
            for (int e = rptr[r]; e < rptr[r + 1]; ++e) rsval[e] = d * rval[e] * dc[rcol[e]];
            double a = lo[r], bb = hi[r];
            if (a != a) a = -__builtin_inf();
            if (bb != bb) bb = __builtin_inf();
            loh[r] = a * d; hih[r] = bb * d;
            const double yh = yv[r] / d;
            ys[r] = yh; y0s[r] = yh; yts[r] = yh;
        }
        for (int j = tid; j < nb; j += kEcpThreads) {
            const double d = dc[j];
            for (int e = cptr[j]; e < cptr[j + 1]; ++e) csval[e] = d * cval[e] * dr[crow[e]];
            ch[j] = cc[j] * d; lh[j] = ll[j] / d; uh[j] = uu[j] / d;
            const double xh = clampd(xg[j] / d, ll[j] / d, uu[j] / d);
            xs[j] = xh; x0s[j] = xh; xts[j] = xh;
        }
        // An LP without rows (an instance without linear rows, before its first cut): ecp_spmv multiplies the entries a lane does
        // not have by element 0 of the vector -- 0.0 * v[0] -- and no row has defined ys[0], y0s[0], yts[0]: a NaN that an earlier
        // workgroup left in this LDS would reach every A'y.  (mmax >= 1: the element exists.)
        if (M == 0 && tid == 0) { ys[0] = 0.0; y0s[0] = 0.0; yts[0] = 0.0; }
        __syncthreads();

        // ============================================================ sigma_max: 20 power passes (hashed start vector) ==
        double smax = 0.0;
        {
            double a1[1];
            a1[0] = 0.0;
            for (int j = tid; j < nb; j += kEcpThreads) {
                uint64_t h = (uint64_t)(c0 + j) * 0x9E3779B97F4A7C15ULL + 0xD1B54A32D192ED03ULL;
                h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ULL; h ^= h >> 32;
                const double v = 0.25 + (double)(h >> 11) * (1.0 / 9007199254740992.0);
                xts[j] = v; a1[0] += v * v;
            }
            wg_reduce<kEcpThreads, 1>(a1, 1, red, q);
            double nrm = sqrt(q[0]);
            __syncthreads();
            for (int j = tid; j < nb; j += kEcpThreads) xts[j] = nrm > 0.0 ? xts[j] / nrm : 0.0;
            __syncthreads();
            const int npow = B.power_passes;
            for (int pass = 0; pass < npow; ++pass) {
                ecp_spmv<4, 4>(M, rptr, rcol, rsval, xts, [&](int) { return EcpPre{0.0, 0.0, 0.0}; }, [&](int r, double acc, const EcpPre&) { yts[r] = acc; });
                __syncthreads();
                a1[0] = 0.0;
                // A'(A v) into xts: the columns read yts and write xts, no hazard
                ecp_spmv<4, 4>(nb, cptr, crow, csval, yts, [&](int) { return EcpPre{0.0, 0.0, 0.0}; },
                               [&](int j, double acc, const EcpPre&) { xts[j] = acc; a1[0] += acc * acc; });
                wg_reduce<kEcpThreads, 1>(a1, 1, red, q);
                nrm = sqrt(q[0]);
                __syncthreads();
                if (pass < npow - 1) for (int j = tid; j < nb; j += kEcpThreads) xts[j] = nrm > 0.0 ? xts[j] / nrm : 0.0;
                __syncthreads();
            }
            smax = sqrt(nrm);                    // ||A'A v|| with ||v|| = 1 -> sigma_max^2
            // restore the iterates the passes overwrote
            for (int j = tid; j < nb; j += kEcpThreads) xts[j] = xs[j];
            for (int r = tid; r < M; r += kEcpThreads) yts[r] = ys[r];
            __syncthreads();
        }
        const double eta_safe = 0.998;
        double eta = fmax(0.998 / fmax(smax, 1e-12), eta_safe);

        // ============================================================ LP: restarted reflected-Halpern PDHG =============
        double v2[2] = {0.0, 0.0};
        for (int j = tid; j < nb; j += kEcpThreads) v2[0] += ch[j] * ch[j];
        for (int r = tid; r < M; r += kEcpThreads) { const double a = loh[r], bb = hih[r]; if (isfinite(a)) v2[1] += a * a; if (isfinite(bb)) v2[1] += bb * bb; }
        wg_reduce<kEcpThreads, 2>(v2, 2, red, q);
        const double nc2 = q[0], nb2 = q[1];
        __syncthreads();
        const double omega_ref = (nc2 > 0.0 && nb2 > 0.0) ? sqrt(nc2 / nb2) : 1.0;
        const double dres_scale = 1.0 + sqrt(nc2);
        double om = om_keep > 0.0 ? om_keep : omega_ref;
        int k = 0, it = 0;
        if (tid == 0) *reinterpret_cast<PdhgCtl*>(st) = pdhg_start();          // (st: the PdhgCtl of this LP solve)
        bool plain_next = false, near_conv = false;
        int lp_status = KTN_STATUS_USERLIMIT;
        double pobj = 0.0;
        const int plain_len = B.check_every - 1;
        const double stall_accept = (tol_p > floor_p * (1.0 + 1e-9)) ? 10.0 : 3.0;
        while (it < B.lp_max_iter) {
            const double tau = eta / om, sigma = eta * om, inv_sigma = 1.0 / sigma;
            if (plain_next) {
                plain_next = false;
                int want = (k <= 1) ? min(31, plain_len) : plain_len;
                if (near_conv && B.near_chunk > 0) want = min(want, B.near_chunk);
                const int np = min(want, B.lp_max_iter - it);
                for (int s = 0; s < np; ++s) {
                    const double w = (double)(k + s + 1) / (double)(k + s + 2);
                    ecp_spmv<4, 4>(nb, cptr, crow, csval, ys, [&](int j) { return EcpPre{ch[j], lh[j], uh[j]}; },
                                   [&](int j, double acc, const EcpPre& p) {
                        const double xv = xs[j];
                        const double xtv = prox_x(xv, tau, p.a, acc, p.b, p.c);
                        xts[j] = 2.0 * xtv - xv;
                        xs[j] = w * (2.0 * xtv - xv) + (1.0 - w) * x0s[j];
                    });
                    __syncthreads();
                    ecp_spmv<4, 4>(M, rptr, rcol, rsval, xts, [&](int r) { return EcpPre{loh[r], hih[r], 0.0}; },
                                   [&](int r, double acc, const EcpPre& p) {
                        const double y1 = ys[r];
                        const double v = y1 - sigma * acc;
                        const double ytv = v + sigma * clampd(-v * inv_sigma, p.a, p.b);   // not prox_y: -v * (1 / sigma) rounds differently from -v / sigma
                        ys[r] = w * (2.0 * ytv - y1) + (1.0 - w) * y0s[r];
                    });
                    __syncthreads();
                }
                k += np; it += np;
                continue;
            }
            double a[kEcpQ];
#pragma unroll
            for (int i = 0; i < kEcpQ; ++i) a[i] = 0.0;
            ecp_spmv<4, 4>(nb, cptr, crow, csval, ys, [&](int j) { return EcpPre{ch[j], lh[j], uh[j]}; },
                           [&](int j, double acc, const EcpPre& p) { xts[j] = prox_x(xs[j], tau, p.a, acc, p.b, p.c); });
            __syncthreads();
            {
                const int lane = tid & 3;
                for (int r = tid / 4; r < M; r += kEcpThreads / 4) {
                    double axt = 0.0, axk = 0.0;
                    for (int e = rptr[r] + lane; e < rptr[r + 1]; e += 4) { const int cl = rcol[e]; const double vv = rsval[e]; axt += vv * xts[cl]; axk += vv * xs[cl]; }
                    axt = group_sum<4>(axt); axk = group_sum<4>(axk);
                    if (lane == 0) {
                        const double loi = loh[r], hii = hih[r], y1 = ys[r];
                        const double ytv = prox_y(y1, sigma, 2.0 * axt - axk, loi, hii);
                        yts[r] = ytv;
                        axv[r] = axt;
                        const ChkRowTerms t = chk_row_terms(ytv, y1, y0s[r], axt, axk, loi, hii, dr[r]);
                        a[0] += t.dyAdx; a[1] += t.dy2; a[2] += t.dobj; a[3] += t.dy0sq; a[9] += t.yt2;
                        a[10] = fmax(a[10], t.viol);
                    }
                }
            }
            __syncthreads();
            ecp_spmv<4, 4>(nb, cptr, crow, csval, yts, [&](int j) { return EcpPre{ch[j], lh[j], uh[j]}; },
                           [&](int j, double aty, const EcpPre& p) {
                const ChkColTerms t = chk_col_terms(xts[j], xs[j], x0s[j], aty, p.a, p.b, p.c, dc[j]);
                a[4] += t.dx2; a[5] += t.pobj; a[6] += t.dobj; a[7] += t.dx0sq; a[8] += t.xt2;
                a[11] = fmax(a[11], t.dres);
            });
            wg_reduce<kEcpThreads, kEcpQ>(a, 10, red, q);
            if (tid == 0) {
                const PdhgSums S{q[0], q[1], q[3], q[4], q[7], q[8], q[9], q[5], q[2] + q[6], q[10], q[11]};
                const PdhgRules rules{tol_p, tol_g, dres_scale, B.stag_factor, 0.1, 3, stall_accept, eta_safe, false, false, M > m_lin,
                                      omega_ref, true, 0.0, 0.0, 0.0, 0.0};
                PdhgCtl& pc = *reinterpret_cast<PdhgCtl*>(st);
                const PdhgStop t = pdhg_stop(S, rules, pc, om, eta, k);
                int action = 0;                               // 0 continue, 1 restart, 2 done, 3 give up, 4 consolidate and restart
                double om1 = om, eta1 = eta;
                if (t.exit != PDHG_EXIT_NONE) action = t.exit == PDHG_EXIT_NAN ? 3 : 2;
                else {
                    const PdhgNext nx = pdhg_next(S, rules, pc, t, om, eta, k, it);
                    om1 = nx.om; eta1 = nx.eta;
                    action = nx.action == PDHG_CONSOLIDATE ? 4 : (nx.action == PDHG_RESTART ? 1 : 0);
                }
                ctl[0] = (double)action; ctl[1] = om1; ctl[2] = eta1; ctl[3] = t.near ? 1.0 : 0.0; ctl[4] = S.pobj;
            }
            __syncthreads();
            const int action = (int)ctl[0];
            om = ctl[1]; eta = ctl[2]; near_conv = ctl[3] != 0.0; pobj = ctl[4];
            __syncthreads();
            ++it;
            if (action == 2) { lp_status = KTN_STATUS_OPTIMAL; break; }
            if (action == 3) { lp_status = KTN_STATUS_ERROR; break; }
            if (action == 4) {
                // one thread per NL slot walks the slot's cuts (newest first): unscaled activity a'x = ax / dr, unscaled multiplier y dr
                for (int i = tid; i < m_nl; i += kEcpThreads) {
                    int best_u = -1, best_l = -1, ncuts = 0;
                    double res_u = -__builtin_inf(), res_l = -__builtin_inf();
                    for (int r = last_cut[i]; r >= 0; r = cut_prev[r]) {
                        ++ncuts;
                        const double axu = axv[r] / dr[r];
                        const double ru = axu - hi[r], rl = lo[r] - axu;
                        if (ru > res_u) { res_u = ru; best_u = r; }
                        if (rl > res_l) { res_l = rl; best_l = r; }
                    }
                    if (ncuts < 2) continue;
                    double mass_u = 0.0, mass_l = 0.0;
                    for (int r = last_cut[i]; r >= 0; r = cut_prev[r]) {
                        const double yu = yts[r] * dr[r];
                        const double axu = axv[r] / dr[r];
                        if (yu < 0.0 && best_u >= 0 && r != best_u && (axu - hi[r]) < -tol_p) { mass_u += yu; yts[r] = 0.0; }
                        else if (yu > 0.0 && best_l >= 0 && r != best_l && (lo[r] - axu) < -tol_p) { mass_l += yu; yts[r] = 0.0; }
                    }
                    if (mass_u != 0.0) yts[best_u] += mass_u / dr[best_u];
                    if (mass_l != 0.0) yts[best_l] += mass_l / dr[best_l];
                }
                __syncthreads();
            }
            if (action == 1 || action == 4) {
                for (int j = tid; j < nb; j += kEcpThreads) { const double v = xts[j]; xs[j] = v; x0s[j] = v; }
                for (int r = tid; r < M; r += kEcpThreads) { const double v = yts[r]; ys[r] = v; y0s[r] = v; }
                k = 0;
                __syncthreads();
                continue;
            }
            {
                const double w = (double)(k + 1) / (double)(k + 2);
                for (int j = tid; j < nb; j += kEcpThreads) xs[j] = w * (2.0 * xts[j] - xs[j]) + (1.0 - w) * x0s[j];
                for (int r = tid; r < M; r += kEcpThreads) ys[r] = w * (2.0 * yts[r] - ys[r]) + (1.0 - w) * y0s[r];
                ++k;
                plain_next = true;
                __syncthreads();
            }
        }
        pdhg_total += it;
        om_keep = om;
        if (lp_status != KTN_STATUS_OPTIMAL) { status = lp_status; break; }          // model.jl:261-263
        // un-scale T(z): x* (kept in LDS xs for the sweep) and the duals
        for (int j = tid; j < nb; j += kEcpThreads) { const double v = xts[j] * dc[j]; xg[j] = v; xs[j] = v; }
        for (int r = tid; r < M; r += kEcpThreads) yv[r] = yts[r] * dr[r];
        objval = pobj;
        __syncthreads();

        // ============================================================ separator sweep over the instance's NL rows ======
        // (The verdict is row_sat / row_violation of kernels.hpp at each of the three places, not one function of this file: as a
        //  function -- by reference, by value, bounds passed or read inside -- it moved a thousand of this kernel's 14 100
        //  instructions to other registers and spill slots; written out, the kernel's code is unchanged.)
        // precompute! + isconstrsat (src/separators.jl:111-120): 16 lanes per separable row, one lane per tape row, G lanes per
        // Jacobian entry and then 16 per row for QUAD rows; flags and row lengths into icnt
        double mv[1] = {0.0};
        int bad_nf = 0;
        {
            const int lane = tid & 15;
            for (int i = tid / 16; i < m_nl; i += kEcpThreads / 16) {
                const int32_t gr = B.nl_rows[nl0 + i];
                if (B.has_tape | B.has_quad) {                                           // (the device row_kind also holds kRowSepLong)
                    const uint8_t rk = B.P.row_kind[gr];
                    if (rk == KTN_ROW_TAPE || rk == KTN_ROW_QUAD) continue;
                }
                const int64_t beg = B.P.rowptr[gr], end = B.P.rowptr[gr + 1];
                double g = 0.0;
                for (int64_t e = beg + lane; e < end; e += 16) {
                    const int ck = B.P.colk[e];
                    const double2 pp = B.P.pp[e];
                    double val, der;
                    atom_eval((unsigned)ck >> kKindShift, pp.x, pp.y, xs[(ck & kColMask) - (int)c0], val, der);
                    g += val;
                }
                g = group_sum<16>(g);
                if (lane == 0) {
                    g += B.P.rconst[gr];
                    const double lb = B.P.lb[gr], ub = B.P.ub[gr];
                    const bool sat = row_sat(g, lb, ub, f_eff);
                    icnt[i] = sat ? 0 : (int)(end - beg);
                    yts[i] = g;                                                         // keep g for the emit pass (m_nl <= mmax)
                    if (!sat) mv[0] = fmax(mv[0], row_violation(g, lb, ub));
                }
            }
            // tape rows: the interpreter of k_tape_eval with x from LDS; node values and adjoints in the rows' own slices of
            // node_val / node_adj, Jacobian entries into B.jac (the instances' node and entry ranges are disjoint)
            if (B.has_tape) {
                for (int i = tid; i < m_nl; i += kEcpThreads) {
                    const int32_t gr = B.nl_rows[nl0 + i];
                    if (B.P.row_kind[gr] != KTN_ROW_TAPE) continue;
                    const double g = ecp_tape_row(B.P, gr, xs, (int)c0, B.jac);
                    const double lb = B.P.lb[gr], ub = B.P.ub[gr];
                    const bool sat = row_sat(g, lb, ub, f_eff);
                    icnt[i] = sat ? 0 : (int)(B.P.rowptr[gr + 1] - B.P.rowptr[gr]);
                    yts[i] = g;
                    if (!sat) mv[0] = fmax(mv[0], row_violation(g, lb, ub));
                }
            }
            // QUAD rows: the two passes of quad_rows.hpp inside the workgroup.  Entry-parallel first (a 1 000-entry row with a
            // diagonal Q and a 3-entry row cost their own work), then 16 lanes per row over the value terms
            if (B.has_quad) {
                const int64_t pe0 = B.blk_qent[b], pe1 = B.blk_qent[b + 1];
                switch (B.quad_group) {
                    case 4: ecp_quad_entries<4>(B, pe0, pe1, xs, (int)c0); break;
                    case 8: ecp_quad_entries<8>(B, pe0, pe1, xs, (int)c0); break;
                    case 16: ecp_quad_entries<16>(B, pe0, pe1, xs, (int)c0); break;
                    case 32: ecp_quad_entries<32>(B, pe0, pe1, xs, (int)c0); break;
                    default: ecp_quad_entries<64>(B, pe0, pe1, xs, (int)c0); break;
                }
                __syncthreads();
                for (int64_t qi = B.blk_qrow[b] + tid / 16; qi < B.blk_qrow[b + 1]; qi += kEcpThreads / 16) {
                    const int32_t gr = B.q_rows[qi];
                    const int i = (int)(B.q_slots[qi] - nl0);
                    const int len = (int)(B.P.rowptr[gr + 1] - B.P.rowptr[gr]);
                    const int64_t tb = B.q_tbase[qi];
                    double g = 0.0;
                    for (int e = lane; e < len; e += 16) g += B.Q.vterm[tb + e];
                    g = group_sum<16>(g);
                    if (lane == 0) {
                        g += B.P.rconst[gr];
                        const double lb = B.P.lb[gr], ub = B.P.ub[gr];
                        const bool sat = row_sat(g, lb, ub, f_eff);
                        icnt[i] = sat ? 0 : len;
                        yts[i] = g;
                        if (!sat) mv[0] = fmax(mv[0], row_violation(g, lb, ub));
                    }
                }
            }
        }
        __syncthreads();
        {
            double t1[1] = {mv[0]};
            wg_reduce<kEcpThreads, 1>(t1, 0, red, q);
            mv[0] = q[0];
        }
        __syncthreads();
        // ranks of the violated rows (serial scan over m_nl ~ 1e2 slots)
        if (tid == 0) {
            int rows = 0;
            for (int i = 0; i < m_nl; ++i) { const int len = icnt[i]; icnt[i] = len > 0 ? ((rows << 1) | 1) : 0; if (len > 0) { ++rows; } }
            // second pass for the entry offsets (row lengths come from the structure again)
            ctl[5] = (double)rows;
        }
        __syncthreads();
        const int V = (int)ctl[5];
        int nnzV = 0;
        if (V > 0) {
            // entry offsets: thread 0 walks the violated rows in order
            // (capacity is tested BEFORE anything is stored: the row pointers of an arena have cap_rows + 1 slots and the
            //  next instance's arena follows -- a dry pass for the entry count, the stores only when rows and entries fit)
            if (tid == 0) {
                int64_t nz = NNZ;
                for (int i = 0; i < m_nl; ++i) if (icnt[i] & 1) {
                    const int32_t gr = B.nl_rows[nl0 + i];
                    nz += B.P.rowptr[gr + 1] - B.P.rowptr[gr];
                }
                const bool fits = (M + V <= A.cap_rows) && (nz <= A.cap_nnz);
                if (fits) {
                    int at = NNZ;
                    for (int i = 0; i < m_nl; ++i) if (icnt[i] & 1) {
                        const int32_t gr = B.nl_rows[nl0 + i];
                        rptr[M + (icnt[i] >> 1)] = at;
                        at += (int)(B.P.rowptr[gr + 1] - B.P.rowptr[gr]);
                    }
                    rptr[M + V] = at;
                }
                ctl[6] = (double)(nz - NNZ);
                ctl[7] = fits ? 0.0 : 1.0;
            }
            __syncthreads();
            nnzV = (int)ctl[6];
            if (ctl[7] != 0.0) { overflow = true; status = KTN_STATUS_ERROR; break; }
            // gencut + round_coefs + _addcut (src/algorithms.jl:3-18, src/model.jl:68-79,200-207): 16 lanes per violated row
            const int lane = tid & 15;
            for (int i = tid / 16; i < m_nl; i += kEcpThreads / 16) {
                if (!(icnt[i] & 1)) continue;
                const int rnew = M + (icnt[i] >> 1);
                const int32_t gr = B.nl_rows[nl0 + i];
                const int64_t beg = B.P.rowptr[gr], end = B.P.rowptr[gr + 1];
                const int dst = rptr[rnew];
                // (tape and QUAD rows: the eval pass left their entries in B.jac)
                const bool in_jac = (B.has_tape && B.P.row_kind[gr] == KTN_ROW_TAPE) || (B.has_quad && B.P.row_kind[gr] == KTN_ROW_QUAD);
                // (ESH) the cut point x_int + lamc (x* - x_int) and g there; lamc == 1: Kelley's cut, the loop below as it ever was.
                // gr, sg and the row's kind are uniform within the 16 lanes, and so is every trip count below.
                double lamc = 1.0, gcut = 0.0;
                bool qmoved = false;
                if constexpr (ESH != 0) {
                    const EcpEsh& E = ecp_esh_arg(esh_arg...);
                    const int sg = (int)E.sig[gr];
                    const double* xi = E.xint + c0;
                    const double tol = E.root_tol * f_eff;
                    if (sg != 0 && !in_jac) {
                        // separable row: the bracketed Newton of esh.hpp on phi(lambda) = sg (g(x_int + lambda (x* - x_int)) - bound)
                        const double bound = sg > 0 ? B.P.ub[gr] : B.P.lb[gr];
                        const double rc = B.P.rconst[gr];
                        EshState S;
                        esh_init(S);
                        int np = 0;
                        for (int it = 0; it < E.iters && !S.done; ++it) {
                            const double lam = S.lam;
                            RowAcc acc;
                            double acc_d = 0.0;
                            for (int64_t e = beg + lane; e < end; e += 16) {
                                const int ck = B.P.colk[e];
                                const double2 pp = B.P.pp[e];
                                const int cl = (ck & kColMask) - (int)c0;
                                const double xv = xs[cl], x0 = xi[cl];
                                const double xp = esh_point(xv, x0, lam);
                                double val, der;
                                atom_eval((unsigned)ck >> kKindShift, pp.x, pp.y, xp, val, der);
                                acc.add(val, der, xp);
                                acc_d += der * (xv - x0);
                            }
                            acc.template reduce<16>();
                            acc_d = group_sum<16>(acc_d);
                            const double g = acc.g + rc;
                            const double phi = sg * (g - bound);
                            ++np;
                            if (esh_step(S, phi, sg * acc_d, !acc.nf && isfinite(phi), tol)) gcut = g;
                        }
                        if (S.have) lamc = S.best;
                        if (lane == 0) esh_cnt[2] += np;
                    } else if (sg != 0 && E.jint != nullptr && B.has_quad && B.P.row_kind[gr] == KTN_ROW_QUAD) {
                        // QUAD row: the closed form of esh_quad.hpp from J* (B.jac, ecp_quad_entries), J0 (jint) and g* (yts[i])
                        double p1 = 0.0, p0 = 0.0;
                        int nfq = 0;
                        for (int64_t e = beg + lane; e < end; e += 16) {
                            const int cl = (B.P.colk[e] & kColMask) - (int)c0;
                            const double js = B.jac[e], j0 = E.jint[e];
                            const double d = xs[cl] - xi[cl];
                            p1 += js * d;
                            p0 += j0 * d;
                            nfq |= !(isfinite(js) && isfinite(j0) && isfinite(d));
                        }
                        p1 = group_sum<16>(p1);
                        p0 = group_sum<16>(p0);
                        nfq = group_or<16>(nfq);
                        const double gs = yts[i];
                        const EshQuadRoot R = esh_quad_root(true, sg, gs, sg > 0 ? B.P.ub[gr] : B.P.lb[gr], tol, p1, p0, nfq);
                        if (R.moved) { lamc = R.lam; gcut = esh_quad_gb(gs, R.lam, p1, R.q); qmoved = true; }
                        if (lane == 0) esh_cnt[2] += 1;
                    }
                    if (lane == 0) { esh_cnt[lamc < 1.0 ? 0 : 1] += 1; if (qmoved) esh_cnt[3] += 1; }
                }
                const bool moved = ESH != 0 && lamc < 1.0;
                double dot = 0.0, mx = -__builtin_inf();
                int nf = 0;
                for (int64_t e = beg + lane; e < end; e += 16) {
                    const int ck = B.P.colk[e];
                    const int cl = (ck & kColMask) - (int)c0;
                    double der;
                    if constexpr (ESH != 0) {
                        if (moved) {
                            const EcpEsh& E = ecp_esh_arg(esh_arg...);
                            const double xp = esh_point(xs[cl], E.xint[c0 + cl], lamc);
                            if (qmoved) {
                                der = esh_quad_coef(lamc, B.jac[e], E.jint[e]);
                            } else {
                                const double2 pp = B.P.pp[e];
                                double val;
                                atom_eval((unsigned)ck >> kKindShift, pp.x, pp.y, xp, val, der);
                            }
                            dot += xp * der;
                            mx = nanmax(mx, der);
                            nf |= !isfinite(der);
                            rcol[dst + (int)(e - beg)] = (uint16_t)cl;
                            rval[dst + (int)(e - beg)] = der;
                            continue;
                        }
                    }
                    if (in_jac) {
                        der = B.jac[e];
                    } else {
                        const double2 pp = B.P.pp[e];
                        double val;
                        atom_eval((unsigned)ck >> kKindShift, pp.x, pp.y, xs[cl], val, der);
                    }
                    dot += xs[cl] * der;
                    mx = nanmax(mx, der);
                    nf |= !isfinite(der);
                    rcol[dst + (int)(e - beg)] = (uint16_t)cl;
                    rval[dst + (int)(e - beg)] = der;
                }
                dot = group_sum<16>(dot);
                mx = group_nanmax<16>(mx);
                nf = group_or<16>(nf);
                if (B.P.pad_zero[gr]) mx = nanmax(mx, 0.0);
                for (int64_t e = beg + lane; e < end; e += 16) {                          // round_coefs (signed max)
                    const double der = rval[dst + (int)(e - beg)];
                    if (round_coef(der, mx, B.cut_coef_rng)) rval[dst + (int)(e - beg)] = 0.0;
                }
                if (lane == 0) {
                    const double bconst = (moved ? gcut : yts[i]) - dot;
                    if constexpr (ESH != 0) ecp_esh_arg(esh_arg...).lam[A.row0 + rnew] = lamc;
                    lo[rnew] = B.P.lb[gr] - bconst;
                    hi[rnew] = B.P.ub[gr] - bconst;
                    const int prev = last_cut[i];
                    double y0 = 0.0;
                    if (prev >= 0) { y0 = yv[prev]; yv[prev] = 0.0; }
                    yv[rnew] = y0;
                    cut_prev[rnew] = prev;
                    last_cut[i] = rnew;
                    if (nf) bad_nf = 1;
                }
            }
            {
                double t1[1] = {(double)bad_nf};
                wg_reduce<kEcpThreads, 1>(t1, 0, red, q);
                if (q[0] != 0.0) { status = KTN_STATUS_ERROR; __syncthreads(); break; }    // model.jl:69-73
            }
            M += V; NNZ += nnzV; numcuts += V;
        }
        __syncthreads();
        last_maxviol = mv[0];
        const bool sat_now = V == 0;
        if (sat_now && tol_p > floor_p * (1.0 + 1e-12)) last_maxviol = 0.0;        // inexact-LP rule: re-solve at the floor tolerance
        else allsat = sat_now;
        if (refining && mv[0] <= B.f_tol && mv[0] < best_viol) {                    // a candidate for the answer (uniform: mv is reduced)
            best_viol = mv[0]; best_obj = objval;
            for (int j = tid; j < nb; j += kEcpThreads) xbest[j] = xg[j];
        }
    }
    // ---- certificate: refine, or done
    if (!allsat && !refining) break;                                               // iteration cap
    if (status != KTN_STATUS_NONE || !(B.cert_tol > 0.0) || m_nl == 0 || B.polish_max_iter <= 0) break;
    if (refining && passes > B.polish_max_iter) break;
    {
        double d1[1] = {0.0};
        for (int i = tid; i < m_nl; i += kEcpThreads) {
            double lam = 0.0;
            for (int r = last_cut[i]; r >= 0; r = cut_prev[r]) lam += fabs(yv[r]);
            const int32_t gr = B.nl_rows[nl0 + i];
            const double lb = B.P.lb[gr], ub = B.P.ub[gr], g = yts[i];
            double v = -__builtin_inf();
            if (isfinite(ub)) v = fmax(v, g - ub);
            if (isfinite(lb)) v = fmax(v, lb - g);
            if (v >= -10.0 * B.f_tol) d1[0] += lam * v;
        }
        wg_reduce<kEcpThreads, 1>(d1, 1, red, q);
        const double D = (q[0] == q[0]) ? fmax(q[0], 0.0) : __builtin_inf();
        const double target = B.cert_tol * fmax(1.0, fabs(objval));
        __syncthreads();
        if (allsat && D <= 0.5 * target) break;                                     // the reference's objective tolerance holds
        if (!refining) {                                                            // the point that met the stop rule is the first candidate
            refining = true;
            best_viol = B.f_tol; best_obj = objval;                                 // (any later point that is strictly inside replaces it)
            for (int j = tid; j < nb; j += kEcpThreads) xbest[j] = xg[j];
        }
        f_eff = fmin(fmax(0.25 * target / D, 0.05), 0.5) * B.f_tol;
        gap_cert = 0.25 * target / (1.0 + 2.0 * fabs(objval));
        allsat = false;
        last_maxviol = 0.0;
    }
  }
    if (refining) {                                                                 // the best point that satisfies the reference's rule
        __syncthreads();
        for (int j = tid; j < nb; j += kEcpThreads) xg[j] = xbest[j];
        objval = best_obj;
        allsat = true;
        last_maxviol = best_viol;
    }
    if (status == KTN_STATUS_NONE) status = (iter >= B.iter_cap && !allsat) ? KTN_STATUS_USERLIMIT : (allsat ? KTN_STATUS_OPTIMAL : KTN_STATUS_USERLIMIT);
    if (tid == 0) {
        double* o = B.res + (int64_t)b * 8;
        o[0] = (double)status; o[1] = (double)iter; o[2] = objval; o[3] = (double)numcuts; o[4] = (double)pdhg_total;
        o[5] = last_maxviol; o[6] = (double)M; o[7] = overflow ? 1.0 : 0.0;
    }
    if constexpr (ESH != 0) {                                                       // each workgroup owns its four counters
        double c4[4] = {(double)esh_cnt[0], (double)esh_cnt[1], (double)esh_cnt[2], (double)esh_cnt[3]};
        __syncthreads();
        wg_reduce<kEcpThreads, 4>(c4, 4, red, q);
        if (tid < 4) ecp_esh_arg(esh_arg...).res[(int64_t)b * 4 + tid] = q[tid];
    }
}

}  // namespace ktn
