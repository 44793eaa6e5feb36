// feas.hpp -- a feasible point and a primal bound after a solve: the other side of the root search of esh.hpp.
// Launched by Engine::feas_compute (feas.hip) only, on the first ktn_get_feasible_point after a solve: a solve that is followed by
// no getter launches none of these kernels.
//
// On the segment from the reference point x_in (feasible) to the LP point x* a taking-part row i with side sigma_i and bound b_i has
//     phi_i(lambda) = sigma_i (g_i(x_in + lambda (x* - x_in)) - b_i)          (the definitions of esh.hpp; the point by esh_point)
// The cut search of esh.hpp stops at the last point with phi >= 0, because a cut wants to separate.  Here every taking-part row --
// violated at x* or not -- gets lambda_i, the last point the search saw with a FINITE phi <= 0:
//     lambda_i = 1                                   where phi_i(1) <= 0 (one pass: a convex row feasible at both ends is feasible between)
//     -tau <= phi_i(lambda_i) <= 0, lambda_i < 1     otherwise, tau = esh_root_tol * f_tol
// by bracketed Newton on phi + tau / 2 from lambda = 1 (for a convex row the iterates come down on the root of phi + tau / 2 from the
// right and enter the window from above, its middle being the target as in k_esh_quad), bisection when a step leaves the bracket or
// the derivative is of no use.  VALIDITY NEVER DEPENDS ON CONVERGENCE: the answer is the bracket's lower end `lo`, which starts at 0
// (x_in, verified feasible by k_feas_verify) and only ever moves to a point with a finite phi <= 0.  A row that runs out of passes
// is flagged (unc) and keeps its lo.
//
//   k_feas_sep<G>    separable rows, G lanes per row over all NL slots (the k_esh_sep layout)
//   k_feas_long      rows of k_sep_eval_long, one 1 024-thread workgroup per row
//   k_feas_tape      tape rows, one lane per row through tape_row_eval, the Jacobian into the feature's own scratch
//   k_feas_quad<G>   QUAD rows: closed form from the Jacobians at x* and x_in, the search on the row's three scalar coefficients otherwise
//   k_feas_min_partial / k_feas_min_final    lambda* = min over the NL slots and the smallest row attaining it: fixed order, no atomics
//   k_feas_point     x_feas = clamp(esh_point(x*, x_in, lambda*), l, u), lambda* read from device memory
//   k_feas_verify_partial / k_feas_verify_final   the maxima of info[3..5] at a point whose rows precompute_all has evaluated
//   k_feas_min_blocks / k_feas_point_blocks / k_feas_verify_blocks   the same per instance of a fused batch, one workgroup per instance
//
// All FP64; the only atomic is the integer counter of evaluation passes; every reduction has a fixed shape.
#pragma once
#include "esh.hpp"
#include "quad_rows.hpp"

namespace ktn {

struct FeasArgs {
    const double* x;               // x* (n0 + 1 entries; the last one is not read by a taking-part row)
    const double* xi;              // x_in
    const int8_t* sig;             // per extended row: sigma_i when row i takes part, else 0
    double* lam;                   // per NL SLOT: lambda_i (filled with 1 before the search; rows that do not take part keep it)
    int32_t* unc;                  // per NL SLOT: 1 where the row ended unconverged (zeroed before the search)
    unsigned long long* cnt;       // [0] evaluation passes (a statistic: the only atomic of the feature)
    double tau;                    // the accepted window is -tau <= phi <= 0
    int iters;                     // passes per row at most
};

// The search, defined once (every lane / thread that holds a row runs it on the same numbers)
struct FeasState {
    double lo, hi, lam;
    bool done, conv;
};
__device__ __forceinline__ void feas_init(FeasState& s) { s.lo = 0.0; s.hi = 1.0; s.lam = 1.0; s.done = false; s.conv = false; }
// phi, dphi at s.lam; fin: phi and every derivative of the row finite.  Afterwards s.lo is the row's answer so far.
__device__ __forceinline__ void feas_step(FeasState& s, double phi, double dphi, bool fin, double tau) {
    if (fin && phi <= 0.0) {                   // a finite phi <= 0: the point is the row's
        s.lo = s.lam;
        if (s.lam == 1.0 || phi >= -tau) { s.done = true; s.conv = true; return; }
    } else {                                   // phi > 0, +-inf or NaN: the answer lies below lambda
        s.hi = s.lam;
    }
    double nl = s.lam - (phi + 0.5 * tau) / dphi;
    if (!(fin && dphi > 0.0 && isfinite(nl) && nl > s.lo && nl < s.hi)) nl = 0.5 * (s.lo + s.hi);
    s.lam = nl;
}

// separable rows: G lanes per row.  rows[k] is NL slot k's row.
template <int G>
__global__ __launch_bounds__(kBlock) void k_feas_sep(NlpDev P, const int32_t* __restrict__ rows, int64_t n, FeasArgs A) {
    const int64_t gid = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    const int lane = threadIdx.x & (G - 1);
    // (no early return: every lane of the wavefront takes part in the butterflies and the ballot)
    const int32_t r = gid < n ? rows[gid] : 0;
    const bool sep = gid < n && P.row_kind[r] == KTN_ROW_SEP;
    const int sg = sep ? (int)A.sig[r] : 0;
    const bool part = sg != 0;
    bool active = part;
    const int64_t beg = part ? P.rowptr[r] : 0, end = part ? P.rowptr[r + 1] : 0;
    const double bound = sg > 0 ? P.ub[r] : (sg < 0 ? P.lb[r] : 0.0);
    const double rc = part ? P.rconst[r] : 0.0;
    FeasState S;
    feas_init(S);
    unsigned long long passes = 0;
    for (int it = 0; it < A.iters; ++it) {
        if (__ballot(active) == 0ull) break;          // uniform trip count per wavefront; finished groups sit predicated off
        const double lam = S.lam;
        RowAcc acc;
        double acc_d = 0.0;
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
            const double phi = sg * ((acc.g + rc) - bound), dphi = sg * acc_d;
            ++passes;
            feas_step(S, phi, dphi, !acc.nf && isfinite(phi), A.tau);
            if (S.done) active = false;
        }
    }
    if (lane == 0 && part) {
        A.lam[gid] = S.lo;
        A.unc[gid] = S.conv ? 0 : 1;
    }
    // the pass counter: one atomic per wavefront (one per row puts every row of the launch on the same address)
    unsigned int pw = (lane == 0 && part) ? (unsigned int)passes : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) pw += __shfl_xor(pw, off, 64);
    if ((threadIdx.x & 63) == 0 && pw) atomicAdd(&A.cnt[0], (unsigned long long)pw);
}

// rows of k_sep_eval_long (device kind kRowSepLong): one workgroup per row
static __global__ __launch_bounds__(1024) void k_feas_long(NlpDev P, const int32_t* __restrict__ rows, const int64_t* __restrict__ slots, FeasArgs A) {
    __shared__ double sh[16][2];
    __shared__ int shn[16];
    const int32_t r = rows[blockIdx.x];
    const int64_t slot = slots[blockIdx.x];
    const int sg = (int)A.sig[r];
    if (sg == 0 || slot < 0) return;                 // (uniform over the workgroup)
    const int64_t beg = P.rowptr[r], end = P.rowptr[r + 1];
    const double bound = sg > 0 ? P.ub[r] : P.lb[r];
    const int wv = threadIdx.x >> 6;
    FeasState S;
    feas_init(S);
    unsigned long long passes = 0;
    for (int it = 0; it < A.iters && !S.done; ++it) {
        // one pass at S.lam: every thread ends with the same totals (partials combined in wavefront order)
        RowAcc a;
        double ad = 0.0;
        for (int64_t e = beg + threadIdx.x; e < end; e += 1024) {
            const int ck = P.colk[e];
            const double2 q = P.pp[e];
            const int c = ck & kColMask;
            const double xs = A.x[c], x0 = A.xi[c];
            const double xv = esh_point(xs, x0, S.lam);
            double val, der;
            atom_eval((unsigned)ck >> kKindShift, q.x, q.y, xv, val, der);
            a.add(val, der, xv); ad += der * (xs - x0);
        }
        a.reduce<64>(); ad = group_sum<64>(ad);
        if ((threadIdx.x & 63) == 0) { sh[wv][0] = a.g; sh[wv][1] = ad; shn[wv] = a.nf; }
        __syncthreads();
        double g = sh[0][0], d = sh[0][1];
        int nf = shn[0];
        for (int k = 1; k < 16; ++k) { g += sh[k][0]; d += sh[k][1]; nf |= shn[k]; }
        g += P.rconst[r];
        __syncthreads();                             // (the cells are reused by the next pass)
        ++passes;
        const double phi = sg * (g - bound);
        feas_step(S, phi, sg * d, !nf && isfinite(phi), A.tau);
    }
    if (threadIdx.x == 0) {
        A.lam[slot] = S.lo;
        A.unc[slot] = S.conv ? 0 : 1;
        atomicAdd(&A.cnt[0], passes);
    }
}

// tape rows: one lane per row; jac is the feature's own Jacobian scratch (indexed like the structure), never the sweep's
static __global__ __launch_bounds__(kBlock) void k_feas_tape(NlpDev P, const int32_t* __restrict__ rows, const int32_t* __restrict__ slots,
                                                      int64_t n, FeasArgs A, double* __restrict__ jac) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const int32_t r = rows[t];
    const int sg = (int)A.sig[r];
    if (sg == 0 || P.row_kind[r] != KTN_ROW_TAPE) return;
    const double bound = sg > 0 ? P.ub[r] : P.lb[r];
    const int64_t beg = P.rowptr[r], end = P.rowptr[r + 1];
    FeasState S;
    feas_init(S);
    unsigned long long passes = 0;
    for (int it = 0; it < A.iters && !S.done; ++it) {
        const double lam = S.lam;
        const double g = tape_row_eval(P, r, [&](int32_t c) { return esh_point(A.x[c], A.xi[c], lam); }, jac);
        double d = 0.0;
        int nf = 0;
        for (int64_t e = beg; e < end; ++e) {
            const int c = P.col[e];
            const double der = jac[e];
            d += der * (A.x[c] - A.xi[c]);
            nf |= !isfinite(der);
        }
        ++passes;
        const double phi = sg * (g - bound);
        feas_step(S, phi, sg * d, !nf && isfinite(phi), A.tau);
    }
    A.lam[slots[t]] = S.lo;
    A.unc[slots[t]] = S.conv ? 0 : 1;
    if (passes) atomicAdd(&A.cnt[0], passes);
}

// QUAD rows, G lanes per row over a QuadList (the k_quad_stats / k_esh_quad layout).  gs, js: values and Jacobian at x*; j0: the
// Jacobian at x_in -- all three evaluated by this feature into its own buffers.  With d = x* - x_in, mu = 1 - lambda,
// P1 = sum J*_e d_e, P0 = sum J0_e d_e, q = P1 - P0 (esh_quad.hpp):
//     phi(lambda) = phi1 - mu sigma P1 + 1/2 mu^2 sigma q,   phi' = sigma P1 - mu sigma q,   phi1 = sigma (g* - bound)
// phi1 <= 0: lambda = 1.  Otherwise phi = -tau / 2 at mu = 2 c / (sigma P1 + sqrt((sigma P1)^2 - 2 sigma q c)), c = phi1 + tau / 2, the
// root free of cancellation; it is taken when every number is finite, the discriminant >= 0, sigma P1 > 0, 0 <= lambda < 1 and the
// three coefficients put phi(lambda) inside [-tau, 0].  Where that fails the row runs feas_step on the three coefficients (Newton
// while the derivative is of use, bisection otherwise; non-finite coefficients leave lo = 0 and the row counted as unconverged).
template <int G>
__global__ __launch_bounds__(kBlock) void k_feas_quad(NlpDev P, QuadList L, const double* __restrict__ gs, const double* __restrict__ js,
                                                      const double* __restrict__ j0, FeasArgs A) {
    const int64_t gid = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    const int lane = threadIdx.x & (G - 1);
    // (no early return: every lane takes part in the butterflies)
    const bool listed = gid < L.n_rows;
    const int32_t r = listed ? L.rows[gid] : 0;
    const int sg = listed ? (int)A.sig[r] : 0;
    const bool live = sg != 0;
    const int64_t beg = live ? P.rowptr[r] : 0, end = live ? P.rowptr[r + 1] : 0;
    double p1 = 0.0, p0 = 0.0;
    for (int64_t e = beg + lane; e < end; e += G) {
        const int c = P.col[e];
        const double d = A.x[c] - A.xi[c];
        p1 += js[e] * d;
        p0 += j0[e] * d;
    }
    p1 = group_sum<G>(p1);
    p0 = group_sum<G>(p0);
    if (!(lane == 0 && live)) return;                // (the butterflies are behind us)
    const double bound = sg > 0 ? P.ub[r] : P.lb[r];
    const double phi1 = sg * (gs[r] - bound), sp1 = sg * p1, sq = sg * (p1 - p0);
    auto phi_at = [&](double lam) { const double mu = 1.0 - lam; return phi1 - mu * sp1 + 0.5 * (mu * mu) * sq; };
    FeasState S;
    feas_init(S);
    unsigned long long passes = 1;
    if (isfinite(phi1) && phi1 <= 0.0) {
        S.lo = 1.0; S.conv = true;
    } else {
        const double c = phi1 + 0.5 * A.tau;
        const double disc = sp1 * sp1 - 2.0 * sq * c;
        const double mu = 2.0 * c / (sp1 + sqrt(disc));
        const double lam = 1.0 - mu;
        const double pl = phi_at(lam);
        if (isfinite(mu) && disc >= 0.0 && sp1 > 0.0 && lam >= 0.0 && lam < 1.0 && pl <= 0.0 && pl >= -A.tau) {
            S.lo = lam; S.conv = true;
        } else {
            passes = 0;
            for (int it = 0; it < A.iters && !S.done; ++it) {
                const double phi = phi_at(S.lam), dphi = sp1 - (1.0 - S.lam) * sq;
                ++passes;
                feas_step(S, phi, dphi, isfinite(phi) && isfinite(dphi), A.tau);
            }
        }
    }
    A.lam[L.slots[gid]] = S.lo;
    A.unc[L.slots[gid]] = S.conv ? 0 : 1;
    atomicAdd(&A.cnt[0], passes);
}

// ---- lambda* = min over the NL slots, and the smallest ROW attaining it: (lambda, row) pairs under the lexicographic order, which is
// associative and commutative exactly, in a fixed shape all the same -- butterfly, the wavefronts' cells in order, block partials,
// one final block.  The number of unconverged rows rides along (a sum of small integers: exact in any order).
struct FeasMin { double lam, row, unc; };       // (row and count as doubles: exact below 2^53, and one shuffle type)
__device__ __forceinline__ FeasMin feas_min(FeasMin a, FeasMin b) {
    const bool tb = b.lam < a.lam || (b.lam == a.lam && b.row < a.row);
    return FeasMin{tb ? b.lam : a.lam, tb ? b.row : a.row, a.unc + b.unc};
}
__device__ __forceinline__ FeasMin feas_block_min(FeasMin v, FeasMin* sh) {          // sh: kBlock / 64 cells; valid in thread 0
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = feas_min(v, FeasMin{__shfl_xor(v.lam, off, 64), __shfl_xor(v.row, off, 64), __shfl_xor(v.unc, off, 64)});
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < kBlock / 64; ++k) v = feas_min(v, sh[k]);
    return v;
}
// res[0] = lambda*, res[1] = the blocking row (-1: no row below 1), res[2] = rows unconverged, res[3] = the lambda x_feas is formed with
__device__ __forceinline__ void feas_store_min(const FeasMin& v, double* __restrict__ res) {
    const bool blocked = v.lam < 1.0;
    res[0] = blocked ? v.lam : 1.0;
    res[1] = blocked ? v.row : -1.0;
    res[2] = v.unc;
    res[3] = res[0];
}
static __global__ __launch_bounds__(kBlock) void k_feas_min_partial(int64_t n, const double* __restrict__ lam, const int32_t* __restrict__ unc,
                                                             const int32_t* __restrict__ rows, FeasMin* __restrict__ part) {
    __shared__ FeasMin sh[kBlock / 64];
    FeasMin v{__builtin_inf(), __builtin_inf(), 0.0};
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < n; s += (int64_t)gridDim.x * kBlock)
        v = feas_min(v, FeasMin{lam[s], (double)rows[s], (double)unc[s]});
    v = feas_block_min(v, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}
static __global__ __launch_bounds__(kBlock) void k_feas_min_final(const FeasMin* __restrict__ part, int np, double* __restrict__ res) {
    __shared__ FeasMin sh[kBlock / 64];
    FeasMin v{__builtin_inf(), __builtin_inf(), 0.0};
    for (int k = threadIdx.x; k < np; k += kBlock) v = feas_min(v, part[k]);
    v = feas_block_min(v, sh);
    if (threadIdx.x == 0) feas_store_min(v, res);
}
// the blocks form: one workgroup per instance over the instance's slot range (seg: the six offsets per instance of k_dual_bound,
// the NL slots at [2], [3] behind n_lin linear rows); an instance without nonlinear rows gets lambda_b = 1
static __global__ __launch_bounds__(kBlock) void k_feas_min_blocks(const int64_t* __restrict__ seg, int64_t n_lin, const double* __restrict__ lam,
                                                            const int32_t* __restrict__ unc, const int32_t* __restrict__ rows, double* __restrict__ res) {
    __shared__ FeasMin sh[kBlock / 64];
    const int64_t* sg = seg + 6 * (int64_t)blockIdx.x;
    FeasMin v{__builtin_inf(), __builtin_inf(), 0.0};
    for (int64_t s = sg[2] - n_lin + threadIdx.x; s < sg[3] - n_lin; s += kBlock) v = feas_min(v, FeasMin{lam[s], (double)rows[s], (double)unc[s]});
    v = feas_block_min(v, sh);
    if (threadIdx.x == 0) feas_store_min(v, res + 4 * (int64_t)blockIdx.x);
}

// The engine's OWN reference point meets the variable bounds only to its auxiliary LP's tolerance (seen: 1e-16 .. 2e-15 outside): it is
// clamped into [l, u] before anything is evaluated there.  A caller's point is taken as given (found = -1 if it lies outside).
static __global__ __launch_bounds__(kBlock) void k_feas_clamp(int64_t n, double* __restrict__ x, const double* __restrict__ l, const double* __restrict__ u) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < n) x[j] = clampd(x[j], l[j], u[j]);
}

// x_feas_j = clamp(esh_point(x*_j, x_in_j, lambda), l_j, u_j) with lambda = res[0] * shrink (shrink = 1: res[0] itself; a back-off
// otherwise); thread 0 leaves the lambda used in res[3] and a zero in the slot of the epigraph variable.
static __global__ __launch_bounds__(kBlock) void k_feas_point(int64_t n, const double* __restrict__ xs, const double* __restrict__ xi,
                                                       const double* __restrict__ l, const double* __restrict__ u, double shrink,
                                                       double* __restrict__ res, double* __restrict__ xf) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const double lam = (shrink == 1.0) ? res[0] : res[0] * shrink;
    if (j == 0) { res[3] = lam; xf[n] = 0.0; }
    if (j < n) xf[j] = clampd(esh_point(xs[j], xi[j], lam), l[j], u[j]);
}
// the blocks form: column j takes the lambda_b of its instance (blkcol: nb + 1 ascending column offsets) and that instance's shrink
static __global__ __launch_bounds__(kBlock) void k_feas_point_blocks(int64_t n, const int64_t* __restrict__ blkcol, int64_t nb, const double* __restrict__ xs,
                                                              const double* __restrict__ xi, const double* __restrict__ l, const double* __restrict__ u,
                                                              const double* __restrict__ shrink, double* __restrict__ res, double* __restrict__ xf) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j == 0) xf[n] = 0.0;
    if (j >= n) return;
    int64_t lo = 0, hi = nb;                                      // blkcol[lo] <= j < blkcol[hi]
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (blkcol[mid] <= j) lo = mid; else hi = mid; }
    const double sh = shrink[lo];
    const double lam = (sh == 1.0) ? res[4 * lo] : res[4 * lo] * sh;
    if (j == blkcol[lo]) res[4 * lo + 3] = lam;
    xf[j] = clampd(esh_point(xs[j], xi[j], lam), l[j], u[j]);
}

// ---- the verification of a point whose rows precompute_all has evaluated into g: four maxima (NaN counts as +inf)
//   [0] max sigma_i (g_i - b_i) over the taking-part rows (-inf: none)      [1] largest violation of a linear row (>= 0)
//   [2] minus the first taking-part row with sigma (g - b) > 0 or not finite (-inf: none)
//   [3] 1 where a coordinate of x lies outside [l, u] or is NaN, else 0
// block partials (wg_reduce: butterfly, then the wavefronts in order), then one final thread over the partials in order; a max is
// order-independent anyway.  rowmap[i] >= 0: row i is linear (the KKT report's map, built at load).
struct FeasVerify {
    const int8_t* sig; const int32_t* rowmap; const double* g; const double* lb; const double* ub;
    const double* x; const double* l; const double* u;
};
__device__ __forceinline__ void feas_verify_row(const FeasVerify& V, int64_t i, double (&v)[4]) {
    const int sg = (int)V.sig[i];
    const double gi = V.g[i];
    if (sg != 0) {
        double w = sg * (gi - (sg > 0 ? V.ub[i] : V.lb[i]));
        if (w != w) w = __builtin_inf();
        v[0] = fmax(v[0], w);
        if (!(w <= 0.0)) v[2] = fmax(v[2], -(double)i);
    }
    if (V.rowmap[i] >= 0) {
        double w = fmax(gi - V.ub[i], V.lb[i] - gi);
        if (w != w) w = __builtin_inf();
        v[1] = fmax(v[1], w);
    }
}
__device__ __forceinline__ void feas_verify_col(const FeasVerify& V, int64_t j, double (&v)[4]) {
    if (!(V.x[j] >= V.l[j] && V.x[j] <= V.u[j])) v[3] = 1.0;
}
static __global__ __launch_bounds__(kBlock) void k_feas_verify_partial(int64_t m0, int64_t n, FeasVerify V, double* __restrict__ part) {
    __shared__ double red[(kBlock / 64) * 4];
    __shared__ double out[4];
    double v[4] = {-__builtin_inf(), 0.0, -__builtin_inf(), 0.0};
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m0 + n; i += stride) {
        if (i < m0) feas_verify_row(V, i, v);
        else feas_verify_col(V, i - m0, v);
    }
    wg_reduce<kBlock, 4>(v, 0, red, out);
    if (threadIdx.x < 4) part[4 * blockIdx.x + threadIdx.x] = out[threadIdx.x];
}
// the blocks form: one workgroup per instance over its rows (brows[browptr[b] .. browptr[b + 1]): the caller rows of instance b) and
// its columns (seg [4], [5], offset by m0); out[8 b + 0..3] the maxima with [2] turned into the row index (-1: none), out[8 b + 4] the
// instance's share c_b'x_b of the objective as k_dual_bound forms it (block_sum: a fixed shape)
static __global__ __launch_bounds__(kBlock) void k_feas_verify_blocks(const int64_t* __restrict__ seg, int64_t m0, const int64_t* __restrict__ browptr,
                                                               const int32_t* __restrict__ brows, FeasVerify V, const double* __restrict__ obj_c,
                                                               double* __restrict__ outb) {
    __shared__ double red[(kBlock / 64) * 4];
    __shared__ double out[4];
    __shared__ double shs[kBlock / 64];
    const int64_t b = blockIdx.x;
    double v[4] = {-__builtin_inf(), 0.0, -__builtin_inf(), 0.0};
    double f = 0.0;
    for (int64_t k = browptr[b] + threadIdx.x; k < browptr[b + 1]; k += kBlock) feas_verify_row(V, brows[k], v);
    for (int64_t j = seg[6 * b + 4] - m0 + threadIdx.x; j < seg[6 * b + 5] - m0; j += kBlock) { feas_verify_col(V, j, v); f += obj_c[j] * V.x[j]; }
    wg_reduce<kBlock, 4>(v, 0, red, out);
    f = block_sum<kBlock>(f, shs);
    if (threadIdx.x == 0) {
        double* o = outb + 8 * b;
        o[0] = out[0]; o[1] = out[1]; o[2] = isfinite(out[2]) ? -out[2] : -1.0; o[3] = out[3]; o[4] = f;
    }
}
// out[0..3] as above with out[2] turned into the row index (-1: none), out[4] = f = g[m0] + x[n0] as k_dual_final forms it
static __global__ void k_feas_verify_final(const double* __restrict__ part, int np, const double* __restrict__ g, const double* __restrict__ x,
                                    int64_t m0, int64_t n0, double* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double v[4] = {-__builtin_inf(), 0.0, -__builtin_inf(), 0.0};
    for (int k = 0; k < np; ++k)
        for (int q = 0; q < 4; ++q) v[q] = fmax(v[q], part[4 * k + q]);
    out[0] = v[0]; out[1] = v[1]; out[2] = isfinite(v[2]) ? -v[2] : -1.0; out[3] = v[3];
    out[4] = g[m0] + x[n0];
}

}  // namespace ktn
