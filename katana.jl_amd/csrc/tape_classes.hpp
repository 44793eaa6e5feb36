// tape_classes.hpp -- tape rows evaluated by SHAPE CLASS: k_tape_classed ("tape rows by shape class").
//
// Rows of one class share the node list (opcodes, operand indices, POWC exponents, relative Jacobian slots, structure
// length); what differs per row -- CONST values and structure columns -- is stored class-major, so lane-consecutive is
// address-consecutive.  A wavefront takes 64 consecutive members of ONE class: the program is read once per wavefront
// (uniform loads), the opcode switch does not diverge, node values, adjoints and the row's Jacobian entries live in an LDS
// image [cell][lane] of 8-byte cells (lane l of a 32-lane half touches one 256-byte bank row: conflict-free), and the
// per-row part of k_gj_stats is folded in.  The arithmetic is tape_node_forward / tape_node_reverse of kernels.hpp, in the
// node order of the interpreter: the results are bit for bit those of k_tape_eval + k_gj_stats.
#pragma once
#include "kernels.hpp"

namespace ktn {

constexpr int kTapeClassMin = 64;        // rows (one full wavefront) from which a class is evaluated by k_tape_classed
constexpr int kTapeClassWave = 64;       // lanes = rows per workgroup (one wavefront)
// LDS cells of 64 x 8 B per wavefront: 2 per node (value, adjoint) + 1 per structure entry.  312 cells = 156 KiB, what one
// wavefront can have of a CU's 160 KiB; a class that needs more stays with the interpreter.  Classes are launched by size
// bucket (cells <= 32, 64, 128, 312), so a long class does not take the occupancy of the short ones.
constexpr int kTapeClassMaxCells = 312;
__host__ __device__ inline int tape_class_bucket(int64_t cells) { return cells <= 32 ? 0 : cells <= 64 ? 1 : cells <= 128 ? 2 : 3; }

struct TapeClassMeta {
    int32_t count;      // member rows
    int32_t nnodes;     // nodes of the program
    int32_t nslots;     // structure length of a member row
    int32_t prog0;      // first node in prog_*
    int64_t mem0;       // first member in mrow / the slot list
    int64_t cst0;       // constant k of member j: cst[cst0 + k * count + j]
    int64_t col0;       // structure column s of member j: scol[col0 + s * count + j]
};

struct TapeClassDev {
    const int32_t* wave_cls;     // class of wavefront w
    const int32_t* wave_first;   // its first member (position inside the class)
    const TapeClassMeta* meta;
    const int32_t* prog_op;
    const int32_t* prog_a;       // operand a | ordinal of a CONST among the row's constants
    const int32_t* prog_b;       // operand b | Jacobian slot of a VAR relative to the row's rowptr
    const double* prog_c;        // POWC exponent
    const double* cst;
    const int32_t* scol;
    const int32_t* mrow;         // member row ids, ascending inside a class
};

// precompute! + the row tail (k_gj_stats' part) of the rows of the classed classes.  One wavefront per workgroup; `mslot` gives the
// index under which a member's flag / cnt are stored: its NL slot in the sweep, its row in precompute_all (k_gj_stats over
// all rows does the same there).  wave_cls / wave_first point at the launch's first wavefront.  Dynamic LDS: (2 nnodes + nslots) * 512 B
// of the largest launched class.
static __global__ __launch_bounds__(kTapeClassWave) void k_tape_classed(NlpDev P, TapeClassDev T, const int32_t* __restrict__ mslot,
                                                                       const double* __restrict__ x, double f_tol, SweepOut O) {
    extern __shared__ double tc_cells[];
    const int lane = threadIdx.x;
    const int c = T.wave_cls[blockIdx.x];
    const TapeClassMeta M = T.meta[c];
    const int j = T.wave_first[blockIdx.x] + lane;
    const bool live = j < M.count;                    // (no early return: every lane takes part in block_max_nonneg)
    const int N = M.nnodes, S = M.nslots;
    double* val = tc_cells + lane;                    // cell k of this lane: [k * 64]
    double* adj = val + (size_t)N * kTapeClassWave;
    double* jl = adj + (size_t)N * kTapeClassWave;
    double viol = 0.0;
    if (live) {
        const int32_t r = T.mrow[M.mem0 + j];
        const int32_t gid = mslot[M.mem0 + j];
        const int32_t* col = T.scol + M.col0 + j;     // column of structure entry s: col[s * count]
        const double* cst = T.cst + M.cst0 + j;
        for (int s = 0; s < S; ++s) jl[s * kTapeClassWave] = 0.0;
        double g;
        if (N == 0) {
            g = P.rconst[r];
        } else {
            const int32_t* pop = T.prog_op + M.prog0;
            const int32_t* pa = T.prog_a + M.prog0;
            const int32_t* pb = T.prog_b + M.prog0;
            const double* pcx = T.prog_c + M.prog0;
            for (int i = 0; i < N; ++i) {
                const int op = pop[i];
                const double a = (op >= KTN_OP_ADD) ? val[pa[i] * kTapeClassWave] : 0.0;
                const double b = (op >= KTN_OP_ADD && op <= KTN_OP_DIV) ? val[pb[i] * kTapeClassWave] : 0.0;
                double v;
                if (op == KTN_OP_CONST) v = cst[(int64_t)pa[i] * M.count];
                else if (op == KTN_OP_VAR) v = x[col[(int64_t)pb[i] * M.count]];
                else v = tape_node_forward(op, a, b, [&]() { return pcx[i]; });
                val[i * kTapeClassWave] = v;
                adj[i * kTapeClassWave] = 0.0;
            }
            adj[(N - 1) * kTapeClassWave] = 1.0;
            for (int i = N - 1; i >= 0; --i) {
                const int op = pop[i];
                const double w = adj[i * kTapeClassWave];
                if (op == KTN_OP_CONST) continue;
                if (op == KTN_OP_VAR) { jl[pb[i] * kTapeClassWave] += w; continue; }
                tape_node_reverse(op, w, i, (int)pa[i], [&]() { return (int)pb[i]; }, [&](int k) { return val[k * kTapeClassWave]; },
                                  [&](int k) -> double& { return adj[k * kTapeClassWave]; }, [&]() { return pcx[i]; });
            }
            g = val[(N - 1) * kTapeClassWave] + P.rconst[r];
        }
        // the row tail of k_gj_stats, entries in storage order; each Jacobian entry is stored once, as it is read
        const int64_t beg = P.rowptr[r];
        const RowJacStats st = row_jac_stats(g, 0, S, [&](int s) { const double der = jl[s * kTapeClassWave]; O.jac[beg + s] = der; return der; },
                                             [&](int s) { return x[col[(int64_t)s * M.count]]; });
        row_store(O, r, g, st.bconst, st.mx, st.nf, P.pad_zero[r]);
        viol = row_verdict(O, gid, S, g, P.lb[r], P.ub[r], f_tol, st.nf);
    }
    block_max_nonneg(O.maxviol, viol);
}

}  // namespace ktn
