/* katana_hip.h -- C ABI of the MI355X-native Extended-Cutting-Plane engine.
 *
 * Drop-in boundary for the ONE hot path of lanl-ansi/Katana.jl:
 * the MathProgBase / KatanaSolver plugin surface and the separator API, re-expressed
 * as plain C so that a Julia `ccall` shim, the Python ctypes host
 * mirror (katana.jl_amd/solver.py) or any other FFI can bind it.  No torch types,
 * no C++ types: plain pointers and sizes.  All indices are 0-based.
 *
 * Every entry point names the reference interface it replaces (file:line relative
 * to the reference tree).  Functions return 0 on success and a negative KTN_E_* code
 * on failure (never throw, never abort); ktn_last_error() gives the message.
 * Host buffers are copied at the call (caller keeps ownership); the library owns all
 * device memory until ktn_destroy.  One handle <-> one host thread at a time; every
 * handle owns its HIP stream.  The library REQUIRES a gfx950 device: there is no CPU
 * fallback, ktn_create fails with KTN_E_NODEVICE when none is visible.
 */
#ifndef KATANA_HIP_H
#define KATANA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KTN_ABI_VERSION 1

/* ---- error codes ------------------------------------------------------------ */
#define KTN_OK            0
#define KTN_E_INVALID    -1   /* bad argument / call order                          */
#define KTN_E_NODEVICE   -2   /* no HIP device (the product has no CPU path)        */
#define KTN_E_HIP        -3   /* a HIP runtime call failed                           */
#define KTN_E_NOMEM      -4
#define KTN_E_UNSUPPORTED -5  /* e.g. unknown tape opcode ("Unsupported feature",
                                 src/nlpeval.jl:28)                                  */
#define KTN_E_CALLBACK   -6   /* the caller's evaluator callback reported a failure  */

/* ---- status vocabulary: MathProgBase.status(m) symbols ------------------------
 * :None src/model.jl:44, :Optimal, :Unbounded :246, LP pass-through e.g. :Infeasible
 * :261-263, :UserLimit :314, :Error :71 */
#define KTN_STATUS_NONE       0
#define KTN_STATUS_OPTIMAL    1
#define KTN_STATUS_UNBOUNDED  2
#define KTN_STATUS_INFEASIBLE 3
#define KTN_STATUS_USERLIMIT  4
#define KTN_STATUS_ERROR      5

#define KTN_MIN 0   /* sense :Min */
#define KTN_MAX 1   /* sense :Max */

/* ---- how a constraint row (or the objective) is evaluated on the device --------
 * Replaces the closures behind MathProgBase.eval_g / eval_jac_g / eval_f /
 * eval_grad_f (call sites src/separators.jl:112-113, src/nlpeval.jl:35-63). */
#define KTN_ROW_SEP  0   /* separable: g_i(x) = sum_e atom_e(x[col_e]) + rconst_i    */
#define KTN_ROW_TAPE 1   /* general: postfix expression tape, reverse-mode AD        */
#define KTN_ROW_HOST 2   /* fallback for evaluators that cannot hand over expressions (no :ExprGraph): values and
                            derivatives come from the caller's own eval_g / eval_jac_g / eval_f / eval_grad_f through
                            the callbacks below, once per sweep; isconstrsat, gencut, round_coefs, _addcut and the LP
                            still run on the device (SURVEY.md section 8b "Evaluator consumed")                     */
#define KTN_ROW_QUAD 3   /* sparse quadratic, declared by the caller (the LP/QP surface, src/solver.jl:46):
                            g_i(x) = rconst_i + sum_e a_e x[c_e] + 1/2 sum_e x[c_e] sum_{k in seg(e)} q_k x[qcol_k]
                            e runs over the row's Jacobian entries [rowptr[i], rowptr[i+1]); a_e = p0[e] (p1 and atom_kind are
                            ignored, as for tape rows); seg(e) = [quad_ptr[e], quad_ptr[e+1]) is row c_e of the SYMMETRIC Q_i,
                            stored in full -- both (r, c) and (c, r).  Symmetry is the caller's contract and is NOT checked:
                            the gradient entry is computed as a_e + s_e with s_e = sum_k q_k x[qcol_k], which is the
                            derivative only of a symmetric Q_i.  Every qcol_k must be a column of the row's own structure.
                            ktn_optimize_blocks evaluates such constraint rows inside its device-side loop (a handle whose
                            OBJECTIVE is KTN_ROW_QUAD keeps the ordinary loop: see there), the supporting-hyperplane
                            root search keeps Kelley's cut on them unless cut_algo = KTN_CUT_SUPPORTING_QUAD; row-sharding
                            them is untested and the Python host mirror refuses it                                     */

/* MathProgBase.eval_g + eval_jac_g (src/separators.jl:112-113) for the KTN_ROW_HOST rows: write g[i] and
 * jac[rowptr[i] .. rowptr[i+1]) (CSR order of ktn_nlp_desc) for every such row i; other entries are ignored.
 * x has num_var entries.  Return 0, or non-zero to make the running ktn_* call fail with KTN_E_CALLBACK. */
typedef int (*ktn_eval_rows_cb)(void* user, const double* x, double* g, double* jac);
/* MathProgBase.eval_f + eval_grad_f (src/nlpeval.jl:35-41) for a KTN_ROW_HOST objective: *f and the dense grad[num_var] */
typedef int (*ktn_eval_obj_cb)(void* user, const double* x, double* f, double* grad);

/* separable atoms, two f64 parameters per Jacobian entry */
#define KTN_ATOM_LIN    0   /* p0 * x                */
#define KTN_ATOM_QUAD   1   /* p0 * (x - p1)^2       */
#define KTN_ATOM_EXP    2   /* p0 * exp(p1 * x)      */
#define KTN_ATOM_NEGLOG 3   /* -p0 * log(x + p1)     */

/* postfix tape opcodes; `arg` is the constant for CONST/POWC and the 0-based
 * variable index (stored as a double) for VAR */
#define KTN_OP_CONST 0
#define KTN_OP_VAR   1
#define KTN_OP_ADD   2
#define KTN_OP_SUB   3
#define KTN_OP_MUL   4
#define KTN_OP_DIV   5
#define KTN_OP_NEG   6
#define KTN_OP_POWC  7   /* x ^ arg, arg constant */
#define KTN_OP_EXP   8
#define KTN_OP_LOG   9
#define KTN_OP_SQRT  10
#define KTN_OP_SIN   11
#define KTN_OP_COS   12

typedef struct ktn_handle_s* ktn_handle;

/* KatanaSolver keyword arguments and defaults, src/solver.jl:34-43 +
 * KatanaModelParams src/Katana.jl:12-19.  `lp_solver` has no counterpart: the LP is
 * solved on the GPU by the built-in first-order method; the lp_* fields tune it. */
typedef struct {
    double  f_tol;          /* 1e-6   feasibility tolerance                         */
    double  cut_coef_rng;   /* 1e9    max coefficient range per cut                 */
    int32_t log_level;      /* 10     print every log_level iterations, 0 = silent  */
    int32_t iter_cap;       /* 10000  iteration cap                                 */
    double  obj_eps;        /* -1.0   objective-delta stop (disabled when < 0)      */
    int32_t vis_data;       /* 0      feature :VisData (src/model.jl:1-4,29-31)     */
    int32_t device;         /* -1     HIP device ordinal; -1 = current device       */
    /* GPU LP (restarted reflected Halpern PDHG) */
    int32_t lp_max_iter;    /* 10000000 PDHG iterations per LP solve                */
    int32_t lp_check_every; /* 64      iterations between KKT checks                */
    int32_t lp_ruiz_iters;  /* 8   Ruiz (max-norm) passes before the Pock-Chambolle pass */
    double  lp_tol_scale;   /* 0.1     LP row tolerance = lp_tol_scale * max viol.  */
    double  lp_tol_floor;   /* 0.3     ... floored at lp_tol_floor * f_tol          */
    double  lp_tol_cap;     /* 10      ... capped                                   */
    double  lp_gap_floor;   /* 1e-7    relative duality-gap tolerance floor         */
    double  lp_gap_cap;     /* 1e-2                                                 */
    int32_t lp_dual_inherit;/* 1       new cut of NL row i inherits the dual of its
                                       previous cut (warm start)                    */
    int32_t profile;        /* 0       per-launch hipEvent timing of the hot kernels */
    /* cut-pool management (the reference never removes cuts, src/model.jl:215) */
    int32_t purge_age;      /* 2       drop a cut that had no multiplier and was slack at x* in this many
                                       consecutive LP solves; 0 = keep every cut like the reference      */
    double  purge_margin;   /* 1e-3    ... slack by more than purge_margin * max(1, |row bound|)          */
    double  purge_min_frac; /* 0.05    compact only when at least this fraction of the LP rows goes      */
    int64_t purge_min_rows; /* 2000    ... and only once the pool holds this many cuts: on small smooth
                                       problems (optimum on a curved face, e.g. test/2d.jl 107_01) dropping
                                       idle cuts makes Kelley's method cycle, so small pools are never purged */
    /* exact small-LP kernel (LPs of at most 32 columns; csrc/dense_lp.hpp) */
    int32_t lp_dense_after; /* 5000    when the first-order LP has not converged after this many iterations the
                                       LP is solved exactly by a dual active-set kernel (what the reference's
                                       simplex does on its small test models); 0 = never, < 0 = always exact */
    /* deepest-cut selection (the north star's "select deepest cuts"; the reference cuts every violated row, src/model.jl:272-283) */
    double  cut_cap_factor; /* 1.0     when more than max(cut_cap_factor * num_var, cut_cap_min) NL rows are violated, only that
                                       many of the deepest (largest g - ub / lb - g) get a cut in this iteration; the stop
                                       rule still needs EVERY row within f_tol.  0 = cut every violated row            */
    int64_t cut_cap_min;    /* 10000                                                                                    */
    double  lp_stag_factor; /* 300     primal-stagnation exit of the LP: rows feasible, primal objective flat over two checks,
                                       gap within lp_stag_factor * tolerance (the dual of a degenerate LP crawls long after
                                       the primal has converged), and a row violation that has stalled below 2x the row
                                       tolerance with everything else converged is accepted; 0 = only the full criteria      */
    int32_t lp_ruiz_warm;   /* 0       > 0: reuse the Ruiz equilibration of the previous LP solve for all but the appended rows and run
                                       only this many passes (measured on cfg3: the different scaling costs 1.8x the PDHG
                                       iterations, so the default stays lp_ruiz_iters passes from scratch)                    */
    int64_t lp_tiled_nnz;   /* 4000000 LPs with at least this many non-zeros run their SpMVs from tiled copies of the matrix
                                       (input vector staged through LDS in 64 KB blocks); 0 = never     */
    int32_t lp_near_check;  /* 7       once a check finds row violation, gap and dual residual within 4x their tolerances the next
                                       check comes after this many iterations instead of lp_check_every (a solve otherwise ends
                                       on average half a chunk after it converged: -17 % PDHG iterations on cfg3); 0 = off      */
    double  dedupe_eps;     /* 1e-6    at every purge pass, cuts of an NL row that agree with the row's newest cut within this relative
                                       tolerance (coefficients and bound, normalised by the largest coefficient) are dropped and
                                       their multipliers moved to the newest cut (the reference's TODO, src/model.jl:215); 0 = off */
    /* terminal refinement of small problems: once every NL row is within f_tol (the reference's stop rule, src/model.jl:257,273)
       the loop keeps cutting rows that are beyond polish_factor * f_tol, with the LP solved to the matching tolerance.  The
       reference's exact simplex vertices end Kelley's method far below f_tol on its small test models (its suite asserts the
       objective to 1e-6, test/3d.jl:124 to 1e-7); a first-order LP solution ends AT f_tol.  The point returned always
       satisfies the reference's rule; these passes are not counted in numiters (stat "polish_iters").                       */
    double  polish_factor;  /* 1e-3    0 or >= 1: off                                                                            */
    int32_t polish_max_var; /* 32      only for problems with at most this many LP columns (where the exact LP kernel applies) */
    int32_t polish_max_iter;/* 30      at most this many refinement passes                                                     */
    /* nonlinear objective (EpigraphNLPEvaluator, src/nlpeval.jl:42-63): every epigraph cut is dense and, close to the optimum, nearly
       parallel to every other one.  The first-order LP works on the exactly equivalent problem in which the epigraph variable
       is measured from the NEWEST cut, t = s + grad f(x_k)'x + b_k: the cuts' common part moves into the cost vector and the rows
       keep only their differences (csrc/kernels.hpp "epigraph reference shift").  The LP that getKatanaCuts exports is unchanged. */
    int32_t epi_shift;      /* 1       0 = solve the LP in the reference's own form                                              */
    /* objective certificate (problems with more than polish_max_var LP columns): at the point that meets the stop rule the engine
       evaluates  sum_i lambda_i (signed residual of NL row i) -- the convexity bound on  f* - objective  with the LP's duals as
       multipliers -- and keeps cutting below f_tol (at most polish_max_iter passes, not counted in numiters) while it exceeds
       obj_cert_tol * max(1, |objective|).  The reference's tests accept an objective within 1e-6 (test/runtests.jl:16-17); its exact
       simplex vertices end Kelley's method far below f_tol, a first-order LP ends AT f_tol times the multipliers.              */
    double  obj_cert_tol;   /* 1e-6    (refines while the sum exceeds half of it)  0 = stop at the reference's rule alone          */
    /* exact mid-size LP solver (csrc/mid_lp.hpp): LPs of 33 .. lp_mid_max_var columns are handed to a dual active-set method with
       the basis inverse in device memory when the first-order method stalls (same hand-over rule as lp_dense_after: the LPs of
       a cutting-plane run on a smooth-face optimum -- the reference's own regime, README.md:5 -- have many nearly parallel cuts
       active at once, which the reference's warm-started simplex re-solves in a handful of pivots, src/model.jl:259)            */
    int32_t lp_mid_max_var; /* 512     largest LP (columns) handed over; at most 4096 (n x n doubles of basis inverse); 0 = never.
                                       A pivot costs O(n^2) and a Kelley re-solve hundreds of pivots (the LP vertex jumps), so
                                       beyond a few hundred columns the hand-over stops paying (DESIGN.md section 5
                                       "Smooth-face optima")                                                                    */
    /* cut generator (the reference's KatanaFirstOrderSeparator(algo) slot, src/separators.jl:73-76): KTN_CUT_KELLEY cuts every
       violated row at the LP point x* (linear_oa_cut, src/algorithms.jl:3-18); KTN_CUT_SUPPORTING searches, row by row, the
       segment from an interior point x_int to x* for the point where the row reaches its bound and cuts there (supporting
       hyperplanes).  x_int is the caller's (ktn_set_interior_point) or found once per loaded problem
       by the engine on the auxiliary min-max problem.  Not with ktn_optimize_blocks (ktn_optimize_blocks_ex with KTN_BLOCKS_SUPPORTING
       runs it inside the device-side loop), a row-sharded handle or a cut exchange. */
    int32_t cut_algo;          /* 0 (KTN_CUT_KELLEY), 1 (KTN_CUT_SUPPORTING) or 2 (KTN_CUT_SUPPORTING_QUAD)                      */
    int32_t esh_root_iters;    /* 20    Newton / bisection steps of a row's root search                                    */
    double  esh_root_tol;      /* 0.1   the search stops once 0 <= phi <= esh_root_tol * f_tol                            */
    int32_t esh_interior_iters;/* 50    rounds of the auxiliary problem that finds x_int                                   */
} ktn_params;

#define KTN_CUT_KELLEY     0   /* tangent at x* (the reference's linear_oa_cut)          */
#define KTN_CUT_SUPPORTING 1   /* tangent at the boundary point between x_int and x*     */
#define KTN_CUT_SUPPORTING_QUAD 2   /* KTN_CUT_SUPPORTING with the declared-quadratic rows (KTN_ROW_QUAD) taking part: their boundary
                                       point has a closed form (k_esh_quad); LPs of at most 32 columns go to the
                                       exact small-LP kernel first; refused where 1 is refused */

/* NL-row blocks over several GPUs with a replicated LP: the exchange step of one cutting-plane round.
 * what = 0: the handle has just swept ITS block of NL rows; its new LP rows are the rows from `first_new_row` on.  The callback
 *           moves every rank's new rows into every rank's LP in rank order (ktn_lp_pack_rows_dev -> all-gather ->
 *           ktn_lp_truncate(first_new_row) -> ktn_lp_append_packed_dev per rank) and returns in scalars[0] the number of rows
 *           appended in total and in scalars[1..n) the MAXIMUM over the ranks of what it found there (largest violation, status
 *           flags, two values the loop's decisions are taken from);
 * what = 1: scalars[0..n) are replaced by their SUM over the ranks (the shares of the objective certificate).
 * Return 0, or non-zero to make the running ktn_* call fail with KTN_E_CALLBACK.  The callback may call ktn_lp_* on the handle. */
typedef int (*ktn_exchange_cb)(void* user, int32_t what, int64_t first_new_row, double* scalars, int32_t nscalars);

/* The device-evaluable statement of the NLP: replaces the
 * MathProgBase.AbstractNLPEvaluator `d` handed to loadproblem! (src/model.jl:86).
 * Jacobian structure is CSR over the num_constr constraints (what initialize! builds
 * from jac_structure, src/separators.jl:92-104). */
typedef struct {
    int64_t num_var;
    int64_t num_constr;
    /* Jacobian structure */
    const int64_t* rowptr;      /* [num_constr+1]                                    */
    const int32_t* col;         /* [nnz]                                             */
    /* per row */
    const uint8_t* row_kind;    /* [num_constr] KTN_ROW_*                            */
    const uint8_t* row_linear;  /* [num_constr] isconstrlinear(d,i), src/model.jl:116 */
    const double*  rconst;      /* [num_constr] constant of separable rows           */
    /* separable atoms, per Jacobian entry (unused entries of tape rows ignored)     */
    const uint8_t* atom_kind;   /* [nnz] KTN_ATOM_*                                  */
    const double*  p0;          /* [nnz]                                             */
    const double*  p1;          /* [nnz]                                             */
    /* tapes: row i owns ops [tape_ptr[i], tape_ptr[i+1]) (empty for separable rows) */
    const int64_t* tape_ptr;    /* [num_constr+1] or NULL when there are no tapes    */
    const int32_t* tape_op;
    const double*  tape_arg;
    /* objective f(x): isobjlinear src/model.jl:125; same two forms                  */
    int32_t obj_linear;
    int32_t obj_kind;           /* KTN_ROW_SEP, KTN_ROW_TAPE, KTN_ROW_HOST or KTN_ROW_QUAD */
    int64_t obj_nnz;            /* separable objective entries                       */
    const int32_t* obj_col;
    const uint8_t* obj_atom_kind;
    const double*  obj_p0;
    const double*  obj_p1;
    double         obj_const;
    int64_t        obj_tape_len;
    const int32_t* obj_tape_op;
    const double*  obj_tape_arg;
    /* sparse-quadratic rows (KTN_ROW_QUAD); all NULL / zero when there are none, so a zero-initialised description of a
     * caller that does not know these fields keeps its meaning.  (They follow the tape fields; the callback triple below
     * stays the last three members, which the bindings rely on.) */
    const int64_t* quad_ptr;    /* [nnz+1] over ALL Jacobian entries, or NULL when there are no KTN_ROW_QUAD rows (the
                                   tape_ptr convention); the segments of the entries of other rows must be empty        */
    const int32_t* quad_col;    /* [qnnz] column of the second factor (0-based, a column of the row's structure)       */
    const double*  quad_val;    /* [qnnz] q_k                                                                          */
    /* objective with obj_kind = KTN_ROW_QUAD: obj_col / obj_p0 are the structure and the linear part a, obj_const the
     * constant, obj_quad_ptr [obj_nnz+1] the segments (NULL: no quadratic part) */
    const int64_t* obj_quad_ptr;
    const int32_t* obj_quad_col;
    const double*  obj_quad_val;
    /* host-evaluator fallback (KTN_ROW_HOST rows / objective); NULL when unused.  Called on the thread that is
     * inside ktn_loadproblem / ktn_optimize / ktn_ecp_step / ktn_sep_precompute / ktn_sep_sweep.            */
    ktn_eval_rows_cb eval_rows;
    ktn_eval_obj_cb  eval_obj;
    void*            eval_user;
} ktn_nlp_desc;

/* ---- plugin surface -------------------------------------------------------------- */

/* defaults of KatanaSolver(...) src/solver.jl:34-43 */
void ktn_default_params(ktn_params* p);

/* KatanaSolver(lp_solver; kwargs) + MathProgBase.NonlinearModel(s)
 * (src/solver.jl:34-43, src/model.jl:41-65) */
/* (on failure no handle exists, so ktn_last_error cannot be asked: the message goes to stderr, the code is returned) */
int ktn_create(const ktn_params* p, ktn_handle* out);
void ktn_destroy(ktn_handle h);
const char* ktn_last_error(ktn_handle h);
int ktn_abi_version(void);
/* sizeof(ktn_params) / sizeof(ktn_nlp_desc) as compiled into the library: a binding checks its own struct mirrors
 * against these before the first call (a layout mismatch would otherwise corrupt memory silently) */
int64_t ktn_sizeof_params(void);
int64_t ktn_sizeof_nlp_desc(void);

/* MathProgBase.loadproblem!(m, num_var, num_constr, l_var, u_var, l_constr, u_constr,
 * sense, d)  src/model.jl:81-173 */
int ktn_loadproblem(ktn_handle h, int64_t num_var, int64_t num_constr,
                    const double* l_var, const double* u_var,
                    const double* l_constr, const double* u_constr,
                    int32_t sense, const ktn_nlp_desc* d);

/* MathProgBase.optimize!(m)  src/model.jl:219-319; returns the status code (>= 0)
 * or a negative error */
int ktn_optimize(ktn_handle h);

/* one pass of the hot loop src/model.jl:258-308 (LP re-solve -> sweep -> cuts);
 * *done = 1 when the loop condition of :257 ends.  ktn_optimize == presolve + steps. */
int ktn_optimize_begin(ktn_handle h);           /* src/model.jl:227-256 (presolve)   */
int ktn_ecp_step(ktn_handle h, int32_t* done);
int ktn_optimize_end(ktn_handle h);             /* src/model.jl:311-318              */
/* forget all cuts and iterates: back to the state right after ktn_loadproblem */
int ktn_reset(ktn_handle h);

/* ---- re-solve after a change of variable bounds or of a linear cost, from the kept cut pool (no
 * counterpart in the reference, whose model is loaded once).  Every row of the pool is a tangent of a convex function or a
 * linear row of the problem and holds whatever the box or the cost is, so both setters keep the rows, their multipliers, the
 * cut lists and ages, x and the LP's scaling, and re-open the run state as ktn_reset does: status :None, ktn_numiters 0, the
 * KKT report and the feasible point answer KTN_E_INVALID until the next solve.  ktn_optimize and ktn_optimize_begin /
 * ktn_ecp_step / ktn_optimize_end then run the ordinary loop from the kept pool; ktn_numcuts goes on counting the pool;
 * ktn_optimize_blocks[_ex] starts from the loaded rows, as always -- unless ktn_optimize_blocks_ex is given KTN_BLOCKS_WARM: both
 * setters keep the arenas, the records and the x of the last device launch, and that flag re-solves every instance from its own
 * cuts (below, at ktn_optimize_blocks_ex).  Both may be called after ktn_loadproblem, solved or not.
 * KTN_E_INVALID on a handle whose status is :Error (ktn_reset or ktn_loadproblem first); KTN_E_UNSUPPORTED on a row-sharded
 * handle and on one with a transport or a cut exchange installed.
 *
 * ktn_set_var_bounds: n == num_var of ktn_loadproblem (the epigraph variable keeps -inf, +inf); l == NULL or u == NULL keeps
 *   that side; a NaN bound is KTN_E_INVALID.  x (ktn_get_solution) is clamped into the new box, stat "warm_clamped_cols" counts
 *   the columns moved.  The engine's own interior point (cut_algo = KTN_CUT_SUPPORTING) is searched again in the new box; the
 *   caller's (ktn_set_interior_point) is kept as given.  Crossed bounds l_j > u_j are accepted: the next ktn_optimize[_begin]
 *   screens every LP row k against the new box once --
 *     amin_k = sum_e (v_e > 0 ? v_e l_c : v_e < 0 ? v_e u_c : 0),  amax_k mirrored (a zero coefficient contributes 0, an infinite
 *     term makes the value -inf / +inf),  S_k = sum_e of the larger finite one of the entry's two absolute terms,
 *     tau_k(b) = lp_tol_floor f_tol + (len_k + 2) 2^-52 (S_k + |b|);   row k proves the box infeasible when
 *     amin_k - hi_k > tau_k(hi_k)  or  lo_k - amax_k > tau_k(lo_k)
 *   -- and a proving row or a crossed column ends the solve with status :Infeasible before any LP is solved.  Stats:
 *   "screen_runs", "screen_infeasible_rows", "screen_first_row" (smallest proving row, or -1), "screen_crossed_cols",
 *   "screen_redundant_rows" (amax_k <= hi_k and amin_k >= lo_k; counted, not removed), "warm_solves".
 * ktn_set_linear_objective: c[n] dense, n == num_var, and the constant c0.  Accepted when the loaded objective was declared
 *   linear and is a KTN_ROW_SEP row of KTN_ATOM_LIN atoms or a KTN_ROW_QUAD row (whose Q is then empty); any other objective is
 *   KTN_E_UNSUPPORTED.  A non-zero (or NaN) c_j on a column outside the objective row's structure is KTN_E_INVALID.  The LP's
 *   cost, the constant and the objective row of the device NLP are rewritten: the KKT report, the objective certificate and
 *   f(x_feas) evaluate the new objective.
 * ktn_lp_row_activity: amin[M], amax[M] (M = ktn_lp_num_rows; m < M is KTN_E_INVALID) of the current rows over the current
 *   bounds, at any time; stats "activity_infeasible_rows", "activity_first_row", "activity_redundant_rows" hold what the screen
 *   would count. */
int ktn_set_var_bounds(ktn_handle h, const double* l, const double* u, int64_t n);
int ktn_set_linear_objective(ktn_handle h, const double* c, int64_t n, double c0);
int ktn_lp_row_activity(ktn_handle h, double* amin, double* amax, int64_t m);

/* ---- re-solve after a change of constraint bounds (DESIGN.md section 14 "Row bounds").  A cut of nonlinear row i taken at a
 * point with tangent constant b is stored as [lb_i - b, ub_i - b]; the tangent of a convex g_i is valid at every level, so the
 * cut for new bounds is the same row with its sides moved by ub_i' - ub_i and lb_i' - lb_i.  ktn_set_row_bounds does that to every
 * cut of the pool in place, along the per-row cut lists, and follows the contract of ktn_set_var_bounds above: coefficients,
 * multipliers, lists, ages, x and the scaling stay, the run state is re-opened, the same handles are refused.
 *
 * ktn_set_row_bounds: m == num_constr of ktn_loadproblem; lb == NULL or ub == NULL keeps that side; a NaN bound is
 *   KTN_E_INVALID.  A NONLINEAR row may move its finite bound(s) but not gain or lose a side (the finite side defines its convex
 *   level set): such a request is KTN_E_INVALID and changes nothing.  Linear rows may gain or lose sides freely; their LP rows
 *   are worked out again from the tangent at the origin and equal those of a fresh load bit for bit.  The epigraph row is never
 *   touched.  Each moved side of a cut is one rounded addition hi + (ub' - ub), the difference formed once per row; a side whose
 *   old and new bound are equal (two infinite ones included) is not written, so unchanged bounds leave the pool bit for bit.
 *   The engine's own interior point is searched again; the caller's is kept as given.  lb_i' > ub_i' is accepted and counted
 *   (stat "screen_crossed_rows"): the next solve ends :Infeasible before any LP, as for crossed columns, and otherwise starts
 *   with the screen of ktn_set_var_bounds.  With a device launch of ktn_optimize_blocks[_ex] standing, the resident arenas get
 *   the same treatment before the call returns (linear rows copied, cut rows shifted), so KTN_BLOCKS_WARM continues from them.
 *   Stats: "rebase_rows" (cut rows moved, pool and arenas), "rebase_kernel_s" (the kernels' own time), "screen_crossed_rows".
 * ktn_lp_get_row_owners: owner[M] (M = ktn_lp_num_rows; m < M is KTN_E_INVALID): for every LP row the caller's constraint row
 *   whose cut list holds it, num_constr for a cut of the epigraph row, -1 for a row in no list (linear rows, engine-made rows,
 *   rows appended without an id).  KTN_E_UNSUPPORTED while the lists are not tracked (rows appended from the host without
 *   global lists) or are global (ktn_lp_enable_global_lists). */
int ktn_set_row_bounds(ktn_handle h, const double* lb, const double* ub, int64_t m);
int ktn_lp_get_row_owners(ktn_handle h, int64_t* owner, int64_t m);

/* MathProgBase.status / getobjval / getsolution / getsolvetime  src/model.jl:337-343;
 * numiters / numcuts src/model.jl:326,333; setwarmstart! (a no-op) :335 */
int     ktn_get_status(ktn_handle h);
double  ktn_get_objval(ktn_handle h);
int64_t ktn_get_num_var(ktn_handle h);     /* incl. the epigraph variable, model.jl:138 */
int     ktn_get_solution(ktn_handle h, double* x_out, int64_t n);
double  ktn_get_solvetime(ktn_handle h);
int64_t ktn_numiters(ktn_handle h);
int64_t ktn_numcuts(ktn_handle h);
int     ktn_setwarmstart(ktn_handle h, const double* x, int64_t n);

/* ---- Lagrange multipliers, reduced costs and a dual bound of the solved NLP (MathProgBase.getconstrduals / getreducedcosts /
 * getobjbound; no counterpart in the reference, which returns none) ------
 * Problem, sense Min:  min f(x)  s.t.  lb_i <= g_i(x) <= ub_i (i < num_constr),  l <= x <= u, x the caller's num_var variables
 * (the epigraph variable and row are internal and never reported).  x* = what ktn_get_solution returns.
 *
 *   d[num_constr]  constraint duals in the caller's row order, signed like ktn_lp_get_duals: d_i > 0 the lower side is active,
 *                  d_i < 0 the upper side (d_i = d f* / d bound_i).  A linear row of the loaded LP: the multiplier of its own LP
 *                  row.  An NL row: the sum of the multipliers of the cuts now in its list, newest to oldest; 0 for an empty list.
 *                  The LP multipliers are those ktn_lp_get_duals returns (unscaled; after an exact mid-size solve: of the true cost).
 *   z[num_var]     reduced costs = the gradient of the Lagrangian at x*:  z = grad f(x*) - J(x*)' d,  J the Jacobian of all
 *                  num_constr rows at x*, grad f the objective row's own Jacobian entries with weight exactly 1.  At a KKT point
 *                  z_j >= 0 on a lower bound, <= 0 on an upper bound, 0 in between.
 *   bound          with d+ = max(d, 0), d- = max(-d, 0), likewise z:
 *                    LB = f(x*) - sum_i d+_i (g_i(x*) - lb_i) + sum_i d-_i (g_i(x*) - ub_i) - sum_j [z+_j (x*_j - l_j) + z-_j (u_j - x*_j)]
 *                  For a convex problem LB <= f* for ANY d (the Lagrangian is convex in x, bounded below by its tangent at x*, and
 *                  the tangent is minimised over the box).  An infinite bound under a non-zero multiplier of that side makes
 *                  LB = -inf; 0 * inf counts as 0.  gap = f(x*) - LB.
 *   sense Max      the three are those of the mirrored Min problem, mirrored back: d and z negated (d stays d f* / d bound), the
 *                  bound is an upper bound, gap = bound - f(x*).
 *
 * The three getters compute once (on the first call) and cache; a solve that is followed by no getter launches nothing for them.
 * The cached values are dropped -- the next getter computes again -- by ktn_loadproblem, ktn_reset, any LP solve and any change
 * of the LP rows, whoever makes it.  Whether the getters ANSWER is a separate rule: KTN_E_INVALID (with a message) while no LP
 * solve has run since the problem was loaded or reset, or since the CALLER last changed the rows through ktn_lp_append_rows[_nl],
 * ktn_lp_append_packed_dev, ktn_lp_truncate or ktn_lp_purge (a call of these counts whether or not it changed a row).  Rows
 * that the engine itself appends or purges -- inside ktn_optimize*, ktn_ecp_step, ktn_sep_sweep, ktn_sweep_lp_point -- do NOT make
 * the getters refuse: a purge compacts the multipliers with the rows and relinks the lists, a new cut starts at 0 or takes over
 * the multiplier of its list's previous cut, so every NL row's sum is still that of the last LP solve (the answer is then
 * recomputed from that state, not served from the cache).  KTN_E_UNSUPPORTED on a row-sharded handle
 * (ktn_dist_init_*) or one with a cut exchange: it owns only a part of the lists.  One handle with ktn_lp_enable_global_lists is
 * served from those lists.  After ktn_optimize_blocks[_ex] that ended in the device loop the multipliers and lists are the
 * arenas'; after its fallback to the ordinary loop the ordinary state's.  m >= num_constr, n >= num_var (buffers too small:
 * KTN_E_INVALID).  KTN_ROW_HOST rows: the caller's callback runs once per computation.
 * Stats: "kkt_evals" times the kernels ran; "kkt_epi_dual" the aggregated multiplier of the epigraph row (a diagnostic: +-1 in an
 * exact LP, NaN for a linear objective). */
int ktn_get_constr_duals(ktn_handle h, double* d_out, int64_t m);
int ktn_get_reduced_costs(ktn_handle h, double* z_out, int64_t n);
int ktn_get_dual_bound(ktn_handle h, double* bound, double* gap);

/* ---- a feasible point and the primal bound it certifies --------------
 * ktn_get_solution returns the LP optimum x*, an OUTER point: it may violate every active nonlinear row by up to f_tol.
 * ktn_get_feasible_point returns x_feas on the segment from a reference point x_in to x* with every taking-part row satisfied, so
 * that for a convex problem   bound of ktn_get_dual_bound <= f* <= f(x_feas)   (Min; mirrored for Max).
 *   x_in           the caller's point (ktn_set_interior_point, accepted under every cut_algo); under KTN_CUT_SUPPORTING[_QUAD]
 *                  without one, the engine's own (found first if that has not happened yet, as by ktn_get_interior_point).  Under
 *                  KTN_CUT_KELLEY without a caller's point there is none: found = 0.  x_in must lie in [l, u] and satisfy every
 *                  taking-part row (found = -1 otherwise); the engine's own point, which meets the bounds only to its auxiliary
 *                  LP's tolerance, is clamped into [l, u] first.
 *   taking part    every row i < num_constr that is not declared linear, of kind SEP, TAPE or QUAD, with exactly one finite side
 *                  (sigma_i = +1: g_i <= ub_i, -1: g_i >= lb_i; b_i that bound), under every cut_algo.  Not the epigraph row, not
 *                  a free nonlinear row.  phi_i(lambda) = sigma_i (g_i(x_in + lambda (x* - x_in)) - b_i).
 *   lambda_i       1 where phi_i(1) <= 0 and is finite; otherwise a point of [0, 1) with -tau <= phi_i(lambda_i) <= 0,
 *                  tau = esh_root_tol * f_tol, found by bracketed Newton on phi + tau / 2 from lambda = 1 (bisection when a step
 *                  leaves the bracket or the derivative is not positive and finite), esh_root_iters passes at most.  A row that
 *                  runs out of passes takes the bracket's lower end -- the last point with a finite phi <= 0, 0 to begin with -- and
 *                  is counted in info[6]: validity never depends on convergence.
 *   lambda*        min_i lambda_i; the blocking row is the smallest row index attaining a minimum below 1.
 *   x_feas         clamp(x_in_j + lambda* (x*_j - x_in_j), l_j, u_j)  (lambda* = 1: x*_j itself)
 *   verification   every row is evaluated at x_feas; found = 1 only if every taking-part row has sigma (g - b) <= 0 there.  If one
 *                  has not (rounding, the clamp), back-off k = 1 .. 8 takes lambda* (1 - 2^(6 k - 48)) and verifies again -- the
 *                  eighth is x_in itself --; found = -2 after eight failures.  Linear rows and bounds are not searched: info[4]
 *                  reports the largest violation of a linear row at x_feas, which convexity bounds by those at x_in and x*.
 * info[KTN_FEAS_INFO_LEN]:
 *   [0] found      1 found; 0 no reference point; -1 the reference point is outside [l, u], violates a taking-part row, or a row is
 *                  not finite there; -2 verification failed
 *   [1] lambda*    (the one x_feas was formed with, back-offs included)
 *   [2] f(x_feas)  the objective row's own value at x_feas, in the caller's sense: f* <= f(x_feas) for Min, >= for Max
 *   [3] max_i sigma_i (g_i - b_i) at x_feas over the taking-part rows: <= 0; -inf when there are none  (found = -1: at x_in)
 *   [4] the largest violation of a linear row at x_feas, >= 0                                          (found = -1: at x_in)
 *   [5] the blocking row, -1 if none; found = -1: the first offending row (-1: the point is outside [l, u])
 *   [6] rows that ended unconverged        [7] back-offs
 * When found != 1, x_out is NaN.  ktn_get_feasible_row_lambdas: lambda_i by caller row (1 for a row that does not take part).
 * Computed on the first call and cached; dropped by ktn_loadproblem, ktn_reset, any LP solve, any change of the LP rows and
 * ktn_set_interior_point.  A solve that is followed by no getter launches nothing for this (stat "feas_evals" stays 0), and what
 * ktn_sep_*, the objective certificate, the KKT report and a following ktn_ecp_step read is left bit for bit.
 * KTN_E_UNSUPPORTED (with a message): KTN_ROW_HOST rows or objective, a nonlinear row with two finite sides, a row-sharded handle
 * or one with a cut exchange.  KTN_E_INVALID: while ktn_get_dual_bound would refuse (no LP solve since load or reset), n < num_var,
 * cap < KTN_FEAS_INFO_LEN.  After ktn_optimize_blocks[_ex] x* is the fused problem's point, as for ktn_get_dual_bound.
 * Stats: "feas_evals" times the kernels ran; "feas_passes" evaluation passes of the last search; "feas_group" lanes per row. */
#define KTN_FEAS_INFO_LEN 8
int ktn_get_feasible_point(ktn_handle h, double* x_out, int64_t n, double* info, int64_t cap);
int ktn_get_feasible_row_lambdas(ktn_handle h, double* lam_out, int64_t m);
/* The same per instance of a fused batch (ktn_set_blocks; rows and columns grouped by instance, refused otherwise as by
 * ktn_blocks_get_dual_bounds): *count = KTN_FEAS_INFO_LEN * n_blocks; info[KTN_FEAS_INFO_LEN b ..] is instance b's record, with
 * lambda_b = the minimum over the instance's own rows (1 for an instance without nonlinear rows), [2] the instance's share c_b'x_b of
 * the fused objective as ktn_blocks_get_dual_bounds forms it, [5] a row index of the fused problem; x_out [num_var] holds every
 * instance's segment of x_feas = clamp(x_in + lambda_b (x* - x_in), l, u), NaN for an instance whose found != 1.  An instance whose
 * reference point fails gets its own code and does not affect the others; back-offs are per instance.  The reference points are the
 * segments of the fused problem's point (ktn_set_interior_point), x* is the fused problem's point also after ktn_optimize_blocks[_ex].
 * x_out == NULL and info == NULL only asks for the count.  One workgroup per instance for lambda_b and for the verification. */
int ktn_blocks_get_feasible_points(ktn_handle h, double* x_out, int64_t n, double* info, int64_t cap, int64_t* count);

/* ---- supporting-hyperplane cuts (cut_algo = KTN_CUT_SUPPORTING or KTN_CUT_SUPPORTING_QUAD) ------
 * The interior point x_int [num_var, without the epigraph variable]: ktn_set_interior_point hands one over (NULL clears
 * it, and the engine then looks for one itself when it next needs it); ktn_loadproblem forgets it, ktn_reset keeps it.
 * ktn_get_interior_point writes the point in use and *found = 1, or *found = 0 when there is none (the engine then
 * cuts as in Kelley's method).  With supporting hyperplanes on it first finds or evaluates the point if that has
 * not happened yet.
 * Stats: "esh_rows" "esh_fallback_rows" "esh_newton_steps" "esh_root_time_s" "esh_interior_found" "esh_interior_rounds"
 *        "esh_interior_s" "esh_interior_depth" "esh_interior_time_s"
 *        "esh_quad_rows" KTN_ROW_QUAD rows cut at their boundary point (KTN_CUT_SUPPORTING_QUAD; cumulative, counted in "esh_rows" too) */
int ktn_set_interior_point(ktn_handle h, const double* x, int64_t n);
int ktn_get_interior_point(ktn_handle h, double* x_out, int64_t n, int32_t* found);
/* lambda of each cut the last sweep appended, in the order of ktn_last_sweep_slots: the cut of that row was taken at
 * x_int + lambda (x* - x_int); 1 = Kelley's cut at x* itself (every cut when cut_algo = KTN_CUT_KELLEY). */
int ktn_last_sweep_lambdas(ktn_handle h, double* lam, int64_t cap, int64_t* count);

/* ---- separator API (batched form of src/separators.jl:23-53,111-120) --------------
 * precompute!(sep, xstar): evaluate g and the sparse Jacobian of ALL rows of the
 * loaded (epigraph-lifted) problem at xstar [num_var incl. aux] on the device. */
int ktn_sep_precompute(ktn_handle h, const double* xstar, int64_t n);
int64_t ktn_sep_num_constr(ktn_handle h);  /* incl. the epigraph row                  */
int64_t ktn_sep_jac_nnz(ktn_handle h);
int ktn_sep_get_g(ktn_handle h, double* g_out, int64_t m);
int ktn_sep_get_jac(ktn_handle h, double* jac_out, int64_t nnz);
int ktn_sep_get_structure(ktn_handle h, int64_t* rowptr_out, int32_t* col_out);
/* isconstrsat(sep, i, lb, ub, f_tol) src/separators.jl:120 -> 1/0 */
int ktn_sep_isconstrsat(ktn_handle h, int64_t i, double lb, double ub, double f_tol);
/* gencut(sep, xstar, bounds, i) -> AffExpr  src/separators.jl:118 +
 * linear_oa_cut src/algorithms.jl:3-18; *nnz in: capacity, out: entries written */
int ktn_sep_gencut(ktn_handle h, int64_t i, int32_t* cols, double* coefs, int64_t* nnz,
                   double* constant);
/* {isconstrsat, gencut, round_coefs, _addcut} over all NL rows at the point of the last
 * precompute (src/model.jl:272-283, 200-207, 68-79): appends the cuts to the LP.
 * Outputs: number of violated rows, largest violation. */
int ktn_sep_sweep(ktn_handle h, double f_tol, int64_t* nviol, double* maxviol);

/* ---- LP introspection: getKatanaCuts / getKatanaSols, src/util.jl:16-36 ------------ */
int64_t ktn_lp_num_rows(ktn_handle h);
int64_t ktn_lp_nnz(ktn_handle h);
int ktn_lp_get_rows(ktn_handle h, int64_t* rowptr, int32_t* col, double* val,
                    double* lo, double* hi);
int ktn_lp_get_objective(ktn_handle h, double* c_out, int64_t n, double* c0);
/* Row multipliers of the last LP solve (> 0: the row's lower side, < 0: its upper side).  After a first-order solve or an exact
 * solve of at most 32 columns: the solve's own multipliers.  After an exact mid-size solve (33 .. lp_mid_max_var columns) that ended
 * optimal, for as long as no row is appended, purged or truncated and no other solve runs: the multipliers of the LP's own cost at
 * the vertex returned, computed on this call; the cutting-plane loop itself keeps those of the solver's perturbed cost, which
 * differ by the perturbation (1e-9 (1 + |c_j|) per column) and are what this call returns in every other state. */
int ktn_lp_get_duals(ktn_handle h, double* y_out, int64_t m);
/* solve the current LP to the given tolerances (tests / tools):
 * row_tol = max unscaled row violation, gap_tol = relative duality gap */
int ktn_lp_solve(ktn_handle h, double row_tol, double gap_tol, int32_t* lp_status,
                 int64_t* pdhg_iters);
/* exactly `iters` PDHG iterations from (x0, y0) with fixed eta/omega, no restart, no
 * rescaling (dr = dc = 1): kernel-level parity hook for tests */
int ktn_lp_pdhg_raw(ktn_handle h, const double* x0, const double* y0, double eta,
                    double omega, int64_t iters, double* x_out, double* y_out);
/* a scripted run from a prescribed state: kernel-level parity hook for tests.  x, y and the anchors x0, y0 are given
 * in the stored LP's space and scaled as a solve scales its start; `k` is the Halpern counter of the first op; the ops
 * run through the launch paths of the solve itself (lane groups, trips, packed / tiled forms and their KTN_*
 * development switches included).  Outputs (each may be NULL) are in the SCALED space: x, y, anchors, the point
 * (xt, yt) of the last check, q[0..15] the row sums and q[16..31] the column sums of the last check, xnext / ynext
 * and *spec = 1 when that check left the next iterate there, and the scaling dr (rows), dc (columns). */
#define KTN_LPOP_STEP 0      /* one plain iteration (x-step, y-step, Halpern update) */
#define KTN_LPOP_CHECK 1     /* a check iteration: (xt, yt) and the 32 sums */
#define KTN_LPOP_ADVANCE 2   /* the Halpern update after a check */
#define KTN_LPOP_RESTART 3   /* restart from the point of the last check (k = 0 afterwards) */
#define KTN_LPS_IDENTITY 1   /* flags: dr = dc = 1 instead of the solve's equilibration */
#define KTN_LPS_PACKED 2     /*        plain steps read the packed per-row / per-column records */
#define KTN_LPS_NO_SPEC 4    /*        checks do not precompute the next iterate */
int ktn_lp_script(ktn_handle h, const double* x, const double* y, const double* x0, const double* y0,
                  double eta, double omega, int64_t k, int32_t flags, const int32_t* ops, int64_t nops,
                  double* x_out, double* y_out, double* x0_out, double* y0_out, double* xt_out,
                  double* yt_out, double* q, double* xnext, double* ynext, int32_t* spec,
                  double* dr, double* dc);
/* the equilibration of the current LP, computed afresh: dr, dc and the factors before the last (sum-norm) pass
 * (dr_r, dc_r; they need lp_ruiz_warm > 0): kernel-level parity hook for tests */
int ktn_lp_scaling(ktn_handle h, double* dr, double* dc, double* dr_r, double* dc_r);
int64_t ktn_num_lp_sols(ktn_handle h);           /* :VisData lp_sols, src/model.jl:267 */
int ktn_get_lp_sol(ktn_handle h, int64_t k, double* x_out, int64_t n);

/* ---- statistics (not in the reference: measurement hooks) ----
 * names: "lp_time_s" "sep_time_s" "pdhg_iters" "lp_solves" "lp_restarts" "sweeps"
 * which form of the separable evaluation the loaded problem takes (written by ktn_loadproblem, read-only):
 *        "sweep_group"          lanes per row G of the row kernels (8, 16, 32, 64)
 *        "sweep_rows_per_group" rows per lane group R of the sweep's row kernel (1, 2, 4); 0 when the sweep is
 *                               column-blocked or batch-blocked
 *        "sweep_blocked"        1 when the sweep is the column-blocked one (long sorted rows)
 *        "sweep_batched"        1 when the sweep is the batch-blocked one (many short rows)
 *        "precompute_multirow"  1 when precompute! runs four rows per lane group
 *        "sep_long_rows"        rows beyond 8 192 entries, evaluated one workgroup per row
 *        "quad_rows" "quad_nnz" KTN_ROW_QUAD rows (the epigraph row of a KTN_ROW_QUAD objective included) and their Q entries
 *        "quad_group"           lanes per Jacobian entry G of k_quad_jac (4 .. 64), from the mean segment length; 0 without such rows
 * which form of the LP kernels the last ktn_lp_script ran (written by it, for tests):
 *        "lp_grp_rows" "lp_grp_cols" lanes per row / column G;   "lp_packed" "lp_packed_trips" packed records on, outputs per group T
 *        "lp_long_rows" "lp_long_cols" rows / columns beyond 2 048 entries;   "lp_tiled" "lp_tiled_check" "lp_tiled_pieces"
 *        "lp_check_spec"        1 when the last check left the next iterate in xnext / ynext;   "lp_check_pinned"
 *        "lp_scale_fused_passes" "lp_scale_split_passes"  equilibration passes in the one-launch / three-kernel form (counters)
 * with params.profile = 1, per hot kernel K in {kx, ky, sweep_eval, tape_eval, quad_eval}:
 *        "K_time_s" "K_launches" "K_bytes"  from the start/stop hipEvents of hipExtLaunchKernelGGL
 *        on the engine's own stream (dispatch begin/end, as rocprofv3 --kernel-trace reports) */
double ktn_get_stat(ktn_handle h, const char* name);

/* ---- multi-GPU building blocks (no reference counterpart) -----
 * The NL rows shard by contiguous blocks: every rank loads the linear rows plus ITS block
 * of NL rows, sweeps it, and the generated cuts are exchanged (RCCL all-gather through
 * torch.distributed in katana.jl_amd/distributed.py) and appended in rank order so that
 * every rank holds the identical LP.  These calls are what that host loop is made of:
 *   ktn_sweep_lp_point   : the loop body of src/model.jl:268-283 at the current LP solution
 *   ktn_lp_get_rows_from : export the rows appended since `first_row` (rowptr rebased to 0)
 *   ktn_lp_truncate      : drop the rows >= nrows again (own cuts are re-appended in rank order).  The cut lists stay valid:
 *                          every list that started in a dropped row now starts at its newest surviving cut (or is empty), so a
 *                          row appended afterwards -- its index is one that was just given up -- links to that cut, never to
 *                          itself; the surviving rows keep their multipliers and ages
 *   ktn_lp_append_rows   : append a CSR block of rows (rowptr 0-based), duals start at 0
 * Use lp_dual_inherit = 0 with truncate/append (row indices of earlier cuts change). */
int ktn_sweep_lp_point(ktn_handle h, double f_tol, int64_t* nviol, double* maxviol);
/* this handle's share of the objective certificate (sum over ITS NL rows of multiplier mass x signed residual at the last sweep's
 * point; the engine's own loop evaluates the same sum over all rows after the stop rule is met, src/model.jl:257 +
 * test/runtests.jl:16-17): the host loop adds the shares of all ranks and clamps at zero.  id_offset = global id of the
 * handle's first NL row (ktn_lp_enable_global_lists), 0 otherwise. */
int ktn_objective_certificate(ktn_handle h, int64_t id_offset, double* sum);
int64_t ktn_lp_nnz_from(ktn_handle h, int64_t first_row);
int ktn_lp_get_rows_from(ktn_handle h, int64_t first_row, int64_t* rowptr, int32_t* col, double* val,
                         double* lo, double* hi);
int ktn_lp_truncate(ktn_handle h, int64_t nrows);
/* Per-NL-row cut lists across ranks: after ktn_lp_enable_global_lists(h, total NL rows of the unsharded problem) rows
 * appended with ktn_lp_append_rows_nl carry the GLOBAL NL-row id of the row they cut (-1: none); the engine then gives them
 * the bookkeeping its own sweep gives local cuts -- the new cut inherits the multiplier of the row's previous cut
 * (lp_dual_inherit), stall consolidation and purging see the lists.  ktn_last_sweep_slots returns, for the cuts the last
 * sweep appended, the local NL slot (0-based position among this handle's NL rows) of each, in row order. */
int ktn_lp_enable_global_lists(ktn_handle h, int64_t nl_total);
int ktn_last_sweep_slots(ktn_handle h, int64_t* slots, int64_t cap, int64_t* count);
int ktn_lp_append_rows_nl(ktn_handle h, int64_t nrows, const int64_t* rowptr, const int32_t* col, const double* val,
                          const double* lo, const double* hi, const int64_t* nl_id);
/* The same exchange without leaving device memory (the north star's "RCCL all-gather of generated cuts over xGMI"): the rows
 * [first_row, M) -- the cuts a sweep just appended -- are written as ONE f64 block
 *     [rowptr[1:] rebased | col | val | lo | hi | global NL-row id = id_offset + local NL slot]      (4 nrows + 2 nnz doubles)
 * into a DEVICE buffer of the caller (dev_out == NULL: size query only), all-gathered by the caller (RCCL), and every rank's
 * block is appended from the device receive buffer by ktn_lp_append_packed_dev, with the bookkeeping of
 * ktn_lp_append_rows_nl.  Both calls return with the engine's stream idle; the caller synchronises its own stream between
 * the all-gather and the appends. */
int ktn_lp_pack_rows_dev(ktn_handle h, int64_t first_row, int64_t id_offset, double* dev_out, int64_t cap,
                         int64_t* nrows, int64_t* nnz);
int ktn_lp_append_packed_dev(ktn_handle h, int64_t nrows, int64_t nnz, const double* dev_in);
/* ONE implementation of the cutting-plane step for the NL-row-block layout (round 4): with an exchange callback installed
 * (after ktn_lp_enable_global_lists; first_nl_id = global id of this handle's first NL row) ktn_ecp_step / ktn_optimize run the
 * engine's own loop -- tolerance schedule, floor rule, purge, refinement by the objective certificate -- and call the callback
 * where the single-GPU loop sweeps: every decision of the loop is taken from what the callback returns, i.e. from the same
 * numbers on every rank.  (Until round 3 a host loop re-stated those rules on top of the building blocks above.)  cb = NULL
 * removes it. */
int ktn_set_cut_exchange(ktn_handle h, ktn_exchange_cb cb, void* user, int64_t first_nl_id);
/* cut-pool purge after an LP solve (what ktn_ecp_step does between the LP and the sweep); deterministic, so ranks that
 * hold identical LPs stay identical */
int ktn_lp_purge(ktn_handle h, int64_t* rows_removed);
int ktn_lp_append_rows(ktn_handle h, int64_t nrows, const int64_t* rowptr, const int32_t* col,
                       const double* val, const double* lo, const double* hi);

/* ---- throughput mode (BASELINE.json configs[4]; the loop being batched is src/model.jl:257-309) ---------------------
 * A batch of independent instances is loaded as ONE block-diagonal problem (variables, rows and the summed linear
 * objective side by side).  ktn_set_blocks(h, nblocks, col_offsets[nblocks + 1]) -- after ktn_loadproblem -- tells the
 * engine which column ranges are the instances: every LP re-solve then runs as one launch with one workgroup per instance
 * (iterates in LDS, __syncthreads() instead of kernel boundaries, restarts and termination decided per instance), while
 * the sweep and the cut bookkeeping keep serving the whole batch at once.  nblocks = 0 switches it off. */
int ktn_set_blocks(ktn_handle h, int64_t nblocks, const int64_t* col_offsets);
/* MathProgBase.optimize! for such a batch with the WHOLE loop of src/model.jl:257-309 of every instance inside its own
 * workgroup (csrc/batch_ecp.hpp): LP scaling, step-size estimate, PDHG with its checks and restarts, the sweep over the
 * instance's NL rows, cut append, column mirror, tolerance schedule and stop rule -- no instance waits for another.  Needs
 * separable, tape or KTN_ROW_QUAD constraint rows (no KTN_ROW_HOST), linear or not, a linear :Min objective, finite variable bounds and the
 * instances' rows grouped instance after instance (instances.fuse_instances, nlp.fuse_problems); `cut_capacity` = room for that many cuts
 * per NL row (<= 0: 12).  One deliberate exception: a handle whose objective row has kind KTN_ROW_QUAD -- even declared linear, as a
 * hand-fused QuadNLP has it -- keeps the ordinary loop; nlp.fuse_problems always emits a KTN_ROW_SEP objective of LIN atoms (a quadratic
 * objective becomes a QUAD constraint row and an epigraph variable per instance there), so nothing that comes through it is affected.
 * Falls back to the ordinary loop when the batch does not qualify or an instance runs out of room or of LP iterations.  Returns the
 * status like ktn_optimize; getters as usual (numiters = the largest per-instance count, numcuts = the sum).  Stats (ktn_get_stat):
 * "ecp_blocks_launches", "ecp_blocks_fallbacks" (cumulative), "ecp_blocks_tape_rows", "ecp_blocks_quad_rows" (tape / QUAD NL rows the
 * last device loop served). */
int ktn_optimize_blocks(ktn_handle h, int32_t cut_capacity);
/* ktn_optimize_blocks with options.  flags = 0 is ktn_optimize_blocks itself.
 *   KTN_BLOCKS_SUPPORTING   cut_algo = KTN_CUT_SUPPORTING / _QUAD runs INSIDE the device-side loop (k_ecp_blocks<1>, csrc/batch_ecp.hpp;
 *       DESIGN.md section 11 "In the device-side loop"): the interior point is found or taken first if that has not happened yet --
 *       ktn_set_interior_point on the fused problem (the concatenation of the instances' points), or the engine's auxiliary problem
 *       on the fused problem --, then every violated separable row that takes part is cut where the segment x_int -> x* leaves it
 *       (the bracketed Newton of csrc/esh.hpp, 16 lanes per row, no launch and no read-back per round) and, under
 *       KTN_CUT_SUPPORTING_QUAD, every such KTN_ROW_QUAD row at its closed-form boundary point (csrc/esh_quad.hpp).  TAPE ROWS KEEP
 *       KELLEY'S CUT in the device loop and count as fallback rows.  With no interior point the launch is Kelley's (k_ecp_blocks<0>).
 *       A batch that falls back runs the ordinary loop with the handle's cut_algo.  Without this flag a handle with cut_algo != 0 is
 *       refused (KTN_E_UNSUPPORTED), as by ktn_optimize_blocks.
 *   KTN_BLOCKS_NO_FALLBACK  return after the device launch: the status is :Optimal only if every instance's is, otherwise the first
 *       other instance's status; ktn_get_solution returns the x the launch wrote; "ecp_blocks_fallbacks" does not count the call; a
 *       batch that does not qualify for the device loop returns KTN_E_UNSUPPORTED.
 *   KTN_BLOCKS_WARM         re-solve the batch from the arenas of the last device launch on the loaded problem (DESIGN.md section 14
 *       "In the device-side loop"): the per-instance LPs with their cuts, multipliers, cut lists and x are still resident, and
 *       after ktn_set_var_bounds / ktn_set_linear_objective every cut is still valid.  Used when a previous device launch stands
 *       (no ktn_reset, ktn_loadproblem, ktn_set_blocks or host fallback since) and cut_capacity is the one it ran with; nothing is
 *       uploaded or resized then.  First k_blocks_rewarm (csrc/batch_warm.hpp, one workgroup per instance) does what
 *       ktn_blocks_rewarm describes, then each instance starts by its state: 1 from its arena, the first LP at the tolerance its
 *       last solve ended at; 2 ends :Infeasible without an LP (0 PDHG iterations), the others are not affected; 0 (the last
 *       record was not :Optimal, or overflowed) from its linear rows, cold.  An instance the screen ends :Infeasible does NOT send
 *       the batch to the ordinary loop, which could not help it: when such instances are the only ones not :Optimal the call
 *       returns the first one's status, as under KTN_BLOCKS_NO_FALLBACK, and "ecp_blocks_fallbacks" does not move.  An instance that
 *       overflows or runs out of LP iterations falls back as always (and the host loop then starts cold, warm state dropped).
 *       Without a usable previous launch the call is the cold launch, bit for bit, and "ecp_blocks_warm_launches" does not move.
 *       A Kelley launch after a supporting one reports lambda = 1 for every row; a supporting launch after a Kelley one has no
 *       lambda for the kept rows and is the cold launch.  ktn_optimize[_begin] (the host loop) drops the warm state too.  Stats: "ecp_blocks_warm_launches" (cumulative); of the last k_blocks_rewarm
 *       "ecp_blocks_warm_instances" (state 1), "ecp_blocks_warm_cold_instances" (state 0), "ecp_blocks_warm_infeasible" (state 2),
 *       "ecp_blocks_warm_dropped_rows", "ecp_blocks_warm_clamped_cols", "ecp_blocks_rewarm_kernel_s" (the kernel's own time).
 * Stats: "esh_rows" "esh_fallback_rows" "esh_newton_steps" "esh_quad_rows" accumulate the instances' counters of a k_ecp_blocks<1>
 * launch; "ecp_blocks_esh_rows" rows moved by the last launch (0 after a Kelley launch).  ktn_last_sweep_lambdas keeps describing
 * the sweeps of the host-driven loop only: the lambdas of a device launch come from ktn_blocks_get_cuts. */
#define KTN_BLOCKS_SUPPORTING  1   /* cut_algo 1 / 2 run inside the device loop (without it: refused, as ktn_optimize_blocks does) */
#define KTN_BLOCKS_NO_FALLBACK 2   /* do not run the ordinary loop when the batch does not qualify or an instance does not end :Optimal */
#define KTN_BLOCKS_WARM        (4) /* start every instance from the arena of the last device launch (cold where there is none) */
int ktn_optimize_blocks_ex(ktn_handle h, int32_t cut_capacity, int32_t flags);
/* The records of the last device launch on the loaded problem, [n_blocks x 8] doubles, instance after instance:
 *   0 status (KTN_STATUS_*)   1 cutting-plane iterations   2 objective (without the loaded problem's constant)
 *   3 cuts (numcuts: the instance's linear rows counted, as the reference does)   4 PDHG iterations
 *   5 largest violation of the last sweep   6 LP rows at the end (linear rows + cut rows)   7 arena overflow (0 / 1)
 * Size convention of ktn_last_sweep_lambdas: *count is always set; with out == NULL nothing else happens, otherwise cap >= *count.
 * KTN_E_INVALID before any device launch on the loaded problem (a batch that did not qualify launched nothing). */
int ktn_blocks_get_results(ktn_handle h, double* out, int64_t cap, int64_t* count);
/* The cut rows of instance `block` in its arena after the last device launch: the rows beyond its linear rows, in LP row order.
 * rowptr [n_rows + 1] (from 0), col [n_nnz] GLOBAL column indices, val [n_nnz] (coefficients after round_coefs), lo / hi [n_rows],
 * nl_slot [n_rows] the position of the cut's row in the engine's NL row list (ktn_last_sweep_slots numbering; from the arena's
 * last_cut / cut_prev lists), lambda [n_rows] where the cut was taken on the segment x_int -> x* (1: at x* itself, everywhere after a
 * Kelley launch).  *n_rows and *n_nnz are always set; with rowptr == NULL nothing else happens, otherwise every buffer is needed with
 * cap_rows >= *n_rows (rowptr: cap_rows + 1) and cap_nnz >= *n_nnz.  KTN_E_INVALID before any device launch on the loaded problem. */
int ktn_blocks_get_cuts(ktn_handle h, int64_t block, int64_t* rowptr, int32_t* col, double* val, double* lo, double* hi,
                        int64_t* nl_slot, double* lambda, int64_t cap_rows, int64_t cap_nnz, int64_t* n_rows, int64_t* n_nnz);
/* The multiplier of each cut row of instance `block` after the last device launch, row for row as in ktn_blocks_get_cuts, unscaled
 * (the arenas keep the multipliers unscaled between LP solves: y = y^ dr).  y_out == NULL only reports *count. */
int ktn_blocks_get_duals(ktn_handle h, int64_t block, double* y_out, int64_t cap, int64_t* count);
/* What has to happen between two device launches on the same arenas, alone (k_blocks_rewarm, csrc/batch_warm.hpp; a warm
 * ktn_optimize_blocks_ex runs it first).  Per instance, in this order: (a) warm only if its last record is :Optimal without
 * overflow, else state 0 and nothing is touched; (b) a crossed column l_j > u_j: state 2; (c) its slice of x is clamped into the
 * box; (d) every arena row, linear rows and cuts, is screened against the box by the test of ktn_set_var_bounds (amin_k, amax_k,
 * S_k, tau_k, 4 lanes per row in a fixed order): a proving row gives state 2, redundant rows are counted; (e) only when the cut
 * rows fill more than half of the cut room, M - m_lin > (cap_rows - m_lin) / 2, cut rows that are idle by the pool's rule
 * (y == 0 and slack > purge_margin * max(1, |finite bounds|) at the clamped x; no ageing) are dropped, the survivors keep their
 * order, multipliers and lambdas, and the cut lists are re-threaded over them (linear rows never move; a dropped row has y == 0, so
 * every list's multiplier sum stands).  out: [n_blocks x 8] doubles, instance after instance:
 *   0 state (0 cold, 1 warm, 2 infeasible)   1 LP rows   2 non-zeros   3 rows dropped   4 columns clamped
 *   5 smallest proving row of the arena (-1: none)   6 crossed columns   7 redundant rows
 * ktn_blocks_get_results / _get_cuts / _get_duals describe the compacted arenas afterwards (slot 6 of a record follows).  Idempotent:
 * until the next setter or launch a second call returns the same records and moves nothing.  Size convention of
 * ktn_blocks_get_results (out == NULL only reports *count = 8 n_blocks and runs nothing).  KTN_E_INVALID without a previous device
 * launch on the loaded problem, or after ktn_reset, ktn_set_blocks or a host fallback. */
int ktn_blocks_rewarm(ktn_handle h, double* out, int64_t cap, int64_t* count);
/* The dual bound of ktn_get_dual_bound per instance of a fused batch (ktn_set_blocks; rows and columns grouped by instance):
 * out[2 b] = bound of instance b from its own rows, columns and share c_b'x_b of the objective (without the loaded problem's
 * constant), out[2 b + 1] = its gap.  One workgroup per instance.  States and errors as ktn_get_dual_bound; out == NULL only
 * reports *count = 2 n_blocks. */
int ktn_blocks_get_dual_bounds(ktn_handle h, double* out, int64_t cap, int64_t* count);

/* ---- row-sharded LP over several GPUs (no reference counterpart: it splits the LP re-solve of
 * src/model.jl:259 and the cut loop of :272-283 over the ranks) -------------------------------------------------------
 * One process per GPU.  Every rank creates a handle, joins the group with ONE of the two calls below BEFORE
 * ktn_loadproblem, and loads ITS shard: all variables and the objective, a block of the linear rows and a block of the NL
 * rows (katana.jl_amd/distributed.py::shard_rows).  ktn_optimize is then a collective call: x is replicated, every rank
 * keeps the cuts it generates (no cut exchange), A x is local and A'y is a local partial plus an all-reduce of an n-vector
 * per PDHG iteration; the stop rule and every restart decision use all-reduced quantities, so all ranks return the same
 * status, objective and solution.  With a nonlinear objective the epigraph row belongs to rank 0.
 *   ktn_dist_unique_id  : 128-byte RCCL id, made by ONE rank and sent to the others (e.g. torch.distributed.broadcast)
 *   ktn_dist_init_rccl  : collectives = ncclAllReduce on the engine's stream (RCCL over xGMI)
 *   ktn_dist_init_callback : collectives through the caller: cb(user, host_buf, count, op) must all-reduce host_buf in
 *                         place over the ranks (op 0: sum, 1: max) and return 0 -- the engine stages through the host.
 *                         For tests (gloo; several ranks sharing one GPU, which RCCL does not allow).
 *   ktn_dist_ipc_export + ktn_dist_init_ipc : peer-buffer transport.  Every rank exposes a buffer of 2 x `capacity` doubles
 *                         (capacity >= the LP's column count) and a page of flag words; export returns their two
 *                         hipIpcMemHandle_t (2 x 64 bytes: data, flags); the caller gathers the `world` pairs in rank order
 *                         (any byte transport: torch.distributed.all_gather, MPI, a file) and hands them to init, which maps
 *                         the peers' buffers (xGMI peer access).  An all-reduce is then: partial written into the exposed slot,
 *                         one single-workgroup kernel that signals every rank and waits for every rank (bounded spin:
 *                         KTN_IPC_TIMEOUT_S, default 20 s, then KTN_E_HIP), and the consumer adding up the world's slots in rank
 *                         order itself -- no ring, no intermediate copy, identical bits on every rank.  2 <= world <= 8, one
 *                         node.  Ranks must destroy their handles together (ktn_destroy runs one last barrier).
 *   ktn_dist_allreduce_probe : collective self-test / timing of whatever transport the handle has: all-reduces (sum, max) a
 *                         vector whose result every rank can compute itself and returns the largest deviation, then the
 *                         mean time of `reps` sum all-reduces of n doubles.                                              */
typedef int (*ktn_allreduce_cb)(void* user, double* host_buf, int64_t count, int32_t op);
int ktn_dist_unique_id(char* out128);
int ktn_dist_init_rccl(ktn_handle h, const char* uid128, int32_t rank, int32_t world);
int ktn_dist_init_callback(ktn_handle h, int32_t rank, int32_t world, ktn_allreduce_cb cb, void* user);
#define KTN_IPC_HANDLE_BYTES 64
int ktn_dist_ipc_export(ktn_handle h, int32_t rank, int32_t world, int64_t capacity, char* out_handles128);
int ktn_dist_init_ipc(ktn_handle h, int32_t rank, int32_t world, const char* all_handles /* world x 128 bytes */);
int ktn_dist_allreduce_probe(ktn_handle h, int64_t n, int32_t reps, double* usec_per_call, double* max_abs_err);
/* leave the peer-buffer transport again (before ktn_loadproblem), e.g. after a failed ktn_dist_allreduce_probe: the handle
 * can then be given another transport (ktn_dist_init_rccl / _callback) -- decided once, at init, in the same process */
int ktn_dist_release_ipc(ktn_handle h);

#ifdef __cplusplus
}
#endif
#endif /* KATANA_HIP_H */
