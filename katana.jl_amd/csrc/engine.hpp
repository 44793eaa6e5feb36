// engine.hpp -- struct Engine: the state of one handle and the declarations of its methods.  No kernel is named here; the methods
// live in
//   load.hip    loadproblem as a list of stages (the index arithmetic that needs no device: load_host.hpp), tape shape classes,
//               QUAD rows, reset
//   sweep.hip   the separator sweep (precompute! + isconstrsat + gencut + round_coefs + _addcut), the host-evaluator rows, the KKT report
//   pool.hip    the cut pool: LP row storage, CSC mirror, working (epigraph-shifted) form, purging, append / pack / unpack
//   lp.hip      the LP solves: scaling, tiled copies, PDHG steps and checks, exact small / mid-size LPs, per-block LPs, recession ray
//   ecp.hip     the cutting-plane loop: begin / step / polish_step / end, objective certificate, device-side batch loop
//   dist.hip    collectives of the row-sharded LP: RCCL, peer buffers, host callback
//   rebound.hip the re-solve from the kept pool: bound, cost and row-bound setters, reopen, the screen of the rows against a new box
//   abi.hip     the C ABI of include/katana_hip.h
// (until the middle of round 4 all of it was engine.hip, one translation unit of 4 100 lines).
//
// Mirrors, function by function, the reference's driver (src/model.jl) with every piece of
// arithmetic on the device:
//   Engine::loadproblem   <- loadproblem!   src/model.jl:81-173
//   Engine::boundroutine  <- boundroutine   src/model.jl:175-197
//   Engine::begin/step/end<- optimize!      src/model.jl:219-319
//   Engine::sweep         <- precompute! + isconstrsat + gencut + round_coefs + _addcut
//   Engine::lp_solve      <- solve(m.linear_model)  (GLPK in the reference) replaced by a
//                            restarted, reflected Halpern PDHG on the growing cut matrix
// The CPU mirror of the LP algorithm used by the tests is oracle/pdlp_mirror.py
// (solve_lp_halpern); it is test infrastructure and never linked or called from here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include <rccl/rccl.h>

#include "common.hpp"
#include "types.hpp"
#include "prims.hpp"

namespace ktn {

static const double kInf = std::numeric_limits<double>::infinity();

// lanes per sparse row: the power of two nearest below the average row length (a row longer
// than G just loops), so that short-row matrices do not idle half of every wavefront
static inline int pick_group(double avg_len) {
    int g = 4;
    while (g < 64 && 2 * g <= avg_len) g <<= 1;
    return g;
}

struct LpResult {
    int status = KTN_STATUS_NONE;   // OPTIMAL / USERLIMIT
    int64_t iters = 0;
    double pobj = 0.0, dobj = 0.0, row_viol = 0.0, gap = 0.0;
    double dres_rel = 0.0;          // dual residual over (1 + ||c||): what the solve's gap tolerance is compared with
    bool exact = false;             // solved by the exact small-LP kernel: no tolerance tightening needed
    bool stag_exit = false;         // ended through the primal-stagnation exit (objective flat, gap within lp_stag_factor x tolerance)
};

// Development switches (tools/README.md), parsed ONCE PER HANDLE at ktn_create from the KTN_* environment of that moment: two
// handles made under different settings can be A/B'd in one process, nothing is `static`, and -- unlike the getenv calls that
// sat inside lp_solve_core until round 3 -- every one of them is listed here, next to ktn_params, with what ships.
struct DevParams {
    bool no_pinned_check = false, debug_load = false, no_csc_merge = false, tiled_general_build = false, debug_blocks = false,
         no_tiled_check = false, no_setup_reuse = false, debug_lp = false, no_packed = false, force_collective = false;
    int sweep_rows = 0;            // KTN_SWEEP_ROWS       NL rows per lane group of the sweep (0 = by size)
    int blk_cfg = -1;              // KTN_BLK_CFG          tuning variant of the column-blocked sweep
    int sweep_blocked = -1;        // KTN_SWEEP_BLOCKED    0 = row kernel instead of the column-blocked sweep
    int sweep_batched = -1;        // KTN_SWEEP_BATCHED    0 = row kernel instead of the batch-blocked sweep for many short rows, 1 = always
    int tape_classed = -1;         // KTN_TAPE_CLASSED     tape rows by shape class (k_tape_classed): -1 = classes of >= 64 rows, 0 = interpreter for
                                   //                      every tape row, 1 = every class of >= 2 rows
    int quad_group = 0;            // KTN_QUAD_GROUP       lanes per Jacobian entry of k_quad_jac (0 = by mean segment length)
    int esh_quad_group = 0;        // KTN_ESH_QUAD_GROUP   lanes per row of k_esh_quad (0 = those of k_quad_stats, by mean row length)
    int ecp_quad_group = 0;        // KTN_ECP_QUAD_GROUP   lanes per Jacobian entry of the QUAD pass of k_ecp_blocks (0 = those of k_quad_jac)
    int tiled_wg = 2;              // KTN_TILED_WG         workgroups per CU of k_spmv_tiled
    int ecp_power = 20;            // KTN_ECP_POWER        power passes of the device-side batch loop
    int grp_rows = 0, grp_cols = 0;// KTN_GRP_ROWS / COLS  lanes per LP row / column (0 = by average length)
    int tiled = -1;                // KTN_TILED            force the tiled SpMV off (0) / on (1)
    double smax_reuse = 0.0;       // KTN_SMAX_REUSE       reuse of the sigma_max estimate (measured: harmful)
    int power_passes = 0;          // KTN_POWER_PASSES     power-iteration passes (0 = 8)
    int omega_robust = 1;          // KTN_OMEGA_ROBUST     0 = initial primal weight from the plain 2-norm ratio
    int packed_trips = 0;          // KTN_PACKED_TRIPS     outputs per lane group of the packed steps (0 = default)
    int first_chunk = 31;          // KTN_FIRST_CHUNK      iterations before the first check after a restart
    int stag_chunk = 0;            // KTN_STAG_CHUNK       check cadence while only the objective is unsettled (measured, off)
    int near_chunk = -1;           // KTN_NEAR_CHUNK       overrides lp_near_check
    int stag_checks = 2;           // KTN_STAG_CHECKS      flat checks the stagnation exit asks for
    double flat_factor = 0.4;      // KTN_FLAT_FACTOR      "flat" = within this fraction of the gap tolerance
    int omega_art = 1;             // KTN_OMEGA_ART        0 = no primal-weight update on restarts the residual did not earn
    double omega_art_k = 256.0;    // KTN_OMEGA_ART_K      period length at which such a restart's ratio gets the full weight 0.5
    double omega_art_clamp = 0.0, omega_clamp = 0.0, omega_clamp_down = 0.0;   // KTN_OMEGA_ART_CLAMP / _CLAMP / _CLAMP_DOWN (measured, off)
    double ipc_timeout_s = 20.0;   // KTN_IPC_TIMEOUT_S    spin bound of the peer-buffer transport
    bool raw_duals = false;        // KTN_RAW_DUALS        ktn_lp_get_duals returns lp_y as the loop sees it, also after an exact mid-size solve
    int mid_refactor = 0;          // KTN_MID_REFACTOR     pivots between refactorisations of the mid-size exact LP (<= 0: kMidRefactor, mid_lp.hpp)
    int kkt_group = 0;             // KTN_KKT_GROUP        lanes per column of k_lagr_grad (0 = by mean column length)
    int feas_group = 0;            // KTN_FEAS_GROUP       lanes per row of k_feas_sep and k_feas_quad (0 = those of the sweep / of k_quad_stats)
    bool feas_xstar_pre = false;   // KTN_FEAS_XSTAR_PRECOMPUTE   the feasible point takes x* from the last ktn_sep_precompute instead of lp_x (tests)
    int poison = 0;                // KTN_POISON           fill every new device allocation (common.hpp): 0 unset, 1 `zero`, 2 `nan` (floating-point
                                   //                      buffers NaN, integer buffers 0), -1 a value that is neither (ktn_create refuses it)
    static bool flag(const char* k) { return std::getenv(k) != nullptr; }
    static int geti(const char* k, int d) { const char* v = std::getenv(k); return v ? std::atoi(v) : d; }
    static double getd(const char* k, double d) { const char* v = std::getenv(k); return v ? std::atof(v) : d; }
    void from_env() {
        no_pinned_check = flag("KTN_NO_PINNED_CHECK"); debug_load = flag("KTN_DEBUG_LOAD"); no_csc_merge = flag("KTN_NO_CSC_MERGE");
        tiled_general_build = flag("KTN_TILED_GENERAL_BUILD"); debug_blocks = flag("KTN_DEBUG_BLOCKS"); no_tiled_check = flag("KTN_NO_TILED_CHECK");
        no_setup_reuse = flag("KTN_NO_SETUP_REUSE"); debug_lp = flag("KTN_DEBUG_LP"); no_packed = flag("KTN_NO_PACKED");
        force_collective = flag("KTN_FORCE_COLLECTIVE");
        sweep_rows = geti("KTN_SWEEP_ROWS", sweep_rows); blk_cfg = geti("KTN_BLK_CFG", blk_cfg); sweep_blocked = geti("KTN_SWEEP_BLOCKED", sweep_blocked);
        sweep_batched = geti("KTN_SWEEP_BATCHED", sweep_batched); tape_classed = geti("KTN_TAPE_CLASSED", tape_classed);
        quad_group = geti("KTN_QUAD_GROUP", quad_group); esh_quad_group = geti("KTN_ESH_QUAD_GROUP", esh_quad_group);
        ecp_quad_group = geti("KTN_ECP_QUAD_GROUP", ecp_quad_group);
        tiled_wg = geti("KTN_TILED_WG", tiled_wg); ecp_power = geti("KTN_ECP_POWER", ecp_power);
        grp_rows = geti("KTN_GRP_ROWS", grp_rows); grp_cols = geti("KTN_GRP_COLS", grp_cols); tiled = geti("KTN_TILED", tiled);
        smax_reuse = getd("KTN_SMAX_REUSE", smax_reuse); power_passes = geti("KTN_POWER_PASSES", power_passes);
        omega_robust = geti("KTN_OMEGA_ROBUST", omega_robust); packed_trips = geti("KTN_PACKED_TRIPS", packed_trips);
        first_chunk = geti("KTN_FIRST_CHUNK", first_chunk); stag_chunk = geti("KTN_STAG_CHUNK", stag_chunk); near_chunk = geti("KTN_NEAR_CHUNK", near_chunk);
        stag_checks = geti("KTN_STAG_CHECKS", stag_checks); flat_factor = getd("KTN_FLAT_FACTOR", flat_factor);
        omega_art = geti("KTN_OMEGA_ART", omega_art); omega_art_k = getd("KTN_OMEGA_ART_K", omega_art_k);
        omega_art_clamp = getd("KTN_OMEGA_ART_CLAMP", omega_art_clamp); omega_clamp = getd("KTN_OMEGA_CLAMP", omega_clamp);
        omega_clamp_down = getd("KTN_OMEGA_CLAMP_DOWN", omega_clamp_down); ipc_timeout_s = getd("KTN_IPC_TIMEOUT_S", ipc_timeout_s);
        mid_refactor = geti("KTN_MID_REFACTOR", mid_refactor); raw_duals = flag("KTN_RAW_DUALS");
        kkt_group = geti("KTN_KKT_GROUP", kkt_group); feas_group = geti("KTN_FEAS_GROUP", feas_group);
        feas_xstar_pre = flag("KTN_FEAS_XSTAR_PRECOMPUTE");
        if (const char* v = std::getenv("KTN_POISON"); v && *v) poison = !std::strcmp(v, "zero") ? 1 : !std::strcmp(v, "nan") ? 2 : -1;
    }
};

struct LoadScratch;                 // load.hip

struct Engine {
    ktn_params prm;
    DevParams dev;
    std::string err;
    hipStream_t stream = nullptr;
    int device = 0;

    // ---- problem (host) ----
    bool loaded = false;
    int64_t n0 = 0, m0 = 0;        // original sizes
    int64_t n_lp = 0;              // LP variables (n0, or n0+1 with the epigraph variable)
    int64_t m_ext = 0;             // rows of the extended structure = m0 + 1 (objective row last)
    int64_t nnz_ext = 0;
    int sense = KTN_MIN;
    bool obj_linear = true;
    bool has_inf_bound = false;
    bool has_big_bound = false;    // a FINITE variable bound with |b| >= kDenseBig: the exact LP paths leave it out and check it afterwards (dense_lp.hpp)
    std::vector<int64_t> h_rowptr;
    std::vector<int32_t> h_col;
    std::vector<uint8_t> h_rowkind;
    std::vector<double> h_lb, h_ub;      // per extended row
    std::vector<int32_t> h_nlrows;
    int64_t m_nl = 0, n_tape_nl = 0;
    int64_t m_nl_global = 0;       // NL rows over all ranks of a row-sharded LP (== m_nl otherwise): decisions that steer collectives use it
    int grp_sweep = 32;
    int sweep_rows_per_group = 1;  // R of k_sep_sweep (1: k_sep_eval); fixed at load from m_nl, G and the CU count
    bool pre_multirow = false;     // precompute_all runs k_sep_sweep<G, 4, true>; fixed at load from m_ext, G and the CU count

    // ---- device NLP ----
    DBuf<int64_t> d_rowptr, d_nodeptr;
    DBuf<int32_t> d_col, d_nodeop, d_nodea, d_nodeb;
    DBuf<uint8_t> d_rowkind, d_padzero;
    DBuf<uint64_t> d_dkeys, d_dsorted;      // deepest-cut selection
    // host-evaluator fallback (KTN_ROW_HOST)
    ktn_eval_rows_cb cb_rows = nullptr;
    ktn_eval_obj_cb cb_obj = nullptr;
    void* cb_user = nullptr;
    int64_t n_host = 0, n_host_nl = 0;
    bool host_constr_rows = false, host_obj = false;
    std::vector<double> h_xh, h_gh, h_jh;
    DBuf<double> d_gh, d_jh;
    DBuf<int32_t> d_hostrows;
    void host_eval(const double* d_x);
    DBuf<int32_t> d_colk;
    DBuf<double2> d_pp;
    // block-major copy of the long rows for the column-blocked sweep (k_sep_eval_blk)
    bool blk_on = false;
    int blk_nb = 0, blk_cfg = 0, blk_cols = kBlkCols, blk_wg_per_cu = 2, num_cus = 256;
    DBuf<int32_t> d_bcolk;
    DBuf<double2> d_bpp;
    DBuf<int64_t> d_bseg;
    DBuf<int4> d_bkind;
    DBuf<SepSlot> d_slots;
    DBuf<SepPartial> d_part;
    DBuf<double> d_rconst, d_lb, d_ub, d_nodec, d_nodeval, d_nodeadj;
    DBuf<int32_t> d_nlrows, d_allrows, d_taperows_all, d_taperows_nl;
    // tape rows by shape class (tape_classes.hpp; built by build_tape_classes at load).  A class holds NL rows only or none: the
    // sweep launches the classes of NL rows, precompute_all all of them; d_tapeint_*: the rows left to k_tape_eval
    int64_t tc_rows = 0, tc_rows_nl = 0;
    struct TcLaunch { int64_t wave0, nwaves; size_t lds; bool nl; };      // one launch: the classes of one size bucket, NL rows or not
    std::vector<TcLaunch> tc_launches;
    bool tc_lds_set = false;
    void launch_tape_classed(bool nl_only, const int32_t* mslot, const double* d_x, double f_tol);
    double tape_bytes = 0.0;                   // algorithmic bytes of one evaluation of the NL tape rows
    DBuf<int32_t> d_tapeint_all, d_tapeint_nl, d_tc_wavecls, d_tc_wavefirst, d_tc_op, d_tc_a, d_tc_b, d_tc_scol, d_tc_mrow, d_tc_mslot;
    DBuf<double> d_tc_c, d_tc_cst;
    DBuf<TapeClassMeta> d_tc_meta;
    DBuf<uint8_t> d_tc_rowflag;                // [m_ext] 1: the row is evaluated by k_tape_classed (k_gj_stats skips it)
    void build_tape_classes(const LoadScratch& S);
    TapeClassDev tape_class_view();
    // KTN_ROW_QUAD rows (quad_rows.hpp; built by build_quad_rows at load): the Q entries in two streams, the QUAD rows' Jacobian
    // entries numbered in row order, and two launch lists -- all QUAD rows (precompute_all), those among the NL rows (sweep)
    int64_t n_quad = 0, n_quad_nl = 0, n_quad_ent = 0, n_quad_ent_nl = 0, quad_nnz = 0;
    int grp_quad = 4, grp_quad_rows = 4;
    double quad_bytes = 0.0;                   // algorithmic bytes of one evaluation of the NL QUAD rows
    DBuf<int32_t> d_qcol, d_qrows_all, d_qrows_nl;
    DBuf<double> d_qval, d_qvterm;
    DBuf<int64_t> d_qptr, d_qjidx, d_qslots_all, d_qslots_nl, d_qtbase_all, d_qtbase_nl, d_qent_nl;
    void build_quad_rows(const ktn_nlp_desc* d, const LoadScratch& S);
    void launch_quad(bool nl_only, const double* d_x, double f_tol);
    // sweep state
    DBuf<double> d_g, d_jac, d_bconst, d_maxc, d_xs, d_ray, d_scal;
    DBuf<int32_t> d_nonfin, d_violslots, d_anynf;
    DBuf<int64_t> d_flag, d_cnt, d_rank, d_cntscan, d_lastcut, d_cutprev;
    DBuf<double> d_ones;
    DBuf<int32_t> d_age, d_age2;
    DBuf<int64_t> d_keep, d_keepnnz, d_newidx, d_newptr, d_cutprev2, lp_rowptr2;
    DBuf<int32_t> lp_col2;
    DBuf<double> lp_val2, lp_lo2, lp_hi2, lp_y2;
    DBuf<char> d_scantmp;
    bool have_precompute = false;

    // ---- LP ----
    DBuf<int64_t> lp_rowptr;
    DBuf<int32_t> lp_col;
    DBuf<double> lp_val, lp_lo, lp_hi, lp_y, lp_c, lp_l, lp_u, lp_x;
    double c0 = 0.0;
    int64_t M = 0, NNZ = 0, M_base = 0, NNZ_base = 0;
    int64_t numcuts = 0, numcuts_base = 0;
    bool lp_dirty = true;
    // matrix version: bumped wherever rows are appended or removed.  A re-solve of the SAME matrix (the floor-tolerance re-solve
    // of an iteration that found every row satisfied) reuses the scaling, the tiled copies and the sigma_max estimate.
    uint64_t lp_version = 1, scaled_version = 0, smax_version = 0;
    bool scaled_identity = false;
    // NL-row blocks over several GPUs with a replicated LP (the north star's design): the caller's callback exchanges the cuts of
    // a sweep (ktn_set_cut_exchange); the cutting-plane loop itself -- floor rule, refinement, certificate -- stays Engine::step
    ktn_exchange_cb exch_cb = nullptr;
    void* exch_user = nullptr;
    int64_t exch_lo = 0;         // global id of this handle's first NL row
    bool exchanging() const { return exch_cb != nullptr; }
    bool sharded_rows = false;   // rows were appended/truncated from the host: cut lists are not tracked ...
    bool glists = false;         // ... unless the host supplies global NL-row ids (ktn_lp_enable_global_lists)
    int64_t nl_total = 0;
    int64_t last_sweep_cuts = 0;
    DBuf<int64_t> d_glast, d_nlid;
    void append_link(int64_t nrows, const int64_t* nl_id_host);       // rows [M, M + nrows) just appended from the host
    void append_link_dev(int64_t nrows);                              // the same with the ids already in d_nlid (device-resident exchange)
    void clip_lists(int64_t nrows);                                   // ktn_lp_truncate: list heads leave the rows >= nrows (k_list_clip)
    int64_t* list_heads() { return glists ? d_glast.p : d_lastcut.p; }
    int64_t list_count() const { return glists ? nl_total : m_nl; }
    bool lists_ok() const { return !sharded_rows || glists; }
    // CSC mirror + scaling + PDHG workspace
    DBuf<int64_t> c_ptr, c_cnt;
    DBuf<int32_t> c_row;
    DBuf<double> c_val, c_sval, r_sval;
    // per mirror position the CSR entry it came from; rows / entries the mirror covers; `lp_epoch` counts the changes that are
    // NOT appends (reset, purge, truncate) -- while it stands still the mirror is extended by a merge instead of a sort
    DBuf<uint32_t> c_perm, c_perm2;
    DBuf<int32_t> c_row2;
    DBuf<int64_t> c_ptr2, c_off;
    int64_t csc_M = -1, csc_NNZ = 0;
    uint64_t lp_epoch = 1, csc_epoch = 0;
    void csc_merge_appended();
    // Working form of the LP during a first-order solve with a nonlinear objective: the epigraph cuts relative to the newest one
    // (kernels.hpp "epigraph reference shift").  The stored LP keeps the reference's form; w_shift says that the CSC mirror,
    // the scaling and the w* arrays currently hold the shifted problem.
    bool w_shift = false;
    int64_t M_lin = 0;                          // LP rows [0, M_lin) are the pass-through linear rows: never epigraph cuts
    DBuf<double> wval, wlo, whi, wc, epi_ref, epi_scal;      // epi_scal: [0] b_ref, [1] a_ref'x
    DBuf<unsigned long long> epi_newest;
    const double* Wval() const { return w_shift ? wval.p : lp_val.p; }
    const double* Wlo() const { return w_shift ? wlo.p : lp_lo.p; }
    const double* Whi() const { return w_shift ? whi.p : lp_hi.p; }
    const double* Wc() const { return w_shift ? wc.p : lp_c.p; }
    bool want_shift(int mode) const { return prm.epi_shift != 0 && !obj_linear && mode == 0 && !row_sharded() && n_blocks == 0; }
    void build_working();
    void ensure_matrix(bool shift);
    void epi_dot(const double* x);              // epi_scal[1] = a_ref'x  (a_ref is zero at the epigraph variable)
    DBuf<uint64_t> k_in, k_out;
    DBuf<uint32_t> p_in, p_out;
    DBuf<char> d_sorttmp;
    DBuf<double> dr_r, dc_r;
    DBuf<ColRec> d_crec;
    DBuf<RowRec> d_rrec;
    DBuf<int2> d_cbl;
    bool packed_on = false;        // plain steps read packed per-column / per-row records (kernels.hpp)
    int packed_trips = 1;          // outputs per lane group in the packed kernels (KTN_PACKED_TRIPS: 1, 2, 4)
    DBuf<double> dr2, dc2;                      // ping-pong partners of dr / dc in the scaling passes
    DBuf<double> dr, dc, statr, statc, ch, lh, uh, loh, hih, xh, yh, x0h, y0h, xth, yth, xbar, pv, pw, box;
    DBuf<double> partials, chk_part, chkout, power_v, power_v0;
    int64_t power_v0_n = -1;                   // size the cached start vector of the power iteration was made for
    // the check sums of a one-GPU solve land in pinned, device-mapped host memory: k_chk_final writes them there and the host
    // reads them after the stream synchronisation -- no copy kernel (4.5 us + a boundary) per check
    double* h_chk = nullptr;
    double* h_chk_dev = nullptr;
    // exact small-LP path (dense_lp.hpp)
    int64_t lp_iter_budget = 0, dense_credit = 0, dense_run = 0;
    DBuf<int32_t> ds_W, ds_valid;
    DBuf<double> ds_dense, ds_out;
    // exact mid-size LP (mid_lp.hpp): basis inverse, working set, x and multipliers persist across the ECP iterations
    DBuf<double> md_Binv, md_hW, md_x, md_lam, md_u, md_d, md_r, md_pv, md_c, md_aug, md_prow, md_fcol;
    int64_t md_since_refactor = 0;
    DBuf<double> md_y;                  // scratch of mid_true_duals: row multipliers of the TRUE cost (lp_y: those of the perturbed cost)
    uint64_t md_y_version = 0;          // lp_version of the last exact mid-size solve that ended optimal (0: none, or another solve since)
    bool mid_true_duals(double* y_out); // ktn_lp_get_duals while that solve's rows and working set stand
    int64_t mid_backoff = 0, mid_backoff_len = 0;      // after a failed exact solve the first-order method carries on alone for a while
    DBuf<int32_t> md_W, md_pi, md_lost;
    DBuf<MidState> md_st;
    bool md_valid = false;
    int64_t mid_credit = 0, mid_run = 0;
    DBuf<int32_t> d_longrows;
    // long COLUMNS of the mirror (a variable that every cut contains: min-max / epigraph-style models): found by find_long_cols
    // after the mirror is built; the column-side kernels then run in their vector form with a workgroup per long column
    DBuf<int32_t> d_longcols;
    int64_t n_longc = 0;
    int64_t col_gain_max = 0;                      // most NL rows sharing one column: what a column can gain per sweep
    int64_t col_len_max = -1, col_scan_rows = 0;   // longest column at the last scan, rows of the LP then (-1: never scanned)
    int64_t col_removed_rows = 0;                  // rows purged / truncated since that scan (appended since = M - col_scan_rows + this)
    void find_long_cols();
    void spmv_cols(const SpMat& AT, const double* v, double* out, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
    static constexpr int kMaxChunk = 512;
    int64_t n_long = 0;
    static constexpr int64_t kLongRow = 2048;
    int64_t max_row_len = (int64_t)1 << 62;    // longest row the LP can hold (NLP structure rows + appended rows): no scan for long rows below kLongRow
    double omega = 1.0;
    bool have_omega = false;
    int grp_rows = 8, grp_cols = 8;
    // tiled copies of A^ (outputs = rows) and A^' (outputs = columns) for LPs beyond the caches (kernels.hpp "tiled SpMV")
    struct TiledBuf {
        DBuf<int64_t> segstart, segtot;
        DBuf<uint16_t> bptr, cur, idx;
        DBuf<int32_t> pcnt;
        DBuf<double> val;
        int nb_in = 0;
        int64_t tiles = 0, grid = 0, pieces = 1;     // persistent grid and the largest number of pieces of a tile
        TiledMat view() const { return TiledMat{segstart.p, bptr.p, idx.p, val.p, nb_in}; }
    } tA, tAT;
    DBuf<double> tpart;
    bool tiled_on = false, tiled_built = false;
    void launch_tiled(const TiledBuf& T, int64_t n_out, int64_t n_in, const double* in, hipEvent_t e0);
    bool build_tiled(TiledBuf& T, int64_t n_out, int64_t n_in, const int64_t* ptr, const int32_t* idx, const double* val, int64_t skip_longer);
    // throughput mode (batch_lp.hpp): the loaded problem is block-diagonal, one workgroup per block runs its LP
    int64_t n_blocks = 0, blocks_built_rows = -1;
    size_t lds_set_lp = 0, lds_set_ecp = 0;      // dynamic-LDS sizes already granted to the two per-instance kernels on this handle's device
    std::vector<int64_t> h_blkcol;
    DBuf<int64_t> d_blkcol;
    DBuf<int32_t> d_blkrowptr, d_blkrows, d_rowloc, d_crowl;
    DBuf<double> d_blkomega, d_blkres;
    int blk_nmax = 0, blk_mmax = 0;
    void build_blocks();
    // optimize_blocks_device: not launched / all :Optimal / some instance not / the instances that are not were all ended
    // :Infeasible by the screen of a warm launch (the host loop cannot help them: no fallback)
    enum { kBlocksUnfit = 0, kBlocksDone = 1, kBlocksOpen = 2, kBlocksScreened = 3 };
    int optimize_blocks_device(int cap_mul, int flags);
    // Warm re-solve of the resident arenas (KTN_BLOCKS_WARM; batch_warm.hpp, DESIGN.md section 14 "In the device-side loop").
    // blocks_warm_ok: the arenas, e_res and lp_x are those of the last device launch on the loaded problem (dropped by ktn_reset,
    // ktn_loadproblem, ktn_set_blocks and a host fallback; kept by the setters).  blocks_rewarmed: h_rewarm holds the records of
    // k_blocks_rewarm for the data in force (dropped by a setter and by a launch), so ktn_blocks_rewarm is idempotent.
    bool blocks_warm_ok = false, blocks_rewarmed = false, reset_keeps_x = false;
    int blocks_cap_mul = 0;
    std::vector<double> h_rewarm;
    DBuf<double> e_rewarm;
    hipEvent_t ev_rewarm[2] = {nullptr, nullptr};
    void blocks_drop_warm() { blocks_warm_ok = false; blocks_rewarmed = false; }
    void blocks_rewarm();                         // k_blocks_rewarm over every instance, unless h_rewarm is current
    // the last device launch on the loaded problem, for ktn_blocks_get_results / ktn_blocks_get_cuts
    bool blocks_launched = false, blocks_last_esh = false;
    std::vector<int64_t> h_ar_row0, h_ar_nnz0, h_ar_rows, h_blklin, h_blknl;      // arena offsets and row capacities, offsets of linear rows / NL slots
    std::vector<double> h_blkres;
    DBuf<double> e_lam, e_res2;                   // k_ecp_blocks<1>: lambda per arena row slot, four counters per instance
    size_t lds_set_ecp_esh = 0;
    void blocks_cuts(int64_t block, std::vector<int64_t>& rowptr, std::vector<int32_t>& col, std::vector<double>& val,
                     std::vector<double>& lo, std::vector<double>& hi, std::vector<int64_t>& slot, std::vector<double>& lam);
    DBuf<EcpArena> d_ar;                          // arenas of the device-side loop
    DBuf<int64_t> d_blklin, d_blknl, d_blkqrow, d_blkqent;
    DBuf<int32_t> e_rptr, e_cptr, e_last, e_prev;
    DBuf<uint16_t> e_rcol, e_crow;
    DBuf<double> e_xbest, e_ax, e_rval, e_rsval, e_lo, e_hi, e_y, e_dr, e_loh, e_hih, e_cval, e_csval, e_dc, e_ch, e_lh, e_uh, e_res;     // batch_ecp.hpp: the whole ECP loop of every instance in its own workgroup
    bool lp_solve_blocks(double tol_p, double tol_g, double eta, LpResult* R, int64_t max_it);
    double smax_prev = 0.0;
    int64_t smax_rows = 0;
    int64_t scal_rows = 0, scal_cols = 0;   // dr[0, scal_rows) / dc[0, scal_cols) hold the scaling of the last solve

    // ---- run state ----
    int status = KTN_STATUS_NONE;
    int lp_status = KTN_STATUS_OPTIMAL;
    int64_t iter = 0;
    double soltime = 0.0, objval = std::numeric_limits<double>::quiet_NaN();
    double last_maxviol = 1e300;
    double obj_prev = kInf;
    bool allsat = false, begun = false, tight_done = false;
    // terminal refinement (DESIGN.md section 5 "Polish"): after the stop rule of model.jl:257,273 holds, small problems keep
    // cutting at polish_factor * f_tol; the point returned is the best one that satisfies the reference's rule
    bool polishing = false, polish_done = false;
    int polish_count = 0;
    double polish_phi = 1e-3;       // the refinement cuts rows beyond polish_phi * f_tol
    double cert_target = 0.0;       // > 0: certificate-driven refinement (kernels.hpp "objective certificate"), ends when met
    double cert_gap = 0.0;          // relative LP gap tolerance of the refinement solves (a quarter of the objective target)
    DBuf<double> d_cert;
    double objective_certificate(int64_t id_offset = 0, bool raw = false);
    double certificate_all_ranks();
    bool sweep_all(const double* d_x, double f_cut, bool lp_ok, int lp_stat, int64_t* nviol, double* maxviol, double* extra0, double* extra1);
    double certificate_blocks(double* gap_tol);
    DBuf<double> d_certblk;
    double best_viol = kInf, best_obj = 0.0;
    DBuf<double> d_xbest;
    // print_header / print_stats bookkeeping  src/model.jl:209-217,252-254,284-303
    int64_t log_cuts_lastprnt = 0, log_max_viol = 0, purged_total = 0;
    bool logging() const { return prm.log_level > 0 && dist.rank == 0; }      // (row-sharded: one table, from rank 0)
    void print_header() const {
        std::printf("%-10s %-15s %-15s %-20s %-20s %-15s\n", "Iteration", "Total cuts", "Cuts added", "Max constr. viol.",
                    "Avg constr. viol.", "Current cuts");
    }
    // model.jl:213-217.  "Current cuts" is numcuts in the reference (it never removes a cut, :215 TODO); here it is the
    // number of cuts still in the LP after purging.
    void print_stats(int64_t iter_lastprnt) const {
        const double avg = (double)log_cuts_lastprnt / ((double)iter_lastprnt * (double)m_nl);
        std::printf("%-10lld %-15lld %-15lld %-20lld %-20.2f %-15lld\n", (long long)iter, (long long)numcuts,
                    (long long)log_cuts_lastprnt, (long long)log_max_viol, avg, (long long)(numcuts - purged_total));
        std::fflush(stdout);
    }
    std::chrono::steady_clock::time_point t_start;
    std::vector<std::vector<double>> lp_sols;
    std::map<std::string, double> stats;
    // profiling events
    std::vector<hipEvent_t> ev_pool;
    struct EvRec { int kind; size_t a, b; double bytes; };
    std::vector<EvRec> ev_recs;
    size_t ev_used = 0;

    PoisonState poison;            // KTN_POISON of this handle and its count of fills; named by the ABI layer around every call (KTN_TRY)
    // parent: the engine that makes this one for a sub-problem of its own (esh_find_interior); the fill mode is the parent's
    explicit Engine(const ktn_params& p, const Engine* parent = nullptr) : prm(p) {
        dev.from_env();
        if (parent) dev.poison = parent->dev.poison;
        if (dev.poison < 0) throw Error(KTN_E_INVALID, "KTN_POISON must be `zero` or `nan`");
        poison.mode = dev.poison;
        PoisonScope poison_scope(&poison);
        if (prm.cut_algo != KTN_CUT_KELLEY && !esh_mode())
            throw Error(KTN_E_INVALID, "cut_algo must be KTN_CUT_KELLEY (0), KTN_CUT_SUPPORTING (1) or KTN_CUT_SUPPORTING_QUAD (2)");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            throw Error(KTN_E_NODEVICE, "no HIP device visible: the Katana HIP engine has no CPU path");
        if (prm.device >= 0) {
            KTN_HIP(hipSetDevice(prm.device));
            device = prm.device;
        } else {
            KTN_HIP(hipGetDevice(&device));
        }
        {
            int cus = 0;
            if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) num_cus = cus;
        }
        KTN_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        partials.resize((size_t)kRedBlocks * kChkQ * 2, stream);
        chkout.resize(kChkQ * 2 + 16, stream);
        if (!dev.no_pinned_check &&
            hipHostMalloc((void**)&h_chk, sizeof(double) * (2 * kChkQ + 16), hipHostMallocMapped) == hipSuccess) {
            if (hipHostGetDevicePointer((void**)&h_chk_dev, h_chk, 0) != hipSuccess) { (void)hipHostFree(h_chk); h_chk = nullptr; h_chk_dev = nullptr; }
        } else {
            h_chk = nullptr;
            (void)hipGetLastError();
        }
        d_scal.resize(8, stream);
        d_anynf.resize(4, stream);
    }
    ~Engine() {
        delete child;
        if (dist.comm) (void)ncclCommDestroy(dist.comm);
        ipc_release();
        for (auto e : ev_pool) (void)hipEventDestroy(e);
        for (auto e : ev_screen) if (e) (void)hipEventDestroy(e);
        for (auto e : ev_rebase) if (e) (void)hipEventDestroy(e);
        for (auto e : ev_rewarm) if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
        if (h_chk) (void)hipHostFree(h_chk);
    }

    void sync() { KTN_HIP(hipStreamSynchronize(stream)); }
    bool chk_pinned() const { return h_chk_dev != nullptr && !row_sharded(); }       // (row-sharded: the sums are all-reduced on the device first)
    double* chk_target() { return chk_pinned() ? h_chk_dev : chkout.p; }
    void check_launch() { KTN_HIP(hipGetLastError()); }

    // ------------------------------------------------------- row-sharded LP over several GPUs ---
    // (kernels.hpp "row-sharded".)  world > 1: this handle holds a block of the linear rows and the
    // cuts of its block of NL rows; x is replicated, y local.  Collectives run on the engine's own stream: RCCL (xGMI)
    // when the communicator was made by ktn_dist_init_rccl, or a host callback (tests: gloo, ranks sharing one GPU).
    struct DistCtx {
        int rank = 0, world = 1;
        bool force = false;            // world == 1 but run the collectives anyway (one-rank RCCL test)
        ncclComm_t comm = nullptr;
        ktn_allreduce_cb cb = nullptr;
        void* user = nullptr;
        std::vector<double> hbuf;
        // peer-buffer transport (ktn_dist_ipc_export / ktn_dist_init_ipc; kernels.hpp "peer-buffer transport")
        struct Ipc {
            bool on = false;
            int64_t cap = 0;                          // doubles per slot
            double* data = nullptr;                   // this rank's exposed buffer: 2 slots
            unsigned long long* flags = nullptr;      // this rank's flag words (uncached)
            void* opened[2 * kIpcMaxRanks] = {};      // what hipIpcOpenMemHandle returned (to close)
            IpcPeers P = {};
            unsigned long long epoch = 0;
            long long timeout_ticks = 0;
            int* h_err = nullptr;                     // pinned, device-mapped: a timed-out spin reports here
            int* h_err_dev = nullptr;
        } ipc;
    } dist;
    // the slot the NEXT all-reduce publishes from: a producer may write its partial straight into it
    int64_t ipc_off() const { return (int64_t)(dist.ipc.epoch & 1ull) * dist.ipc.cap; }
    double* ipc_slot() const { return dist.ipc.data + ipc_off(); }
    void ipc_check() {
        if (dist.ipc.on && dist.ipc.h_err && *dist.ipc.h_err != 0) {
            const int code = *dist.ipc.h_err;           // 1 + r: rank r did not arrive in time; 101 + r: rank r reported its own failure
            if (code > 100)
                throw Error(KTN_E_HIP, "peer-buffer transport: rank " + std::to_string(code - 101) + " gave up (told rank " + std::to_string(dist.rank) + ")");
            throw Error(KTN_E_HIP, "peer-buffer transport: rank " + std::to_string(dist.rank) + " timed out waiting for rank " + std::to_string(code - 1));
        }
    }
    // signal "my slot of this epoch is complete" to every rank and wait for theirs; returns the slot offset to read
    int64_t ipc_barrier();
    void ipc_release();
    void probe_fill(int64_t n, double* v, double value);    // v[j] = value + 1e-3 (j mod 1000): contents of ktn_dist_allreduce_probe
    DBuf<double> d_red;            // small device scratch for scalar reductions
    bool row_sharded() const { return dist.world > 1 || dist.force; }
    void allreduce(double* d, size_t n, int op);          // in place; op 0: sum, 1: max
    // k values reduced over the ranks (host in, host out); every rank gets the identical result
    void allreduce_host(double* v, int k, int op);

    // ------------------------------------------------------------------ profiling ---
    size_t ev_get() {
        if (ev_used == ev_pool.size()) {
            hipEvent_t e;
            KTN_HIP(hipEventCreate(&e));
            ev_pool.push_back(e);
        }
        return ev_used++;
    }
    // profile mode: the timed launches go through launch_ev (launch.hpp), whose start/stop events
    // carry the dispatch's own begin/end timestamps (what rocprofv3 --kernel-trace reports)
    void ev_flush() {   // stream must be synchronised
        static const char* names[6] = {"kx", "ky", "sweep_eval", "allreduce", "tape_eval", "quad_eval"};
        for (auto& r : ev_recs) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev_pool[r.a], ev_pool[r.b]) == hipSuccess) {
                std::string k = names[r.kind];
                stats[k + "_time_s"] += ms * 1e-3;
                stats[k + "_launches"] += 1.0;
                stats[k + "_bytes"] += r.bytes;
            }
        }
        ev_recs.clear();
        ev_used = 0;
    }

    // --------------------------------------------------------------- reductions ---
    double dev_dot(int64_t n, const double* a, const double* b);
    double dev_finite_sq(int64_t n, const double* a);
    void exclusive_scan(const int64_t* in, int64_t* out, size_t n) {
        size_t need = scan_i64_temp_bytes(n);
        d_scantmp.resize(need + 16, stream);
        KTN_HIP(exclusive_scan_i64(d_scantmp.p, need, in, out, n, stream));
    }

    NlpDev nlp_view();
    SweepOut sweep_view();
    LpRows lp_view();
    // device side of ktn_lp_pack_rows_dev / ktn_lp_append_packed_dev (the cut exchange that stays in device memory)
    void pack_rows_launch(int64_t nr, int64_t nz, int64_t first_row, int64_t base, bool ids, int64_t id_offset, double* dev_out);
    void unpack_rows_launch(int64_t nrows, int64_t nnz, const double* dev_in);

    // ================================================================ loadproblem ===
    void loadproblem(int64_t num_var, int64_t num_constr, const double* l_var, const double* u_var,
                     const double* l_constr, const double* u_constr, int32_t sense_, const ktn_nlp_desc* d);
    // its stages, in the order they run (load.hip); LoadScratch: what one stage leaves for the next and nobody needs after the load
    void load_constraint_rows(const ktn_nlp_desc* d, LoadScratch& S);
    void load_epigraph_row(const ktn_nlp_desc* d, LoadScratch& S);
    void load_host_rows(const ktn_nlp_desc* d);
    void load_tape_nodes(const ktn_nlp_desc* d, LoadScratch& S);
    void load_rows_and_box(const double* l_var, const double* u_var, const double* l_constr, const double* u_constr,
                           const ktn_nlp_desc* d, LoadScratch& S);
    void load_upload_nlp(LoadScratch& S);
    void load_blocked_copy(const LoadScratch& S);
    void load_long_rows(const LoadScratch& S);
    void load_batched_copy(const LoadScratch& S);
    void load_sweep_form(const LoadScratch& S);
    void load_sweep_buffers();
    void load_linear_rows(LoadScratch& S);
    void load_objective(LoadScratch& S);
    void load_lp(const LoadScratch& S);
    void reset();

    // ================================================================ separator =====
    // precompute! for every row of the extended structure (jac materialised)
    void precompute_all(const double* d_x);

    // the batched {isconstrsat, gencut, round_coefs, _addcut} over the NL rows
    void sweep(const double* d_x, double f_tol, int64_t* nviol_out, double* maxviol_out, bool* nonfinite_out);
    // sweep + (row-sharded) the stop rule's quantities over all ranks: number of violated rows, largest violation, error flag
    void global_sweep(const double* d_x, double f_tol, int64_t* nviol, double* maxviol, bool* nonfinite);
    double sweep_bytes = 0.0;
    // very long separable rows (kernels.hpp k_sep_eval_long): all of them / those among the NL rows, with their NL slot
    DBuf<int32_t> d_longev_rows, d_longev_nlrows;
    DBuf<int64_t> d_longev_slots, d_longev_nlslots;
    int64_t n_longev = 0, n_longev_nl = 0;
    // batch-blocked sweep for many short rows (kernels.hpp k_sep_sweep_batch): the regrouped copy of the NL entries
    bool sb_on = false;
    int64_t sb_batches = 0;
    int sb_nb = 0;
    bool sb_lds_set = false;
    DBuf<uint16_t> d_sbck, d_sbrow;
    DBuf<double2> d_sbpp;
    DBuf<int64_t> d_sbseg;

    // ================================================================ supporting hyperplanes (esh.hip) ===
    // cut_algo == KTN_CUT_SUPPORTING or KTN_CUT_SUPPORTING_QUAD: every selected violated row that participates
    // is cut at the point x_int + lambda_i (x* - x_int) where it reaches its bound.  Participating: separable or tape program -- under
    // KTN_CUT_SUPPORTING_QUAD also a KTN_ROW_QUAD row not declared linear --, exactly one finite side, not the epigraph row
    // (h_esh_side: +1 upper side, -1 lower side, 0 not participating), and g_i(x_int) at least 10 f_tol inside its bound (d_esh_sig:
    // the side, or 0).
    bool esh_mode() const { return prm.cut_algo == KTN_CUT_SUPPORTING || prm.cut_algo == KTN_CUT_SUPPORTING_QUAD; }
    bool esh_quad_mode() const { return prm.cut_algo == KTN_CUT_SUPPORTING_QUAD; }
    int esh_quad_group() const {                // lanes per row of k_esh_quad
        const int g = dev.esh_quad_group;
        return (g == 4 || g == 8 || g == 16 || g == 32 || g == 64) ? g : grp_quad_rows;
    }
    std::vector<int8_t> h_esh_side;
    DBuf<int8_t> d_esh_sig;
    DBuf<double> d_xint, d_lam;
    DBuf<double> d_jint;                       // Jacobian at x_int by Jacobian entry (k_esh_quad, k_emit_esh); only with taking-part QUAD rows
    int64_t esh_n_quad_part = 0;               // taking-part QUAD rows (0 unless KTN_CUT_SUPPORTING_QUAD)
    DBuf<int32_t> d_tape_nlslots;              // NL slot of each tape NL row (d_taperows_nl)
    DBuf<unsigned long long> d_esh_cnt;         // [0] rows cut at x_b, [1] Newton / bisection passes, [2] QUAD rows among [0]
    std::vector<double> h_xint;                 // the point in use (n0 entries)
    bool xint_given = false, esh_ready = false;
    int xint_found = 0;
    int64_t esh_n_part = 0;
    // the auxiliary min-max problem (variables (x, s), min s, participating rows g_i(x) -+ s against their bound), built at load
    struct EshAux {
        int64_t n = 0, m = 0;
        std::vector<double> lv, uv, lc, uc, rconst, p0, p1, targ, op0, op1;
        std::vector<int64_t> rows;                               // the caller's row of every auxiliary row
        std::vector<int64_t> rowptr, tptr, qptr;                 // qptr [entries + 1]: Q segments of the QUAD rows, empty for the others
        std::vector<int32_t> col, top, ocol, qcol;
        std::vector<double> qval;
        std::vector<uint8_t> kind, lin, akind, okind;
        bool has_tape = false, has_quad = false;
    } aux;
    Engine* child = nullptr;
    void esh_build_aux(const double* l_var, const double* u_var, const double* l_constr, const double* u_constr, const ktn_nlp_desc* d);
    void esh_prepare();                         // find (or take) x_int and evaluate the rows there, once per loaded problem
    void esh_find_interior();
    // root search of the selected violated rows (after the deepest-cut selection, before k_compact) and the cut emission
    bool esh_on = false;                        // this sweep's search ran (its cuts go through k_emit_esh)
    int64_t esh_last_rows = 0;
    void esh_search(const double* d_x, double f_tol);
    void esh_emit(const double* d_x, int64_t V);
    // ktn_sep_gencut for one row at the point of the last precompute
    DBuf<int32_t> d_esh_one;
    DBuf<int64_t> d_esh_slot;
    bool esh_gencut_row(int64_t i, double* coefs, double* constant);
    void esh_last_lambdas(double* out);

    // ================================================================ KKT report (kkt.hpp) ===
    // Constraint duals in the caller's row order, reduced costs and the dual bound, computed on the first getter after a solve and
    // kept until the LP is solved again or its rows change.  kkt_solved: an LP solve (or a device launch of the batch loop:
    // kkt_arena, the multipliers and lists are then the arenas') has run since the caller last appended, truncated or purged rows.
    bool kkt_solved = false, kkt_arena = false, kkt_cached = false, kkt_mirror = false, kkt_seg_ok = false;
    uint64_t kkt_solves = 0, kkt_key_version = 0, kkt_key_solves = 0;
    DBuf<int32_t> d_kkt_rowmap;                  // [m0] position among the linear rows (= LP row), or -1 - NL slot; built at load
    int64_t kkt_n_lin = 0;
    // column mirror of the extended NLP structure, built on first use per loaded problem: 8 (n0 + 2) + (4 + 4) nnz_ext bytes
    DBuf<int64_t> d_kkt_cptr, d_kkt_seg, d_kkt_browptr;
    DBuf<int32_t> d_kkt_crow, d_kkt_nonfin, d_kkt_brows;
    std::vector<int64_t> h_kkt_seg;              // six offsets per instance (k_dual_bound); with them the caller rows of each instance
    void kkt_build_seg();                        // once per ktn_set_blocks (kkt_seg_ok); refuses rows that are not grouped by instance
    DBuf<uint32_t> d_kkt_cperm;
    DBuf<double> d_kkt_x, d_kkt_g, d_kkt_jac, d_kkt_bconst, d_kkt_maxc, d_kkt_d, d_kkt_z, d_kkt_t, d_kkt_out, d_kkt_blk;
    std::vector<double> h_kkt_d, h_kkt_z, h_kkt_blk;      // results on the host; h_kkt_blk: (bound, gap) per instance of a fused batch
    double kkt_bound = 0.0, kkt_gap = 0.0;
    bool kkt_foreign() const { return row_sharded() || dist.cb != nullptr || dist.comm != nullptr || dist.ipc.data != nullptr || exchanging(); }
    void kkt_build_mirror();
    void kkt_compute();
    void kkt_blocks();

    // ================================================================ feasible point (feas.hpp, feas.hip) ===
    // x_feas on the segment from the reference point x_in to x* = lp_x, and what it certifies; computed on the first
    // ktn_get_feasible_point after a solve and kept until the LP is solved again, its rows change or the interior point is set.
    // Answers while the KKT report would (kkt_solved).  The taking-part rows are found once per loaded problem (feas_sides_ok),
    // under every cut_algo.
    bool feas_cached = false, feas_blk_cached = false, feas_sides_ok = false;
    uint64_t feas_key_version = 0, feas_key_solves = 0, feas_blk_key_version = 0, feas_blk_key_solves = 0;
    int64_t feas_n_part = 0, feas_two_sided = -1;       // feas_two_sided: the first nonlinear row with two finite sides, or -1
    DBuf<int8_t> d_feas_sig;
    DBuf<int32_t> d_feas_tslots, d_feas_nonfin, d_feas_unc;
    DBuf<double> d_feas_xin, d_feas_xs, d_feas_x, d_feas_g0, d_feas_j0, d_feas_g1, d_feas_j1, d_feas_bconst, d_feas_maxc, d_feas_lam,
                 d_feas_part, d_feas_res, d_feas_out, d_feas_shrink;
    DBuf<unsigned long long> d_feas_cnt;
    std::vector<double> h_feas_x, h_feas_lam;           // x_feas [n0] (NaN unless found == 1); lambda_i by caller row (1: not taking part)
    double feas_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // KTN_FEAS_INFO_LEN
    std::vector<double> h_feas_blk_x, h_feas_blk_info;  // the blocks form: x_feas [n0] with NaN segments, info [8 per instance]
    void feas_sides();
    void feas_eval(const double* d_x, DBuf<double>& g, DBuf<double>& jac);      // precompute_all into the feature's own buffers
    void feas_run(bool blocks);
    void feas_compute() { feas_run(false); }
    void feas_blocks() { feas_run(true); }

    // ================================================================ re-solve from the kept pool (rebound.hpp, rebound.hip) ===
    // ktn_set_var_bounds / ktn_set_linear_objective change the box or the linear cost in place and re-open the run state; every
    // row of the pool stays.  After a change of bounds the next begin() screens the pool once: a row whose smallest (largest)
    // value over the new box lies beyond its upper (lower) bound, or a crossed column, ends the solve :Infeasible without an LP.
    bool obj_settable = false;        // the loaded objective is a linear row the cost setter can rewrite (SEP of LIN atoms, or QUAD without Q)
    bool screen_pending = false;      // bounds were set since the last begin()
    bool screened_out = false;        // that begin()'s screen proved the box infeasible: step() reports done
    bool reopened = false;            // a setter ran since the last reset(): ktn_optimize_blocks[_ex] starts from the loaded rows
    int64_t crossed_cols = 0;         // columns with l_j > u_j at the last ktn_set_var_bounds
    DBuf<double> d_act_min, d_act_max;
    DBuf<unsigned long long> d_act_cnt;
    hipEvent_t ev_screen[2] = {nullptr, nullptr};
    void reopen();                    // reset() without the items that make up the pool
    void set_var_bounds(const double* l, const double* u, int64_t n);
    void set_linear_objective(const double* c, int64_t n, double c0_new);
    // ktn_set_row_bounds: new constraint bounds in place.  Linear rows: their LP rows again from the tangent at the origin; NL rows:
    // every cut of the row's list shifted by the change (k_rebase_cuts), in the pool and -- with a device launch standing -- in the
    // resident arenas (k_blocks_rebase).  Every copy of the row bounds follows: h_lb / h_ub, d_lb / d_ub, d_slots, aux.lc / aux.uc.
    int64_t crossed_rows = 0;         // caller's rows with lb_i > ub_i at the last ktn_set_row_bounds
    DBuf<double> d_lb_new, d_ub_new;
    hipEvent_t ev_rebase[4] = {nullptr, nullptr, nullptr, nullptr};     // k_rebase_cuts begin / end, k_blocks_rebase begin / end
    void set_row_bounds(const double* lb, const double* ub, int64_t m);
    void blocks_rebase(unsigned long long* cnt, hipEvent_t e0, hipEvent_t e1);     // ecp.hip: k_blocks_rebase, old bounds in d_lb / d_ub, new in d_lb_new / d_ub_new
    void row_owners(int64_t* owner_out);      // ktn_lp_get_row_owners: M entries
    void row_activity(hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);      // k_row_activity over the current rows and bounds, into d_act_*
    bool screen();                    // true: the box is empty or contradicts a row

    // ================================================================ LP ============
    void rebuild_csc();
    void purge_cuts();
    // Capacity for the cut pool up front: growing a buffer is hipMalloc + copy + hipFree (which synchronises the device),
    // and on a large instance the pool passes through a dozen sizes in the first iterations (cfg4: 2.5 of the 4.9 s of a
    // cold solve).  HBM is plentiful (288 GB): reserve for three sweeps' worth of cuts.
    void reserve_lp(int64_t rows, int64_t nnz);
    void find_long_rows();
    bool recession_ray_dense(bool* unbounded);
    void launch_y(const SpMat& A, double sigma, double w, double rho, hipEvent_t e0, hipEvent_t e1);
    void launch_x(const SpMat& AT, double tau, double w, double rho, bool update, hipEvent_t e0, hipEvent_t e1);
    void pdhg_iteration(const SpMat& A, const SpMat& AT, double tau, double sigma, double w, double rho);
    // w_next >= 0: the check kernels also write the Halpern update of this iteration into xnext / ynext (returns true when they did:
    // the plain CSR form only); the caller swaps them in for x / y instead of launching k_halpern2
    bool launch_check(const SpMat& A, const SpMat& AT, double tau, double sigma, double w_next = -1.0, double rho = 1.0);
    DBuf<double> xnext, ynext;
    int chk_nrow = 0, chk_ncol = 0;     // partial blocks of the last check (rows | columns)
    void compute_scaling(bool identity);
    LpResult lp_solve(double tol_p, double tol_g, int mode, bool identity_scaling = false);
    LpResult lp_solve_core(double tol_p, double tol_g, int mode, bool identity_scaling);
    bool lp_solve_dense(LpResult* R);
    bool big_bounds_hold();            // lp_x respects the finite bounds beyond kDenseBig that the exact paths left out
    bool lp_solve_mid(LpResult* R);
    void pdhg_raw(const double* x0, const double* y0, double eta, double omega_, int64_t iters, double* x_out,
                  double* y_out);
    // pieces of lp_solve_core that the scripted test hook shares with it (lp.hip)
    void lp_resize_iterates();
    void lp_pick_groups();
    void lp_choose_tiled(bool same_matrix);
    void lp_set_anchors(bool want_packed);
    void lp_read_check(double* q);
    void lp_restart();
    void lp_advance(bool spec, int64_t k, double rho);
    struct LpScriptIO {
        const double *x, *y, *x0, *y0;
        double eta, omega;
        int64_t k;
        int32_t flags;
        const int32_t* ops;
        int64_t nops;
        double *x_out, *y_out, *x0_out, *y0_out, *xt_out, *yt_out, *q_out, *xnext_out, *ynext_out;
        int32_t* spec_out;
        double *dr_out, *dc_out;
    };
    void lp_script(const LpScriptIO& io);
    void lp_scaling(double* dr_out, double* dc_out, double* drr_out, double* dcr_out);

    // ================================================================ ECP driver ====
    bool recession_ray();
    void boundroutine();
    void begin();
    void step(int32_t* done);
    void polish_step(int32_t* done);
    void end();
};

}  // namespace ktn
