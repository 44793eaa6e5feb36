// pdhg_check.hpp -- what a check iteration of the restarted reflected-Halpern PDHG decides, written once.  The host loop
// (Engine::lp_solve_core) and the device-side cutting-plane loop (k_ecp_blocks) hand it the reduced sums of the check and act on
// what it returns; k_pdhg_blocks keeps a text of its own that must follow it (batch_lp.hpp says why).  What differs between the
// three loops is a field of PdhgRules (DESIGN.md section 5 has the rule text and the table).  Plain C++17 without HIP:
// tests/c/pdhg_rules.cpp runs it on a CPU.
//
// Two functions, because the host's infeasibility certificate sits between them: pdhg_stop (is the LP solved, by which exit)
// and pdhg_next (advance, restart or consolidate; the new primal weight and step size).
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define KTN_HD __host__ __device__
#else
#define KTN_HD
#endif

namespace ktn {

// the reduced quantities of one check (T(z) = (xt, yt), dx = xt - x, dx0 = xt - x0, rows likewise)
struct PdhgSums {
    double dyAdx, dy2, dy0sq, dx2, dx0sq, xt2, yt2;
    double pobj, dobj;          // primal and dual objective
    double pviol, dres;         // largest unscaled row violation / dual residual
};

struct PdhgRules {
    double tol_p, tol_g;
    double dres_scale;          // the dual residual is judged against tol_g * dres_scale
    double stag_factor;         // primal-stagnation and stalled-row exits: gap certified to stag_factor * tol_g; 0: neither exit
    double flat_factor;         // "flat": the objective within flat_factor * tol_g (1 + |pobj|) of its last flat_checks values
    int flat_checks;            // 2 or 3
    double stall_accept;        // a row violation on a plateau is accepted up to stall_accept * tol_p
    double eta_safe;            // the step size the back-offs shrink towards
    bool nan_exit;              // give up on a NaN residual
    bool grow_backoff;          // also back off when the residual grows check after check
    bool consolidate;           // report PDHG_CONSOLIDATE when multiplier mass idles between cuts (at most 8 times)
    double omega_ref;           // the weight stays within 1e-3 .. 1e3 of it
    // weight update on a restart the residual did not earn (r > 0.8 r0); the plain update is {true, 0, 0, 0, 0}
    bool om_art;                // false: no update at all on such a restart
    double om_art_k;            // > 0: theta = 0.5 min(1, k / om_art_k) instead of 0.5
    double om_art_clamp;        // > 1: at most this factor per such restart
    double om_clamp;            // > 1: at most this factor per restart (any)
    double om_clamp_down;       // > 1: at most this factor downwards per restart (any)
};

// carried from check to check; k_ecp_blocks keeps it in the 16 doubles of LDS it calls st[]
struct PdhgCtl {
    double r0, r_prev, r_last;          // residual at the restart, at the previous check, ditto (0 after a consolidation)
    double pobj_h[3], pviol_h[3];       // newest first
    int stall, grow, flat_rows, consolidations;
};
// the state a solve starts with
KTN_HD inline PdhgCtl pdhg_start() { return PdhgCtl{0.0, 0.0, 0.0, {1e300, -1e300, 1e300}, {1e300, -1e300, 1e300}, 0, 0, 0, 0}; }
static_assert(sizeof(PdhgCtl) <= 16 * sizeof(double), "PdhgCtl must fit k_ecp_blocks' st[]");

enum PdhgExit : int { PDHG_EXIT_NONE = 0, PDHG_EXIT_CONVERGED, PDHG_EXIT_STAGNATION, PDHG_EXIT_STALLED_ROW, PDHG_EXIT_NAN };
enum PdhgAction : int { PDHG_ADVANCE = 0, PDHG_RESTART, PDHG_CONSOLIDATE };
enum PdhgBackoff : int { PDHG_BACKOFF_NONE = 0, PDHG_BACKOFF_FLAT, PDHG_BACKOFF_NEG_R2, PDHG_BACKOFF_GROW };

struct PdhgStop {
    double r2, r, gap;          // squared fixed-point residual in the M-norm, its root (0 for r2 < 0), relative duality gap
    bool dres_ok, near, primal_ok;
    PdhgExit exit;
};
struct PdhgNext {
    PdhgAction action;
    double om, eta;
    PdhgBackoff backoff;
};

// (fmin / fmax: a NaN operand is dropped, as in the device loops before this header; the NaN exit therefore tests r2, not r)
KTN_HD inline double pdhg_min(double a, double b) { return std::fmin(a, b); }
KTN_HD inline double pdhg_max(double a, double b) { return std::fmax(a, b); }
KTN_HD inline double pdhg_clamp(double v, double lo, double hi) { return pdhg_min(pdhg_max(v, lo), hi); }

// Termination.  k: Halpern counter (0: the first check after a restart, which sets r0).  Shifts the histories.
KTN_HD inline PdhgStop pdhg_stop(const PdhgSums& s, const PdhgRules& R, PdhgCtl& c, double om, double eta, long long k) {
    PdhgStop t;
    t.r2 = om / eta * s.dx2 - 2.0 * s.dyAdx + s.dy2 / (eta * om);
    t.r = std::sqrt(pdhg_max(t.r2, 0.0));
    t.gap = std::fabs(s.pobj - s.dobj) / (1.0 + std::fabs(s.pobj) + std::fabs(s.dobj));
    if (k == 0) { c.r0 = t.r; c.r_prev = t.r; }
    const double pviol = s.pviol;
    t.dres_ok = s.dres <= R.tol_g * R.dres_scale;
    t.exit = ((pviol <= R.tol_p) && (t.gap <= R.tol_g) && t.dres_ok) ? PDHG_EXIT_CONVERGED : PDHG_EXIT_NONE;
    t.near = (pviol <= 4.0 * R.tol_p) && (t.gap <= 4.0 * R.tol_g) && (s.dres <= 4.0 * R.tol_g * R.dres_scale);
    t.primal_ok = (pviol <= R.tol_p) && t.dres_ok;
    if (R.stag_factor > 0.0 && t.exit == PDHG_EXIT_NONE) {
        // primal-stagnation exit: rows feasible, dual residual converged, objective flat, gap certified to stag_factor tol_g
        const double f = R.flat_factor * R.tol_g * (1.0 + std::fabs(s.pobj));
        const bool flat = std::fabs(s.pobj - c.pobj_h[0]) <= f && std::fabs(s.pobj - c.pobj_h[1]) <= f &&
                          (R.flat_checks < 3 || std::fabs(s.pobj - c.pobj_h[2]) <= f);
        // a row violation unchanged to 2 % over three checks, within the stalled-row allowance, counts as feasible
        const bool plateau = pviol <= R.stall_accept * R.tol_p && std::fabs(pviol - c.pviol_h[0]) <= 0.02 * pviol &&
                             std::fabs(pviol - c.pviol_h[1]) <= 0.02 * pviol && std::fabs(pviol - c.pviol_h[2]) <= 0.02 * pviol;
        if (flat && (pviol <= R.tol_p || plateau) && t.gap <= R.stag_factor * R.tol_g && t.dres_ok) t.exit = PDHG_EXIT_STAGNATION;
        // stalled-row exit: objective, gap and dual residual converged, one row sits a hair above tol_p
        else if (t.gap <= R.tol_g && t.dres_ok && plateau) t.exit = PDHG_EXIT_STALLED_ROW;
    }
    c.pviol_h[2] = c.pviol_h[1]; c.pviol_h[1] = c.pviol_h[0]; c.pviol_h[0] = pviol;
    c.pobj_h[2] = c.pobj_h[1]; c.pobj_h[1] = c.pobj_h[0]; c.pobj_h[0] = s.pobj;
    if (R.nan_exit && t.exit == PDHG_EXIT_NONE && !(t.r2 == t.r2)) t.exit = PDHG_EXIT_NAN;
    return t;
}

// What follows a check that did not end the solve.  it: PDHG iterations before this check.
KTN_HD inline PdhgNext pdhg_next(const PdhgSums& s, const PdhgRules& R, PdhgCtl& c, const PdhgStop& t, double om, double eta,
                                 long long k, long long it) {
    PdhgNext n{PDHG_ADVANCE, om, eta, PDHG_BACKOFF_NONE};
    const double r = t.r;
    // the three restart rules: sufficient decay, necessary decay without progress, a period as long as 0.36 of the solve
    bool restart = k > 0 && (r <= 0.2 * c.r0 || (r <= 0.8 * c.r0 && r > c.r_prev) || (double)k >= 0.36 * (double)(it + 1));
    const bool decayed = r <= 0.8 * c.r0;               // a restart the residual earned
    // step-size safeguard: a residual that no longer moves (or a negative M-norm) means eta * sigma_max > 1; so does one that
    // grows check after check far above the residual the period started with
    if (k > 0 && eta > R.eta_safe * (1.0 + 1e-12)) {
        c.stall = (t.r2 < 0.0 || (c.r_last > 0.0 && r > 0.97 * c.r_last && r < 1.03 * c.r_last)) ? c.stall + 1 : 0;
        if (R.grow_backoff) c.grow = (r > 5.0 * c.r0 && c.r_last > 0.0 && r > c.r_last) ? c.grow + 1 : 0;
        if (c.stall >= 3 || t.r2 < 0.0 || c.grow >= 2) {
            n.eta = pdhg_max(R.eta_safe, 0.85 * eta);
            n.backoff = c.grow >= 2 ? PDHG_BACKOFF_GROW : (t.r2 < 0.0 ? PDHG_BACKOFF_NEG_R2 : PDHG_BACKOFF_FLAT);
            c.stall = 0; c.grow = 0;
            restart = true;
        }
    }
    // objective converged, rows not, residual flat: multiplier mass idles between near-parallel cuts of one NL row
    bool consolidate = false;
    if (R.consolidate && k > 0 && t.gap <= R.tol_g && t.dres_ok && s.pviol > R.tol_p) {
        c.flat_rows = (c.r_last > 0.0 && r > 0.98 * c.r_last) ? c.flat_rows + 1 : 0;
        if (c.flat_rows >= 3 && c.consolidations < 8) { c.flat_rows = 0; ++c.consolidations; consolidate = true; }
    } else {
        c.flat_rows = 0;
    }
    c.r_last = consolidate ? 0.0 : r;                   // (a consolidation restarts with k = 0: the next check sets r0 and r_prev)
    c.r_prev = r;
    if (consolidate) n.action = PDHG_CONSOLIDATE;
    else if (restart) {
        n.action = PDHG_RESTART;
        // guarded primal-weight update: geometric mean of the weight and the ratio of the movements since the last restart
        const double dx = std::sqrt(s.dx0sq), dy = std::sqrt(s.dy0sq);
        if ((R.om_art || decayed) && dx > 1e-8 * (1.0 + std::sqrt(s.xt2)) && dy > 1e-8 * (1.0 + std::sqrt(s.yt2))) {
            const double theta = (!decayed && R.om_art_k > 0.0) ? 0.5 * pdhg_min(1.0, (double)k / R.om_art_k) : 0.5;
            double w = std::exp(theta * std::log(dy / dx) + (1.0 - theta) * std::log(om));
            if (!decayed && R.om_art_clamp > 1.0) w = pdhg_clamp(w, om / R.om_art_clamp, om * R.om_art_clamp);
            if (R.om_clamp > 1.0) w = pdhg_clamp(w, om / R.om_clamp, om * R.om_clamp);
            if (R.om_clamp_down > 1.0) w = pdhg_max(w, om / R.om_clamp_down);
            n.om = pdhg_clamp(w, R.omega_ref * 1e-3, R.omega_ref * 1e3);
        }
    }
    return n;
}

}  // namespace ktn
