// pdhg_rules.cpp -- scripted checks for csrc/pdhg_check.hpp (pdhg_stop / pdhg_next), run on a CPU by tests/test_pdhg_rules.py.
// Every sequence is written so that one rule fires; the expected exits, actions and values below are worked out by hand from
// the rule text of DESIGN.md section 5 ("The check, stated once") and written as literals.
//
// Conventions: tol_p = tol_g = 1e-4, dual-residual scale 2, omega_ref = 1.  sums(r, ...) builds a check whose fixed-point
// residual is r for the given (om, eta): Dy.ADx = |Dy|^2 = 0, |Dx|^2 = r^2 eta / om.  The movements since the restart are 0
// unless a case sets them, so the weight is only updated where a case is about the weight.
#include <cmath>
#include <cstdio>
#include <string>

#include "pdhg_check.hpp"

using namespace ktn;

static PdhgRules host_rules() {
    PdhgRules R{};
    R.tol_p = 1e-4; R.tol_g = 1e-4; R.dres_scale = 2.0;
    R.stag_factor = 20.0; R.flat_factor = 0.4; R.flat_checks = 2; R.stall_accept = 3.0;
    R.eta_safe = 0.5; R.nan_exit = true; R.grow_backoff = true; R.consolidate = true;
    R.omega_ref = 1.0; R.om_art = true; R.om_art_k = 0.0; R.om_art_clamp = 0.0; R.om_clamp = 0.0; R.om_clamp_down = 0.0;
    return R;
}
// what k_pdhg_blocks and k_ecp_blocks pass (k_ecp_blocks with consolidate = true once it has cuts)
static PdhgRules device_rules() {
    PdhgRules R = host_rules();
    R.flat_factor = 0.1; R.flat_checks = 3; R.eta_safe = 0.998; R.nan_exit = false; R.grow_backoff = false; R.consolidate = false;
    return R;
}

struct Pt { double om = 1.0, eta = 1.0; };
static PdhgSums sums(double r, const Pt& p, double pobj, double dobj, double pviol, double dres) {
    PdhgSums s{};
    s.dx2 = r * r * p.eta / p.om;
    s.pobj = pobj; s.dobj = dobj; s.pviol = pviol; s.dres = dres;
    return s;
}
// a check that is far from every exit: gap 0.5, row violation 1
static PdhgSums far(double r, const Pt& p) { return sums(r, p, 1.0, 0.0, 1.0, 0.0); }

static int g_fail = 0;
static std::string g_case;
static bool g_case_ok = true;
static void begin(const char* name) { g_case = name; g_case_ok = true; }
static void end() {
    std::printf("case %s %s\n", g_case.c_str(), g_case_ok ? "ok" : "FAILED");
    if (!g_case_ok) ++g_fail;
}
#define EXPECT(cond) \
    do { if (!(cond)) { g_case_ok = false; std::printf("  %s: line %d: %s\n", g_case.c_str(), __LINE__, #cond); } } while (0)
static bool close_to(double a, double b) { return std::fabs(a - b) <= 1e-12 * std::fabs(b); }

struct Out { PdhgStop t; PdhgNext n; };
// one check as the callers run it: pdhg_next only when no exit fired; om and eta follow the decision
static Out check(const PdhgRules& R, PdhgCtl& c, Pt& p, const PdhgSums& s, long long k, long long it) {
    Out o{};
    o.t = pdhg_stop(s, R, c, p.om, p.eta, k);
    o.n = PdhgNext{PDHG_ADVANCE, p.om, p.eta, PDHG_BACKOFF_NONE};
    if (o.t.exit == PDHG_EXIT_NONE) { o.n = pdhg_next(s, R, c, o.t, p.om, p.eta, k, it); p.om = o.n.om; p.eta = o.n.eta; }
    return o;
}

// ---- termination ---------------------------------------------------------------------------------------------------------
static void convergence(const char* name, const PdhgRules& R) {
    begin(name);
    Pt p;
    { PdhgCtl c = pdhg_start(); const PdhgStop t = pdhg_stop(sums(1.0, p, 1.0, 1.0, 5e-5, 1.5e-4), R, c, 1.0, 1.0, 0);
      EXPECT(t.exit == PDHG_EXIT_CONVERGED); EXPECT(t.near); EXPECT(t.primal_ok); EXPECT(t.gap == 0.0); EXPECT(t.r == 1.0); EXPECT(c.r0 == 1.0); }
    // each of the three conditions alone keeps the solve going: row violation 1.1 tol_p; dual residual 2.1 tol_g against a scale of
    // 2; gap 0.001 / 2.999 = 3.3e-4.  All of them are within 4 tolerances: "near"
    { PdhgCtl c = pdhg_start(); const PdhgStop t = pdhg_stop(sums(1.0, p, 1.0, 1.0, 1.1e-4, 1.5e-4), R, c, 1.0, 1.0, 0);
      EXPECT(t.exit == PDHG_EXIT_NONE); EXPECT(t.near); EXPECT(!t.primal_ok); }
    { PdhgCtl c = pdhg_start(); const PdhgStop t = pdhg_stop(sums(1.0, p, 1.0, 1.0, 5e-5, 2.1e-4), R, c, 1.0, 1.0, 0);
      EXPECT(t.exit == PDHG_EXIT_NONE); EXPECT(t.near); EXPECT(!t.primal_ok); EXPECT(!t.dres_ok); }
    { PdhgCtl c = pdhg_start(); const PdhgStop t = pdhg_stop(sums(1.0, p, 1.0, 0.999, 5e-5, 1.5e-4), R, c, 1.0, 1.0, 0);
      EXPECT(t.exit == PDHG_EXIT_NONE); EXPECT(t.near); EXPECT(t.primal_ok); EXPECT(t.gap > 3.3e-4 && t.gap < 3.4e-4); }
    // a row violation of 5 tol_p is not near
    { PdhgCtl c = pdhg_start(); const PdhgStop t = pdhg_stop(sums(1.0, p, 1.0, 1.0, 5e-4, 1.5e-4), R, c, 1.0, 1.0, 0);
      EXPECT(t.exit == PDHG_EXIT_NONE); EXPECT(!t.near); }
    end();
}

// Primal-stagnation exit.  Rows feasible (0.5 tol_p), dual residual 0, dual objective 0.999, primal objective 1, 1.00005, 1.00006,
// 1.00006, 1.00006: the gap stays near 3.5e-4 (above tol_g, below 20 tol_g).  Host window: 0.4 tol_g (1 + |p|) = 8e-5 over two
// checks -- the third check is within 1e-5 and 6e-5 of the two before it and leaves.  Device window: 0.1 -> 2e-5 over three checks
// -- 6e-5 from the first value is too far until that value has left the history: the fifth check leaves.
static void stagnation(const char* name, const PdhgRules& R, int leaves_at) {
    begin(name);
    const double pobj[5] = {1.0, 1.00005, 1.00006, 1.00006, 1.00006};
    PdhgCtl c = pdhg_start();
    Pt p;
    int left = 0;
    for (int i = 0; i < 5 && !left; ++i) {
        const PdhgStop t = pdhg_stop(sums(1.0, p, pobj[i], 0.999, 5e-5, 0.0), R, c, 1.0, 1.0, 32 * i);
        EXPECT(t.exit == PDHG_EXIT_NONE || t.exit == PDHG_EXIT_STAGNATION);
        if (t.exit == PDHG_EXIT_STAGNATION) left = i + 1;
    }
    EXPECT(left == leaves_at);
    // a gap certificate of 3 tol_g is not met by a gap of 3.5 tol_g: no exit at all
    PdhgRules R3 = R; R3.stag_factor = 3.0;
    c = pdhg_start();
    for (int i = 0; i < 5; ++i) EXPECT(pdhg_stop(sums(1.0, p, pobj[i], 0.999, 5e-5, 0.0), R3, c, 1.0, 1.0, 32 * i).exit == PDHG_EXIT_NONE);
    // ... and stag_factor = 0 switches the exit off
    R3.stag_factor = 0.0;
    c = pdhg_start();
    for (int i = 0; i < 5; ++i) EXPECT(pdhg_stop(sums(1.0, p, pobj[i], 0.999, 5e-5, 0.0), R3, c, 1.0, 1.0, 32 * i).exit == PDHG_EXIT_NONE);
    end();
}

// Stalled-row exit.  Gap 0 (the dual objective follows the primal), dual residual 0, the objective jumping by 1e-3 (never flat, so
// the stagnation exit cannot fire), the row violation `scale` times 2.5, 2.52, 2.49, 2.5 tol_p: a plateau at the fourth check.
static PdhgExit stalled_run(const PdhgRules& R, double scale, double last = 2.5e-4) {
    const double pv[4] = {2.5e-4, 2.52e-4, 2.49e-4, last}, pobj[4] = {1.0, 1.001, 1.0, 1.001};
    PdhgCtl c = pdhg_start();
    Pt p;
    PdhgExit e = PDHG_EXIT_NONE;
    for (int i = 0; i < 4; ++i) {
        e = pdhg_stop(sums(1.0, p, pobj[i], pobj[i], scale * pv[i], 0.0), R, c, 1.0, 1.0, 32 * i).exit;
        if (i < 3) EXPECT(e == PDHG_EXIT_NONE);
    }
    return e;
}
static void stalled_row(const char* name, PdhgRules R) {
    begin(name);
    R.stall_accept = 3.0;
    EXPECT(stalled_run(R, 1.0) == PDHG_EXIT_STALLED_ROW);      // 2.5 tol_p within the allowance of 3
    EXPECT(stalled_run(R, 2.0) == PDHG_EXIT_NONE);             // 5 tol_p is not
    EXPECT(stalled_run(R, 1.0, 2.6e-4) == PDHG_EXIT_NONE);     // 2.6 against 2.49 .. 2.52: more than 2 % of 2.6
    R.stall_accept = 10.0;
    EXPECT(stalled_run(R, 2.0) == PDHG_EXIT_STALLED_ROW);      // an intermediate solve accepts 5 tol_p
    EXPECT(stalled_run(R, 4.4) == PDHG_EXIT_NONE);             // 11 tol_p is beyond 10
    end();
}

static void nan_residual(const char* name, const PdhgRules& R, bool gives_up) {
    begin(name);
    PdhgCtl c = pdhg_start();
    Pt p; p.eta = R.eta_safe;
    EXPECT(check(R, c, p, far(10.0, p), 0, 0).n.action == PDHG_ADVANCE);
    PdhgSums s = far(10.0, p);
    s.dx2 = std::nan("");
    const Out o = check(R, c, p, s, 32, 1000);
    if (gives_up) EXPECT(o.t.exit == PDHG_EXIT_NAN);
    else {                                                        // the device loops take max(NaN, 0) = 0 for the residual: a restart
        EXPECT(o.t.exit == PDHG_EXIT_NONE); EXPECT(o.t.r == 0.0); EXPECT(o.n.action == PDHG_RESTART);
    }
    end();
}

// ---- restarts ------------------------------------------------------------------------------------------------------------
// every sequence starts with a check at k = 0 and r = r0, which sets r0 = r_prev = r and advances
static void start_period(const PdhgRules& R, PdhgCtl& c, Pt& p, double r0) {
    const Out o = check(R, c, p, far(r0, p), 0, 0);
    EXPECT(o.t.exit == PDHG_EXIT_NONE); EXPECT(o.n.action == PDHG_ADVANCE);
    EXPECT(close_to(c.r0, r0)); EXPECT(c.r_prev == c.r0); EXPECT(c.r_last == c.r0);
}
static PdhgNext one_after_start(const PdhgRules& R, double r0, double r, long long k, long long it) {
    PdhgCtl c = pdhg_start();
    Pt p;
    start_period(R, c, p, r0);
    return check(R, c, p, far(r, p), k, it).n;
}
static void restart_rules() {
    const PdhgRules R = host_rules();
    begin("restart_sufficient");       // r <= 0.2 r0; k = 32 of 1000 iterations keeps the artificial rule (k >= 360.36) away
    { const PdhgNext n = one_after_start(R, 10.0, 1.9, 32, 1000);
      EXPECT(n.action == PDHG_RESTART); EXPECT(n.backoff == PDHG_BACKOFF_NONE); EXPECT(n.om == 1.0); EXPECT(n.eta == 1.0); }
    EXPECT(one_after_start(R, 10.0, 2.1, 32, 1000).action == PDHG_ADVANCE);
    end();
    begin("restart_necessary");        // r <= 0.8 r0 and larger than at the previous check
    for (int pass = 0; pass < 2; ++pass) {
        PdhgCtl c = pdhg_start();
        Pt p;
        start_period(R, c, p, 10.0);
        EXPECT(check(R, c, p, far(5.0, p), 32, 1000).n.action == PDHG_ADVANCE);      // 5 <= 8, but below the 10 before it
        EXPECT(c.r_prev == 5.0);
        EXPECT(check(R, c, p, far(pass == 0 ? 6.0 : 4.9, p), 64, 1032).n.action == (pass == 0 ? PDHG_RESTART : PDHG_ADVANCE));
    }
    EXPECT(one_after_start(R, 10.0, 9.0, 32, 1000).action == PDHG_ADVANCE);          // 9 > 8: no decay at all
    end();
    begin("restart_artificial");       // k >= 0.36 (it + 1) = 36.36 with r = 9 of r0 = 10 (no decay; 9 is outside 10 +- 3 %)
    EXPECT(one_after_start(R, 10.0, 9.0, 37, 100).action == PDHG_RESTART);
    EXPECT(one_after_start(R, 10.0, 9.0, 36, 100).action == PDHG_ADVANCE);
    EXPECT(one_after_start(R, 10.0, 9.0, 37, 100).backoff == PDHG_BACKOFF_NONE);
    end();
}

// ---- step-size back-offs ---------------------------------------------------------------------------------------------------
static void backoffs() {
    const PdhgRules R = host_rules();
    begin("backoff_flat_residual");    // three checks in a row within 3 % of the one before: 10 -> 10.1 -> 10.0 -> 10.05
    for (int pass = 0; pass < 3; ++pass) {
        PdhgCtl c = pdhg_start();
        Pt p; p.eta = pass == 0 ? 1.0 : (pass == 1 ? 0.55 : 0.5);
        start_period(R, c, p, 10.0);
        Out o = check(R, c, p, far(10.1, p), 32, 1032);
        EXPECT(o.n.action == PDHG_ADVANCE); EXPECT(c.stall == (pass < 2 ? 1 : 0));
        o = check(R, c, p, far(10.0, p), 64, 1064);
        EXPECT(o.n.action == PDHG_ADVANCE); EXPECT(c.stall == (pass < 2 ? 2 : 0));
        o = check(R, c, p, far(10.05, p), 96, 1096);
        if (pass == 0) { EXPECT(o.n.action == PDHG_RESTART); EXPECT(o.n.backoff == PDHG_BACKOFF_FLAT); EXPECT(o.n.eta == 0.85); EXPECT(c.stall == 0); }
        if (pass == 1) { EXPECT(o.n.action == PDHG_RESTART); EXPECT(o.n.backoff == PDHG_BACKOFF_FLAT); EXPECT(o.n.eta == 0.5); }   // 0.85 * 0.55 < eta_safe
        if (pass == 2) { EXPECT(o.n.action == PDHG_ADVANCE); EXPECT(o.n.backoff == PDHG_BACKOFF_NONE); EXPECT(o.n.eta == 0.5); }   // already at eta_safe
        EXPECT(o.n.om == 1.0);
    }
    {   // a check outside the 3 % starts the count again: 10 -> 10.1 -> 10.0 -> 11 -> 11.1 -> 11.0
        PdhgCtl c = pdhg_start();
        Pt p;
        start_period(R, c, p, 10.0);
        const double r[5] = {10.1, 10.0, 11.0, 11.1, 11.0};
        const int stall[5] = {1, 2, 0, 1, 2};
        for (int i = 0; i < 5; ++i) {
            const Out o = check(R, c, p, far(r[i], p), 32 * (i + 1), 1000 + 32 * (i + 1));
            EXPECT(o.n.action == PDHG_ADVANCE); EXPECT(o.n.eta == 1.0); EXPECT(c.stall == stall[i]);
        }
    }
    end();
    begin("backoff_negative_r2");      // |Dx|^2 = 1, Dy.ADx = 1: r2 = 1 - 2 = -1 at om = eta = 1 -- at once, not after three
    {
        PdhgCtl c = pdhg_start();
        Pt p;
        start_period(R, c, p, 10.0);
        PdhgSums s = far(1.0, p);
        s.dyAdx = 1.0;
        const Out o = check(R, c, p, s, 32, 1000);
        EXPECT(o.t.r2 == -1.0); EXPECT(o.t.r == 0.0);
        EXPECT(o.n.action == PDHG_RESTART); EXPECT(o.n.backoff == PDHG_BACKOFF_NEG_R2); EXPECT(o.n.eta == 0.85);
    }
    end();
    begin("backoff_growing_residual"); // r0 = 1, then 6 and 7.5: above 5 r0 and growing, twice in a row
    for (int pass = 0; pass < 2; ++pass) {
        PdhgRules Rg = R; Rg.grow_backoff = pass == 0;
        PdhgCtl c = pdhg_start();
        Pt p;
        start_period(Rg, c, p, 1.0);
        Out o = check(Rg, c, p, far(6.0, p), 32, 1032);
        EXPECT(o.n.action == PDHG_ADVANCE); EXPECT(c.grow == (pass == 0 ? 1 : 0));
        o = check(Rg, c, p, far(7.5, p), 64, 1064);
        if (pass == 0) { EXPECT(o.n.action == PDHG_RESTART); EXPECT(o.n.backoff == PDHG_BACKOFF_GROW); EXPECT(o.n.eta == 0.85); EXPECT(c.grow == 0); }
        else { EXPECT(o.n.action == PDHG_ADVANCE); EXPECT(o.n.backoff == PDHG_BACKOFF_NONE); EXPECT(o.n.eta == 1.0); }   // the device loops have no such rule
    }
    end();
}

// ---- consolidation ---------------------------------------------------------------------------------------------------------
// gap 0, dual residual 0, a row at 20 tol_p (beyond every allowance: no exit), eta at eta_safe (no back-off), r = 10 at every check
static void consolidation() {
    const PdhgRules R = host_rules();
    begin("consolidation_trigger_and_cap");
    PdhgCtl c = pdhg_start();
    Pt p; p.eta = 0.5;
    const PdhgSums s = sums(10.0, p, 1.0, 1.0, 2e-3, 0.0);
    long long it = 0;
    for (int round = 1; round <= 9; ++round) {
        EXPECT(check(R, c, p, s, 0, it).n.action == PDHG_ADVANCE);                   // k = 0 does not count
        EXPECT(c.flat_rows == 0);
        for (int i = 1; i <= 3; ++i) {
            it += 1000;
            const Out o = check(R, c, p, s, 32 * i, it);
            EXPECT(o.t.exit == PDHG_EXIT_NONE);
            if (i < 3 || round == 9) { EXPECT(o.n.action == PDHG_ADVANCE); EXPECT(c.flat_rows == i); }
            else { EXPECT(o.n.action == PDHG_CONSOLIDATE); EXPECT(c.flat_rows == 0); EXPECT(c.r_last == 0.0); EXPECT(c.consolidations == round); }
            EXPECT(o.n.om == 1.0); EXPECT(o.n.eta == 0.5);
        }
    }
    EXPECT(c.consolidations == 8);
    end();
    begin("consolidation_needs_flat_residual");      // 10, 10, 10, then 9 (below 0.98 of 10): the count starts again
    {
        PdhgCtl c2 = pdhg_start();
        Pt q; q.eta = 0.5;
        const double r[5] = {10.0, 10.0, 10.0, 9.0, 9.0};
        const int flat[5] = {0, 1, 2, 0, 1};
        for (int i = 0; i < 5; ++i) {
            EXPECT(check(R, c2, q, sums(r[i], q, 1.0, 1.0, 2e-3, 0.0), 32 * i, 100000).n.action == PDHG_ADVANCE);
            EXPECT(c2.flat_rows == flat[i]);
        }
        // a loop without the rule (k_pdhg_blocks) never consolidates
        PdhgRules Rn = R; Rn.consolidate = false;
        c2 = pdhg_start();
        for (int i = 0; i < 6; ++i) EXPECT(check(Rn, c2, q, sums(10.0, q, 1.0, 1.0, 2e-3, 0.0), 32 * i, 100000).n.action == PDHG_ADVANCE);
        EXPECT(c2.consolidations == 0);
    }
    end();
}

// ---- primal weight ---------------------------------------------------------------------------------------------------------
// eta at eta_safe.  earned: r = 1 of r0 = 10 at k = 32 of 1000.  unearned: r = 9 at k = 37 of 100 (the artificial rule).
static double weight_after(const PdhgRules& R, bool earned, double om, double dx0sq, double dy0sq, double xt2 = 0.0, double yt2 = 0.0) {
    PdhgCtl c = pdhg_start();
    Pt p; p.eta = 0.5; p.om = om;
    start_period(R, c, p, 10.0);
    PdhgSums s = far(earned ? 1.0 : 9.0, p);
    s.dx0sq = dx0sq; s.dy0sq = dy0sq; s.xt2 = xt2; s.yt2 = yt2;
    const Out o = check(R, c, p, s, earned ? 32 : 37, earned ? 1000 : 100);
    EXPECT(o.n.action == PDHG_RESTART);
    return o.n.om;
}
static void weight() {
    PdhgRules R = host_rules();
    begin("weight_update_and_clamp");
    EXPECT(close_to(weight_after(R, true, 1.0, 1.0, 16.0), 2.0));                 // sqrt(1 * 4 / 1)
    EXPECT(close_to(weight_after(R, true, 4.0, 9.0, 9.0), 2.0));                  // sqrt(4 * 1)
    EXPECT(close_to(weight_after(R, false, 1.0, 1.0, 16.0), 2.0));                // an unearned restart under the plain rule
    EXPECT(weight_after(R, true, 1.0, 1.0, 1e16) == 1e3);                         // sqrt(1e8) = 1e4 -> 1e3 omega_ref
    EXPECT(weight_after(R, true, 1.0, 1e16, 1.0) == 1e-3);                        // 1e-4 -> 1e-3 omega_ref
    R.omega_ref = 2.0;
    EXPECT(weight_after(R, true, 1.0, 1.0, 1e16) == 2e3);
    R.omega_ref = 1.0;
    // the guard: a movement of 1e-9 (<= 1e-8) says nothing; with |xt| = 100 the bar is 1.01e-6
    EXPECT(weight_after(R, true, 1.0, 1e-18, 16.0) == 1.0);
    EXPECT(weight_after(R, true, 1.0, 16.0, 1e-18) == 1.0);
    EXPECT(weight_after(R, true, 1.0, 1e-12, 1e-12, 1e4, 0.0) == 1.0);
    EXPECT(close_to(weight_after(R, true, 1.0, 4e-12, 16e-12, 1e4, 0.0), std::sqrt(2.0)));   // sqrt(4e-6 / 2e-6)
    end();
    begin("weight_damping");
    R.om_art_k = 148.0;                                                           // theta = 0.5 * 37 / 148 = 0.125: 16^0.125 = sqrt(2)
    EXPECT(close_to(weight_after(R, false, 1.0, 1.0, 256.0), 1.4142135623730951));
    EXPECT(close_to(weight_after(R, true, 1.0, 1.0, 256.0), 4.0));                // an earned restart keeps theta = 0.5
    R.om_art_k = 20.0;                                                            // k / K > 1: theta = 0.5
    EXPECT(close_to(weight_after(R, false, 1.0, 1.0, 256.0), 4.0));
    R.om_art_k = 0.0;
    EXPECT(close_to(weight_after(R, false, 1.0, 1.0, 256.0), 4.0));
    R.om_art = false;                                                             // unearned restarts leave the weight alone
    EXPECT(weight_after(R, false, 1.0, 1.0, 256.0) == 1.0);
    EXPECT(close_to(weight_after(R, true, 1.0, 1.0, 256.0), 4.0));
    R.om_art = true; R.om_art_clamp = 2.0;                                        // at most a factor 2 per unearned restart
    EXPECT(weight_after(R, false, 1.0, 1.0, 256.0) == 2.0);
    EXPECT(close_to(weight_after(R, true, 1.0, 1.0, 256.0), 4.0));
    R.om_art_clamp = 0.0; R.om_clamp = 3.0;                                       // at most a factor 3 per restart
    EXPECT(weight_after(R, true, 1.0, 1.0, 256.0) == 3.0);
    R.om_clamp = 0.0; R.om_clamp_down = 2.0;                                      // downwards only: 0.25 -> 0.5, upwards free
    EXPECT(weight_after(R, true, 1.0, 256.0, 1.0) == 0.5);
    EXPECT(close_to(weight_after(R, true, 1.0, 1.0, 256.0), 4.0));
    end();
}

int main() {
    static_assert(sizeof(PdhgCtl) <= 16 * sizeof(double), "the state must fit the 16 doubles k_ecp_blocks reserves");
    convergence("host_convergence", host_rules());
    stagnation("host_stagnation_exit", host_rules(), 3);
    stalled_row("host_stalled_row_exit", host_rules());
    nan_residual("host_nan_residual", host_rules(), true);
    convergence("device_convergence", device_rules());
    stagnation("device_stagnation_exit", device_rules(), 5);
    stalled_row("device_stalled_row_exit", device_rules());
    nan_residual("device_nan_residual", device_rules(), false);
    restart_rules();
    backoffs();
    consolidation();
    weight();
    std::printf("%s\n", g_fail ? "FAILED" : "all ok");
    return g_fail ? 1 : 0;
}
