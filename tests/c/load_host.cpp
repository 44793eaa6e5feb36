// load_host.cpp -- the index arithmetic of loadproblem (csrc/load_host.hpp) on the smallest inputs that reach each branch, run on a
// CPU under AddressSanitizer and UBSan by tests/test_load_host.py.  Expected values are literals worked out by hand from the
// layouts' descriptions; the batched layout is also recomputed by brute force (for each entry its bucket from col / block and
// slot / batch), with no code of the header.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "load_host.hpp"

using namespace ktn;

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

static const double INF = std::numeric_limits<double>::infinity();
enum { L = KTN_ATOM_LIN, Q = KTN_ATOM_QUAD, E = KTN_ATOM_EXP, N = KTN_ATOM_NEGLOG };
constexpr int kShift = 29;

// ---- blocked layout: blk_cols = 4, 10 columns (blocks 0-3, 4-7, 8-9), NL slots = rows 0, 1, 2 ------------------------------------
//   row 0 (SEP): columns 0 L, 1 E, 3 L | 4 N, 5 Q, 6 L | 8 E, 9 Q      entries 0-7    (4 and 8: block edges)
//   row 1 (SEP): columns 2 Q, 3 Q      |               | 9 L           entries 8-10
//   row 2 (TAPE): columns 1, 5                                         entries 11-12  (its segments stay empty)
// p0 = 10 + entry, p1 = 100 + entry.  Written block-major, slot-minor, inside a segment LIN, QUAD, EXP, NEGLOG in stable order:
//   block 0: slot 0: entries 0, 2, 1; slot 1: 8, 9      block 1: slot 0: 5, 4, 3      block 2: slot 0: 7, 6; slot 1: 10
struct Blocked {
    std::vector<int32_t> nlrows{0, 1, 2};
    std::vector<int64_t> rowptr{0, 8, 11, 13};
    std::vector<int32_t> col{0, 1, 3, 4, 5, 6, 8, 9, 2, 3, 9, 1, 5};
    std::vector<uint8_t> rowkind{KTN_ROW_SEP, KTN_ROW_SEP, KTN_ROW_TAPE};
    std::vector<uint8_t> akind{L, E, L, N, Q, L, E, Q, Q, Q, L, 0, 0};
    std::vector<double> p0, p1;
    std::vector<int64_t> bseg;
    std::vector<HostInt4> bkind;
    std::vector<int32_t> bcolk;
    std::vector<HostDouble2> bpp;
    int64_t w = 0;
    Blocked() {
        for (int e = 0; e < 13; ++e) { p0.push_back(10.0 + e); p1.push_back(100.0 + e); }
        w = blocked_layout(nlrows, rowptr, col, rowkind, akind, p0, p1, 4, 3, kShift, bseg, bkind, bcolk, bpp);
    }
};

static void blocked_cases() {
    Blocked B;
    const int order[11] = {0, 2, 1, 8, 9, 5, 4, 3, 7, 6, 10};           // the entry each written position holds
    const int64_t seg[12] = {0, 3, 5, 5, 5, 8, 8, 8, 8, 10, 11, 11};     // bseg[b * 4 + si]; [b * 4 + 3]: end of block b
    begin("blocked_entries_once_in_segment");
    EXPECT(B.w == 11);
    EXPECT(B.bcolk.size() == 13 && B.bpp.size() == 13);                  // sized for every NL entry, the tape row's unused
    for (int k = 0; k < 11 && k < B.w; ++k) {
        const int e = order[k];
        EXPECT(B.bcolk[k] == (B.col[e] | ((int32_t)B.akind[e] << kShift)));
        EXPECT(B.bpp[k].x == 10.0 + e && B.bpp[k].y == 100.0 + e);
    }
    {   // every SEP entry once, in segment (column / 4, slot)
        std::vector<int> seen(11, 0);
        for (int b = 0; b < 3; ++b)
            for (int si = 0; si < 3; ++si)
                for (int64_t k = B.bseg[b * 4 + si]; k < B.bseg[b * 4 + si + 1]; ++k) {
                    const int e = (int)(B.bpp[k].x - 10.0);
                    EXPECT(e >= 0 && e < 11);
                    if (e < 0 || e >= 11) continue;
                    ++seen[e];
                    EXPECT(B.col[e] / 4 == b);
                    EXPECT(e >= B.rowptr[si] && e < B.rowptr[si + 1]);
                }
        for (int e = 0; e < 11; ++e) EXPECT(seen[e] == 1);
    }
    end();

    begin("blocked_kinds_grouped_stable");
    {
        const int ks[9][3] = {{2, 2, 3}, {0, 2, 2}, {0, 0, 0}, {1, 2, 2}, {0, 0, 0}, {0, 0, 0}, {0, 1, 2}, {1, 1, 1}, {0, 0, 0}};
        for (int b = 0; b < 3; ++b)
            for (int si = 0; si < 3; ++si) {
                const HostInt4 k = B.bkind[b * 4 + si];
                EXPECT(k.x == ks[b * 3 + si][0] && k.y == ks[b * 3 + si][1] && k.z == ks[b * 3 + si][2] && k.w == 0);
                // inside the segment: kinds ascend, and within a kind the entries keep their order
                const int64_t s0 = B.bseg[b * 4 + si], s1 = B.bseg[b * 4 + si + 1];
                for (int64_t q = s0; q < s1; ++q) {
                    const int kd = (int)((uint32_t)B.bcolk[q] >> kShift);
                    const int64_t lo = kd == L ? 0 : kd == Q ? k.x : kd == E ? k.y : k.z;
                    const int64_t hi = kd == L ? k.x : kd == Q ? k.y : kd == E ? k.z : s1 - s0;
                    EXPECT(q - s0 >= lo && q - s0 < hi);
                    if (q > s0 && (int)((uint32_t)B.bcolk[q - 1] >> kShift) == kd) EXPECT(B.bpp[q - 1].x < B.bpp[q].x);
                }
            }
    }
    end();

    begin("blocked_tape_row_empty");
    for (int b = 0; b < 3; ++b) {
        EXPECT(B.bseg[b * 4 + 2] == B.bseg[b * 4 + 3]);
        const HostInt4 k = B.bkind[b * 4 + 2];
        EXPECT(k.x == 0 && k.y == 0 && k.z == 0);
    }
    end();

    begin("blocked_bseg_scan");
    EXPECT(B.bseg.size() == 12 && B.bkind.size() == 12);
    for (int k = 0; k < 12; ++k) EXPECT(B.bseg[k] == seg[k]);
    for (int k = 1; k < 12; ++k) EXPECT(B.bseg[k - 1] <= B.bseg[k]);
    EXPECT(B.bseg[11] == 11);                                            // the number of SEP entries
    end();
}

// ---- batched layout: 2 slots per batch, 4 columns per block, 10 columns; NL slots 0-4 = rows 1-5 (row 0 is linear) ------------
//   row 1 (slot 0): columns 0 L, 4 Q, 9 E        row 2 (slot 1): columns 0 N, 1 L, 4 Q        (4: a block edge)
//   row 3 (slot 2): empty, inside batch 1        row 4 (slot 3): columns 3 E, 8 N, 5 L
//   row 5 (slot 4): columns 2 Q, 7 E             (batch 2, partial)
struct Batched {
    std::vector<int32_t> nlrows{1, 2, 3, 4, 5};
    std::vector<int64_t> rowptr{0, 2, 5, 8, 8, 11, 13};
    std::vector<int32_t> col{0, 1, 0, 4, 9, 0, 1, 4, 3, 8, 5, 2, 7};
    std::vector<uint8_t> akind{L, L, L, Q, E, N, L, Q, E, N, L, Q, E};
    std::vector<double> p0, p1;
    std::vector<int64_t> segs;
    std::vector<uint16_t> sck, srw;
    std::vector<HostDouble2> spp;
    Batched() {
        for (int e = 0; e < 13; ++e) { p0.push_back(10.0 + e); p1.push_back(100.0 + e); }
        batched_layout(nlrows, rowptr, col, akind, p0, p1, 2, 4, 3, segs, sck, srw, spp);
    }
};

static void batched_cases() {
    Batched B;
    begin("batched_entries_in_buckets");
    EXPECT(B.sck.size() == 11 && B.srw.size() == 11 && B.spp.size() == 11);
    {   // brute force: bucket after bucket, slot after slot, entry after entry
        size_t k = 0;
        for (int batch = 0; batch < 3; ++batch)
            for (int block = 0; block < 3; ++block)
                for (int kind = 0; kind < 4; ++kind) {
                    EXPECT(B.segs[(size_t)(batch * 3 + block) * 4 + kind] == (int64_t)k);
                    for (int si = 0; si < 5; ++si)
                        for (int64_t e = B.rowptr[B.nlrows[si]]; e < B.rowptr[B.nlrows[si] + 1]; ++e) {
                            if (si / 2 != batch || B.col[e] / 4 != block || B.akind[e] != kind) continue;
                            EXPECT(k < 11);
                            if (k >= 11) continue;
                            EXPECT(B.sck[k] == B.col[e] % 4 && B.srw[k] == si % 2);
                            EXPECT(B.spp[k].x == 10.0 + e && B.spp[k].y == 100.0 + e);
                            ++k;
                        }
                }
        EXPECT(k == 11);
    }
    // by hand: bucket (batch 0, block 1, QUAD) holds column 4 of slots 0 and 1; (batch 1, block 2, NEGLOG) column 8 of slot 3
    {
        const int64_t a = B.segs[(0 * 3 + 1) * 4 + Q], b = B.segs[(1 * 3 + 2) * 4 + N];
        EXPECT(B.segs[(0 * 3 + 1) * 4 + Q + 1] - a == 2);
        EXPECT(B.sck[a] == 0 && B.srw[a] == 0 && B.spp[a].x == 13.0);
        EXPECT(B.sck[a + 1] == 0 && B.srw[a + 1] == 1 && B.spp[a + 1].x == 17.0);
        EXPECT(B.segs[(1 * 3 + 2) * 4 + N + 1] - b == 1);
        EXPECT(B.sck[b] == 0 && B.srw[b] == 1 && B.spp[b].x == 19.0);
    }
    end();

    begin("batched_rows_ascend");
    for (size_t q = 0; q + 1 < B.segs.size(); ++q)
        for (int64_t k = B.segs[q] + 1; k < B.segs[q + 1]; ++k) EXPECT(B.srw[k - 1] <= B.srw[k]);
    end();

    begin("batched_segs_scan");
    EXPECT(B.segs.size() == 3 * 3 * 4 + 1);
    EXPECT(B.segs[0] == 0 && B.segs.back() == 11);
    for (size_t q = 1; q < B.segs.size(); ++q) EXPECT(B.segs[q - 1] <= B.segs[q]);
    {   // counts by hand: batch 0: block 0 L 2 (0 of slot 0, 1 of slot 1), N 1; block 1 Q 2; block 2 E 1
        const int64_t cnt[36] = {2, 0, 0, 1, 0, 2, 0, 0, 0, 0, 1, 0,      // batch 0
                                 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 1,      // batch 1: slot 3 only
                                 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0};     // batch 2
        for (int q = 0; q < 36; ++q) EXPECT(B.segs[q + 1] - B.segs[q] == cnt[q]);
    }
    end();
}

// ---- classification: rows of the shape x^p + c = VAR, POWC p, CONST c, ADD(1, 2) ----------------------------------------------------
struct Tapes {
    std::vector<int32_t> tape_all{0, 1, 2, 3, 4};
    std::vector<int64_t> rowptr{0, 1, 2, 3, 4, 6};                      // row 4: a structure of two entries
    std::vector<int64_t> nl_slot{0, 1, 2, -1, 3};                       // row 3 is not an NL row
    std::vector<int64_t> nodeptr{0};
    std::vector<int32_t> nop, na, nb;
    std::vector<double> nc;
    std::vector<int32_t> cls_of, rep, cnt;
    void row(int r, int column, double p, double c) {
        nop.push_back(KTN_OP_VAR); na.push_back(column); nb.push_back((int32_t)rowptr[r]); nc.push_back(0.0);
        nop.push_back(KTN_OP_POWC); na.push_back(0); nb.push_back(0); nc.push_back(p);
        nop.push_back(KTN_OP_CONST); na.push_back(0); nb.push_back(0); nc.push_back(c);
        nop.push_back(KTN_OP_ADD); na.push_back(1); nb.push_back(2); nc.push_back(0.0);
        nodeptr.push_back((int64_t)nop.size());
    }
    Tapes() {
        row(0, 7, 2.0, 1.0);
        row(1, 3, 2.0, 5.0);      // another column, another constant: the shape of row 0
        row(2, 7, 3.0, 1.0);      // another exponent
        row(3, 7, 2.0, 1.0);      // row 0 again, but not an NL row
        row(4, 7, 2.0, 1.0);      // row 0 again, in a longer structure
        classify_tape_rows(tape_all, rowptr, nl_slot, nodeptr, nop, na, nb, nc, cls_of, rep, cnt);
    }
};

static void classification_cases() {
    Tapes T;
    begin("classify_constants_share_a_class");
    EXPECT(T.cls_of.size() == 5 && T.cls_of[0] == 0 && T.cls_of[1] == 0);
    EXPECT(T.rep.size() == 4 && T.cnt.size() == 4);
    if (T.rep.size() == 4 && T.cnt.size() == 4) {
        EXPECT(T.rep[0] == 0 && T.rep[1] == 2 && T.rep[2] == 3 && T.rep[3] == 4);
        EXPECT(T.cnt[0] == 2 && T.cnt[1] == 1 && T.cnt[2] == 1 && T.cnt[3] == 1);
    }
    end();
    begin("classify_powc_exponent_splits");
    EXPECT(T.cls_of.size() == 5 && T.cls_of[2] == 1);
    end();
    begin("classify_nl_row_splits");
    EXPECT(T.cls_of.size() == 5 && T.cls_of[3] == 2);
    end();
    begin("classify_structure_length_splits");
    EXPECT(T.cls_of.size() == 5 && T.cls_of[4] == 3);
    end();
}

// ---- postfix_to_nodes ------------------------------------------------------------------------------------------------------
struct Nodes { std::vector<int32_t> nop, na, nb; std::vector<double> nc; };
static bool all_free(const std::vector<int64_t>& slot_of) {
    for (int64_t s : slot_of) if (s != -1) return false;
    return true;
}
// the row's structure: columns 3, 5, 3 (3 listed twice), its Jacobian entries from 10
static void malformed(const char* name, std::vector<int32_t> op, std::vector<double> arg, int code, const char* msg) {
    begin(name);
    const int32_t rcols[3] = {3, 5, 3};
    std::vector<int64_t> slot_of(8, -1);
    Nodes D;
    int got = 0;
    std::string what;
    try {
        postfix_to_nodes(op.data(), arg.data(), (int64_t)op.size(), rcols, 3, 10, slot_of, D.nop, D.na, D.nb, D.nc);
    } catch (const Error& e) { got = e.code; what = e.what(); }
    EXPECT(got == code);
    EXPECT(what == msg);
    EXPECT(all_free(slot_of));
    end();
}

static void postfix_cases() {
    begin("postfix_duplicate_column_first_slot");
    {
        const int32_t rcols[3] = {3, 5, 3};
        const int32_t op[3] = {KTN_OP_VAR, KTN_OP_VAR, KTN_OP_ADD};
        const double arg[3] = {3.0, 5.0, 0.0};
        std::vector<int64_t> slot_of(8, -1);
        Nodes D;
        D.nop.push_back(KTN_OP_CONST); D.na.push_back(0); D.nb.push_back(0); D.nc.push_back(9.0);      // an earlier row's node
        postfix_to_nodes(op, arg, 3, rcols, 3, 10, slot_of, D.nop, D.na, D.nb, D.nc);
        EXPECT(D.nop.size() == 4 && D.na.size() == 4 && D.nb.size() == 4 && D.nc.size() == 4);
        if (D.nop.size() == 4) {
            EXPECT(D.nop[1] == KTN_OP_VAR && D.na[1] == 3 && D.nb[1] == 10);      // slot 0, not slot 2
            EXPECT(D.nop[2] == KTN_OP_VAR && D.na[2] == 5 && D.nb[2] == 11);
            EXPECT(D.nop[3] == KTN_OP_ADD && D.na[3] == 0 && D.nb[3] == 1);       // operands: nodes relative to the row's first
        }
        EXPECT(all_free(slot_of));
    }
    end();
    malformed("postfix_binary_underflow", {KTN_OP_VAR, KTN_OP_ADD}, {3.0, 0.0}, KTN_E_INVALID, "malformed tape (binary op underflow)");
    malformed("postfix_stack_not_reduced", {KTN_OP_VAR, KTN_OP_CONST}, {5.0, 1.0}, KTN_E_INVALID, "malformed tape (stack not reduced to one value)");
    malformed("postfix_var_missing_from_row", {KTN_OP_VAR}, {4.0}, KTN_E_INVALID, "tape variable missing from the row's Jacobian structure");
    malformed("postfix_var_beyond_the_columns", {KTN_OP_VAR}, {8.0}, KTN_E_INVALID, "tape variable missing from the row's Jacobian structure");
    malformed("postfix_unknown_opcode", {KTN_OP_VAR, 99}, {3.0, 0.0}, KTN_E_UNSUPPORTED, "Unsupported tape opcode 99");
}

// ---- the box vertex ----------------------------------------------------------------------------------------------------------
static void vertex_cases() {
    begin("vertex_smaller_magnitude_and_tie");
    {
        const double lo[3] = {-1.0, -5.0, -2.0}, hi[3] = {3.0, 2.0, 2.0};
        double v[3] = {9.0, 9.0, 9.0};
        EXPECT(box_vertex(lo, hi, 3, v));
        EXPECT(v[0] == -1.0 && v[1] == 2.0 && v[2] == -2.0);              // the tie takes the lower bound
    }
    end();
    begin("vertex_infinite_sides");
    {
        const double lo[3] = {1.0, -INF, -INF}, hi[3] = {INF, 4.0, INF};
        double v[3] = {9.0, 9.0, 9.0};
        EXPECT(box_vertex(lo, hi, 3, v));
        EXPECT(v[0] == 1.0 && v[1] == 4.0 && v[2] == 0.0);
    }
    end();
    begin("vertex_crossed_bounds_clear_ok");
    {
        const double lo[2] = {0.0, 3.0}, hi[2] = {1.0, 1.0};
        double v[2] = {9.0, 9.0};
        EXPECT(!box_vertex(lo, hi, 2, v));
        EXPECT(v[0] == 0.0 && v[1] == 1.0);
    }
    end();
}

// ---- the epigraph cut at the vertex: columns 0, 2, 1, vertex (1, 2, 3) -------------------------------------------------------------
static void cut_cases() {
    const int32_t col[3] = {0, 2, 1};
    const double vtx[3] = {1.0, 2.0, 3.0};
    begin("cut_nan_coefficient_not_finite");
    {
        const double j[3] = {4.0, std::nan(""), 1.0};
        EXPECT(!epigraph_vertex_cut(col, j, 3, 0.0, vtx, false, 1e9).finite);
        const double k[3] = {4.0, INF, 1.0};
        EXPECT(!epigraph_vertex_cut(col, k, 3, 0.0, vtx, false, 1e9).finite);
        const double f[3] = {4.0, 2.0, 1.0};
        EXPECT(epigraph_vertex_cut(col, f, 3, 0.0, vtx, false, 1e9).finite);
    }
    end();
    begin("cut_pad_zero_lifts_maximum");
    {
        const double j[2] = {-3.0, -1.0};
        // max -1: -3 + 1.5 < -1 goes, -1 stays.  With the dense row's zeros max 0: -3 + 1.5 < 0 goes, -1 + 1.5 >= 0 stays;
        // with range 0.5 both go
        VertexCut c = epigraph_vertex_cut(col, j, 2, 0.0, vtx, false, 1.5);
        EXPECT(c.coef.size() == 2 && c.coef[0] == 0.0 && c.coef[1] == -1.0);
        c = epigraph_vertex_cut(col, j, 2, 0.0, vtx, false, 0.5);
        EXPECT(c.coef.size() == 2 && c.coef[0] == 0.0 && c.coef[1] == -1.0);
        c = epigraph_vertex_cut(col, j, 2, 0.0, vtx, true, 0.5);
        EXPECT(c.coef.size() == 2 && c.coef[0] == 0.0 && c.coef[1] == 0.0);
        c = epigraph_vertex_cut(col, j, 2, 0.0, vtx, true, 1.5);
        EXPECT(c.coef.size() == 2 && c.coef[0] == 0.0 && c.coef[1] == -1.0);
    }
    end();
    begin("cut_rounding_threshold");
    {
        const double j[3] = {8.0, 6.0, 5.0};                              // range 2: 6 + 2 = 8 stays (equality), 5 + 2 < 8 goes
        const VertexCut c = epigraph_vertex_cut(col, j, 3, 10.0, vtx, false, 2.0);
        EXPECT(c.finite && c.coef.size() == 3);
        if (c.coef.size() == 3) EXPECT(c.coef[0] == 8.0 && c.coef[1] == 6.0 && c.coef[2] == 0.0);
    }
    end();
    begin("cut_constant");
    {
        const double j[3] = {8.0, 6.0, 5.0};                              // b = 10 - (1 * 8 + 3 * 6 + 2 * 5): the unrounded coefficients
        EXPECT(epigraph_vertex_cut(col, j, 3, 10.0, vtx, false, 2.0).b == -26.0);
        EXPECT(epigraph_vertex_cut(col, j, 0, 10.0, vtx, true, 2.0).b == 10.0);
    }
    end();
}

int main() {
    blocked_cases();
    batched_cases();
    classification_cases();
    postfix_cases();
    vertex_cases();
    cut_cases();
    std::printf(g_fail ? "%d cases FAILED\n" : "all ok\n", g_fail);
    return g_fail ? 1 : 0;
}
