// load_host.hpp -- the parts of loadproblem (load.hip) that touch neither the engine, the stream nor a device buffer: index
// arithmetic over the caller's structure.  Plain C++ in the manner of pdhg_check.hpp -- no HIP header, no kernel header -- so that
// tests/c/load_host.cpp runs all of it on a CPU under the sanitizers.  Where the device layout is a HIP vector type the layouts
// below are written into a plain struct of the same size and alignment (load.hip asserts both before it uploads them).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <unordered_map>
#include <vector>

#include "error.hpp"

namespace ktn {

struct alignas(16) HostDouble2 { double x, y; };             // double2
struct alignas(16) HostInt4 { int32_t x, y, z, w; };         // int4

// ------------------------------------------------------------------------------------
// A tape VAR's Jacobian slot is the FIRST structure entry of its column; a column listed twice keeps 0 in the other
// entries.  `slot_of` (one entry per column, all -1 on entry and on return) maps a column to that slot, so a row costs
// O(tape + row) instead of a scan of the row per VAR.
// ------------------------------------------------------------------------------------
inline void postfix_to_nodes(const int32_t* op, const double* arg, int64_t len, const int32_t* rcols, int64_t rlen,
                             int64_t jac_base, std::vector<int64_t>& slot_of, std::vector<int32_t>& nop,
                             std::vector<int32_t>& na, std::vector<int32_t>& nb, std::vector<double>& nc) {
    std::vector<int32_t> st;
    const int64_t base = (int64_t)nop.size();
    for (int64_t s = rlen - 1; s >= 0; --s) slot_of[(size_t)rcols[s]] = s;          // backwards: the first slot wins
    struct Reset {                                                                   // (also when a malformed tape throws)
        std::vector<int64_t>& m; const int32_t* c; int64_t n;
        ~Reset() { for (int64_t s = 0; s < n; ++s) m[(size_t)c[s]] = -1; }
    } reset{slot_of, rcols, rlen};
    for (int64_t t = 0; t < len; ++t) {
        const int o = op[t];
        int32_t a = 0, b = 0;
        double c = 0.0;
        switch (o) {
            case KTN_OP_CONST: c = arg[t]; break;
            case KTN_OP_VAR: {
                const double av = arg[t];
                const int64_t slot = (av > -1.0 && av < (double)slot_of.size()) ? slot_of[(size_t)(int64_t)av] : -1;
                const int32_t v = (int32_t)av;
                if (slot < 0) throw Error(KTN_E_INVALID, "tape variable missing from the row's Jacobian structure");
                a = v;
                b = (int32_t)(jac_base + slot);
            } break;
            case KTN_OP_ADD: case KTN_OP_SUB: case KTN_OP_MUL: case KTN_OP_DIV:
                if (st.size() < 2) throw Error(KTN_E_INVALID, "malformed tape (binary op underflow)");
                b = st.back(); st.pop_back();
                a = st.back(); st.pop_back();
                break;
            case KTN_OP_POWC: c = arg[t];  // fallthrough
            case KTN_OP_NEG: case KTN_OP_EXP: case KTN_OP_LOG: case KTN_OP_SQRT: case KTN_OP_SIN: case KTN_OP_COS:
                if (st.empty()) throw Error(KTN_E_INVALID, "malformed tape (unary op underflow)");
                a = st.back(); st.pop_back();
                break;
            default: throw Error(KTN_E_UNSUPPORTED, "Unsupported tape opcode " + std::to_string(o));
        }
        nop.push_back(o); na.push_back(a); nb.push_back(b); nc.push_back(c);
        st.push_back((int32_t)((int64_t)nop.size() - 1 - base));
    }
    if (len > 0 && st.size() != 1) throw Error(KTN_E_INVALID, "malformed tape (stack not reduced to one value)");
}

// ------------------------------------------------------------------------------------
// Shape classes of the tape rows `tape_all` (ascending).  Two rows share a shape when their node lists agree in length, opcodes,
// operand indices, POWC exponents and the VARs' Jacobian slots relative to rowptr, when their structures are equally long,
// and when both or neither are NL rows (nl_slot >= 0; so a class is swept as a whole or not at all).  CONST values, columns,
// rconst and bounds may differ.  The node lists are hashed (O(total nodes)); a row is compared with the first row of its hash's
// classes only, so many distinct shapes cost nothing quadratic.  Classes are numbered by their first member.
//   cls_of[t]: class of tape_all[t];  rep[c]: first member of class c (index into tape_all);  cnt[c]: its size
// ------------------------------------------------------------------------------------
inline void classify_tape_rows(const std::vector<int32_t>& tape_all, const std::vector<int64_t>& rowptr, const std::vector<int64_t>& nl_slot,
                               const std::vector<int64_t>& nodeptr, const std::vector<int32_t>& nop, const std::vector<int32_t>& na,
                               const std::vector<int32_t>& nb, const std::vector<double>& nc, std::vector<int32_t>& cls_of,
                               std::vector<int32_t>& rep, std::vector<int32_t>& cnt) {
    const size_t nt = tape_all.size();
    cls_of.assign(nt, -1); rep.clear(); cnt.clear();
    std::vector<int32_t> next_same;                                  // hash chain of the classes
    auto rel_b = [&](int64_t r, int64_t i) -> int32_t {              // VAR: slot relative to the row; else operand b
        return nop[(size_t)i] == KTN_OP_VAR ? (int32_t)((int64_t)nb[(size_t)i] - rowptr[(size_t)r]) : nb[(size_t)i];
    };
    auto same_shape = [&](int64_t r, int64_t q) {
        const int64_t b0 = nodeptr[(size_t)r], b1 = nodeptr[(size_t)q], n = nodeptr[(size_t)r + 1] - b0;
        if (n != nodeptr[(size_t)q + 1] - b1) return false;
        if (rowptr[(size_t)r + 1] - rowptr[(size_t)r] != rowptr[(size_t)q + 1] - rowptr[(size_t)q]) return false;
        if ((nl_slot[(size_t)r] >= 0) != (nl_slot[(size_t)q] >= 0)) return false;
        for (int64_t i = 0; i < n; ++i) {
            const int op = nop[(size_t)(b0 + i)];
            if (op != nop[(size_t)(b1 + i)]) return false;
            if (op == KTN_OP_CONST) continue;
            if (rel_b(r, b0 + i) != rel_b(q, b1 + i)) return false;
            if (op != KTN_OP_VAR && na[(size_t)(b0 + i)] != na[(size_t)(b1 + i)]) return false;
            if (op == KTN_OP_POWC && std::memcmp(&nc[(size_t)(b0 + i)], &nc[(size_t)(b1 + i)], sizeof(double)) != 0) return false;
        }
        return true;
    };
    std::unordered_map<uint64_t, int32_t> head;                      // hash -> first class with it
    for (size_t t = 0; t < nt; ++t) {
        const int64_t r = tape_all[t];
        const int64_t b0 = nodeptr[(size_t)r], n = nodeptr[(size_t)r + 1] - b0;
        uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;
        auto mix = [&](uint64_t v) { h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2); h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33; };
        mix((uint64_t)(rowptr[(size_t)r + 1] - rowptr[(size_t)r]));
        mix(nl_slot[(size_t)r] >= 0 ? 1u : 0u);
        for (int64_t i = b0; i < b0 + n; ++i) {
            const int op = nop[(size_t)i];
            uint64_t w = (uint64_t)(uint32_t)op;
            if (op != KTN_OP_CONST) w |= (uint64_t)(uint32_t)rel_b(r, i) << 32;
            mix(w);
            if (op > KTN_OP_VAR) mix((uint64_t)(uint32_t)na[(size_t)i]);
            if (op == KTN_OP_POWC) { uint64_t bits; std::memcpy(&bits, &nc[(size_t)i], 8); mix(bits); }
        }
        auto it = head.find(h);
        int32_t c = -1;
        if (it != head.end()) {
            int32_t last = -1;
            for (c = it->second; c >= 0; last = c, c = next_same[(size_t)c])
                if (same_shape(r, tape_all[(size_t)rep[(size_t)c]])) break;
            if (c < 0) { c = (int32_t)rep.size(); rep.push_back((int32_t)t); cnt.push_back(0); next_same.push_back(-1); next_same[(size_t)last] = c; }
        } else {
            c = (int32_t)rep.size(); rep.push_back((int32_t)t); cnt.push_back(0); next_same.push_back(-1);
            head.emplace(h, c);
        }
        cls_of[t] = c;
        ++cnt[(size_t)c];
    }
}

// ------------------------------------------------------------------------------------
// Block-major copy of the NL rows for the column-blocked sweep (kernels.hpp k_sep_eval_blk): segment (b, si) holds the entries
// of NL slot si with columns in [b * blk_cols, (b + 1) * blk_cols), grouped by atom kind in stable order.  Needs every separable
// NL row sorted by column (the segments are found by binary search); a row that is not KTN_ROW_SEP has empty segments.
//   bseg[b * (m_nl + 1) + si]: first entry of the segment, [.. + m_nl]: end of block b
//   bkind[b * (m_nl + 1) + si]: where the QUAD, EXP and NEGLOG entries start inside it (x, y, z)
//   bcolk: column | kind << kind_shift;  bpp: (p0, p1).  Returns the entries written.
// ------------------------------------------------------------------------------------
inline int64_t blocked_layout(const std::vector<int32_t>& nlrows, const std::vector<int64_t>& rowptr, const std::vector<int32_t>& col,
                              const std::vector<uint8_t>& rowkind, const std::vector<uint8_t>& akind, const std::vector<double>& p0,
                              const std::vector<double>& p1, int blk_cols, int blk_nb, int kind_shift, std::vector<int64_t>& bseg,
                              std::vector<HostInt4>& bkind, std::vector<int32_t>& bcolk, std::vector<HostDouble2>& bpp) {
    const int64_t m_nl = (int64_t)nlrows.size();
    int64_t nnz_nl = 0;
    for (int32_t r : nlrows) nnz_nl += rowptr[(size_t)r + 1] - rowptr[(size_t)r];
    bseg.assign((size_t)(m_nl + 1) * blk_nb, 0);
    bkind.assign((size_t)(m_nl + 1) * blk_nb, HostInt4{0, 0, 0, 0});
    bcolk.assign((size_t)nnz_nl, 0);
    bpp.assign((size_t)nnz_nl, HostDouble2{0.0, 0.0});
    // cut[si * (NB + 1) + b]: first entry of row si with column >= b * blk_cols
    std::vector<int64_t> cut((size_t)m_nl * (blk_nb + 1));
    for (int64_t si = 0; si < m_nl; ++si) {
        const int64_t r = nlrows[(size_t)si];
        const int32_t* cb = col.data() + rowptr[(size_t)r];
        const int32_t* ce = (rowkind[(size_t)r] == KTN_ROW_SEP) ? col.data() + rowptr[(size_t)r + 1] : cb;   // tape rows: empty
        for (int b = 0; b <= blk_nb; ++b) {
            const int64_t c0 = (int64_t)b * blk_cols;
            cut[(size_t)si * (blk_nb + 1) + b] =
                rowptr[(size_t)r] + (std::lower_bound(cb, ce, c0, [](int32_t a, int64_t v) { return (int64_t)a < v; }) - cb);
        }
    }
    int64_t w = 0;
    for (int b = 0; b < blk_nb; ++b) {
        for (int64_t si = 0; si < m_nl; ++si) {
            bseg[(size_t)b * (m_nl + 1) + si] = w;
            const int64_t eb = cut[(size_t)si * (blk_nb + 1) + b], ee = cut[(size_t)si * (blk_nb + 1) + b + 1];
            const int64_t w0 = w;
            int32_t kstart[KTN_ATOM_NEGLOG + 1];
            for (int kd = 0; kd <= KTN_ATOM_NEGLOG; ++kd) {      // segment grouped by atom kind (stable)
                kstart[kd] = (int32_t)(w - w0);
                for (int64_t e = eb; e < ee; ++e) {
                    if (akind[(size_t)e] != kd) continue;
                    bcolk[(size_t)w] = col[(size_t)e] | ((int32_t)kd << kind_shift);
                    bpp[(size_t)w] = HostDouble2{p0[(size_t)e], p1[(size_t)e]};
                    ++w;
                }
            }
            bkind[(size_t)b * (m_nl + 1) + si] = HostInt4{kstart[KTN_ATOM_QUAD], kstart[KTN_ATOM_EXP], kstart[KTN_ATOM_NEGLOG], 0};
        }
        bseg[(size_t)b * (m_nl + 1) + m_nl] = w;
    }
    return w;
}

// ------------------------------------------------------------------------------------
// Batch-blocked copy of the NL entries for many short rows (kernels.hpp k_sep_sweep_batch), built in two counting passes:
// bucket (batch of sb_rows slots, block of sb_cols columns, atom kind), rows ascending inside a bucket because the slots are
// visited in order -- 20 B per entry.
//   segs[(batch * sb_nb + block) * 4 + kind]: first entry of the bucket, one trailing total
//   sck: column inside its block;  srw: slot inside its batch;  spp: (p0, p1)
// ------------------------------------------------------------------------------------
inline void batched_layout(const std::vector<int32_t>& nlrows, const std::vector<int64_t>& rowptr, const std::vector<int32_t>& col,
                           const std::vector<uint8_t>& akind, const std::vector<double>& p0, const std::vector<double>& p1, int sb_rows,
                           int sb_cols, int sb_nb, std::vector<int64_t>& segs, std::vector<uint16_t>& sck, std::vector<uint16_t>& srw,
                           std::vector<HostDouble2>& spp) {
    const int64_t m_nl = (int64_t)nlrows.size();
    int64_t nnz_nl = 0;
    for (int32_t r : nlrows) nnz_nl += rowptr[(size_t)r + 1] - rowptr[(size_t)r];
    const size_t nbuck = (size_t)((m_nl + sb_rows - 1) / sb_rows) * sb_nb * 4;
    segs.assign(nbuck + 4, 0);
    for (int64_t si = 0; si < m_nl; ++si) {
        const int64_t r = nlrows[(size_t)si];
        const size_t base = (size_t)(si / sb_rows) * sb_nb * 4;
        for (int64_t e = rowptr[(size_t)r]; e < rowptr[(size_t)r + 1]; ++e)
            ++segs[base + (size_t)(col[(size_t)e] / sb_cols) * 4 + akind[(size_t)e] + 1];
    }
    for (size_t k = 1; k < segs.size(); ++k) segs[k] += segs[k - 1];
    std::vector<int64_t> cur(segs.begin(), segs.begin() + nbuck);
    sck.assign((size_t)nnz_nl, 0); srw.assign((size_t)nnz_nl, 0);
    spp.assign((size_t)nnz_nl, HostDouble2{0.0, 0.0});
    for (int64_t si = 0; si < m_nl; ++si) {
        const int64_t r = nlrows[(size_t)si];
        const size_t base = (size_t)(si / sb_rows) * sb_nb * 4;
        const uint16_t rl = (uint16_t)(si % sb_rows);
        for (int64_t e = rowptr[(size_t)r]; e < rowptr[(size_t)r + 1]; ++e) {
            const int64_t bl = col[(size_t)e] / sb_cols;
            const int64_t w = cur[base + (size_t)bl * 4 + akind[(size_t)e]]++;
            sck[(size_t)w] = (uint16_t)(col[(size_t)e] - bl * sb_cols);
            srw[(size_t)w] = rl;
            spp[(size_t)w] = HostDouble2{p0[(size_t)e], p1[(size_t)e]};
        }
    }
    segs.resize(nbuck + 1);
}

// ------------------------------------------------------------------------------------
// The bound-box vertex of the initial epigraph cut (model.jl:93-97): per column the bound of smaller magnitude (the lower one
// on a tie: the GLPK non-basic rule), the finite one where only one is, 0 where neither.  vtx[0, n) is written;
// returns false when some l_j > u_j.
// ------------------------------------------------------------------------------------
inline bool box_vertex(const double* lv, const double* uv, int64_t n, double* vtx) {
    bool ok = true;
    for (int64_t j = 0; j < n; ++j) {
        const double lo = lv[j], hi = uv[j];
        if (lo > hi) ok = false;
        const bool lf = std::isfinite(lo), uf = std::isfinite(hi);
        if (lf && uf) vtx[j] = (std::fabs(lo) <= std::fabs(hi)) ? lo : hi;   // GLPK non-basic rule
        else if (lf) vtx[j] = lo;
        else if (uf) vtx[j] = hi;
        else vtx[j] = 0.0;
    }
    return ok;
}

// ------------------------------------------------------------------------------------
// gencut + round_coefs of one row at a point (the epigraph cut at the vertex, model.jl:156-164): from the row's columns, its
// Jacobian slice `jac` and its value g there, the cut's coefficients, its constant b = g - sum_e vtx[col_e] jac_e and whether
// every coefficient is finite.  A coefficient more than cut_coef_rng below the largest becomes 0; pad_zero: the reference's
// dense row has structural zeros, which take part in that maximum.
// ------------------------------------------------------------------------------------
struct VertexCut {
    std::vector<double> coef;
    double b = 0.0;
    bool finite = true;
};
inline VertexCut epigraph_vertex_cut(const int32_t* col, const double* jac, int64_t len, double g, const double* vtx, bool pad_zero,
                                     double cut_coef_rng) {
    VertexCut c;
    c.b = g;
    double mx = -std::numeric_limits<double>::infinity();
    for (int64_t e = 0; e < len; ++e) {
        c.coef.push_back(jac[e]);
        c.b += -vtx[col[e]] * jac[e];
        if (!(jac[e] <= mx)) mx = (jac[e] != jac[e]) ? jac[e] : std::max(mx, jac[e]);
        if (!std::isfinite(jac[e])) c.finite = false;
    }
    if (pad_zero && !(mx != mx)) mx = std::max(mx, 0.0);
    for (auto& cf : c.coef) if (cf + cut_coef_rng < mx) cf = 0.0;   // round_coefs
    return c;
}

}  // namespace ktn
