// sweep.hip -- loadproblem! (src/model.jl:81-173) and the separator sweep (src/separators.jl:85-135, src/model.jl:272-283)  (struct Engine: engine.hpp)
#include <cstring>
#include <unordered_map>

#include "engine.hpp"
#include "launch.hpp"
#include "kernels.hpp"
#include "tape_classes.hpp"
#include "quad_rows.hpp"
#include "batch_lp.hpp"
#include "batch_ecp.hpp"
#include "dense_lp.hpp"
#include "kkt.hpp"

namespace ktn {

// ------------------------------------------------------------------------------------
// loadproblem!  src/model.jl:81-173
// ------------------------------------------------------------------------------------
// A tape VAR's Jacobian slot is the FIRST structure entry of its column; a column listed twice keeps 0 in the other
// entries.  `slot_of` (one entry per column, all -1 on entry and on return) maps a column to that slot, so a row costs
// O(tape + row) instead of a scan of the row per VAR.
static void postfix_to_nodes(const int32_t* op, const double* arg, int64_t len, const int32_t* rcols, int64_t rlen,
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

// KTN_ROW_HOST: the caller's evaluator computes g and J of those rows at x (one call per sweep, like the reference's
// precompute!, src/separators.jl:111-116); the values are staged to the device, everything downstream is unchanged.
void Engine::host_eval(const double* d_x) {
    const int64_t nx = std::min<int64_t>(n_lp > 0 ? n_lp : n0, n0 + 1);
    KTN_HIP(hipMemcpyAsync(h_xh.data(), d_x, (size_t)nx * sizeof(double), hipMemcpyDeviceToHost, stream));
    sync();
    if (host_constr_rows) {
        const int rc = cb_rows(cb_user, h_xh.data(), h_gh.data(), h_jh.data());
        if (rc != 0) throw Error(KTN_E_CALLBACK, "eval_rows callback failed (" + std::to_string(rc) + ")");
    }
    if (host_obj) {
        double f = 0.0;
        double* grad = h_jh.data() + h_rowptr[m0];
        const int rc = cb_obj(cb_user, h_xh.data(), &f, grad);
        if (rc != 0) throw Error(KTN_E_CALLBACK, "eval_obj callback failed (" + std::to_string(rc) + ")");
        const double t = (nx > n0) ? h_xh[(size_t)n0] : 0.0;
        h_gh[(size_t)m0] = f - t;                       // f(x) - t, src/nlpeval.jl:45
        grad[n0] = -1.0;                                // src/nlpeval.jl:62
    }
    d_gh.upload(h_gh.data(), (size_t)m_ext, stream);
    d_jh.upload(h_jh.data(), (size_t)nnz_ext, stream);
    NlpDev P = nlp_view();
    SweepOut O = sweep_view();
    launch_n(k_host_scatter, n_host, stream, P, d_hostrows.p, n_host, d_gh.p, d_jh.p, O);
    check_launch();
    stats["host_evals"] += 1.0;
}

// ------------------------------------------------------------------------------------
// Shape classes of the tape rows (tape_classes.hpp).  Two rows share a shape when their node lists agree in length, opcodes,
// operand indices, POWC exponents and the VARs' Jacobian slots relative to rowptr, when their structures are equally long,
// and when both or neither are NL rows (so a class is swept as a whole or not at all).  CONST values, columns, rconst and
// bounds may differ.  The node lists are hashed (O(total nodes)); a row is compared with the first row of its hash's
// classes only, so many distinct shapes cost nothing quadratic.  Members keep ascending row order.
// ------------------------------------------------------------------------------------
void Engine::build_tape_classes(const std::vector<int64_t>& nodeptr, const std::vector<int32_t>& nop, const std::vector<int32_t>& na,
                                const std::vector<int32_t>& nb, const std::vector<double>& nc, const std::vector<int32_t>& tape_all) {
    tc_rows = tc_rows_nl = 0;
    tc_launches.clear();
    const size_t nt = tape_all.size();
    if (nt == 0) {                                                   // no tape rows: nothing to class, nothing to upload
        d_tapeint_all.n = d_tapeint_nl.n = 0;
        tape_bytes = 0.0;
        for (const char* k : {"tape_classes", "tape_classed_rows", "tape_interp_rows", "tape_class_max_nodes", "tape_shapes",
                              "tape_class_lds_bytes", "tape_class_dev_bytes"}) stats[k] = 0.0;
        return;
    }
    std::vector<int32_t> nl_slot((size_t)m_ext, -1);
    for (size_t si = 0; si < h_nlrows.size(); ++si) nl_slot[(size_t)h_nlrows[si]] = (int32_t)si;
    // algorithmic bytes of the NL tape rows: 8 per constant, 4 per column, 8 per gathered x*, 8 per Jacobian entry, 48 of
    // per-row outputs, 8 for row id and slot
    tape_bytes = 0.0;
    for (size_t t = 0; t < nt; ++t) {
        const int64_t r = tape_all[t];
        if (nl_slot[(size_t)r] < 0) continue;
        int64_t k = 0;
        for (int64_t i = nodeptr[(size_t)r]; i < nodeptr[(size_t)r + 1]; ++i) k += nop[(size_t)i] == KTN_OP_CONST ? 1 : 0;
        const int64_t S = h_rowptr[(size_t)r + 1] - h_rowptr[(size_t)r];
        tape_bytes += 8.0 * (double)k + (4.0 + 8.0 + 8.0) * (double)S + 48.0 + 8.0;
    }
    const int64_t min_rows = dev.tape_classed == 0 ? 0 : (dev.tape_classed > 0 ? 2 : kTapeClassMin);
    std::vector<int32_t> cls_of(nt, -1), rep, cnt, next_same;        // per class: first member (index into tape_all), size, hash chain
    if (min_rows > 0 && nt > 0) {
        auto rel_b = [&](int64_t r, int64_t i) -> int32_t {          // VAR: slot relative to the row; else operand b
            return nop[(size_t)i] == KTN_OP_VAR ? (int32_t)((int64_t)nb[(size_t)i] - h_rowptr[(size_t)r]) : nb[(size_t)i];
        };
        auto same_shape = [&](int64_t r, int64_t q) {
            const int64_t b0 = nodeptr[(size_t)r], b1 = nodeptr[(size_t)q], n = nodeptr[(size_t)r + 1] - b0;
            if (n != nodeptr[(size_t)q + 1] - b1) return false;
            if (h_rowptr[(size_t)r + 1] - h_rowptr[(size_t)r] != h_rowptr[(size_t)q + 1] - h_rowptr[(size_t)q]) return false;
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
        std::unordered_map<uint64_t, int32_t> head;                  // hash -> first class with it
        for (size_t t = 0; t < nt; ++t) {
            const int64_t r = tape_all[t];
            const int64_t b0 = nodeptr[(size_t)r], n = nodeptr[(size_t)r + 1] - b0;
            uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;
            auto mix = [&](uint64_t v) { h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2); h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33; };
            mix((uint64_t)(h_rowptr[(size_t)r + 1] - h_rowptr[(size_t)r]));
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
    // the classed classes: large enough, and the LDS image of a wavefront within its budget; NL classes first, by size bucket
    const size_t ncls_all = rep.size();
    std::vector<int32_t> dense(ncls_all, -1), order;
    int64_t max_nodes = 0;
    for (int pass = 0; pass < 8; ++pass)
        for (size_t c = 0; c < ncls_all; ++c) {
            const int64_t r = tape_all[(size_t)rep[c]];
            const int64_t n = nodeptr[(size_t)r + 1] - nodeptr[(size_t)r], S = h_rowptr[(size_t)r + 1] - h_rowptr[(size_t)r];
            if (cnt[c] < min_rows || 2 * n + S > kTapeClassMaxCells) continue;
            if ((nl_slot[(size_t)r] >= 0) != (pass < 4) || tape_class_bucket(2 * n + S) != (pass & 3)) continue;
            dense[c] = (int32_t)order.size();
            order.push_back((int32_t)c);
        }
    const size_t ncls = order.size();
    std::vector<TapeClassMeta> meta(ncls);
    std::vector<int32_t> p_op, p_a, p_b, wave_cls, wave_first;
    std::vector<double> p_c;
    std::vector<uint8_t> rowflag((size_t)m_ext, 0);
    int64_t mem = 0, ncst = 0, ncol = 0;
    std::vector<std::vector<int32_t>> cpos(ncls);                    // positions of the CONST nodes of a class
    int last_bucket = -1;
    size_t max_lds = 0;
    for (size_t k = 0; k < ncls; ++k) {
        const size_t c = (size_t)order[k];
        const int64_t r = tape_all[(size_t)rep[c]];
        const int64_t b0 = nodeptr[(size_t)r], n = nodeptr[(size_t)r + 1] - b0, S = h_rowptr[(size_t)r + 1] - h_rowptr[(size_t)r];
        TapeClassMeta& M = meta[k];
        M.count = cnt[c]; M.nnodes = (int32_t)n; M.nslots = (int32_t)S; M.prog0 = (int32_t)p_op.size();
        M.mem0 = mem; M.cst0 = ncst; M.col0 = ncol;
        for (int64_t i = b0; i < b0 + n; ++i) {
            const int op = nop[(size_t)i];
            p_op.push_back(op);
            if (op == KTN_OP_CONST) { p_a.push_back((int32_t)cpos[k].size()); p_b.push_back(0); cpos[k].push_back((int32_t)(i - b0)); }
            else if (op == KTN_OP_VAR) { p_a.push_back(0); p_b.push_back((int32_t)((int64_t)nb[(size_t)i] - h_rowptr[(size_t)r])); }
            else { p_a.push_back(na[(size_t)i]); p_b.push_back(nb[(size_t)i]); }
            p_c.push_back(op == KTN_OP_POWC ? nc[(size_t)i] : 0.0);
        }
        const bool nl = nl_slot[(size_t)r] >= 0;
        const size_t lds = (size_t)(2 * n + S) * kTapeClassWave * sizeof(double);
        const int bucket = tape_class_bucket(2 * n + S);
        if (tc_launches.empty() || tc_launches.back().nl != nl || bucket != last_bucket) tc_launches.push_back({(int64_t)wave_cls.size(), 0, 0, nl});
        last_bucket = bucket;
        for (int64_t f = 0; f < M.count; f += kTapeClassWave) { wave_cls.push_back((int32_t)k); wave_first.push_back((int32_t)f); }
        tc_launches.back().nwaves = (int64_t)wave_cls.size() - tc_launches.back().wave0;
        tc_launches.back().lds = std::max(tc_launches.back().lds, lds);
        max_lds = std::max(max_lds, lds);
        if (nl) tc_rows_nl += M.count;
        mem += M.count; ncst += (int64_t)cpos[k].size() * M.count; ncol += S * M.count;
        max_nodes = std::max(max_nodes, n);
    }
    tc_rows = mem;
    // members in ascending row order (tape_all is ascending), operands class-major
    std::vector<int32_t> mrow((size_t)mem), mslot((size_t)mem), scol((size_t)ncol), fill(ncls, 0), int_all, int_nl;
    std::vector<double> cst((size_t)ncst);
    for (size_t t = 0; t < nt; ++t) {
        const int32_t r = tape_all[t];
        const int32_t k = cls_of[t] >= 0 ? dense[(size_t)cls_of[t]] : -1;
        if (k < 0) {
            int_all.push_back(r);
            if (nl_slot[(size_t)r] >= 0) int_nl.push_back(r);
            continue;
        }
        const TapeClassMeta& M = meta[(size_t)k];
        const int64_t j = fill[(size_t)k]++;
        mrow[(size_t)(M.mem0 + j)] = r;
        mslot[(size_t)(M.mem0 + j)] = nl_slot[(size_t)r];
        rowflag[(size_t)r] = 1;
        const int64_t b0 = nodeptr[(size_t)r], e0 = h_rowptr[(size_t)r];
        for (size_t q = 0; q < cpos[(size_t)k].size(); ++q) cst[(size_t)(M.cst0 + (int64_t)q * M.count + j)] = nc[(size_t)(b0 + cpos[(size_t)k][q])];
        for (int64_t sl = 0; sl < M.nslots; ++sl) scol[(size_t)(M.col0 + sl * M.count + j)] = h_col[(size_t)(e0 + sl)];
    }
    d_tapeint_all.upload(int_all, stream); d_tapeint_nl.upload(int_nl, stream);
    d_tc_wavecls.upload(wave_cls, stream); d_tc_wavefirst.upload(wave_first, stream); d_tc_meta.upload(meta, stream);
    d_tc_op.upload(p_op, stream); d_tc_a.upload(p_a, stream); d_tc_b.upload(p_b, stream); d_tc_c.upload(p_c, stream);
    d_tc_cst.upload(cst, stream); d_tc_scol.upload(scol, stream); d_tc_mrow.upload(mrow, stream); d_tc_mslot.upload(mslot, stream);
    d_tc_rowflag.upload(rowflag, stream);
    sync();
    stats["tape_classes"] = (double)ncls;
    stats["tape_classed_rows"] = (double)tc_rows;
    stats["tape_interp_rows"] = (double)int_all.size();
    stats["tape_class_max_nodes"] = (double)max_nodes;
    stats["tape_shapes"] = (double)ncls_all;
    stats["tape_class_lds_bytes"] = (double)max_lds;
    stats["tape_class_dev_bytes"] = 8.0 * (double)ncst + 4.0 * (double)ncol + 8.0 * (double)mem + 8.0 * (double)wave_cls.size() +
                                    20.0 * (double)p_op.size() + (double)(sizeof(TapeClassMeta) * ncls) + (double)m_ext;
}

// k_tape_classed over the classes of NL rows (the sweep; mslot: NL slots) or over all classes (precompute_all; mslot: rows)
void Engine::launch_tape_classed(bool nl_only, const int32_t* mslot, const double* d_x, double f_tol) {
    if (tc_launches.empty()) return;
    if (!tc_lds_set) {
        KTN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tape_classed), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(kTapeClassMaxCells * kTapeClassWave * sizeof(double))));
        tc_lds_set = true;
    }
    NlpDev P = nlp_view();
    SweepOut O = sweep_view();
    for (const TcLaunch& q : tc_launches) {
        if (nl_only && !q.nl) continue;
        TapeClassDev T = tape_class_view();
        T.wave_cls += q.wave0; T.wave_first += q.wave0;
        launch(k_tape_classed, (unsigned)q.nwaves, kTapeClassWave, q.lds, stream, P, T, mslot, d_x, f_tol, O);
    }
}

TapeClassDev Engine::tape_class_view() {
    TapeClassDev T;
    T.wave_cls = d_tc_wavecls.p; T.wave_first = d_tc_wavefirst.p; T.meta = d_tc_meta.p;
    T.prog_op = d_tc_op.p; T.prog_a = d_tc_a.p; T.prog_b = d_tc_b.p; T.prog_c = d_tc_c.p;
    T.cst = d_tc_cst.p; T.scol = d_tc_scol.p; T.mrow = d_tc_mrow.p;
    return T;
}

// ------------------------------------------------------------------------------------
// KTN_ROW_QUAD rows (quad_rows.hpp): validation of the caller's quad_* arrays and the device layout.  Host work and uploads
// only; called from loadproblem once the extended structure and the NL row list stand.
// ------------------------------------------------------------------------------------
void Engine::build_quad_rows(const ktn_nlp_desc* d) {
    n_quad = n_quad_nl = n_quad_ent = n_quad_ent_nl = quad_nnz = 0;
    quad_bytes = 0.0;
    stats["quad_rows"] = stats["quad_nnz"] = stats["quad_group"] = 0.0;
    const int64_t nnz0 = h_rowptr[(size_t)m0];
    std::vector<int32_t> qrows;
    bool constr_quad = false;
    for (int64_t i = 0; i < m_ext; ++i)
        if (h_rowkind[(size_t)i] == KTN_ROW_QUAD) { qrows.push_back((int32_t)i); if (i < m0) constr_quad = true; }
    KTN_REQUIRE(!constr_quad || d->quad_ptr != nullptr, "KTN_ROW_QUAD rows without quad_ptr");
    if (d->quad_ptr) {
        KTN_REQUIRE(d->quad_ptr[0] >= 0, "quad_ptr not monotone");
        for (int64_t e = 0; e < nnz0; ++e) KTN_REQUIRE(d->quad_ptr[e + 1] >= d->quad_ptr[e], "quad_ptr not monotone");
        for (int64_t i = 0; i < m0; ++i)
            KTN_REQUIRE(h_rowkind[(size_t)i] == KTN_ROW_QUAD || d->quad_ptr[h_rowptr[(size_t)i + 1]] == d->quad_ptr[h_rowptr[(size_t)i]],
                        "quad_ptr: a row that is not KTN_ROW_QUAD has a non-empty segment");
        KTN_REQUIRE(d->quad_ptr[nnz0] == 0 || (d->quad_col != nullptr && d->quad_val != nullptr), "quad_ptr without quad_col / quad_val");
    }
    const bool obj_quad = h_rowkind[(size_t)m0] == KTN_ROW_QUAD;
    if (obj_quad && d->obj_quad_ptr) {
        KTN_REQUIRE(d->obj_quad_ptr[0] >= 0, "obj_quad_ptr not monotone");
        for (int64_t e = 0; e < d->obj_nnz; ++e) KTN_REQUIRE(d->obj_quad_ptr[e + 1] >= d->obj_quad_ptr[e], "obj_quad_ptr not monotone");
        KTN_REQUIRE(d->obj_quad_ptr[d->obj_nnz] == 0 || (d->obj_quad_col != nullptr && d->obj_quad_val != nullptr),
                    "obj_quad_ptr without obj_quad_col / obj_quad_val");
        KTN_REQUIRE(!(d->obj_linear && d->obj_quad_ptr[d->obj_nnz] > d->obj_quad_ptr[0]), "obj_linear = 1 with a non-empty objective Q");
    }
    if (qrows.empty()) {
        d_qcol.release(); d_qval.release(); d_qptr.release(); d_qjidx.release(); d_qvterm.release();
        return;
    }
    std::vector<int32_t> qcol;
    std::vector<double> qval;
    std::vector<int64_t> qptr(1, 0), jidx, tbase;
    std::vector<uint8_t> in_row((size_t)n0 + 1, 0);
    for (int32_t i : qrows) {
        const int64_t rb = h_rowptr[(size_t)i], re = h_rowptr[(size_t)i + 1];
        const bool obj = i == m0;
        const int64_t* ptr = obj ? d->obj_quad_ptr : d->quad_ptr;
        const int32_t* qc = obj ? d->obj_quad_col : d->quad_col;
        const double* qv = obj ? d->obj_quad_val : d->quad_val;
        const int64_t own = obj ? d->obj_nnz : re - rb;            // (the epigraph row's last entry, t, has no segment)
        const int64_t eb = obj ? 0 : rb;
        for (int64_t e = 0; e < own; ++e) in_row[(size_t)h_col[(size_t)(rb + e)]] = 1;
        tbase.push_back((int64_t)jidx.size());
        const int64_t q0 = (int64_t)qcol.size();
        for (int64_t e = 0; e < re - rb; ++e) {
            if (ptr && e < own)
                for (int64_t k = ptr[eb + e]; k < ptr[eb + e + 1]; ++k) {
                    const int32_t c = qc[k];
                    if (c < 0 || c >= n0 || !in_row[(size_t)c]) {
                        for (int64_t f = 0; f < own; ++f) in_row[(size_t)h_col[(size_t)(rb + f)]] = 0;
                        throw Error(KTN_E_INVALID, "quad_col: column " + std::to_string(c) + " is not in the structure of row " + std::to_string(i));
                    }
                    qcol.push_back(c); qval.push_back(qv[k]);
                }
            jidx.push_back(rb + e);
            qptr.push_back((int64_t)qcol.size());
        }
        for (int64_t e = 0; e < own; ++e) in_row[(size_t)h_col[(size_t)(rb + e)]] = 0;
        if (!obj && d->row_linear && d->row_linear[i])
            KTN_REQUIRE((int64_t)qcol.size() == q0, "row_linear = 1 on a KTN_ROW_QUAD row with a non-empty Q");
    }
    n_quad = (int64_t)qrows.size(); n_quad_ent = (int64_t)jidx.size(); quad_nnz = (int64_t)qcol.size();
    // launch lists: all QUAD rows; the QUAD rows among the NL rows
    std::vector<int64_t> nl_slot((size_t)m_ext, -1), slots_all, slots_nl, tbase_nl, ent_nl;
    std::vector<int32_t> rows_nl;
    for (size_t si = 0; si < h_nlrows.size(); ++si) nl_slot[(size_t)h_nlrows[si]] = (int64_t)si;
    int64_t qnnz_nl = 0;
    for (size_t k = 0; k < qrows.size(); ++k) {
        const int32_t i = qrows[k];
        slots_all.push_back(nl_slot[(size_t)i]);
        if (nl_slot[(size_t)i] < 0) continue;
        rows_nl.push_back(i); slots_nl.push_back(nl_slot[(size_t)i]); tbase_nl.push_back(tbase[k]);
        const int64_t len = h_rowptr[(size_t)i + 1] - h_rowptr[(size_t)i];
        for (int64_t e = 0; e < len; ++e) ent_nl.push_back(tbase[k] + e);
        qnnz_nl += qptr[(size_t)(tbase[k] + len)] - qptr[(size_t)tbase[k]];
    }
    n_quad_nl = (int64_t)rows_nl.size(); n_quad_ent_nl = (int64_t)ent_nl.size();
    if (n_quad_nl == n_quad) ent_nl.clear();                       // the same list: entry t = position
    grp_quad = pick_group(n_quad_ent ? (double)quad_nnz / (double)n_quad_ent : 4.0);
    if (dev.quad_group == 4 || dev.quad_group == 8 || dev.quad_group == 16 || dev.quad_group == 32 || dev.quad_group == 64) grp_quad = dev.quad_group;
    grp_quad_rows = pick_group((double)n_quad_ent / (double)n_quad);
    // algorithmic bytes of one evaluation of the NL QUAD rows: 12 per Q entry and 8 per gathered x; per Jacobian entry the segment
    // pointer, index, (a, -) pair, column, x, Jacobian and value term written and read back; per row its record and outputs
    quad_bytes = 20.0 * (double)qnnz_nl + (8.0 + 8.0 + 16.0 + 4.0 + 8.0 + 16.0 + 16.0 + 4.0 + 8.0) * (double)n_quad_ent_nl + (28.0 + 16.0 + 48.0) * (double)n_quad_nl;
    d_qcol.upload(qcol, stream); d_qval.upload(qval, stream); d_qptr.upload(qptr, stream); d_qjidx.upload(jidx, stream);
    d_qvterm.resize((size_t)n_quad_ent + 1, stream);
    d_qrows_all.upload(qrows, stream); d_qslots_all.upload(slots_all, stream); d_qtbase_all.upload(tbase, stream);
    d_qrows_nl.upload(rows_nl, stream); d_qslots_nl.upload(slots_nl, stream); d_qtbase_nl.upload(tbase_nl, stream); d_qent_nl.upload(ent_nl, stream);
    sync();
    stats["quad_rows"] = (double)n_quad;
    stats["quad_nnz"] = (double)quad_nnz;
    stats["quad_group"] = (double)grp_quad;
}

// k_quad_jac + k_quad_stats over the QUAD rows among the NL rows (the sweep: flags by NL slot) or over all of them (precompute_all)
void Engine::launch_quad(bool nl_only, const double* d_x, double f_tol) {
    const int64_t nr = nl_only ? n_quad_nl : n_quad, ne = nl_only ? n_quad_ent_nl : n_quad_ent;
    if (nr == 0) return;
    NlpDev P = nlp_view();
    SweepOut O = sweep_view();
    QuadDev Q{d_qcol.p, d_qval.p, d_qptr.p, d_qjidx.p, d_qvterm.p};
    QuadList L;
    L.rows = nl_only ? d_qrows_nl.p : d_qrows_all.p;
    L.slots = nl_only ? d_qslots_nl.p : d_qslots_all.p;
    L.tbase = nl_only ? d_qtbase_nl.p : d_qtbase_all.p;
    L.ent = (nl_only && n_quad_nl != n_quad) ? d_qent_nl.p : nullptr;
    L.n_rows = nr; L.n_ent = ne;
    size_t ta = 0, tb = 0;
    const bool ev = prm.profile && nl_only;
    if (ev) { ta = ev_get(); tb = ev_get(); KTN_HIP(hipEventRecord(ev_pool[ta], stream)); }
    with_group(grp_quad, [&](auto g) { launch(k_quad_jac<g()>, group_grid(ne, g()), kBlock, 0, stream, P, Q, L, d_x, O); });
    with_group(grp_quad_rows, [&](auto g) { launch(k_quad_stats<g()>, group_grid(nr, g()), kBlock, 0, stream, P, Q, L, d_x, f_tol, nl_only ? 1 : 0, O); });
    if (ev) { KTN_HIP(hipEventRecord(ev_pool[tb], stream)); ev_recs.push_back({5, ta, tb, quad_bytes}); }
}

void Engine::loadproblem(int64_t num_var, int64_t num_constr, const double* l_var, const double* u_var,
                         const double* l_constr, const double* u_constr, int32_t sense_, const ktn_nlp_desc* d) {
    KTN_REQUIRE(d != nullptr, "nlp description is NULL");
    KTN_REQUIRE(num_var >= 0 && num_constr >= 0, "negative sizes");
    KTN_REQUIRE(d->num_var == num_var && d->num_constr == num_constr, "nlp description sizes disagree with loadproblem");
    KTN_REQUIRE(num_var + 1 < ((int64_t)1 << kKindShift), "num_var too large for the packed 29-bit column index");
    const bool dbg_load = dev.debug_load;
    auto tl0 = std::chrono::steady_clock::now();
    auto lapl = [&](const char* what) {
        if (!dbg_load) return;
        (void)hipStreamSynchronize(stream);
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[load] %-28s %.2f ms\n", what, 1e3 * std::chrono::duration<double>(now - tl0).count());
        tl0 = now;
    };
    loaded = false;
    n0 = num_var; m0 = num_constr; sense = sense_;
    obj_linear = d->obj_linear != 0;
    m_ext = m0 + 1;
    const int64_t nnz0 = m0 ? d->rowptr[m0] : 0;

    // ---- extended structure: rows 0..m0-1 + the objective row f(x) - t over n0+1 variables
    //      (EpigraphNLPEvaluator, src/nlpeval.jl:42-63; only structural non-zeros are stored,
    //       the reference's dense zeros are remembered in pad_zero for round_coefs)
    h_rowptr.assign(d->rowptr, d->rowptr + m0 + 1);
    h_col.assign(d->col, d->col + nnz0);
    // (bulk copies: a batch of 512 instances brings 3e6 entries through here)
    std::vector<uint8_t> akind, padzero(m_ext, 0);
    std::vector<double> p0, p1, rconst(m_ext, 0.0);
    if (d->atom_kind) akind.assign(d->atom_kind, d->atom_kind + nnz0); else akind.assign((size_t)nnz0, 0);
    if (d->p0) p0.assign(d->p0, d->p0 + nnz0); else p0.assign((size_t)nnz0, 0.0);
    if (d->p1) p1.assign(d->p1, d->p1 + nnz0); else p1.assign((size_t)nnz0, 0.0);
    {
        const size_t tail = (size_t)std::max<int64_t>(std::max<int64_t>(d->obj_nnz, d->obj_tape_len), (d->obj_kind == KTN_ROW_HOST ? n0 : 0)) + 2;
        h_col.reserve((size_t)nnz0 + tail); akind.reserve((size_t)nnz0 + tail); p0.reserve((size_t)nnz0 + tail); p1.reserve((size_t)nnz0 + tail);
    }
    h_rowkind.assign(m_ext, KTN_ROW_SEP);
    {
        int32_t cmin = 0, cmax = -1;
        for (int64_t e = 0; e < nnz0; ++e) { const int32_t c = h_col[e]; cmin = std::min(cmin, c); cmax = std::max(cmax, c); }
        KTN_REQUIRE(cmin >= 0 && cmax < n0, "column index out of range");
    }
    for (int64_t i = 0; i < m0; ++i) {
        h_rowkind[i] = d->row_kind ? d->row_kind[i] : KTN_ROW_SEP;
        rconst[i] = d->rconst ? d->rconst[i] : 0.0;
        KTN_REQUIRE(h_rowptr[i + 1] >= h_rowptr[i], "rowptr not monotone");
    }
    // objective row
    std::vector<int32_t> ocols;
    if (d->obj_kind == KTN_ROW_SEP) {
        for (int64_t e = 0; e < d->obj_nnz; ++e) {
            KTN_REQUIRE(d->obj_col[e] >= 0 && d->obj_col[e] < n0, "objective column out of range");
            h_col.push_back(d->obj_col[e]);
            akind.push_back(d->obj_atom_kind ? d->obj_atom_kind[e] : 0);
            p0.push_back(d->obj_p0[e]);
            p1.push_back(d->obj_p1 ? d->obj_p1[e] : 0.0);
        }
        h_col.push_back((int32_t)n0);   // - t
        akind.push_back(KTN_ATOM_LIN);
        p0.push_back(-1.0);
        p1.push_back(0.0);
        rconst[m0] = d->obj_const;
        h_rowkind[m0] = KTN_ROW_SEP;
    } else if (d->obj_kind == KTN_ROW_QUAD) {
        // f(x) - t as a QUAD row: the caller's entries first, then t with coefficient -1 and an empty segment
        KTN_REQUIRE(d->obj_nnz == 0 || (d->obj_col != nullptr && d->obj_p0 != nullptr), "KTN_ROW_QUAD objective without obj_col / obj_p0");
        for (int64_t e = 0; e < d->obj_nnz; ++e) {
            KTN_REQUIRE(d->obj_col[e] >= 0 && d->obj_col[e] < n0, "objective column out of range");
            h_col.push_back(d->obj_col[e]); akind.push_back(0); p0.push_back(d->obj_p0[e]); p1.push_back(0.0);
        }
        h_col.push_back((int32_t)n0); akind.push_back(0); p0.push_back(-1.0); p1.push_back(0.0);
        rconst[m0] = d->obj_const;
        h_rowkind[m0] = KTN_ROW_QUAD;
    } else if (d->obj_kind == KTN_ROW_HOST) {
        // dense row, like the reference's own epigraph row (src/nlpeval.jl:49-54)
        KTN_REQUIRE(d->eval_obj != nullptr, "KTN_ROW_HOST objective without eval_obj callback");
        for (int64_t j = 0; j <= n0; ++j) { h_col.push_back((int32_t)j); akind.push_back(0); p0.push_back(0.0); p1.push_back(0.0); }
        rconst[m0] = 0.0;
        h_rowkind[m0] = KTN_ROW_HOST;
    } else {
        for (int64_t t = 0; t < d->obj_tape_len; ++t)
            if (d->obj_tape_op[t] == KTN_OP_VAR) ocols.push_back((int32_t)d->obj_tape_arg[t]);
        std::sort(ocols.begin(), ocols.end());
        ocols.erase(std::unique(ocols.begin(), ocols.end()), ocols.end());
        for (auto c : ocols) {
            KTN_REQUIRE(c >= 0 && c < n0, "objective tape variable out of range");
            h_col.push_back(c); akind.push_back(0); p0.push_back(0.0); p1.push_back(0.0);
        }
        h_col.push_back((int32_t)n0); akind.push_back(0); p0.push_back(0.0); p1.push_back(0.0);
        rconst[m0] = d->obj_const;
        h_rowkind[m0] = KTN_ROW_TAPE;
    }
    h_rowptr.push_back((int64_t)h_col.size());
    nnz_ext = (int64_t)h_col.size();
    // what ktn_set_linear_objective can rewrite in place: a linear row of LIN atoms, or a QUAD row (obj_linear: its Q is empty)
    obj_settable = obj_linear && (d->obj_kind == KTN_ROW_SEP || d->obj_kind == KTN_ROW_QUAD);
    for (int64_t e = h_rowptr[(size_t)m0]; e < nnz_ext && d->obj_kind == KTN_ROW_SEP; ++e)
        if (akind[(size_t)e] != KTN_ATOM_LIN) obj_settable = false;
    screen_pending = false; crossed_cols = 0;
    for (int64_t i = 0; i < m0; ++i) {                   // atom_kind and p1 are ignored for QUAD rows
        if (h_rowkind[i] != KTN_ROW_QUAD) continue;
        for (int64_t e = h_rowptr[i]; e < h_rowptr[i + 1]; ++e) { akind[(size_t)e] = 0; p1[(size_t)e] = 0.0; }
    }
    padzero[m0] = (h_rowptr[m0 + 1] - h_rowptr[m0]) < (n0 + 1) ? 1 : 0;

    lapl("extended structure (host)");
    // ---- host-evaluated rows
    cb_rows = d->eval_rows; cb_obj = d->eval_obj; cb_user = d->eval_user;
    host_obj = h_rowkind[m0] == KTN_ROW_HOST;
    host_constr_rows = false;
    {
        std::vector<int32_t> hostrows;
        for (int64_t i = 0; i < m_ext; ++i) {
            KTN_REQUIRE(h_rowkind[i] <= KTN_ROW_QUAD, "unknown row kind");
            if (h_rowkind[i] != KTN_ROW_HOST) continue;
            hostrows.push_back((int32_t)i);
            if (i < m0) host_constr_rows = true;
        }
        KTN_REQUIRE(!host_constr_rows || cb_rows != nullptr, "KTN_ROW_HOST rows without eval_rows callback");
        n_host = (int64_t)hostrows.size();
        d_hostrows.upload(hostrows, stream);
        h_gh.assign((size_t)m_ext, 0.0);
        h_jh.assign((size_t)nnz_ext + 1, 0.0);
        h_xh.assign((size_t)n0 + 1, 0.0);
    }

    // ---- tapes -> expression DAGs
    std::vector<int64_t> nodeptr(m_ext + 1, 0);
    std::vector<int32_t> nop, na, nb;
    std::vector<double> nc;
    std::vector<int32_t> tape_all;
    std::vector<int64_t> col_slot;
    for (int64_t i = 0; i < m_ext; ++i) {
        if (h_rowkind[i] == KTN_ROW_TAPE) { col_slot.assign((size_t)n0 + 1, -1); break; }
    }
    for (int64_t i = 0; i < m_ext; ++i) {
        nodeptr[i] = (int64_t)nop.size();
        if (h_rowkind[i] != KTN_ROW_TAPE) continue;
        tape_all.push_back((int32_t)i);
        const int32_t* rc = h_col.data() + h_rowptr[i];
        const int64_t rl = h_rowptr[i + 1] - h_rowptr[i];
        if (i < m0) {
            KTN_REQUIRE(d->tape_ptr != nullptr, "tape row without tape arrays");
            const int64_t tb = d->tape_ptr[i], te = d->tape_ptr[i + 1];
            postfix_to_nodes(d->tape_op + tb, d->tape_arg + tb, te - tb, rc, rl, h_rowptr[i], col_slot, nop, na, nb, nc);
        } else {
            std::vector<int32_t> op(d->obj_tape_op, d->obj_tape_op + d->obj_tape_len);
            std::vector<double> arg(d->obj_tape_arg, d->obj_tape_arg + d->obj_tape_len);
            if (op.empty()) { op.push_back(KTN_OP_CONST); arg.push_back(0.0); }
            op.push_back(KTN_OP_VAR); arg.push_back((double)n0);
            op.push_back(KTN_OP_SUB); arg.push_back(0.0);
            postfix_to_nodes(op.data(), arg.data(), (int64_t)op.size(), rc, rl, h_rowptr[i], col_slot, nop, na, nb, nc);
        }
    }
    nodeptr[m_ext] = (int64_t)nop.size();

    // ---- bounds per extended row; NL row list (model.jl:115-122,144-148)
    h_lb.assign(m_ext, 0.0);
    h_ub.assign(m_ext, 0.0);
    for (int64_t i = 0; i < m0; ++i) { h_lb[i] = l_constr[i]; h_ub[i] = u_constr[i]; }
    h_nlrows.clear();
    std::vector<int64_t> lin_rows;
    for (int64_t i = 0; i < m0; ++i) {
        if (d->row_linear && d->row_linear[i]) lin_rows.push_back(i);
        else h_nlrows.push_back((int32_t)i);
    }
    n_lp = n0;
    std::vector<double> lv(l_var, l_var + n0), uv(u_var, u_var + n0);
    if (!obj_linear) {
        n_lp = n0 + 1;                                  // @variable(m.linear_model, y)  model.jl:137-138
        lv.push_back(-kInf);
        uv.push_back(kInf);
        h_lb[m0] = (sense == KTN_MAX) ? 0.0 : -kInf;    // model.jl:144
        h_ub[m0] = (sense == KTN_MAX) ? kInf : 0.0;
        if (dist.rank == 0) h_nlrows.push_back((int32_t)m0);      // row-sharded: the epigraph row belongs to rank 0
    }
    m_nl = (int64_t)h_nlrows.size();
    build_quad_rows(d);                                          // (validates the quad_* arrays: host-side only, nothing is launched)
    esh_build_aux(l_var, u_var, l_constr, u_constr, d);         // (esh.hip; cut_algo = KTN_CUT_SUPPORTING only)
    has_inf_bound = false;
    for (int64_t j = 0; j < n_lp; ++j)
        if (!std::isfinite(lv[j]) || !std::isfinite(uv[j])) has_inf_bound = true;
    has_big_bound = false;
    for (int64_t j = 0; j < n_lp; ++j)
        if ((std::isfinite(uv[j]) && uv[j] >= kDenseBig) || (std::isfinite(lv[j]) && -lv[j] >= kDenseBig)) has_big_bound = true;

    lapl("tapes, bounds, nl list");
    // ---- upload the NLP
    d_rowptr.upload(h_rowptr, stream); d_col.upload(h_col, stream);
    max_row_len = 2;                                   // (the bound-box vertex row and other engine-made rows are short)
    // (a LINEAR objective's row -- up to n entries -- is stored with the structure but never becomes an LP row: counting it made
    //  every LP solve of cfg3 scan for long rows, a launch and a host round trip each)
    for (int64_t i = 0; i < m0 + (obj_linear ? 0 : 1); ++i) max_row_len = std::max(max_row_len, h_rowptr[(size_t)i + 1] - h_rowptr[(size_t)i]);
    {
        // a cut has the sparsity of its NL row: the most entries ONE column can gain per sweep is the number of NL rows that
        // contain it (1-2 on the BASELINE shapes; m_nl for a variable every row shares -- min-max / epigraph-style models)
        std::vector<int32_t> cnt((size_t)n_lp + 1, 0);
        col_gain_max = 0;
        for (int32_t i : h_nlrows)
            for (int64_t e = h_rowptr[(size_t)i]; e < h_rowptr[(size_t)i + 1]; ++e)
                col_gain_max = std::max<int64_t>(col_gain_max, ++cnt[(size_t)h_col[(size_t)e]]);
    }
    {
        // packed row programs: the three arrays go up as they are and are packed on the device (k_pack_atoms)
        uint8_t kmax = 0;
        for (size_t e = 0; e < akind.size(); ++e) kmax = std::max(kmax, akind[e]);
        KTN_REQUIRE(kmax <= KTN_ATOM_NEGLOG, "unknown atom kind");
        const int64_t ne = (int64_t)h_col.size();
        DBuf<uint8_t> t_ak;
        DBuf<double> t_p0, t_p1;
        t_ak.upload(akind, stream); t_p0.upload(p0, stream); t_p1.upload(p1, stream);
        d_colk.resize((size_t)ne, stream); d_pp.resize((size_t)ne, stream);
        launch_n(k_pack_atoms, ne, stream, ne, d_col.p, t_ak.p, t_p0.p, t_p1.p, d_colk.p, d_pp.p);
        check_launch();
        sync();                                         // the temporaries are freed on leaving the scope
    }
    d_rconst.upload(rconst, stream);
    d_rowkind.upload(h_rowkind, stream); d_padzero.upload(padzero, stream);
    d_lb.upload(h_lb, stream); d_ub.upload(h_ub, stream);
    d_nodeptr.upload(nodeptr, stream); d_nodeop.upload(nop, stream); d_nodea.upload(na, stream);
    d_nodeb.upload(nb, stream); d_nodec.upload(nc, stream);
    d_nodeval.resize(nop.size() + 1, stream); d_nodeadj.resize(nop.size() + 1, stream);
    std::vector<int32_t> allrows(m_ext);
    for (int64_t i = 0; i < m_ext; ++i) allrows[i] = (int32_t)i;
    d_allrows.upload(allrows, stream);
    d_taperows_all.upload(tape_all, stream);
    std::vector<int32_t> tape_nl;
    int64_t nnz_nl = 0;
    for (auto r : h_nlrows) {
        if (h_rowkind[r] == KTN_ROW_TAPE) tape_nl.push_back(r);
        nnz_nl += h_rowptr[r + 1] - h_rowptr[r];
    }
    n_tape_nl = (int64_t)tape_nl.size();
    n_host_nl = 0;
    for (auto r : h_nlrows) n_host_nl += (h_rowkind[r] == KTN_ROW_HOST) ? 1 : 0;
    d_taperows_nl.upload(tape_nl, stream);
    d_nlrows.upload(h_nlrows, stream);
    {   // KKT report: where each original row's multiplier lives (its own LP row, or the cut list of its NL slot)
        std::vector<int32_t> rowmap((size_t)std::max<int64_t>(m0, 1), 0);
        for (size_t k = 0; k < lin_rows.size(); ++k) rowmap[(size_t)lin_rows[k]] = (int32_t)k;
        for (size_t si = 0; si < h_nlrows.size(); ++si) if (h_nlrows[si] < m0) rowmap[(size_t)h_nlrows[si]] = -1 - (int32_t)si;
        d_kkt_rowmap.upload(rowmap, stream);
        kkt_n_lin = (int64_t)lin_rows.size();
        kkt_mirror = false; kkt_seg_ok = false;
        feas_cached = false; feas_blk_cached = false; feas_sides_ok = false;
    }
    build_tape_classes(nodeptr, nop, na, nb, nc, tape_all);
    lapl("tape shape classes");
    grp_sweep = pick_group(m_nl ? (double)nnz_nl / (double)m_nl : 4.0);
    if (grp_sweep < 8) grp_sweep = 8;
    lapl("pack + upload NLP");
    // Long rows (hundreds of entries or more): block-major copy for the column-blocked sweep.  Needs every separable
    // NL row sorted by column (the segments are found by binary search).
    {
        // Measured on cfg3_hbm (2e7 entries, 2048 per row): exp/log atoms 156 -> 123 us, quadratic atoms 171 -> 114 us.
        // KTN_SWEEP_BLOCKED=0 switches it off (tests compare the two paths).
        if (dev.blk_cfg >= 0) blk_cfg = dev.blk_cfg;
        blk_cols = (blk_cfg == 2) ? 16384 : 8192;
        blk_wg_per_cu = (blk_cfg == 2) ? 1 : 2;
        const bool env = dev.sweep_blocked >= 0;
        blk_on = m_nl > 0 && n_lp >= 2 * blk_cols && (double)nnz_nl / (double)m_nl >= 256.0;
        if (env) blk_on = blk_on && dev.sweep_blocked != 0;
        blk_nb = ceil_div(n_lp, blk_cols);
        if (blk_on && (double)(m_nl + 1) * blk_nb > 4e8) blk_on = false;
        for (size_t si = 0; blk_on && si < h_nlrows.size(); ++si) {
            const int64_t r = h_nlrows[si];
            if (h_rowkind[r] != KTN_ROW_SEP) continue;
            for (int64_t e = h_rowptr[r] + 1; e < h_rowptr[r + 1]; ++e)
                if (h_col[e] < h_col[e - 1]) { blk_on = false; break; }
        }
        d_bcolk.release(); d_bpp.release(); d_bseg.release(); d_bkind.release(); d_part.release(); d_slots.release();
        if (blk_on) {
            std::vector<int64_t> bseg((size_t)(m_nl + 1) * blk_nb);
            std::vector<int4> bkind((size_t)(m_nl + 1) * blk_nb, make_int4(0, 0, 0, 0));
            std::vector<int32_t> bcolk((size_t)nnz_nl);
            std::vector<double2> bpp((size_t)nnz_nl);
            // cut[si * (NB + 1) + b]: first entry of row si with column >= b * blk_cols
            std::vector<int64_t> cut((size_t)m_nl * (blk_nb + 1));
            for (int64_t si = 0; si < m_nl; ++si) {
                const int64_t r = h_nlrows[si];
                const int32_t* cb = h_col.data() + h_rowptr[r];
                const int32_t* ce = (h_rowkind[r] == KTN_ROW_SEP) ? h_col.data() + h_rowptr[r + 1] : cb;   // tape rows: empty
                for (int b = 0; b <= blk_nb; ++b) {
                    const int64_t c0 = (int64_t)b * blk_cols;
                    cut[(size_t)si * (blk_nb + 1) + b] =
                        h_rowptr[r] + (std::lower_bound(cb, ce, c0, [](int32_t a, int64_t v) { return (int64_t)a < v; }) - cb);
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
                            if (akind[e] != kd) continue;
                            bcolk[(size_t)w] = h_col[e] | ((int32_t)kd << kKindShift);
                            bpp[(size_t)w] = make_double2(p0[e], p1[e]);
                            ++w;
                        }
                    }
                    bkind[(size_t)b * (m_nl + 1) + si] = make_int4(kstart[KTN_ATOM_QUAD], kstart[KTN_ATOM_EXP], kstart[KTN_ATOM_NEGLOG], 0);
                }
                bseg[(size_t)b * (m_nl + 1) + m_nl] = w;
            }
            d_bcolk.upload(bcolk.data(), (size_t)w, stream);
            d_bpp.upload(bpp.data(), (size_t)w, stream);
            std::vector<SepSlot> slots((size_t)m_nl);
            for (int64_t si = 0; si < m_nl; ++si) {
                const int64_t r = h_nlrows[si];
                SepSlot sl;
                sl.rconst = rconst[r]; sl.lb = h_lb[r]; sl.ub = h_ub[r];
                sl.row = (h_rowkind[r] == KTN_ROW_SEP) ? (int32_t)r : -1;
                sl.len_pad = (int32_t)(((h_rowptr[r + 1] - h_rowptr[r]) << 1) | (padzero[r] ? 1 : 0));
                slots[(size_t)si] = sl;
            }
            d_slots.upload(slots, stream);
            d_bseg.upload(bseg, stream);
            d_bkind.upload(bkind, stream);
            d_part.resize((size_t)m_nl * blk_nb, stream);
        }
    }
    // Very long separable rows get the device-side kind kRowSepLong and their own kernel (kernels.hpp k_sep_eval_long) -- not under
    // the column-blocked sweep, which is the long-row path of the NL rows and reads the host-side kinds
    {
        std::vector<uint8_t> dk(h_rowkind);
        std::vector<int32_t> lr, lnr;
        std::vector<int64_t> ls, lns;
        std::vector<int64_t> slot_of((size_t)m_ext, -1);
        for (int64_t si = 0; si < m_nl; ++si) slot_of[(size_t)h_nlrows[(size_t)si]] = si;
        for (int64_t i = 0; i < m_ext && !blk_on; ++i) {
            if (h_rowkind[i] != KTN_ROW_SEP || h_rowptr[(size_t)i + 1] - h_rowptr[(size_t)i] <= kLongEval) continue;
            dk[(size_t)i] = kRowSepLong;
            lr.push_back((int32_t)i); ls.push_back(slot_of[(size_t)i]);
            if (slot_of[(size_t)i] >= 0) { lnr.push_back((int32_t)i); lns.push_back(slot_of[(size_t)i]); }
        }
        n_longev = (int64_t)lr.size(); n_longev_nl = (int64_t)lnr.size();
        stats["sep_long_rows"] = (double)n_longev;
        if (n_longev > 0) {
            d_rowkind.upload(dk, stream);
            d_longev_rows.upload(lr, stream); d_longev_slots.upload(ls, stream);
            d_longev_nlrows.upload(lnr, stream); d_longev_nlslots.upload(lns, stream);
        }
    }
    // Many short rows: the batch-blocked copy (kernels.hpp k_sep_sweep_batch).  Built on the host in two counting passes over the
    // NL entries -- bucket (batch of 2 048 slots, block of 8 192 columns, atom kind), rows ascending inside a bucket because
    // the slots are visited in order -- 20 B per entry.
    {
        d_sbck.release(); d_sbrow.release(); d_sbpp.release(); d_sbseg.release();
        sb_on = !blk_on && 2 * m_nl >= (int64_t)3 * kSbRows * num_cus && n_tape_nl == 0 && n_host_nl == 0 && n_quad_nl == 0 && (double)nnz_nl / (double)std::max<int64_t>(m_nl, 1) <= 128.0 &&
                n_lp <= (int64_t)kSbCols * 64;
        if (dev.sweep_batched == 0) sb_on = false;
        if (dev.sweep_batched == 1) sb_on = m_nl > 0 && n_tape_nl == 0 && n_host_nl == 0 && n_quad_nl == 0 && n_lp <= (int64_t)kSbCols * 64 && !blk_on;
        if (sb_on) {
            sb_nb = ceil_div(n_lp, (int64_t)kSbCols);
            sb_batches = ceil_div(m_nl, (int64_t)kSbRows);
            const size_t nbuck = (size_t)sb_batches * sb_nb * 4;
            std::vector<int64_t> segs(nbuck + 4, 0);
            for (int64_t si = 0; si < m_nl; ++si) {
                const int64_t r = h_nlrows[(size_t)si];
                const size_t base = (size_t)(si / kSbRows) * sb_nb * 4;
                for (int64_t e = h_rowptr[r]; e < h_rowptr[r + 1]; ++e)
                    ++segs[base + (size_t)(h_col[e] / kSbCols) * 4 + akind[e] + 1];
            }
            for (size_t k = 1; k < segs.size(); ++k) segs[k] += segs[k - 1];
            std::vector<int64_t> cur(segs.begin(), segs.begin() + nbuck);
            std::vector<uint16_t> sck((size_t)nnz_nl), srw((size_t)nnz_nl);
            std::vector<double2> spp((size_t)nnz_nl);
            for (int64_t si = 0; si < m_nl; ++si) {
                const int64_t r = h_nlrows[(size_t)si];
                const size_t base = (size_t)(si / kSbRows) * sb_nb * 4;
                const uint16_t rl = (uint16_t)(si % kSbRows);
                for (int64_t e = h_rowptr[r]; e < h_rowptr[r + 1]; ++e) {
                    const int64_t bl = h_col[e] / kSbCols;
                    const int64_t w = cur[base + (size_t)bl * 4 + akind[e]]++;
                    sck[(size_t)w] = (uint16_t)(h_col[e] - bl * kSbCols);
                    srw[(size_t)w] = rl;
                    spp[(size_t)w] = make_double2(p0[e], p1[e]);
                }
            }
            segs.resize(nbuck + 1);
            d_sbck.upload(sck, stream); d_sbrow.upload(srw, stream); d_sbpp.upload(spp, stream); d_sbseg.upload(segs, stream);
            sync();
        }
        stats["sweep_batched"] = sb_on ? 1.0 : 0.0;
    }
    // Which form of the row kernel the sweep and precompute! take depends on the shape alone: many short rows get several rows
    // per lane group (k_sep_sweep) once one row per group would make several times the resident wavefronts
    {
        const int64_t resident = (int64_t)num_cus * 32;
        const int64_t waves_nl = m_nl * grp_sweep / 64, waves_ext = m_ext * grp_sweep / 64;
        sweep_rows_per_group = dev.sweep_rows > 0 ? (dev.sweep_rows >= 4 ? 4 : dev.sweep_rows >= 2 ? 2 : 1)
                                                  : (waves_nl >= 16 * resident ? 4 : waves_nl >= 8 * resident ? 2 : 1);
        pre_multirow = waves_ext >= 16 * resident;
        stats["sweep_group"] = (double)grp_sweep;
        stats["sweep_rows_per_group"] = (blk_on || sb_on) ? 0.0 : (double)sweep_rows_per_group;
        stats["sweep_blocked"] = blk_on ? 1.0 : 0.0;
        stats["precompute_multirow"] = pre_multirow ? 1.0 : 0.0;
    }
    // algorithmic bytes of one evaluation pass over the NL rows (DESIGN.md "sweep bytes")
    sweep_bytes = (double)nnz_nl * (4 + 16) + 8.0 * (m_nl + 1) + 8.0 * n_lp + 8.0 * 4 * m_nl + 16.0 * m_nl;
    const size_t mm = (size_t)std::max<int64_t>(m_ext, 1);
    d_g.resize(mm, stream); d_bconst.resize(mm, stream); d_maxc.resize(mm, stream); d_nonfin.resize(mm, stream);
    d_jac.resize((size_t)nnz_ext + 1, stream);
    d_flag.resize(mm, stream); d_cnt.resize(mm, stream); d_rank.resize(mm, stream); d_cntscan.resize(mm, stream);
    d_lastcut.resize(mm, stream);
    d_xs.resize((size_t)n0 + 1, stream); d_ray.resize((size_t)n0 + 1, stream);
    d_flag.zero(stream); d_cnt.zero(stream);

    lapl("blocked copy + sweep buffers");
    // ---- tangent at the origin: linear rows and (linear) objective  model.jl:110-133
    d_xs.zero(stream);
    precompute_all(d_xs.p);
    // the LP rows of the linear constraints are written on the device (k_lin_rows): only the row pointers -- structural --
    // come from the host; the objective row's slice of (g, J) is all that travels back
    std::vector<int64_t> rp(1, 0);
    std::vector<int32_t> rc;                            // host-built rows (the epigraph cut at the vertex) follow the linear rows
    std::vector<double> rv, rlo, rhi;
    numcuts = 0;
    const int64_t n_lin = (int64_t)lin_rows.size();
    int64_t nnz_lin = 0;
    {
        rp.reserve((size_t)n_lin + 2);
        std::vector<int32_t> lr((size_t)n_lin);
        for (int64_t k = 0; k < n_lin; ++k) {
            const int64_t i = lin_rows[(size_t)k];
            lr[(size_t)k] = (int32_t)i;
            nnz_lin += h_rowptr[i + 1] - h_rowptr[i];
            rp.push_back(nnz_lin);
            numcuts += 1;                               // model.jl:77
        }
        lp_rowptr.resize((size_t)n_lin + 2, stream);
        KTN_HIP(hipMemcpyAsync(lp_rowptr.p, rp.data(), rp.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream));
        lp_col.resize((size_t)nnz_lin + 1, stream); lp_val.resize((size_t)nnz_lin + 1, stream);
        lp_lo.resize((size_t)n_lin + 1, stream); lp_hi.resize((size_t)n_lin + 1, stream);
        DBuf<int32_t> t_lr;
        t_lr.upload(lr, stream);
        launch_n(k_lin_rows, n_lin, stream, n_lin, t_lr.p, d_rowptr.p, d_col.p, d_jac.p, d_g.p, d_lb.p, d_ub.p, lp_rowptr.p, lp_col.p, lp_val.p, lp_lo.p,
                 lp_hi.p);
        check_launch();
        sync();
    }
    // objective row at the origin: g0[m0] and its Jacobian entries
    const int64_t ob = h_rowptr[m0], ol = h_rowptr[m0 + 1] - ob;
    std::vector<double> j0obj((size_t)std::max<int64_t>(ol, 1));
    double g0obj = 0.0;
    if (ol > 0) KTN_HIP(hipMemcpyAsync(j0obj.data(), d_jac.p + ob, (size_t)ol * sizeof(double), hipMemcpyDeviceToHost, stream));
    KTN_HIP(hipMemcpyAsync(&g0obj, d_g.p + m0, sizeof(double), hipMemcpyDeviceToHost, stream));
    sync();
    lapl("tangent at origin + LP rows (host)");
    std::vector<double> cvec(n_lp, 0.0);
    c0 = 0.0;
    if (prm.log_level > 0) { std::printf(obj_linear ? "objective is linear\n" : "objective is nonlinear\n"); std::fflush(stdout); }   // model.jl:127,135
    if (obj_linear) {
        // gencut(fsep, pt, (0,0), num_constr+1), drop the fictitious aux variable  model.jl:129-133
        for (int64_t e = h_rowptr[m0]; e < h_rowptr[m0 + 1]; ++e)
            if (h_col[e] < n0) cvec[h_col[e]] += j0obj[(size_t)(e - ob)];
        c0 = g0obj;
    } else {
        cvec[n0] = 1.0;                                 // @objective(m.linear_model, sense, y)  model.jl:139
        // initial epigraph cut at the bound-box vertex  model.jl:93-97,156-164
        bool ok = true;
        std::vector<double> vtx(n0 + 1, 0.0);
        for (int64_t j = 0; j < n0; ++j) {
            const double lo = lv[j], hi = uv[j];
            if (lo > hi) ok = false;
            const bool lf = std::isfinite(lo), uf = std::isfinite(hi);
            if (lf && uf) vtx[j] = (std::fabs(lo) <= std::fabs(hi)) ? lo : hi;   // GLPK non-basic rule
            else if (lf) vtx[j] = lo;
            else if (uf) vtx[j] = hi;
            else vtx[j] = 0.0;
        }
        if (!ok) std::fprintf(stderr, "WARNING: Problem variables insufficiently bounded!\n");      // model.jl:156-157
        if (ok && dist.rank == 0) {
            KTN_HIP(hipMemcpyAsync(d_xs.p, vtx.data(), (n0 + 1) * sizeof(double), hipMemcpyHostToDevice, stream));
            precompute_all(d_xs.p);
            std::vector<double> g1 = d_g.to_host(stream);
            vtx[n0] = g1[m0];                           // push!(vertex, eval_f(d, vertex))
            KTN_HIP(hipMemcpyAsync(d_xs.p, vtx.data(), (n0 + 1) * sizeof(double), hipMemcpyHostToDevice, stream));
            precompute_all(d_xs.p);
            g1 = d_g.to_host(stream);
            std::vector<double> j1 = d_jac.to_host(stream);
            double b = g1[m0];
            std::vector<double> coef;
            double mx = -kInf;
            bool finite = true;
            for (int64_t e = h_rowptr[m0]; e < h_rowptr[m0 + 1]; ++e) {
                coef.push_back(j1[e]);
                b += -vtx[h_col[e]] * j1[e];
                if (!(j1[e] <= mx)) mx = (j1[e] != j1[e]) ? j1[e] : std::max(mx, j1[e]);
                if (!std::isfinite(j1[e])) finite = false;
            }
            if (padzero[m0] && !(mx != mx)) mx = std::max(mx, 0.0);
            for (auto& cf : coef) if (cf + prm.cut_coef_rng < mx) cf = 0.0;   // round_coefs
            if (!finite) {
                std::fprintf(stderr, "WARNING: Nonlinear constraint or objective likely undefined within domain\n");   // model.jl:70
                status = KTN_STATUS_ERROR;              // _addcut: warn + :Error, no row added
            } else {
                for (int64_t e = h_rowptr[m0]; e < h_rowptr[m0 + 1]; ++e) {
                    rc.push_back(h_col[e]);
                    rv.push_back(coef[e - h_rowptr[m0]]);
                }
                rp.push_back(nnz_lin + (int64_t)rc.size());
                rlo.push_back(h_lb[m0] - b);
                rhi.push_back(h_ub[m0] - b);
                numcuts += 1;
            }
        }
    }
    lapl("objective");
    // ---- LP: the linear rows are in place (device); rows built on the host (the epigraph cut at the vertex) are appended
    M = n_lin + (int64_t)rlo.size();
    NNZ = nnz_lin + (int64_t)rc.size();
    if (!rlo.empty()) {
        lp_rowptr.resize((size_t)M + 1, stream); lp_col.resize((size_t)NNZ + 1, stream); lp_val.resize((size_t)NNZ + 1, stream);
        lp_lo.resize((size_t)M, stream); lp_hi.resize((size_t)M, stream);
        KTN_HIP(hipMemcpyAsync(lp_rowptr.p + n_lin + 1, rp.data() + n_lin + 1, rlo.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream));
        KTN_HIP(hipMemcpyAsync(lp_col.p + nnz_lin, rc.data(), rc.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        KTN_HIP(hipMemcpyAsync(lp_val.p + nnz_lin, rv.data(), rv.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        KTN_HIP(hipMemcpyAsync(lp_lo.p + n_lin, rlo.data(), rlo.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        KTN_HIP(hipMemcpyAsync(lp_hi.p + n_lin, rhi.data(), rhi.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        sync();
    }
    lp_rowptr.n = (size_t)M + 1; lp_col.n = lp_val.n = (size_t)NNZ; lp_lo.n = lp_hi.n = (size_t)M;
    lp_y.resize((size_t)M, stream); lp_y.zero(stream);
    lp_c.upload(cvec, stream); lp_l.upload(lv, stream); lp_u.upload(uv, stream);
    lp_x.resize((size_t)n_lp, stream); lp_x.zero(stream);
    M_base = M; NNZ_base = NNZ; numcuts_base = numcuts; M_lin = n_lin;
    n_longc = 0; col_len_max = -1; col_scan_rows = 0; col_removed_rows = 0;      // (a new problem: scan its columns at the first solve)
    {
        // room for three sweeps' worth of cuts (each sweep adds at most min(m_nl, cut cap) rows)
        int64_t per_sweep = m_nl;
        if (prm.cut_cap_factor > 0.0)
            per_sweep = std::min<int64_t>(m_nl, std::max<int64_t>((int64_t)(prm.cut_cap_factor * (double)n_lp), prm.cut_cap_min));
        const double avg_nl = m_nl ? (double)nnz_nl / (double)m_nl : 0.0;
        const int64_t rows = M + 3 * per_sweep;
        const int64_t nz = NNZ + (int64_t)(3.0 * (double)per_sweep * avg_nl);
        if ((double)rows * 200.0 + (double)nz * 60.0 < 64e9) reserve_lp(rows, nz);     // stay far below the 288 GB
        d_violslots.reserve((size_t)std::max<int64_t>(m_nl, 1), stream);
    }
    sync();
    lapl("LP upload + reserve");
    loaded = true;
    const int keep_status = status;
    reset();
    lapl("reset");
    if (keep_status == KTN_STATUS_ERROR) status = KTN_STATUS_ERROR;
    // row-sharded: what steers the sequence of collectives must be the same on every rank -- the number of NL rows (a rank
    // whose shard has none would otherwise take the pure-LP tolerance and leave the others' restart pattern) and the
    // load-time error (the vertex cut of the epigraph row is built on rank 0 only)
    m_nl_global = m_nl;
    if (row_sharded()) {
        double cnt = (double)m_nl, bad = (status == KTN_STATUS_ERROR) ? 1.0 : 0.0;
        allreduce_host(&cnt, 1, 0);
        allreduce_host(&bad, 1, 1);
        m_nl_global = (int64_t)(cnt + 0.5);
        if (bad > 0.0) status = KTN_STATUS_ERROR;
    }
}

void Engine::reset() {
    M = M_base; NNZ = NNZ_base; numcuts = numcuts_base;
    lp_rowptr.n = (size_t)M + 1; lp_col.n = (size_t)NNZ; lp_val.n = (size_t)NNZ;
    lp_lo.n = lp_hi.n = lp_y.n = (size_t)M;
    lp_y.zero(stream);
    if (!reset_keeps_x) lp_x.zero(stream);      // (a warm device launch starts from the x of the last one: ktn_optimize_blocks_ex)
    std::vector<int64_t> neg1((size_t)std::max<int64_t>(m_ext, 1), -1);
    d_lastcut.upload(neg1, stream);
    d_age.resize((size_t)std::max<int64_t>(M, 1), stream);
    d_age.zero(stream);
    lp_dirty = true; ++lp_version; ++lp_epoch; have_omega = false; have_precompute = false; sharded_rows = false; scal_rows = 0; smax_rows = 0; n_longc = 0; col_len_max = -1; col_scan_rows = 0; col_removed_rows = 0;
    blocks_built_rows = -1;
    kkt_solved = false; kkt_arena = false; kkt_cached = false; feas_cached = false; feas_blk_cached = false;
    if (d_blkomega.n) d_blkomega.zero(stream);
    if (ds_valid.n) ds_valid.zero(stream);
    dense_credit = dense_run = 0;
    md_valid = false; mid_credit = mid_run = 0; mid_backoff = mid_backoff_len = 0;
    if (glists) KTN_HIP(hipMemsetAsync(d_glast.p, 0xFF, d_glast.n * sizeof(int64_t), stream));
    last_sweep_cuts = 0;
    power_v.n = 0;
    status = KTN_STATUS_NONE; lp_status = KTN_STATUS_OPTIMAL;
    iter = 0; soltime = 0.0; objval = std::numeric_limits<double>::quiet_NaN();
    last_maxviol = 1e300; obj_prev = kInf; allsat = false; begun = false; tight_done = false;
    log_cuts_lastprnt = 0; log_max_viol = 0; purged_total = 0;
    polishing = false; polish_done = false; polish_count = 0; best_viol = kInf; best_obj = 0.0; cert_target = 0.0;
    lp_sols.clear();
    screened_out = false; reopened = false;
    sync();
}

NlpDev Engine::nlp_view() {
    NlpDev P;
    P.rowptr = d_rowptr.p; P.col = d_col.p; P.colk = d_colk.p; P.pp = d_pp.p;
    P.rconst = d_rconst.p; P.row_kind = d_rowkind.p; P.pad_zero = d_padzero.p; P.lb = d_lb.p; P.ub = d_ub.p;
    P.node_ptr = d_nodeptr.p; P.node_op = d_nodeop.p; P.node_a = d_nodea.p; P.node_b = d_nodeb.p;
    P.node_c = d_nodec.p; P.node_val = d_nodeval.p; P.node_adj = d_nodeadj.p;
    return P;
}

SweepOut Engine::sweep_view() {
    SweepOut O;
    O.g = d_g.p; O.jac = d_jac.p; O.bconst = d_bconst.p; O.maxc = d_maxc.p; O.nonfin = d_nonfin.p;
    O.flag = d_flag.p; O.cnt = d_cnt.p; O.maxviol = d_scal.p; O.any_nonfin = d_anynf.p;
    return O;
}

// ================================================================ separator =====
// precompute! for every row of the extended structure (jac materialised)
void Engine::precompute_all(const double* d_x) {
    NlpDev P = nlp_view();
    SweepOut O = sweep_view();
    // many short rows: the R-rows-per-lane-group form of the sweep with the Jacobian store (same sums, same bits); the
    // selection is the sweep's, made once in loadproblem (pre_multirow)
    if (pre_multirow) {
        with_value<8, 16, 32, 64>(grp_sweep, [&](auto g) {            // (grp_sweep >= 8: loadproblem)
            launch(k_sep_sweep<g(), 4, true>, group_grid(m_ext, g(), 4), kBlock, 0, stream, P, d_allrows.p, m_ext, d_x, 0.0, O);
        });
    } else {
        with_group(grp_sweep, [&](auto g) { launch(k_sep_eval<g()>, group_grid(m_ext, g()), kBlock, 0, stream, P, d_allrows.p, m_ext, d_x, 0.0, 1, 0, O); });
    }
    if (n_longev > 0)
        launch(k_sep_eval_long, (unsigned)n_longev, 1024, 0, stream, P, d_longev_rows.p, d_longev_slots.p, d_x, 0.0, 0, O);
    launch_quad(false, d_x, 0.0);
    launch_n(k_tape_eval, (int64_t)d_tapeint_all.n, stream, P, d_tapeint_all.p, (int64_t)d_tapeint_all.n, d_x, O);
    if (n_host > 0) host_eval(d_x);
    // cut constants / maxima of tape rows from the materialised Jacobian (flags unused here)
    KTN_HIP(hipMemsetAsync(d_scal.p, 0, sizeof(double), stream));
    KTN_HIP(hipMemsetAsync(d_anynf.p, 0, sizeof(int32_t), stream));
    // rows of the classed shapes: value, Jacobian and those constants / maxima in one pass (flags by row, as k_gj_stats' here)
    launch_tape_classed(false, d_tc_mrow.p, d_x, 0.0);
    if (tc_rows == 0 || d_tapeint_all.n > 0 || n_host > 0)
        launch_n(k_gj_stats, m_ext, stream, P, d_allrows.p, m_ext, d_x, 0.0, (int)KTN_ROW_TAPE, (const uint8_t*)(tc_rows > 0 ? d_tc_rowflag.p : nullptr), O);
    check_launch();
}

// ================================================================ KKT report (kkt.hpp) =====
// Column mirror of the extended structure (rows 0 .. m0, the objective row last; columns 0 .. n0), by the radix sort the LP's
// mirror uses: keys (col << 32 | row) in CSR order (k_kkt_keys: a thread per entry), a stable sort on the column bits gives row-ordered columns.  Built on the
// first getter after ktn_loadproblem, never changed until the next one.
void Engine::kkt_build_mirror() {
    if (kkt_mirror) return;
    if (nnz_ext >= ((int64_t)1 << 32)) throw Error(KTN_E_UNSUPPORTED, "KKT report: 2^32 Jacobian entries and more are not mirrored");
    const int64_t nc = n0 + 1;
    d_kkt_cptr.resize((size_t)nc + 1, stream);
    d_kkt_crow.resize((size_t)nnz_ext + 1, stream); d_kkt_cperm.resize((size_t)nnz_ext + 1, stream);
    DBuf<int64_t> cnt;
    DBuf<uint64_t> kin, kout;
    DBuf<uint32_t> pin, pout;
    DBuf<char> tmp;
    cnt.resize((size_t)nc + 1, stream); cnt.zero(stream);
    if (nnz_ext > 0) {
        kin.resize((size_t)nnz_ext, stream); kout.resize((size_t)nnz_ext, stream);
        pin.resize((size_t)nnz_ext, stream); pout.resize((size_t)nnz_ext, stream);
        launch_n(k_kkt_keys, nnz_ext, stream, nnz_ext, m_ext, d_rowptr.p, d_col.p, kin.p, pin.p, cnt.p);
        check_launch();
    }
    exclusive_scan(cnt.p, d_kkt_cptr.p, (size_t)nc + 1);
    if (nnz_ext > 0) {
        int bits = 1;
        while (((int64_t)1 << bits) < nc + 1 && bits < 31) ++bits;
        const size_t need = sort_pairs_temp_bytes((size_t)nnz_ext);
        tmp.resize(need + 16, stream);
        KTN_HIP(sort_pairs_u64_u32(tmp.p, need, kin.p, kout.p, pin.p, pout.p, (size_t)nnz_ext, 32, 32 + bits, stream));
        launch_n(k_csc_rows_perm, nnz_ext, stream, nnz_ext, kout.p, pout.p, d_kkt_crow.p, d_kkt_cperm.p);
        check_launch();
    }
    sync();                                             // the temporaries are freed on leaving the scope
    kkt_mirror = true;
    stats["kkt_mirror_bytes"] = 8.0 * (double)(nc + 1) + 8.0 * (double)nnz_ext;
}

void Engine::kkt_compute() {
    KTN_REQUIRE(loaded, "KKT report: no problem loaded");
    if (kkt_foreign())
        throw Error(KTN_E_UNSUPPORTED, "KKT report: a row-sharded handle or one with a cut exchange owns only a part of the cut lists");
    KTN_REQUIRE(kkt_solved, "KKT report: no LP solve since the problem was loaded or reset, or since rows were appended, truncated or purged");
    if (!kkt_arena && !lists_ok())
        throw Error(KTN_E_UNSUPPORTED, "KKT report: rows were appended from the host without cut lists (ktn_lp_enable_global_lists)");
    if (kkt_cached && kkt_key_version == lp_version && kkt_key_solves == kkt_solves) return;
    kkt_cached = false;
    kkt_build_mirror();
    const double sgn = (sense == KTN_MAX) ? -1.0 : 1.0;
    const size_t mm = (size_t)std::max<int64_t>(m_ext, 1);
    d_kkt_d.resize(mm, stream); d_kkt_z.resize((size_t)n0 + 1, stream); d_kkt_t.resize((size_t)(m0 + n0) + 1, stream);
    d_kkt_out.resize(8, stream);
    // ---- 1. constraint duals
    KktSrc S{};
    KTN_HIP(hipMemsetAsync(d_kkt_out.p + 4, 0, 2 * sizeof(double), stream));      // k_row_duals: entries zeroed on an infinite side, their largest
    const bool epi = !obj_linear && !kkt_arena;
    if (kkt_arena) {
        S.y = e_y.p; S.a_last = e_last.p; S.a_prev = e_prev.p; S.arena = d_ar.p;
        S.blk_lin = d_blklin.p; S.blk_nl = d_blknl.p; S.nb = (int64_t)h_ar_row0.size();
        launch_n(k_row_duals<true>, m0, stream, m0, d_kkt_rowmap.p, S, sgn, (int64_t)0, (int64_t)0, (int64_t)-1, (double*)nullptr, (const double*)d_lb.p, (const double*)d_ub.p, (double*)nullptr, d_kkt_d.p);
    } else {
        // what ktn_lp_get_duals returns: the true-cost multipliers of an exact mid-size solve while they stand, lp_y otherwise
        S.y = (!dev.raw_duals && mid_true_duals(nullptr)) ? md_y.p : lp_y.p;
        S.heads = list_heads(); S.prev = d_cutprev.p; S.n_heads = list_count(); S.n_rows = M;
        launch_n(k_row_duals<false>, std::max<int64_t>(m0, 1), stream, m0, d_kkt_rowmap.p, S, sgn, M_lin, M_base, epi ? m_nl - 1 : (int64_t)-1,
                 epi ? d_kkt_out.p + 2 : (double*)nullptr, (const double*)d_lb.p, (const double*)d_ub.p, d_kkt_out.p + 4, d_kkt_d.p);
    }
    check_launch();
    // ---- 2. g and J of every row at x* = lp_x, into buffers of the report's own: what ktn_sep_* and the certificate read stays
    d_kkt_x.resize((size_t)n0 + 1, stream); d_kkt_x.zero(stream);
    KTN_HIP(hipMemcpyAsync(d_kkt_x.p, lp_x.p, (size_t)std::min<int64_t>(n_lp, n0 + 1) * sizeof(double), hipMemcpyDeviceToDevice, stream));
    d_kkt_g.resize(mm, stream); d_kkt_bconst.resize(mm, stream); d_kkt_maxc.resize(mm, stream); d_kkt_nonfin.resize(mm, stream);
    d_kkt_jac.resize((size_t)nnz_ext + 1, stream); d_kkt_jac.zero(stream);
    auto swap_bufs = [&]() { d_g.swap(d_kkt_g); d_jac.swap(d_kkt_jac); d_bconst.swap(d_kkt_bconst); d_maxc.swap(d_kkt_maxc); d_nonfin.swap(d_kkt_nonfin); };
    swap_bufs();
    try {
        precompute_all(d_kkt_x.p);
    } catch (...) {
        swap_bufs();
        throw;
    }
    swap_bufs();
    // ---- 3. reduced costs
    int G = dev.kkt_group;
    if (!(G == 4 || G == 8 || G == 16 || G == 32 || G == 64)) G = pick_group((double)nnz_ext / (double)(n0 + 1));
    with_group(G, [&](auto g) {
        launch(k_lagr_grad<g()>, group_grid(n0, g()), kBlock, 0, stream, n0, (int32_t)m0, d_kkt_cptr.p, d_kkt_crow.p, d_kkt_cperm.p, d_kkt_jac.p, d_kkt_d.p,
               d_kkt_z.p);
    });
    // ---- 4. the bound
    launch_n(k_dual_terms, m0 + n0, stream, m0, n0, sgn, d_kkt_rowmap.p, kkt_n_lin, d_kkt_d.p, d_kkt_z.p, d_kkt_g.p, d_lb.p, d_ub.p, d_kkt_x.p, lp_l.p, lp_u.p,
             d_kkt_t.p);
    if (m0 + n0 > 0) launch(k_sum_partial, kRedBlocks, kBlock, 0, stream, m0 + n0, d_kkt_t.p, partials.p);
    else KTN_HIP(hipMemsetAsync(partials.p, 0, kRedBlocks * sizeof(double), stream));
    launch(k_dual_final, 1, 64, 0, stream, partials.p, (int)kRedBlocks, d_kkt_g.p, d_kkt_x.p, m0, n0, d_kkt_out.p);
    check_launch();
    h_kkt_d.assign((size_t)m0, 0.0); h_kkt_z.assign((size_t)n0, 0.0);
    std::vector<double> out(d_kkt_out.n, 0.0);
    if (m0 > 0) KTN_HIP(hipMemcpyAsync(h_kkt_d.data(), d_kkt_d.p, (size_t)m0 * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (n0 > 0) KTN_HIP(hipMemcpyAsync(h_kkt_z.data(), d_kkt_z.p, (size_t)n0 * sizeof(double), hipMemcpyDeviceToHost, stream));
    d_kkt_out.download(out.data(), out.size(), stream);
    // Min form: LB = f_min - T with f_min = sgn f; mirrored back: bound = sgn LB, gap = T in both senses
    const double T = out[0], f = out[1];
    kkt_bound = sgn * (sgn * f - T);
    kkt_gap = T;
    h_kkt_blk.clear();                                  // (per instance: kkt_blocks, on ktn_blocks_get_dual_bounds only)
    stats["kkt_evals"] += 1.0;
    stats["kkt_epi_dual"] = epi ? out[2] : std::numeric_limits<double>::quiet_NaN();
    stats["kkt_group"] = (double)G;
    stats["kkt_clamped_duals"] = out[4]; stats["kkt_clamped_max"] = out[5];      // (0, 0 after a device launch of the batch loop: the arenas are not clamped)
    kkt_key_version = lp_version; kkt_key_solves = kkt_solves; kkt_cached = true;
}

// The instances' ranges of a fused batch -- linear rows, NL slots, columns, each grouped by instance, instance after instance -- and
// the caller rows of each instance, found once per ktn_set_blocks (kkt_seg_ok); shared by kkt_blocks and the feasible points per
// instance (feas.hip).
void Engine::kkt_build_seg() {
    const int64_t nb = n_blocks;
    if (kkt_seg_ok) return;
    std::vector<int64_t> seg((size_t)nb * 6), bl((size_t)nb + 1, 0), bn((size_t)nb + 1, 0), bptr((size_t)nb + 1, 0);
    std::vector<int32_t> blk_of((size_t)std::max<int64_t>(m0, 1), 0);
    auto block_of_col = [&](int64_t c) { return (int64_t)(std::upper_bound(h_blkcol.begin(), h_blkcol.end(), c) - h_blkcol.begin()) - 1; };
    std::vector<char> is_nl((size_t)std::max<int64_t>(m0, 1), 0);
    for (auto r : h_nlrows) if (r < m0) is_nl[(size_t)r] = 1;
    int64_t prev_l = 0, prev_n = 0;
    bool grouped = true;
    for (int64_t i = 0; i < m0; ++i) {
        if (h_rowptr[i + 1] == h_rowptr[i]) { grouped = false; break; }
        const int64_t b = std::min<int64_t>(std::max<int64_t>(block_of_col(h_col[(size_t)h_rowptr[i]]), 0), nb - 1);
        int64_t& prev = is_nl[(size_t)i] ? prev_n : prev_l;
        if (b < prev) { grouped = false; break; }
        prev = b;
        (is_nl[(size_t)i] ? bn : bl)[(size_t)b + 1] += 1;
        blk_of[(size_t)i] = (int32_t)b; bptr[(size_t)b + 1] += 1;
    }
    if (!grouped) throw Error(KTN_E_UNSUPPORTED, "KKT report: the rows of the fused batch are not grouped by instance");
    for (int64_t b = 0; b < nb; ++b) { bl[(size_t)b + 1] += bl[(size_t)b]; bn[(size_t)b + 1] += bn[(size_t)b]; bptr[(size_t)b + 1] += bptr[(size_t)b]; }
    for (int64_t b = 0; b < nb; ++b) {
        int64_t* s = seg.data() + 6 * b;
        s[0] = bl[(size_t)b]; s[1] = bl[(size_t)b + 1];
        s[2] = kkt_n_lin + bn[(size_t)b]; s[3] = kkt_n_lin + bn[(size_t)b + 1];
        s[4] = m0 + h_blkcol[(size_t)b]; s[5] = m0 + std::min<int64_t>(h_blkcol[(size_t)b + 1], n0);
    }
    // the caller rows of each instance, ascending (the feasible point's per-instance verification, feas.hpp)
    std::vector<int32_t> brows((size_t)std::max<int64_t>(m0, 1), 0);
    {
        std::vector<int64_t> cur(bptr.begin(), bptr.end() - 1);
        for (int64_t i = 0; i < m0; ++i) brows[(size_t)cur[(size_t)blk_of[(size_t)i]]++] = (int32_t)i;
    }
    d_kkt_seg.upload(seg, stream);
    d_kkt_browptr.upload(bptr, stream);
    d_kkt_brows.upload(brows, stream);
    sync();
    h_kkt_seg = seg;
    kkt_seg_ok = true;
}

// The bound per instance of a fused batch (ktn_blocks_get_dual_bounds) from the terms the last evaluation left in d_kkt_t: one
// launch of k_dual_bound, no re-evaluation.
void Engine::kkt_blocks() {
    kkt_compute();
    const int64_t nb = n_blocks;
    KTN_REQUIRE(nb > 0, "KKT report: no blocks set (ktn_set_blocks)");
    if ((int64_t)h_kkt_blk.size() == 2 * nb) return;
    const double sgn = (sense == KTN_MAX) ? -1.0 : 1.0;
    kkt_build_seg();
    d_kkt_blk.resize((size_t)(2 * nb), stream);
    launch(k_dual_bound, (unsigned)nb, kBlock, 0, stream, d_kkt_seg.p, d_kkt_t.p, lp_c.p, d_kkt_x.p, m0, d_kkt_blk.p);
    check_launch();
    const std::vector<double> out = d_kkt_blk.to_host(stream);
    h_kkt_blk.assign((size_t)(2 * nb), 0.0);
    for (int64_t b = 0; b < nb; ++b) {
        const double Tb = out[(size_t)(2 * b)], fb = out[(size_t)(2 * b + 1)];
        h_kkt_blk[(size_t)(2 * b)] = sgn * (sgn * fb - Tb);
        h_kkt_blk[(size_t)(2 * b + 1)] = Tb;
    }
}

// the batched {isconstrsat, gencut, round_coefs, _addcut} over the NL rows
void Engine::sweep(const double* d_x, double f_tol, int64_t* nviol_out, double* maxviol_out, bool* nonfinite_out) {
    auto t0 = std::chrono::steady_clock::now();
    *nviol_out = 0;
    *maxviol_out = 0.0;
    *nonfinite_out = false;
    last_sweep_cuts = 0;
    stats["sweeps"] += 1.0;
    if (m_nl == 0) return;
    if (esh_mode() && !esh_ready) esh_prepare();
    NlpDev P = nlp_view();
    SweepOut O = sweep_view();
    KTN_HIP(hipMemsetAsync(d_scal.p, 0, sizeof(double), stream));
    KTN_HIP(hipMemsetAsync(d_anynf.p, 0, sizeof(int32_t), stream));
    hipEvent_t e0 = nullptr, e1 = nullptr;         // profile: the separable evaluation carries its own start / stop events
    if (prm.profile) {
        const size_t ea = ev_get(), eb = ev_get();
        e0 = ev_pool[ea]; e1 = ev_pool[eb];
        ev_recs.push_back({2, ea, eb, sweep_bytes});
    }
    if (blk_on) {
        // long rows: column-blocked evaluation through LDS, then the block-order combination
        with_value<1, 2, 0>(blk_cfg, [&](auto c) {       // KTN_BLK_CFG: tuning variants kept for the next round's experiments
            constexpr int G = c() == 0 ? 8 : 16, BC = c() == 2 ? 16384 : 8192, BS = c() == 2 ? 1024 : 512;
            launch_ev(k_sep_eval_blk<G, BC, BS, 4>, (unsigned)(num_cus * blk_wg_per_cu), BS, 0, stream, e0, nullptr, d_bcolk.p, d_bpp.p, d_bseg.p, d_bkind.p,
                      m_nl, blk_nb, d_x, n_lp, d_part.p);
        });
        launch_ev(k_sep_combine, grid_n(m_nl), kBlock, 0, stream, nullptr, e1, d_slots.p, m_nl, blk_nb, d_part.p, f_tol, O);
    } else if (sb_on) {
        if (!sb_lds_set) {
            KTN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sep_sweep_batch), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSbLds));
            sb_lds_set = true;
        }
        SbView V{d_sbck.p, d_sbrow.p, d_sbpp.p, d_sbseg.p, sb_nb};
        launch_ev(k_sep_sweep_batch, (unsigned)sb_batches, kSbThreads, kSbLds, stream, e0, e1, V, P, d_nlrows.p, m_nl, d_x, n_lp, f_tol, O);
    } else {
        // many short rows: several rows per lane group (k_sep_sweep) once one row per group would make more wavefronts
        // than the chip holds several times over; small sweeps keep one row per group and all the parallelism (the
        // choice is made once in loadproblem)
        const int R = sweep_rows_per_group;
        with_value<4, 2, 1>(R >= 4 ? 4 : R >= 2 ? 2 : 1, [&](auto r) {
            with_group(grp_sweep, [&](auto g) {
                constexpr int G = g(), RR = r();
                if constexpr (RR == 1) launch_ev(k_sep_eval<G>, group_grid(m_nl, G), kBlock, 0, stream, e0, e1, P, d_nlrows.p, m_nl, d_x, f_tol, 0, 1, O);
                else launch_ev(k_sep_sweep<G, RR>, group_grid(m_nl, G, RR), kBlock, 0, stream, e0, e1, P, d_nlrows.p, m_nl, d_x, f_tol, O);
            });
        });
    }
    if (n_longev_nl > 0)
        launch(k_sep_eval_long, (unsigned)n_longev_nl, 1024, 0, stream, P, d_longev_nlrows.p, d_longev_nlslots.p, d_x, f_tol, 1, O);
    launch_quad(true, d_x, f_tol);
    if (n_tape_nl > 0 || n_host_nl > 0) {
        // tape rows: the classed shapes in one launch (k_tape_classed, statistics folded in), the others through the interpreter
        // and k_gj_stats.  profile: the tape part has an event record of its own (tape_eval_*; sweep_eval_* stays the separable kernel)
        size_t ta = 0, tb = 0;
        const bool ev = prm.profile && n_tape_nl > 0;
        if (ev) { ta = ev_get(); tb = ev_get(); KTN_HIP(hipEventRecord(ev_pool[ta], stream)); }
        const int64_t n_int = (int64_t)d_tapeint_nl.n;
        launch_n(k_tape_eval, n_int, stream, P, d_tapeint_nl.p, n_int, d_x, O);
        if (n_host_nl > 0) host_eval(d_x);
        launch_tape_classed(true, d_tc_mslot.p, d_x, f_tol);
        if (n_int > 0 || n_host_nl > 0)
            launch_n(k_gj_stats, m_nl, stream, P, d_nlrows.p, m_nl, d_x, f_tol, (int)KTN_ROW_TAPE, (const uint8_t*)(tc_rows_nl > 0 ? d_tc_rowflag.p : nullptr),
                     O);
        if (ev) { KTN_HIP(hipEventRecord(ev_pool[tb], stream)); ev_recs.push_back({4, ta, tb, tape_bytes}); }
    }
    check_launch();
    exclusive_scan(d_flag.p, d_rank.p, (size_t)m_nl);
    exclusive_scan(d_cnt.p, d_cntscan.p, (size_t)m_nl);
    int64_t tail[4];
    double mv = 0.0;
    int32_t anynf = 0;
    if (h_chk_dev) {                               // one thread gathers the six scalars into pinned host memory
        double* ht = h_chk + 2 * kChkQ;
        launch(k_host_tail, 1, 1, 0, stream, h_chk_dev + 2 * kChkQ, d_flag.p + (m_nl - 1), d_rank.p + (m_nl - 1), d_cnt.p + (m_nl - 1),
               d_cntscan.p + (m_nl - 1), (const double*)d_scal.p, (const int32_t*)d_anynf.p, (const int32_t*)nullptr);
        sync();
        for (int k = 0; k < 4; ++k) tail[k] = (int64_t)ht[k];
        mv = ht[4]; anynf = (int32_t)ht[5];
    } else {
        KTN_HIP(hipMemcpyAsync(&tail[0], d_flag.p + (m_nl - 1), 8, hipMemcpyDeviceToHost, stream));
        KTN_HIP(hipMemcpyAsync(&tail[1], d_rank.p + (m_nl - 1), 8, hipMemcpyDeviceToHost, stream));
        KTN_HIP(hipMemcpyAsync(&tail[2], d_cnt.p + (m_nl - 1), 8, hipMemcpyDeviceToHost, stream));
        KTN_HIP(hipMemcpyAsync(&tail[3], d_cntscan.p + (m_nl - 1), 8, hipMemcpyDeviceToHost, stream));
        KTN_HIP(hipMemcpyAsync(&mv, d_scal.p, 8, hipMemcpyDeviceToHost, stream));
        KTN_HIP(hipMemcpyAsync(&anynf, d_anynf.p, 4, hipMemcpyDeviceToHost, stream));
        sync();
    }
    if (prm.profile) ev_flush();
    int64_t V = tail[0] + tail[1], nnzV = tail[2] + tail[3];
    *nviol_out = V;                // the stop rule counts EVERY violated row (model.jl:273-283)
    *maxviol_out = mv;
    // Deepest-cut selection: an LP vertex is supported by at most n_lp rows, so when far more rows than that are
    // violated only the cut_cap_factor * n_lp deepest get a cut this iteration (the reference cuts every violated
    // row; with 1e6 NL rows over 1e5 variables that makes the LP 10x larger than it needs to be).  Ties at the
    // threshold are all kept.  Never triggers on the reference's own test models.
    int64_t cap = (prm.cut_cap_factor > 0.0) ? std::max<int64_t>((int64_t)(prm.cut_cap_factor * (double)n_lp), prm.cut_cap_min) : 0;
    if (cap > 0 && row_sharded()) cap = std::max<int64_t>(cap / dist.world, 1);      // every rank selects among ITS rows
    if (cap > 0 && V > cap && !anynf) {
        d_dkeys.resize((size_t)m_nl, stream); d_dsorted.resize((size_t)m_nl, stream);
        launch_n(k_depth_keys, m_nl, stream, P, d_nlrows.p, m_nl, d_g.p, d_flag.p, d_dkeys.p);
        const size_t need = sort_keys_desc_temp_bytes((size_t)m_nl);
        d_sorttmp.resize(need + 16, stream);
        KTN_HIP(sort_keys_desc_u64(d_sorttmp.p, need, d_dkeys.p, d_dsorted.p, (size_t)m_nl, stream));
        launch_n(k_depth_reflag, m_nl, stream, m_nl, d_dkeys.p, d_dsorted.p, cap, d_flag.p, d_cnt.p);
        check_launch();
        exclusive_scan(d_flag.p, d_rank.p, (size_t)m_nl);
        exclusive_scan(d_cnt.p, d_cntscan.p, (size_t)m_nl);
        KTN_HIP(hipMemcpyAsync(&tail[0], d_flag.p + (m_nl - 1), 8, hipMemcpyDeviceToHost, stream));
        KTN_HIP(hipMemcpyAsync(&tail[1], d_rank.p + (m_nl - 1), 8, hipMemcpyDeviceToHost, stream));
        KTN_HIP(hipMemcpyAsync(&tail[2], d_cnt.p + (m_nl - 1), 8, hipMemcpyDeviceToHost, stream));
        KTN_HIP(hipMemcpyAsync(&tail[3], d_cntscan.p + (m_nl - 1), 8, hipMemcpyDeviceToHost, stream));
        sync();
        V = tail[0] + tail[1];
        nnzV = tail[2] + tail[3];
        stats["cut_selections"] += 1.0;
        stats["cuts_skipped"] += (double)(*nviol_out - V);
    }
    if (anynf) {   // model.jl:69-73: "Nonlinear constraint or objective likely undefined within domain"
        std::fprintf(stderr, "WARNING: Nonlinear constraint or objective likely undefined within domain\n");
        *nonfinite_out = true;
        return;
    }
    if (V > 0) {
        if (esh_mode()) esh_search(d_x, f_tol);     // (esh.hip: moves the selected rows' cuts to x_b)
        lp_rowptr.resize((size_t)(M + V + 1), stream);
        lp_lo.resize((size_t)(M + V), stream);
        lp_hi.resize((size_t)(M + V), stream);
        lp_y.resize((size_t)(M + V), stream);
        d_cutprev.resize((size_t)(M + V), stream);
        d_age.resize((size_t)(M + V), stream);
        KTN_HIP(hipMemsetAsync(d_age.p + M, 0, (size_t)V * sizeof(int32_t), stream));
        lp_col.resize((size_t)(NNZ + nnzV), stream);
        lp_val.resize((size_t)(NNZ + nnzV), stream);
        d_violslots.resize((size_t)V, stream);
        LpRows L = lp_view();
        launch_n(k_compact, m_nl, stream, P, d_nlrows.p, m_nl, d_flag.p, d_rank.p, d_cntscan.p, d_bconst.p, M, NNZ, L, d_violslots.p, d_lastcut.p, d_cutprev.p,
                 (int)(prm.lp_dual_inherit && !glists));
        if (esh_mode()) esh_emit(d_x, V);
        else with_group(grp_sweep, [&](auto g) {
            launch(k_emit<g()>, group_grid(V, g()), kBlock, 0, stream, P, d_nlrows.p, d_violslots.p, V, d_x, d_jac.p, d_maxc.p, prm.cut_coef_rng, 1, M, L);
        });
        check_launch();
        M += V;
        NNZ += nnzV;
        numcuts += V;
        last_sweep_cuts = V;
        lp_dirty = true; ++lp_version;
    }
    sync();
    stats["sep_time_s"] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// sweep + (row-sharded) the stop rule's quantities over all ranks: number of violated rows, largest violation, error flag
void Engine::global_sweep(const double* d_x, double f_tol, int64_t* nviol, double* maxviol, bool* nonfinite) {
    sweep(d_x, f_tol, nviol, maxviol, nonfinite);
    if (!row_sharded()) return;
    double v[2] = {(double)*nviol, *nonfinite ? 1.0 : 0.0};
    allreduce_host(v, 2, 0);
    double mv = *maxviol;
    allreduce_host(&mv, 1, 1);
    *nviol = (int64_t)(v[0] + 0.5);
    *nonfinite = v[1] > 0.0;
    *maxviol = mv;
}

}  // namespace ktn
