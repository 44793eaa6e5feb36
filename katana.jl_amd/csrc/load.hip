// load.hip -- loadproblem! (src/model.jl:81-173) as a list of stages, and reset  (struct Engine: engine.hpp; the index arithmetic
// that needs neither the engine nor the device: load_host.hpp)
#include <cstring>

#include "engine.hpp"
#include "launch.hpp"
#include "kernels.hpp"
#include "tape_classes.hpp"
#include "dense_lp.hpp"      // kDenseBig alone (has_big_bound)
#include "load_host.hpp"

namespace ktn {

static_assert(sizeof(HostDouble2) == sizeof(double2) && alignof(HostDouble2) == alignof(double2), "HostDouble2 is uploaded as double2");
static_assert(sizeof(HostInt4) == sizeof(int4) && alignof(HostInt4) == alignof(int4), "HostInt4 is uploaded as int4");

// KTN_DEBUG_LOAD: time since the last lap, the stream drained first (DESIGN.md section 14 quotes the labels)
struct LoadLap {
    bool on = false;
    hipStream_t stream = nullptr;
    std::chrono::steady_clock::time_point t0;
    void operator()(const char* what) {
        if (!on) return;
        (void)hipStreamSynchronize(stream);
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[load] %-28s %.2f ms\n", what, 1e3 * std::chrono::duration<double>(now - t0).count());
        t0 = now;
    }
};

// What the stages of one loadproblem hand to each other and nobody needs afterwards: vectors and a few counts.
struct LoadScratch {
    // the extended structure beside h_rowptr / h_col / h_rowkind: per Jacobian entry, per extended row
    std::vector<uint8_t> akind, padzero;
    std::vector<double> p0, p1, rconst;
    // node lists of the tape rows (postfix_to_nodes), the tape rows in ascending order
    std::vector<int64_t> nodeptr;
    std::vector<int32_t> nop, na, nb, tape_all;
    std::vector<double> nc;
    // the linear rows (LP rows from 0), the NL slot of every extended row (-1: none), the LP box
    std::vector<int64_t> lin_rows, nl_slot;
    std::vector<double> lv, uv;
    int64_t nnz_nl = 0;                     // Jacobian entries of the NL rows
    // the LP as loaded: row pointers of the linear rows, then the rows built on the host (the epigraph cut at the vertex)
    std::vector<int64_t> rp;
    std::vector<int32_t> rc;
    std::vector<double> rv, rlo, rhi, cvec;
    int64_t n_lin = 0, nnz_lin = 0;
    // the objective row at the origin
    std::vector<double> j0obj;
    double g0obj = 0.0;
    LoadLap lap;
};

// ------------------------------------------------------------------------------------
// Shape classes of the tape rows (tape_classes.hpp; which rows share a class: classify_tape_rows, load_host.hpp).  Members keep
// ascending row order.
// ------------------------------------------------------------------------------------
void Engine::build_tape_classes(const LoadScratch& S) {
    const std::vector<int64_t>& nodeptr = S.nodeptr;
    const std::vector<int64_t>& nl_slot = S.nl_slot;
    const std::vector<int32_t>&nop = S.nop, &na = S.na, &nb = S.nb, &tape_all = S.tape_all;
    const std::vector<double>& nc = S.nc;
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
    std::vector<int32_t> cls_of(nt, -1), rep, cnt;                   // per class: first member (index into tape_all), size
    if (min_rows > 0) classify_tape_rows(tape_all, h_rowptr, nl_slot, nodeptr, nop, na, nb, nc, cls_of, rep, cnt);
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
        mslot[(size_t)(M.mem0 + j)] = (int32_t)nl_slot[(size_t)r];
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

// ------------------------------------------------------------------------------------
// KTN_ROW_QUAD rows (quad_rows.hpp): validation of the caller's quad_* arrays and the device layout.  Host work and uploads
// only; called from loadproblem once the extended structure and the NL row list stand.
// ------------------------------------------------------------------------------------
void Engine::build_quad_rows(const ktn_nlp_desc* d, const LoadScratch& S) {
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
    const std::vector<int64_t>& nl_slot = S.nl_slot;
    std::vector<int64_t> slots_all, slots_nl, tbase_nl, ent_nl;
    std::vector<int32_t> rows_nl;
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

// ------------------------------------------------------------------------------------
// loadproblem!  src/model.jl:81-173
// ------------------------------------------------------------------------------------
void Engine::loadproblem(int64_t num_var, int64_t num_constr, const double* l_var, const double* u_var,
                         const double* l_constr, const double* u_constr, int32_t sense_, const ktn_nlp_desc* d) {
    KTN_REQUIRE(d != nullptr, "nlp description is NULL");
    KTN_REQUIRE(num_var >= 0 && num_constr >= 0, "negative sizes");
    KTN_REQUIRE(d->num_var == num_var && d->num_constr == num_constr, "nlp description sizes disagree with loadproblem");
    KTN_REQUIRE(num_var + 1 < ((int64_t)1 << kKindShift), "num_var too large for the packed 29-bit column index");
    LoadScratch S;
    S.lap.on = dev.debug_load; S.lap.stream = stream; S.lap.t0 = std::chrono::steady_clock::now();
    loaded = false;
    n0 = num_var; m0 = num_constr; sense = sense_;
    obj_linear = d->obj_linear != 0;
    m_ext = m0 + 1;

    load_constraint_rows(d, S);
    load_epigraph_row(d, S);
    S.lap("extended structure (host)");
    load_host_rows(d);
    load_tape_nodes(d, S);
    load_rows_and_box(l_var, u_var, l_constr, u_constr, d, S);
    S.lap("tapes, bounds, nl list");
    load_upload_nlp(S);
    build_tape_classes(S);
    S.lap("tape shape classes");
    grp_sweep = pick_group(m_nl ? (double)S.nnz_nl / (double)m_nl : 4.0);
    if (grp_sweep < 8) grp_sweep = 8;
    S.lap("pack + upload NLP");
    load_blocked_copy(S);
    load_long_rows(S);
    load_batched_copy(S);
    load_sweep_form(S);
    load_sweep_buffers();
    S.lap("blocked copy + sweep buffers");
    load_linear_rows(S);
    S.lap("tangent at origin + LP rows (host)");
    load_objective(S);
    S.lap("objective");
    load_lp(S);
    S.lap("LP upload + reserve");
    loaded = true;
    const int keep_status = status;
    reset();
    S.lap("reset");
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

// ---- extended structure: rows 0..m0-1 + the objective row f(x) - t over n0+1 variables
//      (EpigraphNLPEvaluator, src/nlpeval.jl:42-63; only structural non-zeros are stored,
//       the reference's dense zeros are remembered in pad_zero for round_coefs)
// The caller's rows: bulk copies (a batch of 512 instances brings 3e6 entries through here), with room for the objective row.
void Engine::load_constraint_rows(const ktn_nlp_desc* d, LoadScratch& S) {
    std::vector<uint8_t>& akind = S.akind;
    std::vector<double>&p0 = S.p0, &p1 = S.p1;
    const int64_t nnz0 = m0 ? d->rowptr[m0] : 0;
    h_rowptr.assign(d->rowptr, d->rowptr + m0 + 1);
    h_col.assign(d->col, d->col + nnz0);
    S.padzero.assign((size_t)m_ext, 0);
    S.rconst.assign((size_t)m_ext, 0.0);
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
        S.rconst[i] = d->rconst ? d->rconst[i] : 0.0;
        KTN_REQUIRE(h_rowptr[i + 1] >= h_rowptr[i], "rowptr not monotone");
    }
}

// The objective row f(x) - t in its four forms, appended as row m0; what the cost setter may rewrite
void Engine::load_epigraph_row(const ktn_nlp_desc* d, LoadScratch& S) {
    std::vector<uint8_t>& akind = S.akind;
    std::vector<double>&p0 = S.p0, &p1 = S.p1, &rconst = S.rconst;
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
        std::vector<int32_t> ocols;
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
    screen_pending = false; crossed_cols = 0; crossed_rows = 0;
    for (int64_t i = 0; i < m0; ++i) {                   // atom_kind and p1 are ignored for QUAD rows
        if (h_rowkind[i] != KTN_ROW_QUAD) continue;
        for (int64_t e = h_rowptr[i]; e < h_rowptr[i + 1]; ++e) { akind[(size_t)e] = 0; p1[(size_t)e] = 0.0; }
    }
    S.padzero[m0] = (h_rowptr[m0 + 1] - h_rowptr[m0]) < (n0 + 1) ? 1 : 0;
}

// ---- host-evaluated rows: the callbacks, the row list, the staging arrays
void Engine::load_host_rows(const ktn_nlp_desc* d) {
    cb_rows = d->eval_rows; cb_obj = d->eval_obj; cb_user = d->eval_user;
    host_obj = h_rowkind[m0] == KTN_ROW_HOST;
    host_constr_rows = false;
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

// ---- tapes -> expression DAGs: the node lists of every tape row, the objective's with `- t` appended
void Engine::load_tape_nodes(const ktn_nlp_desc* d, LoadScratch& S) {
    S.nodeptr.assign((size_t)m_ext + 1, 0);
    std::vector<int64_t> col_slot;
    for (int64_t i = 0; i < m_ext; ++i) {
        if (h_rowkind[i] == KTN_ROW_TAPE) { col_slot.assign((size_t)n0 + 1, -1); break; }
    }
    for (int64_t i = 0; i < m_ext; ++i) {
        S.nodeptr[i] = (int64_t)S.nop.size();
        if (h_rowkind[i] != KTN_ROW_TAPE) continue;
        S.tape_all.push_back((int32_t)i);
        const int32_t* rc = h_col.data() + h_rowptr[i];
        const int64_t rl = h_rowptr[i + 1] - h_rowptr[i];
        if (i < m0) {
            KTN_REQUIRE(d->tape_ptr != nullptr, "tape row without tape arrays");
            const int64_t tb = d->tape_ptr[i], te = d->tape_ptr[i + 1];
            postfix_to_nodes(d->tape_op + tb, d->tape_arg + tb, te - tb, rc, rl, h_rowptr[i], col_slot, S.nop, S.na, S.nb, S.nc);
        } else {
            std::vector<int32_t> op(d->obj_tape_op, d->obj_tape_op + d->obj_tape_len);
            std::vector<double> arg(d->obj_tape_arg, d->obj_tape_arg + d->obj_tape_len);
            if (op.empty()) { op.push_back(KTN_OP_CONST); arg.push_back(0.0); }
            op.push_back(KTN_OP_VAR); arg.push_back((double)n0);
            op.push_back(KTN_OP_SUB); arg.push_back(0.0);
            postfix_to_nodes(op.data(), arg.data(), (int64_t)op.size(), rc, rl, h_rowptr[i], col_slot, S.nop, S.na, S.nb, S.nc);
        }
    }
    S.nodeptr[m_ext] = (int64_t)S.nop.size();
}

// ---- bounds per extended row; NL row list and the NL slot of every row (model.jl:115-122,144-148); the LP box
void Engine::load_rows_and_box(const double* l_var, const double* u_var, const double* l_constr, const double* u_constr,
                               const ktn_nlp_desc* d, LoadScratch& S) {
    h_lb.assign(m_ext, 0.0);
    h_ub.assign(m_ext, 0.0);
    for (int64_t i = 0; i < m0; ++i) { h_lb[i] = l_constr[i]; h_ub[i] = u_constr[i]; }
    h_nlrows.clear();
    for (int64_t i = 0; i < m0; ++i) {
        if (d->row_linear && d->row_linear[i]) S.lin_rows.push_back(i);
        else h_nlrows.push_back((int32_t)i);
    }
    n_lp = n0;
    std::vector<double>&lv = S.lv, &uv = S.uv;
    lv.assign(l_var, l_var + n0); uv.assign(u_var, u_var + n0);
    if (!obj_linear) {
        n_lp = n0 + 1;                                  // @variable(m.linear_model, y)  model.jl:137-138
        lv.push_back(-kInf);
        uv.push_back(kInf);
        h_lb[m0] = (sense == KTN_MAX) ? 0.0 : -kInf;    // model.jl:144
        h_ub[m0] = (sense == KTN_MAX) ? kInf : 0.0;
        if (dist.rank == 0) h_nlrows.push_back((int32_t)m0);      // row-sharded: the epigraph row belongs to rank 0
    }
    m_nl = (int64_t)h_nlrows.size();
    S.nl_slot.assign((size_t)m_ext, -1);
    for (int64_t si = 0; si < m_nl; ++si) S.nl_slot[(size_t)h_nlrows[(size_t)si]] = si;
    build_quad_rows(d, S);                                       // (validates the quad_* arrays: host-side only, nothing is launched)
    esh_build_aux(l_var, u_var, l_constr, u_constr, d);         // (esh.hip; cut_algo = KTN_CUT_SUPPORTING only)
    has_inf_bound = false;
    for (int64_t j = 0; j < n_lp; ++j)
        if (!std::isfinite(lv[j]) || !std::isfinite(uv[j])) has_inf_bound = true;
    has_big_bound = false;
    for (int64_t j = 0; j < n_lp; ++j)
        if ((std::isfinite(uv[j]) && uv[j] >= kDenseBig) || (std::isfinite(lv[j]) && -lv[j] >= kDenseBig)) has_big_bound = true;
}

// ---- upload the NLP: structure, packed row programs, node lists, row lists, the KKT report's row map
void Engine::load_upload_nlp(LoadScratch& S) {
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
        for (size_t e = 0; e < S.akind.size(); ++e) kmax = std::max(kmax, S.akind[e]);
        KTN_REQUIRE(kmax <= KTN_ATOM_NEGLOG, "unknown atom kind");
        const int64_t ne = (int64_t)h_col.size();
        DBuf<uint8_t> t_ak;
        DBuf<double> t_p0, t_p1;
        t_ak.upload(S.akind, stream); t_p0.upload(S.p0, stream); t_p1.upload(S.p1, stream);
        d_colk.resize((size_t)ne, stream); d_pp.resize((size_t)ne, stream);
        launch_n(k_pack_atoms, ne, stream, ne, d_col.p, t_ak.p, t_p0.p, t_p1.p, d_colk.p, d_pp.p);
        check_launch();
        sync();                                         // the temporaries are freed on leaving the scope
    }
    d_rconst.upload(S.rconst, stream);
    d_rowkind.upload(h_rowkind, stream); d_padzero.upload(S.padzero, stream);
    d_lb.upload(h_lb, stream); d_ub.upload(h_ub, stream);
    d_nodeptr.upload(S.nodeptr, stream); d_nodeop.upload(S.nop, stream); d_nodea.upload(S.na, stream);
    d_nodeb.upload(S.nb, stream); d_nodec.upload(S.nc, stream);
    d_nodeval.resize(S.nop.size() + 1, stream); d_nodeadj.resize(S.nop.size() + 1, stream);
    std::vector<int32_t> allrows(m_ext);
    for (int64_t i = 0; i < m_ext; ++i) allrows[i] = (int32_t)i;
    d_allrows.upload(allrows, stream);
    d_taperows_all.upload(S.tape_all, stream);
    std::vector<int32_t> tape_nl;
    S.nnz_nl = 0;
    for (auto r : h_nlrows) {
        if (h_rowkind[r] == KTN_ROW_TAPE) tape_nl.push_back(r);
        S.nnz_nl += h_rowptr[r + 1] - h_rowptr[r];
    }
    n_tape_nl = (int64_t)tape_nl.size();
    n_host_nl = 0;
    for (auto r : h_nlrows) n_host_nl += (h_rowkind[r] == KTN_ROW_HOST) ? 1 : 0;
    d_taperows_nl.upload(tape_nl, stream);
    d_nlrows.upload(h_nlrows, stream);
    {   // KKT report: where each original row's multiplier lives (its own LP row, or the cut list of its NL slot)
        std::vector<int32_t> rowmap((size_t)std::max<int64_t>(m0, 1), 0);
        for (size_t k = 0; k < S.lin_rows.size(); ++k) rowmap[(size_t)S.lin_rows[k]] = (int32_t)k;
        for (size_t si = 0; si < h_nlrows.size(); ++si) if (h_nlrows[si] < m0) rowmap[(size_t)h_nlrows[si]] = -1 - (int32_t)si;
        d_kkt_rowmap.upload(rowmap, stream);
        kkt_n_lin = (int64_t)S.lin_rows.size();
        kkt_mirror = false; kkt_seg_ok = false;
        feas_cached = false; feas_blk_cached = false; feas_sides_ok = false;
    }
}

// Long rows (hundreds of entries or more): block-major copy for the column-blocked sweep.  Needs every separable
// NL row sorted by column (the segments are found by binary search).
void Engine::load_blocked_copy(const LoadScratch& S) {
    // Measured on cfg3_hbm (2e7 entries, 2048 per row): exp/log atoms 156 -> 123 us, quadratic atoms 171 -> 114 us.
    // KTN_SWEEP_BLOCKED=0 switches it off (tests compare the two paths).
    if (dev.blk_cfg >= 0) blk_cfg = dev.blk_cfg;
    blk_cols = (blk_cfg == 2) ? 16384 : 8192;
    blk_wg_per_cu = (blk_cfg == 2) ? 1 : 2;
    const bool env = dev.sweep_blocked >= 0;
    blk_on = m_nl > 0 && n_lp >= 2 * blk_cols && (double)S.nnz_nl / (double)m_nl >= 256.0;
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
    if (!blk_on) return;
    std::vector<int64_t> bseg;
    std::vector<HostInt4> bkind;
    std::vector<int32_t> bcolk;
    std::vector<HostDouble2> bpp;
    const int64_t w = blocked_layout(h_nlrows, h_rowptr, h_col, h_rowkind, S.akind, S.p0, S.p1, blk_cols, blk_nb, kKindShift, bseg, bkind, bcolk, bpp);
    d_bcolk.upload(bcolk.data(), (size_t)w, stream);
    d_bpp.upload(reinterpret_cast<const double2*>(bpp.data()), (size_t)w, stream);
    std::vector<SepSlot> slots((size_t)m_nl);
    for (int64_t si = 0; si < m_nl; ++si) {
        const int64_t r = h_nlrows[si];
        SepSlot sl;
        sl.rconst = S.rconst[r]; sl.lb = h_lb[r]; sl.ub = h_ub[r];
        sl.row = (h_rowkind[r] == KTN_ROW_SEP) ? (int32_t)r : -1;
        sl.len_pad = (int32_t)(((h_rowptr[r + 1] - h_rowptr[r]) << 1) | (S.padzero[r] ? 1 : 0));
        slots[(size_t)si] = sl;
    }
    d_slots.upload(slots, stream);
    d_bseg.upload(bseg, stream);
    d_bkind.upload(reinterpret_cast<const int4*>(bkind.data()), bkind.size(), stream);
    d_part.resize((size_t)m_nl * blk_nb, stream);
}

// Very long separable rows get the device-side kind kRowSepLong and their own kernel (kernels.hpp k_sep_eval_long) -- not under
// the column-blocked sweep, which is the long-row path of the NL rows and reads the host-side kinds
void Engine::load_long_rows(const LoadScratch& S) {
    std::vector<uint8_t> dk(h_rowkind);
    std::vector<int32_t> lr, lnr;
    std::vector<int64_t> ls, lns;
    const std::vector<int64_t>& slot_of = S.nl_slot;
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

// Many short rows: the batch-blocked copy (kernels.hpp k_sep_sweep_batch; its layout: batched_layout, load_host.hpp)
void Engine::load_batched_copy(const LoadScratch& S) {
    d_sbck.release(); d_sbrow.release(); d_sbpp.release(); d_sbseg.release();
    sb_on = !blk_on && 2 * m_nl >= (int64_t)3 * kSbRows * num_cus && n_tape_nl == 0 && n_host_nl == 0 && n_quad_nl == 0 && (double)S.nnz_nl / (double)std::max<int64_t>(m_nl, 1) <= 128.0 &&
            n_lp <= (int64_t)kSbCols * 64;
    if (dev.sweep_batched == 0) sb_on = false;
    if (dev.sweep_batched == 1) sb_on = m_nl > 0 && n_tape_nl == 0 && n_host_nl == 0 && n_quad_nl == 0 && n_lp <= (int64_t)kSbCols * 64 && !blk_on;
    if (sb_on) {
        sb_nb = ceil_div(n_lp, (int64_t)kSbCols);
        sb_batches = ceil_div(m_nl, (int64_t)kSbRows);
        std::vector<int64_t> segs;
        std::vector<uint16_t> sck, srw;
        std::vector<HostDouble2> spp;
        batched_layout(h_nlrows, h_rowptr, h_col, S.akind, S.p0, S.p1, kSbRows, kSbCols, sb_nb, segs, sck, srw, spp);
        d_sbck.upload(sck, stream); d_sbrow.upload(srw, stream);
        d_sbpp.upload(reinterpret_cast<const double2*>(spp.data()), spp.size(), stream); d_sbseg.upload(segs, stream);
        sync();
    }
    stats["sweep_batched"] = sb_on ? 1.0 : 0.0;
}

// Which form of the row kernel the sweep and precompute! take depends on the shape alone: many short rows get several rows
// per lane group (k_sep_sweep) once one row per group would make several times the resident wavefronts
void Engine::load_sweep_form(const LoadScratch& S) {
    const int64_t resident = (int64_t)num_cus * 32;
    const int64_t waves_nl = m_nl * grp_sweep / 64, waves_ext = m_ext * grp_sweep / 64;
    sweep_rows_per_group = dev.sweep_rows > 0 ? (dev.sweep_rows >= 4 ? 4 : dev.sweep_rows >= 2 ? 2 : 1)
                                              : (waves_nl >= 16 * resident ? 4 : waves_nl >= 8 * resident ? 2 : 1);
    pre_multirow = waves_ext >= 16 * resident;
    stats["sweep_group"] = (double)grp_sweep;
    stats["sweep_rows_per_group"] = (blk_on || sb_on) ? 0.0 : (double)sweep_rows_per_group;
    stats["sweep_blocked"] = blk_on ? 1.0 : 0.0;
    stats["precompute_multirow"] = pre_multirow ? 1.0 : 0.0;
    // algorithmic bytes of one evaluation pass over the NL rows (DESIGN.md "sweep bytes")
    sweep_bytes = (double)S.nnz_nl * (4 + 16) + 8.0 * (m_nl + 1) + 8.0 * n_lp + 8.0 * 4 * m_nl + 16.0 * m_nl;
}

// What a sweep writes: per extended row, per Jacobian entry, per variable
void Engine::load_sweep_buffers() {
    const size_t mm = (size_t)std::max<int64_t>(m_ext, 1);
    d_g.resize(mm, stream); d_bconst.resize(mm, stream); d_maxc.resize(mm, stream); d_nonfin.resize(mm, stream);
    d_jac.resize((size_t)nnz_ext + 1, stream);
    d_flag.resize(mm, stream); d_cnt.resize(mm, stream); d_rank.resize(mm, stream); d_cntscan.resize(mm, stream);
    d_lastcut.resize(mm, stream);
    d_xs.resize((size_t)n0 + 1, stream); d_ray.resize((size_t)n0 + 1, stream);
    d_flag.zero(stream); d_cnt.zero(stream);
}

// ---- tangent at the origin: linear rows and (linear) objective  model.jl:110-133
// the LP rows of the linear constraints are written on the device (k_lin_rows): only the row pointers -- structural --
// come from the host; the objective row's slice of (g, J) is all that travels back
void Engine::load_linear_rows(LoadScratch& S) {
    d_xs.zero(stream);
    precompute_all(d_xs.p);
    std::vector<int64_t>& rp = S.rp;
    rp.assign(1, 0);
    numcuts = 0;
    const int64_t n_lin = S.n_lin = (int64_t)S.lin_rows.size();
    int64_t nnz_lin = 0;
    {
        rp.reserve((size_t)n_lin + 2);
        std::vector<int32_t> lr((size_t)n_lin);
        for (int64_t k = 0; k < n_lin; ++k) {
            const int64_t i = S.lin_rows[(size_t)k];
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
    S.nnz_lin = nnz_lin;
    // objective row at the origin: g0[m0] and its Jacobian entries
    const int64_t ob = h_rowptr[m0], ol = h_rowptr[m0 + 1] - ob;
    S.j0obj.assign((size_t)std::max<int64_t>(ol, 1), 0.0);
    S.g0obj = 0.0;
    if (ol > 0) KTN_HIP(hipMemcpyAsync(S.j0obj.data(), d_jac.p + ob, (size_t)ol * sizeof(double), hipMemcpyDeviceToHost, stream));
    KTN_HIP(hipMemcpyAsync(&S.g0obj, d_g.p + m0, sizeof(double), hipMemcpyDeviceToHost, stream));
    sync();
}

// The LP's cost vector -- or, for a nonlinear objective, the epigraph cut at the bound-box vertex as a host-built row after
// the linear rows (model.jl:93-97,156-164)
void Engine::load_objective(LoadScratch& S) {
    const int64_t ob = h_rowptr[m0], ol = h_rowptr[m0 + 1] - ob;
    S.cvec.assign((size_t)n_lp, 0.0);
    c0 = 0.0;
    if (prm.log_level > 0) { std::printf(obj_linear ? "objective is linear\n" : "objective is nonlinear\n"); std::fflush(stdout); }   // model.jl:127,135
    if (obj_linear) {
        // gencut(fsep, pt, (0,0), num_constr+1), drop the fictitious aux variable  model.jl:129-133
        for (int64_t e = ob; e < ob + ol; ++e)
            if (h_col[e] < n0) S.cvec[h_col[e]] += S.j0obj[(size_t)(e - ob)];
        c0 = S.g0obj;
        return;
    }
    S.cvec[n0] = 1.0;                                   // @objective(m.linear_model, sense, y)  model.jl:139
    std::vector<double> vtx(n0 + 1, 0.0);
    const bool ok = box_vertex(S.lv.data(), S.uv.data(), n0, vtx.data());
    if (!ok) std::fprintf(stderr, "WARNING: Problem variables insufficiently bounded!\n");      // model.jl:156-157
    if (!ok || dist.rank != 0) return;
    KTN_HIP(hipMemcpyAsync(d_xs.p, vtx.data(), (n0 + 1) * sizeof(double), hipMemcpyHostToDevice, stream));
    precompute_all(d_xs.p);
    std::vector<double> g1 = d_g.to_host(stream);
    vtx[n0] = g1[m0];                                   // push!(vertex, eval_f(d, vertex))
    KTN_HIP(hipMemcpyAsync(d_xs.p, vtx.data(), (n0 + 1) * sizeof(double), hipMemcpyHostToDevice, stream));
    precompute_all(d_xs.p);
    g1 = d_g.to_host(stream);
    const std::vector<double> j1 = d_jac.to_host(stream);
    const VertexCut cut = epigraph_vertex_cut(h_col.data() + ob, j1.data() + ob, ol, g1[m0], vtx.data(), S.padzero[m0] != 0, prm.cut_coef_rng);
    if (!cut.finite) {
        std::fprintf(stderr, "WARNING: Nonlinear constraint or objective likely undefined within domain\n");   // model.jl:70
        status = KTN_STATUS_ERROR;                      // _addcut: warn + :Error, no row added
        return;
    }
    for (int64_t e = 0; e < ol; ++e) {
        S.rc.push_back(h_col[ob + e]);
        S.rv.push_back(cut.coef[(size_t)e]);
    }
    S.rp.push_back(S.nnz_lin + (int64_t)S.rc.size());
    S.rlo.push_back(h_lb[m0] - cut.b);
    S.rhi.push_back(h_ub[m0] - cut.b);
    numcuts += 1;
}

// ---- LP: the linear rows are in place (device); rows built on the host (the epigraph cut at the vertex) are appended; the
// cost and the box go up, the pool gets its room
void Engine::load_lp(const LoadScratch& S) {
    const int64_t n_lin = S.n_lin, nnz_lin = S.nnz_lin;
    M = n_lin + (int64_t)S.rlo.size();
    NNZ = nnz_lin + (int64_t)S.rc.size();
    if (!S.rlo.empty()) {
        lp_rowptr.resize((size_t)M + 1, stream); lp_col.resize((size_t)NNZ + 1, stream); lp_val.resize((size_t)NNZ + 1, stream);
        lp_lo.resize((size_t)M, stream); lp_hi.resize((size_t)M, stream);
        KTN_HIP(hipMemcpyAsync(lp_rowptr.p + n_lin + 1, S.rp.data() + n_lin + 1, S.rlo.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream));
        KTN_HIP(hipMemcpyAsync(lp_col.p + nnz_lin, S.rc.data(), S.rc.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        KTN_HIP(hipMemcpyAsync(lp_val.p + nnz_lin, S.rv.data(), S.rv.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        KTN_HIP(hipMemcpyAsync(lp_lo.p + n_lin, S.rlo.data(), S.rlo.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        KTN_HIP(hipMemcpyAsync(lp_hi.p + n_lin, S.rhi.data(), S.rhi.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        sync();
    }
    lp_rowptr.n = (size_t)M + 1; lp_col.n = lp_val.n = (size_t)NNZ; lp_lo.n = lp_hi.n = (size_t)M;
    lp_y.resize((size_t)M, stream); lp_y.zero(stream);
    lp_c.upload(S.cvec, stream); lp_l.upload(S.lv, stream); lp_u.upload(S.uv, stream);
    lp_x.resize((size_t)n_lp, stream); lp_x.zero(stream);
    M_base = M; NNZ_base = NNZ; numcuts_base = numcuts; M_lin = n_lin;
    {
        // room for three sweeps' worth of cuts (each sweep adds at most min(m_nl, cut cap) rows)
        int64_t per_sweep = m_nl;
        if (prm.cut_cap_factor > 0.0)
            per_sweep = std::min<int64_t>(m_nl, std::max<int64_t>((int64_t)(prm.cut_cap_factor * (double)n_lp), prm.cut_cap_min));
        const double avg_nl = m_nl ? (double)S.nnz_nl / (double)m_nl : 0.0;
        const int64_t rows = M + 3 * per_sweep;
        const int64_t nz = NNZ + (int64_t)(3.0 * (double)per_sweep * avg_nl);
        if ((double)rows * 200.0 + (double)nz * 60.0 < 64e9) reserve_lp(rows, nz);     // stay far below the 288 GB
        d_violslots.reserve((size_t)std::max<int64_t>(m_nl, 1), stream);
    }
    sync();
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

}  // namespace ktn
