"""Planted instances restated with KTN_ROW_QUAD rows or a KTN_ROW_QUAD objective, for the fused-batch tests (test code).

A planted instance of `make_instance(family="quad")` has NL rows  sum_j a_j (x_j - c_j)^2 - r <= 0  and a KKT point xhat.
`quad_rows_problem` states every NL row as a QUAD row with cross terms,

    Q = diag(2a) + W,   lin = -2ac - W xhat_S,   const = sum a c^2 + 1/2 xhat_S' W xhat_S - r,

with W = sum_uv w_uv (e_u - e_v)(e_u - e_v)', w_uv in U(0.1, 0.5), a weighted graph Laplacian on the row's columns S: the added
term 1/2 (x - xhat)' W (x - xhat) is convex with value 0 and gradient 0 at xhat, so the KKT point, its multipliers, `opt_obj`
and `planted_obj_bound` carry over unchanged.  `quad_objective_problem` does the same to the separable objective
sum 1/2 d_j (x_j - x0_j)^2 of `make_instance(objective="quad")`."""
import math

import numpy as np

import katana_jl_amd as ktn
import quad_cases as QC

L = ktn._lib


def complete_graph(k):
    return [(u, v) for u in range(k) for v in range(u + 1, k)]


def degree_graph(k, G):
    """the graph of quad_cases.degree_row on k = 2G + 7 positions: hub 0 joined to the 2G leaves 5 .. 2G+4, hubs 1, 2, 3 joined to
    the first G-2, G-1, G of them, position 4 (and the two positions behind the leaves) without an edge.  With the diagonal
    of Q the segments have 2G+1, G-1, G, G+1 and 1 entries (leaves: 2 .. 5)."""
    assert k == 2 * G + 7
    edges = [(0, 5 + j) for j in range(2 * G)]
    for hub, deg in ((1, G - 2), (2, G - 1), (3, G)):
        edges += [(hub, 5 + j) for j in range(deg)]
    return edges


def laplacian(rng, k, edges):
    W = np.zeros((k, k))
    if edges:
        u, v = np.asarray(edges).T
        w = rng.uniform(0.1, 0.5, len(edges))
        np.add.at(W, (u, u), w); np.add.at(W, (v, v), w); np.add.at(W, (u, v), -w); np.add.at(W, (v, u), -w)
    return W


def _triplets(cols, M):
    r, c = np.nonzero(M)
    return cols[r], cols[c], M[r, c]


def _quad_row(rng, inst, i, graph):
    """NL row i of a family="quad" instance as the ("quad", ...) tuple of quad_cases.assemble"""
    s = slice(inst.rowptr[i], inst.rowptr[i + 1])
    cols, a, c = np.asarray(inst.col[s], dtype=np.int64), inst.p0[s], inst.p1[s]
    assert np.all(inst.kind[s] == L.ATOM_QUAD)
    W = laplacian(rng, len(cols), graph(len(cols)))
    xs = inst.xhat[cols]
    lin = -2.0 * a * c - W @ xs
    const = float(np.sum(a * c * c) + 0.5 * xs @ W @ xs + inst.rconst[i])
    qr, qc, qv = _triplets(cols, np.diag(2.0 * a) + W)
    return ("quad", cols, lin, qr, qc, qv, const, False)


def _sep_row(inst, i):
    s = slice(inst.rowptr[i], inst.rowptr[i + 1])
    return ("sep", inst.col[s], inst.kind[s], inst.p0[s], inst.p1[s], float(inst.rconst[i]), i < inst.m_lin)


def _problem(inst, d):
    return ktn.Problem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr, inst.u_constr, inst.sense, d)


def quad_rows(inst, graph=complete_graph, seed=0):
    """the rows of quad_cases.assemble: linear rows SEP, NL rows QUAD with the Laplacian cross term; and their layouts"""
    rng = np.random.default_rng([seed, inst.meta["seed"]])
    return [_sep_row(inst, i) if i < inst.m_lin else _quad_row(rng, inst, i, graph) for i in range(inst.num_constr)]


def quad_rows_problem(inst, graph=complete_graph, seed=0, as_tapes=False):
    """Problem with the NL rows as QUAD rows (as_tapes: the same quadratics as expression tapes, quad_cases.quad_as_expr)"""
    rows = quad_rows(inst, graph, seed)
    objective = ("lin", inst.obj_col, inst.obj_p0)
    d, layouts = QC.assemble(inst.n, rows, objective)
    if as_tapes:
        rows = [("tape", QC.quad_as_expr(*layouts[i], r[6])) if r[0] == "quad" else r for i, r in enumerate(rows)]
        d, _ = QC.assemble(inst.n, rows, objective)
    return _problem(inst, d)


def quadnlp_problem(inst, graph=complete_graph, seed=0):
    """the same model through ktn.QuadNLP: EVERY row of kind QUAD (the linear ones declared linear, empty Q) and the linear
    objective of kind QUAD declared linear"""
    rows = []
    for r in quad_rows(inst, graph, seed):
        if r[0] == "sep":
            rows.append((r[1], r[3], [], [], [], r[5]))
        else:
            rows.append(r[1:7])
    d = ktn.QuadNLP(inst.n, (inst.obj_col, inst.obj_p0), inst.obj_const, None, rows)
    return _problem(inst, d)


def quad_objective_problem(inst, ncross=16, seed=0, sense="Min"):
    """an objective="quad" instance with its objective sum 1/2 d_j (x_j - x0_j)^2 as a KTN_ROW_QUAD objective: diagonal Q plus a
    complete-graph Laplacian centred at xhat on `ncross` columns; the rows stay separable.  sense="Max": the negated objective
    to be maximised (optimum -opt_obj)."""
    rng = np.random.default_rng([seed, inst.meta["seed"], 1])
    assert np.all(inst.obj_kind == L.ATOM_QUAD) and np.array_equal(inst.obj_col, np.arange(inst.n))
    d_j, x0 = 2.0 * inst.obj_p0, inst.obj_p1
    T = np.sort(rng.choice(inst.n, size=ncross, replace=False))
    W = laplacian(rng, ncross, complete_graph(ncross))
    lin = -d_j * x0
    lin[T] -= W @ inst.xhat[T]
    const = float(np.sum(0.5 * d_j * x0 * x0) + 0.5 * inst.xhat[T] @ W @ inst.xhat[T] + inst.obj_const)
    qr, qc, qv = _triplets(T, W)
    qr, qc, qv = np.concatenate([np.arange(inst.n), qr]), np.concatenate([np.arange(inst.n), qc]), np.concatenate([d_j, qv])
    sg = -1.0 if sense == "Max" else 1.0
    rows = [_sep_row(inst, i) for i in range(inst.num_constr)]
    d, _ = QC.assemble(inst.n, rows, ("quad", np.arange(inst.n), sg * lin, qr, qc, sg * qv, sg * const))
    return _problem(inst, d)._replace(sense=sense)


# ---- float64 evaluation straight from a description's arrays ----------------------------------------------------------------
def quad_row_value(col, p0, qptr, qcol, qval, rconst, x):
    """rconst + sum_e x_e (a_e + 1/2 sum_{k in seg(e)} q_k x[qcol_k]) of one row given its slices (qptr: len(col) + 1 absolute)"""
    g = float(rconst)
    for e in range(len(col)):
        k = slice(int(qptr[e]), int(qptr[e + 1]))
        g += x[col[e]] * (p0[e] + 0.5 * float(np.sum(qval[k] * x[qcol[k]])))
    return g


def quad_row_values(d, x):
    """{row: value} of every KTN_ROW_QUAD row of description d at x"""
    out = {}
    for i in np.flatnonzero(d.row_kind == L.ROW_QUAD):
        b, e = int(d.rowptr[i]), int(d.rowptr[i + 1])
        out[int(i)] = quad_row_value(d.col[b:e], d.p0[b:e], d.quad_ptr[b:e + 1], d.quad_col, d.quad_val, d.rconst[i], x)
    return out


def quad_objective_value(d, x):
    return quad_row_value(d.obj_col, d.obj_p0, d.obj_quad_ptr, d.obj_quad_col, d.obj_quad_val, d.obj_const, x)


def cone_problem(rng, cones=1):
    """Katana.jl's documentation example (test_gpu_batch_tapes.cone_model), `cones` times in one block: the cone
    sqrt(x^2 + y^2) <= z - 0.25 a tape row, the paraboloid x^2 + y^2 + z <= 1 a QUAD row, a linear row that never binds;
    optimum -1/2 sum hypot(a, b)"""
    rows, ocol, oval, ub, best = [], [], [], [], 0.0
    for c in range(cones):
        j = 3 * c
        x, y, z = ktn.var(j), ktn.var(j + 1), ktn.var(j + 2)
        a, b = rng.uniform(0.5, 2.0, 2) * rng.choice([-1.0, 1.0], 2)
        rows += [("tape", ktn.sqrt(x * x + y * y) - z),
                 ("quad", [j + 2], [1.0], [j, j + 1], [j, j + 1], [2.0, 2.0], 0.0, False),
                 ("sep", [j, j + 1, j + 2], np.zeros(3, dtype=np.uint8), np.ones(3), np.zeros(3), 0.0, True)]
        ocol += [j, j + 1]; oval += [a, b]; ub += [-0.25, 1.0, 3.0]
        best -= 0.5 * math.hypot(a, b)
    n = 3 * cones
    d, _ = QC.assemble(n, rows, ("lin", ocol, oval))
    assert list(d.row_kind) == [ktn._lib.ROW_TAPE, ktn._lib.ROW_QUAD, ktn._lib.ROW_SEP] * cones
    return ktn.Problem(n, 3 * cones, np.full(n, -2.0), np.full(n, 2.0), [-math.inf] * (3 * cones), ub, "Min", d), best
