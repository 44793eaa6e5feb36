"""The batch of tests/test_gpu_blocks_warm.py and the bridge between a FusedBatch's resident arenas and the plain-Python model of
tests/blocks_warm_ref.py: the six instances of tests/test_gpu_resolve_blocks.py plus four for the edges -- no NL rows, no linear
rows, more than 1 024 arena rows (every row loop and the scan of k_blocks_rewarm take a second trip), and a Problem with a tape
row next to KTN_ROW_QUAD rows (through nlp.fuse_problems: jump_like.Model itself only emits tape and separable rows, so the rows
come from quad_cases.assemble, the tape being the expression form of the first quadratic)."""
import copy

import numpy as np

import katana_jl_amd as ktn
import blocks_warm_ref as W
import fuse_quad_cases as FQ
import quad_cases as QC
from helpers import max_nl_violation

make = ktn.instances.make_instance
N_BASE = 6
BIG_LIN = 1100


def mixed_problem(inst):
    """the NL rows of a family="quad" instance as QUAD rows, the first of them as a tape"""
    rows = FQ.quad_rows(inst)
    objective = ("lin", inst.obj_col, inst.obj_p0)
    d, layouts = QC.assemble(inst.n, rows, objective)
    i = inst.m_lin
    rows[i] = ("tape", QC.quad_as_expr(*layouts[i], rows[i][6]))
    d2, _ = QC.assemble(inst.n, rows, objective)
    return ktn.Problem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr, inst.u_constr, inst.sense, d2), d


def batch():
    """(items of the FusedBatch, per item a function x -> largest NL violation, per item (l_var, u_var), per item its planted optimum)"""
    base = [make(n=24, m_nl=4, k=6, family="explog" if s % 2 else "quad", seed=40 + s) for s in range(N_BASE)]
    no_nl = ktn.instances.make_lp(n=24, m=12, seed=46)             # (an LP: m_nl = 0)
    no_lin = make(n=24, m_nl=4, k=6, family="explog", seed=47, m_lin=0)
    big = make(n=24, m_nl=4, k=6, family="quad", seed=48, m_lin=BIG_LIN)
    qinst = make(n=24, m_nl=4, k=6, family="quad", seed=49)
    mixed, dq = mixed_problem(qinst)
    items = base + [no_nl, no_lin, big, mixed]
    viol = [(lambda x, i=i: max_nl_violation(i, x)) for i in base + [no_nl, no_lin, big]]
    viol.append(lambda x: max(g - float(qinst.u_constr[i]) for i, g in FQ.quad_row_values(dq, np.asarray(x)).items()))
    boxes = [(np.array(i.l_var, dtype=np.float64), np.array(i.u_var, dtype=np.float64)) for i in base + [no_nl, no_lin, big, qinst]]
    return items, viol, boxes, [np.asarray(i.xhat, dtype=np.float64) for i in base + [no_nl, no_lin, big, qinst]]


def with_box(item, l, u):
    """a copy of a batch item with other variable bounds"""
    if isinstance(item, ktn.Problem):
        return item._replace(l_var=np.asarray(l, dtype=np.float64), u_var=np.asarray(u, dtype=np.float64))
    c = copy.copy(item)
    c.l_var, c.u_var = np.asarray(l, dtype=np.float64), np.asarray(u, dtype=np.float64)
    return c


def linear_rows(fb):
    """per instance its rows of the loaded LP in local columns: [(cols, vals, lo, hi)], read once per batch"""
    rp, col, val, lo, hi = fb.m.lp_rows()
    offs = np.asarray(fb.offs)
    out = [[] for _ in range(len(offs) - 1)]
    for r in range(len(lo)):
        c = col[rp[r]:rp[r + 1]]
        b = int(np.searchsorted(offs, c[0], side="right")) - 1
        out[b].append(([int(j - offs[b]) for j in c], [float(v) for v in val[rp[r]:rp[r + 1]]], float(lo[r]), float(hi[r])))
    return out


def nl_counts(fb, lin):
    return [int(ktn.batch._as_problem(it).num_constr) - len(lin[b]) for b, it in enumerate(fb.instances)]


def read_arenas(fb, lin, cap):
    """the resident arenas as the model's Arenas (the linear rows' multipliers are not readable through the ABI: 0 in the model,
    which never looks at them), lists rebuilt from the nl_slot column of ktn_blocks_get_cuts"""
    m, offs = fb.m, np.asarray(fb.offs)
    res = m.blocks_results()
    n_slots = sum(nl_counts(fb, lin))
    out = []
    for b in range(len(offs) - 1):
        c, y = m.blocks_cuts(b), m.blocks_duals(b)
        m_lin, m_nl = len(lin[b]), nl_counts(fb, lin)[b]
        cols = [r[0] for r in lin[b]] + [[int(j - offs[b]) for j in c["col"][c["rowptr"][k]:c["rowptr"][k + 1]]] for k in range(len(c["lo"]))]
        vals = [r[1] for r in lin[b]] + [[float(v) for v in c["val"][c["rowptr"][k]:c["rowptr"][k + 1]]] for k in range(len(c["lo"]))]
        lo = [r[2] for r in lin[b]] + list(c["lo"])
        hi = [r[3] for r in lin[b]] + list(c["hi"])
        prev, last = [-1] * m_lin, [-1] * n_slots
        for k, s in enumerate(c["slot"]):
            s = int(s)
            prev.append(last[s] if s >= 0 else -1)
            if s >= 0:
                last[s] = m_lin + k
        out.append(W.Arena(m_lin, m_lin + cap * m_nl, cols, vals, lo, hi, [0.0] * m_lin + list(y), prev, last,
                           [1.0] * m_lin + list(c["lam"]), status=int(res[b, 0]), overflow=int(res[b, 7])))
    return out


def cut_bits(a):
    """what has to agree bit for bit between an engine arena and the model's: the cut rows' entries, bounds, multipliers, lambdas, slots"""
    m = a.m_lin
    return (a.cols[m:], [[float(v).hex() for v in r] for r in a.vals[m:]], [float(v).hex() for v in a.lo[m:]], [float(v).hex() for v in a.hi[m:]],
            [float(v).hex() for v in a.y[m:]], [float(v).hex() for v in a.lam[m:]], a.slots()[m:])
