"""CPU tier: the reference of the NLP-level report (tests/kkt_ref.py, tests/kkt_cases.py) pinned against planted optima and
closed forms, before any GPU test trusts it.

On the planted family every row is a `<=` row, so the constraint duals are d = -(mu, lam); at (xhat, d) the reduced costs must be
the planted bound multipliers nu, and -- xhat being a KKT point with complementary slackness -- the dual bound must be the
planted optimum itself with a zero gap."""
import numpy as np
import pytest
from mpmath import mp, mpf

import katana_jl_amd as ktn
import kkt_cases
import kkt_ref

PLANTED = [(fam, bf) for fam in ("quad", "explog", "explog+t") for bf in (1.0, 0.5)]


@pytest.fixture(scope="module", params=PLANTED, ids=lambda p: "%s-%g" % p)
def planted(request):
    fam, bf = request.param
    inst = ktn.instances.make_instance(n=60, m_nl=8, k=6, m_lin=20, family=fam, bound_frac=bf)
    d = -np.concatenate([inst.mu, inst.lam])
    return inst, d, kkt_ref.kkt_sep(inst, inst.xhat, d)


def test_planted_fields_reproduce_the_meta_sums(planted):
    inst, _, _ = planted
    assert float(inst.lam.sum()) == inst.meta["lam_sum"] and float(inst.mu.sum()) == inst.meta["mu_sum"]
    assert len(inst.lam) == inst.m_nl and len(inst.mu) == inst.m_lin and len(inst.nu) == inst.n
    # nu is signed like a reduced cost: + on a pinned lower bound, - on a pinned upper bound, 0 elsewhere
    assert np.all(inst.xhat[inst.nu > 0] == inst.l_var[inst.nu > 0]) and np.all(inst.xhat[inst.nu < 0] == inst.u_var[inst.nu < 0])


def test_reference_at_the_planted_point(planted):
    inst, d, R = planted
    # the planted c is itself computed in float64 from the same terms: its rounding is of the size of the bound
    assert np.all(np.abs(R.z - inst.nu) <= 2 * R.e_z), np.max(np.abs(R.z - inst.nu) / R.e_z)
    tol = 1e-12 * (1.0 + abs(inst.opt_obj))
    assert abs(R.LB - inst.opt_obj) <= tol, (R.LB, inst.opt_obj)
    assert abs(R.gap) <= tol, R.gap
    assert np.isfinite(R.e_LB) and R.e_LB <= tol


def test_float64_reference_against_mpmath(planted):
    inst, d, R = planted
    rng = np.random.default_rng(1)
    x = np.clip(inst.xhat + 1e-3 * rng.standard_normal(inst.n), inst.l_var, inst.u_var)      # off the KKT point: every term alive
    dd = d * (1.0 + 1e-2 * rng.standard_normal(len(d)))
    R = kkt_ref.kkt_sep(inst, x, dd)
    z, LB, gap = kkt_ref.kkt_sep_mp(inst, x, dd)
    with mp.workprec(kkt_ref.PREC):
        for j in range(inst.n):
            assert abs(mpf(float(R.z[j])) - z[j]) <= R.e_z[j], (j, R.z[j], float(z[j]), R.e_z[j])
        assert abs(mpf(R.LB) - LB) <= R.e_LB and abs(mpf(R.gap) - gap) <= R.e_LB, (R.LB, float(LB), R.e_LB)
    assert float(LB) <= inst.opt_obj + R.e_LB                    # a valid bound at ANY (x, d) with d <= 0 on these convex rows


def test_max_sense_mirrors_min():
    inst = ktn.instances.make_instance(n=60, m_nl=8, k=6, m_lin=20, family="quad", seed=2)
    d = -np.concatenate([inst.mu, inst.lam])
    R = kkt_ref.kkt_sep(inst, inst.xhat, d)
    neg = ktn.instances.make_instance(n=60, m_nl=8, k=6, m_lin=20, family="quad", seed=2)
    neg.obj_p0 = -neg.obj_p0; neg.sense = "Max"
    Rm = kkt_ref.kkt_sep(neg, neg.xhat, -d)
    assert np.array_equal(Rm.z, -R.z) and Rm.LB == -R.LB and Rm.gap == R.gap


@pytest.mark.parametrize("n", kkt_cases.NS)
@pytest.mark.parametrize("name", kkt_cases.NAMES)
def test_closed_form_points_satisfy_kkt(name, n):
    C = kkt_cases.build(name, n)
    inst = C.inst
    s = -1 if inst.sense == "Max" else 1
    with mp.workdps(kkt_cases.DPS):
        tol = mpf(10) ** -30
        f, g, z = kkt_cases.lagrangian_parts(inst, C.xm, C.dm)
        for i in range(inst.num_constr):
            lo, hi = mpf(float(inst.l_constr[i])), mpf(float(inst.u_constr[i]))
            assert lo - tol <= g[i] <= hi + tol
            dm = s * C.dm[i]
            if dm > 0: assert abs(g[i] - lo) <= tol
            if dm < 0: assert abs(g[i] - hi) <= tol
        for j in range(n):
            lo, hi = mpf(float(inst.l_var[j])), mpf(float(inst.u_var[j]))
            assert lo <= C.xm[j] <= hi
            zm = s * z[j]
            if C.xm[j] == lo: assert zm >= -tol
            elif C.xm[j] == hi: assert zm <= tol
            else: assert abs(zm) <= tol
    # the closed forms of the issue
    lam = np.sqrt(n) / 2
    if name == "a": assert abs(C.ds[0] + lam) <= 1e-15 * lam and np.all(np.abs(C.zs) <= 1e-30)
    if name == "f": assert abs(C.ds[0] - lam) <= 1e-15 * lam and np.all(np.abs(C.zs) <= 1e-30)
    if name == "d": assert abs(C.ds[0] - lam) <= 1e-15 * lam
    if name == "b": assert C.zs[0] < 0 and np.all(np.abs(C.zs[1:]) <= 1e-30) and C.ds[0] < 0
    if name == "c": assert C.ds[0] < 0 and C.ds[1] < 0
    if name == "e": assert abs(C.ds[0] + 2 * (1 - 1 / n)) <= 1e-15 and abs(C.fstar - n * (1 - 1 / n) ** 2) <= 1e-14
    assert np.min(np.abs(C.xs)) >= 0.1                         # what the 1e-2 of the GPU test's closed-form tolerance rests on
    # the float64 reference at the rounded point: the bound certifies the optimum, the gap is roundoff
    R = kkt_ref.kkt_sep(inst, C.xs, C.ds)
    assert abs(R.LB - C.fstar) <= 1e-12 and abs(R.gap) <= 1e-12
    assert np.all(np.abs(R.z - C.zs) <= 2 * R.e_z + 1e-15)


# ---- the description-driven reference (TAPE rows through tape_ref, KTN_ROW_QUAD rows through quad_ref) ----
@pytest.mark.parametrize("n", (5, 8))
def test_description_reference_on_the_ellipsoid_of_quad_cases(n):
    """min c'x s.t. 1/2 (x - x0)'Q(x - x0) <= 1 with a dense Q: at the closed-form x* the multiplier is sqrt(c'Q^-1 c / 2), z = 0 and
    the bound is f*; the QUAD statement and the TAPE statement of the same row give the same report within their bounds"""
    import quad_cases as QC
    C = QC.ellipsoid(n)
    lam = float(np.sqrt(C.c @ np.linalg.solve(C.Q, C.c) / 2.0))
    reps = {}
    for name, prob in (("quad", QC.ellipsoid_quad(C)), ("tape", QC.ellipsoid_tape(C))):
        R = kkt_ref.kkt_desc(prob.d, prob.l_constr, prob.u_constr, prob.l_var, prob.u_var, prob.sense, C.xstar, [-lam])
        reps[name] = R
        assert max(abs(float(v)) for v in R.z) <= 1e-12 and abs(float(R.LB) - C.fstar) <= 1e-12 and abs(float(R.gap)) <= 1e-12
        assert all(0 < float(e) <= 1e-13 for e in R.e_z) and 0 < float(R.e_LB) <= 1e-12
    # off the KKT point, with a perturbed multiplier: every term alive, and the two statements still agree
    rng = np.random.default_rng(n)
    x = C.xstar + 1e-2 * rng.standard_normal(n)
    Rq, Rt = (kkt_ref.kkt_desc(p.d, p.l_constr, p.u_constr, p.l_var, p.u_var, p.sense, x, [-1.1 * lam])
              for p in (QC.ellipsoid_quad(C), QC.ellipsoid_tape(C)))
    with mp.workprec(kkt_ref.PREC):
        assert all(abs(a - b) <= ea + eb for a, b, ea, eb in zip(Rq.z, Rt.z, Rq.e_z, Rt.e_z))
        assert abs(Rq.LB - Rt.LB) <= Rq.e_LB + Rt.e_LB and float(Rq.gap) > 1e-6
    assert float(Rq.LB) <= C.fstar + float(Rq.e_LB)


def test_description_reference_agrees_with_the_separable_one(planted):
    inst, d, R = planted
    D = kkt_ref.kkt_desc(ktn.SeparableNLP(inst), inst.l_constr, inst.u_constr, inst.l_var, inst.u_var, inst.sense, inst.xhat, d)
    with mp.workprec(kkt_ref.PREC):
        assert all(abs(mpf(float(a)) - b) <= e for a, b, e in zip(R.z, D.z, R.e_z))
        assert abs(mpf(R.LB) - D.LB) <= R.e_LB
