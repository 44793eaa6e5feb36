"""Problems (katana_jl_amd.Problem) of SeparableInstances written as expressions: the ExprNLP form and the Julia-shaped
form (every row a tape, the objective a tape declared linear), for the fused-batch tests."""
import numpy as np

import katana_jl_amd as ktn
import tape_ref
from helpers import instance_as_expressions, julia_shaped_nlp


def _problem(inst, d):
    return ktn.Problem(inst.n, inst.num_constr, inst.l_var, inst.u_var, inst.l_constr, inst.u_constr, inst.sense, d)


def expr_problem(inst):
    """ExprNLP: affine rows separable, every other row a tape"""
    obj, cons = instance_as_expressions(ktn, inst)
    return _problem(inst, ktn.ExprNLP(inst.n, obj, cons))


def julia_problem(inst, rng):
    """the Julia binding's shape: every row a tape (linear rows declared linear), the objective a tape declared linear"""
    obj, cons = instance_as_expressions(ktn, inst)
    s_obj = tape_ref.tape_to_sexpr(*obj.tape())
    s_cons = [tape_ref.tape_to_sexpr(*ktn.Expr.wrap(c).tape()) for c in cons]
    return _problem(inst, julia_shaped_nlp(ktn, inst.n, s_obj, s_cons, [i < inst.m_lin for i in range(inst.num_constr)],
                                           True, rng))


def separable_problem(inst):
    return _problem(inst, ktn.SeparableNLP(inst))
