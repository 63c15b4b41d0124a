"""CPU tier of tests/test_batch_barrier.py: the chosen box-constrained problems (tests/_barrier_problems.py) on the two oracles.
N.primalbarriermethod ends every one of them with the expected status within the expected number of steps, and the numpy
restatement and the C oracle (run_oracle on the barrier closure at each step's t, from each stage's own start) agree on status,
iterations and evaluations of every stage: the inputs are not knife-edge."""
import math

import numpy as np
import pytest

import _barrier_problems as P
from _cases import Case, N, run_oracle

HZ_WB = dict(beta="HagerZhang", ls="WolfeBisection", cond="Wolfe", c1=1e-3, c2=0.9, ls_max_iters=100, eps=P.EPS)


def c_oracle_agrees(p, ref, t0, stage_iters):
    """every stage of every centering step of `ref` (the numpy restatement's run of problem p) again on the C oracle"""
    con = N.CvxInequalityConstraint(2 * p.n, p.n)
    hdh, f0 = N.make_boxhdh(p.lb, p.ub), p.f0df0()
    t = t0
    for i, stages in enumerate(ref.centering_results):
        x = p.x0
        for k, r in enumerate(stages):
            fdf = lambda g, xx, t=t: N.evalbarrier(con, g, f0, hdh, xx, t)   # noqa: E731
            c = run_oracle(Case(f"{p.name}-step{i + 1}-stage{k}", "closure", p.n, np.array(x), extra={"fdf": fdf}, max_iters=stage_iters[k], **HZ_WB))
            assert (c.status, c.iters_ran) == (r.status, r.iters_ran), (p.name, i, k, c.status, c.iters_ran, r.status, r.iters_ran)
            assert [int(e) for e in c.trace_objective_evals] == [int(e) for e in r.trace_objective_evals], (p.name, i, k)
            x = r.minimizer
        t = P.MU * t


@pytest.mark.parametrize("tmode", ["verifyt0", "fixed"])
@pytest.mark.parametrize("n", P.SIZES)
@pytest.mark.parametrize("form", P.FORMS)
def test_chosen_problems_on_both_oracles(form, n, tmode):
    for p in P.problems(form, n):
        ref = P.reference_of(p, tmode)
        assert ref.status == "success" and 2 <= ref.iters_ran <= 5, (p.name, ref.status, ref.iters_ran)
        if n >= 64:
            assert ref.iters_ran == 3
        assert all(len(st) == 1 and st[0].status == "success" for st in ref.centering_results)
        t0 = P.first_t(p, tmode)
        assert ref.t_final == t0 * P.MU ** (ref.iters_ran - 1) or math.isclose(ref.t_final, t0 * P.MU ** (ref.iters_ran - 1), rel_tol=1e-15)
        c_oracle_agrees(p, ref, t0, [1000])


def test_mixed_outcomes_on_both_oracles():
    probs = P.mixed_problems()
    for name, p in probs.items():
        ref = P.mixed_reference(p)
        assert (ref.status, ref.iters_ran) == P.MIXED_EXPECT[name], (name, ref.status, ref.iters_ran)
        if name == "outside":
            assert ref.centering_results == [] and math.isnan(ref.t_final)
            continue
        c_oracle_agrees(p, ref, P.first_t(p, "verifyt0"), [P.MIXED_M, P.MIXED_R])
    b5 = P.mixed_reference(probs["b5"]).centering_results
    assert [len(st) for st in b5] == [1, 2, 1] and [r.status for r in b5[1]] == ["max_iters_reached", "success"]
    b4 = P.mixed_reference(probs["b4"]).centering_results
    assert [len(st) for st in b4] == [1, 1, 2] and [r.status for r in b4[2]] == ["max_iters_reached"] * 2
    assert all(len(st) == 1 for name in ("b1", "b2", "halfway") for st in P.mixed_reference(probs[name]).centering_results)
