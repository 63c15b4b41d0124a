"""CPU tier of tests/test_batch_lbfgs_barrier.py: the chosen box-constrained problems (tests/_barrier_lbfgs_problems.py) under
LBFGS(5) on the reference's two restatements.  N.primalbarriermethod (oracle/cgo_oracle_np.py) ends every one of them as that
file records, and the C oracle — run_oracle on the barrier closure at each step's t, from each stage's own start — agrees with
every stage of every centering step to a TENTH of the GPU tier's bar: bitwise on status, iterations, accepted steps and
evaluations per iteration; ≤ 1e-11 on x, f and the trace; ≤ 1e-10 on ∇f.  The inputs are not knife-edge."""
import math

import numpy as np
import pytest

import _barrier_lbfgs_problems as B
import _barrier_problems as P
from _cases import Case, N, run_oracle
from test_batch_lbfgs_abi import figures, held

WB = dict(ls="WolfeBisection", cond="Wolfe", c1=1e-3, c2=0.9, ls_max_iters=100, eps=P.EPS)


def c_oracle_agrees(p, ref, t0, stage_iters, stage_m, worst):
    """every stage of every centering step of `ref` (the numpy restatement's run of problem p) again on the C oracle"""
    con = N.CvxInequalityConstraint(2 * p.n, p.n)
    hdh, f0 = N.make_boxhdh(p.lb, p.ub), p.f0df0()
    t = t0
    for i, stages in enumerate(ref.centering_results):
        x = p.x0
        for k, r in enumerate(stages):
            fdf = lambda g, xx, t=t: N.evalbarrier(con, g, f0, hdh, xx, t)   # noqa: E731
            name = f"{p.name}-step{i + 1}-stage{k}"
            c = run_oracle(Case(name, "closure", p.n, np.array(x), extra={"fdf": fdf}, beta="LBFGS", m=stage_m[k], max_iters=stage_iters[k], **WB))
            for key, v in held(c, B.as_out(r), name, scale=0.1).items():
                if v > worst.get(key, (-1.0, ""))[0]:
                    worst[key] = (v, name)
            x = r.minimizer
        t = P.MU * t


@pytest.mark.parametrize("tmode", B.TMODES)
@pytest.mark.parametrize("n", P.SIZES)
@pytest.mark.parametrize("form", P.FORMS)
def test_chosen_problems_on_both_oracles(form, n, tmode):
    worst = {}
    probs = B.problems(form, n, tmode)
    assert len(probs) == P.BATCH and len({p.b for p in probs}) == P.BATCH
    for p in probs:
        ref = B.reference_of(p, tmode)
        t0 = P.first_t(p, tmode)
        if (form, n, tmode, p.b) in B.NOT_SUCCESS:
            last = ref.centering_results[-1][-1]
            assert (ref.status, ref.iters_ran, last.status) == ("centering_step_issue", 3, "cannot_find_feasible_step") and last.iters_ran in (2, 5), \
                (p.name, ref.status, ref.iters_ran, last.status, last.iters_ran)
            assert all(st[0].status == "success" for st in ref.centering_results[:-1])
        else:
            assert ref.status == "success" and 2 <= ref.iters_ran <= 4, (p.name, tmode, ref.status, ref.iters_ran)
            assert all(st[0].status == "success" for st in ref.centering_results)
            assert ref.t_final == t0 * P.MU ** (ref.iters_ran - 1) or math.isclose(ref.t_final, t0 * P.MU ** (ref.iters_ran - 1), rel_tol=1e-15)
        assert all(len(st) == 1 for st in ref.centering_results)
        c_oracle_agrees(p, ref, t0, [1000], [B.M], worst)
    print(f"{form}-n{n}-{tmode}: the C oracle against the numpy restatement, worst: " + ", ".join(f"{k} {v:.1e} ({nm})" for k, (v, nm) in worst.items()))


def test_the_replacements_stay_within_their_cap():
    """at most one problem of any (form, n, t mode) batch, at most 3 of the 150 — and each replaced problem does miss a tenth of
    the bar on the reference alone, in the figures the module docstring names, with every status, count and step equal"""
    assert sorted(B.INDICES) == sorted(B.REPLACED) and len(B.INDICES) <= 3
    for (form, n, tmode), idx in B.INDICES.items():
        before = [p.b for p in P.problems(form, n)]
        assert len(idx) == len(before) == P.BATCH and len(set(idx)) == P.BATCH
        gone, missed = B.REPLACED[form, n, tmode]
        assert [a for a, b in zip(before, idx) if a != b] == [gone], (form, n, tmode)
        p = P.Prob(form, n, gone)
        ref = P.reference(p, P.t_initial(tmode, n), P.barrier_tol(P.problems(form, n), tmode), cfg_ls=B.np_configs())
        last = ref.centering_results[-1][-1]
        assert (ref.status, ref.iters_ran, last.status) == ("success", 3, "success")
        con = N.CvxInequalityConstraint(2 * n, n)
        hdh, f0, t = N.make_boxhdh(p.lb, p.ub), p.f0df0(), P.first_t(p, tmode) * P.MU ** 2
        c = run_oracle(Case(f"{p.name}-{tmode}-step3", "closure", n, np.array(p.x0), extra={"fdf": lambda g, x: N.evalbarrier(con, g, f0, hdh, x, t)},
                            beta="LBFGS", m=B.M, max_iters=1000, **WB))
        o = B.as_out(last)
        assert (c.status, c.iters_ran) == (o.status, o.iters_ran) and np.array_equal(c.trace_step_size, o.trace_step_size)
        figs = figures(c, o)
        print(f"{p.name} under the {tmode} t, third step, the C oracle against the numpy restatement:", {k: f"{v:.2e}" for k, v in figs.items()})
        assert sorted(k for k, v in figs.items() if v > 0.1 * (1e-9 if k == "gradient" else 1e-10)) == sorted(missed)


@pytest.mark.parametrize("tmode", B.TMODES)
@pytest.mark.parametrize("form,n", B.LBFGS1_BATCHES)
def test_lbfgs_1_on_both_oracles(form, n, tmode):
    """the ring of ONE pair, on the batches where the reference is determined to a tenth of the bar (B.LBFGS1_BATCHES)"""
    worst = {}
    for p in B.problems(form, n, tmode):
        ref = B.reference_of(p, tmode, m=1)
        assert ref.status == "success", (p.name, tmode, ref.status)
        c_oracle_agrees(p, ref, P.first_t(p, tmode), [1000], [1], worst)
    print(f"{form}-n{n}-{tmode} LBFGS(1), worst: " + ", ".join(f"{k} {v:.1e} ({nm})" for k, (v, nm) in worst.items()))


def test_mixed_outcomes_on_both_oracles():
    probs = P.mixed_problems()
    worst = {}
    refs = {name: B.mixed_reference(name, p) for name, p in probs.items()}
    assert {name: (r.status, r.iters_ran) for name, r in refs.items()} == B.MIXED_EXPECT
    for name, p in probs.items():
        ref = refs[name]
        if name == "outside":
            assert ref.centering_results == [] and math.isnan(ref.t_final)
            continue
        c_oracle_agrees(p, ref, P.first_t(p, "verifyt0"), [B.MIXED_M, B.MIXED_R], [B.M, B.M], worst)
    print("mixed batch, worst: " + ", ".join(f"{k} {v:.1e} ({nm})" for k, (v, nm) in worst.items()))
    b4 = refs["b4"].centering_results
    assert [len(st) for st in b4] == [1, 1, 2] and [(r.status, r.iters_ran) for r in b4[2]] == [("max_iters_reached", B.MIXED_M), ("success", 2)]
    for name in ("b1", "b5", "b2"):
        st = refs[name].centering_results
        assert [len(s) for s in st] == [1, 1, 2] and [r.status for r in st[2]] == ["max_iters_reached"] * 2, name
    assert all(len(st) == 1 for st in refs["halfway"].centering_results)
    # … and with a rerun stage of its own m = 3, as the GPU tier runs two ring depths on one handle: determined to the same tenth
    for name in ("b4", "b1"):
        ref = B.mixed_reference(name, probs[name], m_rerun=3)
        c_oracle_agrees(probs[name], ref, P.first_t(probs[name], "verifyt0"), [B.MIXED_M, B.MIXED_R], [B.M, 3], worst)
        print(f"{name} with a rerun stage of LBFGS(3): {ref.status} after {ref.iters_ran}, stages {[[(r.status, r.iters_ran) for r in st] for st in ref.centering_results]}")
