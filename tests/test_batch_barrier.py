"""GPU tier: cgo.primalbarriermethodbatch — many box-constrained fits at once, every stage of every centering step ONE batched
solve with scalars = t and active = the problems still running.  (CPU tier: tests/test_batch_barrier_oracle.py.)

The reference is N.primalbarriermethod (oracle/cgo_oracle_np.py) with N.make_boxhdh and the base objective restated as a closure,
problem by problem.  Every problem is held to it: barrier status, number of centering steps, and EVERY stage `Results` of every
step by tests/test_batch.py's assert_bar (bitwise status, iters_ran, evaluations and accepted steps; ≤ 1e-10 on x, f and the
trace; ≤ 1e-9 on ∇f).  Final t: exact with a fixed t_initial; within 1e-12 relative with verifyt0, where t is one multiplication
of a sum that the bar holds to ≤ 1e-10.

The problems, their parameters and the reasons for them: tests/_barrier_problems.py (separable quadratic bases scaled by
1/sqrt(40 n), barrier_growth_factor = 10, a barrier_tol reached at the third step for n ≥ 64, HagerZhang +
WolfeBisection(Wolfe(1e-3, 0.9), 100, 1e12, 50), ϵ = 1e-2).  Before they were fixed, the EXISTING cgo.primalbarriermethod, one
call per problem, was run on the GPU on every one of the 150 problems of test_every_problem_against_its_oracle and the six of
the mixed batch, and met assert_bar against that oracle on every stage of every centering step; the problems that did not at
first (a smaller ϵ, an ill-conditioned problem in the mixed batch, one problem of 150) were changed, as that file records."""
import math
import types

import numpy as np
import pytest

import _barrier_problems as P
from test_batch import assert_bar, same_bits

pytestmark = pytest.mark.gpu


def configs(cgo, max_iters=1000):
    return (cgo.setupCGConfig(P.EPS, cgo.HagerZhang(), cgo.EnableTrace(), max_iters=max_iters),
            cgo.WolfeBisection(cgo.Wolfe(1e-3, 0.9), 100, 1e12, 50))


def box_of(cgo, probs):
    form = probs[0].form
    if form == "scalar":
        return cgo.BoxConstraints(0.25, 3.0)
    if form == "shared":
        return cgo.BoxConstraints(probs[0].lb, probs[0].ub)
    return cgo.BatchBoxConstraints(np.stack([p.lb for p in probs]), np.stack([p.ub for p in probs]))


def run_batch(cgo, ctx, probs, t0, tol, barrier_max_iters=8, cfg_ls=None, reruns=()):
    cfg, ls = cfg_ls or configs(cgo)
    params = [np.stack([p.rows[j] for p in probs]) for j in range(len(probs[0].rows))]
    return cgo.primalbarriermethodbatch(box_of(cgo, probs), probs[0].base, np.stack([p.x0 for p in probs]), cfg, ls,
                                        cgo.PrimalBarrierConfig(tol, P.MU, barrier_max_iters, t0, 0.0), *reruns, params=params, ctx=ctx)


def as_ref(r):
    """a `Results` of the numpy restatement with its traces as arrays, as assert_bar reads them"""
    return types.SimpleNamespace(objective=r.objective, minimizer=r.minimizer, gradient=r.gradient, iters_ran=r.iters_ran, status=r.status,
                                 trace_objective=np.array(r.trace_objective, dtype=np.float64), trace_grad_norm=np.array(r.trace_grad_norm, dtype=np.float64),
                                 trace_step_size=np.array(r.trace_step_size, dtype=np.float64),
                                 trace_objective_evals=np.array(r.trace_objective_evals, dtype=np.int64))


def assert_problem(got, ref, name, verifyt0):
    assert got.status == ref.status, f"{name}: barrier status {got.status} vs {ref.status}"
    assert got.iters_ran == ref.iters_ran and len(got.centering_results) == len(ref.centering_results), f"{name}: {got.iters_ran} centering steps vs {ref.iters_ran}"
    for i, (gs, rs) in enumerate(zip(got.centering_results, ref.centering_results)):
        assert len(gs) == len(rs), f"{name}: step {i + 1} ran {len(gs)} stages vs {len(rs)}"
        for k, (g, r) in enumerate(zip(gs, rs)):
            assert_bar(g, as_ref(r), f"{name}-step{i + 1}-stage{k}")
    if math.isnan(ref.t_final):
        assert math.isnan(got.t_final)
    elif verifyt0:
        assert abs(got.t_final - ref.t_final) <= 1e-12 * abs(ref.t_final), f"{name}: t {got.t_final!r} vs {ref.t_final!r}"
    else:
        assert got.t_final == ref.t_final, f"{name}: t {got.t_final!r} vs {ref.t_final!r}"
    assert got.total_objective_evals == ref.total_objective_evals == sum(int(e) for rr in got.centering_results for x in rr for e in x.trace.objective_evals)


# ---- 1. sizes, bound forms, t per problem and fixed ------------------------------------------------------------------------------
@pytest.mark.parametrize("tmode", ["verifyt0", "fixed"])
@pytest.mark.parametrize("n", P.SIZES)
@pytest.mark.parametrize("form", P.FORMS)
def test_every_problem_against_its_oracle(cgo, gpu_ctx, form, n, tmode):
    probs = P.problems(form, n)
    out = run_batch(cgo, gpu_ctx, probs, P.t_initial(tmode, n), P.barrier_tol(probs, tmode))
    assert len(out) == len(probs)
    for p, got in zip(probs, out):   # every problem of the batch
        assert_problem(got, P.reference_of(p, tmode), f"{p.name}-{tmode}", tmode == "verifyt0")
    if tmode == "verifyt0":
        assert len({r.t_final for r in out}) > 1   # a t per problem


# ---- 2. mixed outcomes in one batch, and the launch count ------------------------------------------------------------------------
def _mixed_run(cgo, ctx, probs):
    cfg, ls = configs(cgo, P.MIXED_M)
    return run_batch(cgo, ctx, probs, math.nan, P.mixed_tol(), barrier_max_iters=P.MIXED_BARRIER_ITERS, cfg_ls=(cfg, ls),
                     reruns=((cgo.setupCGConfig(P.EPS, cgo.HagerZhang(), cgo.EnableTrace(), max_iters=P.MIXED_R), ls),))


def test_mixed_outcomes_and_one_solve_per_stage(cgo, gpu_ctx, monkeypatch):
    """An infeasible start, a problem the rerun tuple runs for alone, one that exhausts the rerun tuples, one the barrier's
    max_iters stops, two ordinary ones — each ends as the restatement ends it, and the ordinary ones bit for bit as in a batch of
    their own.  Every stage of every centering step is ONE Batch.solve (plus one for verifyt0), whatever the number of problems."""
    probs = P.mixed_problems()
    refs = {name: P.mixed_reference(p) for name, p in probs.items()}
    assert {name: (r.status, r.iters_ran) for name, r in refs.items()} == P.MIXED_EXPECT
    solves = []
    solve = cgo.Batch.solve

    def counted(self, X0, config, ls, **kw):
        r = solve(self, X0, config, ls, **kw)
        solves.append((config.max_iters, None if kw.get("active") is None else int(np.sum(kw["active"])), r.launches))
        return r
    monkeypatch.setattr(cgo.Batch, "solve", counted)
    out = _mixed_run(cgo, gpu_ctx, list(probs.values()))
    for (name, p), got in zip(probs.items(), out):
        assert_problem(got, refs[name], name, True)
    assert out[1].centering_results == [] and out[1].status == "infeasible_start"
    # every step: the five feasible problems; the rerun stage for b5 alone in step 2, for b4 alone in step 3
    stages = [max(len(r.centering_results[i]) for r in refs.values() if len(r.centering_results) > i) for i in range(P.MIXED_BARRIER_ITERS)]
    print("solves (max_iters, active, launches):", solves)
    assert stages == [1, 2, 2] and len(solves) == 1 + sum(stages)
    assert solves[0][0] == 0 and [s[1] for s in solves[1:]] == [5, 5, 1, 5, 1]
    assert all(s[2] == 1 for s in solves)   # 40 and 3 iterations fit one slice of 64: one launch a stage, not one per problem
    monkeypatch.setattr(cgo.Batch, "solve", solve)
    alone = _mixed_run(cgo, gpu_ctx, [probs["b1"], probs["b2"]])
    for a, b in ((alone[0], out[0]), (alone[1], out[5])):
        assert (a.status, a.iters_ran, a.t_final, a.total_objective_evals) == (b.status, b.iters_ran, b.t_final, b.total_objective_evals)
        for sa, sb in zip(a.centering_results, b.centering_results):
            assert len(sa) == len(sb) == 1
            same_bits(sa[0], sb[0])


# ---- 3. the largest n ------------------------------------------------------------------------------------------------------------
def test_largest_problem_with_all_four_slots(cgo, gpu_ctx):
    """n = batch_max_n of the barrier model with K = 4 (BQ2's two slots, lb, ub): the largest row the LDS holds with all four
    slots loaded; two problems, so that row 1 starts where row 0 ends; one centering step of 6 iterations."""
    src = cgo.barrier_objective_source(P.BQ2, cgo.BoxConstraints(np.zeros(2), np.ones(2)))
    model = cgo.ElementwiseObjective(2, src, param=[None] * 4, ctx=gpu_ctx)
    try:
        n = cgo.batch_max_n(model)
    finally:
        model.close()
    print(f"batch_max_n of the barrier model, K = 4: {n}")
    assert n > 513 and n % 2 == 0
    probs = P.problems("rows", n, 2)
    tol, t0 = 1e-30, 5.6 * math.sqrt(n / 40.0)
    cfg, ls = configs(cgo, 6)
    out = run_batch(cgo, gpu_ctx, probs, t0, tol, barrier_max_iters=1, cfg_ls=(cfg, ls))
    for p, got in zip(probs, out):
        ref = P.reference(p, t0, tol, barrier_max_iters=1, cfg_ls=P.np_configs(6))
        assert ref.status == "centering_step_issue" and ref.centering_results[0][0].status == "max_iters_reached"
        assert_problem(got, ref, f"{p.name}-largest", False)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(cgo, gpu_ctx):
    cfg, ls = configs(cgo, 100)
    bc = cgo.setupPrimalBarrierConfig(1e-2, 10.0, 5)
    probs = P.problems("rows", 8, 2)
    X0, rows = np.stack([p.x0 for p in probs]), np.stack([p.rows[0] for p in probs])
    three = "struct BaseObjective { static constexpr int kParams = 3; static constexpr bool kPairOnly = false; };"
    with pytest.raises(AssertionError, match="no two slots"):   # K_base + 2 > 4
        cgo.primalbarriermethodbatch(box_of(cgo, probs), three, X0, cfg, ls, bc, params=[rows, rows, rows], ctx=gpu_ctx)
    with pytest.raises(cgo.CgoError, match="Backtracking") as e:
        cgo.primalbarriermethodbatch(box_of(cgo, probs), P.BQ2, X0, cfg, ls, bc, (cfg, cgo.Backtracking(cgo.Armijo(1e-3), 0.9, 300, 50)),
                                     params=[rows, rows], ctx=gpu_ctx)
    assert e.value.code == 1
