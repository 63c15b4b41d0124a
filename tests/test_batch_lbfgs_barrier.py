"""GPU tier: cgo.primalbarriermethodbatch_lbfgs — primalbarriermethodbatch with a quasi-Newton direction: every stage of every
centering step ONE `BatchLBFGS.solve` with scalars = t and active = the problems still running, on ONE handle opened with the
largest m of the stages.  (CPU tier: tests/test_batch_lbfgs_barrier_oracle.py, which shows the reference's two restatements
agree on every problem used here to a tenth of the bar.)

The reference is N.primalbarriermethod (oracle/cgo_oracle_np.py) under LBFGS(m), problem by problem; every problem is held to it
as tests/test_batch_barrier.py holds the CG form: barrier status, number of centering steps, and EVERY stage `Results` of every
step by tests/test_batch.py's assert_bar (bitwise status, iters_ran, evaluations and accepted steps; ≤ 1e-10 on x, f and the
trace; ≤ 1e-9 on ∇f).  Problems, replacements and their measured misses: tests/_barrier_lbfgs_problems.py.  Six of the 150
problems end :centering_step_issue on a line search that finds no feasible step: those are handed back to the host engine, from a
handle whose four slot rows are the only copy of the problem's data, under the problem's own t."""
import math

import numpy as np
import pytest

import _barrier_lbfgs_problems as B
import _barrier_problems as P
from test_batch import same_bits
from test_batch_barrier import assert_problem, box_of

pytestmark = pytest.mark.gpu
WB = (1e-3, 0.9, 100, 1e12, 50)


def configs(cgo, max_iters=1000, m=B.M):
    return (cgo.setupCGConfig(P.EPS, cgo.LBFGS(m), cgo.EnableTrace(), max_iters=max_iters),
            cgo.WolfeBisection(cgo.Wolfe(WB[0], WB[1]), WB[2], WB[3], WB[4]))


def run_batch(cgo, ctx, probs, t0, tol, rows="device", barrier_max_iters=8, cfg_ls=None, reruns=()):
    cfg, ls = cfg_ls or configs(cgo)
    params = [np.stack([p.rows[j] for p in probs]) for j in range(len(probs[0].rows))]
    return cgo.primalbarriermethodbatch_lbfgs(box_of(cgo, probs), probs[0].base, np.stack([p.x0 for p in probs]), cfg, ls,
                                              cgo.PrimalBarrierConfig(tol, P.MU, barrier_max_iters, t0, 0.0), *reruns, params=params, ctx=ctx, rows=rows)


@pytest.fixture(scope="module")
def sources(cgo, gpu_ctx):
    """One objective of each form's barrier source and base source kept alive for the whole file: the library shares a compiled
    module, and the programs of the batched tiers compiled on it, between objectives of the same text while one of them lives —
    so every test after the first of its form finds its programs."""
    keep = []
    for form in P.FORMS:
        probs = P.problems(form, 2, 2)
        box = box_of(cgo, probs)
        k = len(probs[0].rows)
        keep.append(cgo.ElementwiseObjective(2, cgo.barrier_objective_source(probs[0].base, box), param=[None] * (k + 2 * box.per_variable), ctx=gpu_ctx))
        keep.append(cgo.ElementwiseObjective(2, cgo.api._base_objective_source(probs[0].base), param=[None] * k, ctx=gpu_ctx))
    yield keep
    for o in keep:
        o.close()


# ---- 1. sizes, bound forms, t per problem and fixed, both tiers ---------------------------------------------------------------------
def tier_cases():
    """rows="device": every batch.  rows="lds": n ≤ 64, and ("rows", 513) — four slots at m = 5: 18 rows of 514 doubles in LDS"""
    out = [(form, n, "device") for form in P.FORMS for n in P.SIZES]
    out += [(form, n, "lds") for form in P.FORMS for n in P.SIZES if n <= 64] + [("rows", 513, "lds")]
    return out


@pytest.mark.parametrize("tmode", B.TMODES)
@pytest.mark.parametrize("form,n,rows", tier_cases())
def test_every_problem_against_its_oracle(cgo, gpu_ctx, sources, form, n, rows, tmode):
    probs = B.problems(form, n, tmode)
    out = run_batch(cgo, gpu_ctx, probs, P.t_initial(tmode, n), P.barrier_tol(probs, tmode), rows=rows)
    assert len(out) == len(probs)
    for p, got in zip(probs, out):
        ref = B.reference_of(p, tmode)
        assert_problem(got, ref, f"{p.name}-{tmode}-{rows}", tmode == "verifyt0")
        assert (ref.status != "success") == ((form, n, tmode, p.b) in B.NOT_SUCCESS)
    if tmode == "verifyt0":
        assert len({r.t_final for r in out}) > 1   # a t per problem


@pytest.mark.parametrize("tmode", B.TMODES)
@pytest.mark.parametrize("form,n", B.LBFGS1_BATCHES)
def test_a_ring_of_one_pair(cgo, gpu_ctx, sources, form, n, tmode):
    """LBFGS(1), where the reference is determined (B.LBFGS1_BATCHES)"""
    probs = B.problems(form, n, tmode)
    out = run_batch(cgo, gpu_ctx, probs, P.t_initial(tmode, n), P.barrier_tol(probs, tmode), cfg_ls=configs(cgo, m=1))
    for p, got in zip(probs, out):
        assert_problem(got, B.reference_of(p, tmode, m=1), f"{p.name}-{tmode}-m1", tmode == "verifyt0")


# ---- 2. mixed outcomes in one batch; two ring depths on one handle -------------------------------------------------------------------
def _mixed_run(cgo, ctx, probs, rows="device", m_rerun=B.M):
    cfg, ls = configs(cgo, B.MIXED_M)
    return run_batch(cgo, ctx, probs, math.nan, P.mixed_tol(), rows=rows, barrier_max_iters=B.MIXED_BARRIER_ITERS, cfg_ls=(cfg, ls),
                     reruns=((cgo.setupCGConfig(P.EPS, cgo.LBFGS(m_rerun), cgo.EnableTrace(), max_iters=B.MIXED_R), ls),))


@pytest.mark.parametrize("m_rerun", [B.M, 3])
def test_mixed_outcomes_and_one_solve_per_stage(cgo, gpu_ctx, sources, monkeypatch, m_rerun):
    """An infeasible start, a problem the rerun tuple finishes, three that exhaust it, one the barrier's max_iters stops — each
    ends as the restatement ends it; `active` shrinks as problems end, every stage is ONE BatchLBFGS.solve (plus one for
    verifyt0), and a rerun stage of m = 3 runs on the handle the centering stage of m = 5 runs on: ONE handle is opened for the
    fit, with the largest m."""
    probs = P.mixed_problems()
    refs = {name: B.mixed_reference(name, p, m_rerun) for name, p in probs.items()}
    assert {name: (r.status, r.iters_ran) for name, r in refs.items()} == B.MIXED_EXPECT
    solves, opened = [], []
    solve, init = cgo.BatchLBFGS.solve, cgo.BatchLBFGS.__init__

    def counted(self, X0, config, ls, **kw):
        r = solve(self, X0, config, ls, **kw)
        solves.append((config.max_iters, config.β_config.m, None if kw.get("active") is None else int(np.sum(kw["active"])), r.launches, id(self)))
        return r

    def opening(self, model, params, batch, m, rows="device"):
        init(self, model, params, batch, m, rows=rows)
        opened.append((id(self), self.m, len(params)))
    monkeypatch.setattr(cgo.BatchLBFGS, "solve", counted)
    monkeypatch.setattr(cgo.BatchLBFGS, "__init__", opening)
    out = _mixed_run(cgo, gpu_ctx, list(probs.values()), m_rerun=m_rerun)
    for (name, p), got in zip(probs.items(), out):
        assert_problem(got, refs[name], f"{name}-rerun-m{m_rerun}", True)
    assert out[1].centering_results == [] and out[1].status == "infeasible_start"
    print("handles (id, m, slots):", opened, "solves (max_iters, m, active, launches, handle):", solves)
    # verifyt0 on a handle of the base objective's two slots, the fit on ONE handle of four, both opened with the largest m
    assert [(m, k) for _, m, k in opened] == [(B.M, 2), (B.M, 4)]
    assert solves[0][:3] == (0, B.M, None) and solves[0][4] == opened[0][0] and all(s[4] == opened[1][0] for s in solves[1:])
    # steps 1 and 2: the five feasible problems, all :success; step 3: all five, then the rerun stage for the four the centering stage
    # left at :max_iters_reached (halfway ends :success there)
    assert [s[:3] for s in solves[1:]] == [(B.MIXED_M, B.M, 5), (B.MIXED_M, B.M, 5), (B.MIXED_M, B.M, 5), (B.MIXED_R, m_rerun, 4)]
    assert all(s[3] == 1 for s in solves)   # 45 and 3 iterations fit one slice: one launch a stage, not one per problem
    monkeypatch.setattr(cgo.BatchLBFGS, "solve", solve)
    monkeypatch.setattr(cgo.BatchLBFGS, "__init__", init)
    if m_rerun == B.M:   # a problem's numbers do not depend on its neighbours, nor on the tier
        alone = _mixed_run(cgo, gpu_ctx, [probs["b4"], probs["halfway"]])
        lds = _mixed_run(cgo, gpu_ctx, list(probs.values()), rows="lds")
        for a, b in ((alone[0], out[3]), (alone[1], out[4])) + tuple(zip(lds, out)):
            assert (a.status, a.iters_ran, a.t_final, a.total_objective_evals) == (b.status, b.iters_ran, b.t_final, b.total_objective_evals)
            for sa, sb in zip(a.centering_results, b.centering_results):
                assert len(sa) == len(sb)
                for x, y in zip(sa, sb):
                    same_bits(x, y)


# ---- 3. refusals, before any work -----------------------------------------------------------------------------------------------------
def test_refusals_before_any_work(cgo, gpu_ctx, monkeypatch):
    cfg, ls = configs(cgo, 100)
    bc = cgo.setupPrimalBarrierConfig(1e-2, 10.0, 5)
    probs = P.problems("rows", 8, 2)
    X0, rows = np.stack([p.x0 for p in probs]), np.stack([p.rows[0] for p in probs])

    def no_objective(*a, **kw):
        raise AssertionError("an objective was created")
    monkeypatch.setattr(cgo.api, "ElementwiseObjective", no_objective)
    hz = cgo.setupCGConfig(P.EPS, cgo.HagerZhang(), cgo.EnableTrace(), max_iters=100)
    for stages in ((hz, ls), (cfg, ls, (hz, ls)), (cfg, ls, (cfg, ls), (cgo.setupCGConfig(P.EPS, cgo.BroydenFamily(0.5), cgo.EnableTrace(), max_iters=10), ls))):
        with pytest.raises(cgo.CgoError, match=r"LBFGS\(m\).*primalbarriermethodbatch") as e:
            cgo.primalbarriermethodbatch_lbfgs(box_of(cgo, probs), P.BQ2, X0, stages[0], stages[1], bc, *stages[2:], params=[rows, rows], ctx=gpu_ctx)
        assert e.value.code == 1
    with pytest.raises(cgo.CgoError, match="Backtracking") as e:
        cgo.primalbarriermethodbatch_lbfgs(box_of(cgo, probs), P.BQ2, X0, cfg, ls, bc, (cfg, cgo.Backtracking(cgo.Armijo(1e-3), 0.9, 300, 50)),
                                           params=[rows, rows], ctx=gpu_ctx)
    assert e.value.code == 1
    monkeypatch.undo()
    three = "struct BaseObjective { static constexpr int kParams = 3; static constexpr bool kPairOnly = false; };"
    with pytest.raises(AssertionError, match="no two slots"):   # K_base + 2 > 4, as primalbarriermethodbatch
        cgo.primalbarriermethodbatch_lbfgs(box_of(cgo, probs), three, X0, cfg, ls, bc, params=[rows, rows, rows], ctx=gpu_ctx)


# ---- 4. the batch is the loop of single calls ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tmode", B.TMODES)
def test_batch_equals_the_loop_of_single_calls(cgo, gpu_ctx, sources, tmode):
    """("rows", 64): every problem of the batch against cgo.primalbarriermethod, one call per problem, under the same LBFGS(5) —
    both held to the restatement at the bar, and equal in every status, count and accepted step"""
    n = 64
    probs = B.problems("rows", n, tmode)
    tol, t0 = P.barrier_tol(probs, tmode), P.t_initial(tmode, n)
    out = run_batch(cgo, gpu_ctx, probs, t0, tol)
    cfg, ls = configs(cgo)
    for p, got in zip(probs, out):
        one = cgo.primalbarriermethod(cgo.BoxConstraints(p.lb, p.ub), p.base, p.x0, cfg, ls, cgo.PrimalBarrierConfig(tol, P.MU, 8, t0, 0.0),
                                      param=list(p.rows), ctx=gpu_ctx)
        ref = B.reference_of(p, tmode)
        assert_problem(one, ref, f"{p.name}-{tmode}-single", tmode == "verifyt0")
        assert_problem(got, ref, f"{p.name}-{tmode}-batch", tmode == "verifyt0")
        assert (one.status, one.iters_ran, one.total_objective_evals) == (got.status, got.iters_ran, got.total_objective_evals)
        for sa, sb in zip(one.centering_results, got.centering_results):
            assert [r.iters_ran for r in sa] == [r.iters_ran for r in sb] and all(np.array_equal(x.trace.step_size, y.trace.step_size) for x, y in zip(sa, sb))
