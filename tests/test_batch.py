"""GPU tier: batched solves — cgo.minimizeobjectivebatch, one workgroup per problem (k_batch), finished on the device.

The bar.  Each problem of a batch is a `Case` with that problem's x0 and D; its reference is run_oracle(case).
  bitwise:   status, iters_ran, trace.objective_evals, trace.step_size (bisection steps are dyadic functions of constants);
  relative:  ≤ 1e-10 on minimizer, objective, trace.objective, trace.grad_norm; ≤ 1e-9 on gradient
             (the resident solver's own numbers, tests/test_resident.py).
What is new against the resident solver — which problem a workgroup takes, the initial evaluation in the kernel, the
write-back of rows, the hand-back of a problem to the host engine — is what the tests below walk: distinct problems in one
batch (odd tail, both branches of the two-pairs-per-trip loop, config 1's size), outcomes mixed in one batch, more problems
than CUs, slices, and rows that must not see one another."""
import dataclasses

import numpy as np
import pytest

from _cases import Case, _product_structs, quad_D, rel, relf, run_oracle
from _suite import rosen_x0

pytestmark = pytest.mark.gpu

_ORACLE = {}


def oracle_of(c):
    """run_oracle once per distinct problem (the reference is shared between the tests and never changed)"""
    key = (c.objective, c.n, c.x0.tobytes(), None if c.D is None else c.D.tobytes(), c.beta, c.ls, c.cond, c.c1, c.c2, c.eps,
           c.max_iters, c.zoom_max_iters, c.ls_max_iters)
    if key not in _ORACLE:
        _ORACLE[key] = run_oracle(c)
    return _ORACLE[key]


def run_batch(cgo, ctx, cases, slice_iters=0):
    """the cases (same objective, size, config and line search; their own x0 and D) as ONE batched solve"""
    c0 = cases[0]
    _, _, cfg, ls = _product_structs(c0)
    X0 = np.stack([c.x0 for c in cases])
    D = np.stack([c.D for c in cases]) if c0.D is not None else None
    return cgo.minimizeobjectivebatch(c0.objective, X0, cfg, ls, D=D, ctx=ctx, slice_iters=slice_iters)


def assert_bar(got, ref, name):
    assert got.status == ref.status, f"{name}: status {got.status} vs {ref.status}"
    assert got.iters_ran == ref.iters_ran, f"{name}: iters_ran {got.iters_ran} vs {ref.iters_ran}"
    assert np.array_equal(got.trace.objective_evals, ref.trace_objective_evals), f"{name}: evaluations per iteration differ"
    assert np.array_equal(got.trace.step_size, ref.trace_step_size), f"{name}: accepted steps differ"
    figs = {"minimizer": rel(got.minimizer, ref.minimizer), "objective": relf(got.objective, ref.objective),
            "gradient": rel(got.gradient, ref.gradient)}
    if len(ref.trace_objective):
        figs["trace.objective"] = float(np.max(np.abs(got.trace.objective - ref.trace_objective) / np.maximum(np.abs(ref.trace_objective), 1e-300)))
        figs["trace.grad_norm"] = float(np.max(np.abs(got.trace.grad_norm - ref.trace_grad_norm) / np.maximum(np.abs(ref.trace_grad_norm), 1e-300)))
    print(f"{name}: {got.status} after {got.iters_ran}: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    for k, v in figs.items():
        if k == "objective" and abs(got.objective - ref.objective) <= 1e-290:
            continue   # (both are zero to the last representable digit: a relative figure has no meaning there)
        assert v <= (1e-9 if k == "gradient" else 1e-10), f"{name}: {k} rel diff {v:.3e}"


def assert_batch(cgo, ctx, cases, slice_iters=0):
    out = run_batch(cgo, ctx, cases, slice_iters)
    assert len(out) == len(cases)
    for c, got in zip(cases, out):
        assert_bar(got, oracle_of(c), c.name)
    return out


def same_bits(a, b):
    for f in ("objective", "iters_ran", "status", "total_fdf_evals"):
        assert getattr(a, f) == getattr(b, f) or (f == "objective" and np.isnan(a.objective) and np.isnan(b.objective)), f
    for f in ("minimizer", "gradient"):
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f
    for f in ("objective", "grad_norm", "step_size", "objective_evals"):
        assert np.array_equal(getattr(a.trace, f), getattr(b.trace, f), equal_nan=True), "trace." + f


# ---- 1. distinct problems ------------------------------------------------------------------------------------------------
def quad_problem(n, b, **kw):
    """problem b of the recipe: x0 = ones·(1 + b/8), D = roll(quad_D(n), b)·2^(b mod 3 − 1)"""
    return Case(f"quad{n}-b{b}", "quad_diag", n, np.ones(n) * (1 + b / 8), D=np.roll(quad_D(n), b) * 2.0 ** (b % 3 - 1), **kw)


@pytest.mark.parametrize("beta,c2", [("PolakRibiere", 0.1), ("DaiYuan", 0.8)])
@pytest.mark.parametrize("n", [5, 513, 1000])
def test_distinct_quadratics(cgo, gpu_ctx, n, beta, c2):
    cases = [quad_problem(n, b, beta=beta, c2=c2, eps=1e-9, max_iters=16) for b in range(4)]
    out = assert_batch(cgo, gpu_ctx, cases)
    assert out.handed_back == 0 and out.launches == 1   # all 16 iterations of every problem in the first slice of 64


def test_distinct_quadratics_wolfe_bisection(cgo, gpu_ctx):
    cases = [quad_problem(64, b, beta="HagerZhang", eps=1e-9, max_iters=16, ls="WolfeBisection", cond="Wolfe", c1=1e-3, c2=0.9, ls_max_iters=100)
             for b in range(4)]
    assert_batch(cgo, gpu_ctx, cases)


@pytest.mark.parametrize("n", [2, 32, 1000])
def test_distinct_rosenbrocks(cgo, gpu_ctx, n):
    cases = [Case(f"rosen{n}-b{b}", "rosenbrock_paired", n, rosen_x0(n, seed=7 + b), beta="DaiYuan", max_iters=12, c2=0.8)
             for b in range(4)]
    assert_batch(cgo, gpu_ctx, cases)


def test_booth_from_three_starts(cgo, gpu_ctx):
    """Ten iterations from each start, not the run to ϵ: Booth's minimum is f = 0, where a RELATIVE figure on f and ∇f has no
    bound — run to convergence (f ≈ 3e-12 after 45 iterations from the third start) the reference's own two restatements,
    run_oracle and run_numpy, differ by 2.2e-7 on f and 3.0e-7 on ∇f with identical steps and x equal to 3.6e-14.  After ten
    iterations (f between 6e-6 and 0.16) they agree to ≤ 4.2e-14 on f, 3.7e-14 on ∇f: the horizon where the bar means something."""
    cases = [Case(f"booth-b{b}", "booth", 2, np.array(x0), beta="HagerZhang", max_iters=10)
             for b, x0 in enumerate([[0.43, 1.23], [-2.0, 4.5], [3.0, 0.25]])]
    assert_batch(cgo, gpu_ctx, cases)


# ---- 2. mixed outcomes in one batch ----------------------------------------------------------------------------------------
def mixed_pr():
    n = 64
    D0 = quad_D(n)
    kw = dict(beta="PolakRibiere", c2=0.8, max_iters=50, eps=1e-5)
    probs = [(np.ones(n), D0), (1.5 * np.ones(n), np.roll(D0, 7)), (np.ones(n), np.ones(n)), (np.zeros(n), D0),
             (np.ones(n), np.tile([1.0, 3.0], n // 2))]
    return [Case(f"mixed-pr-b{b}", "quad_diag", n, x0, D=D, **kw) for b, (x0, D) in enumerate(probs)]


def mixed_hz():
    n = 64
    D0 = quad_D(n)
    kw = dict(beta="HagerZhang", c2=0.8, zoom_max_iters=2, max_iters=50)
    probs = [(np.ones(n), D0), (3.0 * np.ones(n), np.roll(D0, 5)), (np.ones(n), 2.0 * np.ones(n)), (np.ones(n), 4.0 * np.ones(n)),
             (np.ones(n), 0.5 * np.ones(n)), (np.zeros(n), D0)]
    return [Case(f"mixed-hz-b{b}", "quad_diag", n, x0, D=D, **kw) for b, (x0, D) in enumerate(probs)]


def test_mixed_outcomes_polak_ribiere(cgo, gpu_ctx):
    """The two problems the reference finishes with :success end on an EXACTLY zero gradient — (zeros, D₀) starts there, (ones,
    ones) lands on x = 0 with its first step — so Σg² = 0, outside sumsq_in_range: the rare path of LinearAlgebra.norm, where 0
    may also be the underflow of tiny squares.  The batched kernel looks at the gradient element by element there (every one ±0 ⇒
    the norm is 0) and keeps such a problem on the device; only the three the line search gives up on go to the host."""
    cases = mixed_pr()
    refs = [oracle_of(c) for c in cases]
    # what the reference does with them (read off the CPU oracle): the hand-backs happen MID-solve, one iteration done
    assert [(r.status, r.iters_ran) for r in refs] == [("non_descent_search_direction", 1), ("non_descent_search_direction", 1),
                                                       ("success", 1), ("success", 0), ("non_descent_search_direction", 1)]
    assert [int(refs[b].trace_objective_evals.sum()) for b in (0, 1, 3, 4)] == [10, 10, 0, 2]
    out = assert_batch(cgo, gpu_ctx, cases)
    print(f"handed_back {out.handed_back} of {len(cases)}")
    # three hand-backs — every status other than :success is the host engine's — so the two finished problems never reached it
    assert out.handed_back == 3


def test_mixed_outcomes_hager_zhang_short_zoom(cgo, gpu_ctx):
    cases = mixed_hz()
    refs = [oracle_of(c) for c in cases]
    assert [(r.status, r.iters_ran) for r in refs] == [("zoom_max_iters_reached", 0), ("zoom_max_iters_reached", 0), ("success", 1),
                                                       ("success", 1), ("success", 2), ("success", 0)]
    assert [int(r.trace_objective_evals[0]) for r in refs[2:4]] == [2, 3]
    out = assert_batch(cgo, gpu_ctx, cases)
    # the two short zooms, handed back before anything completed; the four :success problems end on x = 0 exactly (steps ½, ¼,
    # 1 then 2, and the start itself): an exactly zero gradient, settled on the device
    assert out.handed_back == 2
    for b in (0, 1):
        assert out[b].iters_ran == 0 and len(out[b].trace.step_size) == 0 and np.array_equal(out[b].minimizer, cases[b].x0)


# ---- 3. more problems than CUs -----------------------------------------------------------------------------------------------
def test_more_problems_than_compute_units(cgo, gpu_ctx):
    cases = [quad_problem(5, b, beta="PolakRibiere", c2=0.1, eps=1e-9, max_iters=8) for b in range(300)]
    out = assert_batch(cgo, gpu_ctx, cases)
    assert out.launches <= 2


# ---- 4. slicing is invisible ---------------------------------------------------------------------------------------------------
def test_slicing_is_invisible(cgo, gpu_ctx):
    cases = mixed_pr()
    runs = [run_batch(cgo, gpu_ctx, cases, slice_iters=s) for s in (1, 3, 0)]
    for r in runs[:2]:
        assert r.handed_back == runs[2].handed_back
        for a, b in zip(r, runs[2]):
            same_bits(a, b)
    assert runs[0].launches > runs[2].launches


# ---- 5. nothing leaks between rows -----------------------------------------------------------------------------------------------
def test_rows_do_not_see_one_another(cgo, gpu_ctx):
    n = 513
    cases = [quad_problem(n, b, beta="DaiYuan", c2=0.8, eps=1e-9, max_iters=16) for b in range(4)]
    first = run_batch(cgo, gpu_ctx, cases)
    again = run_batch(cgo, gpu_ctx, cases)
    for a, b in zip(first, again):
        same_bits(a, b)   # reproducible, run to run
    other = list(cases)
    other[1] = dataclasses.replace(cases[1], x0=np.linspace(-3.0, 2.0, n), D=np.roll(quad_D(n), 100) * 7.0)
    changed = run_batch(cgo, gpu_ctx, other)
    for b in (0, 2, 3):
        same_bits(first[b], changed[b])
    assert not np.array_equal(first[1].minimizer, changed[1].minimizer)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(cgo, gpu_ctx):
    n = 8
    X0, D = np.ones((2, n)), np.ones((2, n))
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=4)
    sw = cgo.setupStrongWolfeBisection(1e-5, 0.1)

    def refused(match, kind="quad_diag", X=X0, Dv=D, config=cfg, ls=sw, ctx=gpu_ctx):
        with pytest.raises(cgo.CgoError, match=match) as e:
            cgo.minimizeobjectivebatch(kind, X, config, ls, D=Dv, ctx=ctx)
        assert e.value.code == 1   # CGO_EINVAL

    refused("objective must be", kind="lse", Dv=None)
    refused("objective must be", kind="rosenbrock_chained", Dv=None)
    refused("L-BFGS", config=cgo.setupCGConfig(1e-9, cgo.LBFGS(5), cgo.EnableTrace(), max_iters=4))
    refused("Broyden", config=cgo.setupCGConfig(1e-9, cgo.BroydenFamily(0.5), cgo.EnableTrace(), max_iters=4))
    refused("Backtracking", ls=cgo.Backtracking(cgo.Armijo(1e-4), 0.5, 100, 50))
    refused("batch must be", X=np.ones((0, n)), Dv=np.ones((0, n)))
    refused("even n", kind="rosenbrock_paired", X=np.ones((2, 7)), Dv=None)
    refused("n = 2", kind="booth", X=np.ones((2, 4)), Dv=None)
    refused("param0", Dv=None)
    max_n = cgo.batch_max_n("quad_diag", gpu_ctx)
    assert max_n > 0 and max_n % 2 == 0
    refused("cgo_batch_max_n", X=np.ones((1, max_n + 2)), Dv=np.ones((1, max_n + 2)))
    assert cgo.batch_max_n("rosenbrock_paired", gpu_ctx) > max_n   # no parameter vector: two arrays in the same LDS
    # a multi-rank context (the communicator is never used: the call is refused before anything runs)
    ctx2 = cgo.Context(0)
    try:
        ctx2.set_comm_callback(0, 2, lambda send: np.concatenate([send, send]))
        refused("multi-rank", ctx=ctx2)
    finally:
        ctx2.close()


def test_largest_problem_one_workgroup_holds(cgo, gpu_ctx):
    """n = cgo_batch_max_n: the whole LDS of a CU, rows at its edge (two of them, so that row 1 starts where row 0 ends)."""
    n = cgo.batch_max_n("quad_diag", gpu_ctx)
    cases = [quad_problem(n, b, beta="PolakRibiere", c2=0.1, eps=1e-9, max_iters=6) for b in range(2)]
    assert_batch(cgo, gpu_ctx, cases)
