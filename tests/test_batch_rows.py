"""GPU tier: the batched solves' second tier, rows="device" — k_batch_rows, one workgroup per problem, the problem's rows of x, u
and the parameter slots streamed from device memory in every pass instead of living in LDS.  (CPU tier:
tests/test_batch_rows_abi.py.)

Two bars.
  against the LDS tier (rows="lds"): EVERY number equal as bits — objective, minimizer, gradient, status, iters_ran,
      evaluations, the whole trace, launches, handed_back.  The pass bodies, the order in which a lane accumulates its pairs
      and the workgroup reduction are the same code, so nothing else is acceptable;
  against the CPU oracle, problem by problem: tests/test_batch.py's assert_bar — bitwise status, iters_ran, evaluations and
      accepted steps; ≤ 1e-10 relative on x, f and the trace; ≤ 1e-9 on ∇f.

The streaming loop takes U pairs per lane and trip in workgroups of BLOCK lanes (cgo.batch_rows_shape()): whole trips without
a guard, one last guarded trip, the odd tail element in lane 0.  loop_pairs() walks every boundary of that: npairs = 1, BLOCK ∓ 1,
BLOCK, U·BLOCK ∓ 1, U·BLOCK, 2·U·BLOCK + BLOCK + 1, each with and without an odd tail; then the first size the LDS tier
refuses, and n = 40 001."""
import dataclasses
import math

import numpy as np
import pytest

import _barrier_problems as P
from _cases import Case, _product_structs, quad_D, run_oracle
from _suite import rosen_x0
from test_batch import assert_bar, oracle_of, quad_problem, same_bits
from test_batch_barrier import assert_problem, box_of, configs
from test_batch_scalars import SH, SM
from test_batch_user import data

pytestmark = pytest.mark.gpu

TIERS = ("lds", "device")
# one user body for every number of parameter slots, each reading its scalar (so that a scalar per problem matters)
S0 = "const double t = x - 0.5; gi = s0*t + (t*t)*t; fi = 0.5*s0*(t*t) + 0.25*((t*t)*(t*t));"
S1 = "gi = s0*(p*x); fi = 0.5*s0*((p*x)*x);"
S4 = "const double d = x - p1; gi = s0*((p*d + p2) + p3); fi = s0*((0.5*((p*d)*d) + p2*x) + p3*x);"
BODIES = {0: S0, 1: S1, 2: SH, 3: SM, 4: S4}
SIZES = [1, 2, 5, 64, 513, 1000]


def shape(cgo):
    block, u = cgo.batch_rows_shape()
    assert block == 256 and 1 <= u <= 8
    return block, u


def run_kind(cgo, ctx, cases, rows, slice_iters=0):
    """the cases (tests/test_batch.py's run_batch) in the tier `rows`"""
    c0 = cases[0]
    _, _, cfg, ls = _product_structs(c0)
    X0 = np.stack([c.x0 for c in cases])
    D = np.stack([c.D for c in cases]) if c0.D is not None else None
    out = cgo.minimizeobjectivebatch(c0.objective, X0, cfg, ls, D=D, ctx=ctx, slice_iters=slice_iters, rows=rows)
    assert rows == "auto" or out.rows == rows
    return out


def same_batch(a, b):
    assert (a.launches, a.handed_back, len(a)) == (b.launches, b.handed_back, len(b))
    for ra, rb in zip(a, b):
        assert (ra is None) == (rb is None)
        if ra is not None:
            same_bits(ra, rb)


@pytest.fixture(scope="module")
def models(cgo, gpu_ctx):
    """Each body compiled ONCE for the whole file, one objective of each kept alive (the library shares a module between
    objectives of the same text while one of them lives): the program of its creation, the batch program and the program of
    the device-rows tier."""
    keep = {k: _model(cgo, gpu_ctx, k, 2) for k in BODIES}
    yield keep
    for o in keep.values():
        o.close()


def _model(cgo, ctx, k, n, scalar=1.5):
    o = cgo.ElementwiseObjective(n, BODIES[k], param=[None] * k if k else None, ctx=ctx)
    o.set_scalar(scalar)
    return o


def user_arrays(k, n, batch):
    slots = [np.stack([data(n, b)[0][j] for b in range(batch)]) for j in range(k)]
    return np.stack([data(n, b)[1] for b in range(batch)]), slots


DY = dict(beta="DaiYuan", c2=0.8, eps=1e-9, max_iters=12)


# ---- 1. bit for bit against the LDS tier ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_quadratic_equals_lds_tier_bit_for_bit(cgo, gpu_ctx, n):
    cases = [quad_problem(n, b, beta="PolakRibiere", c2=0.1, eps=1e-9, max_iters=12) for b in range(4)]
    same_batch(run_kind(cgo, gpu_ctx, cases, "lds"), run_kind(cgo, gpu_ctx, cases, "device"))


@pytest.mark.parametrize("n", [2, 64, 1000])
def test_rosenbrock_equals_lds_tier_bit_for_bit(cgo, gpu_ctx, n):
    cases = [Case(f"rosen{n}-b{b}", "rosenbrock_paired", n, rosen_x0(n, seed=7 + b), beta="DaiYuan", max_iters=12, c2=0.8) for b in range(4)]
    same_batch(run_kind(cgo, gpu_ctx, cases, "lds"), run_kind(cgo, gpu_ctx, cases, "device"))


def test_booth_equals_lds_tier_bit_for_bit(cgo, gpu_ctx):
    cases = [Case(f"booth-b{b}", "booth", 2, np.array(x0), beta="HagerZhang", max_iters=10)
             for b, x0 in enumerate([[0.43, 1.23], [-2.0, 4.5], [3.0, 0.25]])]
    same_batch(run_kind(cgo, gpu_ctx, cases, "lds"), run_kind(cgo, gpu_ctx, cases, "device"))


@pytest.mark.parametrize("k", sorted(BODIES))
def test_user_bodies_equal_lds_tier_bit_for_bit(cgo, gpu_ctx, models, k):
    """K = 0 … 4 slots at every size: the model's scalar for all, a scalar per problem (the results' gradient is then
    k_batch_grad's), an `active` mask, and three solves on ONE open Batch."""
    _, _, cfg, ls = _product_structs(Case("cfg", "closure", 2, np.zeros(2), **DY))
    batch = 4
    scalars = np.array([0.75, 1.0, 3.0, 2.0])
    active = np.array([True, False, True, True])
    for n in SIZES:
        X0, slots = user_arrays(k, n, batch)
        model = _model(cgo, gpu_ctx, k, n)
        try:
            one = [cgo.minimizeobjectivebatch(model, X0, cfg, ls, params=slots, ctx=gpu_ctx, rows=r) for r in TIERS]
            same_batch(*one)
            sc = [cgo.minimizeobjectivebatch(model, X0, cfg, ls, params=slots, ctx=gpu_ctx, scalars=scalars, rows=r) for r in TIERS]
            same_batch(*sc)
            opened = []
            for r in TIERS:
                with cgo.Batch(model, slots, batch, rows=r) as B:
                    assert B.rows == r
                    opened.append([B.solve(X0, cfg, ls, scalars=scalars, active=active), B.solve(0.5 * X0, cfg, ls),
                                   B.solve(X0, cfg, ls, scalars=scalars[::-1].copy())])
            for a, b in zip(*opened):
                same_batch(a, b)
            assert opened[1][0][1] is None and opened[1][0].rows == "device"
            same_bits(opened[1][0][0], sc[1][0])   # an active problem of the masked solve is the problem of the full one
        finally:
            model.close()


# ---- 2. every shape of the streaming loop, against the CPU oracle --------------------------------------------------------------------
def loop_pairs(block, u):
    return [1, block - 1, block, block + 1, u * block - 1, u * block, u * block + 1, 2 * u * block + block + 1]


@pytest.mark.parametrize("odd", [0, 1], ids=["even", "odd-tail"])
@pytest.mark.parametrize("which", range(8))
def test_quadratic_at_every_shape_of_the_loop(cgo, gpu_ctx, which, odd):
    block, u = shape(cgo)
    n = 2 * loop_pairs(block, u)[which] + odd
    cases = [quad_problem(n, b, beta="PolakRibiere", c2=0.1, eps=1e-9, max_iters=12) for b in range(3)]
    out = run_kind(cgo, gpu_ctx, cases, "device")
    for c, got in zip(cases, out):
        assert_bar(got, oracle_of(c), c.name)
    assert out.handed_back == 0 and out.launches == 1


@pytest.mark.parametrize("which", range(8))
def test_rosenbrock_at_every_shape_of_the_loop(cgo, gpu_ctx, which):
    block, u = shape(cgo)
    n = 2 * loop_pairs(block, u)[which]
    cases = [Case(f"rosen{n}-b{b}", "rosenbrock_paired", n, rosen_x0(n, seed=7 + b), beta="DaiYuan", max_iters=12, c2=0.8) for b in range(3)]
    for c, got in zip(cases, run_kind(cgo, gpu_ctx, cases, "device")):
        assert_bar(got, oracle_of(c), c.name)


@pytest.mark.parametrize("kind", ["quad_diag", "rosenbrock_paired"])
def test_first_size_the_lds_tier_refuses(cgo, gpu_ctx, kind):
    n = cgo.batch_max_n(kind, gpu_ctx) + 2
    assert cgo.batch_max_n(kind, gpu_ctx, rows="device") == cgo.batch_max_n(kind, gpu_ctx, rows="auto") > 2 ** 31
    if kind == "quad_diag":
        cases = [quad_problem(n, b, beta="PolakRibiere", c2=0.1, eps=1e-9, max_iters=8) for b in range(3)]
    else:
        cases = [Case(f"rosen{n}-b{b}", kind, n, rosen_x0(n, seed=7 + b), beta="DaiYuan", max_iters=8, c2=0.8) for b in range(3)]
    for c, got in zip(cases, run_kind(cgo, gpu_ctx, cases, "device")):
        assert_bar(got, oracle_of(c), c.name)


def test_well_beyond_the_lds_tier(cgo, gpu_ctx):
    """n = 40 001 in a batch of four: 20 trips of the loop and the odd tail, rows 320 KB apart."""
    n = 40001
    cases = [quad_problem(n, b, beta="PolakRibiere", c2=0.1, eps=1e-9, max_iters=15) for b in range(4)]
    out = run_kind(cgo, gpu_ctx, cases, "device")
    for c, got in zip(cases, out):
        assert_bar(got, oracle_of(c), c.name)
    assert out.handed_back == 0 and out.launches == 1


# ---- 3. rows must not see one another -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["start", "slot"])
def test_rows_do_not_see_one_another(cgo, gpu_ctx, where):
    """Problems 0 and 2 of a batch of three carry non-finite numbers — in x0, or in their rows of D; problem 1 equals its own
    batch of one bit for bit (a lane past the end of a row's last trip loads inside its OWN row)."""
    block, u = shape(cgo)
    n = 2 * (u * block + 1) + 1
    kw = dict(beta="DaiYuan", c2=0.8, eps=1e-9, max_iters=10)
    good = quad_problem(n, 1, **kw)
    bad_x = np.full(n, np.nan) if where == "start" else good.x0
    bad_D = good.D if where == "start" else np.full(n, np.inf)
    cases = [dataclasses.replace(good, name="bad0", x0=bad_x, D=bad_D), good, dataclasses.replace(good, name="bad2", x0=bad_x, D=bad_D)]
    alone = run_kind(cgo, gpu_ctx, [good], "device")
    three = run_kind(cgo, gpu_ctx, cases, "device")
    same_bits(three[1], alone[0])
    assert_bar(alone[0], oracle_of(good), good.name)
    assert not np.all(np.isfinite(three[0].minimizer)) or not math.isfinite(three[0].objective)


# ---- 4. mixed outcomes at the first size beyond LDS ----------------------------------------------------------------------------------
def mixed(n, kw, picks):
    """the recipe of tests/test_batch.py's mixed batches at size n (max_iters ≤ 15), plus a problem that runs to max_iters"""
    D0 = quad_D(n)
    probs = [(np.ones(n), D0), (1.5 * np.ones(n), np.roll(D0, 7)), (np.ones(n), np.ones(n)), (np.zeros(n), D0),
             (np.ones(n), np.tile([1.0, 3.0], n // 2)), (np.ones(n), 1.0 + np.arange(n) % 5), (np.ones(n), 2.0 * np.ones(n))]
    return [Case(f"mixed-{kw['beta']}-n{n}-b{b}", "quad_diag", n, probs[b][0], D=probs[b][1], **kw) for b in picks]


@pytest.mark.parametrize("recipe", ["polak-ribiere", "hager-zhang-short-zoom"])
def test_mixed_outcomes_beyond_lds(cgo, gpu_ctx, recipe):
    n = cgo.batch_max_n("quad_diag", gpu_ctx) + 2
    if recipe == "polak-ribiere":
        cases = mixed(n, dict(beta="PolakRibiere", c2=0.8, max_iters=12, eps=1e-5), (0, 1, 2, 3, 4, 5))
        expect = [("non_descent_search_direction", 1), ("non_descent_search_direction", 1), ("success", 1), ("success", 0),
                  ("non_descent_search_direction", 1), ("max_iters_reached", 12)]
    else:
        cases = mixed(n, dict(beta="HagerZhang", c2=0.8, zoom_max_iters=2, max_iters=12), (0, 1, 2, 3, 5, 6))
        expect = [("zoom_max_iters_reached", 0), ("zoom_max_iters_reached", 0), ("success", 1), ("success", 0), ("max_iters_reached", 12),
                  ("success", 1)]
    refs = [oracle_of(c) for c in cases]
    # what the reference does with them: line searches that give up mid-solve and before anything completed, a step that lands
    # on x = 0 exactly (trial_gradient_is_zero), a start at the minimizer (the zero direction after R_INIT), a run to max_iters
    assert [(r.status, r.iters_ran) for r in refs] == expect
    out = run_kind(cgo, gpu_ctx, cases, "device")
    for c, got, ref in zip(cases, out, refs):
        assert_bar(got, ref, c.name)
    print(f"handed_back {out.handed_back} of {len(cases)}")
    # exactly the problems whose line search did not return :success reach the host
    assert out.handed_back == sum(r.status not in ("success", "max_iters_reached") for r in refs) in (2, 3)


# ---- 5. slices ---------------------------------------------------------------------------------------------------------------------
def test_slicing_is_invisible(cgo, gpu_ctx):
    n = cgo.batch_max_n("quad_diag", gpu_ctx) + 2
    cases = mixed(n, dict(beta="PolakRibiere", c2=0.8, max_iters=12, eps=1e-5), (0, 2, 3, 4, 5))
    runs = [run_kind(cgo, gpu_ctx, cases, "device", slice_iters=s) for s in (1, 3, 0)]
    for r in runs[:2]:
        assert r.handed_back == runs[2].handed_back
        for a, b in zip(r, runs[2]):
            same_bits(a, b)
    assert runs[0].launches > runs[1].launches > runs[2].launches == 1


# ---- 6. rows = "auto" ----------------------------------------------------------------------------------------------------------------
def test_auto_takes_lds_where_it_fits_and_device_rows_beyond(cgo, gpu_ctx, models):
    cases = [quad_problem(1000, b, beta="PolakRibiere", c2=0.1, eps=1e-9, max_iters=12) for b in range(3)]
    auto = run_kind(cgo, gpu_ctx, cases, "auto")
    assert auto.rows == "lds"
    same_batch(auto, run_kind(cgo, gpu_ctx, cases, "lds"))
    n = cgo.batch_max_n("quad_diag", gpu_ctx) + 2
    cases = [quad_problem(n, b, beta="PolakRibiere", c2=0.1, eps=1e-9, max_iters=6) for b in range(2)]
    auto = run_kind(cgo, gpu_ctx, cases, "auto")
    assert auto.rows == "device"
    same_batch(auto, run_kind(cgo, gpu_ctx, cases, "device"))
    # … and an open Batch says which tier it runs in
    for n, tier in ((64, "lds"), (cgo.batch_max_n(models[4]) + 2, "device")):
        model = _model(cgo, gpu_ctx, 4, n)
        try:
            with cgo.Batch(model, user_arrays(4, n, 2)[1], 2, rows="auto") as B:
                assert B.rows == tier
        finally:
            model.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def device_memory():
    """(free, total) bytes of the device, from the HIP runtime the library has loaded into the process"""
    import ctypes as C
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert C.CDLL(None).hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value), int(total.value)


def test_refusals(cgo, gpu_ctx):
    n = 8
    X0, D = np.ones((2, n)), np.ones((2, n))
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=4)
    sw = cgo.setupStrongWolfeBisection(1e-5, 0.1)

    def refused(match, kind="quad_diag", X=X0, Dv=D, config=cfg, ls=sw, ctx=gpu_ctx, rows="device", code=1):
        with pytest.raises(cgo.CgoError, match=match) as e:
            cgo.minimizeobjectivebatch(kind, X, config, ls, D=Dv, ctx=ctx, rows=rows)
        assert e.value.code == code

    with pytest.raises(ValueError, match="rows must be"):
        cgo.minimizeobjectivebatch("quad_diag", X0, cfg, sw, D=D, ctx=gpu_ctx, rows="hbm")
    from cgo_amd import _lib
    import ctypes as C
    pol = _lib.BatchPolicyC()
    _lib.lib().cgo_batch_policy_init(C.byref(pol))
    pol.rows = 3
    assert _lib.lib().cgo_batch_max_n_ex(gpu_ctx._h, 0, C.byref(pol)) == 0
    out, cc, lc = _lib.BatchResultsC(), cfg._c(), sw._c()
    assert _lib.lib().cgo_minimize_batch_ex(gpu_ctx._h, cgo.OBJ_KINDS["quad_diag"], n, 2, X0.ctypes.data_as(_lib.dp), D.ctypes.data_as(_lib.dp),
                                           C.byref(cc), C.byref(lc), 0, C.byref(pol), C.byref(out), None) == 1
    assert "cgo_batch_policy.rows" in _lib.lib().cgo_last_error().decode()
    # the LDS tier keeps its limit and its words, under the old call and under rows="lds"
    max_n = cgo.batch_max_n("quad_diag", gpu_ctx)
    big = np.ones((1, max_n + 2))
    refused("cgo_batch_max_n = ", X=big, Dv=big, rows="lds")
    with pytest.raises(cgo.CgoError, match="cgo_batch_max_n = "):
        cgo.minimizeobjectivebatch("quad_diag", big, cfg, sw, D=big, ctx=gpu_ctx)
    # everything cgo_minimize_batch refuses of a config, an objective and a call
    refused("objective must be", kind="lse", Dv=None)
    refused("L-BFGS", config=cgo.setupCGConfig(1e-9, cgo.LBFGS(5), cgo.EnableTrace(), max_iters=4))
    refused("Broyden", config=cgo.setupCGConfig(1e-9, cgo.BroydenFamily(0.5), cgo.EnableTrace(), max_iters=4))
    refused("Backtracking", ls=cgo.Backtracking(cgo.Armijo(1e-4), 0.5, 100, 50))
    refused("batch must be", X=np.ones((0, n)), Dv=np.ones((0, n)))
    refused("even n", kind="rosenbrock_paired", X=np.ones((2, 7)), Dv=None)
    refused("n = 2", kind="booth", X=np.ones((2, 4)), Dv=None)
    refused("param0", Dv=None)
    ctx2 = cgo.Context(0)
    try:
        ctx2.set_comm_callback(0, 2, lambda send: np.concatenate([send, send]))
        refused("multi-rank", ctx=ctx2)
    finally:
        ctx2.close()
    # rows that exceed the device's free memory: (3 + 1) vectors of batch · n doubles asked for, from what is free now.  The
    # call is refused before anything is allocated; the host arrays of the call are one element per problem wide on purpose —
    # the refusal must come from the sizes alone, so the library is called directly with n it never dereferences.
    free, total = device_memory()
    batch = 8
    n_big = int(free // (8 * batch * 2))   # 4 vectors · batch · n_big · 8 bytes = 2 × free
    assert n_big < cgo.batch_max_n("quad_diag", gpu_ctx, rows="device")
    pol.rows = cgo.BATCH_ROWS["device"]
    tiny = np.ones(16)
    rc = _lib.lib().cgo_minimize_batch_ex(gpu_ctx._h, cgo.OBJ_KINDS["quad_diag"], n_big, batch, tiny.ctypes.data_as(_lib.dp),
                                          tiny.ctypes.data_as(_lib.dp), C.byref(cc), C.byref(lc), 0, C.byref(pol), C.byref(out), None)
    msg = _lib.lib().cgo_last_error().decode()
    print(f"free {free} of {total} bytes; refusal: {msg}")
    assert rc == 6 and "bytes of device memory" in msg and f"{4.0 * batch * n_big * 8:.0f}"[:6] in msg   # CGO_ENOMEM, the bytes asked for
    free_after, _ = device_memory()
    assert free_after >= free - (1 << 30)   # nothing is left allocated (of the 2 × free asked for; the slack is for whoever else uses the device)
    small = run_kind(cgo, gpu_ctx, [quad_problem(64, b, beta="PolakRibiere", c2=0.1, eps=1e-9, max_iters=6) for b in range(2)], "device")
    assert [r.status for r in small] == ["max_iters_reached"] * 2


# ---- 8. box-constrained fits ---------------------------------------------------------------------------------------------------------
def run_barrier(cgo, ctx, probs, t0, tol, rows, barrier_max_iters=8, cfg_ls=None):
    cfg, ls = cfg_ls or configs(cgo)
    params = [np.stack([p.rows[j] for p in probs]) for j in range(len(probs[0].rows))]
    return cgo.primalbarriermethodbatch(box_of(cgo, probs), probs[0].base, np.stack([p.x0 for p in probs]), cfg, ls,
                                        cgo.PrimalBarrierConfig(tol, P.MU, barrier_max_iters, t0, 0.0), params=params, ctx=ctx, rows=rows)


def test_barrier_equals_lds_tier_at_every_stage(cgo, gpu_ctx):
    """(Most of this test's time is the one compilation of the barrier objective's source, which the first test of any file
    that uses it pays — tests/test_batch_barrier.py likewise; the two barrier runs themselves take milliseconds.)"""
    probs = P.problems("rows", 513)
    # (one objective of the barrier's source kept alive, so that the two runs share its compiled module)
    keep = cgo.ElementwiseObjective(2, cgo.barrier_objective_source(P.BQ2, box_of(cgo, probs)), param=[None] * 4, ctx=gpu_ctx)
    try:
        a, b = [run_barrier(cgo, gpu_ctx, probs, P.t_initial("fixed", 513), P.barrier_tol(probs, "fixed"), r) for r in TIERS]
    finally:
        keep.close()
    for ra, rb in zip(a, b):
        assert (ra.status, ra.iters_ran, ra.t_final, ra.total_objective_evals) == (rb.status, rb.iters_ran, rb.t_final, rb.total_objective_evals)
        assert len(ra.centering_results) == len(rb.centering_results) > 0
        for sa, sb in zip(ra.centering_results, rb.centering_results):
            assert len(sa) == len(sb)
            for x, y in zip(sa, sb):
                same_bits(x, y)


def test_barrier_beyond_the_lds_tier_with_all_four_slots(cgo, gpu_ctx):
    """n = batch_max_n of the barrier model with K = 4 (BQ2's two slots, lb, ub) + 2 — a box fit with per-variable bounds the
    LDS tier refuses; four problems, one centering step of 6 iterations (tests/test_batch_barrier.py's largest problem)."""
    src = cgo.barrier_objective_source(P.BQ2, cgo.BoxConstraints(np.zeros(2), np.ones(2)))
    model = cgo.ElementwiseObjective(2, src, param=[None] * 4, ctx=gpu_ctx)
    try:
        n = cgo.batch_max_n(model) + 2
    finally:
        model.close()
    probs = P.problems("rows", n, 4)
    tol, t0 = 1e-30, 5.6 * math.sqrt(n / 40.0)
    with pytest.raises(cgo.CgoError, match="cgo_batch_max_n_obj"):
        run_barrier(cgo, gpu_ctx, probs, t0, tol, "lds", barrier_max_iters=1, cfg_ls=configs(cgo, 6))
    out = run_barrier(cgo, gpu_ctx, probs, t0, tol, "device", barrier_max_iters=1, cfg_ls=configs(cgo, 6))
    for p, got in zip(probs, out):
        ref = P.reference(p, t0, tol, barrier_max_iters=1, cfg_ls=P.np_configs(6))
        assert ref.status == "centering_step_issue" and ref.centering_results[0][0].status == "max_iters_reached"
        assert_problem(got, ref, f"{p.name}-beyond-lds", False)
