"""GPU tier: batched solves with β = LBFGS(m) — cgo.minimizeobjectivebatch_lbfgs, one workgroup per problem (k_batch_lbfgs), the
ring of every problem in device memory.  (CPU tier: tests/test_batch_lbfgs_abi.py, which also shows that the reference's own
two restatements agree on every problem used here to a tenth of the bar.)

The bar is tests/test_batch.py's assert_bar against each problem's own run_oracle: bitwise status, iters_ran, evaluations per
iteration and accepted steps; ≤ 1e-10 on x, f and the trace; ≤ 1e-9 on ∇f.  The horizons are short on purpose: L-BFGS
restatements drift apart faster than CG ones (the quadratic at n = 64, m = 4 has run_oracle and run_numpy 3e-8 apart after 50
iterations), and the problems' own docstrings in tests/_batch_lbfgs_problems.py say where a horizon was cut for that."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import _batch_lbfgs_problems as Q
from _cases import _product_structs, quad_D, run_oracle
from test_batch import assert_bar, same_bits

pytestmark = pytest.mark.gpu

_ORACLE = {}
OBJ_USER = 4   # CGO_OBJ_USER (include/cgo.h)


def oracle_of(c):
    key = (c.objective, c.n, c.x0.tobytes(), None if c.D is None else c.D.tobytes(), c.beta, c.m, c.ls, c.cond, c.c1, c.c2, c.eps, c.max_iters,
           c.zoom_max_iters, c.ls_max_iters)
    if key not in _ORACLE:
        _ORACLE[key] = run_oracle(c)
    return _ORACLE[key]


def shape(cgo):
    block, u = cgo.batch_lbfgs_shape()
    assert block == Q.BLOCK and 1 <= u <= 4
    return block, u


def run(cgo, ctx, cases, slice_iters=0):
    c0 = cases[0]
    _, _, cfg, ls = _product_structs(c0)
    X0 = np.stack([c.x0 for c in cases])
    D = np.stack([c.D for c in cases]) if c0.D is not None else None
    out = cgo.minimizeobjectivebatch_lbfgs(c0.objective, X0, cfg, ls, D=D, ctx=ctx, slice_iters=slice_iters)
    assert len(out) == len(cases) and out.rows == "device"
    return out


def held(cgo, ctx, cases, slice_iters=0):
    out = run(cgo, ctx, cases, slice_iters)
    for c, got in zip(cases, out):
        assert_bar(got, oracle_of(c), c.name)
    return out


# ---- 1. distinct problems ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", Q.QUAD_MS)
@pytest.mark.parametrize("n", Q.QUAD_SIZES)
def test_distinct_quadratics(cgo, gpu_ctx, n, m):
    """m = 1 and m = 4 over 16 iterations: the ring wraps"""
    out = held(cgo, gpu_ctx, [Q.quad(n, b, m) for b in range(4)])
    assert out.handed_back == 0 and out.launches == 1


def test_distinct_quadratics_wolfe_bisection(cgo, gpu_ctx):
    batch = Q.distinct_batches()[len(Q.QUAD_SIZES) * len(Q.QUAD_MS)]
    assert batch[0].ls == "WolfeBisection" and batch[0].m == 5
    out = held(cgo, gpu_ctx, batch)
    assert out.handed_back == 0 and out.launches == 1


@pytest.mark.parametrize("n,m", Q.ROSEN)
def test_distinct_rosenbrocks(cgo, gpu_ctx, n, m):
    cases = [Q.rosen(n, b, m) for b in range(4)]
    assert len({c.x0.tobytes() for c in cases}) == 4
    out = held(cgo, gpu_ctx, cases)
    assert out.handed_back == 0 and out.launches == 1


def test_booth_from_three_starts(cgo, gpu_ctx):
    batch = Q.distinct_batches()[-1]
    assert batch[0].objective == "booth"
    out = held(cgo, gpu_ctx, batch)
    assert out.handed_back == 0 and out.launches == 1


# ---- 2. every shape of the ring passes' loop ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("odd", [0, 1], ids=["even", "odd-tail"])
@pytest.mark.parametrize("which", range(8))
def test_quadratic_at_every_shape_of_the_loop(cgo, gpu_ctx, which, odd):
    block, u = shape(cgo)
    n = 2 * Q.loop_pairs(block, u)[which] + odd
    out = held(cgo, gpu_ctx, [Q.quad(n, b, 4, max_iters=8) for b in range(3)])
    assert out.handed_back == 0 and out.launches == 1


# ---- 3. mixed outcomes in one batch ---------------------------------------------------------------------------------------------------
def mixed(cgo, ctx, cases, expect):
    refs = [oracle_of(c) for c in cases]
    assert [(r.status, r.iters_ran) for r in refs] == expect
    out = held(cgo, ctx, cases)
    print(f"handed_back {out.handed_back} of {len(cases)}")
    # exactly the problems whose line search did not return :success reach the host — and their results meet the same bar (above)
    assert out.handed_back == sum(r.status not in ("success", "max_iters_reached") for r in refs)
    return out


def test_mixed_outcomes_quadratics(cgo, gpu_ctx):
    """a step that lands on an exactly zero gradient, a start at the minimizer, a run to convergence: all three stay on the device"""
    out = mixed(cgo, gpu_ctx, Q.mixed_quad(), [("success", 1), ("success", 0), ("success", 21)])
    assert out.handed_back == 0


def test_mixed_outcomes_rosenbrock_hand_back_mid_solve(cgo, gpu_ctx):
    cases = Q.mixed_rosen()
    out = mixed(cgo, gpu_ctx, cases, [("max_iters_reached", 8), ("zoom_max_iters_reached", 3)])
    assert out.handed_back == 1 and int(oracle_of(cases[1]).trace_objective_evals.sum()) == 55


def test_mixed_outcomes_short_zoom_hands_back_at_iteration_zero(cgo, gpu_ctx):
    cases = Q.mixed_quad(2)
    out = mixed(cgo, gpu_ctx, cases, [("zoom_max_iters_reached", 0), ("zoom_max_iters_reached", 0), ("success", 1), ("success", 0)])
    assert out.handed_back == 2
    for b in (0, 1):
        assert out[b].iters_ran == 0 and len(out[b].trace.step_size) == 0 and np.array_equal(out[b].minimizer, cases[b].x0)


# ---- 4. the ring wraps twice -------------------------------------------------------------------------------------------------------
def test_ring_of_eleven_slots_wraps_twice(cgo, gpu_ctx):
    out = held(cgo, gpu_ctx, Q.wrap_batch())
    assert out.handed_back == 0 and all(r.iters_ran == 24 for r in out)


# ---- 5. more problems than CUs ----------------------------------------------------------------------------------------------------
def test_more_problems_than_compute_units(cgo, gpu_ctx):
    out = held(cgo, gpu_ctx, Q.many_batch())
    assert len(out) == 300 and out.launches <= 2 and out.handed_back == 0


# ---- 6. slices ----------------------------------------------------------------------------------------------------------------------
def test_slicing_is_invisible(cgo, gpu_ctx):
    """the QnState, the ring and the trial cache survive a launch boundary exactly"""
    for cases in (Q.mixed_quad(), [Q.rosen(64, b, 10) for b in range(3)] + Q.mixed_rosen()[1:]):
        runs = [run(cgo, gpu_ctx, cases, slice_iters=s) for s in (1, 3, 0)]
        for r in runs[:2]:
            assert r.handed_back == runs[2].handed_back
            for a, b in zip(r, runs[2]):
                same_bits(a, b)
        assert runs[0].launches > runs[1].launches > runs[2].launches == 1


# ---- 7. rows do not see one another ----------------------------------------------------------------------------------------------------
def test_rows_do_not_see_one_another(cgo, gpu_ctx):
    cases = Q.rows_batch()
    n = cases[0].n
    first, again = run(cgo, gpu_ctx, cases), run(cgo, gpu_ctx, cases)
    for a, b in zip(first, again):
        same_bits(a, b)   # reproducible, run to run
    other = list(cases)
    other[1] = dataclasses.replace(cases[1], x0=np.linspace(-3.0, 2.0, n), D=np.roll(quad_D(n), 100) * 7.0)
    changed = run(cgo, gpu_ctx, other)
    for b in (0, 2, 3):
        same_bits(first[b], changed[b])
    assert not np.array_equal(first[1].minimizer, changed[1].minimizer)
    # a neighbour whose rows hold NaN changes nothing
    other[1] = dataclasses.replace(cases[1], x0=np.full(n, np.nan))
    other[3] = dataclasses.replace(cases[3], D=np.full(n, np.nan))
    poisoned = run(cgo, gpu_ctx, other)
    for b in (0, 2):
        same_bits(first[b], poisoned[b])
    assert not math.isfinite(poisoned[1].objective) or not np.all(np.isfinite(poisoned[1].minimizer))


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def device_memory():
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert C.CDLL(None).hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value), int(total.value)


def test_refusals(cgo, gpu_ctx):
    from cgo_amd import _lib
    n = 8
    X0, D = np.ones((2, n)), np.ones((2, n))
    cfg = cgo.setupCGConfig(1e-9, cgo.LBFGS(4), cgo.EnableTrace(), max_iters=4)
    sw = cgo.setupStrongWolfeBisection(1e-5, 0.9)
    L = _lib.lib()

    def refused(match, kind="quad_diag", X=X0, Dv=D, config=cfg, ls=sw, ctx=gpu_ctx):
        with pytest.raises(cgo.CgoError, match=match) as e:
            cgo.minimizeobjectivebatch_lbfgs(kind, X, config, ls, D=Dv, ctx=ctx)
        assert e.value.code == 1   # CGO_EINVAL
        # … and through C, with the same arguments
        Xc = np.ascontiguousarray(X, dtype=np.float64)
        Dc = None if Dv is None else np.ascontiguousarray(Dv, dtype=np.float64)
        out, cc, lc = _lib.BatchResultsC(), config._c(), ls._c()
        rc = L.cgo_minimize_batch_lbfgs(ctx._h, cgo.OBJ_KINDS[kind], Xc.shape[1], Xc.shape[0], Xc.ctypes.data_as(_lib.dp),
                                        Dc.ctypes.data_as(_lib.dp) if Dc is not None else None, C.byref(cc), C.byref(lc), 0, C.byref(out))
        assert rc == 1 and out.launches == 0

    for beta in (cgo.PolakRibiere(), cgo.HagerZhang(), cgo.BroydenFamily(0.5)):
        refused("cgo_minimize_batch", config=cgo.setupCGConfig(1e-9, beta, cgo.EnableTrace(), max_iters=4))
    refused("cgo_batch_lbfgs_max_m = 10", config=cgo.setupCGConfig(1e-9, cgo.LBFGS(11), cgo.EnableTrace(), max_iters=4))
    refused("Backtracking", ls=cgo.Backtracking(cgo.Armijo(1e-4), 0.5, 100, 50))
    refused("objective must be", kind="lse", Dv=None)
    refused("objective must be", kind="rosenbrock_chained", Dv=None)
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
    # a run-time compiled objective has no batched L-BFGS form: its kind is refused by the library (the Python layer raises earlier)
    out, cc, lc = _lib.BatchResultsC(), cfg._c(), sw._c()
    assert L.cgo_minimize_batch_lbfgs(gpu_ctx._h, OBJ_USER, n, 2, X0.ctypes.data_as(_lib.dp), None, C.byref(cc), C.byref(lc), 0, C.byref(out)) == 1
    assert "objective must be" in L.cgo_last_error().decode()
    # n beyond the pass index, and cgo_batch_lbfgs_max_n itself: sizes only, the host arrays are never dereferenced
    max_n = cgo.batch_lbfgs_max_n("quad_diag", gpu_ctx)
    assert max_n == cgo.batch_max_n("quad_diag", gpu_ctx, rows="device") > 2 ** 31 and cgo.batch_lbfgs_max_n("booth", gpu_ctx) == 2
    assert cgo.batch_lbfgs_max_n("lse", gpu_ctx) == 0
    tiny = np.ones(16)
    assert L.cgo_minimize_batch_lbfgs(gpu_ctx._h, cgo.OBJ_KINDS["quad_diag"], max_n + 2, 1, tiny.ctypes.data_as(_lib.dp), tiny.ctypes.data_as(_lib.dp),
                                      C.byref(cc), C.byref(lc), 0, C.byref(out)) == 1
    assert "cgo_batch_lbfgs_max_n" in L.cgo_last_error().decode()
    # a batch of twice the free memory: (3 + 1 + 2·(4+1)) = 14 vectors of batch · n doubles, refused before anything is allocated
    free, total = device_memory()
    batch, vecs = 8, 3 + 1 + 2 * (4 + 1)
    n_big = int(2 * free // (8 * batch * vecs)) & ~1
    assert n_big < max_n
    rc = L.cgo_minimize_batch_lbfgs(gpu_ctx._h, cgo.OBJ_KINDS["quad_diag"], n_big, batch, tiny.ctypes.data_as(_lib.dp), tiny.ctypes.data_as(_lib.dp),
                                    C.byref(cc), C.byref(lc), 0, C.byref(out))
    msg = L.cgo_last_error().decode()
    print(f"free {free} of {total} bytes; refusal: {msg}")
    assert rc == 6 and "bytes of device memory" in msg and f"{float(vecs) * batch * n_big * 8:.0f}"[:6] in msg   # CGO_ENOMEM, the bytes asked for
    free_after, _ = device_memory()
    assert free_after >= free - (1 << 30)   # nothing is left allocated
    small = run(cgo, gpu_ctx, [Q.quad(64, b, 4, max_iters=6) for b in range(2)])
    assert [r.status for r in small] == ["max_iters_reached"] * 2


# ---- 9. the old refusals still hold ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ["lds", "device"])
def test_the_cg_batch_still_refuses_lbfgs(cgo, gpu_ctx, rows):
    cfg = cgo.setupCGConfig(1e-9, cgo.LBFGS(5), cgo.EnableTrace(), max_iters=4)
    with pytest.raises(cgo.CgoError, match="L-BFGS") as e:
        cgo.minimizeobjectivebatch("quad_diag", np.ones((2, 8)), cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), D=np.ones((2, 8)), ctx=gpu_ctx, rows=rows)
    assert e.value.code == 1
