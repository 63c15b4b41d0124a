"""GPU tier: batched L-BFGS solves on RUN-TIME COMPILED objectives with parameter slots and a scalar per problem —
cgo.minimizeobjectivebatch_lbfgs_obj / cgo_minimize_batch_lbfgs_obj: k_batch_lbfgs<UserObjective, 3>, the fifth program of the
objective's module, one workgroup per problem, the ring in device memory.  (CPU tier: tests/test_batch_lbfgs_user_abi.py, which
also shows that the reference's two restatements agree on every problem used here to a tenth of the bar.)

The bar is tests/test_batch.py's assert_bar against each problem's own run_oracle: bitwise status, iters_ran, evaluations per
iteration and accepted steps; ≤ 1e-10 on x, f and the trace; ≤ 1e-9 on ∇f.  Problems: tests/_batch_lbfgs_user_problems.py."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import _batch_lbfgs_user_dump as D
import _batch_lbfgs_user_problems as U
from _cases import _product_structs, run_oracle
from test_batch import assert_bar, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ORACLE = {}


def oracle_of(p):
    """run_oracle once per distinct problem and config (shared between the tests, never changed)"""
    k = p.key()
    if k not in _ORACLE:
        _ORACLE[k] = run_oracle(p.case())
    return _ORACLE[k]


def _model(cgo, ctx, name, n):
    src, k = U.SOURCES[name]
    param = None if k == 0 else (np.ones(n) if k == 1 else [None] * k)   # (the model's own slots are neither read nor written)
    return cgo.ElementwiseObjective(n, src, param=param, ctx=ctx)


@pytest.fixture(scope="module")
def models(cgo, gpu_ctx):
    """Each of the seven sources compiled ONCE for the whole file — the program of its creation and, with the first batched
    L-BFGS solve, its fifth program — and one objective of each kept alive: the library shares a module between objectives of the
    same text while one of them lives.  first[name]: seconds of that first solve (two problems of n = 2, one iteration);
    recorded, not asserted."""
    keep, first = {}, {}
    cfg = cgo.setupCGConfig(1e-9, cgo.LBFGS(2), cgo.EnableTrace(), max_iters=1)
    X0 = np.array([[-1.2, 1.0], [0.5, 0.25]])
    for name, (_, k) in U.SOURCES.items():
        t = time.perf_counter()
        keep[name] = _model(cgo, gpu_ctx, name, 2)
        made = time.perf_counter() - t
        t = time.perf_counter()
        cgo.minimizeobjectivebatch_lbfgs_obj(keep[name], X0, cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), params=[np.ones((2, 2))] * k, ctx=gpu_ctx)
        first[name] = time.perf_counter() - t
        print(f"{name} (K = {k}): objective created in {made:.2f} s, first batched L-BFGS solve (compiles the program) {first[name]:.2f} s")
    yield keep, first
    for o in keep.values():
        o.close()


def run(cgo, ctx, probs, slice_iters=0):
    out = D.solve(cgo, ctx, probs, slice_iters)
    assert len(out) == len(probs) and out.rows == "device"
    return out


def held(cgo, ctx, probs, slice_iters=0):
    out = run(cgo, ctx, probs, slice_iters)
    for p, got in zip(probs, out):
        assert_bar(got, oracle_of(p), p.case().name)
    return out


def stays_on_the_device(cgo, ctx, probs):
    assert all((oracle_of(p).status, oracle_of(p).iters_ran) == ("max_iters_reached", p.kw["max_iters"]) for p in probs)
    out = held(cgo, ctx, probs)
    assert out.handed_back == 0 and out.launches == 1
    return out


# ---- 1. distinct problems ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", U.MS)
@pytest.mark.parametrize("n", U.SIZES)
@pytest.mark.parametrize("name", ["H2", "Q3"])
def test_distinct_problems(cgo, gpu_ctx, models, name, n, m):
    """odd tails (5, 513), a partial and several whole trips, config 1's size; m = 1 and 4 wrap the ring; H2 is no quadratic, so
    its line searches go past their first trial"""
    stays_on_the_device(cgo, gpu_ctx, U.distinct(name, n, m))


def test_distinct_problems_wolfe_bisection(cgo, gpu_ctx, models):
    probs = U.distinct_wolfe_bisection()
    assert probs[0].case().ls == "WolfeBisection"
    stays_on_the_device(cgo, gpu_ctx, probs)


# ---- 2. other slot counts -----------------------------------------------------------------------------------------------------------
def test_four_slots(cgo, gpu_ctx, models):
    stays_on_the_device(cgo, gpu_ctx, U.four_slots())


def test_one_slot_form(cgo, gpu_ctx, models):
    """K = 1: the has_param form, scalar-`p` signatures — and the built-ins' pairs per trip"""
    stays_on_the_device(cgo, gpu_ctx, U.one_slot())


@pytest.mark.parametrize("n,m", U.ROSEN)
def test_struct_without_slots_restates_paired_rosenbrock(cgo, gpu_ctx, models, n, m):
    """K = 0, a `struct UserObjective` with kPairOnly = true: held to the oracle's own rosenbrock_paired case"""
    probs = U.no_slots(n, m)
    assert all(p.case().objective == "rosenbrock_paired" for p in probs)
    out = held(cgo, gpu_ctx, probs)
    assert out.handed_back == 0 and out.launches == 1
    _, _, cfg, ls = _product_structs(probs[0].case())
    builtin = cgo.minimizeobjectivebatch_lbfgs("rosenbrock_paired", np.stack([p.x0 for p in probs]), cfg, ls, ctx=gpu_ctx)
    same = all(np.array_equal(a.minimizer, b.minimizer) and np.array_equal(a.gradient, b.gradient) and a.objective == b.objective and
               np.array_equal(a.trace.objective, b.trace.objective) and np.array_equal(a.trace.grad_norm, b.trace.grad_norm) for a, b in zip(out, builtin))
    print(f"K = 0 struct against the built-in batched L-BFGS paired Rosenbrock: {'equal bit for bit' if same else 'NOT equal bit for bit'}")


# ---- 3. every shape of the ring passes' loop ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("odd", [0, 1], ids=["even", "odd-tail"])
@pytest.mark.parametrize("which", range(8))
@pytest.mark.parametrize("name", ["Q3", "ONE"], ids=["K3", "K1"])
def test_every_shape_of_the_loop(cgo, gpu_ctx, models, name, which, odd):
    block, u = cgo.batch_lbfgs_shape_obj(U.SOURCES[name][1])
    assert block == U.BLOCK and 1 <= u <= cgo.batch_lbfgs_shape()[1]
    probs = U.loop_batch(name, block, u, which, odd)
    assert all(oracle_of(p).status in ("max_iters_reached", "success") for p in probs)   # (one pair, n = 2 or 3: the quadratic converges within 8)
    out = held(cgo, gpu_ctx, probs)
    assert out.handed_back == 0 and out.launches == 1


# ---- 4. the pairs per lane and trip do not change a bit ------------------------------------------------------------------------------
def test_pairs_per_trip_do_not_change_a_bit(cgo, gpu_ctx, models, tmp_path):
    """A second library built with the K ≥ 2 choice forced to the other value —
    make -C conjugategradientoptim.jl_amd/csrc B=_build_u_alt OUT=../lib/libcgo_hip_u_alt.so EXTRA=-DCGO_BATCH_LBFGS_U_SLOTS=2
    (or =1 where the default is 2) — named by CGO_LIB_PATH_U_ALT, solves D.ab_batches() in a process of its own; every number of
    every result equals this library's bit for bit."""
    alt = os.environ.get("CGO_LIB_PATH_U_ALT", "")
    if not alt or not os.path.exists(alt):
        pytest.skip(f"CGO_LIB_PATH_U_ALT names no library with the other pairs per trip ({alt!r})")
    out = tmp_path / "alt.npz"
    env = dict(os.environ, CGO_LIB_PATH=alt, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_batch_lbfgs_user_dump.py"), str(out)], check=True, env=env, timeout=600)
    theirs = dict(np.load(out))
    ours = D.dump(cgo, gpu_ctx)
    assert theirs["shape"][0] == ours["shape"][0] and theirs["shape"][1] != ours["shape"][1], "the other library has the same pairs per trip"
    assert sorted(theirs) == sorted(ours)
    for k in ours:
        if k != "shape":
            assert np.array_equal(ours[k], theirs[k], equal_nan=k.endswith((".x", ".g", ".tf", ".tg", ".scalars"))), k
    print(f"{len(ours) - 1} arrays of {len(D.ab_batches())} batches equal bit for bit at {int(ours['shape'][1])} and {int(theirs['shape'][1])} pairs per trip")


# ---- 5. slots and rows do not mix ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["H2", "Q3", "Q4"], ids=["K2", "K3", "K4"])
def test_slots_and_rows_do_not_mix(cgo, gpu_ctx, models, name):
    probs = [U.Prob(name, 513, b, 4, dict(c2=0.1, eps=1e-9, max_iters=12)) for b in range(4)]
    first = held(cgo, gpu_ctx, probs)   # every slot of every problem holds different data: a swapped or foreign row misses the bar
    swapped = run(cgo, gpu_ctx, [probs[2], probs[1], probs[0], probs[3]])
    for a, b in ((0, 2), (1, 1), (2, 0), (3, 3)):
        same_bits(first[a], swapped[b])
    # one problem's data changed: the others' bits stay
    other = list(probs)
    other[1] = probs[1].with_(slots=tuple(np.roll(v, 7) * 1.5 for v in probs[1].slots), x0=np.linspace(-1.5, 1.0, 513))
    changed = run(cgo, gpu_ctx, other)
    for b in (0, 2, 3):
        same_bits(first[b], changed[b])
    assert not np.array_equal(first[1].minimizer, changed[1].minimizer)
    # a neighbour whose x0 or slot row is NaN changes nothing
    k = len(probs[0].slots)
    other[1] = probs[1].with_(x0=np.full(513, np.nan))
    other[3] = probs[3].with_(slots=probs[3].slots[:k - 1] + (np.full(513, np.nan),))
    poisoned = run(cgo, gpu_ctx, other)
    for b in (0, 2):
        same_bits(first[b], poisoned[b])
    assert not math.isfinite(poisoned[1].objective) or not np.all(np.isfinite(poisoned[1].minimizer))


# ---- 6. mixed outcomes and hand-backs -------------------------------------------------------------------------------------------------
def mixed(cgo, ctx, probs, expect):
    refs = [oracle_of(p) for p in probs]
    assert [(r.status, r.iters_ran) for r in refs] == expect
    out = held(cgo, ctx, probs)
    print(f"handed_back {out.handed_back} of {len(probs)}")
    # exactly the problems whose line search did not return :success reach the host — and their results meet the same bar (above)
    assert out.handed_back == sum(r.status not in ("success", "max_iters_reached") for r in refs)
    return out


def test_mixed_outcomes_hand_backs_with_two_slots(cgo, gpu_ctx, models):
    """the hand-back objective carries the problem's row of EVERY slot: five of six problems are solved again by the engine"""
    out = mixed(cgo, gpu_ctx, U.mixed_h2(), U.MIXED_H2_EXPECT)
    assert out.handed_back == 5


def test_mixed_outcomes_quadratics(cgo, gpu_ctx, models):
    out = mixed(cgo, gpu_ctx, U.mixed_one(), [("success", 1), ("success", 0), ("success", 21)])
    assert out.handed_back == 0


def test_mixed_outcomes_short_zoom_hands_back_at_iteration_zero(cgo, gpu_ctx, models):
    probs = U.mixed_one(2)
    out = mixed(cgo, gpu_ctx, probs, [("zoom_max_iters_reached", 0), ("zoom_max_iters_reached", 0), ("success", 1), ("success", 0)])
    assert out.handed_back == 2
    for b in (0, 1):
        assert out[b].iters_ran == 0 and len(out[b].trace.step_size) == 0 and np.array_equal(out[b].minimizer, probs[b].x0)


# ---- 7. a scalar per problem ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", U.SCALAR_MS)
@pytest.mark.parametrize("n", U.SCALAR_SIZES)
@pytest.mark.parametrize("name", ["SH", "SM"])
def test_scalars(cgo, gpu_ctx, models, name, n, m):
    """six problems, scalars over six orders of magnitude: each is held to the oracle of ITS scalar (the gradient too: k_batch_grad)"""
    stays_on_the_device(cgo, gpu_ctx, U.scalar_batch(name, n, m))


def test_no_scalars_is_the_models_scalar_for_all(cgo, gpu_ctx, models):
    probs = [p.with_(s0=None) for p in U.scalar_batch("SH", 513, 5)]
    _, _, cfg, ls = _product_structs(probs[0].case())
    model = _model(cgo, gpu_ctx, "SH", 513)
    try:
        model.set_scalar(0.75)
        X0 = np.stack([p.x0 for p in probs])
        params = [np.stack([p.slots[j] for p in probs]) for j in range(2)]
        none = cgo.minimizeobjectivebatch_lbfgs_obj(model, X0, cfg, ls, params=params, ctx=gpu_ctx)
        full = cgo.minimizeobjectivebatch_lbfgs_obj(model, X0, cfg, ls, params=params, scalars=np.full(len(probs), 0.75), ctx=gpu_ctx)
    finally:
        model.close()
    for a, b, p in zip(none, full, probs):
        assert a.objective == b.objective and np.array_equal(a.minimizer, b.minimizer)
        assert np.array_equal(a.trace.objective, b.trace.objective) and np.array_equal(a.trace.grad_norm, b.trace.grad_norm)
        assert_bar(a, oracle_of(p.with_(s0=0.75)), p.case().name + "-model-scalar")


def test_hand_back_with_scalars(cgo, gpu_ctx, models):
    """the engine finishes a handed-back problem under the problem's OWN scalar; a scalar of exactly 1.0 reproduces H2's outcome"""
    probs = U.mixed_sh()
    refs = [oracle_of(p) for p in probs]
    for b in (0, 2, 4):
        assert (refs[b].status, refs[b].iters_ran) == U.MIXED_H2_EXPECT[b]
    out = mixed(cgo, gpu_ctx, probs, [(r.status, r.iters_ran) for r in refs])
    assert out.handed_back >= 2


# ---- 8. slicing is invisible ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["mixed", "Q3"])
def test_slicing_is_invisible(cgo, gpu_ctx, models, which):
    """the QnState, the ring and the trial cache survive a launch boundary exactly"""
    probs = U.mixed_h2() if which == "mixed" else U.slice_q3()
    runs = [run(cgo, gpu_ctx, probs, slice_iters=s) for s in (1, 3, 0)]
    for r in runs[:2]:
        assert r.handed_back == runs[2].handed_back
        for a, b in zip(r, runs[2]):
            same_bits(a, b)
    assert runs[0].launches > runs[1].launches > runs[2].launches


# ---- 9. more problems than compute units ----------------------------------------------------------------------------------------------
def test_more_problems_than_compute_units(cgo, gpu_ctx, models):
    """(the horizon is U.many's: 4 iterations, where the reference itself is determined to a tenth of the bar)"""
    out = held(cgo, gpu_ctx, U.many())
    assert len(out) == 300 and out.launches <= 2 and out.handed_back == 0


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------------
def device_memory():
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert C.CDLL(None).hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value), int(total.value)


def test_refusals(cgo, gpu_ctx, models):
    from cgo_amd import _lib
    n = 8
    X0, P = np.ones((2, n)), [np.ones((2, n)), np.zeros((2, n))]
    cfg = cgo.setupCGConfig(1e-9, cgo.LBFGS(4), cgo.EnableTrace(), max_iters=4)
    sw = cgo.setupStrongWolfeBisection(1e-5, 0.9)
    L = _lib.lib()
    h2 = _model(cgo, gpu_ctx, "H2", n)

    def c_call(model, X, params, config, ls, ctx, scalars=None, n_params=None):
        Xc = np.ascontiguousarray(X, dtype=np.float64)
        Pc = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in params]
        prows = (_lib.dp * max(len(Pc), 1))(*[v.ctypes.data_as(_lib.dp) if v is not None else None for v in Pc])
        sc = None if scalars is None else np.ascontiguousarray(scalars, dtype=np.float64)
        out, cc, lc = _lib.BatchResultsC(), config._c(), ls._c()
        out.launches = 7
        rc = L.cgo_minimize_batch_lbfgs_obj(ctx._h, model._h, Xc.shape[0], Xc.ctypes.data_as(_lib.dp), prows, len(Pc) if n_params is None else n_params,
                                            sc.ctypes.data_as(_lib.dp) if sc is not None else None, C.byref(cc), C.byref(lc), 0, C.byref(out))
        return rc, out.launches, L.cgo_last_error().decode()

    def refused(match, model=h2, X=X0, params=P, config=cfg, ls=sw, ctx=gpu_ctx, scalars=None, python=cgo.CgoError):
        with pytest.raises(python, match=match) as e:
            cgo.minimizeobjectivebatch_lbfgs_obj(model, X, config, ls, params=params, scalars=scalars, ctx=ctx)
        if python is cgo.CgoError:
            assert e.value.code == 1   # CGO_EINVAL
        rc, launches, msg = c_call(model, X, params, config, ls, ctx, scalars)   # … and through C, with the same arguments
        assert rc == 1 and launches == 0, msg
        if python is cgo.CgoError:
            assert re.search(match, msg), msg

    try:
        # of a model and of params: what cgo_minimize_batch_obj refuses
        quad = cgo.QuadDiag(np.ones(n), ctx=gpu_ctx)
        refused("run-time compiled", model=quad, params=[])
        ctx2 = cgo.Context(0)
        try:
            refused("another context", ctx=ctx2)
            ctx2.set_comm_callback(0, 2, lambda send: np.concatenate([send, send]))
            sharded = _model(cgo, ctx2, "H2", 2 * n)
            try:
                refused("multi-rank", model=sharded, X=np.ones((2, 2 * n)), params=[np.ones((2, 2 * n))] * 2, ctx=ctx2)
            finally:
                sharded.close()
        finally:
            ctx2.close()
        refused("n_params = 1", params=P[:1])
        refused("n_params = 3", params=P + [P[0]])
        refused(r"params\[1\] is", params=[P[0], None], python=ValueError)
        rc, launches, msg = c_call(h2, X0, P, cfg, sw, gpu_ctx)
        assert rc == 0 and launches >= 1, msg   # (the full call is accepted: the C refusals are no artefact of c_call)
        # of a config: what cgo_minimize_batch_lbfgs refuses
        for beta in (cgo.PolakRibiere(), cgo.HagerZhang(), cgo.BroydenFamily(0.5)):
            refused("cgo_minimize_batch_obj", config=cgo.setupCGConfig(1e-9, beta, cgo.EnableTrace(), max_iters=4))
        refused("cgo_batch_lbfgs_max_m = 10", config=cgo.setupCGConfig(1e-9, cgo.LBFGS(11), cgo.EnableTrace(), max_iters=4))
        refused("Backtracking", ls=cgo.Backtracking(cgo.Armijo(1e-4), 0.5, 100, 50))
        refused("batch must be", X=np.ones((0, n)), params=[np.ones((0, n))] * 2)
        # a scalar that is not finite
        refused("finite", scalars=np.array([1.0, np.nan]), python=ValueError)
        rc, launches, msg = c_call(h2, X0, P, cfg, sw, gpu_ctx, scalars=np.array([np.inf, 1.0]))
        assert rc == 1 and launches == 0 and "scalars[0] is not finite" in msg
        # n beyond the pass index, and cgo_batch_lbfgs_max_n_obj itself: sizes only, the host arrays are never dereferenced
        max_n = cgo.batch_lbfgs_max_n_obj(h2)
        assert max_n == cgo.batch_max_n(h2, rows="device") == cgo.batch_lbfgs_max_n("quad_diag", gpu_ctx) > 2 ** 31
        assert L.cgo_batch_lbfgs_max_n_obj(quad._h) == 0
        quad.close()
        tiny = np.ones(16)
        out, cc, lc = _lib.BatchResultsC(), cfg._c(), sw._c()
        huge = _model(cgo, gpu_ctx, "R0", max_n + 2)   # (no slots: creating it allocates nothing of that size)
        try:
            assert L.cgo_minimize_batch_lbfgs_obj(gpu_ctx._h, huge._h, 1, tiny.ctypes.data_as(_lib.dp), None, 0, None, C.byref(cc), C.byref(lc), 0, C.byref(out)) == 1
            assert "cgo_batch_lbfgs_max_n_obj" in L.cgo_last_error().decode() and out.launches == 0
        finally:
            huge.close()
        # a batch of twice the free memory: (3 + K + 2·(4+1)) vectors of batch · n doubles, refused before anything is allocated.
        # (The model is R0, K = 0: a model WITH slots of that size would itself allocate them.)
        free, total = device_memory()
        batch, vecs = 8, 3 + 0 + 2 * (4 + 1)
        n_big = int(2 * free // (8 * batch * vecs)) & ~1
        assert n_big < max_n
        big = _model(cgo, gpu_ctx, "R0", n_big)
        try:
            rc = L.cgo_minimize_batch_lbfgs_obj(gpu_ctx._h, big._h, batch, tiny.ctypes.data_as(_lib.dp), None, 0, None, C.byref(cc), C.byref(lc), 0, C.byref(out))
            msg = L.cgo_last_error().decode()
        finally:
            big.close()
        print(f"free {free} of {total} bytes; refusal: {msg}")
        assert rc == 6 and out.launches == 0 and "bytes of device memory" in msg and f"{float(vecs) * batch * n_big * 8:.0f}"[:6] in msg   # CGO_ENOMEM
        free_after, _ = device_memory()
        assert free_after >= free - (1 << 30)   # nothing is left allocated
    finally:
        h2.close()
    # the calls that refused such batches before still do
    out, cc, lc = _lib.BatchResultsC(), cfg._c(), sw._c()
    assert L.cgo_minimize_batch_lbfgs(gpu_ctx._h, 4, n, 2, X0.ctypes.data_as(_lib.dp), None, C.byref(cc), C.byref(lc), 0, C.byref(out)) == 1   # CGO_OBJ_USER
    assert "objective must be" in L.cgo_last_error().decode()
    keep, _ = models
    with pytest.raises(cgo.CgoError, match="L-BFGS") as e:
        cgo.minimizeobjectivebatch(keep["H2"], np.ones((2, 2)), cfg, sw, params=[np.ones((2, 2))] * 2, ctx=gpu_ctx)
    assert e.value.code == 1
    small = run(cgo, gpu_ctx, U.distinct("H2", 64, 4)[:2])   # … and the library is as usable as before
    assert [r.status for r in small] == ["max_iters_reached"] * 2
