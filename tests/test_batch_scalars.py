"""GPU tier: batched solves with a SCALAR PER PROBLEM and a batch that stays on the device between solves — cgo.Batch /
cgo_batch_open, cgo_batch_solve, cgo_batch_close; cgo.minimizeobjectivebatch(..., scalars=).  k_batch reads s0v[b] in place of the
launch's s0, and Results.gradient comes from k_batch_grad, a workgroup per row with the row's own scalar.  (CPU tier:
tests/test_batch_scalars_abi.py.)

The bar is tests/test_batch.py's (assert_bar), unchanged: bitwise status, iters_ran, trace.objective_evals, trace.step_size;
≤ 1e-10 relative on minimizer, objective, trace.objective, trace.grad_norm; ≤ 1e-9 on gradient.  Each problem is held to
run_oracle of its own closure — the body restated in numpy WITH ITS SCALAR, operation for operation.

Data of problem b: tests/test_batch_user.py's (p, p1, p2 = fill_uniform(n, 3 | 5 | 6 + 10b, …), x0 = fill_uniform(n, 4 + 10b, −2, 2));
scalars SCALARS[b] = 1e-3, 1, 1e3, 2e-3, 2, 2e3 — neighbours a factor 1e3 apart."""
import ctypes as C
import time

import numpy as np
import pytest

from _cases import Case, _product_structs, rel, run_oracle
from test_batch import assert_bar, same_bits
from test_batch_user import DY, HZ_WB, MIXED, PR, data, mixed
from test_param_slots import BODY

pytestmark = pytest.mark.gpu

SQ = "gi = s0*p*(x - p1); fi = 0.5*s0*((p*(x - p1))*(x - p1));"
SH = "const double d = x - p1; const double r = __builtin_sqrt(1.0 + d*d); gi = s0*(p*(d/r)); fi = s0*(p*(r - 1.0));"
SM = "const double d = x - p1; gi = s0*(p*d + p2); fi = s0*(0.5*((p*d)*d) + p2*x);"   # the mixed-outcome recipe's body, scaled
SOURCES = {"SQ": (SQ, 2), "SH": (SH, 2), "SM": (SM, 3), "Q3": (BODY[3], 3)}
SCALARS = np.array([1e-3, 1.0, 1e3, 2e-3, 2.0, 2e3])
SIZES = [1, 2, 5, 64, 513]   # no pair, one pair, the odd tail, one trip of the row loop, more than one trip with an odd tail


def closure(name, s, s0):
    def sq(g, x):
        d = x - s[1]
        g[:] = (s0 * s[0]) * d
        return float(np.sum((0.5 * s0) * ((s[0] * d) * d)))

    def sh(g, x):
        d = x - s[1]
        r = np.sqrt(1.0 + d * d)
        g[:] = s0 * (s[0] * (d / r))
        return float(np.sum(s0 * (s[0] * (r - 1.0))))

    def sm(g, x):
        d = x - s[1]
        g[:] = s0 * (s[0] * d + s[2])
        return float(np.sum(s0 * (0.5 * ((s[0] * d) * d) + s[2] * x)))

    def q3(g, x):   # BODY[3] reads no scalar
        d = x - s[1]
        g[:] = s[0] * d + s[2]
        return float(np.sum(0.5 * ((s[0] * d) * d) + s[2] * x))
    return {"SQ": sq, "SH": sh, "SM": sm, "Q3": q3}[name]


class Prob:
    """one problem of a batch: the source's name, its K slots, x0 and its own scalar"""

    def __init__(self, name, n, b, s0, slots=None, x0=None):
        k = SOURCES[name][1]
        s, x = data(n, b)
        self.name, self.n, self.b, self.s0 = name, n, b, float(s0)
        self.slots = tuple(np.asarray(v, dtype=np.float64) for v in (s[:k] if slots is None else slots))
        self.x0 = x if x0 is None else np.asarray(x0, dtype=np.float64)

    def case(self, kw):
        return Case(f"{self.name}-n{self.n}-b{self.b}-s{self.s0:g}", "closure", self.n, self.x0,
                    extra={"fdf": closure(self.name, self.slots, self.s0)}, **kw)


_ORACLE = {}


def oracle_of(p, kw):
    """run_oracle once per distinct problem, scalar and config (shared between the tests, never changed)"""
    key = (p.name, p.n, p.s0, p.x0.tobytes(), tuple(v.tobytes() for v in p.slots), tuple(sorted(kw.items())))
    if key not in _ORACLE:
        _ORACLE[key] = run_oracle(p.case(kw))
    return _ORACLE[key]


def _model(cgo, ctx, name, n):
    return cgo.ElementwiseObjective(n, SOURCES[name][0], param=[None] * SOURCES[name][1], ctx=ctx)


def _arrays(probs):
    X0 = np.stack([p.x0 for p in probs])
    params = [np.stack([p.slots[j] for p in probs]) for j in range(len(probs[0].slots))]
    return X0, params, np.array([p.s0 for p in probs])


def _tiny_call(cgo, ctx, name, model):
    k = SOURCES[name][1]
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=1)
    X0 = np.array([[-1.2, 1.0], [0.5, 0.25]])
    t = time.perf_counter()
    cgo.minimizeobjectivebatch(model, X0, cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), params=[np.ones((2, 2))] * k, ctx=ctx,
                               scalars=np.array([1.0, 2.0]))
    return time.perf_counter() - t


@pytest.fixture(scope="module")
def models(cgo, gpu_ctx):
    """Each source compiled ONCE for the whole file, one objective of each kept alive (the library shares a module between
    objectives of the same text while one of them lives).  first[name]: seconds of the first batched solve on it, which
    compiles the batch program — k_batch and k_batch_grad."""
    keep, first = {}, {}
    for name in SOURCES:
        keep[name] = _model(cgo, gpu_ctx, name, 2)
        first[name] = _tiny_call(cgo, gpu_ctx, name, keep[name])
    yield keep, first
    for o in keep.values():
        o.close()


def one_shot(cgo, ctx, probs, kw, scalars=True, slice_iters=0, model_scalar=None):
    _, _, cfg, ls = _product_structs(probs[0].case(kw))
    model = _model(cgo, ctx, probs[0].name, probs[0].n)
    try:
        if model_scalar is not None:
            model.set_scalar(model_scalar)
        X0, params, sc = _arrays(probs)
        return cgo.minimizeobjectivebatch(model, X0, cfg, ls, params=params, ctx=ctx, slice_iters=slice_iters, scalars=sc if scalars else None)
    finally:
        model.close()


def assert_batch(cgo, ctx, probs, kw):
    out = one_shot(cgo, ctx, probs, kw)
    assert len(out) == len(probs)
    for p, got in zip(probs, out):   # every problem of the batch
        assert_bar(got, oracle_of(p, kw), p.case(kw).name)
    return out


def LS_GAVE_UP(status):
    return status not in ("success", "max_iters_reached", "increasing_objective")


def six(name, n):
    return [Prob(name, n, b, SCALARS[b]) for b in range(6)]


# ---- 1. distinct scalars ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name,kw", [("SQ", PR), ("SH", DY), ("SH", HZ_WB)], ids=["quadratic-PolakRibiere", "H2-DaiYuan", "H2-HagerZhang-WolfeBisection"])
def test_distinct_scalars(cgo, gpu_ctx, models, name, kw, n):
    kw = dict(kw, eps=1e-9, max_iters=4 if n <= 2 else (6 if n == 5 else 12))
    probs = six(name, n)
    out = assert_batch(cgo, gpu_ctx, probs, kw)
    assert out.handed_back == sum(LS_GAVE_UP(oracle_of(p, kw).status) for p in probs)   # (n ≤ 2: a quadratic solved exactly ends :non_descent_search_direction)


# ---- 2. the results' gradient ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_results_gradient_is_formed_with_the_problems_own_scalar(cgo, gpu_ctx, models, n):
    """Results.gradient of every problem against the oracle's, ≤ 1e-9 (the ∇f entry of the bar).  One launch over the
    concatenated rows has ONE scalar: whichever it took, the gradient of the five problems with another scalar would be off by
    the ratio of the two, a factor ≥ 2."""
    kw = dict(DY, eps=1e-9, max_iters=4 if n <= 2 else 6)
    probs = six("SH", n)
    out = one_shot(cgo, gpu_ctx, probs, kw)
    for p, got in zip(probs, out):
        ref = oracle_of(p, kw)
        fig = rel(got.gradient, ref.gradient)
        print(f"{p.case(kw).name}: gradient {fig:.2e}")
        assert got.gradient.shape == (n,) and fig <= 1e-9, (p.b, fig)


# ---- 3. rows exchanged -------------------------------------------------------------------------------------------------------
def test_rows_and_scalars_exchanged(cgo, gpu_ctx, models):
    kw = dict(DY, eps=1e-9, max_iters=12)
    probs = six("SH", 513)
    out = assert_batch(cgo, gpu_ctx, probs, kw)
    order = [4, 1, 2, 3, 0, 5]
    swapped = one_shot(cgo, gpu_ctx, [probs[i] for i in order], kw)
    for pos, i in enumerate(order):
        same_bits(out[i], swapped[pos])
    assert not np.array_equal(out[0].minimizer, out[4].minimizer)


# ---- 4. scalars change nothing else ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 513])
def test_equal_scalars_equal_the_models_scalar(cgo, gpu_ctx, models, n):
    """scalars = full(batch, s) against the model's scalar set to s: every status, count, step, f, x and trace entry bit for
    bit; the gradient to the bar, since it comes from the other kernel."""
    s, kw = 37.5, dict(DY, eps=1e-9, max_iters=12)
    probs = [Prob("SH", n, b, s) for b in range(6)]
    with_v = one_shot(cgo, gpu_ctx, probs, kw)
    with_m = one_shot(cgo, gpu_ctx, probs, kw, scalars=False, model_scalar=s)
    for a, b in zip(with_v, with_m):
        for f in ("objective", "iters_ran", "status", "total_fdf_evals"):
            assert getattr(a, f) == getattr(b, f), f
        assert np.array_equal(a.minimizer, b.minimizer)
        for f in ("objective", "grad_norm", "step_size", "objective_evals"):
            assert np.array_equal(getattr(a.trace, f), getattr(b.trace, f)), "trace." + f
        assert rel(a.gradient, b.gradient) <= 1e-9
    for p, got in zip(probs, with_v):
        assert_bar(got, oracle_of(p, kw), p.case(kw).name)


# ---- 5. a call without scalars is the call it was ------------------------------------------------------------------------------
def test_batch_solve_without_scalars_is_minimizeobjectivebatch(cgo, gpu_ctx, models):
    kw = dict(DY, eps=1e-9, max_iters=12)
    probs = [Prob("Q3", 513, b, 1.0) for b in range(4)]
    _, _, cfg, ls = _product_structs(probs[0].case(kw))
    X0, params, _ = _arrays(probs)
    model = _model(cgo, gpu_ctx, "Q3", 513)
    try:
        ref = cgo.minimizeobjectivebatch(model, X0, cfg, ls, params=params, ctx=gpu_ctx)
        with cgo.Batch(model, params, len(probs)) as B:
            got = B.solve(X0, cfg, ls)
    finally:
        model.close()
    assert (got.launches, got.handed_back) == (ref.launches, ref.handed_back)
    for a, b in zip(got, ref):
        same_bits(a, b)   # the gradient too: the same launch over the concatenated rows
    for p, r in zip(probs, got):
        assert_bar(r, oracle_of(p, kw), p.case(kw).name)


# ---- 6. the active mask --------------------------------------------------------------------------------------------------------
def test_active_mask(cgo, gpu_ctx, models):
    from cgo_amd import _lib
    kw = dict(DY, eps=1e-9, max_iters=12)
    n, probs = 64, six("SH", 64)
    full = assert_batch(cgo, gpu_ctx, probs, kw)
    _, _, cfg, ls = _product_structs(probs[0].case(kw))
    X0, params, sc = _arrays(probs)
    active = np.array([1, 0, 1, 0, 0, 1], dtype=bool)
    model = _model(cgo, gpu_ctx, "SH", n)
    try:
        with cgo.Batch(model, params, 6) as B:
            got = B.solve(X0, cfg, ls, scalars=sc, active=active)
            for b in range(6):
                if active[b]:
                    same_bits(got[b], full[b])
                else:
                    assert got[b] is None
            # through the C entry: the rows of an inactive problem still hold what the caller wrote
            S = -12345.0
            f, x, g = np.full(6, S), np.full((6, n), S), np.full((6, n), S)
            it, ev, st = np.full(6, -7, dtype=np.int64), np.full(6, -7, dtype=np.int64), np.full(6, -7, dtype=np.int32)
            cap = kw["max_iters"]
            to, tg, ts, te = np.full((6, cap), S), np.full((6, cap), S), np.full((6, cap), S), np.full((6, cap), -7, dtype=np.int64)
            r = _lib.BatchResultsC()
            r.objective, r.iters_ran, r.status = f.ctypes.data_as(_lib.dp), it.ctypes.data_as(_lib.i64p), st.ctypes.data_as(C.POINTER(C.c_int32))
            r.total_fdf_evals, r.minimizer, r.gradient = ev.ctypes.data_as(_lib.i64p), x.ctypes.data_as(_lib.dp), g.ctypes.data_as(_lib.dp)
            r.trace_objective, r.trace_grad_norm, r.trace_step_size = to.ctypes.data_as(_lib.dp), tg.ctypes.data_as(_lib.dp), ts.ctypes.data_as(_lib.dp)
            r.trace_objective_evals = te.ctypes.data_as(_lib.i64p)
            cc, lc, a8 = cfg._c(), ls._c(), active.astype(np.uint8)
            rc = _lib.lib().cgo_batch_solve(B._h, X0.ctypes.data_as(_lib.dp), sc.ctypes.data_as(_lib.dp), a8.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            C.byref(cc), C.byref(lc), 0, C.byref(r))
            assert rc == 0, _lib.lib().cgo_last_error().decode()
    finally:
        model.close()
    for b in range(6):
        if active[b]:
            assert f[b] == full[b].objective and it[b] == full[b].iters_ran and np.array_equal(x[b], full[b].minimizer) and np.array_equal(g[b], full[b].gradient)
            assert np.array_equal(ts[b, :it[b]], full[b].trace.step_size)
        else:
            assert f[b] == S and it[b] == -7 and ev[b] == -7 and st[b] == -7 and np.all(x[b] == S) and np.all(g[b] == S)
            assert np.all(to[b] == S) and np.all(tg[b] == S) and np.all(ts[b] == S) and np.all(te[b] == -7)


# ---- 7. reuse --------------------------------------------------------------------------------------------------------------------
def test_one_batch_many_solves(cgo, gpu_ctx, models):
    keep, first = models
    n = 513
    kw1, kw2 = dict(DY, eps=1e-9, max_iters=12), dict(HZ_WB, eps=1e-9, max_iters=8)
    p1 = six("SH", n)
    p2 = [Prob("SH", n, b, SCALARS[5 - b]) for b in range(6)]   # the same rows, other scalars
    fresh1, fresh2 = one_shot(cgo, gpu_ctx, p1, kw1), one_shot(cgo, gpu_ctx, p2, kw2)
    X0, params, s1 = _arrays(p1)
    _, _, s2 = _arrays(p2)
    _, _, cfg1, ls1 = _product_structs(p1[0].case(kw1))
    _, _, cfg2, ls2 = _product_structs(p2[0].case(kw2))
    model = _model(cgo, gpu_ctx, "SH", n)
    try:
        with cgo.Batch(model, params, 6) as B:
            a = B.solve(X0, cfg1, ls1, scalars=s1)
            b = B.solve(X0, cfg2, ls2, scalars=s2)
            t = time.perf_counter()
            c = B.solve(X0, cfg1, ls1, scalars=s1)
            third = time.perf_counter() - t
    finally:
        model.close()
    for got, ref in ((a, fresh1), (b, fresh2), (c, fresh1)):
        assert (got.launches, got.handed_back) == (ref.launches, ref.handed_back)
        for x, y in zip(got, ref):
            same_bits(x, y)
    for p, r in zip(p2, b):
        assert_bar(r, oracle_of(p, kw2), p.case(kw2).name)
    print(f"SH: first batched solve {first['SH']:.3f} s (compiles the batch program), a third solve on an open batch {third * 1e3:.2f} ms")
    if first["SH"] > 0.5:   # (a compile, not a cache hit of the compiler's own)
        assert third < 0.25 * first["SH"]


# ---- 8. hand-back ----------------------------------------------------------------------------------------------------------------
def test_hand_back_under_the_problems_own_scalar(cgo, gpu_ctx, models):
    """tests/test_batch_user.py::mixed with the body scaled by s0 and a scalar per problem: the problems whose line search gives
    up are finished by the host engine — on the call's own objective, which must carry THAT problem's scalar to meet the bar."""
    sc = [1e-3, 1.0, 1e3, 2e-3, 2.0, 2e3, 5e2]
    probs = [Prob("SM", q.n, q.b, sc[q.b], slots=q.slots, x0=q.x0) for q in mixed()]
    refs = [oracle_of(p, MIXED) for p in probs]
    expect = sum(LS_GAVE_UP(r.status) for r in refs)
    print("oracle: " + ", ".join(f"{r.status}/{r.iters_ran}" for r in refs))
    assert expect >= 2 and len({r.status for r in refs}) >= 3
    out = assert_batch(cgo, gpu_ctx, probs, MIXED)
    assert out.handed_back == expect


# ---- 9. refusals, through C and through Python -------------------------------------------------------------------------------------
@pytest.fixture()
def env(cgo, gpu_ctx, models):
    n = 8
    model = _model(cgo, gpu_ctx, "SQ", n)
    e = dict(n=n, X0=np.ones((2, n)), P=[np.ones((2, n)) * (j + 1) for j in range(2)], model=model,
             cfg=cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=4), ls=cgo.setupStrongWolfeBisection(1e-5, 0.1))
    e["B"] = cgo.Batch(model, e["P"], 2)
    yield e
    e["B"].close()
    model.close()


def _refused(cgo, env, match, scalars=None, active=None, cfg=None, ls=None):
    from cgo_amd import _lib
    cfg, ls = cfg or env["cfg"], ls or env["ls"]
    with pytest.raises(cgo.CgoError, match=match) as e:
        env["B"].solve(env["X0"], cfg, ls, scalars=scalars, active=active)
    assert e.value.code == 1   # CGO_EINVAL
    out = _lib.BatchResultsC()
    cc, lc = cfg._c(), ls._c()
    sc = None if scalars is None else np.asarray(scalars, dtype=np.float64)
    ac = None if active is None else np.asarray(active, dtype=np.uint8)
    rc = _lib.lib().cgo_batch_solve(env["B"]._h, env["X0"].ctypes.data_as(_lib.dp), None if sc is None else sc.ctypes.data_as(_lib.dp),
                                    None if ac is None else ac.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(cc), C.byref(lc), 0, C.byref(out))
    assert rc == 1 and _lib.lib().cgo_last_error().decode() == e.value.msg


def test_refuses_a_non_finite_scalar(cgo, env):
    _refused(cgo, env, r"scalars\[1\] is not finite", scalars=[1.0, np.nan])
    _refused(cgo, env, r"scalars\[0\] is not finite", scalars=[np.inf, 1.0])
    with pytest.raises(cgo.CgoError, match="not finite"):
        cgo.minimizeobjectivebatch(env["model"], env["X0"], env["cfg"], env["ls"], params=env["P"], scalars=[np.nan, 1.0])


def test_refuses_an_active_mask_that_selects_nothing(cgo, env):
    _refused(cgo, env, "active selects no problem", active=[0, 0])


def test_refuses_scalars_with_a_built_in_kind(cgo, gpu_ctx, env):
    with pytest.raises(ValueError, match="reads no scalar"):
        cgo.minimizeobjectivebatch("quad_diag", env["X0"], env["cfg"], env["ls"], D=np.ones((2, env["n"])), ctx=gpu_ctx, scalars=[1.0, 2.0])


def test_refuses_lbfgs_and_backtracking(cgo, env):
    _refused(cgo, env, "L-BFGS", cfg=cgo.setupCGConfig(1e-9, cgo.LBFGS(5), cgo.EnableTrace(), max_iters=4))
    _refused(cgo, env, "Backtracking", ls=cgo.Backtracking(cgo.Armijo(1e-4), 0.5, 100, 50))
    got = env["B"].solve(env["X0"], env["cfg"], env["ls"], scalars=[1.0, 2.0])   # the batch is as good as before
    assert len(got) == 2 and got[0] is not None
