"""GPU tier: batched solves on RUN-TIME COMPILED objectives with parameter slots — cgo.minimizeobjectivebatch(model, X0, …,
params=[…]) / cgo_minimize_batch_obj: k_batch<UserObjective, 3>, the batch program of the objective's module, one workgroup per
problem, every slot of every problem its own [batch, n] rows.  (CPU tier: tests/test_batch_user_abi.py.)

The bar is tests/test_batch.py's (assert_bar): bitwise status, iters_ran, trace.objective_evals, trace.step_size; ≤ 1e-10
relative on minimizer, objective, trace.objective, trace.grad_norm; ≤ 1e-9 on gradient.  Each problem is held to run_oracle of
its own Case(..., "closure", n, x0, extra={"fdf": fdf}) with the body restated as a numpy closure, as
tests/test_param_slots.py::problem does.  The bodies use + − × ÷ sqrt only, so device and numpy round alike; what is left is
the order of the sums: summing f in five orders (numpy pairwise, sequential, reversed, fsum, pairs first) leaves every step log
of the 96 problems of (1) identical and moves x, f and ∇f by ≤ 1.8e-15 — five orders of magnitude inside the bar.

Data of problem b: p = fill_uniform(n, 3 + 10b, 0.5, 4), p1 = fill_uniform(n, 5 + 10b, −2, 2), p2 = fill_uniform(n, 6 + 10b, −1, 1),
x0 = fill_uniform(n, 4 + 10b, −2, 2); the fourth slot of BODY[4], which the recipe does not name, p3 = fill_uniform(n, 7 + 10b, −1, 1).
"""
import ctypes as C
import time

import numpy as np
import pytest

from _cases import Case, O, _product_structs, run_oracle
from test_batch import assert_bar, same_bits
from test_param_slots import BODY

pytestmark = pytest.mark.gpu

H2 = "const double d = x - p1; const double r = __builtin_sqrt(1.0 + d*d); gi = p*(d/r); fi = p*(r - 1.0);"
ONE = "gi = p*x; fi = 0.5*((p*x)*x);"          # the one-slot has_param form
ROSEN0 = """
struct UserObjective {
    static constexpr bool kParam = false;
    static constexpr bool kPairOnly = true;
    __device__ static inline void eval2(d2 x, d2, double, double &f, d2 &g) {
        const double t1 = x.y - x.x * x.x;
        const double t2 = 1.0 - x.x;
        f += 100.0 * (t1 * t1) + t2 * t2;
        g.x = -400.0 * (x.x * t1) - 2.0 * t2;
        g.y = 200.0 * t1;
    }
    __device__ static inline void eval1(double, double, double, double &, double &g) { g = 0.0; }
};
"""
SOURCES = {"Q3": (BODY[3], 3), "H2": (H2, 2), "Q4": (BODY[4], 4), "ONE": (ONE, 1), "R0": (ROSEN0, 0)}


def closure(name, s):
    """the body `name` on the slots s as the reference's f = fdf!(g, x)"""
    def q(g, x):
        d = x - s[1]
        gi, fi = s[0] * d + s[2], 0.5 * ((s[0] * d) * d) + s[2] * x
        if name == "Q4":
            gi, fi = gi + s[3], fi + s[3] * x
        g[:] = gi
        return float(np.sum(fi))

    def h(g, x):
        d = x - s[1]
        r = np.sqrt(1.0 + d * d)
        g[:] = s[0] * (d / r)
        return float(np.sum(s[0] * (r - 1.0)))

    def one(g, x):
        g[:] = s[0] * x
        return float(np.sum(0.5 * ((s[0] * x) * x)))
    return {"Q3": q, "Q4": q, "H2": h, "ONE": one}[name]


def data(n, b):
    slots = (O.fill_uniform(n, 3 + 10 * b, 0.5, 4.0), O.fill_uniform(n, 5 + 10 * b, -2.0, 2.0), O.fill_uniform(n, 6 + 10 * b, -1.0, 1.0),
             O.fill_uniform(n, 7 + 10 * b, -1.0, 1.0))
    return slots, O.fill_uniform(n, 4 + 10 * b, -2.0, 2.0)


class Prob:
    """one problem of a batch: the source's name, its K slots, x0"""

    def __init__(self, name, n, b, slots=None, x0=None, tag=""):
        k = SOURCES[name][1]
        s, x = data(n, b)
        self.name, self.n, self.b, self.tag = name, n, b, tag
        self.slots = tuple(np.asarray(v, dtype=np.float64) for v in (s[:k] if slots is None else slots))
        self.x0 = x if x0 is None else np.asarray(x0, dtype=np.float64)
        assert len(self.slots) == k

    def case(self, kw):
        nm = f"{self.name}-n{self.n}-b{self.b}{self.tag}"
        if self.name == "R0":
            return Case(nm, "rosenbrock_paired", self.n, self.x0, **kw)
        return Case(nm, "closure", self.n, self.x0, extra={"fdf": closure(self.name, self.slots)}, **kw)


_ORACLE = {}


def oracle_of(p, kw):
    """run_oracle once per distinct problem and config (shared between the tests, never changed)"""
    key = (p.name, p.n, p.x0.tobytes(), tuple(v.tobytes() for v in p.slots), tuple(sorted(kw.items())))
    if key not in _ORACLE:
        _ORACLE[key] = run_oracle(p.case(kw))
    return _ORACLE[key]


PR = dict(beta="PolakRibiere", c2=0.1)
DY = dict(beta="DaiYuan", c2=0.8)
HZ_WB = dict(beta="HagerZhang", ls="WolfeBisection", cond="Wolfe", c1=1e-3, c2=0.9, ls_max_iters=100)


@pytest.fixture(scope="module")
def models(cgo, gpu_ctx):
    """Each source compiled ONCE for the whole file — the program of its creation and, with the first batched solve, the batch
    program — and one objective of each kept alive: the library shares a module between objectives of the same text while one
    of them lives.  first[name]: seconds of that first batched solve (two problems of n = 2, one iteration)."""
    keep, first = {}, {}
    for name in SOURCES:
        keep[name] = _model(cgo, gpu_ctx, name, 2)
        first[name] = _tiny_call(cgo, gpu_ctx, name, keep[name])
    yield keep, first
    for o in keep.values():
        o.close()


def _model(cgo, ctx, name, n):
    src, k = SOURCES[name]
    param = None if k == 0 else (np.ones(n) if k == 1 else [None] * k)   # (the model's own slots are neither read nor written)
    return cgo.ElementwiseObjective(n, src, param=param, ctx=ctx)


def _tiny_call(cgo, ctx, name, model):
    k = SOURCES[name][1]
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=1)
    X0 = np.array([[-1.2, 1.0], [0.5, 0.25]])
    t = time.perf_counter()
    cgo.minimizeobjectivebatch(model, X0, cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), params=[np.ones((2, 2))] * k, ctx=ctx)
    return time.perf_counter() - t


def run_batch(cgo, ctx, probs, kw, slice_iters=0):
    """the problems (one source, one size, their own x0 and slots) under one config as ONE batched solve"""
    p0 = probs[0]
    _, _, cfg, ls = _product_structs(p0.case(kw))
    model = _model(cgo, ctx, p0.name, p0.n)
    try:
        X0 = np.stack([p.x0 for p in probs])
        params = [np.stack([p.slots[j] for p in probs]) for j in range(len(p0.slots))]
        return cgo.minimizeobjectivebatch(model, X0, cfg, ls, params=params, ctx=ctx, slice_iters=slice_iters)
    finally:
        model.close()


def assert_batch(cgo, ctx, probs, kw, slice_iters=0):
    out = run_batch(cgo, ctx, probs, kw, slice_iters)
    assert len(out) == len(probs)
    for p, got in zip(probs, out):
        assert_bar(got, oracle_of(p, kw), p.case(kw).name)
    return out


# ---- 1. distinct problems ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [PR, DY, HZ_WB], ids=["PolakRibiere", "DaiYuan", "HagerZhang-WolfeBisection"])
@pytest.mark.parametrize("n", [5, 64, 513, 1000])
@pytest.mark.parametrize("name", ["Q3", "H2"])
def test_distinct_problems(cgo, gpu_ctx, models, name, n, kw):
    """Odd tail (5, 513), both branches of the two-pairs-per-trip loop, config 1's size; H2 is no quadratic, so its line
    searches go past their first trial.  Every one of the 96 problems ends max_iters_reached under the reference."""
    kw = dict(kw, eps=1e-9, max_iters=6 if n == 5 else 12)
    probs = [Prob(name, n, b) for b in range(4)]
    assert all((oracle_of(p, kw).status, oracle_of(p, kw).iters_ran) == ("max_iters_reached", kw["max_iters"]) for p in probs)
    out = assert_batch(cgo, gpu_ctx, probs, kw)
    assert out.handed_back == 0 and out.launches == 1


@pytest.mark.parametrize("n", [1, 2])
def test_no_pairs_and_one_pair(cgo, gpu_ctx, models, n):
    assert_batch(cgo, gpu_ctx, [Prob("Q3", n, b) for b in range(4)], dict(PR, eps=1e-9, max_iters=4))


def test_one_slot_form(cgo, gpu_ctx, models):
    """K = 1: the has_param form of cgo_objective_create_from_source, scalar-`p` signatures."""
    assert_batch(cgo, gpu_ctx, [Prob("ONE", 513, b) for b in range(3)], dict(DY, eps=1e-9, max_iters=12))


def test_struct_without_slots_restates_paired_rosenbrock(cgo, gpu_ctx, models):
    """K = 0, a `struct UserObjective` with kPairOnly = true: held to the oracle's own rosenbrock_paired case."""
    from _suite import rosen_x0
    n, kw = 1000, dict(DY, max_iters=12)
    probs = [Prob("R0", n, b, slots=(), x0=rosen_x0(n, seed=7 + b)) for b in range(4)]
    out = assert_batch(cgo, gpu_ctx, probs, kw)
    _, _, cfg, ls = _product_structs(probs[0].case(kw))
    builtin = cgo.minimizeobjectivebatch("rosenbrock_paired", np.stack([p.x0 for p in probs]), cfg, ls, ctx=gpu_ctx)
    same = all(np.array_equal(a.minimizer, b.minimizer) and np.array_equal(a.gradient, b.gradient) and a.objective == b.objective and
               np.array_equal(a.trace.objective, b.trace.objective) and np.array_equal(a.trace.grad_norm, b.trace.grad_norm) for a, b in zip(out, builtin))
    print(f"K = 0 struct against the built-in batched paired Rosenbrock: {'equal bit for bit' if same else 'NOT equal bit for bit'}")


# ---- 2. slots do not mix ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["H2", "Q3", "Q4"], ids=["K2", "K3", "K4"])
def test_slots_do_not_mix(cgo, gpu_ctx, models, name):
    """Every slot of every problem holds different data: a swapped, repeated or dropped slot, or a row read from another
    problem, misses the bar.  With problems 0 and 2 exchanged the results are exchanged, bit for bit."""
    kw = dict(DY, eps=1e-9, max_iters=12)
    probs = [Prob(name, 513, b) for b in range(3)]
    flat = [v.tobytes() for p in probs for v in p.slots]
    assert len(set(flat)) == len(flat)
    out = assert_batch(cgo, gpu_ctx, probs, kw)
    swapped = run_batch(cgo, gpu_ctx, [probs[2], probs[1], probs[0]], kw)
    for a, b in ((0, 2), (1, 1), (2, 0)):
        same_bits(out[a], swapped[b])
    assert not np.array_equal(out[0].minimizer, out[2].minimizer)


# ---- 3. mixed outcomes -------------------------------------------------------------------------------------------------------
MIXED = dict(beta="PolakRibiere", c2=0.8, eps=1e-5, max_iters=50)


def mixed():
    n, probs = 64, []
    for b in range(7):
        (p, p1, p2, _), x0 = data(n, b)
        if b in (2, 3, 4):
            p = {2: 2.0, 3: 4.0, 4: 0.5}[b] * np.ones(n)
        if b == 5:   # an exactly zero gradient at the start
            p2, x0 = np.zeros(n), p1.copy()
        probs.append(Prob("Q3", n, b, slots=(p, p1, p2), x0=x0, tag="-mixed"))
    return probs


def test_mixed_outcomes(cgo, gpu_ctx, models):
    probs = mixed()
    refs = [oracle_of(p, MIXED) for p in probs]
    assert [(r.status, r.iters_ran) for r in refs] == [("non_descent_search_direction", 1), ("max_iters_reached", 50), ("success", 1), ("success", 1),
                                                       ("success", 30), ("success", 0), ("non_descent_search_direction", 1)]
    out = assert_batch(cgo, gpu_ctx, probs, MIXED)
    assert out.handed_back == 2   # the two line-search failures


# ---- 4. resume at several depths -------------------------------------------------------------------------------------------
def test_hand_back_resumes_at_several_depths(cgo, gpu_ctx, models):
    """All eight end zoom_max_iters_reached: one is handed back before anything completed (the start path), seven after 1 … 6
    completed iterations (resume, with a trace prefix)."""
    n, kw = 64, dict(beta="HagerZhang", c2=0.1, zoom_max_iters=2, max_iters=30)
    probs = [Prob("H2", n, b, x0=data(n, b)[1] * (1 + b), tag="-resume") for b in range(8)]
    refs = [oracle_of(p, kw) for p in probs]
    assert [(r.status, r.iters_ran) for r in refs] == [("zoom_max_iters_reached", k) for k in (0, 1, 1, 6, 4, 3, 3, 1)]
    out = assert_batch(cgo, gpu_ctx, probs, kw)
    assert out.handed_back == 8


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Q3", "R0"], ids=["K3", "K0"])
def test_largest_problem_one_workgroup_holds(cgo, gpu_ctx, models, name):
    """n = cgo_batch_max_n_obj: the whole LDS of a CU, 2 + K vectors (two problems, so that row 1 starts where row 0 ends);
    two elements more are refused."""
    from _suite import rosen_x0
    keep, _ = models
    sizes = {nm: cgo.batch_max_n(keep[nm]) for nm in SOURCES}
    print("cgo_batch_max_n_obj: " + ", ".join(f"K = {SOURCES[nm][1]}: {sizes[nm]}" for nm in sorted(SOURCES, key=lambda nm: SOURCES[nm][1])))
    n = sizes[name]
    assert n > 0 and n % 2 == 0 and sizes["R0"] > sizes["ONE"] > sizes["H2"] > sizes["Q3"] > sizes["Q4"]
    assert sizes["R0"] == cgo.batch_max_n("rosenbrock_paired", gpu_ctx) and sizes["ONE"] == cgo.batch_max_n("quad_diag", gpu_ctx)   # the same static LDS
    probs = [Prob(name, n, b, slots=() if name == "R0" else None, x0=rosen_x0(n, seed=7 + b) if name == "R0" else None) for b in range(2)]
    assert_batch(cgo, gpu_ctx, probs, dict(PR, eps=1e-9, max_iters=4))
    big = _model(cgo, gpu_ctx, name, n + 2)
    try:
        assert cgo.batch_max_n(big) == n
        cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=4)
        with pytest.raises(cgo.CgoError, match="cgo_batch_max_n") as e:
            cgo.minimizeobjectivebatch(big, np.ones((1, n + 2)), cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1),
                                       params=[np.ones((1, n + 2))] * SOURCES[name][1], ctx=gpu_ctx)
        assert e.value.code == 1
    finally:
        big.close()


def test_more_problems_than_compute_units(cgo, gpu_ctx, models):
    out = assert_batch(cgo, gpu_ctx, [Prob("Q3", 64, b) for b in range(300)], dict(PR, eps=1e-9, max_iters=8))
    assert out.launches <= 2


def test_slicing_is_invisible(cgo, gpu_ctx, models):
    probs = mixed()
    runs = [run_batch(cgo, gpu_ctx, probs, MIXED, slice_iters=s) for s in (1, 3, 0)]
    for r in runs[:2]:
        assert r.handed_back == runs[2].handed_back
        for a, b in zip(r, runs[2]):
            same_bits(a, b)
    assert runs[0].launches > runs[2].launches


def test_trace_off(cgo, gpu_ctx, models):
    """DisableTrace: the same solves, no records kept — the device-finished problems and the hand-backs alike."""
    import dataclasses
    e, ei = np.zeros(0), np.zeros(0, dtype=np.int64)
    for probs, kw, handed in (([Prob("H2", 513, b) for b in range(3)], dict(DY, eps=1e-9, max_iters=12), 0), (mixed(), MIXED, 2)):
        out = run_batch(cgo, gpu_ctx, probs, dict(kw, trace=False))
        assert out.handed_back == handed
        for p, got in zip(probs, out):
            ref = dataclasses.replace(oracle_of(p, kw), trace_objective=e, trace_grad_norm=e, trace_step_size=e, trace_objective_evals=ei)
            assert len(got.trace.objective) == 0 and len(got.trace.grad_norm) == 0
            assert_bar(got, ref, p.case(kw).name + "-notrace")


def test_second_call_compiles_nothing(cgo, gpu_ctx, models):
    """The batch program is compiled by the first batched solve on a source and kept on its module."""
    keep, first = models
    for name in SOURCES:
        again = _tiny_call(cgo, gpu_ctx, name, keep[name])
        fresh = _model(cgo, gpu_ctx, name, 2)   # another objective of the same text: the same module
        try:
            other = _tiny_call(cgo, gpu_ctx, name, fresh)
        finally:
            fresh.close()
        print(f"{name}: first batched solve {first[name]:.3f} s (compiles the batch program), second {again * 1e3:.2f} ms, "
              f"on a second objective of the same source {other * 1e3:.2f} ms")
        if first[name] > 0.5:   # (a compile, not a cache hit of the compiler's own)
            assert again < 0.25 * first[name] and other < 0.25 * first[name]


# ---- 6. refusals, through C and through Python ------------------------------------------------------------------------------
def _c_call(cgo, ctx, model_h, X0, rows, n_params, cfg, ls):
    from cgo_amd import _lib
    L = _lib.lib()
    out = _lib.BatchResultsC()
    cc, lc = cfg._c(), ls._c()
    arr = (_lib.dp * max(len(rows), 1))(*[None if v is None else v.ctypes.data_as(_lib.dp) for v in rows])
    rc = L.cgo_minimize_batch_obj(ctx._h, model_h, X0.shape[0], X0.ctypes.data_as(_lib.dp), arr, n_params, C.byref(cc), C.byref(lc), 0, C.byref(out))
    return rc, L.cgo_last_error().decode()


@pytest.fixture()
def call(cgo, gpu_ctx, models):
    n = 8
    model = _model(cgo, gpu_ctx, "Q3", n)
    env = dict(n=n, X0=np.ones((2, n)), P=[np.ones((2, n)) * (j + 1) for j in range(3)], model=model,
               cfg=cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=4), ls=cgo.setupStrongWolfeBisection(1e-5, 0.1))
    yield env
    model.close()


def _refused(cgo, ctx, env, match, model=None, params=None, cfg=None, ls=None):
    model, params = model or env["model"], env["P"] if params is None else params
    cfg, ls = cfg or env["cfg"], ls or env["ls"]
    with pytest.raises(cgo.CgoError, match=match) as e:
        cgo.minimizeobjectivebatch(model, env["X0"], cfg, ls, params=params, ctx=ctx)
    assert e.value.code == 1   # CGO_EINVAL
    rc, msg = _c_call(cgo, ctx, model._h, env["X0"], params, len(params), cfg, ls)
    assert rc == 1 and e.value.msg == msg


def test_refuses_a_built_in_model(cgo, gpu_ctx, call):
    q = cgo.QuadDiag(np.ones(call["n"]), ctx=gpu_ctx)
    try:
        _refused(cgo, gpu_ctx, call, "cgo_minimize_batch", model=q, params=[])
        assert cgo.batch_max_n(q) == 0
    finally:
        q.close()


def test_refuses_wrong_n_params(cgo, gpu_ctx, call):
    _refused(cgo, gpu_ctx, call, "n_params = 2, the model reads 3", params=call["P"][:2])
    _refused(cgo, gpu_ctx, call, "n_params = 0, the model reads 3", params=[])


def test_refuses_a_null_slot(cgo, gpu_ctx, call):
    _refused(cgo, gpu_ctx, call, r"params\[1\] is null", params=[call["P"][0], None, call["P"][2]])


def test_refuses_lbfgs(cgo, gpu_ctx, call):
    _refused(cgo, gpu_ctx, call, "L-BFGS", cfg=cgo.setupCGConfig(1e-9, cgo.LBFGS(5), cgo.EnableTrace(), max_iters=4))


def test_refuses_backtracking(cgo, gpu_ctx, call):
    _refused(cgo, gpu_ctx, call, "Backtracking", ls=cgo.Backtracking(cgo.Armijo(1e-4), 0.5, 100, 50))


def test_kind_entry_point_still_refuses_user_objectives(cgo, gpu_ctx, call):
    from cgo_amd import _lib
    L = _lib.lib()
    out = _lib.BatchResultsC()
    cc, lc = call["cfg"]._c(), call["ls"]._c()
    X0 = call["X0"]
    rc = L.cgo_minimize_batch(gpu_ctx._h, 4, call["n"], 2, X0.ctypes.data_as(_lib.dp), call["P"][0].ctypes.data_as(_lib.dp), C.byref(cc), C.byref(lc), 0, C.byref(out))   # 4: CGO_OBJ_USER
    assert rc == 1 and "objective must be" in L.cgo_last_error().decode()
    assert L.cgo_batch_max_n(gpu_ctx._h, 4) == 0
    with pytest.raises(ValueError):
        cgo.minimizeobjectivebatch("user", X0, call["cfg"], call["ls"], ctx=gpu_ctx)
