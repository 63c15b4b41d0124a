"""Lazy direction: every second accept + direction + trial launch of a pure-HBM, host-driven solve leaves the
new u unstored, and the next launch rebuilds it from (x_{k+1}, u_k, β_k) on load.

(a) per launch, bit for bit: the lag instantiations against the PLAIN launch on the rebuilt direction — the plain launch is
    the reference, tests/test_kernel_sums.py pins it to exact references;
(b) whole solves, lazy on against lazy off in one process: every number a solve returns, bit for bit;
(c) the profile tells the truth about what ran;
(d) CPU tier: the row list, the entry point.

All GPU solvers use hbm_stream_bytes = 1.0, so that every launch takes the pure-HBM path at small n.  Sizes follow the paths
of that loop (4096 workgroups, chunks of whole 8-pair lines, two 256-pair groups per trip): n = 5 is one workgroup's remainder
path plus the odd tail; 2·4096·8 + 3 one line per workgroup; 2·4096·(512 + 256 + 8) + 1 a full two-group trip, the one-group
remainder, a partial group and the odd tail."""
import os
import re
import threading

import numpy as np
import pytest

import _instances as I
from _cases import quad_D
from _suite import reset_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_ACCEPT, R_DIR, R_TRIAL, R_GRAD, R_ULAG, R_NOWU = 1, 2, 4, 64, 1024, 2048
ADT = R_ACCEPT | R_DIR | R_TRIAL
GRID_BIG = 4096
SIZES = [5, 2 * GRID_BIG * 8 + 3, 2 * GRID_BIG * (512 + 256 + 8) + 1]


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _policy(cgo):
    return cgo.SolverPolicy(resident=False, controller_depth=0, hbm_stream_bytes=1.0)


@pytest.fixture(scope="module")
def ctx(cgo):
    c = cgo.Context(0)
    yield c
    c.close()


# ---- (a) per launch ------------------------------------------------------------------------------------------------------
def _launch_data(kind, n, seed):
    """finite, well-scaled x, u (and D); a_acc, β, β_prev and seven rising steps"""
    rng = np.random.default_rng(seed)
    if kind == "quad":
        sg = rng.choice([-1.0, 1.0], n)
        d = dict(x=sg * rng.uniform(0.5, 1, n), u=sg * rng.uniform(0.5, 1, n), p=rng.uniform(1, 2, n))
        steps = np.sort(rng.uniform(1 / 64, 1 / 8, 7))
    elif kind == "rosen":
        x, u = np.empty(n), np.empty(n)
        x[0::2] = rng.uniform(-1, -0.5, n // 2)
        x[1::2] = x[0::2] ** 2 + rng.uniform(0.5, 1, n // 2)
        u[0::2] = rng.uniform(0.05, 0.1, n // 2)
        u[1::2] = rng.uniform(0.5, 1, n // 2)
        d = dict(x=x, u=u, p=None)
        steps = np.sort(rng.uniform(1e-6, 1e-5, 7))
    else:   # Booth, n = 2
        d = dict(x=np.array([0.43, 1.23]), u=np.array([-0.7, 0.3]), p=None)
        steps = np.sort(rng.uniform(1 / 64, 1 / 8, 7))
    a_acc, beta, beta_prev = (float(v) for v in rng.uniform(1 / 32, 1 / 16, 3))
    return d, a_acc, beta, beta_prev, [float(v) for v in steps]


def _objective(cgo, kind, n, d, ctx):
    if kind == "quad":
        return cgo.QuadDiag(d["p"], ctx)
    return cgo.RosenbrockPaired(n, ctx) if kind == "rosen" else cgo.Booth(ctx)


def _check_launches(cgo, ctx, kind, n):
    d, a_acc, beta, bp, steps = _launch_data(kind, n, 11 + n % 97)
    o = _objective(cgo, kind, n, d, ctx)
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.DisableTrace(), max_iters=5)
    s = cgo.Solver(o, cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), _policy(cgo))
    bad = []
    try:
        x, u = d["x"], d["u"]
        g = s.probe_launch("init", R_GRAD, 0.0, 0.0, [], x)["g"]          # ∇f(x) as the device forms it
        u1 = -g + bp * u                                                   # one multiply, one add, no contraction
        mat = s.probe_launch("materialize_u", R_ULAG, 0.0, 0.0, [], x, u, beta_prev=bp)
        if not (mat["sums"].size == 0 and same(mat["u"], u1) and same(mat["x"], x) and mat["symbol"].endswith(", 1024, 1, true>")):
            bad.append(f"materialise: u_out != −∇f(x) + β_prev·u, x moved, or a row came back [{mat['symbol']}]")
        for k in (1, 3, 7):
            a = steps[:k]
            ref = s.probe_launch("accept_dir_trial", ADT, a_acc, beta, a, x, u1)
            B = s.probe_launch("accept_dir_trial", R_ULAG | ADT, a_acc, beta, a, x, u, beta_prev=bp)
            A = s.probe_launch("accept_trial_lazy", ADT | R_NOWU, a_acc, beta, a, x, u1)
            tag = f"{kind} n={n} k={k}"
            assert ref["symbol"].endswith("true>") and f", {ADT}, " in ref["symbol"], ref["symbol"]
            if not (B["symbol"].endswith("true>") and f", {R_ULAG | ADT}, " in B["symbol"]):
                bad.append(f"{tag}: B ran {B['symbol']}")
            if not (A["symbol"].endswith("true>") and f", {ADT | R_NOWU}, " in A["symbol"]):
                bad.append(f"{tag}: A ran {A['symbol']}")
            if not (same(B["sums"], ref["sums"]) and same(B["x"], ref["x"]) and same(B["u"], ref["u"])):
                bad.append(f"{tag}: launch B on (x, u) differs from the plain launch on (x, u′)")
            if not (same(A["sums"], ref["sums"]) and same(A["x"], ref["x"])):
                bad.append(f"{tag}: launch A's row or x_out differs from the plain launch's")
            if not same(A["u"], u1):
                bad.append(f"{tag}: launch A wrote u")
            # a trial met in the lagged state A leaves: (x_A, u′) with β_prev = β against the plain trial on the plain pair
            tref = s.probe_launch("trial", R_TRIAL, 0.0, 0.0, a, ref["x"], ref["u"])
            tlag = s.probe_launch("trial", R_ULAG | R_TRIAL, 0.0, 0.0, a, A["x"], A["u"], beta_prev=beta)
            if not (tlag["symbol"].endswith("true>") and f", {R_ULAG | R_TRIAL}, " in tlag["symbol"]):
                bad.append(f"{tag}: lagged trial ran {tlag['symbol']}")
            if not same(tlag["sums"], tref["sums"]):
                bad.append(f"{tag}: lagged trial row differs from the plain trial's")
            if not (same(tlag["x"], A["x"]) and same(tlag["u"], A["u"])):
                bad.append(f"{tag}: lagged trial wrote x or u")
    finally:
        s.close(); o.close()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES, ids=lambda n: f"n{n}")
def test_quad_lag_launches_equal_plain_launches(cgo, ctx, n):
    _check_launches(cgo, ctx, "quad", n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [n - 1 for n in SIZES], ids=lambda n: f"n{n}")
def test_rosenbrock_paired_lag_launches_equal_plain_launches(cgo, ctx, n):
    _check_launches(cgo, ctx, "rosen", n)


@pytest.mark.gpu
def test_booth_lag_launches_equal_plain_launches(cgo, ctx):
    _check_launches(cgo, ctx, "booth", 2)


# ---- (b) whole solves ----------------------------------------------------------------------------------------------------
def _solve(cgo, make_obj, cfg, ls, x0, lazy, ctx, chunk=0):
    """One solve through the Solver, lazy direction forced on or off by the setter."""
    o = make_obj(ctx)
    s = cgo.Solver(o, cfg, ls, _policy(cgo))
    try:
        s.set_lazy_direction(lazy)
        s.enable_trial_log()
        s.set_x0(x0)
        s.start()
        s.profile(True)
        while not s.iterate(chunk if chunk > 0 else 1 << 40):
            pass
        prof = s.profile_get()
        r = s.results()
        log = s.trial_log()
    finally:
        s.close(); o.close()
    return dict(r=r, log=log, prof=prof)


def _assert_equal_solves(on, off, name):
    a, b = on["r"], off["r"]
    assert a.status == b.status and a.iters_ran == b.iters_ran, (name, a.status, b.status, a.iters_ran, b.iters_ran)
    assert same(np.array([a.objective]), np.array([b.objective])), name
    for f in ("objective", "grad_norm", "step_size"):
        assert same(getattr(a.trace, f), getattr(b.trace, f)), (name, f)
    assert np.array_equal(a.trace.objective_evals, b.trace.objective_evals), name
    assert same(a.minimizer, b.minimizer) and same(a.gradient, b.gradient), name
    for la, lb in zip(on["log"], off["log"]):
        assert same(la, lb), name
    assert a.total_launches == b.total_launches and a.total_fdf_evals == b.total_fdf_evals, name
    assert "accept_trial_lazy" not in off["prof"] and "materialize_u" not in off["prof"], name


def _pair(cgo, ctx, make_obj, cfg, ls, x0, name, chunk=0, expect_lazy=True):
    on = _solve(cgo, make_obj, cfg, ls, x0, True, ctx, chunk)
    off = _solve(cgo, make_obj, cfg, ls, x0, False, ctx, chunk)
    _assert_equal_solves(on, off, name)
    if expect_lazy:
        assert on["prof"].get("accept_trial_lazy", {}).get("launches", 0) >= 1, (name, on["prof"])
    return on, off


N_MID = 2 * GRID_BIG * 8 + 3


def _quad(cgo, n):
    D = quad_D(n)
    return lambda ctx: cgo.QuadDiag(D, ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("max_iters", [7, 8], ids=lambda m: f"it{m}")
def test_quad_pr_strong_wolfe_lazy_equals_plain(cgo, ctx, max_iters):
    """odd and even horizons: results are fetched once in the lagged and once in the plain state"""
    cfg = cgo.setupCGConfig(1e-12, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=max_iters)
    on, _ = _pair(cgo, ctx, _quad(cgo, N_MID), cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), np.ones(N_MID), f"quad-PR-{max_iters}")
    assert on["r"].iters_ran == max_iters


@pytest.mark.gpu
@pytest.mark.parametrize("max_iters", [4, 5], ids=lambda m: f"it{m}")
def test_rosenbrock_paired_pr_strong_wolfe_lazy_equals_plain(cgo, ctx, max_iters):
    n = 1000
    cfg = cgo.setupCGConfig(1e-5, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=max_iters)
    _pair(cgo, ctx, lambda c: cgo.RosenbrockPaired(n, c), cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), np.tile([-1.2, 1.0], n // 2),
          f"rosen-PR-{max_iters}")


@pytest.mark.gpu
def test_wolfe_bisection_reset_and_upg_path_lazy_equals_plain(cgo, ctx):
    """WolfeBisection's bracket collapse (wolfe.jl:122-130): ‖u + g‖² reads the direction, the reset overwrites it"""
    c = reset_cases()[0]
    from _cases import _product_structs
    _, _, cfg, ls = _product_structs(c)
    on, _ = _pair(cgo, ctx, lambda cx: cgo.RosenbrockPaired(c.n, cx), cfg, ls, c.x0, c.name)
    assert on["prof"].get("upg_norm", {}).get("launches", 0) >= 1 and on["prof"].get("reset_dir", {}).get("launches", 0) >= 1, on["prof"]
    assert on["prof"].get("materialize_u", {}).get("launches", 0) >= 1, on["prof"]


@pytest.mark.gpu
def test_failing_status_returns_the_last_good_iterate_lazy_equals_plain(cgo, ctx):
    n = 64
    x0 = np.ones(n)
    # plain PR + loose curvature condition: an ascent direction at iteration 2 (nocedal.jl:57-63)
    cfg = cgo.setupCGConfig(1e-5, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=50)
    on, _ = _pair(cgo, ctx, _quad(cgo, n), cfg, cgo.setupStrongWolfeBisection(1e-5, 0.8), x0, "st-nondescent")
    assert on["r"].status == "non_descent_search_direction"
    cfg = cgo.setupCGConfig(1e-5, cgo.HagerZhang(), cgo.EnableTrace(), max_iters=50)
    on, _ = _pair(cgo, ctx, _quad(cgo, n), cfg, cgo.StrongWolfeBisection(1e-5, 0.8, 2.0, 1000, 2), x0, "st-zoom", expect_lazy=False)
    assert on["r"].status == "zoom_max_iters_reached"


@pytest.mark.gpu
def test_single_iteration_slices_equal_one_call(cgo, ctx):
    cfg = cgo.setupCGConfig(1e-12, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=9)
    ls = cgo.setupStrongWolfeBisection(1e-5, 0.1)
    whole = _solve(cgo, _quad(cgo, N_MID), cfg, ls, np.ones(N_MID), True, ctx)
    sliced = _solve(cgo, _quad(cgo, N_MID), cfg, ls, np.ones(N_MID), True, ctx, chunk=1)
    plain = _solve(cgo, _quad(cgo, N_MID), cfg, ls, np.ones(N_MID), False, ctx, chunk=1)
    _assert_equal_solves(sliced, plain, "slices")
    _assert_equal_solves(whole, plain, "whole")


@pytest.mark.gpu
def test_rerun_chain_lazy_equals_plain(cgo, monkeypatch):
    """cgo_minimize_rerun builds its solvers itself: the context's default policy and CGO_LAZY_DIR reach them"""
    n = N_MID
    D = quad_D(n)
    ls = cgo.setupStrongWolfeBisection(1e-5, 0.1)
    cfgs = [cgo.setupCGConfig(e, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=m) for e, m in ((1e-2, 5), (1e-4, 4), (1e-6, 6))]
    out = {}
    for lazy in ("1", "0"):
        monkeypatch.setenv("CGO_LAZY_DIR", lazy)
        c = cgo.Context(0)
        c.set_default_policy(_policy(cgo))
        o = cgo.QuadDiag(D, c)
        try:
            out[lazy] = cgo.minimizeobjectivererun(o, np.ones(n), cfgs[0], ls, (cfgs[1], ls), (cfgs[2], ls))
        finally:
            o.close(); c.close()
    assert len(out["1"]) == len(out["0"]) >= 2
    for a, b in zip(out["1"], out["0"]):
        assert a.status == b.status and a.iters_ran == b.iters_ran and a.total_launches == b.total_launches
        assert same(np.array([a.objective]), np.array([b.objective])) and same(a.minimizer, b.minimizer) and same(a.gradient, b.gradient)
        assert same(a.trace.objective, b.trace.objective) and same(a.trace.grad_norm, b.trace.grad_norm) and same(a.trace.step_size, b.trace.step_size)


@pytest.mark.gpu
def test_two_virtual_ranks_lazy_equals_plain(cgo):
    """two contexts of one process as two ranks over the callback transport, each with its contiguous shard"""
    n, W = 2 * N_MID, 2
    D = quad_D(n)
    cfg = cgo.setupCGConfig(1e-12, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=7)
    ls = cgo.setupStrongWolfeBisection(1e-5, 0.1)

    def run(lazy):
        bar = threading.Barrier(W)
        slots, outs, errs = [None] * W, [None] * W, []

        def make_allgather(rank):
            def ag(send):
                slots[rank] = send.copy()
                bar.wait()
                out = np.concatenate(slots)
                bar.wait()
                return out
            return ag

        def worker(rank):
            try:
                c = cgo.Context(0)
                c.set_comm_callback(rank, W, make_allgather(rank))
                outs[rank] = _solve(cgo, lambda cx: cgo.QuadDiag(D, cx), cfg, ls, np.ones(n), lazy, c)
                c.close()
            except Exception as e:  # pragma: no cover
                errs.append(e)
                bar.abort()
        ts = [threading.Thread(target=worker, args=(r,)) for r in range(W)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        assert not errs, errs
        return outs
    on, off = run(True), run(False)
    for r in range(W):
        _assert_equal_solves(on[r], off[r], f"rank {r}")
        assert on[r]["prof"].get("accept_trial_lazy", {}).get("launches", 0) >= 1


# ---- (c) profile ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_profile_names_what_ran(cgo, ctx, monkeypatch):
    n, k = N_MID, 6
    cfg = cgo.setupCGConfig(1e-300, cgo.PolakRibiere(), cgo.DisableTrace(), max_iters=2 * k)
    ls = cgo.setupStrongWolfeBisection(1e-5, 0.1)

    def run(env):
        if env is None:
            monkeypatch.delenv("CGO_LAZY_DIR", raising=False)
        else:
            monkeypatch.setenv("CGO_LAZY_DIR", env)
        o = cgo.QuadDiag(quad_D(n), ctx)
        s = cgo.Solver(o, cfg, ls, _policy(cgo))
        try:
            s.set_x0(np.ones(n)); s.start()
            s.profile(True); s.profile_reset()
            while not s.iterate(2 * k):      # max_iters = 2k: the solve ends there
                pass
            return s.profile_get(), s.kernel_symbol("accept_dir_trial"), s.kernel_symbol("accept_trial_lazy"), s.results(vectors=False)
        finally:
            s.close(); o.close()
    prof, sym, sym_a, r = run(None)          # library policy: on for the separable quadratic
    off, sym_off, sym_a_off, r_off = run("0")
    assert r.iters_ran == r_off.iters_ran == 2 * k
    A, B = prof["accept_trial_lazy"], prof["accept_dir_trial"]
    mat = prof.get("materialize_u", {}).get("launches", 0)
    assert A["launches"] + B["launches"] == off["accept_dir_trial"]["launches"]
    assert 0 <= A["launches"] - B["launches"] <= 1 + mat and B["launches"] >= k - 1 - mat
    assert A["bytes_per_launch"] == 8.0 * n * 4 and B["bytes_per_launch"] == 8.0 * n * 5     # 8n(2 + p + 1), 8n(2 + p + 2), p = 1
    assert sym.endswith("true>") and ", 7, " in sym and f", {R_ULAG | ADT}, " in sym, sym
    assert sym_a == f"k_cg<ObjQuadDiag, {ADT | R_NOWU}, 7, true>", sym_a
    assert "accept_trial_lazy" not in off and "materialize_u" not in off
    assert sym_off == "k_cg<ObjQuadDiag, 7, 7, true>" and sym_a_off == "", (sym_off, sym_a_off)
    assert off["accept_dir_trial"]["bytes_per_launch"] == 8.0 * n * 5


# ---- (d) CPU tier --------------------------------------------------------------------------------------------------------
def test_lag_rows_parse_and_are_what_the_backend_alternates_between(monkeypatch):
    monkeypatch.setitem(I.BITS, "R_ULAG", R_ULAG)
    monkeypatch.setitem(I.BITS, "R_NOWU", R_NOWU)
    assert I.rows("CG_LAG") == [(ADT | R_NOWU, 7), (R_ULAG | ADT, 7), (R_ULAG | R_TRIAL, 7), (R_ULAG, 1)]
    assert not {m for m, _ in I.rows("CG_LAG")} & {m for m, _ in I.rows("CG")}       # the pinned list is untouched
    assert I.stray_uses() == []
    hdr = open(os.path.join(I.CSRC, "cgo_modes.hpp")).read()
    assert re.search(r"R_ULAG = 1024\b", hdr) and re.search(r"R_NOWU = 2048\b", hdr)


def test_entry_point_is_declared_exported_and_bound(cgo):
    from cgo_amd import _lib
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cgo.h")).read(), flags=re.S)
    for name in ("cgo_solver_set_lazy_direction", "cgo_solver_probe_set_beta_prev"):
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert hasattr(cgo.Solver, "set_lazy_direction")
    kinds = [L.cgo_kernel_kind_name(k).decode() for k in range(L.cgo_num_kernel_kinds())]
    assert kinds[-2:] == ["accept_trial_lazy", "materialize_u"] and kinds[:3] == ["init", "trial", "accept_dir_trial"]
    assert "CGO_LAZY_DIR" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
