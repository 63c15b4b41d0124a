"""Replay: at depth d ≥ 2, d − 1 of every d accept + direction + trial launches of a pure-HBM, host-driven solve
store neither x nor u — each rebuilds the current pair in registers from the stored (x_k, u_k) and the (a*, β) of the steps
accepted since — and the d-th replays them and stores both.

(1) per launch, bit for bit: the replay instantiations on (x_0, u_0) with a list of r steps against the PLAIN launch on
    (x_r, u_r), built by r plain accept + direction launches — the plain launch is the reference, tests/test_kernel_sums.py pins
    it to exact references;
(2) whole solves, replay on against lazy off in one process: every number a solve returns, bit for bit;
(3) the profile tells the truth about what ran;
(4) CPU tier: the row list, the entry points.

All GPU solvers use hbm_stream_bytes = 1.0, so that every launch takes the pure-HBM path at small n; the sizes are those of
tests/test_lazy_direction.py (4096 workgroups, chunks of whole 8-pair lines, two 256-pair groups per trip): n = 5 is one
workgroup's remainder path plus the odd tail; 2·4096·8 + 3 one line per workgroup; 2·4096·(512 + 256 + 8) + 1 a full two-group
trip, the one-group remainder, a partial group and the odd tail."""
import os
import re
import threading

import numpy as np
import pytest

import _instances as I
from _cases import quad_D
from _suite import reset_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_ACCEPT, R_DIR, R_TRIAL, R_NOWU, R_REPLAY, R_NOWX = 1, 2, 4, 2048, 4096, 8192
ADT = R_ACCEPT | R_DIR | R_TRIAL
MODE_N, MODE_S, MODE_T, MODE_M = R_REPLAY | ADT | R_NOWU | R_NOWX, R_REPLAY | ADT, R_REPLAY | R_TRIAL, R_REPLAY
GRID_BIG = 4096
SIZES = [5, 2 * GRID_BIG * 8 + 3, 2 * GRID_BIG * (512 + 256 + 8) + 1]
REPLAYED = [0, 1, 2, 7]
NEW_KINDS = ("accept_trial_nostore", "materialize_xu")


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


# ---- (1) per launch ------------------------------------------------------------------------------------------------------
def _launch_data(kind, n, seed):
    """finite, well-scaled x, u (and D); seven (a*, β) pairs to replay, a_acc, β and seven rising steps"""
    rng = np.random.default_rng(seed)
    if kind == "quad":
        sg = rng.choice([-1.0, 1.0], n)
        d = dict(x=sg * rng.uniform(0.5, 1, n), u=sg * rng.uniform(0.5, 1, n), p=rng.uniform(1, 2, n))
        steps = np.sort(rng.uniform(1 / 64, 1 / 8, 7))
        ra = rng.uniform(1 / 32, 1 / 16, 8)
    elif kind == "rosen":
        x, u = np.empty(n), np.empty(n)
        x[0::2] = rng.uniform(-1, -0.5, n // 2)
        x[1::2] = x[0::2] ** 2 + rng.uniform(0.5, 1, n // 2)
        u[0::2] = rng.uniform(0.05, 0.1, n // 2)
        u[1::2] = rng.uniform(0.5, 1, n // 2)
        d = dict(x=x, u=u, p=None)
        steps = np.sort(rng.uniform(1e-6, 1e-5, 7))
        ra = rng.uniform(1e-5, 1e-4, 8)          # |∇f| is in the hundreds here: steps that keep the eight iterates in the valley
    else:   # Booth, n = 2
        d = dict(x=np.array([0.43, 1.23]), u=np.array([-0.7, 0.3]), p=None)
        steps = np.sort(rng.uniform(1 / 64, 1 / 8, 7))
        ra = rng.uniform(1 / 64, 1 / 32, 8)
    rb = rng.uniform(1 / 32, 1 / 16, 8)
    pairs = [(float(a), float(b)) for a, b in zip(ra[:7], rb[:7])]
    return d, pairs, float(ra[7]), float(rb[7]), [float(v) for v in steps]


def _objective(cgo, kind, n, d, ctx):
    if kind == "quad":
        return cgo.QuadDiag(d["p"], ctx)
    return cgo.RosenbrockPaired(n, ctx) if kind == "rosen" else cgo.Booth(ctx)


def _ran(out, mode, npts=None):
    sym = out["symbol"]
    return sym.endswith("true>") and f", {mode}, " in sym and (npts is None or f", {mode}, {npts}, " in sym)


def _check_launches(cgo, ctx, kind, n, r):
    d, pairs, a_acc, beta, steps = _launch_data(kind, n, 23 + n % 97)
    o = _objective(cgo, kind, n, d, ctx)
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.DisableTrace(), max_iters=5)
    s = cgo.Solver(o, cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), _policy(cgo))
    bad = []
    try:
        x0, u0 = d["x"], d["u"]
        xr, ur = x0, u0
        for a_j, b_j in pairs[:r]:                     # (x_r, u_r): r plain accept + direction launches
            step = s.probe_launch("accept_dir", R_ACCEPT | R_DIR, a_j, b_j, [], xr, ur)
            assert _ran(step, R_ACCEPT | R_DIR), step["symbol"]
            xr, ur = step["x"], step["u"]
        assert np.all(np.isfinite(xr)) and np.all(np.isfinite(ur))
        lst = pairs[:r]
        tag0 = f"{kind} n={n} r={r}"
        M = s.probe_launch("materialize_xu", MODE_M, 0.0, 0.0, [], x0, u0, replay=lst)
        if not (M["sums"].size == 0 and same(M["x"], xr) and same(M["u"], ur) and M["symbol"].endswith(f", {MODE_M}, 1, true>")):
            bad.append(f"{tag0}: materialise did not write exactly (x_r, u_r), or a row came back [{M['symbol']}]")
        for k in (1, 3, 7):
            a = steps[:k]
            tag = f"{tag0} k={k}"
            ref = s.probe_launch("accept_dir_trial", ADT, a_acc, beta, a, xr, ur)
            assert _ran(ref, ADT, k) and np.all(np.isfinite(ref["sums"])), ref["symbol"]
            N = s.probe_launch("accept_trial_nostore", MODE_N, a_acc, beta, a, x0, u0, replay=lst)
            S = s.probe_launch("accept_dir_trial", MODE_S, a_acc, beta, a, x0, u0, replay=lst)
            if not _ran(N, MODE_N, k):
                bad.append(f"{tag}: N ran {N['symbol']}")
            if not _ran(S, MODE_S, k):
                bad.append(f"{tag}: S ran {S['symbol']}")
            if not same(N["sums"], ref["sums"]):
                bad.append(f"{tag}: launch N's row differs from the plain launch's on (x_r, u_r)")
            if not (same(N["x"], x0) and same(N["u"], u0)):
                bad.append(f"{tag}: launch N wrote x or u")
            if not (same(S["sums"], ref["sums"]) and same(S["x"], ref["x"]) and same(S["u"], ref["u"])):
                bad.append(f"{tag}: launch S's row, x or u differs from the plain launch's")
            tref = s.probe_launch("trial", R_TRIAL, 0.0, 0.0, a, xr, ur)
            T = s.probe_launch("trial", MODE_T, 0.0, 0.0, a, x0, u0, replay=lst)
            assert _ran(tref, R_TRIAL, k), tref["symbol"]
            if not _ran(T, MODE_T, k):
                bad.append(f"{tag}: T ran {T['symbol']}")
            if not same(T["sums"], tref["sums"]):
                bad.append(f"{tag}: launch T's row differs from the plain trial's on (x_r, u_r)")
            if not (same(T["x"], x0) and same(T["u"], u0)):
                bad.append(f"{tag}: launch T wrote x or u")
    finally:
        s.close(); o.close()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("r", REPLAYED, ids=lambda r: f"r{r}")
@pytest.mark.parametrize("n", SIZES, ids=lambda n: f"n{n}")
def test_quad_replay_launches_equal_plain_launches(cgo, ctx, n, r):
    _check_launches(cgo, ctx, "quad", n, r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", REPLAYED, ids=lambda r: f"r{r}")
@pytest.mark.parametrize("n", [n - 1 for n in SIZES], ids=lambda n: f"n{n}")
def test_rosenbrock_paired_replay_launches_equal_plain_launches(cgo, ctx, n, r):
    _check_launches(cgo, ctx, "rosen", n, r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", REPLAYED, ids=lambda r: f"r{r}")
def test_booth_replay_launches_equal_plain_launches(cgo, ctx, r):
    _check_launches(cgo, ctx, "booth", 2, r)


# ---- (2) whole solves ----------------------------------------------------------------------------------------------------
def _solve(cgo, make_obj, cfg, ls, x0, depth, ctx, chunk=0, between=None):
    """One solve through the Solver: replay depth `depth` forced by the setters, or (depth = 0) lazy direction off.
    between(solver, slice number) runs after every slice of `chunk` iterations that does not end the solve."""
    o = make_obj(ctx)
    s = cgo.Solver(o, cfg, ls, _policy(cgo))
    mid = []
    try:
        s.set_lazy_direction(depth > 0)
        if depth > 0:
            s.set_replay_depth(depth)
        s.enable_trial_log()
        s.set_x0(x0)
        s.start()
        s.profile(True)
        i = 0
        while not s.iterate(chunk if chunk > 0 else 1 << 40):
            if between is not None:
                mid.append(between(s, i))
            i += 1
        prof = s.profile_get()
        r = s.results()
        log = s.trial_log()
    finally:
        s.close(); o.close()
    return dict(r=r, log=log, prof=prof, mid=mid)


def _assert_equal_results(a, b, name):
    assert a.status == b.status and a.iters_ran == b.iters_ran, (name, a.status, b.status, a.iters_ran, b.iters_ran)
    assert same(np.array([a.objective]), np.array([b.objective])), name
    for f in ("objective", "grad_norm", "step_size"):
        assert same(getattr(a.trace, f), getattr(b.trace, f)), (name, f)
    assert np.array_equal(a.trace.objective_evals, b.trace.objective_evals), name
    assert same(a.minimizer, b.minimizer) and same(a.gradient, b.gradient), name
    assert a.total_launches == b.total_launches and a.total_fdf_evals == b.total_fdf_evals, name


def _assert_equal_solves(on, off, name):
    _assert_equal_results(on["r"], off["r"], name)
    assert len(on["log"]) == len(off["log"])
    for la, lb in zip(on["log"], off["log"]):
        assert same(la, lb), name
    for k in NEW_KINDS + ("accept_trial_lazy", "materialize_u"):
        assert k not in off["prof"], (name, k)


def _pair(cgo, ctx, make_obj, cfg, ls, x0, name, depth, chunk=0, between=None, expect_nostore=True):
    on = _solve(cgo, make_obj, cfg, ls, x0, depth, ctx, chunk, between)
    off = _solve(cgo, make_obj, cfg, ls, x0, 0, ctx, chunk, between)
    _assert_equal_solves(on, off, name)
    if expect_nostore:
        assert on["prof"].get("accept_trial_nostore", {}).get("launches", 0) >= 1, (name, on["prof"])
        assert "accept_trial_lazy" not in on["prof"] and "materialize_u" not in on["prof"], (name, on["prof"])
    return on, off


N_MID = 2 * GRID_BIG * 8 + 3


def _quad(cgo, n):
    D = quad_D(n)
    return lambda ctx: cgo.QuadDiag(D, ctx)


def _sw(cgo):
    return cgo.setupStrongWolfeBisection(1e-5, 0.1)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 3, 4, 8], ids=lambda d: f"d{d}")
def test_quad_pr_strong_wolfe_replay_equals_plain(cgo, ctx, depth):
    cfg = cgo.setupCGConfig(1e-12, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=18)
    on, _ = _pair(cgo, ctx, _quad(cgo, N_MID), cfg, _sw(cgo), np.ones(N_MID), f"quad-PR-d{depth}", depth)
    assert on["r"].iters_ran == 18
    assert on["prof"]["accept_dir_trial"]["launches"] >= 1      # at least one whole cycle: an S launch ran


@pytest.mark.gpu
@pytest.mark.parametrize("max_iters", [8, 9, 10, 11], ids=lambda m: f"it{m}")
def test_quad_depth4_ends_at_every_phase_of_the_cycle(cgo, ctx, max_iters):
    """results are fetched with 0, 1, 2 and 3 steps outstanding"""
    cfg = cgo.setupCGConfig(1e-12, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=max_iters)
    on, _ = _pair(cgo, ctx, _quad(cgo, N_MID), cfg, _sw(cgo), np.ones(N_MID), f"quad-PR-d4-{max_iters}", 4)
    assert on["r"].iters_ran == max_iters


@pytest.mark.gpu
@pytest.mark.parametrize("max_iters", [5, 9], ids=lambda m: f"it{m}")
def test_rosenbrock_paired_forced_on_replay_equals_plain(cgo, ctx, max_iters):
    n = 1000
    cfg = cgo.setupCGConfig(1e-5, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=max_iters)
    _pair(cgo, ctx, lambda c: cgo.RosenbrockPaired(n, c), cfg, _sw(cgo), np.tile([-1.2, 1.0], n // 2), f"rosen-PR-{max_iters}", 3)


@pytest.mark.gpu
def test_wolfe_bisection_reset_and_upg_path_replay_equals_plain(cgo, ctx):
    """WolfeBisection's bracket collapse (wolfe.jl:122-130): ‖u + g‖² reads x and u, and the reset now needs the current x too.
    Both are launched with steps outstanding only after a materialise pass (the reset follows the norm within one line search,
    so the pass before the norm serves both)."""
    c = reset_cases()[0]
    from _cases import _product_structs
    _, _, cfg, ls = _product_structs(c)
    on, _ = _pair(cgo, ctx, lambda cx: cgo.RosenbrockPaired(c.n, cx), cfg, ls, c.x0, c.name, 4)
    assert on["prof"].get("upg_norm", {}).get("launches", 0) >= 1 and on["prof"].get("reset_dir", {}).get("launches", 0) >= 1, on["prof"]
    assert on["prof"].get("materialize_xu", {}).get("launches", 0) >= 1, on["prof"]


@pytest.mark.gpu
def test_failing_status_returns_the_last_good_iterate_replay_equals_plain(cgo, ctx):
    n = 64
    x0 = np.ones(n)
    # plain PR + loose curvature condition: an ascent direction at iteration 2 (nocedal.jl:57-63)
    cfg = cgo.setupCGConfig(1e-5, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=50)
    on, _ = _pair(cgo, ctx, _quad(cgo, n), cfg, cgo.setupStrongWolfeBisection(1e-5, 0.8), x0, "st-nondescent", 4)
    assert on["r"].status == "non_descent_search_direction"
    cfg = cgo.setupCGConfig(1e-5, cgo.HagerZhang(), cgo.EnableTrace(), max_iters=50)
    on, _ = _pair(cgo, ctx, _quad(cgo, n), cfg, cgo.StrongWolfeBisection(1e-5, 0.8, 2.0, 1000, 2), x0, "st-zoom", 4, expect_nostore=False)
    assert on["r"].status == "zoom_max_iters_reached"


@pytest.mark.gpu
def test_single_iteration_slices_equal_one_call(cgo, ctx):
    cfg = cgo.setupCGConfig(1e-12, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=11)
    whole = _solve(cgo, _quad(cgo, N_MID), cfg, _sw(cgo), np.ones(N_MID), 4, ctx)
    sliced = _solve(cgo, _quad(cgo, N_MID), cfg, _sw(cgo), np.ones(N_MID), 4, ctx, chunk=1)
    plain = _solve(cgo, _quad(cgo, N_MID), cfg, _sw(cgo), np.ones(N_MID), 0, ctx, chunk=1)
    _assert_equal_solves(sliced, plain, "slices")
    _assert_equal_solves(whole, plain, "whole")
    assert sliced["prof"].get("accept_trial_nostore", {}).get("launches", 0) >= 1


@pytest.mark.gpu
def test_results_fetched_mid_cycle_then_the_solve_continues(cgo, ctx):
    """results(vectors=True) after 2, 4, 6, … iterations: the minimizer and the gradient of the CURRENT iterate, whatever is
    outstanding, and the solve goes on from it"""
    cfg = cgo.setupCGConfig(1e-12, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=13)
    fetch = lambda s, i: s.results(vectors=True)
    on, off = _pair(cgo, ctx, _quad(cgo, N_MID), cfg, _sw(cgo), np.ones(N_MID), "mid-results", 4, chunk=2, between=fetch)
    assert len(on["mid"]) == len(off["mid"]) >= 5
    for i, (a, b) in enumerate(zip(on["mid"], off["mid"])):
        _assert_equal_results(a, b, f"mid-results slice {i}")
    assert on["prof"].get("materialize_xu", {}).get("launches", 0) >= 1, on["prof"]


@pytest.mark.gpu
def test_replay_depth_changed_mid_solve(cgo, ctx):
    cfg = cgo.setupCGConfig(1e-12, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=17)
    depths = [2, 8, 1, 5, 3, 4, 1, 6]

    def change(s, i):
        s.set_replay_depth(depths[i % len(depths)])
    on = _solve(cgo, _quad(cgo, N_MID), cfg, _sw(cgo), np.ones(N_MID), 4, ctx, chunk=2, between=change)
    off = _solve(cgo, _quad(cgo, N_MID), cfg, _sw(cgo), np.ones(N_MID), 0, ctx, chunk=2)
    _assert_equal_solves(on, off, "depth-changes")
    assert on["prof"].get("accept_trial_nostore", {}).get("launches", 0) >= 1
    assert on["prof"].get("accept_trial_lazy", {}).get("launches", 0) >= 1      # the depth-1 slices alternate A / B


@pytest.mark.gpu
def test_rerun_chain_replay_equals_plain(cgo, monkeypatch):
    """cgo_minimize_rerun builds its solvers itself: the context's default policy and CGO_REPLAY_DEPTH reach them"""
    n = N_MID
    D = quad_D(n)
    ls = _sw(cgo)
    cfgs = [cgo.setupCGConfig(e, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=m) for e, m in ((1e-2, 5), (1e-4, 6), (1e-6, 7))]
    out = {}
    for lazy, depth in (("1", "3"), ("0", "3")):
        monkeypatch.setenv("CGO_LAZY_DIR", lazy)
        monkeypatch.setenv("CGO_REPLAY_DEPTH", depth)
        c = cgo.Context(0)
        c.set_default_policy(_policy(cgo))
        o = cgo.QuadDiag(D, c)
        try:
            if lazy == "1":   # what a solver built under this environment launches
                s = cgo.Solver(o, cfgs[0], ls, _policy(cgo))
                sym = s.kernel_symbol("accept_trial_nostore")
                s.close()
                assert sym == f"k_cg<ObjQuadDiag, {MODE_N}, 7, true>", sym
            out[lazy] = cgo.minimizeobjectivererun(o, np.ones(n), cfgs[0], ls, (cfgs[1], ls), (cfgs[2], ls))
        finally:
            o.close(); c.close()
    assert len(out["1"]) == len(out["0"]) >= 2
    for a, b in zip(out["1"], out["0"]):
        _assert_equal_results(a, b, "rerun")


@pytest.mark.gpu
def test_two_virtual_ranks_replay_equals_plain(cgo):
    """two contexts of one process as two ranks over the callback transport, each with its contiguous shard"""
    n, W = 2 * N_MID, 2
    D = quad_D(n)
    cfg = cgo.setupCGConfig(1e-12, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=10)
    ls = _sw(cgo)

    def run(depth):
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
                outs[rank] = _solve(cgo, lambda cx: cgo.QuadDiag(D, cx), cfg, ls, np.ones(n), depth, c)
                c.close()
            except Exception as e:  # pragma: no cover
                errs.append(e)
                bar.abort()
        ts = [threading.Thread(target=worker, args=(r,)) for r in range(W)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        assert not errs, errs
        return outs
    on, off = run(4), run(0)
    for r in range(W):
        _assert_equal_solves(on[r], off[r], f"rank {r}")
        assert on[r]["prof"].get("accept_trial_nostore", {}).get("launches", 0) >= 1


# ---- (3) profile ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_profile_names_what_ran(cgo, ctx, monkeypatch):
    n, iters, d = N_MID, 12, 4
    cfg = cgo.setupCGConfig(1e-300, cgo.PolakRibiere(), cgo.DisableTrace(), max_iters=iters)
    ls = _sw(cgo)
    monkeypatch.delenv("CGO_LAZY_DIR", raising=False)
    monkeypatch.delenv("CGO_REPLAY_DEPTH", raising=False)

    def run(depth, lazy=True):
        o = cgo.QuadDiag(quad_D(n), ctx)
        s = cgo.Solver(o, cfg, ls, _policy(cgo))
        try:
            s.set_lazy_direction(lazy)
            s.set_replay_depth(depth)
            s.set_x0(np.ones(n)); s.start()
            s.profile(True); s.profile_reset()
            while not s.iterate(iters):      # max_iters = iters: the solve ends there
                pass
            syms = {k: s.kernel_symbol(k) for k in ("accept_dir_trial",) + NEW_KINDS}
            return s.profile_get(), syms, s.results(vectors=False)
        finally:
            s.close(); o.close()
    prof, sym, r = run(d)
    off, sym_off, r_off = run(d, lazy=False)
    one, sym_one, r_one = run(1)
    assert r.iters_ran == r_off.iters_ran == r_one.iters_ran == iters
    N, S = prof["accept_trial_nostore"], prof["accept_dir_trial"]
    mat = prof.get("materialize_xu", {}).get("launches", 0)
    assert N["launches"] + S["launches"] == off["accept_dir_trial"]["launches"]
    assert S["launches"] >= iters // d - 1 - mat
    assert N["bytes_per_launch"] == 8.0 * n * 3 and S["bytes_per_launch"] == 8.0 * n * 5     # 8n(2 + p), 8n(2 + p + 2), p = 1
    if mat:
        assert prof["materialize_xu"]["bytes_per_launch"] == 8.0 * n * 5
    assert sym["accept_dir_trial"] == f"k_cg<ObjQuadDiag, {MODE_S}, 7, true>", sym
    assert sym["accept_trial_nostore"] == f"k_cg<ObjQuadDiag, {MODE_N}, 7, true>", sym
    assert sym["materialize_xu"] == f"k_cg<ObjQuadDiag, {MODE_M}, 1, true>", sym
    for p, sy in ((off, sym_off), (one, sym_one)):      # lazy off, and depth 1: the new kinds are absent
        assert not any(k in p for k in NEW_KINDS), p
        assert sy["accept_trial_nostore"] == "" and sy["materialize_xu"] == "", sy
    assert sym_off["accept_dir_trial"] == "k_cg<ObjQuadDiag, 7, 7, true>", sym_off
    assert one["accept_trial_lazy"]["launches"] >= 1 and off["accept_dir_trial"]["bytes_per_launch"] == 8.0 * n * 5


# ---- (4) CPU tier --------------------------------------------------------------------------------------------------------
def test_replay_rows_parse_and_are_disjoint_from_the_pinned_lists(monkeypatch):
    for name, bit in (("R_ULAG", 1024), ("R_NOWU", R_NOWU), ("R_REPLAY", R_REPLAY), ("R_NOWX", R_NOWX)):
        monkeypatch.setitem(I.BITS, name, bit)
    assert I.rows("CG_REPLAY") == [(MODE_N, 7), (MODE_S, 7), (MODE_T, 7), (MODE_M, 1)]
    replay = {m for m, _ in I.rows("CG_REPLAY")}
    assert not replay & {m for m, _ in I.rows("CG")} and not replay & {m for m, _ in I.rows("CG_LAG")}
    assert len(I.rows("CG")) == 12 and len(I.rows("CG_LAG")) == 4
    assert I.stray_uses() == []
    hdr = open(os.path.join(I.CSRC, "cgo_modes.hpp")).read()
    assert re.search(r"R_REPLAY = 4096\b", hdr) and re.search(r"R_NOWX = 8192\b", hdr)
    assert "CGO_CG_REPLAY_ROWS" not in open(os.path.join(I.CSRC, "cgo_rtc.hip")).read()      # built-in objectives only


def test_entry_points_are_declared_exported_and_bound(cgo):
    from cgo_amd import _lib
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cgo.h")).read(), flags=re.S)
    for name in ("cgo_solver_set_replay_depth", "cgo_solver_probe_set_replay", "cgo_solver_set_lazy_direction"):
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert hasattr(cgo.Solver, "set_replay_depth")
    kinds = [L.cgo_kernel_kind_name(k).decode() for k in range(L.cgo_num_kernel_kinds())]
    assert all(k in kinds for k in NEW_KINDS)
    assert kinds[-2:] == ["accept_trial_lazy", "materialize_u"] and kinds[:3] == ["init", "trial", "accept_dir_trial"]
    assert "CGO_REPLAY_DEPTH" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "cgo_solver_policy" in src and not re.search(r"replay", re.search(r"typedef struct cgo_solver_policy \{.*?\} cgo_solver_policy;", src, re.S).group(0))
