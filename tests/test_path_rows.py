"""Predicted path: launches N and S of the replay cycle as path launches k_cg_path<Obj, mode, NACT, true> — the 7-point
lean row with only the first NACT trial points evaluated, those the line search is predicted to ask for, and Σ g⁺·(H g⁺) of each of
them in the slot of Σ y·y.

(1) per launch: path N and S against the lean 7-point N and S given the same steps in the first NACT places — every kept slot of an
    active point, g·u and u·u the same bits, every slot of an inactive point +0.0, x and u as the lean launch leaves them; the
    curvature slots against the correctly rounded exact sum, at the bound of tests/test_kernel_sums.py;
(2) whole solves, prediction on against off in one process: every number a solve returns, bit for bit;
(3) the same with a skewed model: wrong predictions change launches, not numbers;
(4) defaults and refusals.

All solvers use hbm_stream_bytes = 1.0 like tests/test_lean_sums.py, whose policy, sizes and input recipe these are."""
import math

import numpy as np
import pytest

from _cases import quad_D
from test_kernel_sums import summation_depth, two_prod
from test_lean_sums import (LEAN_N, LEAN_S, MODE_N, MODE_S, N_MID, REPLAYED, RS_GTG, RS_PER_POINT, RS_UY, RS_YY, SIZES, _policy,
                            bits, same)
from test_replay_state import _launch_data, _objective

N_BIG = SIZES[2]
NACTS = [1, 2, 3, 5, 7]
GU, UU, W7 = 49, 50, 56
KEPT = [0, 1, 2, 6]          # f, g⁺·u, g⁺·g⁺, y·g⁺: what Polak–Ribière's mask keeps of a point


@pytest.fixture(scope="module")
def ctx(cgo):
    c = cgo.Context(0)
    yield c
    c.close()


# ---- (1) per launch ------------------------------------------------------------------------------------------------------
def _curvature_terms(d, lst, a_acc, beta, steps):
    """g⁺ and D·g⁺ of every trial point, element-wise in the kernels' unfused order: replay, accept, direction, trial"""
    x, u, D = d["x"].copy(), d["u"].copy(), d["p"]
    for ra, rb in lst:
        x = x + ra * u
        u = -(D * x) + rb * u
    x = x + a_acc * u
    u = -(D * x) + beta * u
    out = []
    for a in steps:
        gt = D * (x + a * u)
        out.append((gt, D * gt))
    return out


def _check_path_launches(cgo, ctx, n, r):
    d, pairs, a_acc, beta, steps = _launch_data("quad", n, 23 + n % 97)
    o = _objective(cgo, "quad", n, d, ctx)
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.DisableTrace(), max_iters=5)
    s = cgo.Solver(o, cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), _policy(cgo))
    bad = []
    depth = summation_depth(n, W7, True)
    gam = depth * 2.0 ** -53 / (1 - depth * 2.0 ** -53)
    try:
        x0, u0, lst = d["x"], d["u"], pairs[:r]
        NL = s.probe_launch("accept_trial_nostore", LEAN_N, a_acc, beta, steps, x0, u0, replay=lst)
        SL = s.probe_launch("accept_dir_trial", LEAN_S, a_acc, beta, steps, x0, u0, replay=lst)
        assert NL["symbol"] == f"k_cg<ObjQuadDiag, {LEAN_N}, 7, true>" and SL["symbol"] == f"k_cg<ObjQuadDiag, {LEAN_S}, 7, true>"
        assert NL["sums"].size == SL["sums"].size == W7 and np.all(np.isfinite(NL["sums"]))
        curv = _curvature_terms(d, lst, a_acc, beta, steps)
        for nact in NACTS:
            a = steps[:nact]
            NP = s.probe_launch("accept_trial_nostore", LEAN_N, a_acc, beta, a, x0, u0, replay=lst, path_nact=nact)
            SP = s.probe_launch("accept_dir_trial", LEAN_S, a_acc, beta, a, x0, u0, replay=lst, path_nact=nact)
            for name, path, lean, mode in (("N", NP, NL, LEAN_N), ("S", SP, SL, LEAN_S)):
                tag = f"n={n} r={r} NACT={nact} path {name}"
                if path["symbol"] != f"k_cg_path<ObjQuadDiag, {mode}, {nact}, true>":
                    bad.append(f"{tag}: ran {path['symbol']}")
                if path["sums"].size != W7:
                    bad.append(f"{tag}: row of {path['sums'].size} slots")
                    continue
                pb, lb = bits(path["sums"]), bits(lean["sums"])
                for j in range(nact):
                    b = RS_PER_POINT * j
                    for q in KEPT:
                        if pb[b + q] != lb[b + q]:
                            bad.append(f"{tag}: point {j} slot {q} {path['sums'][b + q]!r} differs from the lean launch's {lean['sums'][b + q]!r}")
                    for q in (RS_GTG, RS_UY):
                        if pb[b + q] != 0:
                            bad.append(f"{tag}: point {j} dropped slot {q} is not +0.0")
                    gt, hg = curv[j]
                    pp, ee = two_prod(gt, hg)
                    exact, absum, tmin = math.fsum(np.concatenate([pp, ee])), float(np.sum(np.abs(pp))), float(np.min(np.abs(pp)))
                    bound = gam * absum * (1 + 1e-12)
                    assert tmin > bound, f"test data: {tag}: smallest curvature term {tmin:.3e} within the bound {bound:.3e}"
                    v = path["sums"][b + RS_YY]
                    if not abs(v - exact) <= bound:
                        bad.append(f"{tag}: point {j} curvature {v!r} vs {exact!r} (bound {bound:.3e})")
                for slot in (GU, UU):
                    if pb[slot] != lb[slot]:
                        bad.append(f"{tag}: direction slot {slot} differs from the lean launch's")
                idle = np.r_[RS_PER_POINT * nact:GU, UU + 1:W7]
                nz = idle[pb[idle] != 0]
                if nz.size:
                    bad.append(f"{tag}: slots {nz.tolist()} of inactive points or padding are not +0.0")
                if not np.all(lb[RS_PER_POINT * nact:GU][np.isin(np.arange(RS_PER_POINT * nact, GU) % RS_PER_POINT, KEPT)] != 0):
                    bad.append(f"{tag}: the lean launch left an inactive point's kept slot +0.0 itself: the inputs do not tell the rows apart")
            if not (same(SP["x"], SL["x"]) and same(SP["u"], SL["u"])):
                bad.append(f"n={n} r={r} NACT={nact}: path S's x or u differs from lean S's")
            if not (same(NP["x"], x0) and same(NP["u"], u0)):
                bad.append(f"n={n} r={r} NACT={nact}: path N wrote x or u")
    finally:
        s.close(); o.close()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("r", REPLAYED, ids=lambda r: f"r{r}")
@pytest.mark.parametrize("n", SIZES, ids=lambda n: f"n{n}")
def test_path_launches_equal_lean_launches_on_their_points(cgo, ctx, n, r):
    _check_path_launches(cgo, ctx, n, r)


@pytest.mark.gpu
def test_probe_rejects_path_rows_it_has_none_for(cgo, ctx):
    """six active points, more steps than the row evaluates, a full row, the trial-only launch, an objective without the trait"""
    d, pairs, a_acc, beta, steps = _launch_data("quad", 5, 1)
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.DisableTrace(), max_iters=5)
    ls = cgo.setupStrongWolfeBisection(1e-5, 0.1)
    o = cgo.QuadDiag(d["p"], ctx)
    s = cgo.Solver(o, cfg, ls, _policy(cgo))
    try:
        for kind, mode, k, nact in (("accept_trial_nostore", LEAN_N, 3, 6), ("accept_dir_trial", LEAN_S, 4, 3),
                                    ("accept_trial_nostore", MODE_N, 2, 2), ("accept_dir_trial", MODE_S, 2, 2),
                                    ("trial", 4096 | 4, 2, 2)):
            with pytest.raises(cgo.CgoError):
                s.probe_launch(kind, mode, a_acc, beta, steps[:k], d["x"], d["u"], replay=pairs[:2], path_nact=nact)
        ok = s.probe_launch("accept_trial_nostore", LEAN_N, a_acc, beta, steps[:3], d["x"], d["u"], replay=pairs[:2])   # the request was for one launch
        assert ok["symbol"] == f"k_cg<ObjQuadDiag, {LEAN_N}, 3, true>"
    finally:
        s.close(); o.close()
    n = N_MID - 1
    dr, pairs, a_acc, beta, steps = _launch_data("rosen", n, 3)
    o = cgo.RosenbrockPaired(n, ctx)
    s = cgo.Solver(o, cfg, ls, _policy(cgo))
    try:
        with pytest.raises(cgo.CgoError):
            s.probe_launch("accept_trial_nostore", LEAN_N, a_acc, beta, steps[:2], dr["x"], dr["u"], replay=pairs[:2], path_nact=2)
    finally:
        s.close(); o.close()


# ---- (2) whole solves ----------------------------------------------------------------------------------------------------
ITERS = 40


def _solve(cgo, ctx, n, depth, predict, skew=None, chunk=0, fetch=False, ls=None, make_obj=None, x0=None):
    """One solve at replay depth `depth` with lean sums forced on; predict: True / False through set_path_prediction, None:
    whatever the library decides.  chunk > 0: slices of that many iterations, results fetched between them with `fetch`."""
    o = make_obj(ctx) if make_obj else cgo.QuadDiag(quad_D(n), ctx)
    cfg = cgo.setupCGConfig(1e-12, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=ITERS)
    s = cgo.Solver(o, cfg, ls if ls is not None else cgo.setupStrongWolfeBisection(1e-5, 0.1), _policy(cgo))
    mid = []
    try:
        s.set_lazy_direction(True)
        s.set_replay_depth(depth)
        s.set_lean_sums(True)
        if predict is not None:
            s.set_path_prediction(predict)
        if skew is not None:
            s.debug_set_path_skew(skew)
        syms0 = {k: s.kernel_symbol(k) for k in ("accept_trial_nostore", "accept_dir_trial")}
        s.enable_trial_log()
        s.set_x0(np.ones(n) if x0 is None else x0)
        s.start()
        while not s.iterate(chunk if chunk > 0 else 1 << 40):
            if fetch:
                mid.append(s.results(vectors=True))
        syms1 = {k: s.kernel_symbol(k) for k in ("accept_trial_nostore", "accept_dir_trial")}
        r = s.results()
        log = s.trial_log()
        stats = s.path_stats()
    finally:
        s.close(); o.close()
    return dict(r=r, log=log, mid=mid, syms0=syms0, syms1=syms1, stats=stats)


def _assert_same_numbers(a, b, name):
    assert a.status == b.status and a.iters_ran == b.iters_ran, (name, a.status, b.status, a.iters_ran, b.iters_ran)
    assert same(np.array([a.objective]), np.array([b.objective])), name
    for f in ("objective", "grad_norm", "step_size"):
        assert same(getattr(a.trace, f), getattr(b.trace, f)), (name, f)
    assert np.array_equal(a.trace.objective_evals, b.trace.objective_evals), name
    assert same(a.minimizer, b.minimizer) and same(a.gradient, b.gradient), name
    assert a.total_fdf_evals == b.total_fdf_evals, name


def _assert_same_solves(on, off, name, mids=True):
    _assert_same_numbers(on["r"], off["r"], name)
    assert len(on["log"]) == len(off["log"]) >= 1
    for la, lb in zip(on["log"], off["log"]):
        assert same(la, lb), name
    if not mids:
        return
    assert len(on["mid"]) == len(off["mid"])
    for i, (a, b) in enumerate(zip(on["mid"], off["mid"])):
        _assert_same_numbers(a, b, f"{name} slice {i}")


@pytest.fixture(scope="module")
def prediction_off(cgo, ctx):
    """the solves with prediction off that the tests below compare against, computed once each"""
    memo = {}

    def get(n, depth, chunk=0):
        key = (n, depth, chunk)
        if key not in memo:
            memo[key] = off = _solve(cgo, ctx, n, depth, False, chunk=chunk, fetch=chunk > 0)
            assert off["syms0"] == off["syms1"] == {"accept_trial_nostore": f"k_cg<ObjQuadDiag, {LEAN_N}, 7, true>",
                                                    "accept_dir_trial": f"k_cg<ObjQuadDiag, {LEAN_S}, 7, true>"}
            assert off["stats"] == dict(by_nact={j: 0 for j in (1, 2, 3, 4, 5, 7)}, predicted=0, tree=0, misses=0)
            assert off["r"].iters_ran == ITERS
        return memo[key]
    return get


def _assert_predicted(on, off, name, max_miss=0.05):
    st = on["stats"]
    searches = on["r"].iters_ran
    print(f"{name}: {st}, launches {on['r'].total_launches} against {off['r'].total_launches}")
    assert st["predicted"] > 0 and st["predicted"] + st["tree"] == sum(st["by_nact"].values()), st
    assert st["by_nact"][7] >= st["tree"], st
    assert st["misses"] <= max_miss * searches, (name, st)
    # every launch the solve asked for with prediction off, plus one trial launch of the tree per miss, and nothing else
    assert on["r"].total_launches == off["r"].total_launches + st["misses"], (name, on["r"].total_launches, off["r"].total_launches, st)
    assert on["syms1"]["accept_trial_nostore"].startswith(f"k_cg_path<ObjQuadDiag, {LEAN_N}, "), on["syms1"]
    assert on["syms1"]["accept_dir_trial"].startswith(f"k_cg_path<ObjQuadDiag, {LEAN_S}, "), on["syms1"]


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 6], ids=lambda d: f"d{d}")
@pytest.mark.parametrize("n", [N_MID, N_BIG], ids=lambda n: f"n{n}")
def test_solve_with_prediction_equals_solve_without(cgo, ctx, prediction_off, n, depth):
    on, off = _solve(cgo, ctx, n, depth, True), prediction_off(n, depth)
    _assert_same_solves(on, off, f"n={n} d={depth}")
    _assert_predicted(on, off, f"n={n} d={depth}")
    assert on["r"].total_launches <= off["r"].total_launches, (on["r"].total_launches, off["r"].total_launches)
    assert on["syms0"] == {"accept_trial_nostore": f"k_cg_path<ObjQuadDiag, {LEAN_N}, 7, true>", "accept_dir_trial": f"k_cg_path<ObjQuadDiag, {LEAN_S}, 7, true>"}


@pytest.mark.gpu
def test_wolfe_bisection_with_prediction_equals_solve_without(cgo, ctx):
    """D ∈ [1, 100] and c2 = 0.9: on the spectrum of the other solves the reference ends a Polak–Ribière solve under the weak Wolfe
    conditions after one iteration, in a direction that is no descent direction (tests/test_path_predict.py)"""
    ls = cgo.WolfeBisection(cgo.Wolfe(1e-4, 0.9), 100, 1e12, 50)
    make = lambda c: cgo.QuadDiag(quad_D(N_MID, 1.0, 100.0), c)
    on, off = _solve(cgo, ctx, N_MID, 6, True, ls=ls, make_obj=make), _solve(cgo, ctx, N_MID, 6, False, ls=ls, make_obj=make)
    assert off["r"].iters_ran == ITERS
    _assert_same_solves(on, off, "WolfeBisection")
    _assert_predicted(on, off, "WolfeBisection")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N_MID, N_BIG], ids=lambda n: f"n{n}")
def test_sliced_solve_with_results_between_slices(cgo, ctx, prediction_off, n):
    """slices of 3 iterations, results fetched after each: materialise passes ride in between the path launches"""
    on, off = _solve(cgo, ctx, n, 6, True, chunk=3, fetch=True), prediction_off(n, 6, 3)
    assert len(on["mid"]) >= ITERS // 3 - 1
    _assert_same_solves(on, off, f"sliced n={n}")
    _assert_same_solves(on, prediction_off(n, 6), f"sliced n={n} against one call", mids=False)
    _assert_predicted(on, off, f"sliced n={n}")


@pytest.mark.gpu
def test_rerun_chain_with_prediction_equals_chain_without(cgo, monkeypatch):
    """cgo_minimize_rerun builds its solvers itself: CGO_PATH_PREDICT reaches them"""
    n = N_MID
    D = quad_D(n)
    ls = cgo.setupStrongWolfeBisection(1e-5, 0.1)
    cfgs = [cgo.setupCGConfig(e, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=m) for e, m in ((1e-2, 12), (1e-4, 14), (1e-6, 14))]
    monkeypatch.setenv("CGO_LAZY_DIR", "1")
    monkeypatch.setenv("CGO_REPLAY_DEPTH", "6")
    monkeypatch.setenv("CGO_LEAN_SUMS", "1")
    out = {}
    for predict in ("1", "0"):
        monkeypatch.setenv("CGO_PATH_PREDICT", predict)
        c = cgo.Context(0)
        c.set_default_policy(_policy(cgo))
        o = cgo.QuadDiag(D, c)
        try:
            s = cgo.Solver(o, cfgs[0], ls, _policy(cgo))      # what a solver built under this environment launches
            sym = s.kernel_symbol("accept_trial_nostore")
            s.close()
            assert sym == (f"k_cg_path<ObjQuadDiag, {LEAN_N}, 7, true>" if predict == "1" else f"k_cg<ObjQuadDiag, {LEAN_N}, 7, true>"), sym
            out[predict] = cgo.minimizeobjectivererun(o, np.ones(n), cfgs[0], ls, (cfgs[1], ls), (cfgs[2], ls))
        finally:
            o.close(); c.close()
    assert len(out["1"]) == len(out["0"]) >= 2
    for a, b in zip(out["1"], out["0"]):
        _assert_same_numbers(a, b, "rerun")
        assert a.total_launches == b.total_launches


# ---- (3) wrong predictions -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("skew", [1.5, 0.6], ids=lambda v: f"skew{v}")
@pytest.mark.parametrize("depth", [2, 6], ids=lambda d: f"d{d}")
@pytest.mark.parametrize("n", [N_MID, N_BIG], ids=lambda n: f"n{n}")
def test_skewed_model_changes_launches_not_numbers(cgo, ctx, prediction_off, n, depth, skew):
    on, off = _solve(cgo, ctx, n, depth, True, skew=skew), prediction_off(n, depth)
    _assert_same_solves(on, off, f"skew {skew} n={n} d={depth}")
    _assert_predicted(on, off, f"skew {skew} n={n} d={depth}", max_miss=1.0)
    assert on["stats"]["misses"] > 0, on["stats"]


# ---- (4) defaults and refusals -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_forced_lean_alone_switches_nothing_on(cgo, ctx, prediction_off, monkeypatch):
    monkeypatch.delenv("CGO_PATH_PREDICT", raising=False)
    dflt = _solve(cgo, ctx, N_MID, 6, None)
    off = prediction_off(N_MID, 6)
    assert dflt["syms0"] == dflt["syms1"] == off["syms0"]
    assert dflt["stats"] == off["stats"]
    _assert_same_solves(dflt, off, "default")
    assert dflt["r"].total_launches == off["r"].total_launches


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rosen", "booth"])
def test_objectives_without_the_trait_keep_their_rows(cgo, ctx, kind):
    n = N_MID - 1 if kind == "rosen" else 2
    d, _, _, _, _ = _launch_data(kind, n, 5)
    make = lambda c: _objective(cgo, kind, n, d, c)
    runs = [_solve(cgo, ctx, n, 6, p, make_obj=make, x0=d["x"]) for p in (True, False)]
    name, pts = ("ObjRosenPaired", 3) if kind == "rosen" else ("ObjBooth", 7)      # (the library's point count for the objective)
    for run in runs:
        assert run["syms0"] == run["syms1"] == {"accept_trial_nostore": f"k_cg<{name}, {LEAN_N}, {pts}, true>",
                                                "accept_dir_trial": f"k_cg<{name}, {LEAN_S}, {pts}, true>"}
        assert run["stats"]["predicted"] == run["stats"]["tree"] == 0 and sum(run["stats"]["by_nact"].values()) == 0
    _assert_same_numbers(runs[0]["r"], runs[1]["r"], kind)
    assert runs[0]["r"].total_launches == runs[1]["r"].total_launches


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["HagerZhang", "Backtracking", "YuanWeiLu"])
def test_configurations_outside_the_model_keep_their_rows(cgo, ctx, what):
    n = N_MID
    o = cgo.QuadDiag(quad_D(n), ctx)
    beta = cgo.HagerZhang() if what == "HagerZhang" else cgo.PolakRibiere()
    ls = {"HagerZhang": lambda: cgo.setupStrongWolfeBisection(1e-5, 0.1), "Backtracking": lambda: cgo.Backtracking(cgo.Armijo(1e-4), 0.5, 100, 50),
          "YuanWeiLu": lambda: cgo.WolfeBisection(cgo.YuanWeiLuWolfe(1e-4, 0.5, 1e-5), 100, 1e12, 50)}[what]()
    s = cgo.Solver(o, cgo.setupCGConfig(1e-12, beta, cgo.EnableTrace(), max_iters=8), ls, _policy(cgo))
    try:
        s.set_lazy_direction(True); s.set_replay_depth(6); s.set_lean_sums(True)
        before = s.kernel_symbol("accept_trial_nostore")
        s.set_path_prediction(True)
        assert s.kernel_symbol("accept_trial_nostore") == before and before.startswith("k_cg<ObjQuadDiag, ")
        s.set_x0(np.ones(n)); s.start()
        while not s.iterate(1 << 40):
            pass
        assert sum(s.path_stats()["by_nact"].values()) == 0
    finally:
        s.close(); o.close()
