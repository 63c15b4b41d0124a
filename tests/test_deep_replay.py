"""Deep replay: replay depth up to 16.  A path launch k_cg_path<Obj, mode, NACT, true> and the deep trial launch
k_cg_trial_deep<Obj, NPTS, true> take the accepted steps beyond the seventh in a second kernel argument; every other reader of a
longer list gets the pair stored first, in passes of seven steps.

(0) CPU tier: the table, the run-time compiled text, the range of the depth, the entry points;
(1) per launch, path rows: N and S with lists of 0 … 15 pairs against a reference built from kernels that existed before —
    materialise passes of at most seven steps, then the same launch with what is left — every slot of the row, and S's x and u;
    with at most seven pairs also against the lean k_cg row, as tests/test_path_rows.py holds it;
(2) per launch, the deep trial launch against materialise-then-k_cg<Obj, R_REPLAY | R_TRIAL, NPTS, true>, and with at most seven
    pairs against that kernel directly: every slot;
(3) whole solves at depths 9, 12 and 16 against lazy direction off and against depth 8, byte for byte, and what
    cgo_solver_replay_stats counts.

Sizes: 2·4096·8 + 3 (one line per workgroup: only the one-group trip, an odd tail element) and 2·4096·520 + 1 (the two-group trip,
then the one-group trip, an odd tail).  All solvers use hbm_stream_bytes = 1.0 like tests/test_replay_state.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _instances as I
from _cases import quad_D
from test_lean_sums import LEAN_N, LEAN_S, MODE_N, MODE_S, RS_GTG, RS_PER_POINT, RS_UY, _policy, bits, same
from test_replay_state import MODE_M, MODE_T, _assert_equal_results, _launch_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_BIG = 4096
N_ONE, N_TWO = 2 * GRID_BIG * 8 + 3, 2 * GRID_BIG * 520 + 1
SIZES = [N_ONE, N_TWO]
LISTS = [0, 1, 7, 8, 11, 15]
NACTS = [1, 3, 7]
GU, UU, W7 = 49, 50, 56
KEPT = [0, 1, 2, 6]          # f, g⁺·u, g⁺·g⁺, y·g⁺: what Polak–Ribière's mask keeps of a point
RMAX = 7


@pytest.fixture(scope="module")
def ctx(cgo):
    c = cgo.Context(0)
    yield c
    c.close()


# ---- (0) CPU tier --------------------------------------------------------------------------------------------------------
def test_deep_trial_rows_parse_and_are_a_family_of_their_own():
    deep = I.rows("CG_DEEP_T")
    assert deep == [(1,), (3,), (5,), (7,)]                       # the point counts a trial launch of a 7-point solver takes
    for fam in ("CG", "CG_REPLAY", "CG_LEAN", "CG_PATH", "CG_LAG"):
        rows = I.rows(fam)
        assert rows and not set(rows) & set(deep), fam
    # the pinned lists are what they were
    assert I.rows("CG_PATH") == [(m, k) for m in (LEAN_N, LEAN_S) for k in (1, 2, 3, 4, 5, 7)]
    assert I.rows("CG_REPLAY") == [(MODE_N, 7), (MODE_S, 7), (MODE_T, 7), (MODE_M, 1)]
    assert I.rows("OBJ_CURV") == [("CGO_OBJ_QUAD_DIAG", "ObjQuadDiag")]
    assert I.stray_uses() == []
    # launched from the table's expander only, for the objectives of the path rows, and not in the run-time compiled module
    text = "\n".join(open(os.path.join(I.CSRC, f)).read() for f in sorted(os.listdir(I.CSRC)) if f.endswith(".hip")).replace("\\\n", " ")
    uses = [line.strip() for line in text.split("\n") if re.search(r"\bk_cg_trial_deep<", line.split("//")[0].replace('"k_cg_trial_deep<', ""))]
    assert uses and all(u.startswith("#define ROW(") for u in uses), uses
    be = open(os.path.join(I.CSRC, "cgo_backend_cg.hip")).read()
    assert "CGO_CG_DEEP_T_ROWS(ROW)" in be
    for name in ("cgo_rtc.hip", "cgo_rtc_batch.hip", "gen_rtc_sources.py"):
        t = open(os.path.join(I.CSRC, name)).read()
        assert "CG_DEEP_T" not in t and "k_cg_trial_deep" not in t and "RDeep" not in t, name


def test_runtime_compiled_text_is_unchanged(tmp_path):
    """RParams, RMAX and the replay loops of cg_pair are the run-time compiled modules' text: deep replay adds nothing to it"""
    out = tmp_path / "rtc.inc"
    subprocess.run([sys.executable, os.path.join(I.CSRC, "gen_rtc_sources.py"), str(out)], check=True, cwd=I.CSRC)
    text = out.read_text()
    for word in ("RDeep", "RDEEP", "RCAP", "rdeep_stage", "nrep2", "cgo_kernels_cg_path"):      # (include/cgo.h, part of the text, names the kernels)
        assert word not in text, word
    assert "__global__ __launch_bounds__(BLOCK) void k_cg(const RParams P)" in text and "void k_cg_trial_deep(" not in text and "void k_cg_path(" not in text
    cg = open(os.path.join(I.CSRC, "cgo_kernels_cg.hip.hpp")).read()
    assert "constexpr int RMAX = 7;" in cg and "double ra[RMAX], rb[RMAX];" in cg and "RDeep" not in cg
    assert cg.count("for (int j = 0; j < RMAX; ++j)") == 2
    for name in ("cgo_modes.hpp", "cgo_ctl.hpp"):
        assert "RDeep" not in open(os.path.join(I.CSRC, name)).read()
    path = open(os.path.join(I.CSRC, "cgo_kernels_cg_path.hip.hpp")).read()
    assert "constexpr int RDEEP = 8;" in path and "constexpr int RCAP = RMAX + RDEEP;" in path


def test_depth_range_in_the_sources():
    capi = open(os.path.join(I.CSRC, "cgo_capi.hip")).read()
    assert 'REQUIRE(d >= 1 && d <= 16, "replay depth: 1 … 16")' in capi
    assert re.search(r'getenv\("CGO_REPLAY_DEPTH"\)\) \{ const int v = atoi\(e\); if \(v >= 1 && v <= 16\)', capi)
    assert re.search(r"static const int kReplayDepth = (\d+);", capi) and 1 <= int(re.search(r"static const int kReplayDepth = (\d+);", capi).group(1)) <= 16
    hpp = open(os.path.join(I.CSRC, "cgo_hip_backend.hpp")).read()
    assert "replay_depth_ = d < 1 ? 1 : (d > 16 ? 16 : d)" in hpp and "rep_a_[15]" in hpp and "rep_b_[15]" in hpp
    be = open(os.path.join(I.CSRC, "cgo_backend_cg.hip")).read()
    assert "d < 1 || d > RCAP + 1" in be
    for doc, word in (("INTEGRATION.md", "CGO_REPLAY_DEPTH"), ("DESIGN.md", "CGO_REPLAY_DEPTH=1…16")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc
    assert '"1" … "16"' in open(os.path.join(os.path.dirname(I.CSRC), "julia", "ConjugateGradientOptimAMD.jl")).read()


def test_entry_points_are_declared_exported_and_bound(cgo):
    from cgo_amd import _lib
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cgo.h")).read(), flags=re.S)
    for name in ("cgo_solver_replay_stats", "cgo_solver_probe_set_deep_trial", "cgo_solver_set_replay_depth", "cgo_solver_probe_set_replay"):
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    for name in ("set_replay_depth", "replay_stats"):
        assert hasattr(cgo.Solver, name), name
    assert "1 … 16" in cgo.Solver.set_replay_depth.__doc__
    assert "cgo_solver_replay_stats" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ---- (1), (2) per launch -------------------------------------------------------------------------------------------------
def _fifteen_pairs(n):
    """x, u, D of tests/test_replay_state.py's recipe, fifteen (a*, β) pairs in its ranges, a_acc, β and seven rising steps"""
    d, pairs, a_acc, beta, steps = _launch_data("quad", n, 23 + n % 97)
    rng = np.random.default_rng(1000 + n % 97)
    more = [(float(a), float(b)) for a, b in zip(rng.uniform(1 / 32, 1 / 16, 8), rng.uniform(1 / 32, 1 / 16, 8))]
    return d, pairs + more, a_acc, beta, steps


def _solver(cgo, ctx, d):
    o = cgo.QuadDiag(d["p"], ctx)
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.DisableTrace(), max_iters=5)
    return o, cgo.Solver(o, cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), _policy(cgo))


def _materialised(s, x, u, lst, keep):
    """(x, u) after the first steps of `lst`, stored by materialise passes of at most seven steps — kernels that existed before deep
    replay — until at most `keep` steps are left; and those steps"""
    while len(lst) > keep:
        take = min(len(lst) - keep, RMAX) if keep else min(len(lst), RMAX)
        M = s.probe_launch("materialize_xu", MODE_M, 0.0, 0.0, [], x, u, replay=lst[:take])
        assert M["symbol"].endswith(f", {MODE_M}, 1, true>") and M["sums"].size == 0, M["symbol"]
        x, u, lst = M["x"], M["u"], lst[take:]
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(u))
    return x, u, lst


def _check_path_rows(cgo, ctx, n, r):
    d, pairs, a_acc, beta, steps = _fifteen_pairs(n)
    o, s = _solver(cgo, ctx, d)
    bad = []
    try:
        x0, u0, lst = d["x"], d["u"], pairs[:r]
        # r ≤ 7: everything stored, the launch starts from an empty list; r > 7: the first seven (fourteen) stored, the rest replayed
        xm, um, rest = _materialised(s, x0, u0, lst, 0 if r <= RMAX else (r - RMAX) % RMAX or RMAX)
        assert len(rest) <= RMAX and (r <= RMAX) == (not rest)
        lean = None
        if r <= RMAX:
            lean = {"N": s.probe_launch("accept_trial_nostore", LEAN_N, a_acc, beta, steps, x0, u0, replay=lst),
                    "S": s.probe_launch("accept_dir_trial", LEAN_S, a_acc, beta, steps, x0, u0, replay=lst)}
            assert lean["N"]["symbol"] == f"k_cg<ObjQuadDiag, {LEAN_N}, 7, true>" and lean["S"]["symbol"] == f"k_cg<ObjQuadDiag, {LEAN_S}, 7, true>"
        for nact in NACTS:
            a = steps[:nact]
            for name, kind, mode in (("N", "accept_trial_nostore", LEAN_N), ("S", "accept_dir_trial", LEAN_S)):
                tag = f"n={n} r={r} NACT={nact} path {name}"
                got = s.probe_launch(kind, mode, a_acc, beta, a, x0, u0, replay=lst, path_nact=nact)
                ref = s.probe_launch(kind, mode, a_acc, beta, a, xm, um, replay=rest, path_nact=nact)
                for out in (got, ref):
                    if out["symbol"] != f"k_cg_path<ObjQuadDiag, {mode}, {nact}, true>":
                        bad.append(f"{tag}: ran {out['symbol']}")
                if got["sums"].size != W7 or not np.all(np.isfinite(got["sums"])):
                    bad.append(f"{tag}: row of {got['sums'].size} slots, or not finite")
                    continue
                if not same(got["sums"], ref["sums"]):
                    diff = np.nonzero(bits(got["sums"]) != bits(ref["sums"]))[0].tolist()
                    bad.append(f"{tag}: slots {diff} differ from materialise-then-launch")
                if name == "N" and not (same(got["x"], x0) and same(got["u"], u0)):
                    bad.append(f"{tag}: launch N wrote x or u")
                if name == "S" and not (same(got["x"], ref["x"]) and same(got["u"], ref["u"])):
                    bad.append(f"{tag}: launch S's x or u differs from materialise-then-launch")
                if lean is not None:      # today's lean row on the launch's points (tests/test_path_rows.py)
                    pb, lb = bits(got["sums"]), bits(lean[name]["sums"])
                    for j in range(nact):
                        b = RS_PER_POINT * j
                        if any(pb[b + q] != lb[b + q] for q in KEPT) or pb[b + RS_GTG] != 0 or pb[b + RS_UY] != 0:
                            bad.append(f"{tag}: point {j} differs from the lean launch's kept slots, or a dropped slot is not +0.0")
                    if pb[GU] != lb[GU] or pb[UU] != lb[UU]:
                        bad.append(f"{tag}: direction sums differ from the lean launch's")
                    idle = np.r_[RS_PER_POINT * nact:GU, UU + 1:W7]
                    if np.any(pb[idle] != 0):
                        bad.append(f"{tag}: slots of inactive points or padding are not +0.0")
                    if name == "S" and not (same(got["x"], lean["S"]["x"]) and same(got["u"], lean["S"]["u"])):
                        bad.append(f"{tag}: launch S's x or u differs from the lean launch's")
    finally:
        s.close(); o.close()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("r", LISTS, ids=lambda r: f"r{r}")
@pytest.mark.parametrize("n", SIZES, ids=lambda n: f"n{n}")
def test_path_launches_with_deep_lists_equal_materialise_then_launch(cgo, ctx, n, r):
    _check_path_rows(cgo, ctx, n, r)


def _check_deep_trial(cgo, ctx, n, r):
    d, pairs, a_acc, beta, steps = _fifteen_pairs(n)
    o, s = _solver(cgo, ctx, d)
    bad = []
    try:
        x0, u0, lst = d["x"], d["u"], pairs[:r]
        xm, um, rest = _materialised(s, x0, u0, lst, 0 if r <= RMAX else (r - RMAX) % RMAX or RMAX)
        for k in (3, 7):
            a = steps[:k]
            tag = f"n={n} r={r} k={k}"
            ref = s.probe_launch("trial", MODE_T, 0.0, 0.0, a, xm, um, replay=rest)
            assert ref["symbol"] == f"k_cg<ObjQuadDiag, {MODE_T}, {k}, true>" and np.all(np.isfinite(ref["sums"])), ref["symbol"]
            T = s.probe_launch("trial", MODE_T, 0.0, 0.0, a, x0, u0, replay=lst, deep_trial=r <= RMAX)
            if T["symbol"] != f"k_cg_trial_deep<ObjQuadDiag, {k}, true>":
                bad.append(f"{tag}: ran {T['symbol']}")
            if not same(T["sums"], ref["sums"]):
                bad.append(f"{tag}: the deep trial launch's row differs from materialise-then-k_cg's")
            if not (same(T["x"], x0) and same(T["u"], u0)):
                bad.append(f"{tag}: the deep trial launch wrote x or u")
            if r <= RMAX:      # the same list through k_cg itself
                direct = s.probe_launch("trial", MODE_T, 0.0, 0.0, a, x0, u0, replay=lst)
                assert direct["symbol"] == f"k_cg<ObjQuadDiag, {MODE_T}, {k}, true>", direct["symbol"]
                if not same(T["sums"], direct["sums"]):
                    bad.append(f"{tag}: the deep trial launch's row differs from k_cg's on the same list")
    finally:
        s.close(); o.close()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("r", [0, 1, 7, 8, 11, 15], ids=lambda r: f"r{r}")
@pytest.mark.parametrize("n", SIZES, ids=lambda n: f"n{n}")
def test_deep_trial_launch_equals_materialise_then_trial(cgo, ctx, n, r):
    _check_deep_trial(cgo, ctx, n, r)


@pytest.mark.gpu
def test_refusals(cgo, ctx):
    """depths 0 and 17; a list of more than seven pairs for a launch that is neither a path row nor launch T; sixteen pairs"""
    d, pairs, a_acc, beta, steps = _fifteen_pairs(5)
    o, s = _solver(cgo, ctx, d)
    try:
        for depth in (0, 17, -1):
            with pytest.raises(cgo.CgoError):
                s.set_replay_depth(depth)
        s.set_replay_depth(16)
        for kind, mode, k in (("materialize_xu", MODE_M, 0), ("accept_trial_nostore", MODE_N, 3), ("accept_dir_trial", MODE_S, 3),
                              ("accept_trial_nostore", LEAN_N, 3), ("accept_dir_trial", LEAN_S, 3)):
            with pytest.raises(cgo.CgoError):
                s.probe_launch(kind, mode, a_acc, beta, steps[:k], d["x"], d["u"], replay=pairs[:8])
            ok = s.probe_launch(kind, mode, a_acc, beta, steps[:k], d["x"], d["u"], replay=pairs[:7])      # seven: today's launch
            assert ok["symbol"].startswith("k_cg<ObjQuadDiag, "), ok["symbol"]
        with pytest.raises(cgo.CgoError):
            s.probe_launch("accept_trial_nostore", LEAN_N, a_acc, beta, steps[:1], d["x"], d["u"], replay=pairs + [(0.1, 0.1)], path_nact=1)
        with pytest.raises(cgo.CgoError):      # the deep trial launch is launch T's twin only
            s.probe_launch("accept_dir_trial", MODE_S, a_acc, beta, steps[:3], d["x"], d["u"], replay=pairs[:2], deep_trial=True)
    finally:
        s.close(); o.close()
    dr, rp, a_acc, beta, steps = _launch_data("rosen", N_ONE - 1, 3)      # an objective without path rows has no deep trial launch
    o = cgo.RosenbrockPaired(N_ONE - 1, ctx)
    s = cgo.Solver(o, cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.DisableTrace(), max_iters=5), cgo.setupStrongWolfeBisection(1e-5, 0.1), _policy(cgo))
    try:
        with pytest.raises(cgo.CgoError):
            s.probe_launch("trial", MODE_T, 0.0, 0.0, steps[:3], dr["x"], dr["u"], replay=rp[:2], deep_trial=True)
    finally:
        s.close(); o.close()


# ---- (3) whole solves ----------------------------------------------------------------------------------------------------
ITERS = 40
N_SOLVE = N_ONE


def _solve(cgo, ctx, depth, max_iters=ITERS, skew=None, chunk=0, between=None, beta=None, n=N_SOLVE):
    """The quadratic with D = 1 + 999·U (seed 24) from x0 = 1 under strong Wolfe (1e-5, 0.1): depth 0 = lazy direction off, else the
    replay cycle of that depth with lean sums and the predicted path on.  between(solver, slice) runs after every slice of `chunk`
    iterations that does not end the solve."""
    o = cgo.QuadDiag(quad_D(n), ctx)
    cfg = cgo.setupCGConfig(1e-12, beta if beta is not None else cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=max_iters)
    s = cgo.Solver(o, cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), _policy(cgo))
    try:
        s.set_lazy_direction(depth > 0)
        if depth > 0:
            s.set_replay_depth(depth)
            s.set_lean_sums(True)
            s.set_path_prediction(True)
        if skew is not None:
            s.debug_set_path_skew(skew)
        s.enable_trial_log()
        s.set_x0(np.ones(n))
        s.start()
        s.profile(True)
        i = 0
        while not s.iterate(chunk if chunk > 0 else 1 << 40):
            if between is not None:
                between(s, i)
            i += 1
        prof = {k: v["launches"] for k, v in s.profile_get().items() if v["launches"]}
        r = s.results()
        out = dict(r=r, log=s.trial_log(), prof=prof, stats=s.replay_stats(), path=s.path_stats(), trial_symbol=s.kernel_symbol("trial"))
    finally:
        s.close(); o.close()
    return out


def _assert_same(a, b, name, launches=True):
    if launches:
        _assert_equal_results(a["r"], b["r"], name)      # minimizer, gradient, objective, traces, iteration count, total_launches
    else:
        ra, rb = a["r"], b["r"]
        assert ra.status == rb.status and ra.iters_ran == rb.iters_ran and ra.total_fdf_evals == rb.total_fdf_evals, name
        assert same(np.array([ra.objective]), np.array([rb.objective])) and same(ra.minimizer, rb.minimizer) and same(ra.gradient, rb.gradient), name
        for f in ("objective", "grad_norm", "step_size"):
            assert same(getattr(ra.trace, f), getattr(rb.trace, f)), (name, f)
        assert np.array_equal(ra.trace.objective_evals, rb.trace.objective_evals), name
    assert len(a["log"]) == len(b["log"]) >= 1
    for la, lb in zip(a["log"], b["log"]):
        assert same(la, lb), name


@pytest.fixture(scope="module")
def plain(cgo, ctx):
    """lazy direction off, and depth 8: computed once"""
    off, d8 = _solve(cgo, ctx, 0), _solve(cgo, ctx, 8)
    assert off["r"].iters_ran == ITERS and off["stats"] == dict(n=0, s=0, t=0, m=0, t_deep=0, m_deep=0, max_list=0)
    _assert_same(d8, off, "depth 8 against lazy direction off", launches=d8["path"]["misses"] == 0)
    assert d8["stats"]["max_list"] == 7 and d8["stats"]["t_deep"] == d8["stats"]["m_deep"] == 0
    return off, d8


def _cycle(accepting, depth):
    """(N, S) of `accepting` launches that nothing interrupts: every depth-th stores"""
    return accepting - accepting // depth, accepting // depth


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [9, 12, 16], ids=lambda d: f"d{d}")
def test_deep_solve_equals_plain_and_depth8(cgo, ctx, plain, depth):
    off, d8 = plain
    on = _solve(cgo, ctx, depth)
    print(f"d={depth}: {on['stats']} {on['path']} {on['prof']}")
    _assert_same(on, d8, f"d={depth} against depth 8")
    _assert_same(on, off, f"d={depth} against lazy direction off", launches=on["path"]["misses"] == 0)
    st, st8 = on["stats"], d8["stats"]
    accepting = st8["n"] + st8["s"]
    assert accepting >= ITERS - 1 and st["n"] + st["s"] == accepting
    assert (st["n"], st["s"]) == _cycle(accepting, depth) and (st8["n"], st8["s"]) == _cycle(accepting, 8)
    assert st["max_list"] == min(accepting - 1, depth - 1) > 7
    assert on["prof"]["accept_trial_nostore"] == st["n"] and on["prof"]["accept_dir_trial"] == st["s"]
    left = accepting % depth                                  # stored for the results, in passes of seven steps
    assert st["m"] == (left + 6) // 7 and st["m_deep"] == max(0, (left - 1) // 7) and st["t_deep"] <= st["t"], st


@pytest.mark.gpu
def test_a_trial_launch_meets_more_than_seven_steps(cgo, ctx, plain):
    """A skewed curvature model mispredicts line searches all through the solve (tests/test_path_rows.py): each miss costs one
    trial-only launch, met with whatever the cycle has outstanding — at depth 16 more than seven steps in half of its phases.
    The numbers are those of the same solve at depth 8 and of the plain solve."""
    off, _ = plain
    on, d8 = _solve(cgo, ctx, 16, skew=0.6), _solve(cgo, ctx, 8, skew=0.6)
    print(f"skewed d=16: {on['stats']} {on['path']}; d=8: {d8['stats']} {d8['path']}")
    _assert_same(on, d8, "skewed d=16 against skewed d=8")
    _assert_same(on, off, "skewed d=16 against lazy direction off", launches=False)
    assert on["path"]["misses"] == d8["path"]["misses"] > 0
    assert on["r"].total_launches == off["r"].total_launches + on["path"]["misses"]
    st = on["stats"]
    assert 1 <= st["t_deep"] <= st["t"], st
    assert d8["stats"]["t_deep"] == 0 and d8["stats"]["max_list"] == 7 and st["max_list"] == 15


@pytest.mark.gpu
@pytest.mark.parametrize("max_iters", [9, 10, 16, 17, 18, 26, 33], ids=lambda m: f"it{m}")
def test_depth16_ends_at_phases_of_the_cycle(cgo, ctx, max_iters):
    """results are fetched with 8, 9, 15, 0, 1, 9 and 0 steps outstanding (one accepting launch per iteration after the first)"""
    on, off = _solve(cgo, ctx, 16, max_iters=max_iters), _solve(cgo, ctx, 0, max_iters=max_iters)
    assert on["r"].iters_ran == max_iters
    _assert_same(on, off, f"d=16 it={max_iters}", launches=on["path"]["misses"] == 0)
    st = on["stats"]
    assert st["n"] + st["s"] == max_iters - 1, st
    left = (st["n"] + st["s"]) % 16
    assert st["n"] - 15 * st["s"] == left and st["m"] == (left + 6) // 7 and st["m_deep"] == max(0, (left - 1) // 7), st      # passes that met 15 and 8 steps: both deep


@pytest.mark.gpu
def test_depth_changed_mid_solve_through_deep_depths(cgo, ctx):
    """slices of eleven iterations at depths 16, 3, 12, 1, 9 and 16 again: the slices at 16 and 12 end with ten steps outstanding"""
    depths = [3, 12, 1, 9, 16]
    seen = []

    def change(s, i):
        seen.append(s.replay_stats())
        s.set_replay_depth(depths[i % len(depths)])
    on, off = _solve(cgo, ctx, 16, max_iters=60, chunk=11, between=change), _solve(cgo, ctx, 0, max_iters=60, chunk=11)
    print(f"depth changes: {on['stats']} {on['prof']}")
    assert on["r"].iters_ran == 60
    _assert_same(on, off, "depth changes", launches=on["path"]["misses"] == 0)
    assert len(seen) == 5 and seen[0]["max_list"] > 7 and seen[0]["m"] == 0          # the first slice ran depth 16
    assert on["stats"]["m_deep"] >= 1 and on["stats"]["m"] >= on["stats"]["m_deep"] + 1, on["stats"]
    assert on["prof"].get("materialize_xu", 0) == on["stats"]["m"]
    assert on["prof"].get("accept_trial_lazy", 0) >= 1          # the depth-1 slice alternates A / B


@pytest.mark.gpu
def test_prediction_switched_off_with_twelve_steps_outstanding(cgo, ctx, plain):
    """launch S then runs its lean row, which replays seven steps at most: the pair is stored in two passes first"""
    off, _ = plain
    at = {}

    def switch(s, i):
        st = s.replay_stats()
        if not at and st["n"] - 15 * st["s"] == 12:
            at.update(st)
            assert s.kernel_symbol("trial") == "k_cg_trial_deep<ObjQuadDiag, 3, true>"      # what a trial launch would run now
            s.set_path_prediction(False)
    on = _solve(cgo, ctx, 16, chunk=1, between=switch)
    assert at and at["m"] == 0, at
    _assert_same(on, off, "prediction off mid-cycle", launches=on["path"]["misses"] == 0)
    st = on["stats"]
    assert st["m"] >= 2 and st["m_deep"] == 1 and on["prof"]["materialize_xu"] == st["m"], st
    assert on["trial_symbol"] == "k_cg<ObjQuadDiag, 4, 3, true>"
    assert st["max_list"] == 11          # the twelfth launch N replayed eleven steps; from the switch on the cycle is depth 8's


@pytest.mark.gpu
def test_dai_yuan_at_depth16_runs_depth8(cgo, ctx):
    """no lean rows for this flavour, so no path rows: the request runs as depth 8, silently"""
    runs = {d: _solve(cgo, ctx, d, beta=cgo.DaiYuan()) for d in (16, 8, 0)}
    for d in (16, 8):
        assert sum(runs[d]["path"]["by_nact"].values()) == 0
        _assert_same(runs[d], runs[0], f"Dai–Yuan d={d}")
    assert runs[16]["prof"] == runs[8]["prof"] and runs[16]["stats"] == runs[8]["stats"]
    assert runs[16]["stats"]["max_list"] == 7 and runs[16]["stats"]["s"] >= 1 and runs[16]["stats"]["t_deep"] == 0
