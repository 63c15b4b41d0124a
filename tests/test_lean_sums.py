"""Lean sums: launches N and S of the replay cycle in instantiations that do not form the trial sums the solver's
β flavour never reads (beta_unread_sums, cgo_ctl.hpp) — under Polak–Ribière Σ g⁺·g, Σ y·y and Σ u·y of every trial point.

(1) per launch, bit for bit: lean N and lean S against full N and full S on the same inputs (tests/test_replay_state.py pins the
    full ones to the plain launch): every kept slot the same bits, every dropped slot +0.0, x and u as the full launch leaves them;
(2) whole solves, lean on against lean off in one process: every number a solve returns, bit for bit;
(3) the profile and the reported symbols tell the truth about what ran;
(4) CPU tier: the row list, the mode bits, the entry point;
(5) CPU tier: the mask — β computed from sums whose masked slots are 0.0 or NaN is β computed from the full sums, every flavour.

All GPU solvers use hbm_stream_bytes = 1.0 like tests/test_replay_state.py, whose sizes and input recipe these are."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import _instances as I
from _cases import quad_D
from test_replay_state import _launch_data, _objective

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_ACCEPT, R_DIR, R_TRIAL, R_NOWU, R_REPLAY, R_NOWX = 1, 2, 4, 2048, 4096, 8192
R_NOGTG, R_NOYY, R_NOUY, R_NOYGT = 16384, 32768, 65536, 131072
ADT = R_ACCEPT | R_DIR | R_TRIAL
MODE_N, MODE_S = R_REPLAY | ADT | R_NOWU | R_NOWX, R_REPLAY | ADT
PR_MASK = R_NOGTG | R_NOYY | R_NOUY
LEAN_N, LEAN_S = MODE_N | PR_MASK, MODE_S | PR_MASK
RS_GTG, RS_YY, RS_UY, RS_PER_POINT = 3, 4, 5, 7
GRID_BIG = 4096
SIZES = [5, 2 * GRID_BIG * 8 + 3, 2 * GRID_BIG * (512 + 256 + 8) + 1]
N_MID = SIZES[1]
REPLAYED = [0, 2, 7]
POINTS = [1, 3, 7]


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
def _ran(out, mode, npts):
    return out["symbol"].endswith("true>") and f", {mode}, {npts}, " in out["symbol"]


def _check_lean_launches(cgo, ctx, kind, n, r):
    d, pairs, a_acc, beta, steps = _launch_data(kind, n, 23 + n % 97)
    o = _objective(cgo, kind, n, d, ctx)
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.DisableTrace(), max_iters=5)
    s = cgo.Solver(o, cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), _policy(cgo))
    bad = []
    try:
        x0, u0, lst = d["x"], d["u"], pairs[:r]
        for k in POINTS:
            a = steps[:k]
            tag = f"{kind} n={n} r={r} k={k}"
            N = s.probe_launch("accept_trial_nostore", MODE_N, a_acc, beta, a, x0, u0, replay=lst)
            S = s.probe_launch("accept_dir_trial", MODE_S, a_acc, beta, a, x0, u0, replay=lst)
            NL = s.probe_launch("accept_trial_nostore", LEAN_N, a_acc, beta, a, x0, u0, replay=lst)
            SL = s.probe_launch("accept_dir_trial", LEAN_S, a_acc, beta, a, x0, u0, replay=lst)
            assert _ran(N, MODE_N, k) and _ran(S, MODE_S, k), (N["symbol"], S["symbol"])
            assert np.all(np.isfinite(N["sums"])) and np.all(np.isfinite(S["sums"])), tag
            if not _ran(NL, LEAN_N, k):
                bad.append(f"{tag}: lean N ran {NL['symbol']}")
            if not _ran(SL, LEAN_S, k):
                bad.append(f"{tag}: lean S ran {SL['symbol']}")
            dropped = np.zeros(N["sums"].size, dtype=bool)
            for j in range(k):
                dropped[[RS_PER_POINT * j + RS_GTG, RS_PER_POINT * j + RS_YY, RS_PER_POINT * j + RS_UY]] = True
            for name, lean, full in (("N", NL, N), ("S", SL, S)):
                if lean["sums"].shape != full["sums"].shape:
                    bad.append(f"{tag}: lean {name}'s row has {lean['sums'].size} slots, the full one {full['sums'].size}")
                    continue
                diff = np.nonzero(bits(lean["sums"])[~dropped] != bits(full["sums"])[~dropped])[0]
                if diff.size:
                    bad.append(f"{tag}: lean {name}: kept slots {np.nonzero(~dropped)[0][diff].tolist()} differ from the full launch's")
                nz = np.nonzero(bits(lean["sums"])[dropped] != 0)[0]
                if nz.size:
                    bad.append(f"{tag}: lean {name}: dropped slots {np.nonzero(dropped)[0][nz].tolist()} are not +0.0")
                if not np.all(bits(full["sums"])[dropped] != 0):
                    bad.append(f"{tag}: full {name} left a dropped slot +0.0 itself: the inputs do not tell the rows apart")
            if not (same(SL["x"], S["x"]) and same(SL["u"], S["u"])):
                bad.append(f"{tag}: lean S's x or u differs from full S's")
            if not (same(NL["x"], x0) and same(NL["u"], u0)):
                bad.append(f"{tag}: lean N wrote x or u")
    finally:
        s.close(); o.close()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("r", REPLAYED, ids=lambda r: f"r{r}")
@pytest.mark.parametrize("n", SIZES, ids=lambda n: f"n{n}")
def test_quad_lean_launches_equal_full_launches(cgo, ctx, n, r):
    _check_lean_launches(cgo, ctx, "quad", n, r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", REPLAYED, ids=lambda r: f"r{r}")
def test_rosenbrock_paired_lean_launches_equal_full_launches(cgo, ctx, r):
    _check_lean_launches(cgo, ctx, "rosen", N_MID - 1, r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", REPLAYED, ids=lambda r: f"r{r}")
def test_booth_lean_launches_equal_full_launches(cgo, ctx, r):
    _check_lean_launches(cgo, ctx, "booth", 2, r)


@pytest.mark.gpu
def test_probe_rejects_lean_modes_it_has_no_row_for(cgo, ctx):
    """a mask without rows, the lean bits on the trial-only launch, and any lean mode on a stencil objective"""
    d, pairs, a_acc, beta, steps = _launch_data("quad", 5, 1)
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.DisableTrace(), max_iters=5)
    ls = cgo.setupStrongWolfeBisection(1e-5, 0.1)
    o = cgo.QuadDiag(d["p"], ctx)
    s = cgo.Solver(o, cfg, ls, _policy(cgo))
    try:
        for kind, mode in (("accept_trial_nostore", MODE_N | R_NOGTG), ("accept_dir_trial", MODE_S | R_NOYGT),
                           ("accept_dir_trial", LEAN_N), ("accept_trial_nostore", LEAN_S),
                           ("trial", R_REPLAY | R_TRIAL | PR_MASK), ("accept_dir_trial", ADT | PR_MASK)):
            with pytest.raises(cgo.CgoError):
                s.probe_launch(kind, mode, a_acc, beta, steps[:3], d["x"], d["u"], replay=pairs[:2])
    finally:
        s.close(); o.close()
    o = cgo.RosenbrockChained(64, ctx)
    s = cgo.Solver(o, cfg, ls, _policy(cgo))
    try:
        x = np.tile([-1.2, 1.0], 32)
        for kind, mode in (("accept_trial_nostore", LEAN_N), ("accept_dir_trial", LEAN_S)):
            with pytest.raises(cgo.CgoError):
                s.probe_launch(kind, mode, 1e-4, 0.1, [1e-4], x, -x, replay=[])
    finally:
        s.close(); o.close()


# ---- (2) whole solves ----------------------------------------------------------------------------------------------------
def _solve(cgo, make_obj, cfg, ls, x0, depth, lean, ctx, chunk=0, between=None):
    """One solve through the Solver at replay depth `depth`; lean: True / False through set_lean_sums, None: whatever the
    library and the environment decide.  between(solver, slice number) runs after every slice of `chunk` iterations that
    does not end the solve."""
    o = make_obj(ctx)
    s = cgo.Solver(o, cfg, ls, _policy(cgo))
    mid = []
    try:
        s.set_lazy_direction(True)
        s.set_replay_depth(depth)
        if lean is not None:
            s.set_lean_sums(lean)
        syms = {k: s.kernel_symbol(k) for k in ("accept_trial_nostore", "accept_dir_trial")}
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
    return dict(r=r, log=log, prof=prof, mid=mid, syms=syms)


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
    assert len(on["log"]) == len(off["log"]) >= 1
    for la, lb in zip(on["log"], off["log"]):
        assert same(la, lb), name
    assert set(on["prof"]) == set(off["prof"]), (name, on["prof"], off["prof"])


def _lean_symbols(syms, obj="ObjQuadDiag"):
    return syms["accept_trial_nostore"] == f"k_cg<{obj}, {LEAN_N}, 7, true>" and syms["accept_dir_trial"] == f"k_cg<{obj}, {LEAN_S}, 7, true>"


def _full_symbols(syms, obj="ObjQuadDiag"):
    return syms["accept_trial_nostore"] == f"k_cg<{obj}, {MODE_N}, 7, true>" and syms["accept_dir_trial"] == f"k_cg<{obj}, {MODE_S}, 7, true>"


def _quad(cgo, n):
    D = quad_D(n)
    return lambda ctx: cgo.QuadDiag(D, ctx)


def _sw(cgo):
    return cgo.setupStrongWolfeBisection(1e-5, 0.1)


def _cfg(cgo, beta=None, iters=13):
    return cgo.setupCGConfig(1e-12, beta if beta is not None else cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=iters)


@pytest.fixture(scope="module")
def lean_off(cgo, ctx):
    """the lean-off solves the tests below compare against, one per depth, computed once"""
    memo = {}

    def get(depth):
        if depth not in memo:
            memo[depth] = _solve(cgo, _quad(cgo, N_MID), _cfg(cgo), _sw(cgo), np.ones(N_MID), depth, False, ctx)
            assert _full_symbols(memo[depth]["syms"]), memo[depth]["syms"]
            assert memo[depth]["r"].iters_ran == 13
            assert memo[depth]["prof"]["accept_trial_nostore"]["launches"] >= 1
        return memo[depth]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 4, 6, 8], ids=lambda d: f"d{d}")
def test_quad_pr_strong_wolfe_lean_equals_full_by_setter(cgo, ctx, lean_off, monkeypatch, depth):
    monkeypatch.delenv("CGO_LEAN_SUMS", raising=False)
    on = _solve(cgo, _quad(cgo, N_MID), _cfg(cgo), _sw(cgo), np.ones(N_MID), depth, True, ctx)
    assert _lean_symbols(on["syms"]), on["syms"]
    _assert_equal_solves(on, lean_off(depth), f"quad-PR-d{depth}")
    assert on["prof"]["accept_trial_nostore"]["launches"] >= 1
    if depth <= 6:
        assert on["prof"]["accept_dir_trial"]["launches"] >= 1      # at least one whole cycle: an S launch ran


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 4, 6, 8], ids=lambda d: f"d{d}")
def test_quad_pr_strong_wolfe_lean_equals_full_by_environment(cgo, ctx, lean_off, monkeypatch, depth):
    monkeypatch.setenv("CGO_LEAN_SUMS", "1")
    on = _solve(cgo, _quad(cgo, N_MID), _cfg(cgo), _sw(cgo), np.ones(N_MID), depth, None, ctx)
    monkeypatch.setenv("CGO_LEAN_SUMS", "0")
    off = _solve(cgo, _quad(cgo, N_MID), _cfg(cgo), _sw(cgo), np.ones(N_MID), depth, None, ctx)
    assert _lean_symbols(on["syms"]) and _full_symbols(off["syms"]), (on["syms"], off["syms"])
    _assert_equal_solves(on, off, f"quad-PR-env-d{depth}")
    _assert_equal_solves(on, lean_off(depth), f"quad-PR-env-d{depth} against the setter's lean-off solve")


@pytest.mark.gpu
def test_results_fetched_mid_cycle_lean_equals_full(cgo, ctx):
    """results(vectors=True) after 2, 4, 6, … iterations: materialise passes ride in between the lean launches"""
    fetch = lambda s, i: s.results(vectors=True)
    on = _solve(cgo, _quad(cgo, N_MID), _cfg(cgo), _sw(cgo), np.ones(N_MID), 4, True, ctx, chunk=2, between=fetch)
    off = _solve(cgo, _quad(cgo, N_MID), _cfg(cgo), _sw(cgo), np.ones(N_MID), 4, False, ctx, chunk=2, between=fetch)
    _assert_equal_solves(on, off, "mid-results")
    assert len(on["mid"]) == len(off["mid"]) >= 5
    for i, (a, b) in enumerate(zip(on["mid"], off["mid"])):
        _assert_equal_results(a, b, f"mid-results slice {i}")
    assert on["prof"].get("materialize_xu", {}).get("launches", 0) >= 1, on["prof"]


@pytest.mark.gpu
def test_lean_switch_toggled_mid_solve(cgo, ctx, lean_off):
    """no pass is needed to switch: the stored state is the same either way"""
    seen = []

    def toggle(s, i):
        s.set_lean_sums(i % 2 == 1)
        seen.append(s.kernel_symbol("accept_trial_nostore"))
    on = _solve(cgo, _quad(cgo, N_MID), _cfg(cgo), _sw(cgo), np.ones(N_MID), 4, True, ctx, chunk=2, between=toggle)
    off = _solve(cgo, _quad(cgo, N_MID), _cfg(cgo), _sw(cgo), np.ones(N_MID), 4, False, ctx, chunk=2)
    _assert_equal_solves(on, off, "toggle")
    _assert_equal_solves(on, lean_off(4), "toggle against one call")
    assert f", {MODE_N}, " in seen[0] and f", {LEAN_N}, " in seen[1], seen
    assert "materialize_xu" not in on["prof"], on["prof"]


@pytest.mark.gpu
def test_rerun_chain_lean_equals_full(cgo, monkeypatch):
    """cgo_minimize_rerun builds its solvers itself: CGO_LEAN_SUMS reaches them"""
    n = N_MID
    D = quad_D(n)
    ls = _sw(cgo)
    cfgs = [cgo.setupCGConfig(e, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=m) for e, m in ((1e-2, 5), (1e-4, 6), (1e-6, 7))]
    monkeypatch.setenv("CGO_LAZY_DIR", "1")
    monkeypatch.setenv("CGO_REPLAY_DEPTH", "3")
    out = {}
    for lean in ("1", "0"):
        monkeypatch.setenv("CGO_LEAN_SUMS", lean)
        c = cgo.Context(0)
        c.set_default_policy(_policy(cgo))
        o = cgo.QuadDiag(D, c)
        try:
            s = cgo.Solver(o, cfgs[0], ls, _policy(cgo))      # what a solver built under this environment launches
            syms = {k: s.kernel_symbol(k) for k in ("accept_trial_nostore", "accept_dir_trial")}
            s.close()
            assert (_lean_symbols if lean == "1" else _full_symbols)(syms), syms
            out[lean] = cgo.minimizeobjectivererun(o, np.ones(n), cfgs[0], ls, (cfgs[1], ls), (cfgs[2], ls))
        finally:
            o.close(); c.close()
    assert len(out["1"]) == len(out["0"]) >= 2
    for a, b in zip(out["1"], out["0"]):
        _assert_equal_results(a, b, "rerun")


@pytest.mark.gpu
def test_two_virtual_ranks_lean_equals_full(cgo):
    """two contexts of one process as two ranks over the callback transport: the exchanged rows carry the zeros"""
    n, W = 2 * N_MID, 2
    D = quad_D(n)
    cfg = _cfg(cgo, iters=10)
    ls = _sw(cgo)

    def run(lean):
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
                outs[rank] = _solve(cgo, lambda cx: cgo.QuadDiag(D, cx), cfg, ls, np.ones(n), 4, lean, c)
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
        assert _lean_symbols(on[r]["syms"]) and _full_symbols(off[r]["syms"])
        assert on[r]["prof"].get("accept_trial_nostore", {}).get("launches", 0) >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", ["HagerZhang", "DaiYuan"])
def test_flavours_without_rows_keep_the_full_rows(cgo, ctx, monkeypatch, flavour):
    monkeypatch.setenv("CGO_LEAN_SUMS", "1")
    cfg = _cfg(cgo, getattr(cgo, flavour)())
    on = _solve(cgo, _quad(cgo, N_MID), cfg, _sw(cgo), np.ones(N_MID), 4, True, ctx)
    monkeypatch.setenv("CGO_LEAN_SUMS", "0")
    off = _solve(cgo, _quad(cgo, N_MID), cfg, _sw(cgo), np.ones(N_MID), 4, False, ctx)
    assert _full_symbols(on["syms"]) and _full_symbols(off["syms"]), (on["syms"], off["syms"])
    _assert_equal_solves(on, off, flavour)
    assert on["prof"].get("accept_trial_nostore", {}).get("launches", 0) >= 1, on["prof"]


# ---- (3) profile and symbols ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_profile_and_symbols_name_what_ran(cgo, ctx, lean_off, monkeypatch):
    monkeypatch.delenv("CGO_LEAN_SUMS", raising=False)
    n = N_MID
    on = _solve(cgo, _quad(cgo, n), _cfg(cgo), _sw(cgo), np.ones(n), 4, True, ctx)
    off = lean_off(4)
    dflt = _solve(cgo, _quad(cgo, n), _cfg(cgo), _sw(cgo), np.ones(n), 4, None, ctx)      # hbm_stream_bytes = 1.0 switches nothing on
    assert _lean_symbols(on["syms"]), on["syms"]
    assert off["syms"] == dflt["syms"] == {"accept_trial_nostore": "k_cg<ObjQuadDiag, 14343, 7, true>", "accept_dir_trial": "k_cg<ObjQuadDiag, 4103, 7, true>"}
    assert set(on["prof"]) == set(off["prof"]) == set(dflt["prof"])
    for kind in on["prof"]:
        assert on["prof"][kind]["launches"] == off["prof"][kind]["launches"], kind
        assert on["prof"][kind]["bytes_per_launch"] == off["prof"][kind]["bytes_per_launch"], kind
    assert on["prof"]["accept_trial_nostore"]["bytes_per_launch"] == 8.0 * n * 3
    assert on["prof"]["accept_dir_trial"]["bytes_per_launch"] == 8.0 * n * 5


# ---- (4) CPU tier: the table ---------------------------------------------------------------------------------------------
def test_lean_rows_parse_and_are_disjoint_from_the_pinned_lists(monkeypatch):
    for name, bit in (("R_ULAG", 1024), ("R_NOWU", R_NOWU), ("R_REPLAY", R_REPLAY), ("R_NOWX", R_NOWX),
                      ("R_NOGTG", R_NOGTG), ("R_NOYY", R_NOYY), ("R_NOUY", R_NOUY), ("R_NOYGT", R_NOYGT)):
        monkeypatch.setitem(I.BITS, name, bit)
    assert I.rows("CG_LEAN") == [(LEAN_N, 7), (LEAN_S, 7)]
    assert len(I.mode_points("CG_LEAN")) * len(I.rows("OBJ")) == 24
    lean = {m for m, _ in I.rows("CG_LEAN")}
    for fam in ("CG", "CG_LAG", "CG_REPLAY"):
        assert not lean & {m for m, _ in I.rows(fam)}, fam
    assert (len(I.rows("CG")), len(I.rows("CG_LAG")), len(I.rows("CG_REPLAY"))) == (12, 4, 4)
    assert I.stray_uses() == []
    hdr = open(os.path.join(I.CSRC, "cgo_modes.hpp")).read()
    for name, bit in (("R_NOGTG", 16384), ("R_NOYY", 32768), ("R_NOUY", 65536), ("R_NOYGT", 131072)):
        assert re.search(r"\b%s = %d\b" % (name, bit), hdr), name
    assert "CGO_CG_LEAN_ROWS" not in open(os.path.join(I.CSRC, "cgo_rtc.hip")).read()      # built-in objectives only
    assert "CGO_CG_LEAN_ROWS(ROW)" in open(os.path.join(I.CSRC, "cgo_backend_cg.hip")).read()


def test_entry_point_is_declared_exported_and_bound(cgo):
    from cgo_amd import _lib
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cgo.h")).read(), flags=re.S)
    name = "cgo_solver_set_lean_sums"
    assert re.search(r"\bint %s\s*\(" % name, src)
    assert hasattr(L, name) and name in _lib.SIGNATURES
    assert hasattr(cgo.Solver, "set_lean_sums")
    assert "CGO_LEAN_SUMS" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert not re.search(r"lean", re.search(r"typedef struct cgo_solver_policy \{.*?\} cgo_solver_policy;", src, re.S).group(0))


# ---- (5) CPU tier: the mask ----------------------------------------------------------------------------------------------
MASK_PROGRAM = r'''
#include <cstdio>
#include <cstring>
#include <cmath>
#include "cgo_ctl.hpp"
using namespace cgo;
static unsigned long long st = 0x9E3779B97F4A7C15ull;
static double rnd(double lo, double hi) {   // splitmix64
    unsigned long long z = (st += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return lo + (hi - lo) * (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
static TrialSums masked(TrialSums t, int m, double v) {
    if (m & CTL_NOGTG) t.gtg = v;
    if (m & CTL_NOYY) t.yy = v;
    if (m & CTL_NOUY) t.uy = v;
    if (m & CTL_NOYGT) t.ygt = v;
    return t;
}
static double beta_of(int kind, const TrialSums &t, double gu, double gg, double uu, bool &ok) {
    ok = beta_norms_fast_ok(kind, t, uu);
    return beta_from_sums(kind, 0.1, t, gu, gg, uu, beta_norms_fast(t, uu));
}
int main() {
    static_assert(CTL_NOGTG == 16384 && CTL_NOYY == 32768 && CTL_NOUY == 65536 && CTL_NOYGT == 131072, "the mode bits of the k_cg family");
    const int all = CTL_NOGTG | CTL_NOYY | CTL_NOUY | CTL_NOYGT;
    int bad = 0;
    for (int kind = 0; kind <= CGO_BETA_BROYDEN_FAMILY; ++kind) {
        const int m = beta_unread_sums(kind);
        std::printf("mask %d %d\n", kind, m);
        if (m & ~all) { std::printf("kind %d: a bit that names no droppable sum (f, gtu and gtgt have none)\n", kind); ++bad; }
        for (int i = 0; i < 400; ++i) {
            TrialSums t;
            t.f = rnd(-10, 10); t.gtu = rnd(-3, 3); t.gtgt = rnd(1e-3, 50); t.gtg = rnd(-50, 50);
            t.yy = rnd(1e-3, 80); t.uy = rnd(-5, 5); t.ygt = rnd(-40, 40);
            if (i % 7 == 0) t.gtg = t.gtgt * rnd(0.0, 2.0);      // both branches of Salleh–Alhawarat
            if (i % 50 == 0) t.yy = 1e-300;                       // the range tests of the norms
            if (i % 50 == 1) t.gtgt = 1e305;
            const double gu = rnd(-4, -1e-3), gg = rnd(1e-3, 60), uu = (i % 50 == 2) ? 1e-290 : rnd(1e-3, 60);
            bool ok0, ok1, ok2;
            const double b0 = beta_of(kind, t, gu, gg, uu, ok0);
            const double b1 = beta_of(kind, masked(t, m, 0.0), gu, gg, uu, ok1);
            const double b2 = beta_of(kind, masked(t, m, std::nan("")), gu, gg, uu, ok2);
            if (std::memcmp(&b0, &b1, 8) || std::memcmp(&b0, &b2, 8) || ok0 != ok1 || ok0 != ok2) {
                if (bad < 20) std::printf("kind %d draw %d: beta %a / zeros %a / NaNs %a, norms ok %d %d %d\n", kind, i, b0, b1, b2, ok0, ok1, ok2);
                ++bad;
            }
        }
    }
    std::printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
'''


def test_masked_sums_give_the_same_beta_for_every_flavour(tmp_path):
    """host code with its own main: β (beta_from_sums on beta_norms_fast) and beta_norms_fast_ok from 400 seeded TrialSums per
    flavour, full / masked slots 0.0 / masked slots NaN — bitwise equal; f, gtu and gtgt are in no mask"""
    src, exe = tmp_path / "lean_mask.cpp", tmp_path / "lean_mask"
    src.write_text(MASK_PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", I.CSRC, str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("bad 0"), r.stdout + r.stderr
    masks = {int(a): int(b) for a, b in re.findall(r"^mask (\d+) (\d+)$", r.stdout, re.M)}
    HZ, YWS, SA, LS, PR, HS, DY, LBFGS, BROYDEN = range(9)
    assert masks[PR] == PR_MASK
    assert masks[HZ] == R_NOGTG and masks[SA] == R_NOYY | R_NOUY | R_NOYGT and masks[DY] == R_NOGTG | R_NOYY | R_NOYGT
    assert masks[LS] == masks[HS] == R_NOGTG | R_NOYY
    assert masks[YWS] == masks[LBFGS] == masks[BROYDEN] == 0
