"""Late scaling of f in the lean rows: the quadratic's objective term is ½·(D·x²), and lean N and lean S add the
raw terms D·x² and multiply each lane's f accumulators by ½ once, before the reduction.  Scaling by a power of two commutes with
rounding while every nonzero term and partial sum is a normal number and the unscaled sum is finite, so inside that domain a lean
launch's f slots are the full launch's bit for bit.

(1) per launch, bit for bit, on inputs spread over 140 decades (all terms normal, all sums finite): lean N and lean S against
    full N and full S — every kept slot, the f slots included; dropped slots +0.0; x and u; the symbols that ran;
(2) outside the domain (n = 5, subnormal terms D·x²): every slot but f bit for bit, f within (number of terms) × 2^-1074;
(3) paired Rosenbrock and Booth declare no scale: their lean launches are their full launches bit for bit;
(4) CPU tier: who declares the trait, the A/B switch, the row lists, and the arithmetic fact (1) rests on.

All GPU solvers use hbm_stream_bytes = 1.0 like tests/test_lean_sums.py, whose sizes and launch recipe these are."""
import glob
import os
import re

import numpy as np
import pytest

import _instances as I
from test_replay_state import _launch_data, _objective

R_ACCEPT, R_DIR, R_TRIAL, R_NOWU, R_REPLAY, R_NOWX = 1, 2, 4, 2048, 4096, 8192
R_NOGTG, R_NOYY, R_NOUY, R_NOYGT = 16384, 32768, 65536, 131072
ADT = R_ACCEPT | R_DIR | R_TRIAL
MODE_N, MODE_S = R_REPLAY | ADT | R_NOWU | R_NOWX, R_REPLAY | ADT
PR_MASK = R_NOGTG | R_NOYY | R_NOUY
LEAN_N, LEAN_S = MODE_N | PR_MASK, MODE_S | PR_MASK
RS_F, RS_GTG, RS_YY, RS_UY, RS_PER_POINT = 0, 3, 4, 5, 7
GRID_BIG = 4096
SIZES = [5, 2 * GRID_BIG * 8 + 3, 2 * GRID_BIG * (512 + 256 + 8) + 1]
N_MID = SIZES[1]
REPLAYED = [0, 2, 7]
POINTS = [1, 3, 7]
TINY = 2.0 ** -1074


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


def _wide(rng, n):
    """magnitudes log-uniform in [1e-70, 1e70], mixed signs, about 1 % exact zeros"""
    v = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-70.0, 70.0, n)
    v[rng.random(n) < 0.01] = 0.0
    return v


_WIDE = {}


def _wide_data(n):
    """x, u over 140 decades and D in [1, 1000], once per size: D·x² ≥ 1e-140 wherever it is not zero.  With steps ≤ 1/8 and
    β ≤ 1/16, V = max(1000·|x|, |u|) grows by less than 127 per step (x ← x + a·u, u ← −D·x + β·u), so after seven replayed
    steps and the accepted one V < 1e73·127^8 < 1e90, a trial point is below 1e90 and every product below 1e186: the sums of
    6.4e6 of them are finite (the test asserts it on the full launch)"""
    if n not in _WIDE:
        rng = np.random.default_rng(1000 + n % 97)
        _WIDE[n] = dict(x=_wide(rng, n), u=_wide(rng, n), p=rng.uniform(1.0, 1000.0, n))
    return _WIDE[n]


def _ran(out, mode, npts):
    return out["symbol"].endswith("true>") and f", {mode}, {npts}, " in out["symbol"]


def _dropped(size, k):
    d = np.zeros(size, dtype=bool)
    for j in range(k):
        d[[RS_PER_POINT * j + RS_GTG, RS_PER_POINT * j + RS_YY, RS_PER_POINT * j + RS_UY]] = True
    return d


def _four(s, a_acc, beta, a, x0, u0, lst):
    return (s.probe_launch("accept_trial_nostore", MODE_N, a_acc, beta, a, x0, u0, replay=lst),
            s.probe_launch("accept_dir_trial", MODE_S, a_acc, beta, a, x0, u0, replay=lst),
            s.probe_launch("accept_trial_nostore", LEAN_N, a_acc, beta, a, x0, u0, replay=lst),
            s.probe_launch("accept_dir_trial", LEAN_S, a_acc, beta, a, x0, u0, replay=lst))


def _solver(cgo, o):
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.DisableTrace(), max_iters=5)
    return cgo.Solver(o, cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), _policy(cgo))


def _compare(tag, k, N, S, NL, SL, x0, u0, bad, f_bound=None):
    """lean against full; f_bound: None — the f slots bit for bit like every kept slot —, or the largest |difference| allowed"""
    if not _ran(NL, LEAN_N, k):
        bad.append(f"{tag}: lean N ran {NL['symbol']}")
    if not _ran(SL, LEAN_S, k):
        bad.append(f"{tag}: lean S ran {SL['symbol']}")
    dropped = _dropped(N["sums"].size, k)
    fslot = np.zeros(N["sums"].size, dtype=bool)
    fslot[[RS_PER_POINT * j + RS_F for j in range(k)]] = True
    for name, lean, full in (("N", NL, N), ("S", SL, S)):
        if lean["sums"].shape != full["sums"].shape:
            bad.append(f"{tag}: lean {name}'s row has {lean['sums'].size} slots, the full one {full['sums'].size}")
            continue
        kept = ~dropped if f_bound is None else ~dropped & ~fslot
        diff = np.nonzero(kept & (bits(lean["sums"]) != bits(full["sums"])))[0]
        if diff.size:
            what = [(int(i), float(lean["sums"][i]).hex(), float(full["sums"][i]).hex()) for i in diff[:4]]
            bad.append(f"{tag}: lean {name}: kept slots {diff.tolist()} differ from the full launch's (slot, lean, full): {what}")
        if f_bound is not None:
            err = np.abs(lean["sums"][fslot] - full["sums"][fslot])
            print(f"{tag}: lean {name} f {[float(v).hex() for v in lean['sums'][fslot]]} full {[float(v).hex() for v in full['sums'][fslot]]}")
            if not np.all(err <= f_bound):
                bad.append(f"{tag}: lean {name}: f slots off by {err.tolist()}, allowed {f_bound}")
        nz = np.nonzero(bits(lean["sums"])[dropped] != 0)[0]
        if nz.size:
            bad.append(f"{tag}: lean {name}: dropped slots {np.nonzero(dropped)[0][nz].tolist()} are not +0.0")
    if not (same(SL["x"], S["x"]) and same(SL["u"], S["u"])):
        bad.append(f"{tag}: lean S's x or u differs from full S's")
    if not (same(NL["x"], x0) and same(NL["u"], u0) and same(N["x"], x0) and same(N["u"], u0)):
        bad.append(f"{tag}: a no-store launch wrote x or u")


# ---- (1) per launch, inside the domain -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("r", REPLAYED, ids=lambda r: f"r{r}")
@pytest.mark.parametrize("n", SIZES, ids=lambda n: f"n{n}")
def test_quad_lean_f_slots_equal_the_full_launch_bit_for_bit(cgo, ctx, n, r):
    _, pairs, a_acc, beta, steps = _launch_data("quad", n, 23 + n % 97)
    d = _wide_data(n)
    o = cgo.QuadDiag(d["p"], ctx)
    s = _solver(cgo, o)
    bad = []
    try:
        x0, u0, lst = d["x"], d["u"], pairs[:r]
        for k in POINTS:
            tag = f"quad n={n} r={r} k={k}"
            N, S, NL, SL = _four(s, a_acc, beta, steps[:k], x0, u0, lst)
            assert _ran(N, MODE_N, k) and _ran(S, MODE_S, k), (N["symbol"], S["symbol"])
            assert np.all(np.isfinite(N["sums"])) and np.all(np.isfinite(S["sums"])), tag      # the domain: every full-row sum finite
            f = N["sums"][[RS_PER_POINT * j + RS_F for j in range(k)]]
            assert np.all(f >= 2.0 ** -1021), (tag, f)                                          # … and f itself far from subnormal
            _compare(tag, k, N, S, NL, SL, x0, u0, bad)
    finally:
        s.close(); o.close()
    assert not bad, "\n".join(bad)


# ---- (2) outside the domain: subnormal terms -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_subnormal_terms_move_only_the_f_slots_and_by_less_than_one_subnormal_step_per_term(cgo, ctx):
    """n = 5, D = 1, u = 0, nothing replayed: the accept step leaves x, the new direction is −x, and the trial point of step a is
    x·(1 − a) exactly for the steps below.  Elements 0 and 1 (one lane) sit at 2^-536, so at a = ½ both terms are 2^-1074: halved
    one by one they round to zero, summed first they give 2^-1074 — early and late scaling differ in the last subnormal bit there,
    and the other steps give terms of a few subnormal steps each.  Elements 2, 3 and the odd tail add a subnormal, a zero and a
    normal term.  The documented bound is one subnormal step per term: 5 × 2^-1074."""
    n = 5
    x0 = np.array([2.0 ** -536, 2.0 ** -536, 3 * 2.0 ** -537, 0.0, 2.0 ** -530])
    u0 = np.zeros(n)
    steps = [0.5, 0.25, 0.75, 0.125, 0.375, 0.625, 0.875]
    o = cgo.QuadDiag(np.ones(n), ctx)
    s = _solver(cgo, o)
    bad = []
    try:
        for k in POINTS:
            tag = f"subnormal k={k}"
            N, S, NL, SL = _four(s, 0.25, 0.5, steps[:k], x0, u0, [])
            assert _ran(N, MODE_N, k) and _ran(S, MODE_S, k), (N["symbol"], S["symbol"])
            assert np.all(np.isfinite(N["sums"])) and np.all(np.isfinite(S["sums"])), tag
            f = N["sums"][[RS_PER_POINT * j + RS_F for j in range(k)]]
            assert np.all(f < 2.0 ** -1022) and np.all(f > 0.0), (tag, f)                       # the sums ARE subnormal
            _compare(tag, k, N, S, NL, SL, x0, u0, bad, f_bound=n * TINY)
    finally:
        s.close(); o.close()
    assert not bad, "\n".join(bad)


# ---- (3) objectives that declare no scale ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [("rosen", N_MID - 1), ("booth", 2)], ids=["rosen", "booth"])
def test_objectives_without_a_scale_keep_their_lean_launches(cgo, ctx, kind, n):
    d, pairs, a_acc, beta, steps = _launch_data(kind, n, 23 + n % 97)
    o = _objective(cgo, kind, n, d, ctx)
    s = _solver(cgo, o)
    bad = []
    try:
        N, S, NL, SL = _four(s, a_acc, beta, steps, d["x"], d["u"], pairs[:2])
        assert _ran(N, MODE_N, 7) and _ran(S, MODE_S, 7), (N["symbol"], S["symbol"])
        assert np.all(np.isfinite(N["sums"])) and np.all(np.isfinite(S["sums"]))
        _compare(f"{kind} n={n} r=2 k=7", 7, N, S, NL, SL, d["x"], d["u"], bad)
    finally:
        s.close(); o.close()
    assert not bad, "\n".join(bad)


# ---- (4) CPU tier ----------------------------------------------------------------------------------------------------------
def _functors():
    """name → body of every objective functor (`struct Obj… { … };`) in the kernel headers"""
    out = {}
    for path in sorted(glob.glob(os.path.join(I.CSRC, "*.hpp"))):
        for m in re.finditer(r"^struct (Obj\w+) \{.*?^\};", open(path).read(), re.M | re.S):
            out[m.group(1)] = m.group(0)
    return out


def test_only_the_quadratic_declares_a_scale():
    fs = _functors()
    assert {"ObjQuadDiag", "ObjRosenPaired", "ObjBooth"} <= set(fs), sorted(fs)
    assert [name for name, body in fs.items() if "kFScale" in body] == ["ObjQuadDiag"]
    q = fs["ObjQuadDiag"]
    assert re.search(r"static constexpr double kFScale = 0\.5;", q) and "eval2_raw" in q and "eval1_raw" in q


def test_switch_and_trait_stand_in_the_kernel_header():
    hdr = open(os.path.join(I.CSRC, "cgo_kernels_cg.hip.hpp")).read()
    assert "#ifdef CGO_LEAN_SCALE_EARLY" in hdr
    m = re.search(r"struct LateF \{.*?\};\n", hdr, re.S)
    assert m and "ObjFScale<Obj>::declared && (MODE & R_LEAN) != 0" in m.group(0), "on where the objective declares it and the row is lean"
    assert hdr.index("struct RW {") < hdr.index("struct LateF {") < hdr.index("void cg_pair(")
    assert "CGO_LEAN_SCALE_EARLY" not in open(os.path.join(I.CSRC, "Makefile")).read()       # an EXTRA= switch, never a default


def test_row_lists_are_unchanged(monkeypatch):
    for name, bit in (("R_ULAG", 1024), ("R_NOWU", R_NOWU), ("R_REPLAY", R_REPLAY), ("R_NOWX", R_NOWX),
                      ("R_NOGTG", R_NOGTG), ("R_NOYY", R_NOYY), ("R_NOUY", R_NOUY), ("R_NOYGT", R_NOYGT)):
        monkeypatch.setitem(I.BITS, name, bit)
    assert I.rows("CG_LEAN") == [(LEAN_N, 7), (LEAN_S, 7)] == [(129031, 7), (118791, 7)]
    assert len(I.mode_points("CG_LEAN")) * len(I.rows("OBJ")) == 24
    assert (len(I.rows("CG")), len(I.rows("CG_LAG")), len(I.rows("CG_REPLAY"))) == (12, 4, 4)
    hdr = open(os.path.join(I.CSRC, "cgo_modes.hpp")).read()
    assert not re.search(r"R_\w+ = 262144\b", hdr), "no new mode bit"


def test_halving_commutes_with_sequential_summation_over_the_tested_range():
    """the arithmetic fact (1) rests on, on the CPU: Σ ½·t and ½·Σ t, summed in index order, are the same bits for the terms
    t = (D·x)·x of the widest test vector's first 2^16 elements — and differ once terms are subnormal"""
    d = _wide_data(SIZES[2])
    x, p = d["x"][:1 << 16], d["p"][:1 << 16]
    t = (p * x) * x
    assert np.all((t == 0.0) | (t >= 1e-141)) and np.count_nonzero(t == 0.0) > 100
    early, late = np.cumsum(0.5 * t), 0.5 * np.cumsum(t)
    assert np.all(np.isfinite(late)) and same(early, late)
    for chunk in (x[:4096], x[4096:8192]):           # a lane-sized chain starting from its own zero
        tc = (p[:4096] * chunk) * chunk
        assert same(np.cumsum(0.5 * tc), 0.5 * np.cumsum(tc))
    sub = np.array([TINY, TINY])
    assert np.cumsum(0.5 * sub)[-1] == 0.0 and 0.5 * np.cumsum(sub)[-1] == TINY
