"""Controller-armed rounds, one batch at a time (cgo_solver_probe_armed): every sum, every word of the record and of the next state.

The trajectory suites see an armed round only through the numbers the host replay reads — the sums of the points the line search
lands on, the sums the β flavour uses, `a_acc`, `beta`, `npts` and `a[0..npts)` of a record.  Here

(a) one round on the exact data of tests/test_kernel_sums.py (every summation order gives the same bits): all 56 slots of the
    record and the device row against the exact row, x and u bit for bit, the record's echo of the state it ran with — for every
    form of a round: `k_cg_armed` (default and strict tails), `k_cg + k_finalize_ctl`, `+ k_finalize_t` above 64 rows, pure-HBM;
(b) the decision: `accepted`, the whole next CtlState, the argument block and the round counter against ctl_step as the HOST
    compiles it (tests/hostsim: sim_ctl_step) on that exact row, byte for byte — every β flavour, both bisection line searches,
    Backtracking (never accepted), with f_x, eps and max_iters chosen so that rounds are accepted and stopped;
(c) a decision table of synthetic rows reaching every way ctl_decide can leave: on the CPU tier the host-compiled ctl_step is held
    to the table's hand-stated `accepted` column and to the trial-point tree written out here in Python; on the GPU
    k_finalize_ctl<10|24|40|56> alone (form "controller") is held to the host's bytes on the same table;
(d) chains of 8, 12 and 7 rounds — one by one and as captured graphs of 8, 8 + 4 and 4 + 2 + 1 — against a chain of plain
    host-driven launches of a second solver (controller_depth = 0) with the host-compiled ctl_step in between, every record
    slot, x and u bit for bit, with the controller stopping inside the batch and idle records behind it;
(e) a stopped controller moves nothing, the round counter runs on from probe to probe, the 64-slot record ring wraps;
(f) the symbols reached are the armed rows of csrc/cgo_instances.def and the four widths of k_finalize_ctl, no more, no fewer.
"""
import ctypes as C
import math
from collections import defaultdict

import numpy as np
import pytest

import _instances as I
from _cases import sim_lib
from test_kernel_sums import (BLOCK, GRID_BIG, R_ACCEPT, R_DIR, R_TRIAL, TAIL_GROUP, Booth, Data, Quad, Rosen, User, _make_objective,
                              bits, exact_period, expected_cg, grid_cg, launch_inputs, npts_for, rosen_valley_period, row_width)

ADT = R_ACCEPT | R_DIR | R_TRIAL
NSUMS, MAXP, PIPE_RING = 56, 7, 64
KS = (1, 2, 3, 5, 7)                                       # trial steps: padding points at every width
WIDTHS = (10, 24, 40, 56)
ON = {Quad: "ObjQuadDiag", Rosen: "ObjRosenPaired", Booth: "ObjBooth", User: "UserObjective"}
N_TWO_LEVEL = 2 * 512 * 65 + 1                             # 65 workgroups: both levels of the fused tail, k_finalize_t in between
N_HBM = (2 * (GRID_BIG * 8 + 1) + 1, 2 * (GRID_BIG + 5) + 1)
SIZES_SMALL = (1, 2, 3, 17, 127, 128, 129, 511, 512, 513)
TAILS = {"fused": dict(fused_tail=True), "finalize": dict(fused_tail=False), "strict": dict(strict_tail=True)}
BIG_MAX_ITERS = 1 << 40

REACHED = set()
CELLS = defaultdict(int)                                   # (symbols, n, form) cells checked bit for bit
TABLE_ROWS_ON_DEVICE = [0]


# ---- the controller's blocks (csrc/cgo_ctl.hpp) and the host-compiled ctl_step ----------------------------------------------
def _structs():
    from cgo_amd import _lib

    class CtlConfigC(C.Structure):
        _fields_ = [("ls", _lib.LSConfigC), ("eps", C.c_double), ("mu", C.c_double), ("beta_kind", C.c_int32), ("maxp", C.c_int32),
                    ("max_iters", C.c_int64)]
    return _lib, CtlConfigC


_HOST = []


def host():
    """(library, CtlConfigC): sim_ctl_step bound, the struct sizes checked against the C++ side."""
    if not _HOST:
        _lib, CtlConfigC = _structs()
        L = sim_lib()
        L.sim_ctl_step.restype = C.c_int
        L.sim_ctl_step.argtypes = [C.POINTER(CtlConfigC), C.POINTER(_lib.CtlStateC), _lib.dp, C.POINTER(_lib.CtlRecordC)]
        L.sim_ctl_sizes.restype = None
        L.sim_ctl_sizes.argtypes = [_lib.i64p]
        sz = (C.c_int64 * 3)()
        L.sim_ctl_sizes(sz)
        assert list(sz) == [C.sizeof(CtlConfigC), C.sizeof(_lib.CtlStateC), C.sizeof(_lib.CtlRecordC)] and sz[2] == 8 * 67
        _HOST.append((L, _lib, CtlConfigC))
    return _HOST[0]


def make_config(ls, beta, maxp, eps, max_iters):
    """CtlConfig as the engine fills it (cgo_engine.cpp): the solver's line search, β kind and μ, the launch's row layout."""
    L, _lib, CtlConfigC = host()
    b = beta._c()
    return CtlConfigC(ls._c(), float(eps), b.mu, b.kind, int(maxp), int(max_iters))


def make_state(st):
    L, _lib, _ = host()
    a = [float(v) for v in st["a"]]
    s = _lib.CtlStateC()
    s.f_x, s.gg, s.a_acc, s.beta = float(st["f_x"]), float(st["gg"]), float(st["a_acc"]), float(st["beta"])
    s.a[:] = a + [a[-1]] * (MAXP - len(a))
    s.npts, s.go, s.it = int(st.get("npts", len(a))), int(st.get("go", 1)), int(st.get("it", 0))
    return s


def host_round(cfg, s, row):
    """One round on the host: ctl_step where the controller runs, the idle record where it has stopped (tail_ctl_idle / the
    go == 0 branch of k_finalize_ctl: zero record, npts = −1, state untouched).  Advances `s`; returns the record."""
    L, _lib, _ = host()
    rec = _lib.CtlRecordC()
    if s.go == 0:
        rec.npts = -1
        return rec
    r = np.zeros(NSUMS)
    r[:len(row)] = row
    L.sim_ctl_step(C.byref(cfg), C.byref(s), r.ctypes.data_as(_lib.dp), C.byref(rec))
    return rec


def args_bytes(s):
    _, _lib, _ = host()
    a = _lib.CtlArgsC(s.a_acc, s.beta, s.a, s.go)
    return bytes(a)


def state_dict(s):
    return dict(f_x=s.f_x, gg=s.gg, a_acc=s.a_acc, beta=s.beta, a=list(s.a), npts=s.npts, go=s.go, it=s.it)


# ---- configurations -----------------------------------------------------------------------------------------------------
def betas(cgo):
    return {"HagerZhang": cgo.HagerZhang(), "YuanWangSheng": cgo.YuanWangSheng(0.1), "SallehAlhawarat": cgo.SallehAlhawarat(),
            "LiuStorrey": cgo.LiuStorrey(), "PolakRibiere": cgo.PolakRibiere(), "HestenesStiefel": cgo.HestenesStiefel(),
            "DaiYuan": cgo.DaiYuan(), "BroydenFamily": cgo.BroydenFamily(0.5)}


def line_searches(cgo):
    return {"SW": cgo.StrongWolfeBisection(1e-4, 0.9, 2.0, 1000, 100),
            "WB": cgo.WolfeBisection(cgo.Wolfe(1e-4, 0.9), 100, 10.0, 20),
            "WB-short": cgo.WolfeBisection(cgo.Wolfe(1e-4, 0.9), 100, 0.25, 20),      # max_step_size 0.25: first step 0.125 after a_acc = 0
            "WB-1.5": cgo.WolfeBisection(cgo.Wolfe(1e-4, 0.9), 100, 1.5, 20),
            "WB-inf": cgo.WolfeBisection(cgo.Wolfe(1e-4, 0.9), 100, math.inf, 20),
            "WB-nan": cgo.WolfeBisection(cgo.Wolfe(1e-4, 0.9), 100, math.nan, 20),
            "WB-kat": cgo.WolfeBisection(cgo.Wolfe(0.25, 0.5), 100, 10.0, 20),
            "YWL": cgo.WolfeBisection(cgo.YuanWeiLuWolfe(1e-4, 0.9, 1e-5), 100, 10.0, 20),
            "YWL-kat": cgo.WolfeBisection(cgo.YuanWeiLuWolfe(0.25, 0.5, 0.125), 100, 10.0, 20),
            "BT": cgo.Backtracking(cgo.Armijo(1e-4), 0.5, 100, 20)}


def _solver(cgo, obj, tail, beta, ls, points, big=False, depth=4):
    pol = cgo.SolverPolicy(resident=False, controller_depth=depth, points=points, hbm_stream_bytes=1.0 if big else None, **TAILS[tail])
    cfg = cgo.setupCGConfig(1e-9, beta, cgo.DisableTrace(), max_iters=5)
    return cgo.Solver(obj, cfg, ls, pol)


def expected_symbols(obj, p, n, tail, big):
    """What one round launches (pipe_round_kernels): ONE armed launch where the fused tail applies (built-in objective, at most
    1024 workgroups, never pure-HBM), else the plain launch, k_finalize_t above 64 rows, k_finalize_ctl."""
    grid = GRID_BIG if big else grid_cg(n, p)
    if tail != "finalize" and obj is not User and not big and grid <= 1024:
        return [f"k_cg_armed<{ON[obj]}, {p}>"]
    W = row_width(p)
    mid = [f"k_finalize_t<{W}>"] if grid > TAIL_GROUP else []
    return [f"k_cg<{ON[obj]}, {ADT}, {p}, {'true' if big else 'false'}>"] + mid + [f"k_finalize_ctl<{W}>"]


def test_line_search_configs_pass_the_library_validation(cgo):
    """CPU tier: every line-search configuration of this module passes the check that creating a solver applies (the reference's
    @asserts: wolfe.jl:233,278, nocedal.jl:22-26), so a case list cannot fail at solver creation on the GPU only."""
    from cgo_amd import _lib
    for name, ls in line_searches(cgo).items():
        c = ls._c()
        assert _lib.lib().cgo_check_ls_config(C.byref(c)) == 0, (name, _lib.lib().cgo_last_error())


def test_geometry_of_the_sizes():
    """CPU tier: the sizes reach the edges they are here for."""
    assert grid_cg(N_TWO_LEVEL, 1) == 65 == grid_cg(N_TWO_LEVEL, 7) and grid_cg(N_TWO_LEVEL - 1, 7) == 65 and grid_cg(513, 7) == 1
    assert grid_cg(2 * 512 * 64, 7) == 64 and TAIL_GROUP == 64 and BLOCK == 256
    assert expected_symbols(Quad, 7, N_TWO_LEVEL, "finalize", False) == ["k_cg<ObjQuadDiag, 7, 7, false>", "k_finalize_t<56>", "k_finalize_ctl<56>"]
    assert expected_symbols(Booth, 3, 2, "finalize", False) == ["k_cg<ObjBooth, 7, 3, false>", "k_finalize_ctl<24>"]
    assert expected_symbols(Quad, 7, 17, "strict", False) == ["k_cg_armed<ObjQuadDiag, 7>"]


# ---- (a) + (b): one round, exact data ------------------------------------------------------------------------------------
# Steps for (b): the step the line search asks for first (ls_first_step of a_acc) comes first, so that a single-point launch can
# be accepted at all.  Quad / user / Booth: a_acc = 0.5 as in tests/test_kernel_sums.py; the quartic runs on its valley data with
# a_acc = β = 0 (its budget), where the Wolfe bisection with max_step_size = 0.25 starts at min(1, 0.25 / 2) = 0.125.
B_STEPS = {"quad_diag": [0.5, 0.25, 0.75, 1.0, 1.25, 1.5, 1.75], "user_quad": [0.5, 0.25, 0.75, 1.0, 1.25, 1.5, 1.75],
           "booth": [0.5, 0.25, 0.75, 1.0, 1.25, 1.5, 1.75], "rosenbrock_paired": [0.125 * (j + 1) for j in range(7)]}
VARIANTS = {   # f_x, eps, max_iters − it: both outcomes (the reference decides which; the tests assert that both occur)
    "go": (2.0 ** 40, 1e-30, BIG_MAX_ITERS), "eps": (2.0 ** 40, 1e300, BIG_MAX_ITERS), "last": (2.0 ** 40, 1e-30, 1),
    "high": (-2.0 ** 40, 1e-30, BIG_MAX_ITERS)}


def round_inputs(obj, n, k, beta0=False):
    """(data, state scalars, steps) of one exact round: the recipe of test_kernel_sums' accept + direction + trial launch; with
    beta0 the direction is −∇f (β = 0: g·u < 0 whatever the data) and the steps are B_STEPS."""
    d, a_acc, beta = launch_inputs(obj.name, ADT, n)
    if beta0:
        return d, a_acc, 0.0, B_STEPS[obj.name][:k]
    from test_kernel_sums import STEPS
    return d, a_acc, beta, STEPS[obj.name][:k]


_EXP = {}


def exact_round(obj, n, k, beta0=False):
    key = (obj.name, n, k, beta0)
    if key not in _EXP:
        d, a_acc, beta, a = round_inputs(obj, n, k, beta0)
        _EXP[key] = expected_cg(obj, d, ADT, a, a_acc, beta)
    return _EXP[key]


def check_round(tag, got, want_row, want_vec, cfg, st_in, round0, mism):
    """One probed round against the exact row and the host-compiled decision.  True where everything matched."""
    L, _lib, _ = host()
    rec = got["records"][0]
    W = want_row.size
    ok = True

    def bad(msg):
        nonlocal ok
        ok = False
        mism.append(f"{tag}: {msg}")
    if got["width"] != W:
        bad(f"row width {got['width']}, expected {W}")
        return False, None
    if not np.array_equal(bits(rec["sums"][:W]), bits(want_row)):
        i = np.nonzero(bits(rec["sums"][:W]) != bits(want_row))[0]
        bad(f"record sums differ in slots {i[:12].tolist()}: got {rec['sums'][i[:4]].tolist()} want {want_row[i[:4]].tolist()}")
    if np.any(bits(rec["sums"][W:]) != 0):
        bad(f"record slots behind the row are not +0.0: {np.nonzero(bits(rec['sums'][W:]))[0][:8].tolist()}")
    if not np.array_equal(bits(got["out_dev"][:W]), bits(want_row)):
        bad("the device copy of the row (out_dev) differs from the exact row")
    for key in ("x", "u"):
        if not np.array_equal(bits(got[key]), bits(want_vec[key])):
            i = int(np.nonzero(bits(got[key]) != bits(want_vec[key]))[0][0])
            bad(f"{key} differs first at element {i}: got {got[key][i]!r}, want {want_vec[key][i]!r}")
    s = make_state(st_in)
    echo = (s.a_acc, s.beta, list(s.a), s.npts)
    if not (bits(rec["a_acc"]) == bits(echo[0]) and bits(rec["beta"]) == bits(echo[1]) and np.array_equal(bits(rec["a"]), bits(echo[2]))
            and rec["npts"] == echo[3]):
        bad(f"the record does not echo the state it ran with: a_acc {rec['a_acc']} beta {rec['beta']} a {rec['a']} npts {rec['npts']}")
    want_rec = host_round(cfg, s, want_row)
    if rec["accepted"] != want_rec.accepted:
        bad(f"accepted = {rec['accepted']}, the host-compiled ctl_step says {want_rec.accepted}")
    if rec["bytes"] != bytes(want_rec):
        bad("the record differs from the host-compiled ctl_step's, byte for byte")
    if got["st"]["bytes"] != bytes(s):
        bad(f"CtlState after the round differs from the host's: device {dict((k, v) for k, v in got['st'].items() if k != 'bytes')}, host {state_dict(s)}")
    if got["args"]["bytes"] != args_bytes(s):
        bad("the argument block after the round is not the host state's (a_acc, beta, a, go)")
    if round0 is not None and got["round"] != round0 + 1:
        bad(f"round counter {got['round']}, expected {round0 + 1}")
    return ok, want_rec.accepted


def run_rounds(cgo, contexts, obj, n, tail, big, ks=KS, beta="PolakRibiere", ls="SW", variants=("go",), beta0=False, outcomes=None):
    """Every k of `ks` (one solver per point count) × `variants`, one round each."""
    mism = []
    d = round_inputs(obj, n, 1, beta0)[0]
    o = _make_objective(cgo, obj, n, contexts[tail], d)
    B, LS = betas(cgo)[beta], line_searches(cgo)[ls]
    try:
        for p in sorted({npts_for(k) for k in ks}):
            s = _solver(cgo, o, tail, B, LS, p, big)
            round0 = None
            try:
                for k in [k for k in ks if npts_for(k) == p]:
                    _, a_acc, b, a = round_inputs(obj, n, k, beta0)
                    want_row, want_vec = exact_round(obj, n, k, beta0)
                    for v in variants:
                        f_x, eps, left = VARIANTS[v]
                        st = dict(f_x=f_x, gg=3.0, a_acc=a_acc, beta=b, a=a, it=3)
                        cfg = make_config(LS, B, p, eps, 3 + left)
                        got = s.probe_armed(st, 1, "rounds", d.full["x"], d.full["u"], max_iters=3 + left, eps=eps)
                        REACHED.update(got["symbols"])
                        tag = f"{obj.name} n={n} {tail}{' pure-HBM' if big else ''} k={k} {beta}/{ls}/{v} [{' + '.join(got['symbols'])}]"
                        if got["symbols"] != expected_symbols(obj, p, n, tail, big):
                            mism.append(f"{tag}: expected {expected_symbols(obj, p, n, tail, big)}")
                        ok, acc = check_round(tag, got, want_row, want_vec, cfg, st, round0, mism)
                        round0 = got["round"]
                        if ok:
                            CELLS[(tuple(got["symbols"]), n, tail)] += 1
                        if outcomes is not None:
                            outcomes[beta].add(acc)
            finally:
                s.close()
    finally:
        o.close()
    return mism


def _report(mism):
    assert not mism, f"{len(mism)} round(s) differ:\n" + "\n".join(mism[:20])


@pytest.fixture(scope="module")
def contexts(cgo):
    out = {name: cgo.Context(0) for name in TAILS}
    yield out
    for c in out.values():
        c.close()


def sizes_for(obj):
    if obj is Booth:
        return [2]
    if obj is Rosen:   # pairs only: the even sizes, and the even neighbour of the two-level size
        return [n for n in SIZES_SMALL if n % 2 == 0] + [N_TWO_LEVEL + 1]
    if obj is User:    # one run-time compiled module per objective: fewer sizes (as in test_kernel_sums)
        return [17, 513, N_TWO_LEVEL]
    return list(SIZES_SMALL) + [N_TWO_LEVEL]


def hbm_sizes_for(obj):
    return [] if obj is Booth else [n + (n & 1 if obj is Rosen else 0) for n in N_HBM]


def test_exact_rounds_meet_their_preconditions():
    """CPU tier: the exact data stay exact and order-independent for every round of (a) and (b) (expected_cg asserts it), at the
    largest and smallest sizes of each objective."""
    for obj in (Quad, Rosen, Booth):
        ns = sizes_for(obj) + hbm_sizes_for(obj)
        for n in sorted(set(ns[:2] + ns[-3:])):
            for k in KS:
                exact_round(obj, n, k)
                exact_round(obj, n, k, beta0=True)


A_CASES = [(obj, n) for obj in (Quad, Rosen, Booth, User) for n in sizes_for(obj)]


@pytest.mark.gpu
@pytest.mark.parametrize("obj,n", A_CASES, ids=[f"{o.name}-n{n}" for o, n in A_CASES])
def test_one_round_exact_every_word(cgo, contexts, obj, n):
    """(a) + (b) on the data of (a): k_cg_armed under the default and the strict tail, the un-fused round (one or two reduction
    launches by size); every slot, x, u, the echo, and the decision against the host-compiled ctl_step."""
    mism = []
    for tail in TAILS:
        mism += run_rounds(cgo, contexts, obj, n, tail, False)
    _report(mism)


H_CASES = [(obj, n) for obj in (Quad, Rosen, User) for n in hbm_sizes_for(obj)]


@pytest.mark.gpu
@pytest.mark.parametrize("obj,n", H_CASES, ids=[f"{o.name}-n{n}" for o, n in H_CASES])
def test_one_pure_hbm_round_exact_every_word(cgo, contexts, obj, n):
    """hbm_stream_bytes = 1: k_cg<…, true> on 4096 chunks, k_finalize_t, k_finalize_ctl."""
    _report(run_rounds(cgo, contexts, obj, n, "fused", True))


B_FORMS = {"armed": ("fused", False, 17), "armed-strict": ("strict", False, 17), "ctl": ("finalize", False, 17),
           "t+ctl": ("finalize", False, N_TWO_LEVEL), "pure-HBM": ("fused", True, N_HBM[1])}
B_LS = ("SW", "WB", "YWL", "BT")


def _b_outcomes_on_the_host(cgo, forms=("armed",)):
    """The decisions of (b)'s case list as the host-compiled ctl_step takes them on the exact rows: β flavour → outcomes."""
    out = defaultdict(set)
    B, LSS = betas(cgo), line_searches(cgo)
    for form in forms:
        tail, big, n = B_FORMS[form]
        for beta in B:
            for ls in B_LS:
                for k in (1, 3, 7):
                    _, a_acc, b, a = round_inputs(Quad, n, k, True)
                    row = exact_round(Quad, n, k, True)[0]
                    for f_x, eps, left in VARIANTS.values():
                        s = make_state(dict(f_x=f_x, gg=3.0, a_acc=a_acc, beta=b, a=a, it=3))
                        rec = host_round(make_config(LSS[ls], B[beta], npts_for(k), eps, 3 + left), s, row)
                        out[beta].add(rec.accepted)
                        assert not (ls == "BT" and rec.accepted), "Backtracking can never be accepted by the controller"
    return out


def test_decision_cases_hold_both_outcomes_for_every_flavour(cgo):
    """CPU tier: on the reference, (b)'s case list contains accepted and stopped rounds for every β flavour."""
    out = _b_outcomes_on_the_host(cgo, tuple(B_FORMS))
    assert set(out) == set(betas(cgo)) and all(v == {0, 1} for v in out.values()), dict(out)


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(B_FORMS))
def test_decision_and_next_state_every_flavour(cgo, contexts, form):
    """(b): all seven β flavours and Broyden × StrongWolfeBisection, WolfeBisection (Wolfe and Yuan–Wei–Lu), Backtracking × four
    (f_x, eps, max_iters) variants at one size per form of a round; the quartic under the Wolfe bisection as well."""
    tail, big, n = B_FORMS[form]
    mism, outcomes = [], defaultdict(set)
    for beta in betas(cgo):
        for ls in B_LS:
            mism += run_rounds(cgo, contexts, Quad, n, tail, big, ks=(1, 3, 7), beta=beta, ls=ls, variants=tuple(VARIANTS), beta0=True,
                               outcomes=outcomes)
    nr = n + (n & 1)
    for ls in ("SW", "WB-short"):
        mism += run_rounds(cgo, contexts, Rosen, nr, tail, big, ks=(1, 3), beta="HagerZhang", ls=ls, variants=("go", "last"), beta0=True)
    if not big:
        mism += run_rounds(cgo, contexts, Booth, 2, tail, big, ks=(2, 5), beta="DaiYuan", ls="WB", variants=("go", "high"), beta0=True)
    _report(mism)
    assert all(v == {0, 1} for v in outcomes.values()), dict(outcomes)


# ---- (c) the decision table ------------------------------------------------------------------------------------------------
# Base numbers: ϕ₀ = f_x = 10, dϕ₀ = g·u = −8, c1 = 1e-4, c2 = 0.9: a trial is "too high" above 10 − 8e-4·a, the strong curvature
# test passes for |dϕ| ≤ 7.2, the weak one for dϕ ≥ −7.2.  Points are (step, ϕ, dϕ[, overrides of the other sums]).
OK, SHORT, HIGH = (5.0, 1.0), (5.0, -8.0), (20.0, 0.0)   # accepted | curvature fails, dϕ < 0 (step too short) | too high
TINY, HUGE = 5e-324, 1.5e308


def _case(name, pts, accepted, idx=None, ls="SW", beta="PolakRibiere", why="", **kw):
    d = dict(name=name, pts=[(p[0], p[1], p[2], p[3] if len(p) > 3 else {}) for p in pts], accepted=accepted, idx=idx, ls=ls, beta=beta,
             why=why, f_x=10.0, gg=4.0, a_acc=1.0, beta_in=0.5, it=3, go=1, gu=-8.0, uu=4.0, eps=1e-9, max_iters=1000)
    d.update(kw)
    assert (idx is not None) == bool(accepted) or kw.get("go") == 0
    return d


def _norm_threshold(eps):
    """the smallest Σ g⁺² whose square root reaches eps·(1 + 1e-9), and its predecessor"""
    thr = eps * (1.0 + 1e-9)
    g = thr * thr
    while math.sqrt(g) >= thr:
        g = math.nextafter(g, 0.0)
    while math.sqrt(g) < thr:
        g = math.nextafter(g, math.inf)
    return g, math.nextafter(g, 0.0)


def decision_table():
    T = []
    fill = lambda j: (100.0 + j, 99.0 + j, 98.0 + j)   # a point no search asks for
    # success at every index: through extrapolation (1 → 1.5) and through zoom (1 too high → 0.5)
    for idx in range(MAXP):
        for kind, first, second in (("extrapolation", (1.0, *SHORT), (1.5, 3.0, 1.0)), ("zoom", (1.0, *HIGH), (0.5, 6.0, 1.0))):
            n = max(idx + 1, 2)
            pts = [fill(j) for j in range(n)]
            pts[idx] = second
            pts[1 if idx == 0 else 0] = first
            T.append(_case(f"{kind}-lands-on-{idx}", pts, 1, idx, why=f"second step of the search sits at index {idx}"))
    T.append(_case("first-trial", [(1.0, *OK)], 1, 0, why="nocedal.jl:78-110 at its first trial"))
    # the speculation tree in its own order: a0, h0, h1, g0, g1, q0, q1 = 1, 1/2, 3/2, 3/4, 5/4, 7/8, 9/8
    T.append(_case("zoom-two-levels", [(1.0, *HIGH), (0.5, 6.0, -8.0), fill(2), (0.75, 5.5, 1.0)], 1, 3, why="zoom: lo moves once"))
    T.append(_case("extrapolate-then-zoom", [(1.0, *SHORT), fill(1), (1.5, *HIGH), fill(3), (1.25, 4.0, 1.0)], 1, 4, why="zoom(a_prev, a)"))
    T.append(_case("zoom-run-lo", [(1.0, *HIGH), (0.5, 6.0, -8.0), fill(2), (0.75, 5.5, -8.0), fill(4), (0.875, 5.25, 1.0)], 1, 5,
                   why="run_lo ≥ 2: the third midpoint of a run of the lower bound"))
    T.append(_case("extrapolate-zoom-hi", [(1.0, *SHORT), fill(1), (1.5, *HIGH), fill(3), (1.25, *HIGH), fill(5), (1.125, 4.0, 1.0)], 1, 6,
                   why="zoom: hi moves, then the quarter next to a0"))
    T.append(_case("zoom-run-hi", [(1.0, *HIGH), (0.5, *HIGH), (0.25, *HIGH), (0.125, 6.0, 1.0)], 1, 3, why="run_hi ≥ 2"))
    T.append(_case("extrapolation-k3", [(1.0, *SHORT), (1.5, 4.5, -8.0), (2.25, 4.0, -8.0), (3.375, 3.5, 1.0)], 1, 3, why="k ≥ 3: a monotone run of extrapolations"))
    T.append(_case("not-lower", [(1.0, *SHORT), (1.5, 5.0, 1.0), (1.25, 4.0, 1.0)], 1, 2, why="ϕ ≥ ϕ_prev at k > 0 → zoom(a_prev, a)"))
    T.append(_case("dphi-positive", [(1.0, 5.0, 8.0), (0.5, 4.0, 1.0)], 1, 1, why="dϕ ≥ 0 → zoom(a, a_prev)"))
    T.append(_case("miss-zoom", [(1.0, *HIGH)], 0, why="the zoom asks for 1/2, which was not launched"))
    T.append(_case("miss-with-three-points", [(1.0, *HIGH), (0.75, *OK), (1.5, *OK)], 0, why="neither candidate is the step asked for"))
    T.append(_case("miss-first-step", [(0.75, *OK)], 0, why="the first step (a_acc = 1) was not launched"))
    T.append(_case("non-descent", [(1.0, *OK)], 0, gu=1.0, why="dϕ₀ > 0"))
    T.append(_case("non-descent-wolfe", [(1.0, *OK)], 0, ls="WB", gu=1.0, why="dϕ₀ > 0"))
    T.append(_case("d0-zero", [(1.0, 5.0, 0.0)], 1, 0, gu=0.0, why="dϕ₀ = 0 is not > 0: the search runs"))
    T.append(_case("phi0-inf-wolfe", [(1.0, *OK)], 0, ls="WB", f_x=math.inf, why="wolfe.jl: non-finite ϕ₀"))
    T.append(_case("phi0-nan-wolfe", [(1.0, *OK)], 0, ls="WB", f_x=math.nan, why="wolfe.jl: non-finite ϕ₀"))
    T.append(_case("phi0-nan-strong", [(1.0, *OK)], 1, 0, f_x=math.nan, why="nocedal.jl has no such test: every comparison with NaN is false, the curvature test passes"))
    T.append(_case("f-nan", [(1.0, math.nan, 1.0)], 0, why=":success on comparisons with NaN, then optim.jl:108-121: f not finite"))
    T.append(_case("f-neg-inf", [(1.0, -math.inf, 1.0)], 0, why=":success, f not finite"))
    T.append(_case("f-pos-inf", [(1.0, math.inf, 1.0)], 0, why="too high → zoom → miss"))
    T.append(_case("f-pos-inf-zoom-hit", [(1.0, math.inf, 1.0), (0.5, 6.0, 1.0)], 1, 1, why="too high → zoom lands on a finite point"))
    T.append(_case("dphi-nan", [(1.0, 5.0, math.nan)], 0, why="neither test holds for NaN → extrapolation → miss"))
    T.append(_case("dphi-nan-then-hit", [(1.0, 5.0, math.nan), (1.5, 3.0, 1.0)], 1, 1, why="NaN at a point the search leaves behind does not stop it"))
    T.append(_case("dphi-pos-inf", [(1.0, 5.0, math.inf)], 0, why="dϕ ≥ 0 → zoom → miss"))
    T.append(_case("dphi-neg-inf", [(1.0, 5.0, -math.inf)], 0, why="extrapolation → miss"))
    for nm, g, acc in (("gtgt-low-inside", 1e-280, 1), ("gtgt-low-outside", math.nextafter(1e-280, 0.0), 0), ("gtgt-high-inside", 1e300, 1),
                       ("gtgt-high-outside", math.nextafter(1e300, math.inf), 0), ("gtgt-nan", math.nan, 0), ("gtgt-zero", 0.0, 0)):
        T.append(_case(nm, [(1.0, 5.0, 1.0, dict(gtgt=g))], acc, 0 if acc else None, eps=1e-200, why="Σ g⁺² against [1e-280, 1e300]: the scaled norm is the host's"))
    g_hi, g_lo = _norm_threshold(0.5)
    T.append(_case("norm-at-threshold", [(1.0, 5.0, 1.0, dict(gtgt=g_hi))], 1, 0, eps=0.5, why="‖g⁺‖ ≥ ϵ(1 + 1e-9)"))
    T.append(_case("norm-below-threshold", [(1.0, 5.0, 1.0, dict(gtgt=g_lo))], 0, eps=0.5, why="‖g⁺‖ one ulp of Σ below ϵ(1 + 1e-9): the stop test is the host's"))
    T.append(_case("last-iteration", [(1.0, *OK)], 0, max_iters=4, why="it + 1 == max_iters"))
    T.append(_case("one-before-last", [(1.0, *OK)], 1, 0, max_iters=5, why="it + 1 < max_iters"))
    T.append(_case("a-next-nan", [(1.0, *OK)], 0, ls="WB-nan", why="max_step_size = NaN: the first step and a_next are NaN"))
    T.append(_case("yws-in-range", [(1.0, *OK)], 1, 0, beta="YuanWangSheng", why="both norms from Σ"))
    T.append(_case("yws-uu-out-of-range", [(1.0, *OK)], 0, beta="YuanWangSheng", uu=1e-290, why="norm(u) needs the scaled form"))
    T.append(_case("yws-yy-out-of-range", [(1.0, 5.0, 1.0, dict(yy=1e301))], 0, beta="YuanWangSheng", why="norm(y) needs the scaled form"))
    T.append(_case("pr-uu-out-of-range", [(1.0, *OK)], 1, 0, uu=1e-290, why="Polak–Ribière reads no norm"))
    T.append(_case("sa-in-range", [(1.0, *OK)], 1, 0, beta="SallehAlhawarat", why="norm(g⁺) from Σ"))
    T.append(_case("sa-gtgt-out-of-range", [(1.0, 5.0, 1.0, dict(gtgt=1e301))], 0, beta="SallehAlhawarat", why="norm(g⁺) needs the scaled form"))
    T.append(_case("wolfe-first-trial", [(1.0, *OK)], 1, 0, ls="WB", why="wolfe.jl:51-78 at its first trial"))
    T.append(_case("wolfe-shrink", [(1.0, *HIGH), (0.5, *OK)], 1, 1, ls="WB", why="step too long → (lb + ub)/2"))
    T.append(_case("wolfe-double", [(1.0, *SHORT), (0.5, *HIGH), (2.0, *OK)], 1, 2, ls="WB", why="step too short, ub = ∞ → 2a"))
    T.append(_case("wolfe-max-step", [(1.0, *SHORT), (2.0, *OK)], 0, ls="WB-1.5", why="2a > max_step_size"))
    T.append(_case("wolfe-collapse", [(TINY, *HIGH)], 0, ls="WB", a_acc=TINY, why="(0 + 5e-324)/2 = 0: the bracket collapsed, vector work is the host's"))
    T.append(_case("wolfe-halving", [(1.0, math.inf, 0.0), (0.5, *OK)], 1, 1, ls="WB", why="findfeasiblestepsize! halves past a non-finite ϕ"))
    T.append(_case("wolfe-halving-dphi", [(1.0, 5.0, math.nan), (0.5, *OK)], 1, 1, ls="WB", why="… and past a non-finite dϕ"))
    T.append(_case("wolfe-halving-miss", [(1.0, math.inf, 0.0), (2.0, *OK)], 0, ls="WB", why="the halved step was not launched"))
    kat = dict(a_acc=0.5, uu=25.0)   # tests/test_abi.py::test_condition_evaluators_kats: YWL bounds 9.5 / −3, Wolfe 9 / −4
    T.append(_case("ywl-accepts", [(0.5, 9.25, -2.0)], 1, 0, ls="YWL-kat", why="9.25 ≤ 9.5 and −2 ≥ −3", **kat))
    T.append(_case("wolfe-rejects-the-same", [(0.5, 9.25, -2.0)], 0, ls="WB-kat", why="9.25 > 9: too long → 1/4 not launched", **kat))
    T.append(_case("ywl-too-short", [(0.5, 9.25, -3.5)], 0, ls="YWL-kat", why="−3.5 < −3 → 2a not launched", **kat))
    T.append(_case("ywl-uu-matters", [(0.5, 9.25, -2.0)], 0, ls="YWL-kat", a_acc=0.5, uu=1.0, why="min(1, c1·a·uu/2 = 1/16): 9.25 > 9.03125"))
    # trial points of the NEXT search from a denormal and from a huge accepted step: zero and duplicate candidates, overflow
    for ls in ("SW", "WB-inf"):
        T.append(_case(f"next-points-from-denormal-{ls}", [(TINY, *OK)], 1, 0, ls=ls, a_acc=TINY, why="(0 + a)/2 = 0 and a duplicate of 2a among the candidates"))
        T.append(_case(f"next-points-from-huge-{ls}", [(HUGE, 5.0, 0.0)], 1, 0, ls=ls, a_acc=HUGE, gu=-1e-310, why="candidates overflow to ∞"))
    T.append(_case("stopped", [(1.0, *OK)], 0, go=0, why="go == 0: the round is idle"))
    T.append(_case("backtracking", [(1.0, *OK)], 0, ls="BT", why="the controller runs the two bisection searches only"))
    return T


def table_row(c, maxp):
    """(state dict, 56-slot row) of a table case for a launch of `maxp` points; None where the case needs more points."""
    pts = c["pts"]
    if len(pts) > maxp:
        return None
    row = np.zeros(NSUMS)
    for j in range(maxp):
        step, f, gtu, ov = pts[min(j, len(pts) - 1)]   # a launch evaluates its full row: padding points repeat the last one
        v = dict(gtgt=4.0, gtg=1.0, yy=2.0, uy=-3.0, ygt=1.5)
        v.update(ov)
        row[7 * j:7 * j + 7] = [f, gtu, v["gtgt"], v["gtg"], v["yy"], v["uy"], v["ygt"]]
    row[7 * maxp], row[7 * maxp + 1] = c["gu"], c["uu"]
    st = dict(f_x=c["f_x"], gg=c["gg"], a_acc=c["a_acc"], beta=c["beta_in"], a=[p[0] for p in pts], it=c["it"], go=c["go"])
    return st, row


def tree_points(ls, a0, maxp):
    """The steps a launch of `maxp` points evaluates for a line search starting at a0, from the comments of ls_first_hints and
    ls_trial_points_n: the zoom midpoint (0 + a0)/2 and the extrapolation (a0·growth + a0)/2 (Wolfe bisection: 2·a0); five points
    add the grandchild on a0's side under each, seven one more level; only distinct, finite, positive candidates, in that order."""
    c = ls._c()
    h0 = (0.0 + a0) / 2
    h1 = (a0 * c.a_max_growth_factor + a0) / 2 if c.kind == 0 else 2.0 * a0
    g0, g1 = (h0 + a0) / 2, (a0 + h1) / 2
    q0, q1 = (g0 + a0) / 2, (a0 + g1) / 2
    cands = {1: [], 3: [h0, h1], 5: [h0, h1, g0, g1], 7: [h0, h1, g0, g1, q0, q1]}[maxp]
    pts = [a0]
    for v in cands:
        if len(pts) < maxp and math.isfinite(v) and v > 0.0 and v not in pts:
            pts.append(v)
    return pts


def first_step(ls, a):
    c = ls._c()
    if c.kind == 0:
        return a if (0.0 < a and math.isfinite(a)) else 1.0
    return a if (c.max_step_size > a and a > 0.0) else min(1.0, c.max_step_size / 2)


def test_decision_table_on_the_host(cgo):
    """CPU tier: the host-compiled ctl_step takes the table's hand-stated decisions at every width a case fits, lands on the stated
    point, and arms the next launch with the trial points of the tree above; a stopped or refusing round leaves go = 0 and the
    rest of the state alone.  The table reaches every exit it claims."""
    T = decision_table()
    B, LSS = betas(cgo), line_searches(cgo)
    names = [c["name"] for c in T]
    assert len(set(names)) == len(names)
    landed = defaultdict(set)
    checked = 0
    for c in T:
        for maxp in (1, 3, 5, 7):
            tr = table_row(c, maxp)
            if tr is None:
                continue
            st, row = tr
            ls = LSS[c["ls"]]
            cfg = make_config(ls, B[c["beta"]], maxp, c["eps"], c["max_iters"])
            s = make_state(st)
            before = bytes(s)
            rec = host_round(cfg, s, row)
            tag = f"{c['name']} maxp={maxp} ({c['why']})"
            assert rec.accepted == c["accepted"], tag
            checked += 1
            if c["go"] == 0:
                assert rec.npts == -1 and bytes(s) == before and not any(rec.sums) and rec.a_acc == 0.0, tag
                continue
            assert np.array_equal(bits(np.array(rec.sums[:])), bits(row)) and rec.npts == len(c["pts"]), tag
            assert bits(rec.a_acc) == bits(st["a_acc"]) and bits(rec.beta) == bits(st["beta"]), tag
            if not c["accepted"]:
                after = make_state(st)
                after.go = 0
                assert bytes(s) == bytes(after), tag + ": a refusing round changes nothing but go"
                continue
            step, f, gtu, ov = c["pts"][c["idx"]]
            landed[c["ls"][:2]].add(c["idx"])
            assert s.go == 1 and s.it == c["it"] + 1 and bits(s.a_acc) == bits(step) and bits(s.f_x) == bits(f) and s.gg == ov.get("gtgt", 4.0), tag
            want = tree_points(ls, first_step(ls, step), maxp)
            assert s.npts == len(want) and list(s.a) == want + [want[-1]] * (MAXP - len(want)), f"{tag}: next points {list(s.a)}, tree {want}"
            if c["beta"] == "PolakRibiere":
                assert s.beta == ov.get("ygt", 1.5) / c["gg"], tag
    assert landed["SW"] == set(range(MAXP)) and {0, 1, 2} <= landed["WB"] | landed["YW"]
    for maxp, ls, a, want in ((7, "SW", TINY, [TINY, 2 * TINY]), (7, "WB-inf", TINY, [TINY, 2 * TINY]), (3, "SW", HUGE, [HUGE, HUGE / 2]),
                              (7, "WB-inf", HUGE, [HUGE, HUGE / 2]), (7, "SW", 1.0, [1, .5, 1.5, .75, 1.25, .875, 1.125])):
        assert tree_points(LSS[ls], a, maxp) == want, (maxp, ls, a)   # zero and duplicate candidates dropped, ∞ dropped
    assert checked >= 4 * 40


@pytest.mark.gpu
@pytest.mark.parametrize("maxp", (1, 3, 5, 7))
def test_decision_table_on_the_device(cgo, contexts, maxp):
    """k_finalize_ctl<10 | 24 | 40 | 56> alone on the table's rows (form "controller"): record, state, arguments and round counter
    equal the host-compiled ctl_step's, byte for byte."""
    T = decision_table()
    B, LSS = betas(cgo), line_searches(cgo)
    d = launch_inputs("quad_diag", ADT, 17)[0]
    o = _make_objective(cgo, Quad, 17, contexts["fused"], d)
    mism = []
    W = row_width(maxp)
    try:
        groups = defaultdict(list)
        for c in T:
            if table_row(c, maxp) is not None:
                groups[(c["ls"], c["beta"])].append(c)
        for (lsn, bn), cases in groups.items():
            s = _solver(cgo, o, "fused", B[bn], LSS[lsn], maxp)
            round0 = None
            try:
                for c in cases:
                    st, row = table_row(c, maxp)
                    got = s.probe_armed(st, 1, "controller", max_iters=c["max_iters"], eps=c["eps"], row=row)
                    REACHED.update(got["symbols"])
                    tag = f"{c['name']} maxp={maxp} ({c['why']})"
                    if got["symbols"] != [f"k_finalize_ctl<{W}>"]:
                        mism.append(f"{tag}: launched {got['symbols']}")
                    hs = make_state(st)
                    want = host_round(make_config(LSS[lsn], B[bn], maxp, c["eps"], c["max_iters"]), hs, row[:W])
                    rec = got["records"][0]
                    if rec["accepted"] != c["accepted"]:
                        mism.append(f"{tag}: accepted = {rec['accepted']}")
                    if rec["bytes"] != bytes(want):
                        w = np.frombuffer(bytes(want), dtype=np.int64)
                        g = np.frombuffer(rec["bytes"], dtype=np.int64)
                        mism.append(f"{tag}: record words {np.nonzero(w != g)[0].tolist()} differ from the host's")
                    if got["st"]["bytes"] != bytes(hs):
                        mism.append(f"{tag}: state {dict((k, v) for k, v in got['st'].items() if k != 'bytes')} vs host {state_dict(hs)}")
                    args_want = args_bytes(hs) if st["go"] else args_bytes(make_state(st))
                    if got["args"]["bytes"] != args_want:
                        mism.append(f"{tag}: argument block differs from the host state's")
                    if st["go"] and not np.array_equal(bits(got["out_dev"][:W]), bits(row[:W])):
                        mism.append(f"{tag}: out_dev is not the row")
                    if round0 is not None and got["round"] != round0 + 1:
                        mism.append(f"{tag}: round {got['round']} after {round0}")
                    round0 = got["round"]
                    TABLE_ROWS_ON_DEVICE[0] += 1
            finally:
                s.close()
    finally:
        o.close()
    _report(mism)


# ---- (d) chains of rounds ------------------------------------------------------------------------------------------------
# Real data, chosen on the CPU (chain_on_numpy below with the host-compiled ctl_step) so that the first trial is accepted five
# times in a row and max_iters = 6 stops the controller in round 6 of every batch.
CHAIN_MAX_ITERS = 6
CHAIN_ROUNDS = {1: 8, 3: 12, 7: 7}                          # points → rounds: graph splits 8, 8 + 4, 4 + 2 + 1


def chain_inputs(kind, n):
    """x, u = −∇f(x), parameter vector, the first state's scalars (a_acc, β) and the line search."""
    rng = np.random.default_rng(1000 + n % 997)
    if kind == "quad_diag":
        p = 1.0 + rng.integers(0, 9, n) / 16.0              # D ∈ [1, 1.5]
        x = rng.uniform(-1.0, 1.0, n)
        return x, -(p * x), p, 0.5, 0.0, "SW"
    t = 1.0 + rng.uniform(-0.05, 0.05, n // 2)              # near the valley floor around (1, 1)
    x = np.empty(n)
    x[0::2], x[1::2] = t, t * t + rng.uniform(-0.01, 0.01, n // 2)
    return x, -_np_grad(kind, x, None)[1], None, 2.0 ** -11, 0.0, "WB"


def _np_grad(kind, x, p):
    if kind == "quad_diag":
        g = p * x
        return 0.5 * (g * x), g
    xe, xo = x[0::2], x[1::2]
    t1, t2 = xo - xe * xe, 1.0 - xe
    g = np.empty_like(x)
    g[0::2], g[1::2] = -400.0 * (xe * t1) - 2.0 * t2, 200.0 * t1
    return 100.0 * (t1 * t1) + t2 * t2, g


def np_round(kind, x, u, p, a_acc, beta, a, maxp):
    """One accept + direction + trial launch in plain numpy (sums in numpy's order: for choosing inputs, not a reference)."""
    x1 = x + a_acc * u
    f0, g = _np_grad(kind, x1, p)
    un = -g + beta * u
    row = np.zeros(NSUMS)
    for j in range(maxp):
        ft, gt = _np_grad(kind, x1 + a[j] * un, p)
        y = gt - g
        row[7 * j:7 * j + 7] = [ft.sum(), gt @ un, gt @ gt, gt @ g, y @ y, un @ y, y @ gt]
    row[7 * maxp], row[7 * maxp + 1] = g @ un, un @ un
    return row, x1, un


def first_state(kind, n, maxp, cgo):
    x, u, p, a_acc, beta, lsn = chain_inputs(kind, n)
    ls = line_searches(cgo)[lsn]
    f0, g = _np_grad(kind, x + a_acc * u, p)
    pts = tree_points(ls, first_step(ls, a_acc), maxp)
    return x, u, p, dict(f_x=float(f0.sum()), gg=float(g @ g), a_acc=a_acc, beta=beta, a=pts, it=0), lsn


def chain_reference(cgo, kind, n, maxp, rounds, launch):
    """The reference chain: `launch(a_acc, beta, a[0..maxp), x, u)` → (row, x, u) for every round the controller runs, the
    host-compiled ctl_step in between.  Returns the records, the final state, x, u."""
    x, u, p, st, lsn = first_state(kind, n, maxp, cgo)
    cfg = make_config(line_searches(cgo)[lsn], betas(cgo)["PolakRibiere"], maxp, 1e-9, CHAIN_MAX_ITERS)
    s = make_state(st)
    recs = []
    for _ in range(rounds):
        row = None
        if s.go:
            row, x, u = launch(s.a_acc, s.beta, list(s.a)[:maxp], x, u)
        recs.append(host_round(cfg, s, row))
    return recs, s, x, u


CHAIN_CASES = [(kind, n + (n & 1 if kind != "quad_diag" else 0), p) for kind in ("quad_diag", "rosenbrock_paired") for n in (17, N_TWO_LEVEL)
               for p in (1, 3, 7)]


def _accepted_before_stop(recs):
    acc = [r.accepted for r in recs if r.npts >= 0]
    return sum(acc), len(acc)


def test_chain_inputs_accept_rounds_on_the_numpy_model(cgo):
    """CPU tier: with numpy's sums in place of the kernel's the chains accept at least three rounds, stop inside the batch and
    leave idle rounds behind — the inputs are fit for (d).  (The GPU test asserts the same on its own reference chain.)"""
    for kind, n, maxp in CHAIN_CASES:
        p = chain_inputs(kind, n)[2]
        recs, s, _, _ = chain_reference(cgo, kind, n, maxp, CHAIN_ROUNDS[maxp], lambda a_acc, beta, a, x, u: np_round(kind, x, u, p, a_acc, beta, a, maxp))
        acc, ran = _accepted_before_stop(recs)
        assert acc >= 3 and ran == acc + 1 and ran < len(recs) and s.go == 0, (kind, n, maxp, acc, ran)


@pytest.mark.gpu
@pytest.mark.parametrize("tail", ("fused", "finalize"))
@pytest.mark.parametrize("kind,n,maxp", CHAIN_CASES, ids=[f"{k}-n{n}-p{p}" for k, n, p in CHAIN_CASES])
def test_chains_of_rounds_against_plain_launches(cgo, contexts, kind, n, maxp, tail):
    """(d): r armed rounds, one by one and as captured graphs, against r plain accept + direction + trial launches of a
    host-driven solver with the host-compiled ctl_step between them: every slot of every record, the final state, x and u bit
    for bit; the stopping round and the idle rounds behind it."""
    rounds = CHAIN_ROUNDS[maxp]
    x0, u0, p, st, lsn = first_state(kind, n, maxp, cgo)
    obj = Quad if kind == "quad_diag" else Rosen
    # (an objective per solver: a solver's first probe re-allocates its objective's parameter vector)
    objs = [cgo.QuadDiag(p, contexts[tail]) if obj is Quad else cgo.RosenbrockPaired(n, contexts[tail]) for _ in range(3)]
    B, LS = betas(cgo)["PolakRibiere"], line_searches(cgo)[lsn]
    plain = _solver(cgo, objs[0], tail, B, LS, maxp, depth=0)
    armed = {form: _solver(cgo, objs[1 + j], tail, B, LS, maxp) for j, form in enumerate(("rounds", "graph"))}
    mism = []
    try:
        def launch(a_acc, beta, a, x, u):
            r = plain.probe_launch("accept_dir_trial", ADT, a_acc, beta, a, x, u)
            assert r["symbol"] == f"k_cg<{ON[obj]}, {ADT}, {maxp}, false>", r["symbol"]
            return r["sums"], r["x"], r["u"]
        recs, s, xr, ur = chain_reference(cgo, kind, n, maxp, rounds, launch)
        acc, ran = _accepted_before_stop(recs)
        assert acc >= 3 and ran == acc + 1 and ran < rounds and s.go == 0, f"the reference chain accepted {acc} of {ran} rounds it ran"
        outs = {}
        for form, sv in armed.items():
            got = outs[form] = sv.probe_armed(st, rounds, form, x0, u0, max_iters=CHAIN_MAX_ITERS, eps=1e-9)
            REACHED.update(got["symbols"])
            tag = f"{kind} n={n} p={maxp} {tail} {form}"
            if got["symbols"] != expected_symbols(obj, maxp, n, tail, False) * rounds:   # (an idle round launches the same kernels)
                mism.append(f"{tag}: launched {got['symbols'][:4]}… ({len(got['symbols'])} symbols) for {rounds} rounds")
            for r, (rec, want) in enumerate(zip(got["records"], recs)):
                if rec["bytes"] != bytes(want):
                    w, g = np.frombuffer(bytes(want), dtype=np.int64), np.frombuffer(rec["bytes"], dtype=np.int64)
                    mism.append(f"{tag}: round {r}: record words {np.nonzero(w != g)[0][:10].tolist()} differ from (plain row, host ctl_step); "
                                f"npts {rec['npts']}/{want.npts} accepted {rec['accepted']}/{want.accepted}")
                    break
            for r in range(ran, rounds):
                rec = got["records"][r]
                if rec["npts"] != -1 or rec["accepted"] or any(rec["bytes"][:8 * 65]):
                    mism.append(f"{tag}: round {r} behind the stop is not an idle record")
            if got["st"]["bytes"] != bytes(s) or got["args"]["bytes"] != args_bytes(s):
                mism.append(f"{tag}: final state / arguments differ from the reference chain's")
            if not (np.array_equal(bits(got["x"]), bits(xr)) and np.array_equal(bits(got["u"]), bits(ur))):
                mism.append(f"{tag}: x or u after the batch differ from the plain chain's (as the stopping round left them)")
            if not mism:
                CELLS[(tuple(expected_symbols(obj, maxp, n, tail, False)), n, f"{tail}-chain-{form}")] += 1
        a, b = outs["rounds"], outs["graph"]
        if [r["bytes"] for r in a["records"]] != [r["bytes"] for r in b["records"]] or a["st"]["bytes"] != b["st"]["bytes"] or \
                not np.array_equal(bits(a["x"]), bits(b["x"])) or not np.array_equal(bits(a["u"]), bits(b["u"])):
            mism.append(f"{kind} n={n} p={maxp} {tail}: the captured graphs differ from the rounds launched one by one")
        if a["round"] - rounds != b["round"] - rounds:
            mism.append(f"{kind} n={n} p={maxp} {tail}: round counters {a['round']} / {b['round']}")
    finally:
        plain.close()
        for sv in armed.values():
            sv.close()
        for o in objs:
            o.close()
    _report(mism)


# ---- (e) ring and idle -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tail", ("fused", "finalize"))
def test_idle_batches_round_counter_and_ring_wrap(cgo, contexts, tail):
    """A batch started with go = 0 leaves x, u and the device row alone and files idle records; the device round counter runs on
    from probe to probe; more than 64 rounds in all wrap the record ring, every record still validating (the probe returns
    CGO_ESTATE otherwise) and landing in order."""
    n, k = 129, 7
    d, a_acc, beta, a = round_inputs(Quad, n, k)
    want_row, want_vec = exact_round(Quad, n, k)
    o = _make_objective(cgo, Quad, n, contexts[tail], d)
    B, LS = betas(cgo)["PolakRibiere"], line_searches(cgo)["SW"]
    s = _solver(cgo, o, tail, B, LS, 7)
    try:
        st = dict(f_x=2.0 ** 40, gg=3.0, a_acc=a_acc, beta=beta, a=a, it=3)
        first = s.probe_armed(st, 1, "rounds", d.full["x"], d.full["u"], max_iters=4)   # runs, then stops (last iteration)
        assert np.array_equal(bits(first["out_dev"][:56]), bits(want_row)) and first["st"]["go"] == 0
        total, rnd = 1, first["round"]
        idle = dict(st, go=0)
        for form, r in (("rounds", 32), ("graph", 32), ("rounds", 5), ("graph", 7)):
            got = s.probe_armed(idle, r, form, d.full["x"], d.full["u"], max_iters=4)
            assert got["round"] == rnd + r, (form, r, got["round"], rnd)
            rnd, total = got["round"], total + r
            assert np.array_equal(bits(got["x"]), bits(d.full["x"])) and np.array_equal(bits(got["u"]), bits(d.full["u"]))
            assert np.array_equal(bits(got["out_dev"]), bits(first["out_dev"])), "an idle batch wrote the device row"
            assert len(got["records"]) == r and all(q["npts"] == -1 and not q["accepted"] and not any(q["bytes"][:8 * 65]) for q in got["records"])
            assert got["st"]["go"] == 0 and got["args"]["go"] == 0 and got["st"]["bytes"] == bytes(make_state(idle))
        assert total > PIPE_RING
        # … and a running round behind the wrap is still the exact round
        again = s.probe_armed(st, 1, "rounds", d.full["x"], d.full["u"], max_iters=BIG_MAX_ITERS)
        mism = []
        check_round("after the wrap", again, want_row, want_vec, make_config(LS, B, 7, 1e-9, BIG_MAX_ITERS), st, rnd, mism)
        _report(mism)
    finally:
        s.close(); o.close()


@pytest.mark.gpu
def test_probe_refuses_what_the_engine_would_not_arm(cgo, contexts):
    d = launch_inputs("quad_diag", ADT, 17)[0]
    o = _make_objective(cgo, Quad, 17, contexts["fused"], d)
    B, LS = betas(cgo)["PolakRibiere"], line_searches(cgo)["SW"]
    st = dict(f_x=1.0, gg=1.0, a_acc=0.5, beta=0.0, a=[0.5], it=0)
    try:
        s = _solver(cgo, o, "fused", B, LS, 3, depth=0)
        with pytest.raises(cgo.CgoError) as e:
            s.probe_armed(st, 1, "rounds", d.full["x"], d.full["u"])
        assert e.value.code == 1
        s.close()
        s = _solver(cgo, o, "fused", B, LS, 3)
        for kw in (dict(rounds=0), dict(rounds=33), dict(rounds=2, form="controller"), dict(x=None)):
            args = dict(rounds=1, form="rounds", x=d.full["x"], u=d.full["u"])
            args.update(kw)
            with pytest.raises(cgo.CgoError) as e:
                s.probe_armed(st, **args)
            assert e.value.code == 1, kw
        s.probe_armed(st, 1, "rounds", d.full["x"], d.full["u"])
        with pytest.raises(cgo.CgoError):
            s.start()                      # for probing only
        s.close()
    finally:
        o.close()


# ---- (f) coverage ----------------------------------------------------------------------------------------------------------
def module_symbols():
    """what this module's case lists are written to reach"""
    builtin = [ON[o] for o in (Quad, Rosen, Booth)]
    return {f"k_cg_armed<{on}, {npts_for(k)}>" for on in builtin for k in KS} | {f"k_finalize_ctl<{row_width(npts_for(k))}>" for k in KS}


def test_armed_rows_have_tests():
    """CPU tier: the symbols this module expects are exactly the armed rows of csrc/cgo_instances.def × its objectives and the
    four widths of k_finalize_ctl: a new armed row cannot come without a test here."""
    functors = [f for _, f in I.rows("OBJ")]
    want = {f"k_cg_armed<{f}, {p}>" for f in functors for mode, p in I.mode_points("CG_ARMED")} | {f"k_finalize_ctl<{w}>" for w in WIDTHS}
    assert all(mode == ADT for mode, _ in I.mode_points("CG_ARMED")) and len(functors) == 3
    assert module_symbols() == want
    assert I.stray_uses() == []


@pytest.mark.gpu
def test_coverage_of_every_armed_instantiation(cgo, contexts):
    """Every k_cg_armed instantiation and every width of k_finalize_ctl was launched by a probe whose round was checked; what this
    run has not reached yet (the test on its own, the module split or reordered) is probed here at n = 17."""
    small = {Quad: 17, Rosen: 16, Booth: 2}
    mism = []
    for obj, n in small.items():
        ks = [k for k in KS if f"k_cg_armed<{ON[obj]}, {npts_for(k)}>" not in REACHED]
        if ks:
            mism += run_rounds(cgo, contexts, obj, n, "fused", False, ks=ks)
    ks = [k for k in KS if f"k_finalize_ctl<{row_width(npts_for(k))}>" not in REACHED]
    if ks:
        mism += run_rounds(cgo, contexts, Quad, 17, "finalize", False, ks=ks)
    _report(mism)
    still = sorted(module_symbols() - REACHED)
    assert not still, f"never probed: {still}"
    print(f"\n[armed kernel sums] {len(CELLS)} (symbols, size, form) cells checked bit for bit in {sum(CELLS.values())} rounds, "
          f"{TABLE_ROWS_ON_DEVICE[0]} table rows on the device")
