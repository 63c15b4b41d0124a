"""Every sum slot and vector of every launch of the stored-gradient family, one launch at a time (cgo_solver_probe_launch).

The family is k_fused<Obj, MODE, BIG> (csrc/cgo_kernels.hip.hpp) with the kernels only it uses: k_trial_point (the host
closure's trial point), k_scaled_norm / k_finalize_maxsum (LinearAlgebra.norm's rare path) and the non-canonical
k_finalize_t<NS, 256> over up to 1024 partial rows (two launches at 4096 rows without the fused tail).  A solver runs on it
for β = LBFGS on an element-wise objective, for a host closure, under policy.stored_gradient, and the kernel-level entry
points (updatedir_, beta_partials, evalϕdϕ) launch it directly.  The machinery is that of test_kernel_sums (imported):

(a) exact dyadic data — x, u, g (a free input here: the gradient is stored, not recomputed), D, a, β, a_acc such that every
    product is exact and every slot's Σ|term| stays below 2⁵³ quanta, asserted operation by operation — so that every
    summation order gives the same bits: the whole NS = 10 row must equal the exact sums bit for bit, slots a mode does not
    accumulate must be +0.0, and x, u, g⁺ must equal the numpy restatement of body2 / body1 (vectors a mode does not write:
    what was put there, or NaN).  The paired Rosenbrock data are coarse enough (x, g on a 1/2 grid, unit trial step) that
    modes 12 and 15 admit exact data too: NO cell of (a) falls back to the bound of (b);
(b) random data: every slot within γ_d·Σ|t| of the correctly rounded exact sum, d from the launch's own depth;
(c) the host-closure path: k_trial_point's vector as the closure receives it, the closure's f in S_F, the zeroed g and u of
    the initial evaluation, u = −g after the reset;
(d) the norm passes on data whose maximum is a power of two (max, NaN count, Σ (v/max)², padding: bitwise) and on random data;
(e) updatedir_ (M_DIR alone) and beta_partials, bitwise;
(f) the launch lists here name every (objective, mode) instantiation launch_obj / launch_any and the run-time compiled module
    can dispatch (CPU tier, parsed from the source), and every one of them × {grid-stride, pure-HBM} was reached.

A cell is (instantiation symbol, n, tail); it counts only when its whole row and every vector were compared.
"""
import math
import os
import subprocess
import sys
from collections import defaultdict

import numpy as np
import pytest

import _instances as I
import test_kernel_sums as K
from test_kernel_sums import (BLOCK, GRID_BIG, NAN_BITS, SIZES, TAILS, A, M, S, Booth, Data, Quad, Rosen, User, _dy, _f,
                              big_chunk_pairs, bits, contexts, exact_period, exact_sum, two_prod)  # noqa: F401 (contexts: fixture)

ROOT = K.ROOT
NS, GRID_SMALL = 10, 1024
F, GTU, GTGT, GTG, YY, UY, YGT, GU, UU, GG = range(NS)
M_ACCEPT, M_DIR, M_TRIAL, M_BETA, M_INIT, M_RESET, M_UPG, M_BETAONLY = 1, 2, 4, 8, 16, 32, 64, 128
FINALIZE_2STAGE_BYTES = 131072                             # cgo_hip_backend.hip two_stage_rows: rows·ns·8 above this

# what a solver's engine issues (kind, mode); M_DIR alone and M_BETAONLY come from the kernel-level entries / the host closure
LAUNCHES = [("init", M_INIT), ("trial", M_TRIAL), ("trial", M_TRIAL | M_BETA), ("accept_dir_trial", 15), ("accept_dir", 3),
            ("accept_only", M_ACCEPT), ("reset_dir", M_RESET), ("upg_norm", M_UPG)]
OBJ_MODES = (M_INIT, M_TRIAL | M_BETA, M_TRIAL, 15)        # instantiated per objective (launch_obj, the run-time module)
FREE_MODES = (3, M_ACCEPT, M_DIR, M_RESET, M_UPG, M_BETAONLY)   # objective-free: ObjQuadDiag's instantiation whatever the objective
OBJ_NAMES = {"quad_diag": "ObjQuadDiag", "rosenbrock_paired": "ObjRosenPaired", "booth": "ObjBooth", "user_quad": "UserObjective"}


def grid_for(n):
    """grid_for / grid_capped of cgo_hip_backend.hip: two pairs per lane, at most GRID_SMALL workgroups."""
    return min(max(1, -(-(n >> 1) // (BLOCK * 2))), GRID_SMALL)


def symbol_for(obj_name, mode, big):
    on = OBJ_NAMES[obj_name] if mode & (M_TRIAL | M_INIT) else "ObjQuadDiag"
    return f"k_fused<{on}, {mode}, {'true' if big else 'false'}>"


# ---- sizes: which edge each one hits -----------------------------------------------------------------------------------
FINALIZE_ROWS = (25, 26, 200, 201, 1024)
HBM_CHUNKS = {2 * GRID_BIG * 264: "pure-HBM: chunks of 264 pairs, lanes 0–7 take a two-at-a-time main trip",
              2 * GRID_BIG * 520: "pure-HBM: chunks of 520 pairs, every lane a main trip, lanes 0–7 the remainder too",
              2 * (GRID_BIG * 520 - 1) + 1: "pure-HBM: chunks of 520 pairs, the last one a pair short, odd tail element"}


def _sizes():
    s = dict(SIZES)                                        # big_chunk_pairs and the odd-tail path are the same as k_cg's
    for n2, what in ((257, "one workgroup, lane 0 alone takes a two-at-a-time main trip"),
                     (512, "one workgroup, every lane exactly one main trip, no remainder"),
                     (513, "second workgroup, lane 0 of the first a main trip")):
        s[2 * n2] = "grid-stride: " + what
        s[2 * n2 + 1] = s[2 * n2] + ", odd tail element"
    for rows in FINALIZE_ROWS:
        s[2 * 512 * rows] = f"k_finalize_t<NS, 256> over {rows} rows" + (": the grid cap, every lane one main trip, no remainder" if rows == GRID_SMALL else "")
    s[2 * (GRID_SMALL * 512 + 1) + 1] = "grid cap: lane 0 takes a main trip and the remainder, odd tail element"
    return s


S_SIZES = _sizes()
LARGE = 2 * 512 * 200                                      # from here on: the fused tail only


def stride_trips(n2, grid):
    """(main trips, remainder taken) per lane of k_fused's grid-stride loop."""
    T = grid * BLOCK
    i = np.arange(T)
    main = np.maximum(0, -(-(n2 - T - i) // (2 * T)))
    return main, (i + 2 * T * main) < n2


def chunk_trips(length):
    """the same for one pure-HBM chunk of `length` pairs"""
    t = np.arange(BLOCK)
    main = np.maximum(0, -(-(length - BLOCK - t) // (2 * BLOCK)))
    return main, (t + 2 * BLOCK * main) < length


def finalize_trips(rows):
    """values per lane and load trips per lane of the single-stage k_finalize_t<NS, 256> (G = 25, U = 8)"""
    G = BLOCK // NS
    tid = np.arange(G * NS)
    vals = np.maximum(0, -(-(rows * NS - tid) // (G * NS)))
    return vals, -(-vals // 8)


def test_sizes_hit_the_edges_they_claim():
    """CPU tier: every claim of the size table follows from BLOCK 256, two pairs per lane, GRID_SMALL 1024, GRID_BIG 4096, chunks
    rounded to 8 pairs, G = 25 row groups and the 8-deep unroll."""
    assert set(SIZES) <= set(S_SIZES)
    main, rem = stride_trips(257, grid_for(514))
    assert grid_for(514) == 1 and main[0] == 1 and main[1:].sum() == 0 and not rem[0] and rem[1:].all()
    main, rem = stride_trips(512, grid_for(1024))
    assert grid_for(1024) == 1 and (main == 1).all() and not rem.any()
    main, rem = stride_trips(513, grid_for(1026))
    assert grid_for(1026) == 2 and main[0] == 1 and main[1:].sum() == 0 and rem[1:].all() and rem.size == 512
    n2 = GRID_SMALL * 512
    main, rem = stride_trips(n2, grid_for(2 * n2))
    assert grid_for(2 * n2) == GRID_SMALL and (main == 1).all() and not rem.any()
    main, rem = stride_trips(n2 + 1, grid_for(2 * n2 + 3))
    assert grid_for(2 * n2 + 3) == GRID_SMALL and (main == 1).all() and rem[0] and not rem[1:].any()
    for rows in FINALIZE_ROWS:
        assert grid_for(2 * 512 * rows) == rows and rows * NS * 8 <= FINALIZE_2STAGE_BYTES   # one stage
    assert GRID_BIG * NS * 8 > FINALIZE_2STAGE_BYTES                                         # 4096 rows: two stages
    v25, t25 = finalize_trips(25)
    v26, t26 = finalize_trips(26)
    assert (v25 == 1).all() and (v26[:10] == 2).all() and (v26[10:] == 1).all()
    v200, t200 = finalize_trips(200)
    v201, t201 = finalize_trips(201)
    assert (v200 == 8).all() and (t200 == 1).all() and (v201[:10] == 9).all() and (t201[:10] == 2).all() and (t201[10:] == 1).all()
    assert finalize_trips(1024)[0].max() == 41
    for j in (8, 16):                                      # the SIZES chunks only ever take the remainder branch
        assert chunk_trips(j)[0].sum() == 0
    main, rem = chunk_trips(264)
    assert big_chunk_pairs(GRID_BIG * 264) == 264 and (main[:8] == 1).all() and main[8:].sum() == 0 and rem[8:].all() and not rem[:8].any()
    main, rem = chunk_trips(520)
    assert big_chunk_pairs(GRID_BIG * 520) == 520 and (main == 1).all() and rem[:8].all() and not rem[8:].any()
    assert big_chunk_pairs(GRID_BIG * 520 - 1) == 520 and (GRID_BIG * 520 - 1) - 520 * (GRID_BIG - 1) == 519
    for n in HBM_CHUNKS:                                   # default policy keeps them grid-stride: forced for the pure-HBM run
        assert 8.0 * n * 7 < 4.5e8 and grid_for(n) == GRID_SMALL
    for n in (K1, K1 + 1):                                 # k_trial_point / k_scaled_norm: 1024 workgroups of 256, second trip
        assert min(-(-n // BLOCK), GRID_SMALL) == GRID_SMALL and -(-n // (GRID_SMALL * BLOCK)) == (1 if n == K1 else 2)


K1 = GRID_SMALL * BLOCK                                    # one element per lane of k_trial_point's / k_scaled_norm's capped grid


# ---- the kernel restated (body2 / body1, unfused, in the kernel's order) ------------------------------------------------
def fused_model(obj, x, u, g, p, mode, a, a_acc, beta, single, gt=None):
    """One k_fused launch on a block of pairs (or the odd tail element).  (terms, vectors): terms[slot] = [(factors,
    per_element)], a term is the product of its one or two factors (per_element False: the per-pair f terms)."""
    grad = obj.g1 if single else obj.g2
    fe = obj.per_elem_f or single
    T, out = defaultdict(list), {}
    if mode & M_ACCEPT:
        x = A(x, M(a_acc, u))
        out["x"] = x
    if mode & (M_DIR | M_RESET):
        un = A(-g, M(beta, u)) if mode & M_DIR else -g
        T[GU].append(((g, un), True)); T[UU].append(((un, un), True))
        out["u"] = u = un
    if mode & M_TRIAL:
        f, gp = grad(A(x, M(a, u)), p)
        out["g"] = gp
        T[F].append(((f,), fe)); T[GTU].append(((gp, u), True)); T[GTGT].append(((gp, gp), True))
        if mode & M_BETA:
            y = S(gp, g)
            T[GTG].append(((gp, g), True)); T[YY].append(((y, y), True)); T[UY].append(((u, y), True)); T[YGT].append(((y, gp), True))
    if mode & M_INIT:
        f, gp = grad(x, p)
        out["g"], out["u"] = gp, -gp
        T[F].append(((f,), fe)); T[GTGT].append(((gp, gp), True))
    if mode & M_UPG:
        t = A(u, g)
        T[UU].append(((t, t), True))
    if mode & M_BETAONLY:
        y = S(gt, g)
        for slot, fac in ((GTU, (gt, u)), (GTGT, (gt, gt)), (GTG, (gt, g)), (YY, (y, y)), (UY, (u, y)), (YGT, (y, gt)), (GG, (g, g)),
                          (GU, (g, u)), (UU, (u, u))):
            T[slot].append((fac, True))
    return T, out


def reads_u(mode):
    return bool(mode & (M_ACCEPT | M_DIR | M_TRIAL | M_UPG | M_BETAONLY))


def reads_g(mode):
    return bool(mode & (M_DIR | M_BETA | M_RESET | M_UPG | M_BETAONLY))


def expected_fused(obj, d, mode, a, a_acc, beta, gt_key=None, f_host=0.0, g_key="g", u_key="u", x_key="x"):
    """The exact row and the vectors (x, u, g = the g⁺ buffer) one k_fused launch leaves on Data d; None: NaN (never written,
    never put).  gt_key: the stored g⁺ M_BETAONLY reads; f_host: the closure's f, which joins S_F."""
    terms, weights = defaultdict(list), defaultdict(list)
    parts = {"x": [], "u": [], "g": []}
    zeros = lambda k, blk: np.zeros_like(blk["x"]) if k is None else blk[k]
    for part, blk in (("pairs", d.block if d.n2 else None), ("single", d.single)):
        if blk is None:
            continue
        single = part == "single"
        T, out = fused_model(obj, blk[x_key], zeros(u_key, blk), zeros(g_key, blk), blk.get("p"), mode, a, a_acc, beta, single,
                             gt=blk[gt_key] if gt_key else None)
        for s, lst in T.items():
            for fac, per_elem in lst:
                arr = M(*fac) if len(fac) == 2 else fac[0]
                terms[s].append(arr)
                weights[s].append(np.ones(arr.size, np.int64) if single else (d.celem if per_elem else d.cpair))
        m, lo = (1, d.n - 1) if single else (2 * d.n2, 0)
        for key in parts:
            v = out.get(key)
            if v is None:
                src = {"x": x_key, "u": u_key if reads_u(mode) else None, "g": gt_key}[key]
                v = None if src is None else d.full[src][lo:lo + m]
            parts[key].append(None if v is None else np.resize(v, m))
    sums = np.zeros(0 if mode == M_ACCEPT else NS)
    for s in terms:
        sums[s] = exact_sum(terms[s], weights[s])
    if mode & M_BETAONLY:
        sums[F] = f_host
    return sums, {k: (None if any(q is None for q in v) else np.concatenate(v)) for k, v in parts.items()}


# ---- exact data ----------------------------------------------------------------------------------------------------------
# quad: the k_cg module's period plus a stored gradient g and a closure gradient gp on the same grids.  Paired Rosenbrock: x, g on
# a 1/2 grid, u = ±1/2, a_acc = β = 1/2 and a UNIT trial step: the trial point stays on a 1/4 grid, g⁺ on a 1/4 grid below 2¹⁴,
# so that even the squares of mode 15 keep under 2⁵³ quanta at a million elements.
SCAL = {"quad_diag": (0.5, 0.75, 0.25), "user_quad": (0.5, 0.75, 0.25), "rosenbrock_paired": (0.5, 0.5, 1.0), "booth": (0.5, 0.75, 0.25)}
_PERIODS = {}


def stored_period(name):
    if name not in _PERIODS:
        if name == "booth":
            per = dict(x=np.array([0.5, 1.25]), u=np.array([-0.25, 0.75]), g=np.array([0.5, -1.0]), gp=np.array([1.5, 0.25]))
        else:
            per = dict(exact_period(name))
            rng = np.random.default_rng(1234)
            L = 2 * K.PERIOD_PAIRS
            if name == "rosenbrock_paired":
                per["g"], per["gp"] = _dy(rng, L, -2, 2, 0.5), _dy(rng, L, -2, 2, 0.5)
            else:
                per["g"], per["gp"] = _dy(rng, L, -6, 6, 0.25), _dy(rng, L, -5, 5, 0.5)
        _PERIODS[name] = per
    return _PERIODS[name]


def obj_sizes(obj):
    if obj is Booth:
        return [2]
    return [n for n in sorted(S_SIZES) if not (obj is Rosen and n % 2)]


USER_SIZES = [17, 1027, 2 * (GRID_BIG * 8 + 1) + 1, 2 * 512 * 26]


def test_exact_data_meet_their_preconditions():
    """CPU tier: for every objective, mode and size of (a), (c), (e) every product is exact and every slot's Σ|term| < 2⁵³
    quanta (M / A / exact_sum assert it) — the checks the GPU tests make before they compare, without a GPU."""
    for obj in (Quad, Rosen, Booth):
        ns = obj_sizes(obj)
        for n in ns[:4] + ns[-6:] + ([] if obj is not Quad else list(HBM_CHUNKS)):
            d = Data(n, stored_period(obj.name))
            a_acc, beta, a = SCAL[obj.name]
            for _, mode in LAUNCHES:
                expected_fused(obj, d, mode, a, a_acc, beta)
    for n in C_SIZES:
        _host_expected(Data(n, stored_period("quad_diag")))
    for n in E_SIZES:
        d = Data(n, stored_period("quad_diag"))
        expected_fused(Quad, d, M_DIR, 0.0, 0.0, 0.75)
        expected_fused(Quad, d, M_BETAONLY, 0.0, 0.0, 0.0, gt_key="gp")


# ---- GPU: (a) --------------------------------------------------------------------------------------------------------------
REACHED = set()
CELLS = defaultdict(int)
VALUES = [0]


def _solver(cgo, obj, tail, big, beta=None):
    pol = cgo.SolverPolicy(stored_gradient=True, resident=False, controller_depth=0, hbm_stream_bytes=1.0 if big else None, **TAILS[tail])
    cfg = cgo.setupCGConfig(1e-9, beta or cgo.PolakRibiere(), cgo.DisableTrace(), max_iters=5)
    return cgo.Solver(obj, cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), pol)


def _objective(cgo, obj, n, ctx, d):
    return K._make_objective(cgo, obj, n, ctx, d)


def _note(got, n, tail, ok):
    for sym in got["symbol"].split(" + "):
        REACHED.add(sym)
        if ok:
            CELLS[(sym, n, tail)] += 1
    if ok:
        VALUES[0] += got["sums"].size + 3 * n


def _run(cgo, ctxs, obj, n, tails=tuple(TAILS), bigs=(False, True), launch_list=None, beta=None):
    mism, cache = [], {}
    d = Data(n, stored_period(obj.name))
    a_acc, beta_s, a = SCAL[obj.name]
    for tail in tails:
        for big in bigs:
            o = _objective(cgo, obj, n, ctxs[tail], d)
            s = _solver(cgo, o, tail, big, beta)
            try:
                for kind, mode in (launch_list or LAUNCHES):
                    if mode not in cache:
                        cache[mode] = expected_fused(obj, d, mode, a, a_acc, beta_s)
                    want_sums, want = cache[mode]
                    got = s.probe_launch(kind, mode, a_acc, beta_s, [a] if mode & M_TRIAL else [], d.full["x"],
                                         d.full["u"] if reads_u(mode) else None, d.full["g"] if reads_g(mode) else None)
                    tag = f"{obj.name} n={n} {tail} {'pure-HBM' if big else 'grid-stride'} {kind}/{mode} [{got['symbol']}]"
                    ok = got["symbol"] == symbol_for(obj.name, mode, big)
                    if not ok:
                        mism.append(f"{tag}: expected {symbol_for(obj.name, mode, big)}")
                    ok = ok and K._compare(tag, got, want_sums, want, mism)
                    _note(got, n, tail, ok)
            finally:
                s.close(); o.close()
    return mism


def _tails(n):
    return tuple(TAILS) if n < LARGE else ("fused",)


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(S_SIZES), ids=lambda n: f"n{n}")
def test_quad_exact_every_slot(cgo, contexts, n):
    K._report(_run(cgo, contexts, Quad, n, tails=_tails(n)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(HBM_CHUNKS), ids=lambda n: f"n{n}")
def test_quad_exact_pure_hbm_main_trip(cgo, contexts, n):
    """Chunks of 264 and 520 pairs: the two-at-a-time main trip of the BIG branch (and, by default policy, the same sizes
    grid-stride at the grid cap with four main trips per lane)."""
    K._report(_run(cgo, contexts, Quad, n, tails=("fused",)))


@pytest.mark.gpu
def test_two_launch_finalize_at_4096_rows(cgo, contexts):
    """fused_tail off on the pure-HBM path: k_finalize_t<NS, 256> twice (64 groups of 64 rows, then 64 rows) — here at a size
    where all 4096 workgroups are busy and at one where 3583 of them store rows of zeros."""
    for n in (2 * GRID_BIG * 16 + 1, 2 * (GRID_BIG + 5)):
        K._report(_run(cgo, contexts, Quad, n, tails=("finalize", "strict"), bigs=(True,)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [n for n in sorted(S_SIZES) if n % 2 == 0], ids=lambda n: f"n{n}")
def test_rosenbrock_paired_exact_every_slot(cgo, contexts, n):
    K._report(_run(cgo, contexts, Rosen, n, tails=_tails(n)))


@pytest.mark.gpu
def test_booth_exact_every_slot(cgo, contexts):
    K._report(_run(cgo, contexts, Booth, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("n", USER_SIZES, ids=lambda n: f"n{n}")
def test_user_module_exact_every_slot(cgo, contexts, n):
    """The run-time compiled module's k_fused<UserObjective, {16, 12, 4, 15}, {false, true}> (and, on the same solver, the
    objective-free launches); every tail at one size."""
    K._report(_run(cgo, contexts, User, n, tails=tuple(TAILS) if n == 1027 else ("fused",)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 1026, 2 * (GRID_BIG * 8 + 1) + 1], ids=lambda n: f"n{n}")
def test_lbfgs_solver_line_search_launches(cgo, contexts, n):
    """β = LBFGS(m) on an element-wise objective runs its initial evaluation and its line-search trials on this family (no
    policy asked for it): M_INIT and both trial modes, the probe choosing M_BETA, exact as above."""
    K._report(_run(cgo, contexts, Quad, n, tails=("fused",), beta=cgo.LBFGS(5),
                   launch_list=[("init", M_INIT), ("trial", M_TRIAL), ("trial", M_TRIAL | M_BETA), ("reset_dir", M_RESET), ("upg_norm", M_UPG)]))


# ---- (b) random data --------------------------------------------------------------------------------------------------------
def finalize_adds(rows):
    """additions on a term's way through the stored-gradient finalize: one stage — a lane's ⌈rows / G⌉ rows, then the G = 25
    groups in turn — or, above 128 KB of rows, two stages of 64-row groups (two k_finalize_t launches or k_finalize_one)."""
    G = BLOCK // NS
    if rows * NS * 8 > FINALIZE_2STAGE_BYTES:
        return 2 * (-(-64 // G) + G)
    return -(-rows // G) + G


def fused_depth(n, big):
    """d of γ_d for one k_fused launch: every term is one FMA into its lane's accumulator (exact product, one rounding per
    addition), two terms per pair and ⌈pairs per lane⌉ pairs (grid-stride: n2 / (grid·256); pure-HBM: chunk / 256), one more
    for the odd tail element and one for the closure's f, then the wave's six exchange levels, two levels over the four
    waves ((w0 + w1) + (w2 + w3)) and the finalize's additions for the launch's row count."""
    n2 = n >> 1
    grid = GRID_BIG if big else grid_for(n)
    ppl = -(-big_chunk_pairs(n2) // BLOCK) if big else -(-n2 // (grid * BLOCK))
    return 2 * ppl + 2 + 6 + 2 + finalize_adds(grid)


B_SIZES = {"quad": [17, 1027, 2 * (GRID_BIG + 5) + 1, 2 * GRID_BIG * 16 + 1, 2 * 512 * 201],
           "rosen": [16, 1026, 2 * (GRID_BIG + 5), 2 * GRID_BIG * 16]}
_B_DATA = {}


def random_stored(kind, n):
    """test_kernel_sums.random_data plus a stored gradient that keeps every term of every slot away from zero: quad g of x's
    sign in [2.5, 3] (y = g⁺ − g, u_new = −g + β·u, u + g all of one sign per element); rosen g = ½∇f(x) (∇f > 0 there)."""
    if (kind, n) not in _B_DATA:
        data, scal, su, sg = K.random_data(kind, n, 3000 + n)
        rng = np.random.default_rng(4000 + n)
        if kind == "quad":
            data["g"] = np.sign(data["x"]) * rng.uniform(2.5, 3.0, n)
        else:
            K.CHECK_EXACT[0] = False
            try:
                data["g"] = 0.5 * Rosen.g2(data["x"], None)[1]
            finally:
                K.CHECK_EXACT[0] = True
        _B_DATA[(kind, n)] = (data, scal, su, sg)
    return _B_DATA[(kind, n)]


def b_expected(kind, n, mode):
    data, (a_acc, beta), su, sg = random_stored(kind, n)
    along_g = bool(mode & M_DIR) and bool(mode & M_TRIAL)
    a = (sg if along_g else su)[0]
    if along_g and kind != "quad":
        a_acc = 0.0
    obj = Quad if kind == "quad" else Rosen
    T = defaultdict(list)
    parts = {"x": [], "u": [], "g": []}
    n2 = n >> 1
    K.CHECK_EXACT[0] = False
    try:
        for single, sl in ((False, slice(0, 2 * n2)), (True, slice(n - 1, n))):
            if (single and not n & 1) or (not single and n2 == 0):
                continue
            Ts, out = fused_model(obj, data["x"][sl], data["u"][sl], data["g"][sl], None if data["p"] is None else data["p"][sl],
                                  mode, a, a_acc, beta, single)
            for slot, lst in Ts.items():
                T[slot] += lst
            for key in parts:
                v = out.get(key)
                if v is None and (key == "x" or (key == "u" and reads_u(mode))):
                    v = data[key][sl]
                parts[key].append(v)
    finally:
        K.CHECK_EXACT[0] = True
    vec = {k: (None if any(q is None for q in v) else np.concatenate(v)) for k, v in parts.items()}
    return a, a_acc, beta, K._slot_refs(T), vec


def test_random_data_meet_the_guard():
    """CPU tier: in every slot of every launch of (b) the smallest term exceeds the slot's bound on either streaming path,
    so that a dropped or doubled element cannot hide inside it."""
    for kind, sizes in B_SIZES.items():
        for n in sizes:
            for _, mode in LAUNCHES:
                refs = b_expected(kind, n, mode)[3]
                d = max(fused_depth(n, False), fused_depth(n, True))
                for slot, (exact, absum, tmin) in refs.items():
                    assert tmin > d * 2.0 ** -53 * absum * 1.01, (kind, n, mode, slot, tmin, absum)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [(kd, n) for kd, ns in B_SIZES.items() for n in ns], ids=lambda v: str(v))
def test_random_within_summation_bound(cgo, contexts, kind, n):
    """Every mode on random data, both streaming paths, every tail: each slot within γ_d·Σ|tᵢ| of the correctly rounded sum of
    its exact terms, γ_d = d·u / (1 − d·u), u = 2⁻⁵³, d = fused_depth(n, big) — the classical bound of recursive summation:
    a term enters through one FMA (its product exact, the addition one rounding; an f term is added as it is) and every
    further addition on its path to the row — lane, wave, workgroup, finalize — is one rounding, whatever the order.
    Slots without terms are +0.0 and the vectors equal the unfused numpy restatement bit for bit."""
    data = random_stored(kind, n)[0]
    mism, cache = [], {}
    for tail in _tails(n):
        for big in (False, True):
            ctx = contexts[tail]
            o = cgo.QuadDiag(data["p"], ctx) if kind == "quad" else cgo.RosenbrockPaired(n, ctx)
            s = _solver(cgo, o, tail, big)
            try:
                for kd, mode in LAUNCHES:
                    if mode not in cache:
                        cache[mode] = b_expected(kind, n, mode)
                    a, a_acc, beta, refs, vec = cache[mode]
                    got = s.probe_launch(kd, mode, a_acc, beta, [a] if mode & M_TRIAL else [], data["x"],
                                         data["u"] if reads_u(mode) else None, data["g"] if reads_g(mode) else None)
                    tag = f"{kind} n={n} {tail} {'pure-HBM' if big else 'grid'} {kd}/{mode} [{got['symbol']}]"
                    _slot_bound_check(tag, got, 0 if mode == M_ACCEPT else NS, refs, vec, fused_depth(n, big), mism)
                    _note(got, n, tail, False)
            finally:
                s.close(); o.close()
    K._report(mism)


def _slot_bound_check(tag, got, W, refs, vec, d, mism):
    if got["sums"].size != W:
        mism.append(f"{tag}: row of {got['sums'].size} slots, expected {W}")
        return
    gam = d * 2.0 ** -53 / (1 - d * 2.0 ** -53)
    for slot in range(W):
        v = got["sums"][slot]
        if slot not in refs:
            if bits(np.array([v]))[0] != 0:
                mism.append(f"{tag}: slot {slot} carries no term, holds {v!r}")
            continue
        exact, absum, tmin = refs[slot]
        bound = gam * absum * (1 + 1e-12)
        assert tmin > bound, f"test data: {tag} slot {slot}: smallest term {tmin:.3e} within the bound {bound:.3e}"
        if not abs(v - exact) <= bound:
            mism.append(f"{tag}: slot {slot} {v!r} vs {exact!r} (bound {bound:.3e}, d = {d})")
    for key in ("x", "u", "g"):
        w, g = vec.get(key), got[key]
        wb = np.full(g.size, NAN_BITS) if w is None else bits(w)
        if not np.array_equal(bits(g), wb):
            i = int(np.nonzero(bits(g) != wb)[0][0])
            mism.append(f"{tag}: {key}_out differs first at element {i}: got {g[i]!r}, want {'NaN' if w is None else repr(w[i])}")


# ---- (c) the host-closure path ---------------------------------------------------------------------------------------------
C_SIZES = [1, 255, 256, 257, K1, K1 + 1]
F_INIT, F_TRIAL, F_ADT = 1234.5, -77.25, 3.0e5 + 0.125


def _host_expected(d):
    """what init, trial and accept_dir_trial must leave: (vector the closure receives, row(s), x, u, g⁺ buffer) each"""
    a_acc, beta, a = SCAL["quad_diag"]
    full = d.full
    out = {}
    # init: the closure sees x; M_BETAONLY on (g⁺ = gp, g = 0, u = 0) with f in S_F; swap; M_RESET on g = gp
    r0, _ = expected_fused(Quad, d, M_BETAONLY, 0.0, 0.0, 0.0, gt_key="gp", f_host=F_INIT, g_key=None, u_key=None)
    r1, v1 = expected_fused(Quad, d, M_RESET, 0.0, 0.0, 0.0, g_key="gp")
    out["init"] = (full["x"], np.concatenate([r0, r1]), dict(x=full["x"], u=v1["u"], g=np.zeros(d.n)))
    # trial: the closure sees x + a·u, unfused
    r, _ = expected_fused(Quad, d, M_BETAONLY, 0.0, 0.0, 0.0, gt_key="gp", f_host=F_TRIAL)
    out["trial"] = (A(full["x"], M(a, full["u"])), r, dict(x=full["x"], u=full["u"], g=full["gp"]))
    # accept_dir_trial: accept_dir (x ← x + a_acc·u, u ← −g + β·u), then the trial along the new u
    r0, v0 = expected_fused(Quad, d, M_ACCEPT | M_DIR, 0.0, a_acc, beta)
    d2 = _with_u(d, v0["u"])
    r1, _ = expected_fused(Quad, d2, M_BETAONLY, 0.0, 0.0, 0.0, gt_key="gp", f_host=F_ADT)
    out["accept_dir_trial"] = (A(v0["x"], M(a, v0["u"])), np.concatenate([r0, r1]), dict(x=v0["x"], u=v0["u"], g=full["gp"]))
    return out


def _with_u(d, u_full):
    """Data d with another (equally periodic) u"""
    per = dict(stored_period("quad_diag"))
    L = per["u"].size
    per["u"] = np.resize(u_full, L) if u_full.size >= L else np.concatenate([u_full, per["u"][u_full.size:]])
    return Data(d.n, per)


@pytest.mark.gpu
@pytest.mark.parametrize("n", C_SIZES, ids=lambda n: f"n{n}")
def test_host_closure_launches_exact(cgo, contexts, n):
    """A HostObjective whose closure records the vector it is handed (bitwise x at init, x + a·u unfused afterwards — at
    n = 1024·256 + 1 element n − 1 is the only one of k_trial_point's second grid-stride trip), asserts its length and returns
    dyadic g⁺ and f: every slot of the M_BETAONLY row (S_F = f exactly; at init Σ g², Σ g·u, Σ u² = 0 show the zeroed g and u,
    which the probe had filled with NaN), the reset's row and u = −g, accept_dir's row and vectors, bit for bit."""
    d = Data(n, stored_period("quad_diag"))
    want = _host_expected(d)
    a_acc, beta, a = SCAL["quad_diag"]
    mism = []
    seen = {}

    def make(f):
        def fdf(g, x):
            assert x.size == n and g.size == n, (x.size, g.size, n)
            seen["x"] = x.copy()
            g[:] = d.full["gp"]
            return f
        return fdf
    for tail in _tails(n):
        for big in (False, True):
            for kind, f, args, syms in (
                    ("init", F_INIT, (0.0, 0.0, [], d.full["x"], None, None), ("k_trial_point", 128, 32)),
                    ("trial", F_TRIAL, (0.0, 0.0, [a], d.full["x"], d.full["u"], d.full["g"]), ("k_trial_point", 128)),
                    ("accept_dir_trial", F_ADT, (a_acc, beta, [a], d.full["x"], d.full["u"], d.full["g"]), (3, "k_trial_point", 128))):
                o = cgo.HostObjective(make(f), n, contexts[tail])
                s = _solver(cgo, o, tail, big)
                try:
                    seen.clear()
                    got = s.probe_launch(kind, 0, *args)
                    o.reraise()
                    tag = f"host closure n={n} {tail} {'pure-HBM' if big else 'grid-stride'} {kind} [{got['symbol']}]"
                    sym = " + ".join(t if isinstance(t, str) else symbol_for("quad_diag", t, big) for t in syms)
                    xp, row, vec = want[kind]
                    ok = got["symbol"] == sym
                    if not ok:
                        mism.append(f"{tag}: expected {sym}")
                    if "x" not in seen or not np.array_equal(bits(seen["x"]), bits(xp)):
                        i = -1 if "x" not in seen else int(np.nonzero(bits(seen["x"]) != bits(xp))[0][0])
                        mism.append(f"{tag}: the closure's vector differs from the trial point first at element {i}")
                        ok = False
                    ok = ok and K._compare(tag, got, row, vec, mism)
                    _note(got, n, tail, ok)
                finally:
                    s.close(); o.close()
    K._report(mism)


# ---- (d) the norm passes -----------------------------------------------------------------------------------------------------
D_SIZES = [1, 64, 65, 256, 257, K1 + 1]
NORM_SYMS = "k_scaled_norm<0> + k_scaled_norm<1>"


def _dyadic_vec(n, scale, seed):
    """k·scale/8, |k| ≤ 8, some −0.0, exactly one element of magnitude `scale` (a power of two), at a place that depends on n"""
    rng = np.random.default_rng(seed)
    v = rng.integers(-7, 8, n) * (scale / 8)
    v[rng.random(n) < 0.1] = -0.0
    v[(5 * n) // 7] = -scale
    return v


def norm_cases(n):
    """name -> (v, expected maximum, expected NaN count, pass 1 runs)"""
    c = {}
    for name, sc in (("unit", 1.0), ("tiny", 2.0 ** -600), ("huge", 2.0 ** 600)):
        c[name] = (_dyadic_vec(n, sc, 11 + n), sc, 0, True)
    for pos in (0, 63, 64, 255, 256, n - 1):
        if pos < n:
            v = np.zeros(n)
            v[pos] = -0.375
            c[f"single@{pos}"] = (v, 0.375, 0, True)      # (r = ±1 exactly whatever the maximum)
    v = _dyadic_vec(n, 4.0, 5)
    v[n - 1] = np.nan
    c["nan-last"] = (v, float(np.max(np.abs(v[:-1]))) if n > 1 else 0.0, 1, False)
    for name, val in (("+inf", np.inf), ("-inf", -np.inf)):
        v = _dyadic_vec(n, 1.0, 6)
        v[n // 2] = val
        c[name] = (v, np.inf, 0, False)
    c["zero"] = (np.zeros(n), 0.0, 0, False)
    c["minus-zero"] = (np.full(n, -0.0), 0.0, 0, False)
    return c


def norm_depth(n):
    """additions on a term's way through k_scaled_norm<1> + k_finalize_maxsum<1>: a lane's trips, six wave levels, the four
    waves in turn, then the rows one after the other (one lane, fixed order)"""
    grid = min(max(1, -(-n // BLOCK)), GRID_SMALL)
    return -(-n // (grid * BLOCK)) + 6 + 3 + grid


def _norm_probe(s, which, v, other):
    """the vector v as `which` sees it; the other buffers hold `other` (a vector the pass must not read for this `which`)"""
    if which == 0:
        return s.probe_launch("scaled_norm", 0, 0.0, 0.0, [], other, other, v), dict(x=other, u=other, g=None)
    if which == 1:
        return s.probe_launch("scaled_norm", 1, 0.0, 0.0, [], v, other, other), dict(x=None, u=other, g=v)
    return s.probe_launch("scaled_norm", 3, 0.0, 0.0, [], other, v, other), dict(x=other, u=v, g=None)


def _norm_row(v, mx, nans, second):
    row0 = np.zeros(NS)
    row0[0], row0[1] = mx, nans
    if not second:
        return row0
    r = v / mx
    assert np.all(r * mx == v), "test data: v / max is not exact"
    row1 = np.zeros(NS)
    row1[0] = exact_sum([M(r, r)], [np.ones(v.size, np.int64)])
    return np.concatenate([row0, row1])


@pytest.mark.gpu
@pytest.mark.parametrize("n", D_SIZES, ids=lambda n: f"n{n}")
def test_norm_passes_exact(cgo, contexts, n):
    """scaled_norm on g, g⁺, u and g⁺ − g: max|v|, the NaN count, Σ (v/max)² and the eight / nine padding slots bit for bit, on
    vectors near 2⁻⁶⁰⁰ and 2⁶⁰⁰ (why the path exists), a single nonzero at the lane, wave and workgroup boundaries, NaN in the
    last element, ±Inf, zeros, −0.0; pass 1 skipped (10 slots) exactly where the engine skips it; no vector touched."""
    mism = []
    o = cgo.QuadDiag(np.ones(n), contexts["fused"])
    s = _solver(cgo, o, "fused", False)
    other = np.full(n, 3.0)
    try:
        for name, (v, mx, nans, second) in norm_cases(n).items():
            want = _norm_row(np.where(np.isnan(v), 0.0, v), mx, nans, second)
            for which in (0, 1, 3):
                got, vec = _norm_probe(s, which, v, other)
                ok = _norm_compare(f"norm n={n} which={which} {name}", got, want, vec, second, mism)
                _note(got, n, "fused", ok)
            # which = 4: g⁺ − g exact, different from both: g = v + w − … choose g⁺ = v + t, g = t with t on v's grid
            t = np.where(np.isfinite(v), np.ldexp(3.0, int(math.log2(mx)) - 3) if mx not in (0.0, np.inf) else 0.5, 0.0)
            gp = np.where(np.isfinite(v), v + t, v)
            assert np.array_equal(bits((gp - t) + 0.0), bits(v + 0.0)) or np.isnan(v).any(), "test data: g⁺ − g is not v"
            got = s.probe_launch("scaled_norm", 4, 0.0, 0.0, [], gp, other, t)
            ok = _norm_compare(f"norm n={n} which=4 {name}", got, want, dict(x=None, u=other, g=gp), second, mism)
            _note(got, n, "fused", ok)
    finally:
        s.close(); o.close()
    K._report(mism)


def _norm_compare(tag, got, want, vec, second, mism):
    sym = NORM_SYMS if second else "k_scaled_norm<0>"
    if got["symbol"] != sym:
        mism.append(f"{tag}: launched {got['symbol']}, expected {sym}")
        return False
    return K._compare(tag, got, want, vec, mism)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [257, K1 + 1], ids=lambda n: f"n{n}")
def test_norm_passes_random(cgo, contexts, n):
    """Random data: the maximum and the count exact; Σ within (d + 3)·u·Σr² of the correctly rounded sum of the squared
    quotients r = fl(v / max): r·r is one rounding, the d = norm_depth(n) additions one each (d + 1), and the quotient's own
    rounding moves r² by 2u relatively (the + 2 that also covers the distance to Σ (v/max)² in real numbers)."""
    rng = np.random.default_rng(99 + n)
    mism = []
    o = cgo.QuadDiag(np.ones(n), contexts["fused"])
    s = _solver(cgo, o, "fused", False)
    try:
        for which in (0, 1, 3, 4):
            v = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3)
            if which == 4:
                g = rng.standard_normal(n)
                got = s.probe_launch("scaled_norm", 4, 0.0, 0.0, [], v, None, g)
                v = v - g
            else:
                got = _norm_probe(s, which, v, np.full(n, 3.0))[0]
            mx = float(np.max(np.abs(v)))
            r = v / mx
            p, e = two_prod(r, r)
            ref, sq = math.fsum(np.concatenate([p, e])), float(np.sum(p))
            bound = (norm_depth(n) + 3) * 2.0 ** -53 * sq
            row = got["sums"]
            tag = f"norm random n={n} which={which}"
            if row.size != 2 * NS or row[0] != mx or bits(row[1:NS]).any() or bits(row[NS + 1:]).any():
                mism.append(f"{tag}: row {row!r}, maximum {mx!r}")
            elif not abs(row[NS] - ref) <= bound:
                mism.append(f"{tag}: Σ {row[NS]!r} vs {ref!r} (bound {bound:.3e})")
            _note(got, n, "fused", False)
    finally:
        s.close(); o.close()
    K._report(mism)


# ---- (e) kernel-level entries ------------------------------------------------------------------------------------------------
E_SIZES = [1, 2, 513, 1027, 2 * (GRID_BIG * 8 + 1) + 1]


def kernel_level_mismatches(cgo, big):
    """updatedir_ (the only dispatcher of M_DIR alone): u ← −g + β·u and Σ g·u, Σ u² bitwise at five edge sizes; beta_partials:
    all nine sums (GG, GU, UU included).  These entries have no solver: their streaming path is the library's threshold or
    the CGO_BIG_BYTES override read once per process — `big` says which this process runs."""
    mism = []
    for n in E_SIZES:
        d = Data(n, stored_period("quad_diag"))
        want, vec = expected_fused(Quad, d, M_DIR, 0.0, 0.0, 0.75)
        u = d.full["u"].copy()
        gu, uu = cgo.updatedir_(u, d.full["g"], 0.75)
        if not (np.array_equal(bits(u), bits(vec["u"])) and bits(np.array([gu, uu])).tolist() == bits(want[[GU, UU]]).tolist()):
            mism.append(f"updatedir_ n={n}: ({gu!r}, {uu!r}) vs ({want[GU]!r}, {want[UU]!r}) or u differs")
        else:
            REACHED.add(symbol_for("quad_diag", M_DIR, big)); CELLS[(symbol_for("quad_diag", M_DIR, big), n, "entry")] += 1
        want, _ = expected_fused(Quad, d, M_BETAONLY, 0.0, 0.0, 0.0, gt_key="gp")
        got = cgo.beta_partials(d.full["gp"], d.full["g"], d.full["u"])
        want9 = want[[GTU, GTGT, GTG, YY, UY, YGT, GG, GU, UU]]   # out9's order (include/cgo.h)
        if bits(got).tolist() != bits(want9).tolist():
            mism.append(f"beta_partials n={n}: {got!r} vs {want9!r}")
        else:
            REACHED.add(symbol_for("quad_diag", M_BETAONLY, big)); CELLS[(symbol_for("quad_diag", M_BETAONLY, big), n, "entry")] += 1
    return mism


def _env_big():
    try:
        return float(os.environ.get("CGO_BIG_BYTES", "0")) > 0.0
    except ValueError:
        return False


@pytest.mark.gpu
def test_kernel_level_entries_exact(cgo):
    K._report(kernel_level_mismatches(cgo, _env_big()))


@pytest.mark.gpu
def test_kernel_level_entries_exact_pure_hbm():
    """The same in a process started under CGO_BIG_BYTES=1 (the override is read once per process; without it M_DIR alone takes
    the pure-HBM path only above 5.8e7 elements): k_fused<ObjQuadDiag, 2, true> and <…, 128, true> through the entries."""
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport cgo_amd, test_stored_gradient_kernel_sums as T\n"
            "m = T.kernel_level_mismatches(cgo_amd, True)\nprint('\\n'.join(m)); print('ENTRIES', 'FAIL' if m else 'OK')\n"
            % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CGO_BIG_BYTES="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ENTRIES OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    for mode in (M_DIR, M_BETAONLY):
        REACHED.add(symbol_for("quad_diag", mode, True))


# ---- (f) coverage --------------------------------------------------------------------------------------------------------------
def test_dispatch_tables_have_tests():
    """CPU tier: every (objective, mode) launch_obj / launch_any can dispatch — the rows of csrc/cgo_instances.def, from which the
    run-time module's k_fused list is built too — is in this module's launch lists, so that a new instantiation cannot arrive
    untested."""
    assert {m for m, in I.rows("FUSED_OBJ")} == set(OBJ_MODES)
    assert {m for m, in I.rows("FUSED_FREE")} == set(FREE_MODES)
    assert {functor for kind, functor in I.rows("OBJ")} == set(OBJ_NAMES.values()) - {"UserObjective"}
    engine = {mode for _, mode in LAUNCHES}
    assert set(OBJ_MODES) <= engine and set(FREE_MODES) - {M_DIR, M_BETAONLY} <= engine   # those two: (c), (e)


@pytest.mark.gpu
def test_coverage_of_every_instantiation(cgo, contexts):
    """Every k_fused instantiation the library can dispatch × {grid-stride, pure-HBM} was launched by a checked probe or entry.
    What the tests above have not reached (this test on its own) is probed here at one small size; M_DIR alone on the
    pure-HBM path exists only for the kernel-level entry in a process of its own (test_kernel_level_entries_exact_pure_hbm)."""
    ON = {"ObjQuadDiag": (Quad, 17), "ObjRosenPaired": (Rosen, 16), "ObjBooth": (Booth, 2), "UserObjective": (User, 17)}
    want = {f"k_fused<{on}, {m}, {b}>" for on in ON for m in OBJ_MODES for b in ("false", "true")}
    want |= {f"k_fused<ObjQuadDiag, {m}, {b}>" for m in FREE_MODES for b in ("false", "true")}
    mism = []
    for on, (obj, n) in ON.items():
        for big in (False, True):
            todo = [(kd, m) for kd, m in LAUNCHES if symbol_for(obj.name, m, big) not in REACHED]
            if todo:
                mism += _run(cgo, contexts, obj, n, tails=("fused",), bigs=(big,), launch_list=todo)
    if not {symbol_for("quad_diag", M_DIR, _env_big()), symbol_for("quad_diag", M_BETAONLY, _env_big())} <= REACHED:
        mism += kernel_level_mismatches(cgo, _env_big())
    for big in (False, True):
        if symbol_for("quad_diag", M_BETAONLY, big) not in REACHED:   # through a host closure's trial
            d = Data(17, stored_period("quad_diag"))

            def fdf(g, x):
                g[:] = d.full["gp"]
                return F_TRIAL
            o = cgo.HostObjective(fdf, 17, contexts["fused"])
            s = _solver(cgo, o, "fused", big)
            try:
                got = s.probe_launch("trial", 0, 0.0, 0.0, [0.25], d.full["x"], d.full["u"], d.full["g"])
                xp, row, vec = _host_expected(d)["trial"]
                _note(got, 17, "fused", K._compare(f"host trial {got['symbol']}", got, row, vec, mism))
            finally:
                s.close(); o.close()
    if symbol_for("quad_diag", M_DIR, True) not in REACHED:
        test_kernel_level_entries_exact_pure_hbm()
    K._report(mism)
    still = sorted(want - REACHED)
    assert not still, f"{len(still)} instantiations never probed: {still}"
    print(f"\n[stored-gradient kernel sums] {len(CELLS)} (instantiation, size, tail) cells checked bit for bit, "
          f"{sum(CELLS.values())} launches, {VALUES[0]:.3g} values")


@pytest.mark.gpu
def test_probe_refuses_what_the_engine_does_not_issue(cgo, contexts):
    """CGO_EINVAL for a mode of another kind, M_DIR alone, more than one trial step; a probed solver does not start."""
    o = cgo.QuadDiag(np.ones(8), contexts["fused"])
    s = _solver(cgo, o, "fused", False)
    x = np.ones(8)
    try:
        for kind, variant, a in (("trial", M_INIT, [0.5]), ("accept_dir", M_DIR, []), ("trial", M_TRIAL, [0.5, 1.0]), ("trial", M_TRIAL, []),
                                 ("dir_trial", 0, [0.5]), ("scaled_norm", 2, []), ("init", M_BETAONLY, [])):
            with pytest.raises(Exception):
                s.probe_launch(kind, variant, 0.0, 0.0, a, x, x, x)
        s.probe_launch("trial", M_TRIAL, 0.0, 0.0, [0.5], x, x)
        with pytest.raises(Exception):
            s.start()
    finally:
        s.close(); o.close()
