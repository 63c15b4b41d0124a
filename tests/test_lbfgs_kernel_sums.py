"""Every sum slot and every vector of every L-BFGS pass launch, one pass at a time (cgo_solver_probe_lbfgs).

The trajectory suites see the L-BFGS passes only through the numbers the engine reads, and L-BFGS forgives small errors: the
row slots of pairs that do not exist, the padding slots, the ring's padding between slots and the pure-HBM instantiations of
most passes are never looked at there.  Here one pass runs on given x, u, g, g⁺ and whole S / Y rings (absent slots NaN;
every buffer, the rings included, carries NaN slack that the probe checks after the launch), and the whole row, the vectors
and both rings after it are compared with references:

(a) exact dyadic data (the witnesses of test_kernel_sums: every product and element-wise sum asserted exact, every slot's
    terms below 2⁵³ quanta): rows, vectors and rings bit for bit, for every non-log-sum-exp instantiation on both streaming
    paths, counts {0, 1, 3, 4, 5, 8, 9, 10, 11, 12} capped at each kernel's limit, wrapped slot lists (slot ≠ list position)
    and a target slot no list entry names; the deferred push with new_in_list 0 and 1;
(b) random data: u of k_lbfgs_combine (j order) and of k_lbfgs_combine_spec (per-wave partials added in wave order) match a
    numpy restatement bit for bit (the kernels are unfused); every slot within γ_d·Σ|t| of the correctly rounded exact sum,
    d the launch's summation depth, each slot's smallest term asserted above its bound;
(c) the log-sum-exp passes against 50-digit mpmath: g⁺ of k_lbfgs_push_gram_lse with |Δg⁺_k| ≤ 2(p_k(3 + |xp_k − M|)u +
    λ|xp_k|u), p_k = exp(xp_k − M)/S (1 ulp of exp, the rounding of its argument, the division, λ·xp and the final
    addition; the factor 2 covers second-order terms); its slot 63 (Σ g⁺²) and the other sums against the device's own g⁺
    within (γ_d + u)Σ|t|; xo = x + a·u, s, y bit for bit; k_lbfgs_combine_lse's u bit for bit, its statistics through the
    bounds of test_kernel_sums._lse_phi_check; k_lbfgs_combine_spec<ObjLse> without push: S' = Σ exp(xp − M_r) and
    T' = Σ exp(xp − M_r)·u within Σ e_k(2 + |xp_k − M_r|)u + γ_d·Σ|t| of mpmath, the exp-free slots (Q, R, g·u, u·u, y_j·u)
    as plain sums;
(d) the Gram entries lbfgs_push_spec derives from a one-pass row: element-wise (exact data, every entry bit for bit against
    the exact inner products of s = a_s·u, y = ∇f(xp) − g, g⁺ = ∇f(xp)); log-sum-exp (κ-corrected algebra) against 50-digit
    inner products of the true s, y, g⁺, within 1e-12·(Σ|terms|) — asserted far below every entry — and the guard: a trial
    that raises the log-sum-exp by more than log 2 is refused;
(e) sizes from the kernels' own geometry (CPU test: each size hits the edge it claims);
(f) coverage: a CPU test parses the k_lbfgs_* launches of cgo_backend_lbfgs.hip and the run-time compiled names of
    cgo_rtc.hip; a GPU test asserts every instantiation was probed and checked.
"""
import math
import os
import re
from collections import defaultdict

import numpy as np
import pytest

import _instances as I
from test_kernel_sums import (BLOCK, GRID_BIG, NAN_BITS, SIZES, A, M, S as SUB, _dy, _f, _lse_phi_check, big_chunk_pairs,
                              bits, busy_workgroups, exact_sum, lse_reference, two_prod)

CSRC = I.CSRC
NS, NG, GRAM_MAXC, GRAM_MAXC_LSE, SPEC_MAXC, GRID_SMALL = 10, 64, 12, 11, 10, 1024
S_GU, S_UU = 7, 8
COUNTS = (0, 1, 3, 4, 5, 8, 9, 10, 11, 12)
U53 = 2.0 ** -53


# ---- (e) sizes -----------------------------------------------------------------------------------------------------------
def grid_for(n):
    n2 = n >> 1
    return max(1, min(GRID_SMALL, -(-n2 // (BLOCK * 2))))


def lse_round_trips(n2, big):
    """k_lbfgs_push_gram_lse: for every busy workgroup, the number of pairs each of its four 64-pair trips holds in its last
    round (pure-HBM: the chunk's; grid-stride: workgroup 0's)."""
    per = big_chunk_pairs(n2) if big else n2
    last = per % 256 if per % 256 else 256
    return [max(0, min(64, last - 64 * w)) for w in range(4)]


def _lbfgs_sizes():
    s = dict(SIZES)
    s[2 * (128 + 10)] = "grid-stride, one workgroup: trips 0, 1 of the four-trip round full, trip 2 partial, trip 3 empty"
    s[2 * (128 + 10) + 1] = s[2 * (128 + 10)] + ", odd tail element"
    n2 = GRID_BIG * 64 + 1
    s[2 * n2 + 1] = "pure-HBM: chunks of 72 pairs, trip 0 full, trip 1 partial (8 pairs), trips 2, 3 empty; odd tail element"
    s[1024] = "ring stride: n mod 16 = 0"
    s[1025] = "ring stride: n mod 16 = 1"
    s[1039] = "ring stride: n mod 16 = 15"
    return s


LSIZES = _lbfgs_sizes()
SMALL = sorted(n for n in LSIZES if n <= 1039)
LARGE = sorted(n for n in LSIZES if n > 1039)


def test_sizes_hit_the_edges_they_claim():
    """CPU tier: the L-BFGS size table's claims follow from the geometry constants."""
    assert lse_round_trips(138, False) == [64, 64, 10, 0]
    n2 = GRID_BIG * 64 + 1
    assert big_chunk_pairs(n2) == 72 and lse_round_trips(n2, True) == [64, 8, 0, 0] and busy_workgroups(n2) < GRID_BIG
    assert {n % 16 for n in LSIZES} >= {0, 1, 15}
    assert any(n & 1 for n in LSIZES) and min(LSIZES) == 1
    for j in (1, 2):
        assert 2 * (GRID_BIG * 8 * j) in LSIZES and 2 * (GRID_BIG * 8 * j + 1) + 1 in LSIZES


# ---- slot lists and data -------------------------------------------------------------------------------------------------
def slot_list(count, P, target):
    """newest first, wrapping below slot 0: no entry is the target, position j holds slot (target − 1 − j) mod P"""
    assert count < P
    return [(target - 1 - j) % P for j in range(count)]


def exact_inputs(n, P, seed, listed, lite_slot=None):
    rng = np.random.default_rng(seed)
    d = dict(x=_dy(rng, n, -8, 8, 0.25), u=_dy(rng, n, -6, 6, 0.25), g=_dy(rng, n, -8, 8, 0.25), gt=_dy(rng, n, -8, 8, 0.25),
             p=rng.integers(1, 3, n).astype(np.float64))
    Sr, Yr = np.full((P, n), np.nan), np.full((P, n), np.nan)
    for q in listed:
        if q != lite_slot:
            Sr[q], Yr[q] = _dy(rng, n, -4, 4, 0.25), _dy(rng, n, -4, 4, 0.25)
    d["S"], d["Y"] = Sr, Yr
    return d


def random_inputs(n, P, seed, listed, lse=False):
    """one sign per element for every vector (x, u, g⁺, rings positive; g negative), magnitudes in [1/2, 1]: every term of
    every slot keeps away from zero, y = g⁺ − g > 0"""
    rng = np.random.default_rng(seed)
    U = lambda lo, hi: rng.uniform(lo, hi, n)
    d = dict(x=U(0.5, 1), u=U(0.5, 1), g=-U(0.5, 1), gt=U(0.5, 1), p=U(1, 2))
    Sr, Yr = np.full((P, n), np.nan), np.full((P, n), np.nan)
    for q in listed:
        Sr[q], Yr[q] = U(0.5, 1), U(0.5, 1)
    d["S"], d["Y"] = Sr, Yr
    return d


COEF = dict(a=0.5, a_s=0.25, a_trial=0.75, cg=-1.0, rho=0.5, scale=0.75, dot_host=1.25)


def coefs(count):
    return [0.125 * (j + 1) for j in range(count)], [-0.25 * (1 + (j % 3)) for j in range(count)]


# ---- models (csrc/cgo_kernels.hip.hpp, unfused, in the kernels' order) -----------------------------------------------------
class Quad:
    name, kind = "quad_diag", "ObjQuadDiag"

    @staticmethod
    def grad(x, p, exact):
        g = M(p, x) if exact else p * x
        f = M(0.5, M(g, x)) if exact else 0.5 * (g * x)
        return f, g


class User(Quad):
    name, kind = "user_quad", "UserObjective"
    SOURCE = "gi = p*x; fi = 0.5*(gi*x);"


class Rosen:
    """kPairOnly: eval2 per pair (f of the pair in one sum), even n only"""
    name, kind = "rosenbrock_paired", "ObjRosenPaired"

    @staticmethod
    def grad(x, p, exact):
        mul, add, sub = _ops(exact)
        xe, xo = x[0::2], x[1::2]
        t1 = sub(xo, mul(xe, xe))
        t2 = sub(1.0, xe)
        g = np.empty_like(x)
        g[0::2] = sub(mul(-400.0, mul(xe, t1)), mul(2.0, t2))
        g[1::2] = mul(200.0, t1)
        f = np.zeros_like(x)
        f[0::2] = add(mul(100.0, mul(t1, t1)), mul(t2, t2))
        return f, g


def rosen_exact_inputs(n, P, seed, listed):
    """the quartic's budget: x, g on a 1/2 grid in [−1, 1], u and the (sparse) ring in {−1, 0, 1}; with the coefficients of
    pass_params every trial point stays on a 1/2 grid, so that ∇f has ≤ 25 significant bits and every product is exact"""
    rng = np.random.default_rng(seed)
    d = dict(x=_dy(rng, n, -2, 2, 0.5, False), u=_dy(rng, n, -1, 1, 1.0, False), g=_dy(rng, n, -2, 2, 0.5, False),
             gt=_dy(rng, n, -2, 2, 0.5, False), p=np.ones(n))
    Sr, Yr = np.full((P, n), np.nan), np.full((P, n), np.nan)
    for q in listed:
        Sr[q] = _dy(rng, n, -1, 1, 1.0, False) * (rng.uniform(0, 1, n) < 0.25)
        Yr[q] = _dy(rng, n, -1, 1, 1.0, False) * (rng.uniform(0, 1, n) < 0.25)
    d["S"], d["Y"] = Sr + 0.0, Yr + 0.0
    return d


def pass_params(obj, c, push=False):
    """(cy, cs, cg, a_trial, a_lite, a_s_lite) of one pass: the quadratic takes the general coefficients; the quartic ±1/2,
    a unit trial step, and under the deferred push no g in u and no cy·y for the pair formed in registers"""
    if obj is not Rosen:
        cy, cs = coefs(c)
        return cy, cs, COEF["cg"], COEF["a_trial"], 0.25, 0.5
    cy = [0.5 * (-1) ** j for j in range(c)]
    cs = [-0.5 * (-1) ** j for j in range(c)]
    if push and c:
        cy[0] = 0.0
    return cy, cs, (0.0 if push else -1.0), 1.0, 0.5, 1.0


def _ops(exact):
    return (M, A, SUB) if exact else (lambda a, b: _f(a) * _f(b), lambda a, b: _f(a) + _f(b), lambda a, b: _f(a) - _f(b))


def model_push(d, a, a_s, slot, lst, exact, gram):
    mul, add, sub = _ops(exact)
    s, y = mul(a_s, d["u"]), sub(d["gt"], d["g"])
    out = dict(x=add(d["x"], mul(a, d["u"])), S=d["S"].copy(), Y=d["Y"].copy())
    out["S"][slot], out["Y"][slot] = s, y
    T = {0: [(s, y)], 1: [(y, y)], 2: [(s, d["gt"])]}
    if gram:
        T[3] = [(y, d["gt"])]
        for j, q in enumerate(lst):
            Sj, Yj = d["S"][q], d["Y"][q]
            for k, (l, r) in enumerate(((Sj, d["gt"]), (Yj, d["gt"]), (Sj, y), (Yj, s), (Yj, y))):
                T[4 + 5 * j + k] = [(l, r)]
    return T, out, (NG if gram else NS)


def combine_u(d, lst, cy, cs, cg, exact, waves=None, ring=None):
    """u = cg·g + Σ_j (cy_j·y_j + cs_j·s_j): in j order (waves None) or as four per-wave partials (wave w: pairs j ≡ w mod 4,
    wave 0 starting from cg·g) added in wave order"""
    mul, add, _ = _ops(exact)
    Sr, Yr = ring if ring is not None else (d["S"], d["Y"])
    if waves is None:
        r = mul(cg, d["g"])
        for j, q in enumerate(lst):
            r = add(r, mul(cy[j], Yr[q] if not callable(Yr) else Yr(j)))
            r = add(r, mul(cs[j], Sr[q] if not callable(Sr) else Sr(j)))
        return r
    parts = []
    for w in range(4):
        r = mul(cg, d["g"]) if w == 0 else np.zeros_like(d["g"])
        for j in range(w, len(lst), 4):
            yj = Yr(j) if callable(Yr) else Yr[lst[j]]
            sj = Sr(j) if callable(Sr) else Sr[lst[j]]
            r = add(r, mul(cy[j], yj))
            r = add(r, mul(cs[j], sj))
        parts.append(r)
    u = parts[0]
    for w in (1, 2, 3):
        u = add(u, parts[w])
    return u


def model_combine(d, lst, cy, cs, cg, exact):
    u = combine_u(d, lst, cy, cs, cg, exact)
    return {S_GU: [(d["g"], u)], S_UU: [(u, u)]}, dict(x=d["x"], u=u, S=d["S"], Y=d["Y"]), NS


def model_spec(obj, d, lst, cy, cs, cg, a_trial, exact, push=None):
    """k_lbfgs_combine_spec<element-wise objective, ·, PUSH>; push = (a, a_s, lite_slot, new_in_list)"""
    mul, add, sub = _ops(exact)
    out = dict(S=d["S"].copy(), Y=d["Y"].copy())
    x, g = d["x"], d["g"]
    Sfun, Yfun = (lambda j: d["S"][lst[j]]), (lambda j: d["Y"][lst[j]])
    if push is not None:
        a, a_s, ls, nil = push
        x = add(x, mul(a, d["u"]))
        _, gp = obj.grad(x, d["p"], exact)
        sn, yn = mul(a_s, d["u"]), sub(gp, g)
        g = gp
        out["S"][ls], out["Y"][ls] = sn, yn
        if nil:
            Sfun = lambda j: sn if j == 0 else d["S"][lst[j]]
            Yfun = lambda j: yn if j == 0 else d["Y"][lst[j]]
    dd = dict(d, g=g)
    u = combine_u(dd, lst, cy, cs, cg, exact, waves=True, ring=(Sfun, Yfun))
    xp = add(x, mul(a_trial, u))
    f, gt = obj.grad(xp, d["p"], exact)
    y = sub(gt, g)
    fp = f.copy()
    if obj is not Rosen:   # eval2: f of the pair = f_even + f_odd (one rounding), the odd tail element alone
        n2 = f.size >> 1
        fp = np.concatenate([add(f[0:2 * n2:2], f[1:2 * n2:2]), f[2 * n2:]])
    else:
        fp = f[0::2]
    T = {0: [(fp,)], 1: [(gt, u)], 2: [(gt, gt)], 3: [(y, gt)], 4: [(u, y)], 5: [(g, u)], 6: [(u, u)], 7: [(y, y)]}
    for j in range(len(lst)):
        sj, yj = Sfun(j), Yfun(j)
        for k, (l, r) in enumerate(((sj, gt), (yj, gt), (sj, y), (yj, y), (yj, u))):
            T[13 + 5 * j + k] = [(l, r)]
    out.update(x=x, u=u, g=g)
    return T, out, NG, dict(xp=xp, gt=gt, y=y)


def model_lite(obj, d, a, a_s, slot, exact):
    mul, add, sub = _ops(exact)
    x = add(d["x"], mul(a, d["u"]))
    _, gt = obj.grad(x, d["p"], exact)
    out = dict(x=x, g=gt, S=d["S"].copy(), Y=d["Y"].copy())
    out["S"][slot], out["Y"][slot] = mul(a_s, d["u"]), sub(gt, d["g"])
    return {}, out, 0


def model_loop(d, lp, exact):
    mul, add, _ = _ops(exact)
    vec = lambda ring, slot: d["g"] if ring == 2 else (d["S"] if ring == 0 else d["Y"])[slot]
    dot = lp["dot_host"]
    if lp.get("dots") is not None:
        dot = 0.0
        for row in lp["dots"]:
            dot = dot + row[S_GU]
    alpha = np.array(lp["alpha"], dtype=np.float64)
    coef = 0.0
    if lp["loop_mode"] == 0:
        coef = lp["rho"] * dot
        alpha[lp["k"]] = coef
    elif lp["loop_mode"] == 1:
        coef = alpha[lp["k"]] - lp["rho"] * dot
    q = d["g"] if lp["q_from_g"] else d["u"]
    T = {}
    out = dict(x=d["x"], u=d["u"], S=d["S"], Y=d["Y"], alpha=alpha)
    if lp["loop_mode"] != 2:
        v = vec(lp["v_ring"], lp["v_slot"])
        q = add(q, mul(-coef if lp["loop_mode"] == 0 else coef, v)) if not exact else \
            (SUB(q, M(coef, v)) if lp["loop_mode"] == 0 else A(q, M(coef, v)))
        if lp["apply_scale"]:
            q = mul(lp["scale"], q)
        if lp["final_step"]:
            q = -q
            T[S_UU] = [(q, q)]
        out["u"] = q
    T[S_GU] = [(vec(lp["w_ring"], lp["w_slot"]), q)]
    return T, out, NS


# ---- comparison ----------------------------------------------------------------------------------------------------------
def exact_row(T, W):
    row = np.zeros(W)
    for slot, terms in T.items():
        arrs = [M(*t) if len(t) == 2 else _f(t[0]) for t in terms]
        row[slot] = exact_sum(arrs, [np.ones(a.size, np.int64) for a in arrs])
    return row


def depth(n, big):
    """longest chain of roundings a term goes through: the lane's own accumulation (64-lane trips of the wave-split kernels
    are the longest: two terms per pair), the odd element, six wave levels, the four waves, the row levels"""
    n2 = n >> 1
    grid = GRID_BIG if big else grid_for(n)
    per_lane = -(-big_chunk_pairs(n2) // 64) if big else -(-n2 // (grid * 64))
    return 2 * per_lane + 1 + 6 + 3 + 2 * (math.ceil(math.log2(max(grid, 2))) + 6)


def slot_refs(T):
    out = {}
    for slot, terms in T.items():
        parts, mags = [], []
        for t in terms:
            if len(t) == 2:
                pp, ee = two_prod(*np.broadcast_arrays(_f(t[0]), _f(t[1])))
                parts += [pp, ee]
            else:
                pp = _f(t[0])
                parts.append(pp)
            mags.append(np.abs(pp).ravel())
        m = np.concatenate(mags)
        out[slot] = (math.fsum(np.concatenate([q.ravel() for q in parts])), float(np.sum(m)), float(np.min(m)) if m.size else 0.0)
    return out


def _vec_mismatch(tag, key, got, want, mism):
    wb = np.full(got.shape, NAN_BITS) if want is None else bits(np.broadcast_to(want, got.shape))
    gb = bits(got)
    if not np.array_equal(gb, wb):
        i = np.unravel_index(int(np.argmax(gb.ravel() != wb.ravel())), got.shape)
        mism.append(f"{tag}: {key} differs first at {tuple(int(v) for v in i)}: got {got[i]!r}, want "
                    f"{'NaN' if want is None else np.broadcast_to(want, got.shape)[i]!r}")
        return False
    return True


def check(tag, got, T, W, out, exact, n, big, mism, keys=("x", "u", "g", "gt", "S", "Y"), d=None):
    ok = True
    if got["sums"].size != W:
        mism.append(f"{tag}: row of {got['sums'].size} slots, expected {W}")
        return False
    if exact:
        want = exact_row(T, W)
        if not np.array_equal(bits(got["sums"]), bits(want)):
            bad = list(np.nonzero(bits(got["sums"]) != bits(want))[0])
            mism.append(f"{tag}: slots differing {bad[:12]}: got {[got['sums'][i] for i in bad[:4]]} want {[want[i] for i in bad[:4]]}")
            ok = False
    else:
        dd = depth(n, big)
        gam = dd * U53 / (1 - dd * U53)
        refs = slot_refs(T)
        for slot in range(W):
            v = got["sums"][slot]
            if slot not in refs:
                if v != 0.0:
                    mism.append(f"{tag}: slot {slot} carries no term, holds {v!r}")
                    ok = False
                continue
            ex, absum, tmin = refs[slot]
            bound = gam * absum * (1 + 1e-12)
            assert tmin > bound, f"test data: {tag} slot {slot}: smallest term {tmin:.3e} within the bound {bound:.3e}"
            if not abs(v - ex) <= bound:
                mism.append(f"{tag}: slot {slot} {v!r} vs {ex!r} (bound {bound:.3e})")
                ok = False
    for key in keys:
        want = out.get(key, None if d is None else d.get(key))
        if key in ("S", "Y") or want is not None or (d is not None and d.get(key) is not None):
            ok = _vec_mismatch(tag, key, got[key], want, mism) and ok
    return ok


# ---- GPU ---------------------------------------------------------------------------------------------------------------
REACHED = set()
CELLS = defaultdict(int)


def _solver(cgo, obj, m, big, form=None, fuse_grad=None):
    pol = cgo.SolverPolicy(resident=False, controller_depth=0, hbm_stream_bytes=1.0 if big else None, lbfgs_form=form,
                           lbfgs_fuse_grad=fuse_grad)
    cfg = cgo.setupCGConfig(1e-9, cgo.LBFGS(m), cgo.DisableTrace(), max_iters=5)
    return cgo.Solver(obj, cfg, cgo.setupStrongWolfeBisection(1e-5, 0.9), pol)


def _objective(cgo, kind, n, p, lam=1e-3):
    if kind is Quad:
        return cgo.QuadDiag(p)
    if kind is User:
        return cgo.ElementwiseObjective(n, User.SOURCE, param=p)
    if kind is Rosen:
        return cgo.RosenbrockPaired(n)
    return cgo.LogSumExp(n, lam)


def _report(mism):
    assert not mism, f"{len(mism)} pass(es) differ from the reference:\n" + "\n".join(mism[:20])


def _note(got, ok, n, exact):
    """the instantiations of a pass whose whole row and every vector were compared (REACHED: coverage), and the cells that
    matched bit for bit"""
    REACHED.update(got["symbols"])
    if ok and exact:
        for s in got["symbols"]:
            CELLS[(s, n)] += 1


def run_elementwise(cgo, obj, n, big, m, counts, exact=True, passes=("push_gram", "direction_gram", "direction_trial",
                                                                      "push_lite", "deferred0", "deferred1")):
    """the Gram / one-pass passes of an element-wise objective at history size m"""
    mism = []
    P = m + 1
    target = 3 % P
    seed = 1000 + n
    lst_all = slot_list(min(m, max(counts)), P, target)
    d = (rosen_exact_inputs if obj is Rosen and exact else exact_inputs if exact else random_inputs)(n, P, seed, lst_all)
    o = _objective(cgo, obj, n, d["p"])
    s = _solver(cgo, o, m, big)
    path = "pure-HBM" if big else "grid"
    try:
        for c in counts:
            if c > m:
                continue
            lst = lst_all[:c]
            cy, cs, cg, a_tr, a_lite, as_lite = pass_params(obj, c)
            vec = dict(x=d["x"], u=d["u"], g=d["g"], gt=d["gt"], S=d["S"], Y=d["Y"])
            for ps in passes:
                tag = f"{obj.name} m={m} n={n} {path} {ps} count={c}"
                if ps == "push_gram" and c <= GRAM_MAXC:
                    got = s.probe_lbfgs("push_gram", **vec, a=COEF["a"], a_s=COEF["a_s"], slot=target, list=lst)
                    T, out, W = model_push(d, COEF["a"], COEF["a_s"], target, lst, exact, True)
                elif ps == "direction_gram" and c <= GRAM_MAXC:
                    got = s.probe_lbfgs("direction_gram", **vec, list=lst, cy=cy, cs=cs, cg=cg)
                    T, out, W = model_combine(d, lst, cy, cs, cg, exact)
                elif ps == "direction_trial" and m <= SPEC_MAXC:
                    got = s.probe_lbfgs("direction_trial", **vec, list=lst, cy=cy, cs=cs, cg=cg, a_trial=a_tr)
                    T, out, W, _ = model_spec(obj, d, lst, cy, cs, cg, a_tr, exact)
                elif ps == "push_lite" and m <= SPEC_MAXC:
                    got = s.probe_lbfgs("push_lite", **vec, a=COEF["a"], a_s=COEF["a_s"], slot=target)
                    T, out, W = model_lite(obj, d, COEF["a"], COEF["a_s"], target, exact)
                elif ps in ("deferred0", "deferred1") and m <= SPEC_MAXC and c >= 1 and c < m:
                    nil = ps == "deferred1"
                    # new_in_list 1: the new pair is list[0] (its ring slot NaN: it must come from registers); 0: it did not
                    # join the history, its slot is the free one behind the list
                    lite = lst[0] if nil else (target - 1 - c) % P
                    vv = dict(vec)
                    if nil:
                        vv["S"], vv["Y"] = d["S"].copy(), d["Y"].copy()
                        vv["S"][lite], vv["Y"][lite] = np.nan, np.nan
                    dd = dict(d, S=vv["S"], Y=vv["Y"])
                    cy, cs, cg, a_tr, a_lite, as_lite = pass_params(obj, c, push=True)
                    got = s.probe_lbfgs("direction_trial", **vv, list=lst, cy=cy, cs=cs, cg=cg, a_trial=a_tr,
                                        deferred_push=1, lite_slot=lite, a_lite=a_lite, a_s_lite=as_lite, M_lite=0.0, S_lite=1.0)
                    if got["new_in_list"] != int(nil):
                        mism.append(f"{tag}: new_in_list {got['new_in_list']}, expected {int(nil)}")
                    T, out, W, _ = model_spec(obj, dd, lst, cy, cs, cg, a_tr, exact, push=(a_lite, as_lite, lite, nil))
                else:
                    continue
                tag += f" [{' + '.join(got['symbols'])}]"
                ok = check(tag, got, T, W, out, exact, n, big, mism, d=d)
                _note(got, ok, n, exact)
    finally:
        s.close(); o.close()
    return mism


def run_two_loop(cgo, obj, n, big, exact=True, m=13):
    """k_lbfgs_push and one k_lbfgs_loop launch for each (mode, final_step, apply_scale) the two-loop issues, with the dot
    from the host, from one device row and from a block of three rows"""
    mism = []
    P = m + 1
    target = 3
    lst = slot_list(m, P, target)
    d = (exact_inputs if exact else random_inputs)(n, P, 3000 + n, lst)
    o = _objective(cgo, obj, n, d["p"])
    s = _solver(cgo, o, m, big)
    path = "pure-HBM" if big else "grid"
    vec = dict(x=d["x"], u=d["u"], g=d["g"], gt=d["gt"], S=d["S"], Y=d["Y"])
    try:
        got = s.probe_lbfgs("push", **vec, a=COEF["a"], a_s=COEF["a_s"], slot=target)
        T, out, W = model_push(d, COEF["a"], COEF["a_s"], target, [], exact, False)
        tag = f"{obj.name} m={m} n={n} {path} push [{' + '.join(got['symbols'])}]"
        _note(got, check(tag, got, T, W, out, exact, n, big, mism, d=d), n, exact)
        alpha = [0.25 * (k + 1) for k in range(64)]
        rows = np.zeros((3, NS))
        rows[:, S_GU] = [0.5, -1.25, 2.0]
        loops = [(2, 0, 0, 1, 2, 0, lst[0]), (0, 0, 0, 1, 1, 0, lst[1]), (0, 0, 1, 0, 1, 1, lst[-1]), (1, 0, 0, 0, 0, 1, lst[2]),
                 (1, 1, 0, 0, 0, 2, 0)]
        for mode, final, scale, qg, vring, wring, wslot in loops:
            for src in ("host", "row", "block"):
                k = 5
                lp = dict(loop_mode=mode, final_step=final, apply_scale=scale, k=k, q_from_g=qg, v_ring=vring, v_slot=lst[k],
                          w_ring=wring, w_slot=wslot, rho=COEF["rho"], scale=COEF["scale"], dot_host=COEF["dot_host"], alpha=alpha)
                if src != "host":
                    lp["dots"] = rows[:1] if src == "row" else rows
                got = s.probe_lbfgs("loop", **vec, **lp)
                T, out, W = model_loop(d, dict(lp, dots=lp.get("dots")), exact)
                tag = f"{obj.name} n={n} {path} loop mode={mode} final={final} scale={scale} dot={src} [{' + '.join(got['symbols'])}]"
                ok = check(tag, got, T, W, out, exact, n, big, mism, d=d)
                ok = _vec_mismatch(tag, "alpha", got["alpha"], out["alpha"], mism) and ok
                _note(got, ok, n, exact)
    finally:
        s.close(); o.close()
    return mism


class _ModelOnly:
    """stands in for cgo in the CPU-tier precondition test: every probe returns a zero row of the pass's width, so that the
    run functions build every exact reference (asserting its exactness witnesses) without a GPU"""
    WIDTH = {"push": NS, "push_gram": NG, "direction_gram": NS, "direction_trial": NG, "push_lite": 0, "loop": NS}

    class _S:
        def __init__(self, *a, **k):
            pass

        def probe_lbfgs(self, pass_name, **kw):
            n = kw["x"].size
            P = kw["S"].shape[0] if kw.get("S") is not None else 1
            nil = int(bool(kw.get("deferred_push")) and len(kw.get("list", [])) > 0 and kw["list"][0] == kw.get("lite_slot"))
            return dict(sums=np.zeros(_ModelOnly.WIDTH[pass_name]), symbols=[], new_in_list=nil, alpha=np.zeros(64),
                        S=np.zeros((P, n)), Y=np.zeros((P, n)), **{k: np.zeros(n) for k in ("x", "xo", "u", "g", "gt")})

        def close(self):
            pass

    def __getattr__(self, name):
        return self._S


def test_exact_data_meet_their_preconditions():
    """CPU tier: every exact reference of (a) — each objective, pass, count and size class, both history forms — is exact
    and order-independent (the witnesses assert it), run here so that an edit to the data fails without a GPU"""
    fake = _ModelOnly()
    for n in (1, 17, 276, 277, 1039, 2 * (GRID_BIG + 5) + 1, 2 * (GRID_BIG * 8 * 2 + 1) + 1):
        for obj in (Quad, Rosen):
            if obj is Rosen and n & 1:
                continue
            run_elementwise(fake, obj, n, False, 10, COUNTS)
            run_elementwise(fake, obj, n, False, 12, (11, 12), passes=("push_gram", "direction_gram"))
        run_two_loop(fake, Quad, n, False)
    n = max(LSIZES)
    run_elementwise(fake, Quad, n, False, 10, (5, 10))
    run_elementwise(fake, Rosen, n - 1, False, 10, (5, 10))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL, ids=lambda n: f"n{n}")
def test_quad_exact_every_slot(cgo, n):
    """(a) QuadDiag at every small size: one-pass form (m = 10), Gram form at counts 11 and 12 (m = 12), two-loop (m = 13),
    both streaming paths, every count."""
    mism = []
    for big in (False, True):
        mism += run_elementwise(cgo, Quad, n, big, 10, COUNTS)
        mism += run_elementwise(cgo, Quad, n, big, 12, (11, 12), passes=("push_gram", "direction_gram"))
        mism += run_two_loop(cgo, Quad, n, big)
        if n % 2 == 0:   # (the paired objective: even n)
            mism += run_elementwise(cgo, Rosen, n, big, 10, COUNTS, passes=("direction_trial", "push_lite", "deferred0", "deferred1"))
    _report(mism)


@pytest.mark.gpu
@pytest.mark.parametrize("n", LARGE, ids=lambda n: f"n{n}")
def test_quad_exact_large(cgo, n):
    """(a) the large sizes (pure-HBM chunk edges, partial four-trip rounds): one or two counts per pass."""
    mism = []
    for big in (False, True):
        mism += run_elementwise(cgo, Quad, n, big, 10, (5, 10))
        mism += run_elementwise(cgo, Quad, n, big, 12, (12,), passes=("push_gram", "direction_gram"))
        mism += run_two_loop(cgo, Quad, n, big)
        mism += run_elementwise(cgo, Rosen, n - (n & 1), big, 10, (5, 10), passes=("direction_trial", "push_lite", "deferred0",
                                                                                    "deferred1"))
    _report(mism)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 277, 1025], ids=lambda n: f"n{n}")
def test_user_module_exact(cgo, n):
    """(a) the run-time compiled k_lbfgs_combine_spec / k_lbfgs_push_lite of an ElementwiseObjective"""
    mism = []
    for big in (False, True):
        mism += run_elementwise(cgo, User, n, big, 10, (0, 4, 9, 10),
                                passes=("direction_trial", "push_lite", "deferred0", "deferred1"))
    _report(mism)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [(Quad, 513), (Quad, 2 * (GRID_BIG + 5) + 1), (User, 1025)],
                         ids=lambda v: getattr(v, "name", str(v)))
def test_random_within_summation_bound(cgo, kind, n):
    """(b) random data: u and every written vector bit for bit against the numpy restatement (j order for k_lbfgs_combine,
    per-wave partials in wave order for k_lbfgs_combine_spec), every slot within γ_d·Σ|t| of the correctly rounded sum"""
    mism = []
    for big in (False, True):
        mism += run_elementwise(cgo, kind, n, big, 10, (3, 10), exact=False)
        if kind is Quad:
            mism += run_two_loop(cgo, kind, n, big, exact=False)
    _report(mism)


# ---- (c) log-sum-exp -----------------------------------------------------------------------------------------------------
def _mp_softmax_terms(xp, M, S, lam):
    import mpmath as mp
    mp.mp.dps = 50
    return np.array([float(mp.e ** (mp.mpf(float(v)) - mp.mpf(float(M))) / mp.mpf(float(S)) + mp.mpf(lam) * mp.mpf(float(v)))
                     for v in xp])


def _plain_sums(tag, row, terms, gam, mism):
    for slot, (l, r) in terms.items():
        p, ee = two_prod(*np.broadcast_arrays(_f(l), _f(r)))
        ex = math.fsum(np.concatenate([p, ee]))
        bound = (gam + U53) * float(np.sum(np.abs(p))) * 1.01 + 1e-300
        if not abs(row[slot] - ex) <= bound:
            mism.append(f"{tag}: slot {slot} {row[slot]!r} vs {ex!r} (bound {bound:.2e})")


def lse_data(n, P, lst, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, n)
    x[n // 3] = 3.0
    d = dict(x=x, u=rng.uniform(-1, 1, n), g=rng.uniform(-0.1, 0.1, n), gt=None)
    Sr, Yr = np.full((P, n), np.nan), np.full((P, n), np.nan)
    for q in lst:
        Sr[q], Yr[q] = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    d["S"], d["Y"] = Sr, Yr
    return d


def _mp_exp(v, M):
    import mpmath as mp
    mp.mp.dps = 50
    Mm = mp.mpf(float(M))
    return np.array([float(mp.e ** (mp.mpf(float(t)) - Mm)) for t in v])


def lse_spec_row_check(tag, got, x, g, u, ring, c, lam, Mr, a_trial, n, big, mism):
    """Every slot of a k_lbfgs_combine_spec<ObjLse, …> row.  The element values are propagated with error bounds from
    e_k = exp(xp_k − M_r) at 50 digits (u = 2⁻⁵³): δe_k ≤ e_k(|xp_k − M_r| + |M_r| + 2.5)u (the rounded argument, 1 ulp of exp,
    the reference's own rounding), p = e (1/S_r = 1), δĝ = δp + u(|λxp| + |ĝ|), δŷ = δĝ + u|ŷ|; x, xp, g, u and the ring
    vectors are exact (u, x, g are the device's own, checked bit for bit before).  Each slot Σ l·r must lie within
    2·(Σ(δl|r| + |l|δr + δlδr) + (γ_d + u)Σ|l·r|) of the correctly rounded sum of the reference products; slot 0 (Σ e) within
    2·(Σδe + γ_d·Σe); every slot of a pair beyond `c` is zero."""
    xp = x + a_trial * u
    e = _mp_exp(xp, Mr)
    ee = e * (np.abs(xp - Mr) + abs(Mr) + 2.5) * U53
    gh = e + lam * xp
    egh = ee + U53 * (np.abs(lam * xp) + np.abs(gh))
    yh = gh - g
    eyh = egh + U53 * np.abs(yh)
    z = np.zeros(n)
    V = dict(p=(e, ee), xp=(xp, z), u=(u, z), g=(g, z), gh=(gh, egh), yh=(yh, eyh))
    T = {0: ("p",), 1: ("p", "u"), 2: ("xp", "xp"), 3: ("xp", "u"), 4: ("gh", "gh"), 5: ("g", "u"), 6: ("u", "u"),
         7: ("yh", "yh"), 8: ("yh", "p"), 9: ("p", "p"), 10: ("u", "yh"), 11: ("p", "xp"), 12: ("yh", "xp"), 63: ("gh", "p")}
    Sf, Yf = ring
    for j in range(c):
        V[f"s{j}"], V[f"y{j}"] = (Sf(j), z), (Yf(j), z)
        for q, (l, r) in enumerate(((f"s{j}", "yh"), (f"s{j}", "p"), (f"y{j}", "yh"), (f"y{j}", "p"), (f"y{j}", "u"))):
            T[13 + 5 * j + q] = (l, r)
    gam = depth(n, big) * U53 * 1.01
    row = got["sums"]
    if row.size != NG:
        mism.append(f"{tag}: row of {row.size} slots, expected {NG}")
        return False
    ok = True
    for slot in range(NG):
        if slot not in T:
            if row[slot] != 0.0:
                mism.append(f"{tag}: padding slot {slot} holds {row[slot]!r}")
                ok = False
            continue
        t = T[slot]
        if len(t) == 1:
            v, err = V[t[0]]
            ref, bound = math.fsum(v), float(np.sum(err)) + gam * float(np.sum(np.abs(v)))
        else:
            (lv, le), (rv, rerr) = V[t[0]], V[t[1]]
            pp, pe = two_prod(lv, rv)
            ref = math.fsum(np.concatenate([pp, pe]))
            bound = float(np.sum(le * np.abs(rv) + np.abs(lv) * rerr + le * rerr)) + (gam + U53) * float(np.sum(np.abs(pp)))
        if not abs(row[slot] - ref) <= 2 * bound + 1e-300:
            mism.append(f"{tag}: slot {slot} {row[slot]!r} vs {ref!r} (bound {2 * bound:.2e})")
            ok = False
    return ok


def _lse_grad_ok(tag, gv, xn, M, S, lam, mism):
    """g⁺_k = exp(xn_k − M)/S + λ·xn_k within 2(p_k(3 + |xn_k − M|)u + λ|xn_k|u) of 50 digits"""
    gref = _mp_softmax_terms(xn, M, S, lam)
    p = np.exp(xn - M) / S
    tol = 2 * (p * (3 + np.abs(xn - M)) * U53 + lam * np.abs(xn) * U53)
    bad = np.nonzero(~(np.abs(gv - gref) <= tol))[0]
    if bad.size:
        mism.append(f"{tag}: g⁺[{bad[0]}] {gv[bad[0]]!r} vs {gref[bad[0]]!r} (tol {tol[bad[0]]:.2e})")
        return False
    return True


def lse_cells(cgo, n, big, ms=(10, 11, 12), counts=None, lam=1e-3, one_pass=True):
    """(c) the log-sum-exp passes at history sizes m: the Gram push — fused (k_lbfgs_push_gram_lse, m ≤ 11, count up to 11)
    or plain (m = 12); the direction — k_lbfgs_combine_spec<ObjLse> with and without the deferred push (m = 10), else
    k_lbfgs_combine_lse; the lite push (m = 10)"""
    mism = []
    path = "pure-HBM" if big else "grid"
    for m in ms:
        P = m + 1
        lst = slot_list(m, P, 3)
        d = lse_data(n, P, lst, 500 + n)
        xn = d["x"] + 0.5 * d["u"]
        Mx = float(np.max(xn))
        Sx = float(np.sum(np.exp(xn - Mx)))
        fused = m <= GRAM_MAXC_LSE
        o = cgo.LogSumExp(n, lam)
        s = _solver(cgo, o, m, big)
        gam = depth(n, big) * U53 * 1.01
        try:
            vec = dict(x=d["x"], u=d["u"], g=d["g"], S=d["S"], Y=d["Y"])
            for c in (counts or sorted({0, 1, 5, min(m, GRAM_MAXC_LSE), m} - ({12} if fused else set()))):
                got = s.probe_lbfgs("push_gram", **vec, gt=None if fused else d["g"] + 0.25, a=0.5, a_s=0.5, slot=3,
                                    list=lst[:c], stats=(Mx, Sx))
                tag = f"lse m={m} n={n} {path} push_gram count={c} [{' + '.join(got['symbols'])}]"
                if got["symbols"] != [f"{'k_lbfgs_push_gram_lse' if fused else 'k_lbfgs_push_gram'}<{str(big).lower()}>"]:
                    mism.append(f"{tag}: unexpected instantiation")
                    continue
                nm = len(mism)
                gt = got["gt"]
                if fused:
                    _lse_grad_ok(tag, gt, xn, Mx, Sx, lam, mism)
                    _vec_mismatch(tag, "xo", got["xo"], xn, mism)
                    _vec_mismatch(tag, "x", got["x"], d["x"], mism)
                else:
                    _vec_mismatch(tag, "x", got["x"], xn, mism)
                    _vec_mismatch(tag, "gt", gt, d["g"] + 0.25, mism)
                sv, yv = 0.5 * d["u"], gt - d["g"]
                _vec_mismatch(tag, "S[3]", got["S"][3], sv, mism)
                _vec_mismatch(tag, "Y[3]", got["Y"][3], yv, mism)
                terms = {0: (sv, yv), 1: (yv, yv), 2: (sv, gt), 3: (yv, gt)}
                for j, q in enumerate(lst[:c]):
                    for k, (l, r) in enumerate(((d["S"][q], gt), (d["Y"][q], gt), (d["S"][q], yv), (d["Y"][q], sv), (d["Y"][q], yv))):
                        if 4 + 5 * j + k != 63 or not fused:
                            terms[4 + 5 * j + k] = (l, r)
                if fused:
                    terms[63] = (gt, gt)
                _plain_sums(tag, got["sums"], terms, gam, mism)
                for slot in range(NG):
                    if slot not in terms and got["sums"][slot] != 0.0:
                        mism.append(f"{tag}: padding slot {slot} holds {got['sums'][slot]!r}")
                _note(got, len(mism) == nm, n, False)
            if not one_pass:
                continue
            # the direction with the first trial's statistics; the iterate's statistics (M, S) = (0, Σ exp x)
            S0 = float(np.sum(np.exp(d["x"])))
            Mr = 0.0 + math.log(S0)
            c = min(m, SPEC_MAXC if m == 10 else 12)
            cy, cs = coefs(c)
            ring0 = (lambda j: d["S"][lst[j]], lambda j: d["Y"][lst[j]])
            got = s.probe_lbfgs("direction_trial", **vec, gt=None, list=lst[:c], cy=cy, cs=cs, cg=-1.0, a_trial=0.5, stats=(0.0, S0))
            tag = f"lse m={m} n={n} {path} direction_trial count={c} [{' + '.join(got['symbols'])}]"
            nm = len(mism)
            if m == 10:
                u = combine_u(d, lst[:c], cy, cs, -1.0, False, waves=True)
                if _vec_mismatch(tag, "u", got["u"], u, mism):
                    lse_spec_row_check(tag, got, d["x"], d["g"], u, ring0, c, lam, Mr, 0.5, n, big, mism)
            else:
                u = combine_u(d, lst[:c], cy, cs, -1.0, False)
                _vec_mismatch(tag, "u", got["u"], u, mism)
                xp = d["x"] + 0.5 * u
                phi_r, dphi_r, _ = lse_reference(xp, u, lam)
                _lse_phi_check(tag, got["sums"], xp, u, lam, gam, (phi_r, dphi_r), mism)
                _plain_sums(tag, got["sums"], {S_GU: (d["g"], u), S_UU: (u, u)}, gam, mism)
                for slot in (5, 6, 9):
                    if got["sums"][slot] != 0.0:
                        mism.append(f"{tag}: padding slot {slot} holds {got['sums'][slot]!r}")
            for sym in (f"k_lbfgs_combine_spec<ObjLse, {str(big).lower()}, false>" if m == 10 else
                        f"k_lbfgs_combine_lse<{str(big).lower()}>",):
                if got["symbols"] != [sym]:
                    mism.append(f"{tag}: launched {got['symbols']}, expected {sym}")
            _note(got, len(mism) == nm, n, False)
            if m != 10:
                continue
            # the lite push and the deferred push (new_in_list 0 and 1) with the accepted trial's statistics (Ml, Sl)
            Ml, Sl = 1.0, float(np.sum(np.exp(d["x"] + 0.25 * d["u"] - 1.0)))
            xl = d["x"] + 0.25 * d["u"]
            got = s.probe_lbfgs("push_lite", **vec, a=0.25, a_s=0.5, slot=3, stats=(Ml, Sl))
            tag = f"lse n={n} {path} push_lite [{' + '.join(got['symbols'])}]"
            nm = len(mism)
            _vec_mismatch(tag, "x", got["x"], xl, mism)
            _lse_grad_ok(tag, got["g"], xl, Ml, Sl, lam, mism)
            _vec_mismatch(tag, "S[3]", got["S"][3], 0.5 * d["u"], mism)
            _vec_mismatch(tag, "Y[3]", got["Y"][3], got["g"] - d["g"], mism)
            if got["sums"].size:
                mism.append(f"{tag}: a row of {got['sums'].size} slots")
            _note(got, len(mism) == nm, n, False)
            c = 4
            cy, cs = coefs(c)
            for nil in (0, 1):
                lite = lst[0] if nil else (3 - 1 - c) % P
                Sr, Yr = d["S"].copy(), d["Y"].copy()
                if nil:
                    Sr[lite], Yr[lite] = np.nan, np.nan
                got = s.probe_lbfgs("direction_trial", x=d["x"], u=d["u"], g=d["g"], S=Sr, Y=Yr, list=lst[:c], cy=cy, cs=cs, cg=-1.0,
                                    a_trial=0.5, stats=(0.0, S0), deferred_push=1, lite_slot=lite, a_lite=0.25, a_s_lite=0.5,
                                    M_lite=Ml, S_lite=Sl)
                tag = f"lse n={n} {path} deferred push new_in_list={nil} [{' + '.join(got['symbols'])}]"
                nm = len(mism)
                if got["new_in_list"] != nil:
                    mism.append(f"{tag}: new_in_list {got['new_in_list']}")
                if got["symbols"] != [f"k_lbfgs_combine_spec<ObjLse, {str(big).lower()}, true>"]:
                    mism.append(f"{tag}: launched {got['symbols']}")
                _vec_mismatch(tag, "x", got["x"], xl, mism)
                gp = got["g"]
                _lse_grad_ok(tag, gp, xl, Ml, Sl, lam, mism)
                sn, yn = 0.5 * d["u"], gp - d["g"]
                _vec_mismatch(tag, f"S[{lite}]", got["S"][lite], sn, mism)
                _vec_mismatch(tag, f"Y[{lite}]", got["Y"][lite], yn, mism)
                ring = (lambda j: sn if (nil and j == 0) else Sr[lst[j]], lambda j: yn if (nil and j == 0) else Yr[lst[j]])
                u = combine_u(dict(d, g=gp), lst[:c], cy, cs, -1.0, False, waves=True, ring=ring)
                if _vec_mismatch(tag, "u", got["u"], u, mism):
                    lse_spec_row_check(tag, got, xl, gp, u, ring, c, lam, Mr, 0.5, n, big, mism)
                _note(got, len(mism) == nm, n, False)
        finally:
            s.close(); o.close()
    return mism


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 17, 277, 1025, 2 * (GRID_BIG * 8 + 1) + 1], ids=lambda n: f"n{n}")
def test_lse_passes_against_mpmath(cgo, n):
    """(c) every log-sum-exp pass (lse_cells) on both streaming paths"""
    _report(lse_cells(cgo, n, False) + lse_cells(cgo, n, True))


@pytest.mark.gpu
def test_lse_push_four_trip_round_pure_hbm(cgo):
    """(c) k_lbfgs_push_gram_lse<true> at n = 524291: chunks of 72 pairs, so trip 1 of the four-trip round is partial and g⁺ of
    waves 1–3 passes through LDS on the pure-HBM path; count 11 (GRAM_MAXC_LSE) and 4"""
    n = 2 * (GRID_BIG * 64 + 1) + 1
    assert lse_round_trips(n >> 1, True) == [64, 8, 0, 0]
    _report(lse_cells(cgo, n, True, ms=(11,), counts=(4, 11), one_pass=False))


# ---- (d) the host's Gram entries from a one-pass row ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 1025, 4097], ids=lambda n: f"n{n}")
def test_push_spec_gram_entries(cgo, n):
    """(d) element-wise: every Gram entry lbfgs_push_spec derives equals the exact inner product of s = a_s·u, y = ∇f(xp) − g,
    g⁺ = ∇f(xp) bit for bit (exact data); log-sum-exp: the κ-corrected algebra against 50-digit inner products of the true
    s, y, g⁺ = exp(xp − lse(xp)) + λ·xp within 2·(the exp's element-wise error carried through) + 1e-12·Σ|terms| (asserted
    below 1e-4 of every entry), also near the minimiser where ‖p‖/‖g⁺‖ ≈ 1e4; the guards: a trial that raises the
    log-sum-exp by more than log 2, and an element-wise trial with ‖g⁺‖² = 0, are refused."""
    import mpmath as mp
    mp.mp.dps = 50
    mism = []
    m, P, c = 10, 11, 6
    lst = slot_list(c, P, 3)
    cy, cs = coefs(c)
    # element-wise
    d = exact_inputs(n, P, 77 + n, lst)
    o = _objective(cgo, Quad, n, d["p"])
    s = _solver(cgo, o, m, False)
    try:
        got = s.probe_lbfgs("direction_trial", x=d["x"], u=d["u"], g=d["g"], S=d["S"], Y=d["Y"], list=lst, cy=cy, cs=cs, cg=-1.0,
                            a_trial=0.75, spec_check=1, spec_a_x=0.75, spec_a_s=0.5, spec_slot=3, spec_list=lst)
        _, out, _, ex = model_spec(Quad, d, lst, cy, cs, -1.0, 0.75, True)
        sv, y, gt = M(0.5, out["u"]), ex["y"], ex["gt"]
        want = [(sv, y), (y, y), (sv, gt), (y, gt), (gt, gt)]
        for j, q in enumerate(lst):
            want += [(d["S"][q], gt), (d["Y"][q], gt), (d["S"][q], y), (d["Y"][q], sv), (d["Y"][q], y)]
        if not got["spec_ok"]:
            mism.append(f"quad n={n}: lbfgs_push_spec refused the row")
        else:
            wv2 = np.array([exact_sum([M(l, r)], [np.ones(n, np.int64)]) for l, r in want])
            if not np.array_equal(bits(got["gram"]), bits(wv2)):
                bad = list(np.nonzero(bits(got["gram"]) != bits(wv2))[0])
                mism.append(f"quad n={n}: Gram entries {bad[:8]} differ: {got['gram'][bad[:3]]} vs {wv2[bad[:3]]}")
        # the guard: a trial at the minimiser (x = g = 0, empty ring vectors: u = 0, g⁺ = 0) has ‖g⁺‖² below 1e-280 — refused
        z = np.zeros(n)
        Z = np.where(np.isnan(d["S"]), np.nan, 0.0)
        got = s.probe_lbfgs("direction_trial", x=z, u=z, g=z, S=Z, Y=Z, list=lst, cy=cy, cs=cs, cg=-1.0, a_trial=0.75, spec_check=1,
                            spec_a_x=0.75, spec_a_s=0.5, spec_slot=3, spec_list=lst)
        if got["spec_ok"]:
            mism.append(f"quad n={n}: lbfgs_push_spec accepted a row with ‖g⁺‖² = 0")
    finally:
        s.close(); o.close()
    # log-sum-exp
    lam = 1e-3
    d = lse_data(n, P, lst, 88 + n)
    d["x"] *= 0.25
    S0 = math.fsum(np.exp(d["x"]))
    # near the minimiser x* = −1/(nλ): ‖p‖/‖g⁺‖ ≈ 1e4, the regime in which Σp², Σp·xp, Σxp² cancel (‖p‖/‖g⁺‖)²-fold
    rng = np.random.default_rng(99 + n)
    xm = -1.0 / (n * lam) + 1e-5 * rng.uniform(-1, 1, n)
    xmp = [mp.mpf(float(v)) for v in xm]
    lm = max(xmp) + mp.log(mp.fsum(mp.e ** (v - max(xmp)) for v in xmp))
    dm = dict(d, x=xm, g=np.array([float(mp.e ** (v - lm) + mp.mpf(lam) * v) for v in xmp]))
    Sm = math.fsum(np.exp(xm - float(lm))) * math.exp(float(lm))
    o = cgo.LogSumExp(n, lam)
    s = _solver(cgo, o, m, False)
    try:
        # accepted: the step changes lse by less than log 2 · refused by lbfgs_push_spec's guard: the reference a quarter of
        # lse(x)'s (the trial raises the log-sum-exp by ≈ log 4 over it) · a trial far out (exp overflows) is taken again by
        # k_lse_stats inside the direction pass, nothing is speculated, and the push is refused as well
        for case, dd, a_tr, stats, scale, expect_ok in (
                ("accepted", d, 0.5, (0.0, S0), 1.0, True), ("rise by log 4", d, 1e-3, (0.0, S0 / 4.0), 1.0, False),
                ("overflow", d, 1e4, (0.0, S0), 1.0, False), ("near the minimiser", dm, 0.5, (float(lm), Sm / math.exp(float(lm))), 1e-10, True)):
            cyc, csc = [v * scale for v in cy], [v * scale for v in cs]
            got = s.probe_lbfgs("direction_trial", x=dd["x"], u=dd["u"], g=dd["g"], S=dd["S"], Y=dd["Y"], list=lst, cy=cyc, cs=csc,
                                cg=-1.0, a_trial=a_tr, stats=stats, spec_check=1, spec_a_x=a_tr, spec_a_s=0.5, spec_slot=3,
                                spec_list=lst)
            tag = f"lse n={n} {case}"
            if got["spec_ok"] != expect_ok:
                mism.append(f"{tag}: lbfgs_push_spec {'accepted' if got['spec_ok'] else 'refused'} the row")
                continue
            if not expect_ok:
                continue
            u = got["u"]
            xpf = dd["x"] + a_tr * u
            xp = [mp.mpf(float(v)) for v in xpf]
            mx = max(xp)
            lse = mx + mp.log(mp.fsum(mp.e ** (v - mx) for v in xp))
            gtm = [mp.e ** (v - lse) + mp.mpf(lam) * v for v in xp]
            sm = [mp.mpf(0.5) * mp.mpf(float(v)) for v in u]
            ym = [a - mp.mpf(float(b)) for a, b in zip(gtm, dd["g"])]
            # what the exp of the one-pass row leaves in g⁺ and y, element by element (the row's own error; see
            # lse_spec_row_check): δ_k = 2·p_k·(|xp_k − M_r| + |M_r| + 2.5)·u, M_r the reference maximum
            Mr = stats[0] + math.log(stats[1])
            pk = np.array([float(mp.e ** (v - lse)) for v in xp])
            dk = 2 * pk * (np.abs(xpf - Mr) + abs(Mr) + 2.5) * U53
            vecm = lambda v: [mp.mpf(float(t)) for t in v]

            def dot(A_, B_, dA, dB):
                af = np.array([float(a) for a in A_]); bf = np.array([float(b) for b in B_])
                err = float(np.sum(np.abs(af) * dB + dA * np.abs(bf) + dA * dB))
                return mp.fsum(a * b for a, b in zip(A_, B_)), float(mp.fsum(abs(a * b) for a, b in zip(A_, B_))), err
            z = np.zeros(n)
            want = [dot(sm, ym, z, dk), dot(ym, ym, dk, dk), dot(sm, gtm, z, dk), dot(ym, gtm, dk, dk), dot(gtm, gtm, dk, dk)]
            names = ["s·y", "y·y", "s·g⁺", "y·g⁺", "‖g⁺‖²"]
            for j, q in enumerate(lst):
                want += [None, None, dot(vecm(dd["S"][q]), ym, z, dk), dot(vecm(dd["Y"][q]), sm, z, z), dot(vecm(dd["Y"][q]), ym, z, dk)]
                names += [f"s{j}·g⁺", f"y{j}·g⁺", f"s{j}·y", f"y{j}·s", f"y{j}·y"]
            for i, w in enumerate(want):
                if w is None:
                    continue
                val, mag, err = w
                bound = 2 * err + 1e-12 * mag
                if i < 5 or case != "near the minimiser":   # (there the pair entries with y sum ± terms of ≈ 1e-8 to ≈ 0)
                    assert bound < 1e-4 * abs(float(val)), f"test data: {tag} {names[i]} too close to zero for its bound"
                if not abs(got["gram"][i] - float(val)) <= bound:
                    mism.append(f"{tag}: {names[i]} {got['gram'][i]!r} vs {float(val)!r} (bound {bound:.2e})")
    finally:
        s.close(); o.close()
    _report(mism)


# ---- (f) coverage --------------------------------------------------------------------------------------------------------
def dispatched_lbfgs_kernels():
    """k_lbfgs_* names launched in cgo_backend_lbfgs.hip and compiled at run time (rows of csrc/cgo_instances.def)"""
    src = open(os.path.join(CSRC, "cgo_backend_lbfgs.hip")).read()
    names = set(re.findall(r"\b(k_lbfgs_[a-z_]+)<", src))
    objs = set(re.findall(r"launch_(?:spec|lite)<(Obj[A-Za-z]+)>", src))
    return names, {kernel for kernel, key, nbools in I.rows("RTC_LBFGS")}, objs


def expected_instantiations():
    want = set()
    for b in ("false", "true"):
        for k in ("k_lbfgs_push", "k_lbfgs_push_gram", "k_lbfgs_push_gram_lse", "k_lbfgs_combine", "k_lbfgs_combine_lse", "k_lbfgs_loop"):
            want.add(f"{k}<{b}>")
        for on in ("ObjLse", "ObjQuadDiag", "ObjRosenPaired", "UserObjective"):
            want.add(f"k_lbfgs_push_lite<{on}, {b}>")
            for push in ("false", "true"):
                want.add(f"k_lbfgs_combine_spec<{on}, {b}, {push}>")
    return want


def test_dispatch_tables_have_tests():
    """CPU tier: the L-BFGS kernels the backend launches and the run-time compiled module builds are those this module
    expects (a new variant cannot arrive untested)."""
    names, rtc_names, objs = dispatched_lbfgs_kernels()
    assert names == {"k_lbfgs_push", "k_lbfgs_push_gram", "k_lbfgs_push_gram_lse", "k_lbfgs_combine", "k_lbfgs_combine_lse",
                     "k_lbfgs_combine_spec", "k_lbfgs_push_lite", "k_lbfgs_loop"}, names
    assert rtc_names == {"k_lbfgs_combine_spec", "k_lbfgs_push_lite"}
    assert objs == {"ObjLse", "ObjQuadDiag", "ObjRosenPaired"}
    assert len(expected_instantiations()) == 36


@pytest.mark.gpu
def test_coverage_of_every_instantiation(cgo):
    """Every k_lbfgs_* instantiation ran in a pass whose whole row (where it has one) and every vector were compared with a
    reference: REACHED holds only such passes.  What the tests above did not reach (this test run alone, or the module split)
    is probed here, at small sizes, by the same checks — element-wise bit for bit, log-sum-exp through lse_cells."""
    mism = []
    if expected_instantiations() - REACHED:
        for big in (False, True):
            mism += run_elementwise(cgo, Quad, 17, big, 10, (0, 4, 10))
            mism += run_elementwise(cgo, Quad, 17, big, 12, (12,), passes=("push_gram", "direction_gram"))
            mism += run_elementwise(cgo, User, 17, big, 10, (4,), passes=("direction_trial", "push_lite", "deferred0", "deferred1"))
            mism += run_elementwise(cgo, Rosen, 16, big, 10, (4,), passes=("direction_trial", "push_lite", "deferred0", "deferred1"))
            mism += run_two_loop(cgo, Quad, 17, big)
            mism += lse_cells(cgo, 17, big)
    _report(mism)
    still = sorted(expected_instantiations() - REACHED)
    assert not still, f"{len(still)} instantiations never probed: {still}"
    bitwise = len({(s, n) for (s, n) in CELLS})
    print(f"\n[lbfgs kernel sums] {bitwise} (instantiation, size) cells checked bit for bit, {sum(CELLS.values())} passes")


# ---- history sizes where the forms switch, end to end ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m", [11, 12, 13])
@pytest.mark.parametrize("kind", ["lse", "quad_diag"])
def test_history_size_boundaries_against_the_oracle(cgo, gpu_ctx, kind, m, monkeypatch):
    """m = 11, 12, 13 with max_iters ≥ m + 4 (the ring wraps), against the oracle at TOL; which form ran, from the push counts
    (speculated, fused, plain): m = 11 log-sum-exp: every push fused (k_lbfgs_push_gram_lse; direction k_lbfgs_combine_lse),
    element-wise: Gram form, not one-pass · m = 12: plain k_lbfgs_push_gram pushes (k_lse_grad first) · m = 13: the two-loop
    (k_lbfgs_push, no Gram push counted).  At m = 12 the two-loop form takes the same step sequence as the Gram form."""
    from _cases import Case, assert_parity, first_divergence, quad_D, run_gpu, run_oracle
    from test_gpu_parity import TOL, lse_x0
    n = 4097 if kind == "lse" else 20001
    # λ = 1e-6 (config 4's): the log-sum-exp solve runs all m + 6 iterations (with λ = 1e-3 it converges after 11)
    extra = dict(lam=1e-6, eps=1e-12) if kind == "lse" else dict(D=quad_D(n, 1.0, 50.0), eps=1e-9)
    x0 = lse_x0(n) if kind == "lse" else np.ones(n)
    c = Case(f"{kind}{n}-LBFGS{m}", kind, n, x0, beta="LBFGS", m=m, max_iters=m + 6, c2=0.9, **extra)
    got, ref = run_gpu(c), run_oracle(c)
    assert_parity(got, ref, TOL, c.name)
    assert got.iters_ran >= m + 4, (c.name, got.iters_ran, got.status)   # m + 1 ring slots: the ring has wrapped
    sp, fu, pl = tuple(got.lbfgs_pushes)
    if m == 13:
        assert (sp, fu, pl) == (0, 0, 0), got.lbfgs_pushes
    elif kind == "lse" and m == 11:   # fused wherever the accepted trial's statistics are at hand, never speculated
        assert sp == 0 and fu >= m + 1 and fu + pl == got.iters_ran, got.lbfgs_pushes
    else:
        assert sp == 0 and fu == 0 and pl == got.iters_ran, got.lbfgs_pushes
    if m == 12:
        monkeypatch.setenv("CGO_LBFGS_TWO_LOOP", "1")
        two = run_gpu(c)
        assert tuple(two.lbfgs_pushes) == (0, 0, 0)
        assert first_divergence(got, two) is None and two.iters_ran == got.iters_ran and two.status == got.status
