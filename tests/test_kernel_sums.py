"""Every sum slot of every launch of the gradient-free CG family, one launch at a time (cgo_solver_probe_launch).

The trajectory suites see a kernel's row only through the numbers the line search happens to read: a 7-point launch reduces
51 sums, the engine reads point j only when the search lands on hint j, and each β flavour reads only some of a point's seven
sums.  Here every slot of every point — the padding points that repeat a[k−1] and the padding slots included — and every
vector a launch writes are compared with references that leave no room for tolerance games:

(a) exact data: x, u, D, a_j, β, a_acc are dyadic numbers with few significant bits, so that every element-wise result and
    every product is exact in double (checked here, operation by operation, with the error-free two-sum / two-product
    transformations) and the sum of the magnitudes of each slot's terms stays below 2⁵³ of the slot's smallest quantum
    (checked here in integer arithmetic), so that EVERY summation order gives the same bits: the device row must equal the
    exact sum bit for bit, whatever the launch geometry, tail or policy;
(b) random data against the correctly rounded exact sum of the exact products, within the classical bound of recursive
    summation over the launch's own summation depth;
(c) the log-sum-exp launches against a 50-digit mpmath reference;
(d) the instantiations the probes reached cover every k_cg / k_chain instantiation launch_cg / launch_chain can dispatch
    (checked against the table they expand from by a CPU-tier test, so that a new variant cannot come without a test here).

The data of (a) are periodic with a period of 1531 pairs (a prime: no chunk, wave or grid stride of a launch is a multiple of
it), so that the expected rows of the large sizes come from one period and per-pair multiplicities; below one period the
vectors are not periodic at all.
"""
import math
import os
from collections import defaultdict

import numpy as np
import pytest

import _instances as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# launch geometry (csrc/cgo_kernels.hip.hpp, cgo_hip_backend.hip)
BLOCK, GRID_BIG, TAIL_GROUP = 256, 4096, 64
R_ACCEPT, R_DIR, R_TRIAL, R_INIT, R_RESET, R_UPG, R_GRAD, R_GRADT, R_PROJ, R_EDGES = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
RS = 7                                                     # sums per trial point
F, GTU, GTGT, GTG, YY, UY, YGT = range(RS)
NAN_BITS = np.int64(0x7FF87FF87FF87FF8)                    # what the probe puts where an input is absent


def npts_for(k):
    return 1 if k <= 1 else (3 if k <= 3 else (5 if k <= 5 else 7))


def row_width(npts):
    return {1: 10, 3: 24, 5: 40, 7: 56}[npts]


def grid_cg(n, npts):
    """grid_cg / grid_capped of cgo_hip_backend.hip (two pairs per lane, capped)."""
    n2 = n >> 1
    blocks = max(1, -(-n2 // (BLOCK * 2)))
    cap = (256 if n <= 2000000 else 512) if npts >= 5 else (256 if n <= 16000000 else 512)
    return min(blocks, cap)


def big_chunk_pairs(n2, grid=GRID_BIG):
    per = -(-n2 // grid)
    return (per + 7) & ~7


def busy_workgroups(n2):
    per = big_chunk_pairs(n2)
    return 0 if per == 0 else min(GRID_BIG, -(-n2 // per))


# ---- sizes: which edge of the launch geometry each one hits ------------------------------------------------------------
def _sizes():
    s = {}
    for n in (1, 2, 3):
        s[n] = "fewer than one pair per lane of the first wave; n = 1, 3: only the odd tail element path"
    for n in (15, 16, 17):
        s[n] = "one pair-trip of one wave, partial"
    w = 64 * 2                                            # one wave: 64 lanes × one pair
    for n in (w - 1, w, w + 1):
        s[n] = "around one wave of pairs"
    g = BLOCK * 2                                         # one workgroup: 256 lanes × one pair
    for n in (g - 1, g, g + 1):
        s[n] = "around one workgroup of pairs"
    for j in (1, 2):
        for d in (-1, 0, 1):
            n2 = GRID_BIG * 8 * j + d                     # pure-HBM chunks of exactly 8j pairs at d = 0; one pair short / over
            s[2 * n2] = f"pure-HBM: {GRID_BIG} chunks of 8·{j} pairs {'minus one pair' if d < 0 else 'plus one pair' if d > 0 else 'exactly'}"
            s[2 * n2 + 1] = s[2 * n2] + ", odd tail element"
    n2 = GRID_BIG + 5                                     # share of 2 pairs rounds up to 8: 513 busy workgroups, 3583 empty
    s[2 * n2] = "pure-HBM: per-workgroup share rounds from 2 pairs up to 8, most workgroups empty"
    s[2 * n2 + 1] = s[2 * n2] + ", odd tail element"
    return s


SIZES = _sizes()
BIG_DEFAULT_N = (1 << 25) + 17                            # above the default pure-HBM threshold: no forced policy needed


def test_sizes_hit_the_edges_they_claim():
    """CPU tier: the size table's claims follow from the geometry constants."""
    for j in (1, 2):
        assert big_chunk_pairs(GRID_BIG * 8 * j) == 8 * j and busy_workgroups(GRID_BIG * 8 * j) == GRID_BIG
        assert big_chunk_pairs(GRID_BIG * 8 * j + 1) == 8 * j + 8 and busy_workgroups(GRID_BIG * 8 * j + 1) < GRID_BIG
        assert big_chunk_pairs(GRID_BIG * 8 * j - 1) == 8 * j
    assert -(-(GRID_BIG + 5) // GRID_BIG) == 2 and big_chunk_pairs(GRID_BIG + 5) == 8 and busy_workgroups(GRID_BIG + 5) == 513
    assert grid_cg(2 * GRID_BIG * 16, 3) == 128 == GRID_BIG * 16 // (2 * BLOCK)   # grid-stride: two whole pairs per lane, none left
    assert 8 * BIG_DEFAULT_N * 3 > 4.5e8 > 0 and grid_cg(BIG_DEFAULT_N, 7) == 512   # trial: pure-HBM; accept+dir+trial: 512 workgroups


# ---- exact arithmetic witnesses ----------------------------------------------------------------------------------------
_SPLIT = 134217729.0   # 2^27 + 1 (Dekker)


def _split(a):
    c = _SPLIT * a
    hi = c - (c - a)
    return hi, a - hi


def _f(v):
    return np.asarray(v, dtype=np.float64)


CHECK_EXACT = [True]   # (b) runs the same models on random data: plain IEEE arithmetic, no exactness assertions


def M(a, b):
    """a·b, asserted exact (two-product error term zero)."""
    a, b = np.broadcast_arrays(_f(a), _f(b))
    p = a * b
    if not CHECK_EXACT[0]:
        return p
    ah, al = _split(a)
    bh, bl = _split(b)
    err = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    assert np.all(err == 0) and np.all(np.isfinite(p)), "test data: a product is not exact in double"
    return p


def A(a, b):
    """a + b, asserted exact (two-sum error term zero)."""
    a, b = np.broadcast_arrays(_f(a), _f(b))
    s = a + b
    if not CHECK_EXACT[0]:
        return s
    bb = s - a
    err = (a - (s - bb)) + (b - bb)
    assert np.all(err == 0) and np.all(np.isfinite(s)), "test data: a sum is not exact in double"
    return s


def S(a, b):
    return A(a, -_f(b))


def exact_sum(terms, weights):
    """Σ wᵢ·tᵢ of exactly representable terms, in integers; asserts that Σ wᵢ|tᵢ| < 2⁵³ quanta, i.e. that every partial sum
    in ANY order is an exact double — then the device's sum must be these bits whatever its order."""
    t = np.concatenate([_f(x).ravel() for x in terms]) if terms else np.zeros(0)
    w = np.concatenate([np.asarray(x, dtype=np.int64).ravel() for x in weights]) if weights else np.zeros(0, np.int64)
    keep = (t != 0) & (w != 0)
    t, w = t[keep], w[keep]
    if t.size == 0:
        return 0.0
    m, e = np.frexp(t)
    mant = np.abs((m * 2.0 ** 53).astype(np.int64))
    low = e.astype(np.int64) - 53 + np.round(np.log2((mant & -mant).astype(np.float64))).astype(np.int64)
    q = int(low.min())                                   # the slot's quantum 2^q
    ints = np.ldexp(t, -q)
    assert np.all(np.abs(ints) < 2.0 ** 53) and np.all(ints == np.round(ints))
    bound = float(np.sum(np.abs(ints) * w.astype(np.float64)))   # relative error < 1e-12 below 2^52: the exact value < 2^53
    assert bound < 2.0 ** 52, f"test data: a slot's terms add up to 2^{math.log2(bound):.1f} quanta (order-dependent)"
    total = int(np.sum(ints.astype(np.int64) * w))
    return math.ldexp(float(total), q)


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


# ---- the element-wise objectives (csrc/cgo_kernels.hip.hpp functors, unfused, in the kernels' order) ---------------------
class Quad:
    name, kind, per_elem_f, param = "quad_diag", "quad_diag", True, True

    @staticmethod
    def g2(x, p):                      # eval2 = eval1 per element
        g = M(p, x)
        return M(0.5, M(g, x)), g

    g1 = g2


class Rosen:
    name, kind, per_elem_f, param = "rosenbrock_paired", "rosenbrock_paired", False, False

    @staticmethod
    def g2(x, p):
        xe, xo = x[0::2], x[1::2]
        t1 = S(xo, M(xe, xe))
        t2 = S(1.0, xe)
        f = A(M(100.0, M(t1, t1)), M(t2, t2))
        g = np.empty_like(x)
        g[0::2] = S(M(-400.0, M(xe, t1)), M(2.0, t2))
        g[1::2] = M(200.0, t1)
        return f, g

    @staticmethod
    def g1(x, p):
        return np.zeros(0), np.zeros_like(x)


class Booth(Rosen):
    name, kind = "booth", "booth"

    @staticmethod
    def g2(x, p):
        a, b = x[0::2], x[1::2]
        t1 = S(A(a, M(2.0, b)), 7.0)
        t2 = S(A(M(2.0, a), b), 5.0)
        f = A(M(t1, t1), M(t2, t2))
        g = np.empty_like(x)
        g[0::2] = A(M(2.0, t1), M(M(2.0, t2), 2.0))
        g[1::2] = A(M(M(2.0, t1), 2.0), M(2.0, t2))
        return f, g


class User(Quad):
    name = "user_quad"
    SOURCE = "gi = p*x; fi = 0.5*(gi*x);"


def cg_model(obj, x, u, p, x2, mode, a, a_acc, beta, single):
    """One k_cg launch on a block of pairs (or the odd tail element: `single`).  Returns (terms, vectors): terms[slot] is a
    list of (factors, per_element) — a term is the product of its one or two factors; per_element False for per-pair f
    terms — and vectors the x / u / g the launch leaves."""
    grad = obj.g1 if single else obj.g2
    npts = npts_for(len(a)) if mode & R_TRIAL else 1
    GU, UU = RS * npts, RS * npts + 1
    T = defaultdict(list)
    fe = obj.per_elem_f or single
    x1 = A(x, M(a_acc, u)) if mode & R_ACCEPT else x
    out = {"x": x1}
    g = None
    if mode & (R_DIR | R_TRIAL | R_INIT | R_RESET | R_UPG | R_GRAD | R_PROJ):
        f0, g = grad(x1, p)
    un = u
    if mode & R_INIT:
        T[F].append(((f0,), fe)); T[GTGT].append(((g, g), True))
        un = -g
        out["u"] = un
    if mode & (R_DIR | R_RESET):
        un = A(-g, M(beta, u)) if mode & R_DIR else -g
        T[GU].append(((g, un), True)); T[UU].append(((un, un), True))
        out["u"] = un
    if mode & R_UPG:
        t = A(u, g)
        T[UU].append(((t, t), True))
    if mode & R_GRAD:
        out["g"] = g
    if mode & R_GRADT:
        out["g"] = grad(A(x1, M(a[0], u)), p)[1]
    if mode & R_PROJ:
        gz = grad(A(x1, M(a[0], u)), p)[1]
        xn = A(x2, M(beta, gz))
        out["g"] = xn
        ft, gt = grad(xn, p)
        _point_sums(T, 0, ft, fe, gt, g, u)
    if mode & R_TRIAL:
        for j in range(npts):
            ft, gt = grad(A(x1, M(a[j], un)), p)
            _point_sums(T, j, ft, fe, gt, g, un)
    return T, out


def _point_sums(T, j, ft, fe, gt, g, u):
    b = RS * j
    y = S(gt, g)
    T[b + F].append(((ft,), fe))
    for s, (l, r) in ((GTU, (gt, u)), (GTGT, (gt, gt)), (GTG, (gt, g)), (YY, (y, y)), (UY, (u, y)), (YGT, (y, gt))):
        T[b + s].append(((l, r), True))


PERIOD_PAIRS = 1531


class Data:
    """Periodic exact data for n elements: element i of a vector is period[i mod 2·1531] (pairs stay aligned)."""

    def __init__(self, n, per):
        self.n, self.n2, self.odd = n, n >> 1, n & 1
        self.full = {k: np.resize(v, n) for k, v in per.items()}
        P = min(self.n2, PERIOD_PAIRS)
        self.block = {k: v[:2 * P] for k, v in per.items()}
        cp = np.array([self.n2 // PERIOD_PAIRS + (1 if q < self.n2 % PERIOD_PAIRS else 0) for q in range(P)], dtype=np.int64)
        self.cpair, self.celem = cp, np.repeat(cp, 2)
        self.single = {k: v[n - 1:n] for k, v in self.full.items()} if self.odd else None


def expected_cg(obj, d: Data, mode, a, a_acc, beta, with_u=True):
    """The exact row and vectors of one k_cg launch on Data d (None for a vector the launch leaves as NaN)."""
    npts = npts_for(len(a)) if mode & R_TRIAL else 1
    aa = list(a) + [a[-1]] * (npts - len(a)) if a else [0.0] * npts
    terms, weights = defaultdict(list), defaultdict(list)
    parts = {"x": [], "u": [], "g": []}
    for part, blk in (("pairs", d.block if d.n2 else None), ("single", d.single)):
        if blk is None:
            continue
        T, out = cg_model(obj, blk["x"], blk["u"], blk.get("p"), blk.get("x2"), mode, aa, a_acc, beta, part == "single")
        for s, lst in T.items():
            for fac, per_elem in lst:
                arr = M(*fac) if len(fac) == 2 else fac[0]
                terms[s].append(arr)
                weights[s].append(np.ones(arr.size, np.int64) if part == "single" else (d.celem if per_elem else d.cpair))
        m = 2 * d.n2 if part == "pairs" else 1
        lo = 0 if part == "pairs" else d.n - 1
        for key in parts:
            v = out.get(key)
            if v is None and key == "u" and with_u:
                v = d.full["u"][lo:lo + m]
            parts[key].append(None if v is None else np.resize(v, m))
    sums = np.zeros(0 if mode in (R_ACCEPT, R_GRAD, R_GRADT) else row_width(npts))   # (those launches leave no row)
    for s in terms:
        sums[s] = exact_sum(terms[s], weights[s])
    vec = {k: (None if any(p is None for p in v) else np.concatenate(v)) for k, v in parts.items()}
    return sums, vec


# ---- data --------------------------------------------------------------------------------------------------------------
def _dy(rng, size, lo, hi, q, nonzero=True):
    """dyadic values k·q, k integer in [lo, hi] (q a power of two)."""
    k = rng.integers(lo, hi + 1, size)
    if nonzero:
        k[k == 0] = hi
    return k * q


def exact_period(obj_name, seed=7):
    rng = np.random.default_rng(seed)
    L = 2 * PERIOD_PAIRS
    if obj_name in ("quad_diag", "user_quad"):
        return dict(x=_dy(rng, L, -8, 8, 0.25), u=_dy(rng, L, -6, 6, 0.25), p=rng.integers(1, 5, L).astype(np.float64),
                    x2=_dy(rng, L, -8, 8, 0.25))
    if obj_name == "rosenbrock_paired":   # the quartic: x, u on a coarse grid (xp of ≤ 4 significant bits)
        return dict(x=_dy(rng, L, -2, 2, 0.5, False), u=_dy(rng, L, -1, 1, 0.5), x2=_dy(rng, L, -2, 2, 0.5, False))
    raise KeyError(obj_name)


# Steps: distinct per point, so that a point's sums in another point's slots show.  The quartic's budget: for a trial along
# the input u, xp = x + a·u on a 1/8 grid; along u = −∇f (accept + direction + trial, direction + trial) even that grid
# leaves no budget — those launches run on the valley data below with a_acc = β = 0, where ∇f is small.
STEPS = {"quad_diag": [0.25 * (j + 1) for j in range(7)], "user_quad": [0.25 * (j + 1) for j in range(7)],
         "rosenbrock_paired": [0.125 * (j + 1) for j in range(7)], "booth": [0.25 * (j + 1) for j in range(7)]}
SCAL = {"quad_diag": (0.5, 0.75), "user_quad": (0.5, 0.75), "rosenbrock_paired": (0.5, 0.5), "booth": (0.5, 0.75)}


def rosen_valley_period(seed=11):
    """pairs (t, t²), t ∈ {1/2, 1}: ∇f = (−2(1 − t), 0)"""
    rng = np.random.default_rng(seed)
    t = rng.choice([0.5, 1.0], PERIOD_PAIRS)
    x = np.empty(2 * PERIOD_PAIRS)
    x[0::2], x[1::2] = t, t * t
    return dict(x=x, u=_dy(rng, 2 * PERIOD_PAIRS, -1, 1, 0.5))


def launches(obj_name):
    """(kind, variant, k) of every launch the engine issues for this objective."""
    L = [("init", R_INIT, 0), ("init", R_GRAD, 0), ("accept_dir", R_ACCEPT | R_DIR, 0), ("accept_only", R_ACCEPT, 0),
         ("reset_dir", R_RESET, 0), ("upg_norm", R_UPG, 0), ("dir_trial", R_DIR, 0), ("sys_project", R_PROJ, 1),
         ("scaled_norm", R_GRAD, 1), ("scaled_norm", R_GRADT, 1)]
    for k in range(1, 8):
        L += [("trial", R_TRIAL, k), ("accept_dir_trial", R_ACCEPT | R_DIR | R_TRIAL, k), ("dir_trial", R_DIR | R_TRIAL, k)]
    return L


def launch_inputs(obj_name, mode, n):
    """(data, a_acc, beta) for one launch of the exact matrix."""
    a_acc, beta = SCAL[obj_name]
    if obj_name == "booth":
        per = dict(x=np.array([0.5, 1.25]), u=np.array([-0.25, 0.75]), x2=np.array([1.5, -0.5]))
        return Data(n, per), a_acc, beta
    if obj_name == "rosenbrock_paired":
        if (mode & R_TRIAL) and (mode & R_DIR):
            return Data(n, rosen_valley_period()), 0.0, 0.0
        if mode & R_PROJ:
            beta = 0.0    # x2 + m·∇f(z): ∇f(z) has ~10 bits; m = 0 keeps x2 on its grid (the projection's own sums still checked)
    return Data(n, exact_period(obj_name)), a_acc, beta


def needs_u(mode):
    return bool(mode & (R_ACCEPT | R_DIR | R_TRIAL | R_UPG | R_GRADT | R_PROJ))


def test_exact_data_meet_their_preconditions():
    """CPU tier: for every objective, launch and size of the exact matrix the data are exact and order-independent — the
    same checks the GPU test makes before it asserts, run here so that an edit to the data fails without a GPU."""
    for obj in (Quad, Rosen, Booth):
        sizes = [2] if obj is Booth else [n for n in sorted(SIZES) if not (obj is Rosen and n % 2)]
        for n in sizes[-4:] + sizes[:3]:
            for kind, mode, k in launches(obj.name):
                d, a_acc, beta = launch_inputs(obj.name, mode, n)
                expected_cg(obj, d, mode, STEPS[obj.name][:k], a_acc, beta)
    d, a_acc, beta = launch_inputs("quad_diag", R_TRIAL, BIG_DEFAULT_N)
    for kind, mode, k in (("trial", R_TRIAL, 7), ("accept_dir_trial", R_ACCEPT | R_DIR | R_TRIAL, 7)):
        expected_cg(Quad, d, mode, STEPS["quad_diag"][:k], a_acc, beta)


# ---- the stencil objective (csrc/cgo_kernels_chain.hip.hpp), on whole vectors -------------------------------------------
def _chain_grad(xm, x0, xp, em, ep):
    g = np.zeros_like(x0)
    t1 = S(x0, M(xm, xm))
    g = np.where(em, A(g, M(200.0, t1)), g)
    t2 = S(1.0, x0)
    t1b = S(xp, M(x0, x0))
    g = np.where(ep, A(g, S(M(-2.0, t2), M(400.0, M(x0, t1b)))), g)
    return g


def _chain_terms(x):
    t2 = S(1.0, x[:-1])
    t1 = S(x[1:], M(x[:-1], x[:-1]))
    return A(M(t2, t2), M(100.0, M(t1, t1)))


def expected_chain(x, u, mode, a, a_acc, beta, terms_out=None):
    N = x.size
    npts = 3 if (mode & R_TRIAL) and len(a) >= 2 else 1
    W, EDGE = (24, 10) if npts == 1 else (32, 24)
    aa = list(a) + [a[-1]] * (npts - len(a)) if a else [0.0] * 3
    idx = np.arange(N)
    em, ep = idx >= 1, idx <= N - 2

    def grad(v):
        vm = np.concatenate([[0.0], v[:-1]])
        vp = np.concatenate([v[1:], [0.0]])
        return _chain_grad(vm, v, vp, em, ep)
    T = defaultdict(list)
    GU, UU = RS * npts, RS * npts + 1
    uu = u if u is not None else np.zeros(N)
    x1 = A(x, M(a_acc, uu)) if mode & R_ACCEPT else x
    out = {"x": x1, "u": u, "g": None}
    if mode & R_EDGES:
        xn, un = x, uu
    else:
        g = grad(x1)
        un = uu
        if mode & R_DIR:
            un = A(-g, M(beta, uu))
        elif mode & (R_INIT | R_RESET):
            un = -g
        if mode & (R_DIR | R_INIT | R_RESET):
            out["u"] = un
        if mode & R_INIT:
            T[F].append((_chain_terms(x1),)); T[GTGT].append((g, g))
        if mode & (R_DIR | R_RESET):
            T[GU].append((g, un)); T[UU].append((un, un))
        if mode & R_UPG:
            t = A(uu, g)
            T[UU].append((t, t))
        if mode & R_GRAD:
            out["g"] = g
        if mode & (R_TRIAL | R_GRADT):
            for j in range(npts):
                xp = A(x1, M(aa[j], un))
                gt = grad(xp)
                if mode & R_GRADT:
                    out["g"] = gt
                if mode & R_TRIAL:
                    b = RS * j
                    y = S(gt, g)
                    T[b + F].append((_chain_terms(xp),))
                    for s, (l, r) in ((GTU, (gt, un)), (GTGT, (gt, gt)), (GTG, (gt, g)), (YY, (y, y)), (UY, (un, y)), (YGT, (y, gt))):
                        T[b + s].append((l, r))
        xn = x1
    if terms_out is not None:
        terms_out.update(T)
    sums = np.zeros(W)
    for s, ts in T.items():
        if CHECK_EXACT[0]:   # ((b) takes the terms instead: terms_out)
            arrs = [M(*f) if len(f) == 2 else f[0] for f in ts]
            sums[s] = exact_sum(arrs, [np.ones(a.size, np.int64) for a in arrs])
    # this rank's edge values: the first pair and the last pair (phantom element of an odd N: 0) after the launch
    pad = lambda v: np.concatenate([v, [0.0]]) if N & 1 else v
    xe, ue = pad(xn), pad(un)
    sums[EDGE:EDGE + 8] = np.array([xe[0], xe[1], ue[0], ue[1], xe[-2], xe[-1], ue[-2], ue[-1]]) + 0.0
    return sums, out


# ---- GPU -------------------------------------------------------------------------------------------------------------
TAILS = {"fused": dict(fused_tail=True), "finalize": dict(fused_tail=False), "strict": dict(strict_tail=True)}
REACHED = set()                                            # symbols the probes launched (coverage, test_coverage_*)
CELLS = defaultdict(int)                                   # (symbol, n, tail) cells checked bit for bit


@pytest.fixture(scope="module")
def contexts(cgo):
    out = {}
    for name in TAILS:
        out[name] = cgo.Context(0)
    yield out
    for c in out.values():
        c.close()


def _solver(cgo, obj, tail, big):
    pol = cgo.SolverPolicy(resident=False, controller_depth=0, hbm_stream_bytes=1.0 if big else None, **TAILS[tail])
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.DisableTrace(), max_iters=5)
    return cgo.Solver(obj, cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), pol)


def _make_objective(cgo, obj, n, ctx, d):
    if obj is User:
        return cgo.ElementwiseObjective(n, User.SOURCE, param=d.full["p"], ctx=ctx)
    if obj is Quad:
        return cgo.QuadDiag(d.full["p"], ctx)
    if obj is Rosen:
        return cgo.RosenbrockPaired(n, ctx)
    return cgo.Booth(ctx)


def _compare(tag, got, want_sums, want, mism):
    if got["sums"].size != want_sums.size or not np.array_equal(bits(got["sums"]), bits(want_sums)):
        bad = [] if got["sums"].size != want_sums.size else list(np.nonzero(bits(got["sums"]) != bits(want_sums))[0])
        mism.append(f"{tag}: row of {got['sums'].size} slots, expected {want_sums.size}; slots differing {bad[:12]}: "
                    f"got {[got['sums'][i] for i in bad[:4]]} want {[want_sums[i] for i in bad[:4]]}")
        return False
    for key in ("x", "u", "g"):
        w = want.get(key)
        g = got[key]
        wb = np.full(g.size, NAN_BITS) if w is None else bits(w)
        if not np.array_equal(bits(g), wb):
            i = int(np.nonzero(bits(g) != wb)[0][0])
            mism.append(f"{tag}: {key}_out differs first at element {i} of {g.size}: got {g[i]!r}, want "
                        f"{'NaN (not written)' if w is None else w[i]!r}")
            return False
    return True


def _run_cg(cgo, contexts, obj, n, tails=tuple(TAILS), bigs=(False, True), launch_list=None):
    mism = []
    exp_cache = {}
    for tail in tails:
        for big in bigs:
            o = _make_objective(cgo, obj, n, contexts[tail], launch_inputs(obj.name, R_TRIAL, n)[0])
            s = _solver(cgo, o, tail, big)
            try:
                for kind, mode, k in (launch_list or launches(obj.name)):
                    d, a_acc, beta = launch_inputs(obj.name, mode, n)
                    a = STEPS[obj.name][:k]
                    key = (kind, mode, k)
                    if key not in exp_cache:
                        exp_cache[key] = expected_cg(obj, d, mode, a, a_acc, beta, with_u=needs_u(mode))
                    want_sums, want = exp_cache[key]
                    got = s.probe_launch(kind, mode, a_acc, beta, a, d.full["x"], d.full["u"] if needs_u(mode) else None,
                                         d.full["x2"] if mode & R_PROJ else None)
                    REACHED.add(got["symbol"])
                    if _compare(f"{obj.name} n={n} {tail} {'pure-HBM' if big else 'grid-stride'} {kind}/{mode} k={k} "
                                f"[{got['symbol']}]", got, want_sums, want, mism):
                        CELLS[(got["symbol"], n, tail)] += 1
            finally:
                s.close(); o.close()
    return mism


def _report(mism):
    assert not mism, f"{len(mism)} launch(es) differ from the exact reference:\n" + "\n".join(mism[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(SIZES), ids=lambda n: f"n{n}")
def test_quad_exact_every_slot(cgo, contexts, n):
    _report(_run_cg(cgo, contexts, Quad, n))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [n for n in sorted(SIZES) if n % 2 == 0], ids=lambda n: f"n{n}")
def test_rosenbrock_paired_exact_every_slot(cgo, contexts, n):
    _report(_run_cg(cgo, contexts, Rosen, n))


@pytest.mark.gpu
def test_booth_exact_every_slot(cgo, contexts):
    _report(_run_cg(cgo, contexts, Booth, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 513, 2 * (GRID_BIG * 8 + 1) + 1, 2 * (GRID_BIG + 5) + 1], ids=lambda n: f"n{n}")
def test_user_module_exact_every_slot(cgo, contexts, n):
    """The run-time compiled module table (obj->rtc->cg(mode, npts, big)) — one module per objective, so fewer sizes; its tail
    code is compiled into the module, so one size runs the finalize and strict tails as well."""
    _report(_run_cg(cgo, contexts, User, n, tails=tuple(TAILS) if n == 513 else ("fused",)))


@pytest.mark.gpu
def test_default_pure_hbm_path_exact(cgo, contexts):
    """n = 2²⁵ + 17: the library's own threshold (4.5e8 bytes read-only) sends trial launches down the pure-HBM path; the
    accept + direction + trial launch stays below its 1.4e9 and runs grid-stride on 512 workgroups (two row levels)."""
    mism = _run_cg(cgo, contexts, Quad, BIG_DEFAULT_N, tails=("fused",), bigs=(False,),
                   launch_list=[("trial", R_TRIAL, 7), ("accept_dir_trial", R_ACCEPT | R_DIR | R_TRIAL, 7), ("trial", R_TRIAL, 2)])
    _report(mism)
    assert any(sym.endswith("true>") and "ObjQuadDiag" in sym for sym, n, _ in CELLS if n == BIG_DEFAULT_N)


CHAIN_SIZES = [2, 3, 17, 128, 129, 513, 2 * (GRID_BIG + 5) + 1, 2 * GRID_BIG * 8]


def chain_launches():
    L = [("init", R_INIT, 0), ("init", R_GRAD, 0), ("init", R_EDGES, 0), ("accept_dir", R_ACCEPT | R_DIR, 0),
         ("accept_only", R_ACCEPT, 0), ("reset_dir", R_RESET, 0), ("upg_norm", R_UPG, 0), ("scaled_norm", R_GRAD, 1),
         ("scaled_norm", R_GRADT, 1)]
    for k in (1, 2, 3):
        L += [("trial", R_TRIAL, k), ("accept_dir_trial", R_ACCEPT | R_DIR | R_TRIAL, k)]
    return L


def chain_data(n, seed=5):
    rng = np.random.default_rng(seed)
    return _dy(rng, n, -2, 2, 0.5, False), _dy(rng, n, -1, 1, 0.5)


CHAIN_STEPS, CHAIN_SCAL = [0.5, 1.0, 1.5], (0.5, 0.5)


def _chain_inputs(mode):
    # along u = −∇f the quartic leaves no budget on general data (see STEPS): a_acc = β = 0 and x on the valley there
    return (0.0, 0.0, True) if (mode & R_TRIAL) and (mode & R_DIR) else (*CHAIN_SCAL, False)


def _chain_x(n, valley):
    x, u = chain_data(n)
    if valley:   # x = 0: ∇f = (−2, …, −2, 0), so that the trial points along u = −∇f stay on a coarse grid
        x = np.zeros(n)
    return x, u


def test_chain_data_meet_their_preconditions():
    for n in CHAIN_SIZES:
        for kind, mode, k in chain_launches():
            a_acc, beta, valley = _chain_inputs(mode)
            x, u = _chain_x(n, valley)
            expected_chain(x, u if needs_u(mode) or mode & R_EDGES else None, mode, CHAIN_STEPS[:k], a_acc, beta)


def _run_chain(cgo, contexts, n, tails=tuple(TAILS), bigs=(False, True), launch_list=None):
    mism = []
    for tail in tails:
        for big in bigs:
            o = cgo.RosenbrockChained(n, contexts[tail])
            s = _solver(cgo, o, tail, big)
            try:
                for kind, mode, k in (launch_list or chain_launches()):
                    a_acc, beta, valley = _chain_inputs(mode)
                    x, u = _chain_x(n, valley)
                    uin = u if needs_u(mode) or mode & R_EDGES else None
                    want_sums, want = expected_chain(x, uin, mode, CHAIN_STEPS[:k], a_acc, beta)
                    got = s.probe_launch(kind, mode, a_acc, beta, CHAIN_STEPS[:k], x, uin)
                    REACHED.add(got["symbol"])
                    if _compare(f"chained n={n} {tail} {'pure-HBM' if big else 'grid-stride'} {kind}/{mode} k={k} [{got['symbol']}]",
                                got, want_sums if mode not in (R_ACCEPT, R_GRAD, R_GRADT) else np.zeros(0), want, mism):
                        CELLS[(got["symbol"], n, tail)] += 1
            finally:
                s.close(); o.close()
    return mism


@pytest.mark.gpu
@pytest.mark.parametrize("n", CHAIN_SIZES, ids=lambda n: f"n{n}")
def test_rosenbrock_chained_exact_every_slot(cgo, contexts, n):
    _report(_run_chain(cgo, contexts, n))


# ---- (b) random data against the correctly rounded sum -----------------------------------------------------------------
def two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def summation_depth(n, W, big):
    """Longest chain of additions any one term goes through in a launch with W-slot rows (each adds at most one rounding):
    the lane's own accumulation (two terms per pair, pairs i, i + step, … or one pure-HBM chunk — the k_cg chunk, which is
    never shorter than the stencil's), the wave's six exchange levels, the four waves, then the row levels (tail_sum /
    k_finalize_t: rows per lane, then G = 256 / W interleaved row groups) — twice when there are more than 64 rows — and the
    odd tail element."""
    n2 = n >> 1
    grid = GRID_BIG if big else grid_cg(n, 7 if W >= 40 else 1)
    pairs_per_lane = -(-big_chunk_pairs(n2) // BLOCK) if big else -(-n2 // (grid * BLOCK))
    G = BLOCK // W
    levels = 1 if grid <= TAIL_GROUP else 2
    rows = min(grid, TAIL_GROUP)
    return 2 * pairs_per_lane + 1 + 6 + 2 + levels * (-(-rows // G) + G)


def _slot_refs(T):
    """slot -> (correctly rounded exact sum, Σ|tᵢ|, min |tᵢ|) of the terms T[slot] (products of two factors enter exactly,
    as through one FMA; one-factor terms — the f terms — as they are)."""
    out = {}
    for slot, lst in T.items():
        parts, mags = [], []
        for fac in lst:
            fac = fac[0] if isinstance(fac[0], tuple) else fac    # (factors, per_element) of cg_model, or factors (chain)
            if len(fac) == 2:
                pp, ee = two_prod(*np.broadcast_arrays(_f(fac[0]), _f(fac[1])))
                parts += [pp, ee]
            else:
                pp = _f(fac[0])
                parts.append(pp)
            mags.append(np.abs(pp).ravel())
        m = np.concatenate(mags)
        out[slot] = (math.fsum(np.concatenate([q.ravel() for q in parts])), float(np.sum(m)), float(np.min(m)) if m.size else 0.0)
    return out


def float_cg(obj, x, u, p, x2, mode, a, a_acc, beta, with_u):
    """cg_model in plain IEEE arithmetic on whole vectors: the slot references and the vectors (bitwise: the kernels' element-wise
    arithmetic is unfused and in the same order)."""
    n, n2 = x.size, x.size >> 1
    npts = npts_for(len(a)) if mode & R_TRIAL else 1
    aa = list(a) + [a[-1]] * (npts - len(a)) if a else [0.0] * npts
    T = defaultdict(list)
    parts = {"x": [], "u": [], "g": []}
    CHECK_EXACT[0] = False
    try:
        for single, sl in ((False, slice(0, 2 * n2)), (True, slice(n - 1, n))):
            if (single and not n & 1) or (not single and n2 == 0):
                continue
            Ts, out = cg_model(obj, x[sl], u[sl], None if p is None else p[sl], x2[sl], mode, aa, a_acc, beta, single)
            for slot, lst in Ts.items():
                T[slot] += lst
            for key in parts:
                v = out.get(key)
                if v is None and key == "u" and with_u:
                    v = u[sl]
                parts[key].append(v)
    finally:
        CHECK_EXACT[0] = True
    vec = {k: (None if any(q is None for q in v) else np.concatenate(v)) for k, v in parts.items()}
    W = 0 if mode in (R_ACCEPT, R_GRAD, R_GRADT) else row_width(npts)
    return W, _slot_refs(T), vec


def random_data(kind, n, seed):
    """Random data whose every sum term is bounded away from zero (the guard below asserts it):
    quad: x, u of one sign per element, magnitudes in [1/2, 1], x2 of the other sign, D in [1, 2]; small a_acc and β keep
          u_new = −∇f(x + a_acc·u) + β·u of that sign, u + ∇f too;
    rosen: x in [−1, −1/2], t = y − x² in [1/2, 1] (∇f > 0), u = (small positive, positive): the Hessian keeps y = g⁺ − g
           positive along u; along u_new = −∇f (magnitude ~ 100) the steps are ~1e−5;
    chain: x in [−1, −1/2] (every t_k < 0, ∇f < 0), u positive."""
    rng = np.random.default_rng(seed)
    U = lambda lo, hi: rng.uniform(lo, hi, n)
    if kind == "quad":
        sg = rng.choice([-1.0, 1.0], n)
        st = list(np.sort(U(1 / 64, 1 / 8)[:7]))
        return dict(x=sg * U(0.5, 1), u=sg * U(0.5, 1), x2=-sg * U(0.5, 1), p=U(1, 2)), (1 / 16, 1 / 16), st, st
    if kind == "rosen":
        x = np.empty(n); u = np.empty(n)
        x[0::2] = U(-1, -0.5)[: n // 2]
        x[1::2] = x[0::2] ** 2 + U(0.5, 1)[: n // 2]
        u[0::2] = U(0.05, 0.1)[: n // 2]
        u[1::2] = U(0.5, 1)[: n // 2]
        return dict(x=x, u=u, x2=x.copy(), p=None), (1 / 1024, 1 / 16), list(np.sort(U(1 / 1024, 1 / 128)[:7])), \
            list(np.sort(U(1e-6, 1e-5)[:7]))
    x = U(-1, -0.5)
    return dict(x=x, u=U(0.5, 1), x2=None, p=None), (1 / 1024, 1 / 16), list(np.sort(U(1 / 4096, 1 / 1024)[:3])), \
        list(np.sort(U(1e-7, 1e-6)[:3]))


def _b_launches(kind):
    if kind == "chain":
        return [c for c in chain_launches() if c[1] != R_EDGES]
    L = launches("quad_diag")
    if kind == "rosen":   # the projection: x2 + m·∇f(z) with ∇f ~ 100 has no sign to keep; covered exactly in (a)
        L = [c for c in L if c[1] != R_PROJ]
    return L


B_SIZES = {"quad": [17, 513, 2 * (GRID_BIG + 5) + 1, 2 * GRID_BIG * 16 + 1],
           "rosen": [16, 512, 2 * (GRID_BIG + 5), 2 * GRID_BIG * 16],
           "chain": [17, 513, 2 * (GRID_BIG + 5) + 1, 2 * GRID_BIG * 8 + 1]}


def b_expected(kind, n, mode, k, data, scal, steps_u, steps_g):
    a_acc, beta = scal
    along_g = (mode & R_TRIAL) and (mode & R_DIR)
    a = (steps_g if along_g else steps_u)[:k]
    if along_g and kind != "quad":
        a_acc = 0.0
    if kind == "chain":
        T = {}
        CHECK_EXACT[0] = False
        try:
            _, vec = expected_chain(data["x"], data["u"] if needs_u(mode) else None, mode, a, a_acc, beta, terms_out=T)
        finally:
            CHECK_EXACT[0] = True
        npts = 3 if (mode & R_TRIAL) and k >= 2 else 1
        W = 0 if mode in (R_ACCEPT, R_GRAD, R_GRADT) else (24 if npts == 1 else 32)
        nsums = RS * npts + 2 if W else 0   # (the edge values behind the sums: checked in (a))
        return a, a_acc, W, nsums, _slot_refs(T), vec
    obj = Quad if kind == "quad" else Rosen
    W, refs, vec = float_cg(obj, data["x"], data["u"], data["p"], data["x2"], mode, a, a_acc, beta, needs_u(mode))
    return a, a_acc, W, W, refs, vec


def _b_check(tag, got, W, nsums, refs, vec, depth_W, n, big, mism):
    if got["sums"].size != W:
        mism.append(f"{tag}: row of {got['sums'].size} slots, expected {W}")
        return
    d = summation_depth(n, depth_W, big)
    gam = d * 2.0 ** -53 / (1 - d * 2.0 ** -53)
    for slot in range(nsums):
        v = got["sums"][slot]
        if slot not in refs:
            if v != 0.0:
                mism.append(f"{tag}: slot {slot} carries no term, holds {v!r}")
            continue
        exact, absum, tmin = refs[slot]
        bound = gam * absum * (1 + 1e-12)
        assert tmin > bound, f"test data: {tag} slot {slot}: smallest term {tmin:.3e} within the bound {bound:.3e}"
        if not abs(v - exact) <= bound:
            mism.append(f"{tag}: slot {slot} {v!r} vs {exact!r} (bound {bound:.3e})")
    for key in ("x", "u", "g"):
        w, g = vec.get(key), got[key]
        wb = np.full(g.size, NAN_BITS) if w is None else bits(w)
        if not np.array_equal(bits(g), wb):
            i = int(np.nonzero(bits(g) != wb)[0][0])
            mism.append(f"{tag}: {key}_out differs first at element {i}: got {g[i]!r}, want {'NaN' if w is None else repr(w[i])}")


def test_random_data_meet_the_guard():
    """CPU tier: every slot of every launch of (b) has its smallest term above its bound, on both streaming policies."""
    for kind, sizes in B_SIZES.items():
        for n in sizes:
            data, scal, su, sg = random_data(kind, n, 2000 + n)
            for _, mode, k in _b_launches(kind):
                a, a_acc, W, nsums, refs, vec = b_expected(kind, n, mode, k, data, scal, su, sg)
                for big in (False, True):
                    d = summation_depth(n, W or 10, big)
                    for slot, (exact, absum, tmin) in refs.items():
                        assert tmin > d * 2.0 ** -53 * absum * 1.01, (kind, n, mode, k, slot, tmin, absum)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [(kd, n) for kd, ns in B_SIZES.items() for n in ns], ids=lambda v: str(v))
def test_random_within_summation_bound(cgo, contexts, kind, n):
    """Every launch mode and point count of QuadDiag, paired and chained Rosenbrock, grid-stride and pure-HBM, every tail, on
    random data: each slot within γ_d·Σ|tᵢ| of the correctly rounded sum of its exact terms, γ_d = d·u / (1 − d·u),
    u = 2⁻⁵³, d = the launch's summation depth (summation_depth) — the classical bound of recursive summation, c = 1: the
    products enter exactly (one FMA each) and every addition on a term's path to the row is one rounding.  Each slot's
    smallest term is asserted to exceed its bound, so a dropped or doubled element cannot hide in it; slots without terms
    must be zero and the vectors equal bit for bit (unfused element-wise arithmetic in the kernels' order)."""
    data, scal, su, sg = random_data(kind, n, 2000 + n)
    cache = {}
    mism = []
    for tail in TAILS:
        for big in (False, True):
            ctx = contexts[tail]
            o = cgo.QuadDiag(data["p"], ctx) if kind == "quad" else (cgo.RosenbrockPaired(n, ctx) if kind == "rosen" else cgo.RosenbrockChained(n, ctx))
            s = _solver(cgo, o, tail, big)
            try:
                for kd, mode, k in _b_launches(kind):
                    if (mode, k) not in cache:
                        cache[(mode, k)] = b_expected(kind, n, mode, k, data, scal, su, sg)
                    a, a_acc, W, nsums, refs, vec = cache[(mode, k)]
                    got = s.probe_launch(kd, mode, a_acc, scal[1], a, data["x"], data["u"] if needs_u(mode) else None,
                                         data["x2"] if mode & R_PROJ else None)
                    REACHED.add(got["symbol"])
                    _b_check(f"{kind} n={n} {tail} {'pure-HBM' if big else 'grid'} {kd}/{mode} k={k} [{got['symbol']}]",
                             got, W, nsums, refs, vec, W or 10, n, big, mism)
            finally:
                s.close(); o.close()
    _report(mism)


# ---- (c) log-sum-exp ---------------------------------------------------------------------------------------------------
LSE_CASES = {
    "dominant": lambda n, rng: (np.where(np.arange(n) == n // 3, 40.0, rng.uniform(-1, 1, n)), rng.uniform(-1, 1, n)),
    "all-equal": lambda n, rng: (np.full(n, 0.75), np.full(n, -0.5)),
    "near+700": lambda n, rng: (700.0 + rng.uniform(-2, 2, n), rng.uniform(-1, 1, n)),
    "near-700": lambda n, rng: (-700.0 + rng.uniform(-2, 2, n), rng.uniform(-1, 1, n)),
    "max-moves": lambda n, rng: (np.where(np.arange(n) == 0, 3.0, 0.0) + rng.uniform(-0.1, 0.1, n),
                                 np.where(np.arange(n) == n - 1, 8.0, 0.0)),   # a = 1: the maximum moves from element 0 to n−1
}


def lse_reference(xp, u, lam):
    import mpmath as mp
    mp.mp.dps = 50
    xs = [mp.mpf(float(v)) for v in xp]
    m = max(xs)
    Sx = mp.fsum(mp.e ** (v - m) for v in xs)
    lse = m + mp.log(Sx)
    sm = [mp.e ** (v - lse) for v in xs]
    phi = lse + mp.mpf(lam) / 2 * mp.fsum(v * v for v in xs)
    dphi = mp.fsum(s * float(w) for s, w in zip(sm, u)) + mp.mpf(lam) * mp.fsum(v * float(w) for v, w in zip(xs, u))
    g = [s + mp.mpf(lam) * v for s, v in zip(sm, xs)]
    return phi, dphi, g


LSE_U = 2.0 ** -53


def _lse_gamma(n, big):
    """γ_d for the log-sum-exp launches: d = 2·(pairs per lane) + 16 (each lane's running (max, Σ) rescales at most once per
    element, then 6 + 2 wave levels) + 2·⌈log₂ rows⌉ (the row merges of k_finalize_lse, ≤ 1024 rows per stage)."""
    d = 2 * (-(-(n >> 1) // (BLOCK * (GRID_BIG if big else 1)))) + 16 + 8 + 2 * math.ceil(math.log2(max(GRID_BIG if big else 1024, 2)))
    return d * LSE_U / (1 - d * LSE_U)


def _lse_phi_check(tag, row, xp, uu, lam, gam, ref, mism):
    """ϕ, dϕ from a k_lse_stats row as the engine forms them, against the mpmath reference (phi_r, dphi_r); Q, R against the
    correctly rounded sums of the device's own terms.  Tolerances (u = 2⁻⁵³, eₖ = exp(xpₖ − M)):
      ϕ:  δS/S ≤ (Σ eₖ·(2 + |xpₖ − M|)·u)/S + γ_d       (1 ulp for exp plus the rounding of its argument; the summation)
          |Δϕ| ≤ 2·(δS/S + 4u·(|M| + |log S|) + λ/2·γ_d·Q)
      dϕ: |Δ| ≤ 2·((Σ eₖ|uₖ|(2 + |xpₖ − M|)u + γ_d Σ eₖ|uₖ|)/S + |T/S|·(δS/S + u) + λ·γ_d·Σ|xpₖuₖ|)
    The factor 2 covers the second-order terms and the final additions; nothing here is fitted to the results."""
    phi_r, dphi_r = ref
    Mx, Sx, Tx, Q, R = row[0], row[1], row[2], row[3], row[4]
    phi = (Mx + math.log(Sx)) + 0.5 * lam * Q
    dphi = Tx / Sx + lam * R
    if Mx != xp.max():
        mism.append(f"{tag}: M {Mx!r} is not max xp {xp.max()!r}")
    e = np.exp(xp - Mx)
    Sr = float(np.sum(e))
    dS = float(np.sum(e * (2 + np.abs(xp - Mx)))) * LSE_U / Sr + gam
    tol_phi = 2 * (dS + 4 * LSE_U * (abs(Mx) + abs(math.log(Sr))) + 0.5 * lam * gam * float(np.sum(xp * xp)))
    eu = float(np.sum(e * np.abs(uu)))
    tol_dphi = 2 * ((float(np.sum(e * np.abs(uu) * (2 + np.abs(xp - Mx)))) * LSE_U + gam * eu) / Sr
                    + abs(Tx / Sx) * (dS + LSE_U) + lam * gam * float(np.sum(np.abs(xp * uu))))
    if not abs(phi - float(phi_r)) <= tol_phi:
        mism.append(f"{tag}: ϕ {phi!r} vs {float(phi_r)!r} (tol {tol_phi:.2e})")
    if not abs(dphi - float(dphi_r)) <= tol_dphi:
        mism.append(f"{tag}: dϕ {dphi!r} vs {float(dphi_r)!r} (tol {tol_dphi:.2e})")
    _lse_sums_check(tag, row, {3: (xp, xp), 4: (xp, uu)}, gam, mism)
    return Mx, Sr, dS


def _lse_sums_check(tag, row, slot_terms, gam, mism):
    """slots formed as plain Σ l·r (one rounding per product, then the summation): within (γ_d + u)·Σ|l·r| of the
    correctly rounded exact sum."""
    for slot, (l, r) in slot_terms.items():
        p, ee = two_prod(*np.broadcast_arrays(_f(l), _f(r)))
        ex = math.fsum(np.concatenate([p, ee]))
        bound = (gam + LSE_U) * float(np.sum(np.abs(p))) * 1.01
        if not abs(row[slot] - ex) <= bound:
            mism.append(f"{tag}: slot {slot} {row[slot]!r} vs {ex!r} (bound {bound:.2e})")


def _lse_zero_slots(tag, row, used, mism):
    for slot in range(10):
        if slot not in used and row[slot] != 0.0:
            mism.append(f"{tag}: padding slot {slot} holds {row[slot]!r}")


def _lse_grad_check(tag, gr, xp, uu, g, lam, Mx, Sr, dS, gref, beta_sums, mism, gam):
    """g⁺ₖ: |Δ| ≤ 2·(softmaxₖ·((3 + |xpₖ − M|)·u + δS/S) + λ|xpₖ|·u) against mpmath; the row's sums against those of the
    device's own g⁺ (and the stored g): GTU, GTGT and — with β — GTG, YY, UY, YGT, y = g⁺ − g; every other slot zero."""
    sm = np.exp(xp - Mx) / Sr
    tol_g = 2 * (sm * ((3 + np.abs(xp - Mx)) * LSE_U + dS) + lam * np.abs(xp) * LSE_U)
    bad = np.nonzero(~(np.abs(gr["g"] - gref) <= tol_g))[0]
    if bad.size:
        i = int(bad[0])
        mism.append(f"{tag}: g⁺[{i}] {gr['g'][i]!r} vs {gref[i]!r} (tol {tol_g[i]:.2e})")
    gt = gr["g"]
    terms = {2: (gt, gt)}
    if uu is not None:
        terms[1] = (gt, uu)
    if beta_sums:
        y = gt - g
        terms.update({3: (gt, g), 4: (y, y), 5: (uu, y), 6: (y, gt)})
    _lse_sums_check(tag, gr["sums"], terms, gam, mism)
    _lse_zero_slots(tag, gr["sums"], set(terms), mism)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(LSE_CASES))
@pytest.mark.parametrize("n", [1, 3, 17, 513, 2 * (GRID_BIG + 5) + 1], ids=lambda n: f"n{n}")
def test_lse_stats_and_grad_against_mpmath(cgo, contexts, case, n):
    """k_lse_stats (trial at a: ϕ, dϕ, Q, R) and k_lse_grad with the getβ sums (stored gradient g seeded, nonzero) against
    50 digits and the correctly rounded sums of the device's own element-wise values (tolerances: _lse_phi_check,
    _lse_grad_check); padding slots zero.  λ = 1e−3 also runs the other launches the engine issues: the fused accept +
    direction + trial (x, u bit for bit, Σ g·u_new, Σ u_new²), the evaluation at x with the initial gradient (u = −g⁺ bit for
    bit) and g⁺ without the β sums."""
    rng = np.random.default_rng(77 + n)
    x, u = LSE_CASES[case](n, rng)
    g = rng.uniform(-1, 1, n)
    a = 1.0 if case == "max-moves" else 0.5
    a_acc, beta = 0.25, 0.5
    mism = []
    for lam in (0.0, 1e-3, 1.0):
        xp = x + a * u
        phi_r, dphi_r, g_r = lse_reference(xp, u, lam)
        gref = np.array([float(v) for v in g_r])
        more = lam == 1e-3
        if more:
            x1 = x + a_acc * u
            un = -g + beta * u
            xq = x1 + a * un
            ref_q = lse_reference(xq, un, lam)
            ref_0 = lse_reference(x, np.zeros(n), lam)
        for big in (False, True):
            o = cgo.LogSumExp(n, lam, contexts["fused"])
            s = _solver(cgo, o, "fused", big)
            tag = f"{case} n={n} λ={lam} {'pure-HBM' if big else 'grid'}"
            gam = _lse_gamma(n, big)
            try:
                st = s.probe_launch("lse_stats", 0, 0.0, 0.0, [a], x, u)
                Mx, Sr, dS = _lse_phi_check(tag + " stats", st["sums"], xp, u, lam, gam, (phi_r, dphi_r), mism)
                _lse_zero_slots(tag + " stats", st["sums"], {0, 1, 2, 3, 4}, mism)
                gr = s.probe_launch("lse_grad", 1, 0.0, 0.0, [a], x, u, aux=g)
                _lse_grad_check(tag + " grad+β", gr, xp, u, g, lam, Mx, Sr, dS, gref, True, mism, gam)
                REACHED.update((st["symbol"], gr["symbol"]))
                if more:
                    gr0 = s.probe_launch("lse_grad", 0, 0.0, 0.0, [a], x, u)
                    _lse_grad_check(tag + " grad", gr0, xp, u, None, lam, Mx, Sr, dS, gref, False, mism, gam)
                    st3 = s.probe_launch("lse_stats", 3, a_acc, beta, [a], x, u, aux=g)
                    if not (np.array_equal(bits(st3["x"]), bits(x1)) and np.array_equal(bits(st3["u"]), bits(un))):
                        mism.append(f"{tag} accept+dir: x / u after the launch differ from x + a·u, −g + β·u")
                    _lse_phi_check(tag + " accept+dir", st3["sums"], xq, un, lam, gam, ref_q[:2], mism)
                    _lse_sums_check(tag + " accept+dir", st3["sums"], {7: (g, un), 8: (un, un)}, gam, mism)
                    _lse_zero_slots(tag + " accept+dir", st3["sums"], {0, 1, 2, 3, 4, 7, 8}, mism)
                    st4 = s.probe_launch("lse_stats", 4, 0.0, 0.0, [], x)
                    M0, S0, dS0 = _lse_phi_check(tag + " at x", st4["sums"], x, np.zeros(n), lam, gam, ref_0[:2], mism)
                    gi = s.probe_launch("lse_grad", 2, 0.0, 0.0, [], x)
                    _lse_grad_check(tag + " init", gi, x, None, None, lam, M0, S0, dS0, np.array([float(v) for v in ref_0[2]]),
                                    False, mism, gam)
                    if not np.array_equal(bits(gi["u"]), bits(-gi["g"])):
                        mism.append(f"{tag} init: u is not −g⁺")
                    REACHED.update((gr0["symbol"], st3["symbol"], st4["symbol"], gi["symbol"]))
            finally:
                s.close(); o.close()
    _report(mism)


# ---- (d) coverage --------------------------------------------------------------------------------------------------------
def expected_cg_instantiations():
    out = set()
    for kind, mode, k in launches("quad_diag"):
        out.add((mode, npts_for(k) if mode & R_TRIAL else 1))
    return out


def expected_chain_instantiations():
    return {(mode, 3 if (mode & R_TRIAL) and k >= 2 else 1) for kind, mode, k in chain_launches()}


def test_dispatch_tables_have_tests():
    """CPU tier: every instantiation launch_cg / launch_chain can dispatch (the rows of csrc/cgo_instances.def they expand
    from) is in this module's launch lists: a new variant cannot be added without a test.  The armed form exists for the
    points of its mode's rows and for no other mode."""
    assert I.mode_points("CG") == expected_cg_instantiations()
    assert I.mode_points("CHAIN") == expected_chain_instantiations()
    assert I.mode_points("CG_ARMED") == {(m, p) for m, p in I.mode_points("CG") if m == R_ACCEPT | R_DIR | R_TRIAL}


def test_no_launch_outside_the_table():
    """CPU tier: what makes the rows "everything the dispatcher can launch" — in csrc/*.hip no kernel of the table's families
    (k_cg, k_cg_armed, k_chain, k_fused, k_resident, k_resident_chain) is launched or has its address taken anywhere but in
    the macros that expand the table."""
    assert I.stray_uses() == []


@pytest.mark.gpu
def test_coverage_of_every_instantiation(cgo, contexts):
    """Every k_cg instantiation of the built-in objectives and the run-time compiled one (both streaming policies) and every
    k_chain instantiation for one rank was launched by a probe whose row and vectors were checked.  After the whole module
    the tests above have reached them all; an instantiation they have not (this test run on its own, or the module split or
    reordered) is probed here, at one small size, against the exact reference of (a) — so the assertion does not depend
    on what else ran."""
    ON = {"ObjQuadDiag": (Quad, 17), "ObjRosenPaired": (Rosen, 16), "ObjBooth": (Booth, 2), "UserObjective": (User, 17)}
    want = set()
    for on in ON:
        for mode, npts in expected_cg_instantiations():
            for big in ("false", "true"):
                want.add(f"k_cg<{on}, {mode}, {npts}, {big}>")
    for mode, npts in expected_chain_instantiations():
        for big in ("false", "true"):
            if mode == R_EDGES and big == "true":
                continue   # moves no vector bytes (bytes_r = 0): no streaming threshold, not even 1 byte, makes it pure-HBM
            want.add(f"k_chain<{mode}, {npts}, {big}>")
    missing = want - REACHED
    mism = []
    for on, (obj, n) in ON.items():
        for big in (False, True):
            todo = [(kd, mode, k) for kd, mode, k in launches(obj.name)
                    if f"k_cg<{on}, {mode}, {npts_for(k) if mode & R_TRIAL else 1}, {str(big).lower()}>" in missing]
            if todo:
                mism += _run_cg(cgo, contexts, obj, n, tails=("fused",), bigs=(big,), launch_list=todo)
    for big in (False, True):
        todo = [(kd, mode, k) for kd, mode, k in chain_launches()
                if f"k_chain<{mode}, {3 if (mode & R_TRIAL) and k >= 2 else 1}, {str(big).lower()}>" in missing]
        if todo:
            mism += _run_chain(cgo, contexts, 17, tails=("fused",), bigs=(big,), launch_list=todo)
    _report(mism)
    still = sorted(want - REACHED)
    assert not still, f"{len(still)} instantiations never probed: {still[:10]}"
    bitwise = sum(1 for (sym, n, tail) in CELLS if sym.startswith(("k_cg", "k_chain")))
    print(f"\n[kernel sums] {bitwise} (instantiation, size, tail) cells checked bit for bit, {sum(CELLS.values())} launches")
