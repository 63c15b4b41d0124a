"""Every sum slot and vector of every pass of the batched solves, in EVERY workgroup (cgo_batch_probe).

The batch suites (tests/test_batch*.py) see the device side of k_batch, k_batch_rows and k_batch_lbfgs only as whole
trajectories.  Here a script of passes runs in ONE launch of the kernel's PROBE twin — the product kernel with the script in
place of its scalar loop — on a batch in which every problem has ITS OWN data (a seed per problem: a workgroup that reads a
neighbour's row fails bit for bit), and everything the launch leaves is compared:

(a) exact dyadic data: every product and element-wise sum is exact in double and each slot's Σ|t| stays below 2⁵³ quanta (the
    witnesses of tests/test_kernel_sums.py), so ANY summation order gives the same bits.  All W slots of every workgroup's row
    after every pass — padded points, padding slots +0.0, the 64 − W doubles behind a narrow row untouched — and x, u and every
    ring row after the launch, bit for bit; the padding element of an odd n still the NaN pattern in every row and no sum NaN:
    it was neither read nor written.  After a push: x = xp, the free slot = (s, y), every other ring slot untouched, the slots
    of absent pairs and 54–63 of the row +0.0, and the QnState word for word what qn_update + qn_coefficients of cgo_qn.hpp
    make of the device's own row on the host (tests/hostsim).  After a combine: u bitwise the unfused restatement
    −γ·g, + cy_j·Y_j (j ascending), + cs_j·S_j (j ascending).
(b) the dropped candidate (s·y < 0 exactly): the old count, only sg / yg of the stored pairs change, the rejected pair lies in
    the free slot, the next combine does not read it and the next push overwrites it.
(c) s_j·y ≠ y_j·s: pushes on paired Rosenbrock, where the two slots differ (asserted on the CPU tier).
(d) run-time compiled objectives that read a scalar per problem and four parameter slots.
(e) random data: the LDS tier's rows bitwise the device-rows tier's, pass by pass; every slot of all three tiers within
    γ_d·Σ|t| of the correctly rounded exact sum, d from the geometry; vectors bitwise the plain IEEE model's.
(f) skipped problems keep their bits; (g) the results' gradient; (h) every instantiation of the table was launched.
"""
import ctypes as C
import math
import os
import re
import subprocess
from collections import defaultdict
from contextlib import contextmanager

import numpy as np
import pytest

import _instances as I
from test_kernel_sums import (CHECK_EXACT, NAN_BITS, R_ACCEPT, R_DIR, R_INIT, R_TRIAL, RS, A, Booth, M, Quad, Rosen, S, _dy,
                              _slot_refs, bits, cg_model, exact_sum, random_data)
from test_lbfgs_kernel_sums import slot_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW = 64                                   # stride of a stored row
QS_PAIR0, QP_PER_PAIR, QN_MAX_M, QN_SLOTS = 4, 5, 10, 11
SJYN, YJSN = 2, 3                          # s_j·y and y_j·s within a pair's five sums


def _define(header, name):
    return int(re.search(r"^#define %s (\d+)" % name, open(os.path.join(I.CSRC, header)).read(), re.M).group(1))


# ---- geometry: parsed from the sources (asserted against the library on the GPU tier) ------------------------------------
BLOCK = 256
U = {"lds": 2,                                                            # ResDev::pass: two independent pairs per trip
     "device": _define("cgo_kernels_batch_rows.hip.hpp", "CGO_BATCH_ROWS_U"),
     "lbfgs": _define("cgo_kernels_batch_lbfgs.hip.hpp", "CGO_BATCH_LBFGS_U")}
RES_BUDGET, RES_STOP = (int(re.search(r"\b%s = (\d+)," % k, open(os.path.join(I.CSRC, "cgo_resident.hpp")).read()).group(1))
                        for k in ("RES_BUDGET", "RES_STOP"))
TIER_KERNEL = {"lds": "k_batch", "device": "k_batch_rows", "lbfgs": "k_batch_lbfgs"}
TIER_FAMILY = {"lds": "BATCH", "device": "BATCH_DEVROWS", "lbfgs": "BATCH_LBFGS"}


def pair_counts(u):
    return [1, BLOCK - 1, BLOCK, BLOCK + 1, u * BLOCK - 1, u * BLOCK, u * BLOCK + 1, 2 * u * BLOCK + BLOCK + 1]


def sizes(tier, odd_too=True):
    out = [] if not odd_too else [1, 3]
    for c in pair_counts(U[tier]):
        out += [2 * c] + ([2 * c + 1] if odd_too else [])
    return sorted(set(out))


def test_sizes_hit_the_edges_they_claim():
    """CPU tier: with U pairs per lane and trip, the pair counts are one pair, around one pair per lane, around one whole
    trip, and two whole trips plus a partial one whose last lane-block holds a single pair."""
    assert "two independent pairs per trip" in open(os.path.join(I.CSRC, "cgo_kernels_resident.hip.hpp")).read()
    for tier, u in U.items():
        assert 1 <= u <= 8
        trip = u * BLOCK
        c = pair_counts(u)
        assert c[4] // trip == 0 and c[5] // trip == 1 and c[5] % trip == 0 and c[6] % trip == 1
        assert c[7] // trip == 2 and c[7] % trip == BLOCK + 1     # TAIL trip: lane 0 holds two pairs, lane 1 … one, clamped beyond
        ns = sizes(tier)
        assert {1, 3, 2, 2 * trip + 3}.issubset(ns) and all((n ^ 1) in ns or n in (1, 2, 3) for n in ns if n > 3)
        assert max(ns) <= 2 * (2 * 8 * BLOCK + BLOCK + 1) + 1 and max(ns) < 10500


# ---- arithmetic: the exact witnesses of test_kernel_sums, or plain IEEE ---------------------------------------------------
@contextmanager
def arith(exact):
    old = CHECK_EXACT[0]
    CHECK_EXACT[0] = exact
    try:
        yield
    finally:
        CHECK_EXACT[0] = old


class UserQ0(Quad):
    """no parameter slot"""
    name, K, SOURCE, param = "user_q0", 0, "gi = x; fi = 0.5*(x*x);", False

    @staticmethod
    def g2(x, p):
        return M(0.5, M(x, x)), x + 0.0

    g1 = g2


class UserSM(Quad):
    """reads s0 and three slots (tests/test_batch_scalars.py: SM)"""
    name, K = "user_sm", 3
    SOURCE = "const double d = x - p1; gi = s0*(p*d + p2); fi = s0*(0.5*((p*d)*d) + p2*x);"

    def __init__(self, s0):
        self.s0 = s0

    def g2(self, x, p):
        d = S(x, p[1])
        pd = M(p[0], d)
        return M(self.s0, A(M(0.5, M(pd, d)), M(p[2], x))), M(self.s0, A(pd, p[2]))

    g1 = g2


class UserQ4(Quad):
    """four slots (tests/test_param_slots.py: BODY[4])"""
    name, K = "user_q4", 4
    SOURCE = "const double d = x - p1; gi = (p*d + p2) + p3; fi = (0.5*((p*d)*d) + p2*x) + p3*x;"

    def g2(self, x, p):
        d = S(x, p[1])
        pd = M(p[0], d)
        return A(A(M(0.5, M(pd, d)), M(p[2], x)), M(p[3], x)), A(A(pd, p[2]), p[3])

    g1 = g2


def _psl(p, sl):
    return None if p is None else p[..., sl]


def _parts(n):
    n2 = n >> 1
    return ([(False, slice(0, 2 * n2))] if n2 else []) + ([(True, slice(n - 1, n))] if n & 1 else [])


def grad(obj, x, p):
    g = np.empty_like(x)
    for single, sl in _parts(x.size):
        g[sl] = (obj.g1 if single else obj.g2)(x[sl], _psl(p, sl))[1]
    return g


def cg_pass(obj, x, u, p, mode, a, a_acc, beta):
    """one pass of ResDev / RowsDev on one problem: (T: slot → factor tuples, x', u')"""
    T = defaultdict(list)
    xn, un = x.copy(), u.copy()
    for single, sl in _parts(x.size):
        Ts, out = cg_model(obj, x[sl], u[sl], _psl(p, sl), None, mode, list(a), a_acc, beta, single)
        for s, lst in Ts.items():
            T[s] += [fac for fac, _ in lst]
        xn[sl] = out["x"]
        if "u" in out:
            un[sl] = out["u"]
    return T, xn, un


def push_pass(obj, x, u, p, Sr, Yr, lst, free, a):
    """LbfgsDev::push_update's pass: (T, xp, ring with (s, y) in the free slot)"""
    g = grad(obj, x, p)
    s = M(a, u)
    xp = A(x, s)
    gp = grad(obj, xp, p)
    y = S(gp, g)
    T = {0: [(s, y)], 1: [(y, y)], 2: [(s, gp)], 3: [(y, gp)]}
    for j, q in enumerate(lst):
        b = QS_PAIR0 + QP_PER_PAIR * j
        for k, fac in enumerate(((Sr[q], gp), (Yr[q], gp), (Sr[q], y), (Yr[q], s), (Yr[q], y))):
            T[b + k] = [fac]
    S2, Y2 = Sr.copy(), Yr.copy()
    S2[free], Y2[free] = s, y
    return T, xp, S2, Y2


def combine_pass(obj, x, p, Sr, Yr, lst, gamma, cy, cs, a):
    """LbfgsDev::combine_trial: u in the kernel's order, g·u, u·u and the trial block on (x, u)"""
    g = grad(obj, x, p)
    u = M(-gamma, g)
    for j, q in enumerate(lst):
        u = A(u, M(cy[j], Yr[q]))
    for j, q in enumerate(lst):
        u = A(u, M(cs[j], Sr[q]))
    T, _, _ = cg_pass(obj, x, u, p, R_TRIAL, a, 0.0, 0.0)
    T[3 * RS] = [(g, u)]
    T[3 * RS + 1] = [(u, u)]
    return T, u


def exact_row(T, W):
    """the row's bits: W slots (slots without terms +0.0), the NaN pattern behind them"""
    row = np.full(ROW, NAN_BITS, dtype=np.int64)
    v = np.zeros(W)
    for s, lst in T.items():
        terms = [M(*fac) if len(fac) == 2 else fac[0] for fac in lst]
        v[s] = exact_sum(terms, [np.ones(np.size(t), np.int64) for t in terms])
    row[:W] = bits(v)
    return row


def sim_row(T, W):
    """CPU tier stand-in for a device row: every slot the correctly rounded exact sum of its terms"""
    row = np.full(ROW, NAN_BITS, dtype=np.int64)
    v = np.zeros(W)
    for s, (ex, _, _) in _slot_refs(T).items():
        v[s] = ex
    row[:W] = bits(v)
    return row


def depth(n):
    """Longest chain of additions a term goes through in one workgroup's pass: the busiest lane's own accumulation (lane 0:
    ⌈npairs / BLOCK⌉ pairs, two terms each, and the odd tail element), then wg_reduce_n over 256 lanes: six exchange levels
    within a wave, three additions across the four waves."""
    lane = 2 * -(-(n >> 1) // BLOCK) + (n & 1)
    wave_levels, across_waves = 6, 3
    return lane + wave_levels + across_waves


def check_row_bound(tag, got_bits, T, W, n, mism):
    """(e)(ii): every slot within γ_d·Σ|t| of the correctly rounded exact sum; slots without terms +0.0; the tail untouched"""
    d = depth(n)
    gam = d * 2.0 ** -53 / (1 - d * 2.0 ** -53)
    refs = _slot_refs(T)
    row = got_bits.view(np.float64)
    for s in range(W):
        if s not in refs:
            if got_bits[s] != 0:
                mism.append(f"{tag}: slot {s} carries no term, holds {row[s]!r}")
            continue
        ex, absum, tmin = refs[s]
        if absum == 0.0:       # every term an exact zero (y = g⁺ − g at a step of 0): the sum is +0.0, no room at all
            if got_bits[s] != 0:
                mism.append(f"{tag}: slot {s} sums exact zeros, holds {row[s]!r}")
            continue
        bound = gam * absum * (1 + 1e-12)
        assert tmin > bound, f"test data: {tag} slot {s}: smallest term {tmin:.3e} within the bound {bound:.3e}"
        if not abs(row[s] - ex) <= bound:
            mism.append(f"{tag}: slot {s} {row[s]!r} vs {ex!r} (bound {bound:.3e})")
    if not np.all(got_bits[W:] == NAN_BITS):
        mism.append(f"{tag}: something was stored behind the {W} slots of the row")


# ---- the quasi-Newton state as the kernel holds it (csrc/cgo_qn.hpp) ------------------------------------------------------
QN = np.dtype([("m", "i4"), ("count", "i4"), ("free_slot", "i4"), ("pad", "i4"), ("list", "i4", QN_SLOTS + 1), ("gamma", "f8"),
               ("rho", "f8", QN_SLOTS), ("sg", "f8", QN_SLOTS), ("yg", "f8", QN_SLOTS), ("SY", "f8", QN_SLOTS * QN_SLOTS),
               ("YY", "f8", QN_SLOTS * QN_SLOTS)])
COEF = np.dtype([("count", "i4"), ("pad", "i4"), ("gamma", "f8"), ("cy", "f8", QN_MAX_M), ("cs", "f8", QN_MAX_M),
                 ("a", "f8", QN_MAX_M), ("c", "f8", QN_MAX_M)])


def test_the_state_mirror_matches_the_header():
    src = open(os.path.join(I.CSRC, "cgo_qn.hpp")).read()
    assert int(re.search(r"QN_MAX_M = (\d+)", src).group(1)) == QN_MAX_M and "QN_SLOTS = QN_MAX_M + 1" in src
    assert int(re.search(r"QN_SUMS = (\d+)", src).group(1)) == ROW
    assert "enum QnSum : int { QS_SY = 0, QS_YY, QS_SGN, QS_YGN, QS_PAIR0 }" in src
    assert "enum QnPairSum : int { QP_SJG = 0, QP_YJG, QP_SJYN, QP_YJSN, QP_YJYN, QP_PER_PAIR }" in src
    body = re.sub(r"//.*", "", src[src.index("struct QnState {"):src.index("static_assert(sizeof(QnState)")])
    assert re.findall(r"\b(m|count|free_slot|pad_|list|gamma|rho|sg|yg|SY|YY)\b(?=[,;\[])", body) == \
        ["m", "count", "free_slot", "pad_", "list", "gamma", "rho", "sg", "yg", "SY", "YY"]
    assert QN.itemsize % 8 == 0 and QN.itemsize == 8 * (2 + 6 + 1 + 3 * QN_SLOTS + 2 * QN_SLOTS ** 2)


def qn_state(m, lst, free, rng):
    """a state with `lst` stored (newest first), `free` the candidate's slot, dyadic scalars"""
    q = np.zeros((), dtype=QN)
    q["m"], q["count"], q["free_slot"] = m, len(lst), free
    q["list"][:len(lst)] = lst
    q["gamma"] = 0.5
    P = m + 1
    for name, size in (("rho", QN_SLOTS), ("sg", QN_SLOTS), ("yg", QN_SLOTS), ("SY", QN_SLOTS ** 2), ("YY", QN_SLOTS ** 2)):
        q[name][:] = _dy(rng, size, 1, 8, 0.125)
    q["SY"][P * P:] = 0.0
    q["YY"][P * P:] = 0.0
    return q


@pytest.fixture(scope="module")
def simq(tmp_path_factory):
    """qn_update + qn_coefficients of cgo_qn.hpp, compiled with the host compiler (tests/hostsim/sim_batch_lbfgs.cpp)"""
    so = tmp_path_factory.mktemp("simq_sums") / "libsim_batch_lbfgs.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unknown-pragmas", "-shared",
                    "-o", str(so), os.path.join(ROOT, "tests", "hostsim", "sim_batch_lbfgs.cpp")], check=True)
    L = C.CDLL(str(so))
    L.simq_update.restype = C.c_int
    L.simq_update.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    assert L.simq_state_bytes() == QN.itemsize and L.simq_coef_bytes() == COEF.itemsize
    return L


def host_update(L, q, row_bits):
    """(state', coefficients, kept) of lane 0's recursion on the 64 sums `row_bits`"""
    qi = np.ascontiguousarray(np.asarray(q, dtype=QN).reshape(1))
    sums = np.ascontiguousarray(row_bits.view(np.float64))
    qo, co, kept = np.zeros(1, dtype=QN), np.zeros(1, dtype=COEF), C.c_int32(-1)
    assert L.simq_update(qi.ctypes.data, sums.ctypes.data, qo.ctypes.data, co.ctypes.data, C.byref(kept)) == 0
    return qo[0], co[0], bool(kept.value)


def words(q):
    return np.ascontiguousarray(np.asarray(q, dtype=QN).reshape(-1)).view(np.uint64).reshape(-1, QN.itemsize // 8)


# ---- data: every problem its own ------------------------------------------------------------------------------------------
STEPS = [0.25, 0.5, 0.75]


def exact_problem(obj, n, seed, ring=None):
    """dyadic x, u and slots of one problem; ring = (m, listed slots): S, Y [m + 1][n], absent slots NaN"""
    rng = np.random.default_rng(seed)
    if obj is Booth:
        k = rng.integers(-3, 4, 4)
        d = dict(x=np.array([0.5, 1.25]) + 0.25 * k[:2], u=np.array([-0.25, 0.75]) + 0.25 * k[2:], p=None)
    elif obj is Rosen:       # the valley: pairs (t, t²), t ∈ {1/2, 1} — ∇f = (−2(1 − t), 0); u, S, Y sparse in {−1, 0, 1}
        t = rng.choice([0.5, 1.0], n // 2)
        x = np.empty(n)
        x[0::2], x[1::2] = t, t * t
        d = dict(x=x, u=_dy(rng, n, -1, 1, 1.0) * (rng.uniform(0, 1, n) < 0.5) + 0.0, p=None)
    else:
        K = getattr(obj, "K", 1)
        p = None
        if K:
            p = np.stack([rng.integers(1, 5, n).astype(np.float64)] + [_dy(rng, n, -4, 4, 0.25) for _ in range(K - 1)])
        d = dict(x=_dy(rng, n, -8, 8, 0.25), u=_dy(rng, n, -6, 6, 0.25), p=p if K != 1 else p[0])
    if ring is not None:
        m, listed = ring
        Sr, Yr = np.full((m + 1, n), np.nan), np.full((m + 1, n), np.nan)
        for q in listed:
            if obj is Rosen:
                Sr[q] = _dy(rng, n, -1, 1, 1.0) * (rng.uniform(0, 1, n) < 0.25) + 0.0
                Yr[q] = _dy(rng, n, -1, 1, 1.0) * (rng.uniform(0, 1, n) < 0.25) + 0.0
            else:
                Sr[q], Yr[q] = _dy(rng, n, -4, 4, 0.25), _dy(rng, n, -4, 4, 0.25)
        d["S"], d["Y"] = Sr, Yr
    return d


def cg_script(obj):
    """INIT → trial (k = 1) → trial (k = 3) → accept+dir+trial (k = 3) → trial → accept+dir (k = 0) → trial: wide and narrow
    rows alternate, a lane re-reads in place what it stored.  The quartic has no exactness budget along u = −∇f after a
    step: there a_acc = β = 0 (the steps of paired Rosenbrock are exercised on random data, (e))."""
    a_acc, beta = (0.0, 0.0) if obj is Rosen else (0.5, 0.75)
    st = [0.125, 0.25, 0.375] if obj is Rosen else STEPS
    return [("init",), ("trial", st[:1]), ("trial", st), ("accept_dir_trial", a_acc, beta, st), ("trial", st[1:]),
            ("accept_dir_trial", a_acc, beta, []), ("trial", st[:2])]


TRIAL_ONLY = [("trial", STEPS[:2]), ("trial", STEPS)]


def pad3(a):
    a = list(a)
    return a + [a[-1] if a else 0.0] * (3 - len(a))


def run_cg_model(obj, d, script, exact):
    """the rows (exact: their bits; else the factor lists) and the vectors after the script, for one problem"""
    x, u, p = d["x"], d["u"], d["p"]
    rows = []
    with arith(exact):
        for item in script:
            if item[0] == "init":
                T, x, u = cg_pass(obj, x, u, p, R_INIT, [], 0.0, 0.0)
                W = 10
            elif item[0] == "trial":
                T, x, u = cg_pass(obj, x, u, p, R_TRIAL, pad3(item[1]), 0.0, 0.0)
                W = 24
            else:
                k = len(item[3])
                T, x, u = cg_pass(obj, x, u, p, R_ACCEPT | R_DIR | (R_TRIAL if k else 0), pad3(item[3]) if k else [], item[1], item[2])
                W = 24 if k else 10
            rows.append((exact_row(T, W) if exact else T, W))
    return rows, x, u


def _stack(ds, key, n):
    return None if ds[0][key] is None else np.stack([np.asarray(d[key]).reshape(-1, n) for d in ds])


def params_of(obj, ds, n):
    P = _stack(ds, "p", n)                       # [batch][K][n]
    return [] if P is None else [np.ascontiguousarray(P[:, j]) for j in range(P.shape[1])]


def padding_intact(tag, got, keys, n, mism):
    if n & 1:
        for key in keys:
            if got[key] is not None and not np.all(bits(got[key][..., n]) == NAN_BITS):
                mism.append(f"{tag}: the padding element of a row of {key} was written")


def vec_eq(tag, key, got, want, mism):
    if not np.array_equal(bits(got), bits(want)):
        i = int(np.nonzero(bits(got).ravel() != bits(want).ravel())[0][0])
        mism.append(f"{tag}: {key} differs first at flat element {i}: got {got.ravel()[i]!r}, want {np.asarray(want).ravel()[i]!r}")


def _report(mism):
    assert not mism, f"{len(mism)} mismatches, first 12:\n" + "\n".join(mism[:12])


REACHED = set()


def probe(cgo, tier, obj, kind, ds, script, n, **kw):
    X, Uv = _stack(ds, "x", n)[:, 0], _stack(ds, "u", n)[:, 0]
    got = cgo.batch_probe(tier, kind, X, Uv, script, params=params_of(obj, ds, n), **kw)
    REACHED.add(got["symbol"])
    assert got["ld"] == n + (n & 1) and got["points"] == 3
    return got


def check_cg(cgo, tier, obj, kind, n, batch, script, exact, seed0, mism, scalars=None, objs=None, gradient=False):
    ds = [exact_problem(obj, n, seed0 + 17 * b) if exact else float_problem(obj, n, seed0 + 17 * b) for b in range(batch)]
    got = probe(cgo, tier, obj, kind, ds, script, n, scalars=scalars, gradient=gradient)
    tag0 = f"{tier} {getattr(obj, 'name', obj)} n={n} batch={batch}"
    rows = got["rows"].view(np.int64)
    for b, d in enumerate(ds):
        ob = objs[b] if objs else obj
        want, x, u = run_cg_model(ob, d, script, exact)
        for q, (w, W) in enumerate(want):
            tag = f"{tag0} problem {b} pass {q} {script[q][0]} [{got['symbol']}]"
            assert got["width"][q, b] == W, tag
            if exact:
                if not np.array_equal(rows[q, b], w):
                    s = int(np.nonzero(rows[q, b] != w)[0][0])
                    mism.append(f"{tag}: slot {s} {rows[q, b, s:s + 1].view(np.float64)[0]!r} vs {w[s:s + 1].view(np.float64)[0]!r}")
            else:
                check_row_bound(tag, rows[q, b], w, W, n, mism)
            if script[q][0] != "init" and W == 24:   # what the member function returned = the row's points
                if not np.array_equal(bits(got["ts"][q, b, :3].ravel()), rows[q, b, :21]):
                    mism.append(f"{tag}: the returned TrialSums are not the row's")
        writes = any(it[0] == "accept_dir_trial" for it in script)
        assert got["done"][b] == sum(it[0] == "accept_dir_trial" for it in script) and got["passes"][b] == len(script)
        if tier == "lds" and not writes:            # no completed iteration: k_batch writes nothing back
            x, u = d["x"], d["u"]
        vec_eq(f"{tag0} problem {b}", "x", got["x"][b, :n], x, mism)
        vec_eq(f"{tag0} problem {b}", "u", got["u"][b, :n], u, mism)
        if gradient:
            with arith(exact):
                g = grad(ob, x, d["p"])
            vec_eq(f"{tag0} problem {b}", "g", got["g"][b, :n], g, mism)
    padding_intact(tag0, got, ("x", "u") + (("g",) if gradient and scalars is not None else ()), n, mism)
    return got, ds


def float_problem(obj, n, seed):
    kind = "rosen" if obj is Rosen else "quad"
    data, scal, su, sg = random_data(kind, n, seed)
    return dict(x=data["x"], u=data["u"], p=data["p"], scal=scal, su=su, sg=sg)


# ---- CPU tier: the data are what the GPU tier assumes -----------------------------------------------------------------------
def lbfgs_cases():
    """(m, count, free slot): wrapped slot lists whose slots differ from their positions, a free slot no entry names"""
    return [(1, 0, 0), (1, 1, 1), (4, 1, 0), (4, 3, 1), (10, 0, 5), (10, 3, 1), (10, 9, 4), (10, 10, 7)]


def test_lbfgs_cases_cover_the_counts_and_wrap():
    assert {c for _, c, _ in lbfgs_cases()} == {0, 1, 3, 9, 10} and {m for m, _, _ in lbfgs_cases()} == {1, 4, 10}
    for m, c, free in lbfgs_cases():
        lst = slot_list(c, m + 1, free)
        assert free not in lst and len(set(lst)) == c and all(0 <= q <= m for q in lst)
        if c > 1:
            assert any(q != j for j, q in enumerate(lst)) and (c < 3 or lst != sorted(lst, reverse=True) or free > 0)


def lbfgs_problem(obj, n, m, c, free, seed):
    lst = slot_list(c, m + 1, free)
    d = exact_problem(obj, n, seed, ring=(m, lst))
    d["q"] = qn_state(m, lst, free, np.random.default_rng(seed + 5))
    d["lst"] = lst
    return d


PUSH_A = 0.5


def coefs(obj, c):
    if obj is Rosen:
        return 1.0, [0.5 * (-1) ** j for j in range(c)], [-0.5 * (-1) ** j for j in range(c)]
    return 0.5, [0.125 * (j + 1) for j in range(c)], [-0.25 * (1 + (j % 3)) for j in range(c)]


def test_exact_data_meet_their_preconditions():
    """CPU tier: every product and element-wise sum of the exact cases is exact and every slot order-independent (M, A, S and
    exact_sum assert it) — at the largest and the smallest shapes of each tier, for every objective and script."""
    for tier in ("lds", "device"):
        ns = sizes(tier)
        for obj in (Quad, Rosen, Booth, UserQ4(), UserSM(0.75), UserQ0):
            for n in ([2] if obj is Booth else [n for n in (ns[-1], ns[-2], 3, 1, 10056, 10055) if not (obj is Rosen and n & 1)]):
                d = exact_problem(obj, n, 100 + n)
                for script in (cg_script(obj), TRIAL_ONLY):
                    run_cg_model(obj, d, script, True)
    ns = sizes("lbfgs")
    for obj in (Quad, Rosen):
        for m, c, free in lbfgs_cases():
            for n in (ns[-1], ns[-2], 3, 1):
                if obj is Rosen and n & 1:
                    continue
                d = lbfgs_problem(obj, n, m, c, free, 300 + n)
                with arith(True):
                    T, xp, S2, Y2 = push_pass(obj, d["x"], d["u"], d["p"], d["S"], d["Y"], d["lst"], free, PUSH_A)
                    exact_row(T, ROW)
                    gam, cy, cs = coefs(obj, c)
                    T, u = combine_pass(obj, d["x"], d["p"], d["S"], d["Y"], d["lst"], gam, cy, cs, pad3([0.25] if obj is Rosen else STEPS))
                    exact_row(T, 24)


def test_sjyn_and_yjsn_differ_on_paired_rosenbrock():
    """(c) CPU tier: on the exact paired-Rosenbrock pushes the slots s_j·y and y_j·s hold different values for every stored
    pair — a kernel that swaps them cannot pass."""
    for m, c, free in lbfgs_cases():
        if c == 0:
            continue
        for n in (2 * BLOCK, sizes("lbfgs")[-1] & ~1):
            d = lbfgs_problem(Rosen, n, m, c, free, 300 + n)
            with arith(True):
                T, *_ = push_pass(Rosen, d["x"], d["u"], None, d["S"], d["Y"], d["lst"], free, PUSH_A)
                row = exact_row(T, ROW).view(np.float64)
            for j in range(c):
                b = QS_PAIR0 + QP_PER_PAIR * j
                assert row[b + SJYN] != row[b + YJSN], (m, c, n, j)


def drop_problem(obj, n, m, c, free, seed):
    """(b) s·y < 0 exactly.  The quadratic: D with negative entries that outweigh the positive ones.  Paired Rosenbrock: pairs
    (0, w), w ∈ {1, 2}, u = (±1, 0), a = 1/2 — the Hessian's (1, 1) entry 1200·xe² − 400·w + 2 is negative along the whole step."""
    d = lbfgs_problem(obj, n, m, c, free, seed)
    rng = np.random.default_rng(seed + 9)
    if obj is Rosen:
        d["x"][0::2], d["x"][1::2] = 0.0, rng.choice([1.0, 2.0], n // 2)
        d["u"][0::2], d["u"][1::2] = rng.choice([-1.0, 1.0], n // 2), 0.0
    else:
        d["p"] = np.where(rng.uniform(0, 1, n) < 0.75, -4.0, 1.0)
        d["u"] = _dy(rng, n, 1, 6, 0.25) * rng.choice([-1.0, 1.0], n)
    return d


# the combine after the drop: the quartic has moved to a point of large ∇f — no exactness budget for a trial step there (k = 0)
DROP_SIZES = {Rosen: (2 * BLOCK, 2 * (U["lbfgs"] * BLOCK + 1)), Quad: (3, 2 * BLOCK + 1, 2 * (U["lbfgs"] * BLOCK + 1) + 1)}
DROP_TRIAL = {Quad: STEPS, Rosen: []}


def test_the_drop_happens_exactly_where_planned(simq):
    """(b) CPU tier: the model's exact row of the drop cases has s·y < 0, the host's qn_update returns "dropped" on it, keeps
    count, list, free slot, γ, ρ and the Gram blocks and changes only sg / yg of the stored pairs."""
    for obj in (Quad, Rosen):
        for m, c, free, n in [(m, c, free, n) for m, c, free in ((4, 3, 1), (10, 9, 4), (1, 1, 1)) for n in DROP_SIZES[obj]]:
            d = drop_problem(obj, n, m, c, free, 700)
            with arith(True):
                T, xp, S2, Y2 = push_pass(obj, d["x"], d["u"], d["p"], d["S"], d["Y"], d["lst"], free, PUSH_A)
                row = exact_row(T, ROW)
                gam, cy, cs = coefs(obj, c)        # … and the combine and the zero-step push that follow on the device are exact too
                T2, u2 = combine_pass(obj, xp, d["p"], S2, Y2, d["lst"], gam, cy, cs, pad3(DROP_TRIAL[obj]))
                exact_row(T2, 24)
                exact_row(push_pass(obj, xp, u2, d["p"], S2, Y2, d["lst"], free, 0.0)[0], ROW)
            assert row.view(np.float64)[0] < 0.0
            q2, co, kept = host_update(simq, d["q"], row)
            assert not kept and q2["count"] == c and q2["free_slot"] == free and list(q2["list"]) == list(d["q"]["list"])
            for name in ("gamma", "rho", "SY", "YY"):
                assert np.array_equal(bits(q2[name]), bits(d["q"][name])), name
            changed = np.nonzero(bits(q2["sg"]) != bits(d["q"]["sg"]))[0]
            assert set(changed) <= set(d["lst"]) and len(changed) > 0
            if obj is Rosen:
                for j in range(c):
                    b = QS_PAIR0 + QP_PER_PAIR * j
                    assert row[b + SJYN] != row[b + YJSN]


def probe_cases():
    """(tier, objective template name) of every case of this file: what test_coverage_* holds against the table"""
    out = set()
    for tier in ("lds", "device", "lbfgs"):
        for name in ("ObjQuadDiag", "ObjRosenPaired", "ObjBooth"):
            out.add((tier, name))
    out |= {("lds", "UserObjective"), ("device", "UserObjective")}
    return out


def expected_instantiations():
    want = set()
    for tier, fam in TIER_FAMILY.items():
        for (npts,) in I.rows(fam):
            for _, tname in I.rows("OBJ"):
                want.add(f"{TIER_KERNEL[tier]}<{tname}, {npts}, true>")
    for tier in ("lds", "device"):
        for (npts,) in I.rows(TIER_FAMILY[tier]):
            want.add(f"{TIER_KERNEL[tier]}<UserObjective, {npts}, true>")
    return want


def test_dispatch_tables_have_tests():
    """(h) CPU tier: every row of the three batch lists × CGO_OBJ_ROWS (and the user module's two kernels) has a probe case
    here, and no launch or address-taking of a batch kernel sits outside a `#define ROW(` expander of the table."""
    cases = probe_cases()
    for sym in expected_instantiations():
        kern, tname = re.match(r"(\w+)<(\w+), 3, true>", sym).groups()
        tier = {v: k for k, v in TIER_KERNEL.items()}[kern]
        assert (tier, tname) in cases, sym
    assert len(expected_instantiations()) == 11
    assert I.stray_uses() == []
    probe_tu = open(os.path.join(I.CSRC, "cgo_backend_batch_probe.hip")).read()
    for fam in TIER_FAMILY.values():
        assert f"CGO_{fam}_ROWS(ROW)" in probe_tu
    for tu in ("cgo_backend_batch.hip", "cgo_backend_batch_rows.hip", "cgo_backend_batch_lbfgs.hip"):   # the product units do not see the twins
        assert ", true>" not in open(os.path.join(I.CSRC, tu)).read()


def test_the_entry_point_is_declared_host_only_and_refuses_without_a_device(cgo):
    """CPU tier: cgo_batch_probe is declared between the CGO_HOST_ONLY markers (the text of the run-time compiled modules stays
    what it was), has its ctypes twin, and its argument checks need no device."""
    from cgo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cgo.h")).read()
    host_only = hdr[hdr.index("/* CGO_HOST_ONLY_BEGIN"):hdr.index("/* CGO_HOST_ONLY_END */")]
    assert "int cgo_batch_probe(cgo_ctx *ctx, cgo_batch_probe_args *p);" in host_only and "int64_t cgo_batch_probe_qn_bytes(void);" in host_only
    assert hdr.count("cgo_batch_probe_args;") == 1 and "#define CGO_BATCH_PROBE_MAX_PASSES 32" in host_only
    assert len(_lib.SIGNATURES["cgo_batch_probe"][1]) == 2 and _lib.SIGNATURES["cgo_batch_probe_qn_bytes"][0] is C.c_int64
    L = cgo.lib()
    assert L.cgo_batch_probe_qn_bytes() == QN.itemsize
    assert L.cgo_batch_probe(None, None) == 1 and "null argument" in L.cgo_last_error().decode()
    assert C.sizeof(_lib.BatchPassC) == 8 * (1 + 7 + 2 + 1 + 1 + 20) and C.sizeof(_lib.BatchPassOutC) == 8 * 53
    with pytest.raises(ValueError, match="tier must be"):
        cgo.batch_probe("hbm", "quad_diag", np.ones((1, 4)), np.ones((1, 4)), [("init",)])
    with pytest.raises(ValueError, match="no pass kind"):
        cgo.batch_probe("lds", "quad_diag", np.ones((1, 4)), np.ones((1, 4)), [("reset",)], params=[np.ones((1, 4))])
    mk = open(os.path.join(I.CSRC, "Makefile")).read()
    assert "cgo_backend_batch_probe.hip" in mk
    # a program of its own: exactly the twins of tiers 0 and 1, and no product program lists a twin
    assert I.rtc_program_kernels("RTC_BATCH_PROBE") == ["k_batch<UserObjective, 3, true>", "k_batch_rows<UserObjective, 3, true>"]
    for prog in ("RTC_BATCH", "RTC_BATCH_ROWS", "RTC_BATCH_LBFGS", "RTC_BATCH_LBFGS_LDS"):
        assert not [k for k in I.rtc_program_kernels(prog) if ", true>" in k], prog
    assert "k_batch" not in open(os.path.join(I.CSRC, "cgo_rtc.hip")).read()


# ---- GPU tier ----------------------------------------------------------------------------------------------------------------
KIND = {Quad: "quad_diag", Rosen: "rosenbrock_paired", Booth: "booth"}


@pytest.fixture(scope="module")
def models(cgo, gpu_ctx):
    """the run-time compiled objectives, one module each, compiled once per test module"""
    made = {}

    def get(cls, n):
        key = (cls.name, n)
        if key not in made:
            made[key] = cgo.ElementwiseObjective(n, cls.SOURCE, param=[None] * cls.K, ctx=gpu_ctx)
        return made[key]
    yield get
    for o in made.values():
        o.close()


@pytest.mark.gpu
def test_geometry_is_the_librarys(cgo):
    assert cgo.batch_lbfgs_shape() == (BLOCK, U["lbfgs"]) and cgo.batch_rows_shape() == (BLOCK, U["device"])
    assert cgo.batch_probe_qn_words() * 8 == QN.itemsize and cgo.batch_lbfgs_max_m() == QN_MAX_M


@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["lds", "device"])
def test_cg_tiers_exact_every_slot(cgo, gpu_ctx, tier):
    """(a) tiers 0 and 1: the seven-pass script and the trial-only script at every shape, batches of 1 and 3."""
    mism = []
    for obj in (Quad, Rosen, Booth):
        ns = [2] if obj is Booth else [n for n in sizes(tier) if not (obj is Rosen and n & 1)]
        for n in ns:
            for batch in (1, 3):
                check_cg(cgo, tier, obj, KIND[obj], n, batch, cg_script(obj), True, 1000 + n, mism, gradient=True)
                check_cg(cgo, tier, obj, KIND[obj], n, batch, TRIAL_ONLY, True, 2000 + n, mism)
    _report(mism)


@pytest.mark.gpu
def test_lds_tier_at_the_largest_problem_it_holds(cgo, gpu_ctx, models):
    """(a) cgo_batch_max_n and one less, for an objective without a slot and one with one slot"""
    mism = []
    top1 = cgo.batch_max_n("quad_diag")
    for n in (top1, top1 - 1):
        check_cg(cgo, "lds", Quad, "quad_diag", n, 3, cg_script(Quad), True, 3000 + n, mism)
    n0 = cgo.batch_max_n(models(UserQ0, 16))      # (the limit is the module's, whatever the model's size)
    assert n0 > top1 and n0 % 2 == 0
    check_cg(cgo, "lds", Rosen, "rosenbrock_paired", cgo.batch_max_n("rosenbrock_paired"), 3, cg_script(Rosen), True, 3100, mism)
    for n in (n0, n0 - 1):
        check_cg(cgo, "lds", UserQ0, models(UserQ0, n), n, 3, cg_script(UserQ0), True, 3200 + n, mism)
    with pytest.raises(cgo.CgoError) as e:
        check_cg(cgo, "lds", Quad, "quad_diag", top1 + 1, 1, TRIAL_ONLY, True, 1, mism)
    assert e.value.code == 1 and "cgo_batch_max_n" in e.value.msg
    _report(mism)


@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["lds", "device"])
def test_more_workgroups_than_compute_units(cgo, gpu_ctx, tier):
    """(a) 300 problems of n = 5, every row checked"""
    mism = []
    check_cg(cgo, tier, Quad, "quad_diag", 5, 300, cg_script(Quad), True, 4000, mism, gradient=True)
    _report(mism)


@pytest.mark.gpu
@pytest.mark.parametrize("tier", ["lds", "device"])
def test_scalars_per_problem_and_parameter_slots(cgo, gpu_ctx, models, tier):
    """(d) a body that reads s0 (a different dyadic scalar per problem, three slots) and one with four slots, a different row
    per slot and problem; the results' gradient with scalars is k_batch_grad's, which must leave the padding alone (g)."""
    mism = []
    for n in (3, 2 * BLOCK + 1, 2 * (U[tier] * BLOCK + 1), sizes(tier)[-1]):
        sc = np.array([0.75, 1.5, 0.5])
        check_cg(cgo, tier, UserSM(1.0), models(UserSM, n), n, 3, cg_script(Quad), True, 5000 + n, mism, scalars=sc,
                 objs=[UserSM(s) for s in sc], gradient=True)
        check_cg(cgo, tier, UserQ4(), models(UserQ4, n), n, 3, cg_script(Quad), True, 5100 + n, mism, gradient=True)
    _report(mism)


def random_sizes(kind):
    return (2 * BLOCK + (kind == "quad"), 2 * (U["device"] * BLOCK + 1) + (kind == "quad"), sizes("device")[-1] - (kind != "quad"))


def random_script(kind, d0):
    """problem 0's steps for the whole batch (the script is the launch's)"""
    (a_acc, beta), su, sg = d0["scal"], d0["su"][:3], d0["sg"][:3]
    if kind != "quad":
        a_acc = 0.0     # (random_data: along u = −∇f of the quartic the steps are the tiny ones, and x stays)
    script = [("init",), ("trial", sg[:1]), ("accept_dir_trial", a_acc, beta, sg), ("trial", sg[:2]), ("accept_dir_trial", a_acc, beta, []),
              ("trial", sg)]
    return ([("trial", su)] if kind == "quad" else []) + script


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["quad", "rosen"])
def test_random_data_tiers_agree_and_meet_the_bound(cgo, gpu_ctx, kind):
    """(e) random data (terms bounded away from zero): (i) the LDS tier's rows are bitwise the device-rows tier's, all W slots
    of every pass; (ii) every slot within γ_d·Σ|t| of the correctly rounded exact sum of the device-order terms; (iii) the
    vectors bitwise the plain IEEE model's."""
    mism = []
    obj = Quad if kind == "quad" else Rosen
    for n in random_sizes(kind):
        script = random_script(kind, float_problem(obj, n, 6000 + n))
        got = {}
        for tier in ("lds", "device"):
            got[tier], _ = check_cg(cgo, tier, obj, KIND[obj], n, 3, script, False, 6000 + n, mism)
        if not np.array_equal(got["lds"]["rows"], got["device"]["rows"]):
            q, b, s = [int(v[0]) for v in np.nonzero(got["lds"]["rows"] != got["device"]["rows"])]
            mism.append(f"{kind} n={n}: the tiers' rows differ first at pass {q}, problem {b}, slot {s}")
        for key in ("x", "u"):
            vec_eq(f"{kind} n={n} LDS vs device rows", key, got["lds"][key], got["device"][key], mism)
    _report(mism)


def _lbfgs_inputs(ds, n, m):
    return dict(m=m, S=np.stack([d["S"] for d in ds]), Y=np.stack([d["Y"] for d in ds]), qn=words(np.array([d["q"] for d in ds], dtype=QN)))


def check_push(tag, got, q, b, d, a, obj, simq, exact, n, mism, expect_kept=None):
    """after a push: the row, x = xp, the free slot = (s, y), the rest of the ring untouched, absent pairs and 54–63 +0.0, the
    state = the host's recursion on the device's own row.  d is updated to what the problem holds afterwards."""
    rows = got["rows"].view(np.int64)
    free, lst, c = int(d["q"]["free_slot"]), list(d["lst"]), len(d["lst"])
    with arith(exact):
        T, xp, S2, Y2 = push_pass(obj, d["x"], d["u"], d["p"], d["S"], d["Y"], lst, free, a)
        if got.get("sim"):
            rows[q, b] = sim_row(T, ROW)
            got["width"][q, b] = ROW
        if exact:
            w = exact_row(T, ROW)
            if not np.array_equal(rows[q, b], w):
                s = int(np.nonzero(rows[q, b] != w)[0][0])
                mism.append(f"{tag}: push slot {s} {rows[q, b, s:s + 1].view(np.float64)[0]!r} vs {w[s:s + 1].view(np.float64)[0]!r}")
        else:
            check_row_bound(tag, rows[q, b], T, ROW, n, mism)
    if np.any(rows[q, b, QS_PAIR0 + QP_PER_PAIR * c:] != 0):
        mism.append(f"{tag}: a slot of an absent pair (j ≥ {c}) or of 54–63 of the push row is not +0.0")
    assert got["width"][q, b] == ROW
    q2, co, kept = host_update(simq, d["q"], rows[q, b])
    if got.get("sim"):
        got["stored"][q, b] = q2["count"]
    if expect_kept is not None:
        assert kept == expect_kept, tag
    if got["stored"][q, b] != q2["count"]:
        mism.append(f"{tag}: push_update returned {got['stored'][q, b]} stored pairs, the host's recursion {q2['count']}")
    d.update(x=xp, S=S2, Y=Y2, q=q2, co=co, lst=[int(v) for v in q2["list"][:q2["count"]]], kept=kept)


def check_combine(tag, got, q, b, d, obj, coef, a, exact, n, mism):
    rows = got["rows"].view(np.int64)
    gam, cy, cs, c = coef
    with arith(exact):
        T, u = combine_pass(obj, d["x"], d["p"], d["S"], d["Y"], d["lst"][:c], gam, cy, cs, pad3(a))
        if got.get("sim"):
            rows[q, b] = sim_row(T, 24)
            got["gu"][q, b], got["uu"][q, b] = rows[q, b, 21:23].view(np.float64)
            got["stored"][q, b] = c
        if exact:
            w = exact_row(T, 24)
            if not np.array_equal(rows[q, b], w):
                s = int(np.nonzero(rows[q, b] != w)[0][0])
                mism.append(f"{tag}: combine slot {s} {rows[q, b, s:s + 1].view(np.float64)[0]!r} vs {w[s:s + 1].view(np.float64)[0]!r}")
        else:
            check_row_bound(tag, rows[q, b], T, 24, n, mism)
    if bits(got["gu"][q, b:b + 1])[0] != rows[q, b, 21] or bits(got["uu"][q, b:b + 1])[0] != rows[q, b, 22]:
        mism.append(f"{tag}: the returned g·u, u·u are not the row's")
    d["u"] = u


def final_vectors(tag, got, b, d, n, mism):
    vec_eq(tag, "x", got["x"][b, :n], d["x"], mism)
    vec_eq(tag, "u", got["u"][b, :n], d["u"], mism)
    for key in ("S", "Y"):       # every slot, absent ones (NaN rows) included: untouched means the same bits
        vec_eq(tag, key, got[key][b, :, :n], d[key], mism)
    if not np.array_equal(words(d["q"])[0], got["qn"][b]):
        i = int(np.nonzero(words(d["q"])[0] != got["qn"][b])[0][0])
        mism.append(f"{tag}: the QnState differs from the host's recursion first at word {i}")


@pytest.mark.gpu
@pytest.mark.parametrize("obj", [Quad, Rosen], ids=["quad", "rosen"])
def test_lbfgs_single_passes_exact(cgo, gpu_ctx, simq, obj):
    """(a), (c) tier 2: one push, and one combine on given coefficients, for every (m, count, free slot) of lbfgs_cases at
    every shape — wrapped slot lists, absent ring slots NaN."""
    mism = []
    ns = [n for n in sizes("lbfgs") if not (obj is Rosen and n & 1)]
    for i, n in enumerate(ns):
        cases = lbfgs_cases() if n in (ns[-1], ns[-2], ns[0], 2 * BLOCK) else lbfgs_cases()[i % 4::4]
        for m, c, free in cases:
            for batch in ((1, 3) if (m, c) == (10, 9) else (3,)):
                gam, cy, cs = coefs(obj, c)
                a_tr = [0.25] if obj is Rosen else STEPS
                ds = [lbfgs_problem(obj, n, m, c, free, 8000 + n + 31 * b) for b in range(batch)]
                got = probe(cgo, "lbfgs", obj, KIND[obj], ds, [("push", PUSH_A)], n, **_lbfgs_inputs(ds, n, m))
                for b, d in enumerate(ds):
                    tag = f"lbfgs {obj.name} n={n} m={m} c={c} free={free} problem {b} push"
                    check_push(tag, got, 0, b, d, PUSH_A, obj, simq, True, n, mism)
                    final_vectors(tag, got, b, d, n, mism)
                padding_intact(f"lbfgs {obj.name} n={n} m={m} c={c}", got, ("x", "u", "S", "Y"), n, mism)
                ds = [lbfgs_problem(obj, n, m, c, free, 8000 + n + 31 * b) for b in range(batch)]
                got = probe(cgo, "lbfgs", obj, KIND[obj], ds, [("combine", a_tr, (c, gam, cy, cs))], n, **_lbfgs_inputs(ds, n, m))
                for b, d in enumerate(ds):
                    tag = f"lbfgs {obj.name} n={n} m={m} c={c} free={free} problem {b} combine"
                    check_combine(tag, got, 0, b, d, obj, (gam, cy, cs, c), a_tr, True, n, mism)
                    final_vectors(tag, got, b, d, n, mism)
                padding_intact(f"lbfgs {obj.name} n={n} m={m} c={c}", got, ("x", "u", "S", "Y"), n, mism)
    ds = [lbfgs_problem(Booth, 2, 4, 3, 1, 8900 + b) for b in range(3)] if obj is Quad else []
    if ds:
        got = probe(cgo, "lbfgs", Booth, "booth", ds, [("push", 0.25)], 2, **_lbfgs_inputs(ds, 2, 4))
        for b, d in enumerate(ds):
            check_push(f"lbfgs booth problem {b}", got, 0, b, d, 0.25, Booth, simq, True, 2, mism)
            final_vectors(f"lbfgs booth problem {b}", got, b, d, 2, mism)
    _report(mism)


LBFGS_SCRIPT_CASES = [(4, 3, 1), (10, 9, 4), (1, 0, 0)]


def script_problems(n, m, c, free):
    ds = []
    for b in range(3):
        d = lbfgs_problem(Quad, n, m, c, free, 9000 + n + 31 * b)
        rng = np.random.default_rng(9100 + n + b)     # one sign per element, D > 0: every pair has s·y > 0 and no term near zero
        sg = rng.choice([-1.0, 1.0], n)
        d.update(x=sg * _dy(rng, n, 4, 8, 0.25), p=rng.integers(1, 3, n).astype(np.float64))
        for q in d["lst"]:
            d["S"][q], d["Y"][q] = sg * _dy(rng, n, 1, 4, 0.25), sg * _dy(rng, n, 1, 4, 0.25)
        ds.append(d)
    return ds


def check_lbfgs_script(got, ds, n, m, c, simq, mism):
    rows = got["rows"].view(np.int64)
    for b, d in enumerate(ds):
        tag0 = f"lbfgs script n={n} m={m} c={c} problem {b}"
        exact = True
        for q, item in enumerate(LBFGS_SCRIPT):
            tag = f"{tag0} pass {q} {item[0]}"
            if item[0] == "init":
                with arith(True):
                    T, d["x"], d["u"] = cg_pass(Quad, d["x"], d["u"], d["p"], R_INIT, [], 0.0, 0.0)
                    if not got.get("sim") and not np.array_equal(rows[q, b], exact_row(T, 10)):
                        mism.append(f"{tag}: the row differs")
            elif item[0] == "push":
                check_push(tag, got, q, b, d, item[1], Quad, simq, exact, n, mism, expect_kept=True)
            elif item[0] == "combine":
                exact = False
                co = d["co"]
                check_combine(tag, got, q, b, d, Quad, (float(co["gamma"]), list(co["cy"]), list(co["cs"]), int(co["count"])), item[1],
                              False, n, mism)
                assert got["stored"][q, b] == co["count"]
            else:
                with arith(False):
                    T, _, _ = cg_pass(Quad, d["x"], d["u"], d["p"], R_TRIAL, pad3(item[1]), 0.0, 0.0)
                if got.get("sim"):
                    rows[q, b] = sim_row(T, 24)
                check_row_bound(tag, rows[q, b], T, 24, n, mism)
        if not got.get("sim"):
            assert got["done"][b] == 3 and got["passes"][b] == len(LBFGS_SCRIPT)
            final_vectors(tag0, got, b, d, n, mism)
    if not got.get("sim"):
        padding_intact(f"lbfgs script n={n}", got, ("x", "u", "S", "Y"), n, mism)


def sim_got(npass, batch):
    return dict(sim=True, rows=np.full((npass, batch, ROW), NAN_BITS, dtype=np.int64).view(np.uint64), width=np.zeros((npass, batch), np.int64),
                stored=np.zeros((npass, batch), np.int64), gu=np.zeros((npass, batch)), uu=np.zeros((npass, batch)))


def test_random_and_script_data_meet_the_guard(simq):
    """CPU tier: every slot of the random-data cases (e) and of the passes of the L-BFGS script that are held to the summation
    bound has its smallest |term| above that bound — with correctly rounded sums standing in for the device's rows."""
    for m, c, free in LBFGS_SCRIPT_CASES:
        for n in (3, sizes("lbfgs")[-1]):
            mism = []
            check_lbfgs_script(sim_got(len(LBFGS_SCRIPT), 3), script_problems(n, m, c, free), n, m, c, simq, mism)
            _report(mism)
    for kind, obj in (("quad", Quad), ("rosen", Rosen)):
        for n in random_sizes(kind):
            d = float_problem(obj, n, 6000 + n)
            rows, _, _ = run_cg_model(obj, d, random_script(kind, d), False)
            for q, (T, W) in enumerate(rows):
                check_row_bound(f"{kind} n={n} pass {q}", sim_row(T, W), T, W, n, [])


LBFGS_SCRIPT = [("init",), ("push", 0.125), ("combine", STEPS), ("trial", STEPS[:2]), ("push", 0.0625), ("combine", []), ("push", 0.03125)]


@pytest.mark.gpu
@pytest.mark.parametrize("m,c,free", LBFGS_SCRIPT_CASES)
def test_lbfgs_script_in_one_launch(cgo, gpu_ctx, simq, m, c, free):
    """tier 2: INIT → push → combine (k = 3) → trial → push → combine (k = 0) → push in ONE launch, the combines on the
    coefficients the device's own push left.  Those are quotients of sums, so from the first combine on the data are no longer
    dyadic: the vectors stay bitwise (the model takes the coefficients the host's recursion makes of the device's own push
    row, which the state must equal word for word), the rows are held to the summation bound of (e); INIT and the first push
    are exact."""
    mism = []
    for n in (3, 2 * BLOCK + 1, 2 * (U["lbfgs"] * BLOCK + 1), sizes("lbfgs")[-1]):
        ds = script_problems(n, m, c, free)
        got = probe(cgo, "lbfgs", Quad, "quad_diag", ds, LBFGS_SCRIPT, n, **_lbfgs_inputs(ds, n, m))
        check_lbfgs_script(got, ds, n, m, c, simq, mism)
    _report(mism)


@pytest.mark.gpu
@pytest.mark.parametrize("obj", [Quad, Rosen], ids=["quad", "rosen"])
def test_dropped_candidate_on_the_device(cgo, gpu_ctx, simq, obj):
    """(b) push (s·y < 0: dropped) → combine → push in one launch: the first push returns the old count and leaves the rejected
    pair in the free slot; the combine gives the u of the stored pairs alone (it does not read that slot: were it read, the
    exact row would differ); the second push overwrites the same slot and nothing else of the ring."""
    mism = []
    for m, c, free in ((4, 3, 1), (10, 9, 4), (1, 1, 1)):
        for n in DROP_SIZES[obj]:
            ds = [drop_problem(obj, n, m, c, free, 700 + 31 * b) for b in range(3)]
            gam, cy, cs = coefs(obj, c)
            a_tr = DROP_TRIAL[obj]
            script = [("push", PUSH_A), ("combine", a_tr, (c, gam, cy, cs)), ("push", 0.0)]
            got = probe(cgo, "lbfgs", obj, KIND[obj], ds, script, n, **_lbfgs_inputs(ds, n, m))
            for b, d in enumerate(ds):
                tag = f"drop {obj.name} n={n} m={m} c={c} problem {b}"
                q0, lst0 = d["q"].copy(), list(d["lst"])
                check_push(tag + " push 0", got, 0, b, d, PUSH_A, obj, simq, True, n, mism, expect_kept=False)
                assert got["stored"][0, b] == c and d["lst"] == lst0 and d["q"]["free_slot"] == free
                for name in ("gamma", "rho", "SY", "YY", "list", "count"):
                    assert np.array_equal(np.asarray(d["q"][name]), np.asarray(q0[name])), (tag, name)
                check_combine(tag + " combine", got, 1, b, d, obj, (gam, cy, cs, c), a_tr, True, n, mism)
                # the second push: a zero step from the combined u — s = 0, y = 0, written over the rejected pair
                check_push(tag + " push 1", got, 2, b, d, 0.0, obj, simq, True, n, mism, expect_kept=False)
                assert np.all(d["S"][free] == 0) and np.all(d["Y"][free] == 0)
                final_vectors(tag, got, b, d, n, mism)
            padding_intact(f"drop {obj.name} n={n}", got, ("x", "u", "S", "Y"), n, mism)
    _report(mism)


@pytest.mark.gpu
def test_skipped_problems_keep_their_bits(cgo, gpu_ctx, simq):
    """(f) a skipped problem costs its workgroup a return: rows, ring, QnState and state keep their bits, its entries of the
    rows buffer still hold the NaN pattern, and the neighbours' rows are those of the same batch without the skip."""
    mism = []
    n, m, c, free = 2 * BLOCK + 1, 4, 3, 1
    for tier in ("lds", "device", "lbfgs"):
        if tier == "lbfgs":
            ds = [lbfgs_problem(Quad, n, m, c, free, 9500 + b) for b in range(3)]
            script, kw = [("push", PUSH_A), ("trial", STEPS)], _lbfgs_inputs(ds, n, m)
        else:
            ds = [exact_problem(Quad, n, 9500 + b) for b in range(3)]
            script, kw = cg_script(Quad), {}
        full = probe(cgo, tier, Quad, "quad_diag", ds, script, n, **kw)
        part = probe(cgo, tier, Quad, "quad_diag", ds, script, n, skip=[0, 1, 0], **kw)
        for b in (0, 2):
            if not np.array_equal(full["rows"][:, b], part["rows"][:, b]):
                mism.append(f"{tier}: the rows of problem {b} changed with its neighbour skipped")
            for key in ("x", "u") + (("S", "Y", "qn") if tier == "lbfgs" else ()):
                if not np.array_equal(bits(full[key][b]) if key != "qn" else full[key][b], bits(part[key][b]) if key != "qn" else part[key][b]):
                    mism.append(f"{tier}: {key} of problem {b} changed with its neighbour skipped")
        assert part["reason"][1] == RES_STOP and part["done"][1] == 0 and part["passes"][1] == 0      # as preset
        assert all(part["reason"][b] == RES_BUDGET for b in (0, 2))
        if not np.all(part["rows"][:, 1].view(np.int64) == NAN_BITS):
            mism.append(f"{tier}: the skipped problem's workgroup stored a row")
        vec_eq(f"{tier} skipped", "x", part["x"][1, :n], ds[1]["x"], mism)
        vec_eq(f"{tier} skipped", "u", part["u"][1, :n], ds[1]["u"], mism)
        if tier == "lbfgs":
            vec_eq("lbfgs skipped", "S", part["S"][1, :, :n], ds[1]["S"], mism)
            vec_eq("lbfgs skipped", "Y", part["Y"][1, :, :n], ds[1]["Y"], mism)
            assert np.array_equal(part["qn"][1], words(ds[1]["q"])[0])
        padding_intact(f"{tier} with a skip", part, ("x", "u") + (("S", "Y") if tier == "lbfgs" else ()), n, mism)
    _report(mism)


@pytest.mark.gpu
def test_refusals(cgo, gpu_ctx):
    """what the loop of a tier never issues, k beyond the instantiation's points, more than 32 passes, a combine without
    coefficients, a state that names a slot outside the ring: CGO_EINVAL, nothing launched"""
    d = [exact_problem(Quad, 8, 1)]
    dl = [lbfgs_problem(Quad, 8, 4, 3, 1, 1)]
    kw = _lbfgs_inputs(dl, 8, 4)
    bad = [("lds", d, [("push", 0.5)], {}), ("device", d, [("combine", STEPS, (0, 1.0, [], []))], {}),
           ("lbfgs", dl, [("accept_dir_trial", 0.5, 0.5, STEPS)], kw), ("lds", d, [("trial", [0.1, 0.2, 0.3, 0.4])], {}),
           ("device", d, [("trial", [])], {}), ("lbfgs", dl, [("combine", STEPS)], kw), ("lbfgs", dl, [("combine", STEPS, (5, 1.0, [0.0] * 5, [0.0] * 5))], kw)]
    for tier, ds, script, k2 in bad:
        with pytest.raises(cgo.CgoError) as e:
            probe(cgo, tier, Quad, "quad_diag", ds, script, 8, **k2)
        assert e.value.code == 1, (tier, script, e.value.msg)
    with pytest.raises(ValueError):
        probe(cgo, "lds", Quad, "quad_diag", d, [("trial", STEPS)] * 33, 8)
    for field, v in (("free_slot", 5), ("count", 5), ("m", 3)):
        q = dl[0]["q"].copy()
        q[field] = v
        kw2 = dict(kw, qn=words(np.array([q], dtype=QN)))
        with pytest.raises(cgo.CgoError) as e:
            probe(cgo, "lbfgs", Quad, "quad_diag", dl, [("push", 0.5)], 8, **kw2)
        assert e.value.code == 1 and "outside the ring" in e.value.msg
    q = dl[0]["q"].copy()
    q["list"][7] = 9       # (an entry the count does not reach is checked all the same)
    with pytest.raises(cgo.CgoError):
        probe(cgo, "lbfgs", Quad, "quad_diag", dl, [("push", 0.5)], 8, **dict(kw, qn=words(np.array([q], dtype=QN))))


@pytest.mark.gpu
def test_coverage_of_every_instantiation(cgo):
    """(h) runs last in this file: every instantiation of the table was launched and checked above"""
    missing = expected_instantiations() - REACHED
    assert not missing, f"never launched: {sorted(missing)}"
    assert REACHED <= expected_instantiations(), sorted(REACHED - expected_instantiations())
