"""Every sum slot of every pass of the resident solver, in EVERY workgroup (cgo_solver_probe_resident).

The trajectory suites (tests/test_resident.py) see the device side of k_resident / k_resident_chain only through the numbers
the line search happens to read, to 1e-10, and only through workgroup 0.  Here a scripted sequence of passes runs in ONE launch
of the product kernel's PROBE instantiation — the engine's own plan, exchange buffers, write-back rule and round counter — and
after every pass every workgroup stores the whole row of totals it holds:

(a) exact dyadic data (the periods of tests/test_kernel_sums.py: every product exact, Σ|t| < 2⁵³ quanta per slot, so that every
    summation order gives the same bits): the row of every workgroup equals the exact row bit for bit — all W slots, padded
    points equal to the point they repeat, padding slots +0.0, the 56 − W doubles behind a narrow row untouched — what the
    member functions returned in workgroup 0 is that row, and x, u after the launch are the model's.  Trial passes leave the
    state alone, so a launch is any number of them and ONE accepting pass; launches follow one another on the same solver, so
    that narrow rows land in buffers that carried wide ones and the round counter crosses launches;
(b) random data (terms bounded away from zero): (i) all workgroups' rows bitwise equal to workgroup 0's — the invariant the
    whole replicated-control-flow design rests on, which exact data cannot test; (ii) each slot within γ_d·Σ|t| of the
    correctly rounded exact sum, d from the resident summation tree; vectors bitwise equal to the plain IEEE model's — with
    several accepting passes in a row, mixed widths in one launch;
(c) every dispatchable k_resident* instantiation (the rows of csrc/cgo_instances.def, on the CPU tier) was probed.
"""
import os
import re
from collections import defaultdict

import numpy as np
import pytest

import _instances as I
from test_kernel_sums import (rosen_valley_period, CHAIN_SCAL, CHAIN_STEPS, CHECK_EXACT, NAN_BITS, R_ACCEPT, R_DIR, R_TRIAL, RS, STEPS, Booth, Data,
                              Quad, Rosen, User, _chain_x, _make_objective, _slot_refs, bits, expected_cg, expected_chain,
                              float_cg, launch_inputs, random_data)

CSRC = I.CSRC
ACC, ACC_T = R_ACCEPT | R_DIR, R_ACCEPT | R_DIR | R_TRIAL


# ---- the plan, from the sources ------------------------------------------------------------------------------------------
def _const(text, name):
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", text)
    assert m, name
    return m.group(1).strip()


def _constants():
    res = open(os.path.join(CSRC, "cgo_kernels_resident.hip.hpp")).read()
    cg = open(os.path.join(CSRC, "cgo_kernels_cg.hip.hpp")).read()
    ker = open(os.path.join(CSRC, "cgo_kernels.hip.hpp")).read()
    be = open(os.path.join(CSRC, "cgo_backend_cg.hip")).read()
    c = dict(GSIZE=int(_const(res, "RES_GSIZE")), GROUPS=int(_const(res, "RES_GROUPS")), XBUFS=int(_const(res, "RES_XBUFS")),
             NR7=int(_const(cg, "NR7")), MAXP=int(_const(cg, "MAXP")))
    assert _const(res, "RES_WMAX") == "NR7"
    m = re.search(r"constexpr\s+int\s+BLOCK\s*=\s*(\d+)", ker + cg)
    c["BLOCK"] = int(m.group(1))
    m = re.search(r"pol_\.resident_chunk >= 2 \? \(int64_t\)\(pol_\.resident_chunk & ~1\) : \(int64_t\)(\d+)", be)
    c["CHUNK"] = int(m.group(1))
    assert "const int64_t avail = (int64_t)max_lds - static_lds - 512;" in be
    assert "chunk = (((n + cus - 1) / cus) + 1) & ~1LL;" in be and "int64_t chunk_max = (avail / (8 * vecs)) & ~1LL;" in be
    return c


K = _constants()
BLOCK, GSIZE, WMAX = K["BLOCK"], K["GSIZE"], K["NR7"]
CUS = K["GSIZE"] * K["GROUPS"]              # the MI355X has 256 CUs = the most the two-level exchange holds
MAX_LDS = 160 * 1024                       # LDS per workgroup on gfx950
# static LDS of the instantiations (tot, fs, s_out, the workgroup reduction's rows), as the compiler reports it for gfx950; it
# only enters the largest size that fits — the GPU test asserts the plan it predicts, so a stale figure fails loudly
STATIC_LDS = {1: 3712, 3: 4480, 7: 6272}
STATIC_LDS_CHAIN = {1: 1408, 3: 2176}


def row_width(np_):
    return {1: 10, 3: 24, 7: 56}[np_]


def chunk_max(vecs, static_lds):
    return ((MAX_LDS - static_lds - 512) // (8 * vecs)) & ~1


def plan(n, policy_chunk, vecs, static_lds):
    """res_plan (cgo_backend_cg.hip) for an element-wise objective: (grid, chunk) or None where it does not fit."""
    want = (policy_chunk & ~1) if policy_chunk and policy_chunk >= 2 else K["CHUNK"]
    cm = chunk_max(vecs, static_lds)
    if cm < 2:
        return None
    chunk = min(want, cm)
    grid = -(-n // chunk)
    if grid > CUS:
        chunk = ((-(-n // CUS)) + 1) & ~1
        if chunk > cm:
            return None
        grid = -(-n // chunk)
    return grid, chunk


def plan_chain(n, npts):
    chunk = n + (n & 1)
    return (1, chunk) if chunk <= chunk_max(4, STATIC_LDS_CHAIN[npts]) else None


def last_chunk(n, grid, chunk):
    return n - (grid - 1) * chunk


# ---- sizes: (policy chunk, n) -> the edge it hits --------------------------------------------------------------------------
CHUNKS = (2, 8, 512, 1024, 4096)


def _sizes():
    s = {}
    for n in (1, 2, 3):
        s[(None, n)] = "one workgroup; n = 1: no pair at all, only the odd tail element; n = 3: one pair and the odd element"
    for c in CHUNKS:
        s[(c, c - 1)] = "one workgroup, one element short of its chunk (odd tail element)"
        s[(c, c)] = "one workgroup, chunk exactly full: no exchange"
        s[(c, c + 1)] = "two workgroups, the last holds ONE element (npairs == 0, odd)"
        s[(c, c + 2)] = "two workgroups, the last holds one pair"
        s[(c, 16 * c - 1)] = "16 workgroups = one full group, the last one element short"
        s[(c, 16 * c)] = "16 workgroups = exactly one group of the two-hop exchange"
        s[(c, 16 * c + 1)] = "17 workgroups: a second group of ONE workgroup holding one element"
        s[(c, 17 * c + 1)] = "18 workgroups: a second group of two"
        s[(c, 255 * c + 1)] = "256 workgroups = 16 full groups, the last holds one element"
        s[(c, 256 * c)] = "256 workgroups, every chunk full"
        s[(c, 256 * c + 2)] = "chunk growth: more than 256 chunks of the policy's size, chunk = ⌈n/256⌉ rounded up to even (n even)"
        s[(c, 256 * c + 3)] = "chunk growth, n odd"
    for pairs in (255, 256, 257, 511, 512, 513):
        c = 2 * pairs
        s[(c, 2 * c + 2)] = f"chunks of {pairs} pairs: the two-pair trip and its one-pair remainder around one / two lanes' worth; last workgroup one pair"
        s[(c, 2 * c + 1)] = f"chunks of {pairs} pairs; last workgroup one element"
    s[(None, 1000000)] = "default policy, BASELINE config 2: 245 workgroups = 15 groups + 5"
    return s


SIZES = _sizes()


def test_sizes_hit_the_edges_they_claim():
    """CPU tier: the size table's claims follow from the constants parsed out of the sources — all but one: the static LDS of
    the instantiations (STATIC_LDS, STATIC_LDS_CHAIN) is the compiler's figure for gfx950, typed in above.  It enters only
    chunk_max, i.e. the largest sizes that fit (test_largest_sizes); the GPU tests assert the plan of every launch against
    this model, so a figure that has drifted fails there."""
    assert (BLOCK, GSIZE, K["GROUPS"], K["XBUFS"], WMAX, K["CHUNK"]) == (256, 16, 16, 4, 56, 4096)
    sl = STATIC_LDS[3]
    for c in CHUNKS:
        for vecs in (2, 3):
            P = lambda n: plan(n, c, vecs, sl)
            assert P(c - 1) == (1, c) and P(c) == (1, c)
            g, ch = P(c + 1)
            assert (g, ch) == (2, c) and last_chunk(c + 1, g, ch) == 1
            assert last_chunk(c + 2, *P(c + 2)) == 2
            assert P(16 * c - 1) == (16, c) and P(16 * c) == (16, c)
            assert P(16 * c + 1) == (17, c) and last_chunk(16 * c + 1, 17, c) == 1 and 17 - GSIZE == 1
            assert P(17 * c + 1) == (18, c)
            assert P(255 * c + 1) == (256, c) and last_chunk(255 * c + 1, 256, c) == 1
            assert P(256 * c) == (256, c)
            for n in (256 * c + 2, 256 * c + 3):
                g, ch = P(n)
                assert ch == c + 2 and ch % 2 == 0 and g <= 256 and g * ch >= n > (g - 1) * ch
    for pairs in (255, 256, 257, 511, 512, 513):
        c = 2 * pairs
        assert plan(2 * c + 2, c, 3, sl) == (3, c) and plan(2 * c + 1, c, 3, sl) == (3, c)
        # lane `tid` of a full chunk takes pairs tid, tid + 256 (one trip), …: 255 / 256 pairs: remainder only; 257: one lane
        # makes a trip; 511 / 512: (almost) every lane one trip and no remainder; 513: lane 0 a trip AND a remainder
        def lane(tid):   # ResDev::pass on a full chunk: (two-pair trips, one-pair remainder) of lane tid
            i, trips = tid, 0
            while i + BLOCK < pairs:
                trips, i = trips + 1, i + 2 * BLOCK
            return trips, i < pairs
        L = [lane(t) for t in range(BLOCK)]
        want = {255: [(0, True)] * 255 + [(0, False)],                # no trip; lane 255 has nothing at all
                256: [(0, True)] * 256,                               # every lane the remainder only
                257: [(1, False)] + [(0, True)] * 255,                # lane 0 alone makes a trip
                511: [(1, False)] * 255 + [(0, True)],                # lane 255 alone is left without a trip
                512: [(1, False)] * 256,                              # every lane one trip, no remainder
                513: [(1, True)] + [(1, False)] * 255}[pairs]         # lane 0 a trip AND a remainder
        assert L == want, pairs
        assert sum(2 * t + r for t, r in L) == pairs
    g, ch = plan(1000000, None, 3, sl)
    assert (g, ch) == (245, 4096) and divmod(g, GSIZE) == (15, 5)
    for key in SIZES:
        assert plan(key[1], key[0], 3, sl) is not None and plan(key[1], key[0], 2, sl) is not None, key


def largest(vecs, npts):
    return CUS * chunk_max(vecs, STATIC_LDS[npts])


def test_largest_sizes():
    for vecs in (2, 3):
        for npts in (1, 3, 7):
            n = largest(vecs, npts)
            assert plan(n, None, vecs, STATIC_LDS[npts]) == (256, chunk_max(vecs, STATIC_LDS[npts]))
            assert plan(n + 1, None, vecs, STATIC_LDS[npts]) is None
    assert largest(3, 3) > 1600000          # "up to n ≈ 1.6e6" with a parameter vector
    for npts in (1, 3):
        cm = chunk_max(4, STATIC_LDS_CHAIN[npts])
        assert plan_chain(cm, npts) == (1, cm) and plan_chain(cm - 1, npts) == (1, cm) and plan_chain(cm + 1, npts) is None


ROSEN_GENERAL_MAX = 1 << 19
CHAIN_SIZES = [2, 3, 4, 5, 6, 7, 510, 511, 512, 513, 514, 1000, 1001]


# ---- scripts ---------------------------------------------------------------------------------------------------------------
def launches_for(npts):
    """The launches of (a) on one solver, in order: (trial ks, accept k or None).  Every (kind, k) the kernel can run: trial
    k = 1 … min(npts, 3), accept_dir_trial k = 0 … npts.  The order of the accepting passes puts a narrow row (k = 0: 10
    slots) two rounds after a wide one (k = npts) and a wide one two rounds after that — the slot a workgroup clears two
    rounds ahead of a NARROW round is read by a WIDE one — and a narrow row into the buffer that carried wide rows two and
    four rounds earlier; pass counts 2, 2, 2, 2, 3, 4, 3, …: the round counter carried between launches is not a multiple of
    the four buffers."""
    nt = min(npts, 3)
    order = {7: [7, 7, 0, 7, 0, 3, 5, 0, 1, 2, 4, 6], 3: [3, 3, 0, 3, 0, 2, 1, 0], 1: [1, 1, 0, 1, 0]}[npts]
    ntrial = [1, 1, 1, 1, 2, 3, 2, 1, 2, 3, 1, 2]
    out, t = [], 0
    for j, ka in enumerate(order):
        ks = []
        for _ in range(ntrial[j]):
            ks.append(1 + t % nt)
            t += 1
        out.append((ks, ka))
    out.append(([1 + q % nt for q in range(3)], None))   # trials only: nothing is written back, no swap
    return out


def test_scripts_cover_every_pass_and_mix_the_widths():
    for npts in (1, 3, 7):
        L = launches_for(npts)
        nt = min(npts, 3)
        assert {k for ks, _ in L for k in ks} == set(range(1, nt + 1))
        assert {ka for _, ka in L if ka is not None} == set(range(0, npts + 1))
        widths = []
        for ks, ka in L:
            widths += [row_width(nt)] * len(ks)
            if ka is not None:
                widths.append(10 if ka == 0 else row_width(npts))
        assert len(widths) >= 9
        counts = [len(ks) + (ka is not None) for ks, ka in L]
        assert sum(1 for c in counts if c % 4) >= 2 and any(sum(counts[:j]) % 4 for j in range(1, len(counts)))
        if npts > 1:
            wide = row_width(npts)
            assert any(widths[r] == 10 and widths[r - 2] == wide and widths[r - 4] == wide for r in range(4, len(widths)))
            assert any(widths[r] == wide and widths[r - 2] == 10 and widths[r - 4] == wide for r in range(4, len(widths)))


def pad(a, m):
    a = list(a)
    return a + [a[-1]] * (m - len(a)) if a else []


def expected_pass(obj, d, npts, kind, k, a_acc, beta):
    """(row, vectors or None) of one resident pass on Data d — the k_cg model of tests/test_kernel_sums.py with the resident
    widths: a trial runs min(npts, 3) points, an accepting pass npts (k = 0: one point's layout, no trial)."""
    st = STEPS[obj.name]
    if kind == "trial":
        row, vec = expected_cg(obj, d, R_TRIAL, pad(st[:k], min(npts, 3)), 0.0, 0.0)
        return row, None
    if k == 0:
        return expected_cg(obj, d, ACC, [], a_acc, beta)
    return expected_cg(obj, d, ACC_T, pad(st[:k], npts), a_acc, beta)


def model_launch(obj, n, npts, ks, ka):
    """inputs and expectations of one launch of (a): data, script, rows, final x / u"""
    mode = ACC if ka == 0 else ACC_T
    d, a_acc, beta = launch_inputs(obj.name, mode if ka is not None else R_TRIAL, n)
    if obj is Rosen and n > ROSEN_GENERAL_MAX and not (ka is not None and ka > 0):
        # the quartic's general data run out of budget (Σ|t| ≥ 2⁵² quanta in the f slot) near 1e6 elements: above 2¹⁹ the
        # trials and the direction-only accept run on the valley data as well, the accept with a_acc = β = 1/2
        d = Data(n, rosen_valley_period())
    st = STEPS[obj.name]
    script, rows = [], []
    for k in ks:
        script.append(("trial", st[:k]))
        rows.append(expected_pass(obj, d, npts, "trial", k, 0, 0)[0])
    x, u = d.full["x"], d.full["u"]
    if ka is not None:
        script.append(("accept_dir_trial", a_acc, beta, st[:ka]))
        row, vec = expected_pass(obj, d, npts, "accept", ka, a_acc, beta)
        rows.append(row)
        x, u = vec["x"], vec["u"]
    return d, script, rows, x, u


def objects_for(key):
    """(objective, n) pairs that run a size: odd n is QuadDiag's (and the user body's); paired Rosenbrock takes the even
    neighbour below — 16c − 2, 255c, 17c: a short last workgroup that is not a single pair, 17 full workgroups — unless that
    neighbour is a size of the table itself"""
    c, n = key
    out = [(Quad, n)]
    if n % 2 == 0:
        out.append((Rosen, n))
    elif n > 2 and (c, n - 1) not in SIZES:
        out.append((Rosen, n - 1))
    return out


# even sizes for the objective without a parameter vector: 17 workgroups with a second group of one PAIR, 256 with a last pair
EVEN_EXTRA = [(c, m * c + 2) for c in CHUNKS for m in (16, 255) if (c, m * c + 2) not in SIZES]   # (c = 2: 255c + 2 = 256c)


def test_even_extra_sizes():
    for c, n in EVEN_EXTRA:
        g, ch = plan(n, c, 2, STATIC_LDS[3])
        assert ch == c and g == (n - 2) // c + 1 and last_chunk(n, g, ch) == 2 and (c, n) not in SIZES


def test_exact_data_meet_their_preconditions():
    """CPU tier: every launch of (a) — the trials on the accepting pass's data included — is exact and order-independent (the
    model asserts it operation by operation and slot by slot)."""
    for obj in (Quad, Rosen, Booth):
        keys = [(None, 2)] if obj is Booth else [k for k in ((None, 3), (8, 137), (512, 16 * 512 + 1), (4096, 256 * 4096 + 2),
                                                             (None, 1000000), (None, largest(2, 1)), (None, largest(3, 1)))]
        for c, n in keys:
            if obj is Rosen:
                n &= ~1
            for npts in (1, 3, 7):
                for ks, ka in launches_for(npts):
                    model_launch(obj, n, npts, ks, ka)
    for n in CHAIN_SIZES + [chunk_max(4, STATIC_LDS_CHAIN[1]), chunk_max(4, STATIC_LDS_CHAIN[3]) - 1]:
        for npts in (1, 3):
            for ks, ka in launches_for(npts):
                chain_model_launch(n, npts, ks, ka)


def chain_model_launch(n, npts, ks, ka):
    valley = ka is not None and ka > 0      # along u = −∇f the quartic has no budget on general data: x = 0, a_acc = β = 0 there
    a_acc, beta = (0.0, 0.0) if valley else CHAIN_SCAL
    x, u = _chain_x(n, valley)
    nt = min(npts, 3)
    W, Wt = row_width(npts), row_width(nt)
    script, rows = [], []
    for k in ks:
        script.append(("trial", CHAIN_STEPS[:k]))
        rows.append(expected_chain(x, u, R_TRIAL, pad(CHAIN_STEPS[:k], nt), 0.0, 0.0)[0][:Wt])
    xo, uo = x, u
    if ka is not None:
        script.append(("accept_dir_trial", a_acc, beta, CHAIN_STEPS[:ka]))
        if ka == 0:
            s, out = expected_chain(x, u, ACC, [], a_acc, beta)
            rows.append(s[:10])
        else:
            s, out = expected_chain(x, u, ACC_T, pad(CHAIN_STEPS[:ka], npts), a_acc, beta)
            rows.append(s[:W])
        xo, uo = out["x"], out["u"]
    return (x, u), script, rows, xo, uo


# ---- GPU -------------------------------------------------------------------------------------------------------------------
REACHED = set()
CELLS = defaultdict(int)            # (symbol, n, policy chunk) -> passes whose rows were compared in every workgroup
SLOTS = [0]


@pytest.fixture(scope="module")
def ctx(cgo):
    c = cgo.Context(0)
    yield c
    c.close()


def _solver(cgo, o, chunk, npts):
    pol = cgo.SolverPolicy(resident=True, controller_depth=0, resident_chunk=chunk, resident_points=npts)
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.DisableTrace(), max_iters=5)
    return cgo.Solver(o, cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), pol)


def check_launch(tag, got, script, rows, x, u, npts, mism, exact=True):
    """rows of every workgroup, the doubles behind them, the member functions' outputs, x, u"""
    ok = True
    for q, want in enumerate(rows):
        r = got["rows"][q]
        if r.shape[1] != want.size:
            mism.append(f"{tag} pass {q}: rows of {r.shape[1]} slots, expected {want.size}")
            return False
        if exact:
            bad = np.nonzero(bits(r) != bits(want)[None, :])
            if bad[0].size:
                w, s = int(bad[0][0]), int(bad[1][0])
                mism.append(f"{tag} pass {q} {script[q][0]} k={len(script[q][-1])}: {bad[0].size} cells differ in "
                            f"{np.unique(bad[0]).size} of {r.shape[0]} workgroups; first: workgroup {w} slot {s} holds {r[w, s]!r}, exact {want[s]!r}")
                ok = False
        if not np.all(bits(got["tail"][q]) == NAN_BITS):
            mism.append(f"{tag} pass {q}: doubles behind the row's {want.size} slots were written")
            ok = False
        # the mapping row -> TrialSums / gu / uu, as workgroup 0 got them
        o, r0 = got["out"][q], r[0]
        kind, k = script[q][0], len(script[q][-1])
        npt = min(npts, 3) if kind == "trial" else (0 if k == 0 else npts)
        ts = np.zeros((7, 7))
        ts[:npt] = r0[:RS * npt].reshape(npt, RS)
        gu, uu = (0.0, 0.0) if kind == "trial" else ((r0[RS], r0[RS + 1]) if k == 0 else (r0[RS * npts], r0[RS * npts + 1]))
        if not (np.array_equal(bits(o["ts"]), bits(ts)) and bits(o["gu"]) == bits(gu) and bits(o["uu"]) == bits(uu)):
            mism.append(f"{tag} pass {q}: what {kind} returned is not its row")
            ok = False
        SLOTS[0] += r.size
    for name, w in (("x", x), ("u", u)):
        if not np.array_equal(bits(got[name]), bits(w)):
            i = int(np.nonzero(bits(got[name]) != bits(w))[0][0])
            mism.append(f"{tag}: {name} after the launch differs first at element {i} of {w.size}: {got[name][i]!r}, want {w[i]!r}")
            ok = False
    return ok


def _report(mism):
    assert not mism, f"{len(mism)} mismatch(es):\n" + "\n".join(mism[:20])


def run_exact(cgo, ctx, obj, key, npts_list=(1, 3, 7)):
    chunk, n = key
    mism = []
    vecs = 3 if obj.param else 2
    for npts in npts_list:
        o = _make_objective(cgo, obj, n, ctx, launch_inputs(obj.name, R_TRIAL, n)[0])
        s = _solver(cgo, o, chunk, npts)
        try:
            rnd = 0
            for ks, ka in launches_for(npts):
                d, script, rows, x, u = model_launch(obj, n, npts, ks, ka)
                got = s.probe_resident(script, d.full["x"], d.full["u"])
                REACHED.add(got["symbol"])
                tag = f"{obj.name} n={n} chunk={chunk} points={npts} grid={got['grid']}x{got['chunk']} round0={got['round0']} [{got['symbol']}]"
                # (the user module's kernel too: it has the built-in instantiation's static LDS, which this asserts at its largest size)
                assert (got["grid"], got["chunk"]) == plan(n, chunk, vecs, STATIC_LDS[npts]), tag
                assert got["round0"] == rnd and got["points"] == npts, tag
                assert got["wrote_back"] == (ka is not None)
                rnd += len(script)
                if check_launch(tag, got, script, rows, x, u, npts, mism):
                    CELLS[(got["symbol"], n, chunk)] += len(script)
        finally:
            s.close(); o.close()
    return mism


def _ids(key):
    return f"c{key[0]}-n{key[1]}"


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(SIZES, key=lambda k: (k[0] or 0, k[1])), ids=_ids)
def test_exact_every_slot_every_workgroup(cgo, ctx, key):
    """(a) QuadDiag at every size, paired Rosenbrock at the even ones and at the even neighbours of the odd ones, points 1, 3, 7."""
    mism = []
    for obj, n in objects_for(key):
        mism += run_exact(cgo, ctx, obj, (key[0], n))
    _report(mism)


@pytest.mark.gpu
@pytest.mark.parametrize("key", EVEN_EXTRA, ids=_ids)
def test_exact_even_extra_sizes(cgo, ctx, key):
    _report(run_exact(cgo, ctx, Rosen, key) + run_exact(cgo, ctx, Quad, key))


@pytest.mark.gpu
def test_booth_exact(cgo, ctx):
    _report(run_exact(cgo, ctx, Booth, (None, 2)))


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(SIZES, key=lambda k: (k[0] or 0, k[1])), ids=_ids)
def test_user_module_exact(cgo, ctx, key):
    """The run-time compiled module's k_resident<UserObjective, 3> — a binary of its own, so QuadDiag's cells do not cover it:
    every size of the table, odd and even (the user body takes odd n like QuadDiag), its plan asserted as well.  One module
    is compiled per objective, i.e. per size; its PROBE form on the first probe of that objective, from the same source."""
    _report(run_exact(cgo, ctx, User, key, npts_list=(3,)))


@pytest.mark.gpu
def test_user_module_largest_size_that_fits_and_one_more(cgo, ctx):
    n = largest(3, 3)
    _report(run_exact(cgo, ctx, User, (None, n), npts_list=(3,)))
    d = launch_inputs(User.name, R_TRIAL, n + 1)[0]
    o = _make_objective(cgo, User, n + 1, ctx, d)
    s = _solver(cgo, o, None, 3)
    try:
        with pytest.raises(cgo.CgoError) as e:
            s.probe_resident([("trial", [0.25])], d.full["x"], d.full["u"])
        assert e.value.code == 1
    finally:
        s.close(); o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("param", [True, False], ids=["with-parameter-vector", "without"])
def test_largest_size_that_fits_and_one_more(cgo, ctx, param):
    """256 workgroups with chunks that fill the LDS (QuadDiag: x, u, D; paired Rosenbrock: x, u); one element more (for the
    paired objective: one pair more) is not the resident solver's: CGO_EINVAL."""
    obj = Quad if param else Rosen
    for npts in (1, 3, 7):
        n = largest(3 if param else 2, npts)
        _report(run_exact(cgo, ctx, obj, (None, n), npts_list=(npts,)))
        n1 = n + (1 if param else 2)
        d = launch_inputs(obj.name, R_TRIAL, n1)[0]
        o = _make_objective(cgo, obj, n1, ctx, d)
        s = _solver(cgo, o, None, npts)
        try:
            with pytest.raises(cgo.CgoError) as e:
                s.probe_resident([("trial", [0.25])], d.full["x"], d.full["u"])
            assert e.value.code == 1
        finally:
            s.close(); o.close()


# ---- a second launch that continues from the state the first one's accept left ------------------------------------------------
CONT_KEYS = [(8, 137), (512, 17 * 512 + 1), (None, 1000000)]
CONT_STEPS, CONT_SCAL = [(j + 1) / 64 for j in range(3)], (1 / 64, 0.25)


def continued_model(n, npts):
    """QuadDiag: launch 1 = [trial, accept k = npts] on the exact period; launch 2 = [trial k = 1, trial k = min(npts, 2), accept
    k = 0] on the state launch 1 wrote back — still periodic (element-wise), its exactness asserted like the first's."""
    from test_kernel_sums import cg_model, exact_period
    d, script1, rows1, x1, u1 = model_launch(Quad, n, npts, [1], npts)
    per = exact_period("quad_diag")
    a_acc, beta = launch_inputs("quad_diag", ACC_T, n)[1:]
    _, out = cg_model(Quad, per["x"], per["u"], per["p"], per["x2"], ACC_T, pad(STEPS["quad_diag"][:npts], npts), a_acc, beta, False)
    d2 = Data(n, dict(x=out["x"], u=out["u"], p=per["p"], x2=per["x2"]))
    assert np.array_equal(bits(d2.full["x"]), bits(x1)) and np.array_equal(bits(d2.full["u"]), bits(u1))
    nt = min(npts, 3)
    script2, rows2 = [], []
    for k in (1, min(npts, 2)):
        script2.append(("trial", CONT_STEPS[:k]))
        rows2.append(expected_cg(Quad, d2, R_TRIAL, pad(CONT_STEPS[:k], nt), 0.0, 0.0)[0])
    script2.append(("accept_dir_trial", *CONT_SCAL, []))
    row, vec = expected_cg(Quad, d2, ACC, [], *CONT_SCAL)
    rows2.append(row)
    return d, (script1, rows1, x1, u1), (script2, rows2, vec["x"], vec["u"])


def test_continued_launch_data_meet_their_preconditions():
    for chunk, n in CONT_KEYS:
        for npts in (1, 3, 7):
            continued_model(n, npts)


@pytest.mark.gpu
@pytest.mark.parametrize("key", CONT_KEYS, ids=_ids)
def test_second_launch_continues_from_the_accepted_state(cgo, ctx, key):
    """Two launches back to back (2 and 3 passes): the second reads what the first wrote back and swapped in — uploaded again
    from the first's own output, so its input IS the device's result — and starts at exchange round 2."""
    chunk, n = key
    mism = []
    for npts in (1, 3, 7):
        d, first, second = continued_model(n, npts)
        o = _make_objective(cgo, Quad, n, ctx, d)
        s = _solver(cgo, o, chunk, npts)
        try:
            got = s.probe_resident(first[0], d.full["x"], d.full["u"])
            tag = f"quad_diag n={n} chunk={chunk} points={npts} [{got['symbol']}] launch 1"
            ok = check_launch(tag, got, *first, npts, mism)
            got2 = s.probe_resident(second[0], got["x"], got["u"])
            assert got2["round0"] == 2 and got2["wrote_back"]
            if check_launch(tag[:-1] + "2", got2, *second, npts, mism) and ok:
                CELLS[(got["symbol"], n, chunk)] += 5
        finally:
            s.close(); o.close()
    _report(mism)


def run_chain_exact(cgo, ctx, n):
    mism = []
    for npts in (1, 3):
        o = cgo.RosenbrockChained(n, ctx)
        s = _solver(cgo, o, None, npts)
        try:
            for ks, ka in launches_for(npts):
                (x, u), script, rows, xo, uo = chain_model_launch(n, npts, ks, ka)
                got = s.probe_resident(script, x, u)
                REACHED.add(got["symbol"])
                tag = f"chained n={n} points={npts} [{got['symbol']}]"
                assert (got["grid"], got["chunk"]) == plan_chain(n, npts), tag
                if check_launch(tag, got, script, rows, xo, uo, npts, mism):
                    CELLS[(got["symbol"], n, None)] += len(script)
        finally:
            s.close(); o.close()
    return mism


@pytest.mark.gpu
@pytest.mark.parametrize("n", CHAIN_SIZES, ids=lambda n: f"n{n}")
def test_chain_exact(cgo, ctx, n):
    """k_resident_chain: the window flags at the first / last / last-but-one pair, the padded element of odd n, two LDS copies."""
    _report(run_chain_exact(cgo, ctx, n))


@pytest.mark.gpu
def test_chain_largest_sizes(cgo, ctx):
    cm1, cm3 = chunk_max(4, STATIC_LDS_CHAIN[1]), chunk_max(4, STATIC_LDS_CHAIN[3])
    mism = []
    for n in sorted({cm3, cm3 - 1}):
        mism += run_chain_exact(cgo, ctx, n)
    _report(mism)
    for npts, cm in ((1, cm1), (3, cm3)):
        x, u = _chain_x(cm + 1, False)
        o = cgo.RosenbrockChained(cm + 1, ctx)
        s = _solver(cgo, o, None, npts)
        try:
            with pytest.raises(cgo.CgoError) as e:
                s.probe_resident([("trial", [0.5])], x, u)
            assert e.value.code == 1
        finally:
            s.close(); o.close()


@pytest.mark.gpu
def test_probed_solver_refuses_to_run_and_bad_passes_are_refused(cgo, ctx):
    d = launch_inputs("quad_diag", R_TRIAL, 137)[0]
    o = _make_objective(cgo, Quad, 137, ctx, d)
    s = _solver(cgo, o, 8, 3)
    try:
        for bad in ([("trial", [])], [("trial", [0.25] * 4)], [("accept_dir_trial", 0.5, 0.5, [0.25] * 4)]):
            with pytest.raises(cgo.CgoError) as e:
                s.probe_resident(bad, d.full["x"], d.full["u"])
            assert e.value.code == 1
        s.probe_resident([("trial", [0.25])], d.full["x"], d.full["u"])
        with pytest.raises(cgo.CgoError) as e:
            s.start()
        assert e.value.code == 5
    finally:
        s.close(); o.close()
    o = _make_objective(cgo, Quad, 137, ctx, d)
    pol = cgo.SolverPolicy(resident=False, controller_depth=0)
    s = cgo.Solver(o, cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.DisableTrace(), max_iters=5), cgo.setupStrongWolfeBisection(1e-5, 0.1), pol)
    try:
        with pytest.raises(cgo.CgoError) as e:
            s.probe_resident([("trial", [0.25])], d.full["x"], d.full["u"])
        assert e.value.code == 1
    finally:
        s.close(); o.close()


# ---- (b) random data -------------------------------------------------------------------------------------------------------
U53 = 2.0 ** -53


def resident_depth(chunk, W, grid, terms_per_pair=2):
    """Longest chain of additions a term goes through on its way into a total (one rounding each; the products enter exactly):
    the lane's accumulator over its ⌈pairs/256⌉ pairs × terms per pair, the odd element, six wave levels, four waves
    (wg_reduce_n), then per hop of the exchange at most four rows per lane and the Gp = 256 / W lane-group partials — two hops."""
    trips = -(-(chunk // 2) // BLOCK)
    hops = 0 if grid == 1 else 2
    return terms_per_pair * trips + 1 + 6 + 4 + hops * (4 + BLOCK // W)


def b_script(kind, npts):
    """several accepting passes in a row, mixed widths, trials in between: ≥ 9 passes in ONE launch"""
    if kind == "chain":
        return [("A", npts), ("T", 1), ("A", 0), ("T", min(npts, 2)), ("A", 1), ("A", 0), ("T", min(npts, 3)), ("A", npts), ("T", 1), ("A", 0)]
    if kind == "rosen":
        return [("T", 1), ("A", npts), ("T", min(npts, 2)), ("A", 0), ("T", min(npts, 3)), ("A", npts), ("T", 1), ("T", 1), ("A", 0), ("T", 1)]
    return [("A", npts), ("T", 1), ("A", 0), ("T", min(npts, 3)), ("A", npts), ("A", 0), ("A", max(npts - 2, 1)), ("T", min(npts, 2)),
            ("A", 0), ("A", npts), ("T", 1)]


def b_model(kind, n, npts, seed):
    """script, per-pass (W, refs), final x, u — the plain IEEE model, pass after pass"""
    data, scal, su, sg = random_data(kind, n, seed)
    x, u = data["x"].copy(), data["u"].copy()
    x0, u0 = x.copy(), u.copy()
    nt = min(npts, 3)
    moved = False                         # after the first accept u = −∇f + β·u: the small steps
    script, refs = [], []
    for what, k in b_script(kind, npts):
        st = (sg if moved else su)
        a_acc = scal[0] if not moved or kind == "quad" else st[0]
        beta = scal[1]
        if what == "T":
            a = list(st[:k])
            script.append(("trial", a))
            mode, ap = R_TRIAL, pad(a, nt)
        else:
            a = list(sg[:k])              # the accepting pass's trials run along the NEW direction
            script.append(("accept_dir_trial", a_acc, beta, a))
            mode, ap = (ACC, []) if k == 0 else (ACC_T, pad(a, npts))
        if kind == "chain":
            T = {}
            CHECK_EXACT[0] = False
            try:
                _, vec = expected_chain(x, u, mode, ap, a_acc if what == "A" else 0.0, beta if what == "A" else 0.0, terms_out=T)
            finally:
                CHECK_EXACT[0] = True
            W = 10 if (what == "A" and k == 0) else row_width(nt if what == "T" else npts)
            r = _slot_refs(T)
        else:
            obj = Quad if kind == "quad" else Rosen
            W, r, vec = float_cg(obj, x, u, data["p"], x, mode, ap, a_acc if what == "A" else 0.0, beta if what == "A" else 0.0, True)
        refs.append((W, r))
        if what == "A":
            x, u = vec["x"], vec["u"]
            moved = True
    return data, x0, u0, script, refs, x, u


B_CASES = [("quad", 8, 137, 7), ("quad", 8, 137, 3), ("quad", 2, 2 * 256 + 3, 7), ("quad", 512, 16 * 512 + 1, 7), ("quad", 512, 17 * 512 + 1, 1),
           ("quad", 1024, 255 * 1024 + 1, 3), ("rosen", 8, 136, 7), ("rosen", 512, 17 * 512 + 2, 3), ("rosen", 1024, 40 * 1024 + 2, 7),
           ("chain", None, 1001, 3), ("chain", None, 514, 1), ("chain", None, 7, 3)]


def _b_plan(kind, chunk, n, npts):
    if kind == "chain":
        return plan_chain(n, npts)
    return plan(n, chunk, 3 if kind == "quad" else 2, STATIC_LDS[npts])


def b_guard(kind, chunk, n, npts):
    data, x0, u0, script, refs, x, u = b_model(kind, n, npts, 4000 + n)
    grid, ch = _b_plan(kind, chunk, n, npts)
    for q, (W, r) in enumerate(refs):
        d = resident_depth(ch, W, grid, 2 if kind != "chain" else 4)
        for slot, (exact, absum, tmin) in r.items():
            assert tmin > d * U53 * absum * 1.01, (kind, n, npts, q, slot, tmin, absum)
    return data, x0, u0, script, refs, x, u, grid, ch


def test_random_data_meet_the_guard():
    """CPU tier: every slot of every pass of (b) has its smallest term above its bound, so that a dropped or doubled element
    cannot hide in it; the chained scripts have ≥ 3 writing passes (both LDS copies have been source and destination)."""
    for kind, chunk, n, npts in B_CASES:
        b_guard(kind, chunk, n, npts)
    for kind in ("quad", "rosen", "chain"):
        for npts in (1, 3, 7):
            sc = b_script(kind, npts)
            assert len(sc) >= 9 and sum(1 for w, _ in sc if w == "A") >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("kind,chunk,n,npts", B_CASES, ids=lambda v: str(v))
def test_random_all_workgroups_agree_and_within_bound(cgo, ctx, kind, chunk, n, npts):
    """(b): (i) every workgroup's row bitwise equal to workgroup 0's in every pass; (ii) each slot within γ_d·Σ|t| of the
    correctly rounded exact sum (d: resident_depth; slots without terms zero); x, u after the launch bitwise the model's."""
    data, x0, u0, script, refs, x, u, grid, ch = b_guard(kind, chunk, n, npts)
    o = cgo.QuadDiag(data["p"], ctx) if kind == "quad" else (cgo.RosenbrockPaired(n, ctx) if kind == "rosen" else cgo.RosenbrockChained(n, ctx))
    s = _solver(cgo, o, chunk, npts)
    mism = []
    try:
        got = s.probe_resident(script, x0, u0)
        REACHED.add(got["symbol"])
        tag = f"{kind} n={n} chunk={chunk} points={npts} grid={got['grid']} [{got['symbol']}]"
        assert (got["grid"], got["chunk"]) == (grid, ch), tag
        want_rows = [np.zeros(W) for W, _ in refs]
        check_launch(tag, got, script, want_rows, x, u, npts, mism, exact=False)
        for q, (W, r) in enumerate(refs):
            rows = got["rows"][q]
            diff = np.nonzero(bits(rows) != bits(rows[0])[None, :])
            if diff[0].size:
                mism.append(f"{tag} pass {q}: workgroup {int(diff[0][0])} holds {rows[diff[0][0], diff[1][0]]!r} in slot {int(diff[1][0])}, "
                            f"workgroup 0 {rows[0, diff[1][0]]!r} ({np.unique(diff[0]).size} workgroups differ)")
            d = resident_depth(ch, W, grid, 2 if kind != "chain" else 4)
            gam = d * U53 / (1 - d * U53)
            for slot in range(W):
                v = rows[0, slot]
                if slot not in r:
                    if bits(v) != 0:
                        mism.append(f"{tag} pass {q}: slot {slot} carries no term, holds {v!r}")
                    continue
                exact, absum, tmin = r[slot]
                if not abs(v - exact) <= gam * absum * (1 + 1e-12):
                    mism.append(f"{tag} pass {q}: slot {slot} {v!r} vs {exact!r} (bound {gam * absum:.3e})")
    finally:
        s.close(); o.close()
    _report(mism)


@pytest.mark.gpu
def test_random_default_policy_all_workgroups_agree(cgo, ctx):
    """(b)(i) at BASELINE config 2's size under the default policy (245 workgroups: 15 groups + 5), 7 and 3 points."""
    n = 1000000
    data, scal, su, sg = random_data("quad", n, 4000 + n)
    mism = []
    for npts in (3, 7):
        o = cgo.QuadDiag(data["p"], ctx)
        s = _solver(cgo, o, None, npts)
        script = []
        for what, k in b_script("quad", npts):
            script.append(("trial", su[:k]) if what == "T" else ("accept_dir_trial", scal[0], scal[1], sg[:k]))
        try:
            for rep in range(2):
                got = s.probe_resident(script, data["x"], data["u"])
                assert got["grid"] == 245 and got["round0"] == rep * len(script)
                for q, rows in enumerate(got["rows"]):
                    diff = np.nonzero(bits(rows) != bits(rows[0])[None, :])
                    if diff[0].size:
                        mism.append(f"points={npts} launch {rep} pass {q}: {np.unique(diff[0]).size} workgroups differ from workgroup 0")
                    assert np.all(np.isfinite(rows))
        finally:
            s.close(); o.close()
    _report(mism)


# ---- (c) coverage ----------------------------------------------------------------------------------------------------------
WANT = {f"k_resident<{on}, {p}>" for on in ("ObjQuadDiag", "ObjRosenPaired", "ObjBooth") for p in (1, 3, 7)} | \
    {"k_resident_chain<1>", "k_resident_chain<3>", "k_resident<UserObjective, 3>"}


def test_dispatch_tables_have_tests():
    """CPU tier: the dispatchable instantiations (the rows of csrc/cgo_instances.def) are the ones this module probes; each has
    its PROBE twin: res_kernel / res_kernel_for and the run-time module expand both forms from the same row."""
    can = {f"k_resident<{on}, {p}>" for kind, on in I.rows("OBJ") for p, in I.rows("RESIDENT")}
    can |= {f"k_resident_chain<{p}>" for p, in I.rows("RESIDENT_CHAIN")} | {f"k_resident<UserObjective, {p}>" for p, in I.rows("RTC_RESIDENT")}
    assert can == WANT


@pytest.mark.gpu
def test_coverage_of_every_instantiation(cgo, ctx):
    """Every dispatchable instantiation was probed with its whole row compared in every workgroup; one the tests above did
    not reach (this test on its own) is probed here at a small multi-workgroup size."""
    reached = lambda: {s.replace(", true>", ">") for s in REACHED}
    mism = []
    for sym in sorted(WANT - reached()):
        m = re.match(r"k_resident(_chain)?<(?:(\w+), )?(\d)>", sym)
        npts = int(m.group(3))
        if m.group(1):
            mism += run_chain_exact(cgo, ctx, 513)
        else:
            obj = {"ObjQuadDiag": Quad, "ObjRosenPaired": Rosen, "ObjBooth": Booth, "UserObjective": User}[m.group(2)]
            key = (None, 2) if obj is Booth else ((8, 137) if obj.param else (8, 136))
            mism += run_exact(cgo, ctx, obj, key, npts_list=(npts,))
    _report(mism)
    assert not WANT - reached(), sorted(WANT - reached())
    assert all(any(sym.replace(", true>", ">") == w for (sym, n, c) in CELLS) for w in WANT)
    print(f"\n[resident kernel sums] {len(CELLS)} (instantiation, size, chunk) cells, {sum(CELLS.values())} passes, "
          f"{SLOTS[0]} (workgroup, slot) values compared")
