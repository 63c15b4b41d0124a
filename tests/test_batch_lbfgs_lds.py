"""GPU tier: the LDS tier of batched L-BFGS solves — rows="lds" of cgo.minimizeobjectivebatch_lbfgs[_obj]
(k_batch_lbfgs_lds: one workgroup per problem, its rows and ring in LDS during a launch).  CPU tier: tests/test_batch_lbfgs_lds_abi.py.

The design constraint is that every number has the BITS of the device tier (rows="device", k_batch_lbfgs), which
tests/test_batch_lbfgs.py and tests/test_batch_lbfgs_user.py hold to the oracle: so most of this file compares the two tiers as
uint64 views, and the loop shapes of the new kernel are held to the oracle with tests/test_batch.py's assert_bar as well."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import _batch_lbfgs_problems as Q
import _batch_lbfgs_user_problems as U
from _cases import _product_structs, run_oracle
from test_batch import assert_bar
from test_batch_kernel_sums import (KIND, PUSH_A, RES_BUDGET, RES_STOP, STEPS, Booth, Quad, Rosen, _lbfgs_inputs, _stack, coefs,
                                    drop_problem, lbfgs_problem, padding_intact, params_of, words)
from test_kernel_sums import NAN_BITS

pytestmark = pytest.mark.gpu

_ORACLE = {}
ROWS_LDS, ROWS_DEVICE, ROWS_AUTO = 0, 1, 2      # CGO_BATCH_ROWS_* (include/cgo.h)
TNAME = {Quad: "ObjQuadDiag", Rosen: "ObjRosenPaired", Booth: "ObjBooth"}


def oracle_of(c):
    key = (c.objective, c.n, c.x0.tobytes(), None if c.D is None else c.D.tobytes(), c.beta, c.m, c.ls, c.cond, c.c1, c.c2, c.eps, c.max_iters,
           c.zoom_max_iters, c.ls_max_iters)
    if key not in _ORACLE:
        _ORACLE[key] = run_oracle(c)
    return _ORACLE[key]


def u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b, tag=""):
    """every array of two Results as uint64 views (so NaN payloads and the sign of zero count)"""
    assert (a.status, a.iters_ran, a.total_fdf_evals) == (b.status, b.iters_ran, b.total_fdf_evals), tag
    for f in ("objective", "minimizer", "gradient"):
        assert np.array_equal(u64(getattr(a, f)), u64(getattr(b, f))), f"{tag}: {f}"
    for f in ("objective", "grad_norm", "step_size"):
        assert np.array_equal(u64(getattr(a.trace, f)), u64(getattr(b.trace, f))), f"{tag}: trace.{f}"
    assert np.array_equal(a.trace.objective_evals, b.trace.objective_evals), f"{tag}: trace.objective_evals"


def same_batch(lds, dev, tag=""):
    assert len(lds) == len(dev) and (lds.launches, lds.handed_back) == (dev.launches, dev.handed_back), (tag, lds.launches, dev.launches)
    for b, (x, y) in enumerate(zip(lds, dev)):
        same_bits(x, y, f"{tag} problem {b}")


def run(cgo, ctx, cases, rows, slice_iters=0):
    c0 = cases[0]
    _, _, cfg, ls = _product_structs(c0)
    X0 = np.stack([c.x0 for c in cases])
    D = np.stack([c.D for c in cases]) if c0.D is not None else None
    out = cgo.minimizeobjectivebatch_lbfgs(c0.objective, X0, cfg, ls, D=D, ctx=ctx, slice_iters=slice_iters, rows=rows)
    assert len(out) == len(cases)
    return out


def limit(cgo, ctx, c):
    return cgo.batch_lbfgs_max_n(c.objective, ctx, m=c.m, rows="lds")


def both(cgo, ctx, cases, slice_iters=0, tag=""):
    lds, dev = run(cgo, ctx, cases, "lds", slice_iters), run(cgo, ctx, cases, "device", slice_iters)
    assert lds.rows == "lds" and dev.rows == "device"
    same_batch(lds, dev, tag or cases[0].name)
    return lds


# ---- 1. identity with the device tier on every batch of the device tier's tests ------------------------------------------------------
def every_batch(cgo):
    block, u = cgo.batch_lbfgs_shape()
    assert block == Q.BLOCK
    return Q.all_batches(block, u)


@pytest.mark.parametrize("part", range(4))
def test_every_batch_of_the_device_tier_has_the_same_bits(cgo, gpu_ctx, part):
    """Left out of rows="lds" — n above what one workgroup's LDS holds for its m — are exactly: paired Rosenbrock n = 1000, m = 10
    (24 rows: n ≤ 810), the quadratic n = 1000, m = 10 (25 rows: n ≤ 778), and the two batches of the device tier's longest loop
    shape, the quadratic n = 2562 and n = 2563 with m = 4 (13 rows of 2564 doubles are 267 KB: n ≤ 1496).  They run under
    rows="auto" on device rows, with the same bits, and are refused under rows="lds".  (rows="auto" is device rows for the others too: the rule of include/cgo.h.)  Every other batch of
    tests/_batch_lbfgs_problems.all_batches runs in both tiers."""
    batches = every_batch(cgo)
    out_names = sorted(b[0].name for b in batches if b[0].n > limit(cgo, gpu_ctx, b[0]))
    assert out_names == ["quad1000-m10-b0", "quad2562-m4-b0", "quad2563-m4-b0", "rosen1000-m10-b0"], out_names
    ran = 0
    for i, cases in enumerate(batches):
        fits = cases[0].n <= limit(cgo, gpu_ctx, cases[0])
        if i % 4 != part:
            ran += fits
            continue
        if fits:
            both(cgo, gpu_ctx, cases)
            auto = run(cgo, gpu_ctx, cases, "auto")
            assert auto.rows == "device"       # the rule of include/cgo.h as measured: device rows at every n
            ran += 1
        else:
            auto, dev = run(cgo, gpu_ctx, cases, "auto"), run(cgo, gpu_ctx, cases, "device")
            assert auto.rows == "device"
            same_batch(auto, dev, cases[0].name)
            with pytest.raises(cgo.CgoError, match=r"cgo_batch_lbfgs_max_n_ex = %d" % limit(cgo, gpu_ctx, cases[0])) as e:
                run(cgo, gpu_ctx, cases, "lds")
            assert e.value.code == 1
    assert ran == len(batches) - 4


# ---- 2. every shape of the new kernel's loops -----------------------------------------------------------------------------------------
def lds_pairs(cgo, K=1):
    block, u = cgo.batch_lbfgs_lds_shape(K)
    assert block == Q.BLOCK and 1 <= u <= 8
    T = u * block
    return block, T, [1, block - 1, block, T - 1, T, T + 1, 2 * T + 1]


def held_and_same(cgo, ctx, cases):
    out = both(cgo, ctx, cases)
    for c, got in zip(cases, out):
        assert_bar(got, oracle_of(c), c.name)
    return out


@pytest.mark.parametrize("odd", [0, 1], ids=["even", "odd-tail"])
@pytest.mark.parametrize("which", range(7))
def test_quadratic_at_every_shape_of_the_lds_loops(cgo, gpu_ctx, which, odd):
    _, _, pairs = lds_pairs(cgo)
    n = 2 * pairs[which] + odd
    out = held_and_same(cgo, gpu_ctx, [Q.quad(n, b, 3, max_iters=8) for b in range(3)])
    assert out.handed_back == 0 and out.launches == 1


def test_rosenbrock_around_one_trip_and_booth(cgo, gpu_ctx):
    _, T, _ = lds_pairs(cgo, 0)
    for n in (2 * T - 2, 2 * T, 2 * T + 2):
        out = held_and_same(cgo, gpu_ctx, [Q.rosen(n, b, 3, max_iters=8) for b in range(3)])
        assert out.handed_back == 0 and out.launches == 1
    booth = Q.distinct_batches()[-1]
    assert booth[0].objective == "booth"
    held_and_same(cgo, gpu_ctx, booth)


# ---- 3. at the limit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,m", [("quad_diag", 10), ("quad_diag", 1), ("rosenbrock_paired", 5)])
def test_at_the_largest_n_the_lds_holds(cgo, gpu_ctx, kind, m):
    n = cgo.batch_lbfgs_max_n(kind, gpu_ctx, m=m, rows="lds")
    K = 1 if kind == "quad_diag" else 0
    rows = cgo.batch_lbfgs_lds_rows(K, m)
    print(f"{kind} m = {m}: {rows} rows, largest n = {n}")
    # the helper's own arithmetic: even, and one more pair would pass 160 KiB less the kernel's static LDS (≥ 7 KB) and the slack
    assert n % 2 == 0 and 8 * rows * n <= 160 * 1024 - 512 - 7000 < 8 * rows * (n + 2) + 2048
    assert cgo.batch_lbfgs_max_n(kind, gpu_ctx, m=m, rows="auto") == cgo.batch_lbfgs_max_n(kind, gpu_ctx) == cgo.batch_lbfgs_max_n(kind, gpu_ctx, m=m)
    assert cgo.batch_lbfgs_max_n(kind, gpu_ctx, m=11, rows="lds") == 0 == cgo.batch_lbfgs_max_n(kind, gpu_ctx, m=0, rows="lds")
    make = (lambda nn, b: Q.quad(nn, b, m, max_iters=6)) if kind == "quad_diag" else (lambda nn, b: Q.rosen(nn, b, m, max_iters=6))
    out = both(cgo, gpu_ctx, [make(n, b) for b in range(2)])
    assert out.handed_back == 0 and all(r.iters_ran == 6 for r in out)
    over = [make(n + 2, b) for b in range(2)]
    with pytest.raises(cgo.CgoError, match=r"cgo_batch_lbfgs_max_n_ex = %d" % n) as e:
        run(cgo, gpu_ctx, over, "lds")
    assert e.value.code == 1
    auto = run(cgo, gpu_ctx, over, "auto")
    assert auto.rows == "device"
    same_batch(auto, run(cgo, gpu_ctx, over, "device"))


# ---- 4. the ring across launches ---------------------------------------------------------------------------------------------------
def test_ring_survives_launch_boundaries(cgo, gpu_ctx):
    """m = 10 over 24 iterations, the ring of 11 slots wraps twice: one launch against slices of 1 and 3 iterations — the load
    of the stored pairs at entry and the write-back of the written slots at exit, with records and trace"""
    cases = Q.wrap_batch()
    assert cases[0].m == 10 and cases[0].n <= limit(cgo, gpu_ctx, cases[0])
    one = both(cgo, gpu_ctx, cases)
    assert one.launches == 1 and all(r.iters_ran == 24 for r in one)
    for c, got in zip(cases, one):
        assert_bar(got, oracle_of(c), c.name)
    launches = []
    for s in (1, 3):
        sliced = run(cgo, gpu_ctx, cases, "lds", slice_iters=s)
        assert sliced.rows == "lds" and sliced.handed_back == 0
        for b, (x, y) in enumerate(zip(sliced, one)):
            same_bits(x, y, f"slice_iters {s} problem {b}")
        launches.append(sliced.launches)
    assert launches[0] > launches[1] > 1


# ---- 5. mixed outcomes ----------------------------------------------------------------------------------------------------------------
def test_mixed_outcomes_have_the_device_tiers_pattern(cgo, gpu_ctx):
    for cases, expect, handed in ((Q.mixed_quad(), [("success", 1), ("success", 0), ("success", 21)], 0),
                                  (Q.mixed_rosen(), [("max_iters_reached", 8), ("zoom_max_iters_reached", 3)], 1),
                                  (Q.mixed_quad(2), [("zoom_max_iters_reached", 0), ("zoom_max_iters_reached", 0), ("success", 1), ("success", 0)], 2)):
        out = both(cgo, gpu_ctx, cases)
        assert [(r.status, r.iters_ran) for r in out] == expect and out.handed_back == handed
        for c, got in zip(cases, out):
            assert_bar(got, oracle_of(c), c.name)
    for s in (1, 3):   # a hand-back in a later launch: the slices before it wrote their rows back
        same_batch(run(cgo, gpu_ctx, Q.mixed_rosen(), "lds", slice_iters=s), run(cgo, gpu_ctx, Q.mixed_rosen(), "device", slice_iters=s))


# ---- 6. isolation -----------------------------------------------------------------------------------------------------------------------
def test_rows_do_not_see_one_another(cgo, gpu_ctx):
    cases = Q.rows_batch()
    n = cases[0].n
    alone = [run(cgo, gpu_ctx, [c], "lds")[0] for c in cases]
    other = list(cases)
    other[1] = dataclasses.replace(cases[1], x0=np.full(n, np.nan))
    other[3] = dataclasses.replace(cases[3], D=np.full(n, np.nan))
    poisoned = run(cgo, gpu_ctx, other, "lds")
    for b in (0, 2):
        same_bits(poisoned[b], alone[b], f"problem {b} beside NaN neighbours")
    assert not math.isfinite(poisoned[1].objective) or not np.all(np.isfinite(poisoned[1].minimizer))
    same_batch(poisoned, run(cgo, gpu_ctx, other, "device"))


# ---- 7. run-time compiled objectives --------------------------------------------------------------------------------------------------
def solve_user(cgo, ctx, model, probs, rows, slice_iters=0):
    p0 = probs[0]
    _, _, cfg, ls = _product_structs(p0.case())
    k = U.SOURCES[p0.name][1]
    X0 = np.stack([p.x0 for p in probs])
    params = [np.stack([p.slots[j] for p in probs]) for j in range(k)]
    scalars = None if p0.s0 is None else np.array([p.s0 for p in probs])
    return cgo.minimizeobjectivebatch_lbfgs_obj(model, X0, cfg, ls, params=params, scalars=scalars, ctx=ctx, slice_iters=slice_iters, rows=rows)


@pytest.mark.parametrize("name", ["H2", "Q4", "SM", "R0"])
def test_run_time_compiled_objectives(cgo, gpu_ctx, name):
    """K = 2, K = 4, K = 3 with a scalar per problem, and K = 0 (the struct that restates paired Rosenbrock), m = 5, at n = 1000
    clamped to what the LDS holds for that K: one source compiled once, one program of the tier"""
    src, k = U.SOURCES[name]
    m = 5
    probe_model = cgo.ElementwiseObjective(4, src, param=None if k == 0 else (np.ones(4) if k == 1 else [None] * k), ctx=gpu_ctx)
    try:
        top = cgo.batch_lbfgs_max_n_obj(probe_model, m=m, rows="lds")
        assert cgo.batch_lbfgs_max_n_obj(probe_model, m=m, rows="auto") == cgo.batch_lbfgs_max_n_obj(probe_model) > 2 ** 31
        n = min(1000, top)
        assert top % 2 == 0 and n // 2 > Q.BLOCK and (n // 2) % Q.BLOCK != 0, (top, n)   # a whole block of pairs and a partial one
        rows = cgo.batch_lbfgs_lds_rows(k, m)
        assert 8 * rows * top <= 160 * 1024 - 512 - 7000 < 8 * rows * (top + 2) + 2048
        kw = dict(c2=0.5, eps=1e-9, max_iters=8)
        if name == "R0":
            cases = [Q.rosen(n, b, m, max_iters=8) for b in range(3)]
            probs = [U.Prob("R0", n, b, m, dict(c2=c.c2, max_iters=c.max_iters), slots=(), x0=c.x0) for b, c in enumerate(cases)]
        elif name == "SM":
            probs = [U.Prob(name, n, b, m, kw, s0=U.SCALARS[b]) for b in range(3)]
        else:
            probs = [U.Prob(name, n, b, m, kw) for b in range(3)]
        model = cgo.ElementwiseObjective(n, src, param=None if k == 0 else (np.ones(n) if k == 1 else [None] * k), ctx=gpu_ctx)
        try:
            lds, dev = solve_user(cgo, gpu_ctx, model, probs, "lds"), solve_user(cgo, gpu_ctx, model, probs, "device")
            assert lds.rows == "lds" and dev.rows == "device" and all(r.iters_ran > 0 for r in lds)
            same_batch(lds, dev, name)
            same_batch(solve_user(cgo, gpu_ctx, model, probs, "lds", slice_iters=3), solve_user(cgo, gpu_ctx, model, probs, "device", slice_iters=3), name + " sliced")
            auto = solve_user(cgo, gpu_ctx, model, probs, "auto")
            assert auto.rows == "device"       # the rule of include/cgo.h as measured
            same_batch(auto, dev, name + " auto")
            if name == "R0":
                same_batch(lds, run(cgo, gpu_ctx, cases, "lds"), "R0 against the built-in")
        finally:
            model.close()
        if top + 2 <= 4096:   # beyond the limit: refused under "lds" with the helper's name and value, device rows under "auto"
            big = cgo.ElementwiseObjective(top + 2, src, param=None if k == 0 else (np.ones(top + 2) if k == 1 else [None] * k), ctx=gpu_ctx)
            try:
                over = [U.Prob(name, top + 2, b, m, dict(c2=0.5, eps=1e-9, max_iters=2), s0=(U.SCALARS[b] if name == "SM" else None)) for b in range(2)] \
                    if name != "R0" else [U.Prob("R0", top + 2, b, m, dict(c2=0.5, max_iters=2), slots=(), x0=Q.rosen(top + 2, b, m).x0) for b in range(2)]
                with pytest.raises(cgo.CgoError, match=r"cgo_batch_lbfgs_max_n_ex = %d" % top) as e:
                    solve_user(cgo, gpu_ctx, big, over, "lds")
                assert e.value.code == 1
                assert solve_user(cgo, gpu_ctx, big, over, "auto").rows == "device"
            finally:
                big.close()
    finally:
        probe_model.close()


# ---- 8. the probe, tier 3 against tier 2 ----------------------------------------------------------------------------------------------
def probe(cgo, tier, obj, ds, script, n, **kw):
    X, Uv = _stack(ds, "x", n)[:, 0], _stack(ds, "u", n)[:, 0]
    got = cgo.batch_probe(tier, KIND[obj], X, Uv, script, params=params_of(obj, ds, n), **kw)
    assert got["ld"] == n + (n & 1) and got["points"] == 3
    return got


def same_probe(tag, a, b):
    for key in ("rows", "width", "stored", "qn", "reason", "done", "passes"):
        assert np.array_equal(a[key], b[key]), f"{tag}: {key}"
    for key in ("ts", "gu", "uu", "x", "u", "S", "Y"):
        assert np.array_equal(u64(a[key]), u64(b[key])), f"{tag}: {key}"


def probe_sizes(cgo, obj):
    block, T, _ = lds_pairs(cgo, 1 if obj is Quad else 0)
    if obj is Booth:
        return [2]
    return [2, 2 * block, 2 * (T + 1)] + ([2 * block + 1] if obj is Quad else [])


@pytest.mark.parametrize("obj", [Quad, Rosen, Booth], ids=["quad", "rosen", "booth"])
def test_probe_tier_3_has_the_bits_of_tier_2(cgo, gpu_ctx, obj):
    """R_INIT, trial (k = 3), push, combine (k = 3), a push whose candidate is dropped (a zero step: s·y = 0), combine, and a combine
    on given coefficients, with m = 10 and the ring full; then the exact s·y < 0 drop of tests/test_batch_kernel_sums.py.  Every
    row of every pass in every workgroup, every `out`, x, u, S, Y, the quasi-Newton states and the counters equal tier 2's on the
    same inputs; the padding element stays the NaN pattern (the NaN slack is checked by the library itself: CGO_ESTATE otherwise)."""
    m, c, free = 10, 10, 7
    gam, cy, cs = coefs(obj, c)
    script = [("init",), ("trial", STEPS), ("push", 0.125), ("combine", STEPS), ("push", 0.0), ("combine", STEPS[:1]), ("combine", STEPS, (c, gam, cy, cs))]
    for n in probe_sizes(cgo, obj):
        ds = [lbfgs_problem(obj, n, m, c, free, 4100 + 17 * b + n) for b in range(3)]
        kw = _lbfgs_inputs(ds, n, m)
        t3, t2 = probe(cgo, "lbfgs_lds", obj, ds, script, n, **kw), probe(cgo, "lbfgs", obj, ds, script, n, **kw)
        assert t3["symbol"] == f"k_batch_lbfgs_lds<{TNAME[obj]}, 3, true>" and t2["symbol"] == f"k_batch_lbfgs<{TNAME[obj]}, 3, true>"
        same_probe(f"{obj.name} n={n}", t3, t2)
        assert np.all(t3["done"] == 2) and np.all(t3["passes"] == len(script)) and np.all(t3["reason"] == RES_BUDGET)
        assert np.all(t3["stored"][4] == t3["stored"][2])          # the zero step was dropped: the count stays
        mism = []
        padding_intact(f"{obj.name} n={n}", t3, ("x", "u", "S", "Y"), n, mism)
        assert not mism, mism
    if obj is Booth:
        return
    for mm, cc, ff in ((4, 3, 1), (1, 1, 1)):
        n = 2 * Q.BLOCK + (1 if obj is Quad else 0)
        ds = [drop_problem(obj, n, mm, cc, ff, 700 + 31 * b) for b in range(3)]
        g2, cy2, cs2 = coefs(obj, cc)
        script2 = [("push", PUSH_A), ("combine", STEPS if obj is Quad else [], (cc, g2, cy2, cs2)), ("push", 0.0)]
        kw = _lbfgs_inputs(ds, n, mm)
        t3, t2 = probe(cgo, "lbfgs_lds", obj, ds, script2, n, **kw), probe(cgo, "lbfgs", obj, ds, script2, n, **kw)
        same_probe(f"drop {obj.name} m={mm}", t3, t2)
        assert np.all(t3["stored"][0] == cc)


def test_probe_skipped_and_unfinished_problems_are_left_alone(cgo, gpu_ctx):
    """a skipped problem's rows, ring and state keep their bits; and a script that completes no iteration (R_INIT and a trial: what a
    problem handed back at iteration 0 has run) leaves x, u and the ring in device memory as uploaded — k_batch's rule, where the
    device tier has stored u = −g by then"""
    n, m, c, free = 2 * Q.BLOCK + 1, 4, 3, 1
    ds = [lbfgs_problem(Quad, n, m, c, free, 9500 + b) for b in range(3)]
    kw = _lbfgs_inputs(ds, n, m)
    script = [("push", PUSH_A), ("trial", STEPS)]
    full, part = probe(cgo, "lbfgs_lds", Quad, ds, script, n, **kw), probe(cgo, "lbfgs_lds", Quad, ds, script, n, skip=[0, 1, 0], **kw)
    for b in (0, 2):
        assert np.array_equal(full["rows"][:, b], part["rows"][:, b])
        for key in ("x", "u", "S", "Y"):
            assert np.array_equal(u64(full[key][b]), u64(part[key][b])), key
        assert np.array_equal(full["qn"][b], part["qn"][b])
    assert part["reason"][1] == RES_STOP and part["done"][1] == 0 and part["passes"][1] == 0
    assert np.all(part["rows"][:, 1].view(np.int64) == NAN_BITS)
    for key in ("x", "u"):
        assert np.array_equal(u64(part[key][1, :n]), u64(ds[1][key])), key
    for key in ("S", "Y"):
        assert np.array_equal(u64(part[key][1, :, :n]), u64(ds[1][key])), key
    assert np.array_equal(part["qn"][1], words(ds[1]["q"])[0])
    idle = [("init",), ("trial", STEPS)]
    t3, t2 = probe(cgo, "lbfgs_lds", Quad, ds, idle, n, **kw), probe(cgo, "lbfgs", Quad, ds, idle, n, **kw)
    for key in ("rows", "width", "stored", "reason", "done", "passes", "qn"):
        assert np.array_equal(t3[key], t2[key]), key
    assert np.all(t3["done"] == 0)
    for b, d in enumerate(ds):
        assert np.array_equal(u64(t3["x"][b, :n]), u64(d["x"])) and np.array_equal(u64(t3["u"][b, :n]), u64(d["u"]))      # as uploaded
        assert np.array_equal(u64(t3["S"][b, :, :n]), u64(d["S"])) and np.array_equal(u64(t3["Y"][b, :, :n]), u64(d["Y"]))
        assert not np.array_equal(u64(t2["u"][b, :n]), u64(d["u"]))                                                         # the device tier's R_INIT stored u = −g


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------
def device_memory():
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert C.CDLL(None).hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value), int(total.value)


def test_refusals(cgo, gpu_ctx):
    from cgo_amd import _lib
    n = 8
    X0, D = np.ones((2, n)), np.ones((2, n))
    cfg = cgo.setupCGConfig(1e-9, cgo.LBFGS(4), cgo.EnableTrace(), max_iters=4)
    sw = cgo.setupStrongWolfeBisection(1e-5, 0.9)
    L = _lib.lib()

    def policy(rows):
        pol = _lib.BatchPolicyC()
        L.cgo_batch_policy_init(C.byref(pol))
        pol.rows = rows
        return pol

    def c_call(kind, X, Dv, config, ls, ctx, pol):
        Xc = np.ascontiguousarray(X, dtype=np.float64)
        Dc = None if Dv is None else np.ascontiguousarray(Dv, dtype=np.float64)
        out, cc, lc, used = _lib.BatchResultsC(), config._c(), ls._c(), C.c_int32(-1)
        rc = L.cgo_minimize_batch_lbfgs_ex(ctx._h, cgo.OBJ_KINDS[kind], Xc.shape[1], Xc.shape[0], Xc.ctypes.data_as(_lib.dp),
                                           Dc.ctypes.data_as(_lib.dp) if Dc is not None else None, C.byref(cc), C.byref(lc), 0,
                                           C.byref(pol) if pol is not None else None, C.byref(out), C.byref(used))
        return rc, out, used.value

    def refused(match, kind="quad_diag", X=X0, Dv=D, config=cfg, ls=sw, ctx=gpu_ctx):
        for rows in ("lds", "auto"):
            with pytest.raises(cgo.CgoError, match=match) as e:
                cgo.minimizeobjectivebatch_lbfgs(kind, X, config, ls, D=Dv, ctx=ctx, rows=rows)
            assert e.value.code == 1   # CGO_EINVAL
        for pol in (policy(ROWS_LDS), policy(ROWS_AUTO), policy(ROWS_DEVICE), None):   # … and through C, with the same arguments
            rc, out, _ = c_call(kind, X, Dv, config, ls, ctx, pol)
            assert rc == 1 and out.launches == 0

    for beta in (cgo.PolakRibiere(), cgo.HagerZhang(), cgo.BroydenFamily(0.5)):
        refused("cgo_minimize_batch", config=cgo.setupCGConfig(1e-9, beta, cgo.EnableTrace(), max_iters=4))
    refused("cgo_batch_lbfgs_max_m = 10", config=cgo.setupCGConfig(1e-9, cgo.LBFGS(11), cgo.EnableTrace(), max_iters=4))
    refused("Backtracking", ls=cgo.Backtracking(cgo.Armijo(1e-4), 0.5, 100, 50))
    refused("objective must be", kind="lse", Dv=None)
    refused("objective must be", kind="rosenbrock_chained", Dv=None)
    refused("batch must be", X=np.ones((0, n)), Dv=np.ones((0, n)))
    refused("even n", kind="rosenbrock_paired", X=np.ones((2, 7)), Dv=None)
    refused("n = 2", kind="booth", X=np.ones((2, 4)), Dv=None)
    refused("param0", Dv=None)
    ctx2 = cgo.Context(0)
    try:
        ctx2.set_comm_callback(0, 2, lambda send: np.concatenate([send, send]))
        refused("multi-rank", ctx=ctx2)
    finally:
        ctx2.close()
    # a policy the library does not know
    for rows in (3, -1, 7):
        rc, out, _ = c_call("quad_diag", X0, D, cfg, sw, gpu_ctx, policy(rows))
        assert rc == 1 and "cgo_batch_policy.rows" in L.cgo_last_error().decode() and out.launches == 0
        assert L.cgo_batch_lbfgs_max_n_ex(gpu_ctx._h, 0, 4, C.byref(policy(rows))) == 0
    bad = policy(ROWS_LDS)
    bad.size = 8
    rc, _, _ = c_call("quad_diag", X0, D, cfg, sw, gpu_ctx, bad)
    assert rc == 1 and "cgo_batch_policy_init" in L.cgo_last_error().decode()
    # a null policy and DEVICE are the call without one; LDS and AUTO report the tier that ran
    for pol, want in ((None, ROWS_DEVICE), (policy(ROWS_DEVICE), ROWS_DEVICE), (policy(ROWS_LDS), ROWS_LDS), (policy(ROWS_AUTO), ROWS_DEVICE)):
        rc, out, used = c_call("quad_diag", X0, D, cfg, sw, gpu_ctx, pol)
        assert rc == 0 and used == want and out.launches >= 1
    # Booth: two elements, whatever the LDS holds; kinds without a batched form: 0
    assert cgo.batch_lbfgs_max_n("booth", gpu_ctx, m=3, rows="lds") == 2 and cgo.batch_lbfgs_max_n("lse", gpu_ctx, m=3, rows="lds") == 0
    # tier 3 of the probe takes built-in objectives only
    src, k = U.SOURCES["H2"]
    model = cgo.ElementwiseObjective(n, src, param=[None] * k, ctx=gpu_ctx)
    try:
        d = [lbfgs_problem(Quad, n, 4, 3, 1, 1)]
        with pytest.raises(cgo.CgoError, match="no PROBE twin") as e:
            cgo.batch_probe("lbfgs_lds", model, d[0]["x"][None], d[0]["u"][None], [("push", 0.5)], params=[np.ones((1, n))] * k, **_lbfgs_inputs(d, n, 4))
        assert e.value.code == 1
    finally:
        model.close()
    p = _lib.BatchProbeC()
    p.tier = 4
    assert L.cgo_batch_probe(gpu_ctx._h, C.byref(p)) == 1 and "0 (LDS), 1 (device rows), 2 (L-BFGS) or 3 (L-BFGS in LDS)" in L.cgo_last_error().decode()
    # a batch of twice the free memory, of a size the LDS holds: refused before anything is allocated
    free, total = device_memory()
    vecs, nn = 3 + 1 + 2 * (4 + 1), 64
    batch = int(2 * free // (8 * nn * vecs))
    assert batch < 2 ** 31
    tiny = np.ones(16)
    out, cc, lc, used = _lib.BatchResultsC(), cfg._c(), sw._c(), C.c_int32(-1)
    pol = policy(ROWS_LDS)
    rc = L.cgo_minimize_batch_lbfgs_ex(gpu_ctx._h, cgo.OBJ_KINDS["quad_diag"], nn, batch, tiny.ctypes.data_as(_lib.dp), tiny.ctypes.data_as(_lib.dp),
                                       C.byref(cc), C.byref(lc), 0, C.byref(pol), C.byref(out), C.byref(used))
    msg = L.cgo_last_error().decode()
    print(f"free {free} of {total} bytes; refusal: {msg}")
    assert rc == 6 and "bytes of device memory" in msg   # CGO_ENOMEM
    free_after, _ = device_memory()
    assert free_after >= free - (1 << 30)   # nothing is left allocated
    small = run(cgo, gpu_ctx, [Q.quad(64, b, 4, max_iters=6) for b in range(2)], "lds")
    assert [r.status for r in small] == ["max_iters_reached"] * 2 and small.rows == "lds"
