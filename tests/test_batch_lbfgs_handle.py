"""GPU tier: cgo.BatchLBFGS / cgo_batch_lbfgs_open, _solve — a batch of L-BFGS problems that stays on the device between solves.
(CPU tier: tests/test_batch_lbfgs_handle_abi.py.)

The handle adds no arithmetic: a solve on it runs the kernels of the one-shot call (k_batch_lbfgs, k_batch_lbfgs_lds) on rows that
were uploaded once and a ring that was allocated once, for the largest m the handle may be asked for.  So the bar is EQUALITY OF
BITS with cgo.minimizeobjectivebatch_lbfgs_obj on the same inputs, rows and m — every array of every result compared as uint64
words — and that call is held to the oracle by tests/test_batch_lbfgs_user.py and tests/test_batch_lbfgs_lds.py.  What can go
wrong on a handle and not in a one-shot call: state of an earlier solve read by a later one (the ring, the QnState, the scalars,
the records), a ring laid out for m_max read with m, the dynamic LDS of the launch, an inactive problem's rows written, a
handed-back problem fed from the caller's arrays of `params`, which are the caller's again once open returns.
Problems: tests/_batch_lbfgs_user_problems.py."""
import ctypes as C
import re

import numpy as np
import pytest

import _batch_lbfgs_user_problems as U
from _cases import _product_structs

pytestmark = pytest.mark.gpu
TIERS = ("device", "lds")


# ---- the two sides -----------------------------------------------------------------------------------------------------------
def arrays(probs):
    k = U.SOURCES[probs[0].name][1]
    X0 = np.stack([p.x0 for p in probs])
    params = [np.stack([p.slots[j] for p in probs]) for j in range(k)]
    scalars = None if probs[0].s0 is None else np.array([p.s0 for p in probs])
    return X0, params, scalars


def configs(probs, m=None):
    _, _, cfg, ls = _product_structs(probs[0].case() if m is None else probs[0].with_(m=m).case())
    return cfg, ls


def model_of(cgo, ctx, probs):
    src, k = U.SOURCES[probs[0].name]
    n = probs[0].n
    return cgo.ElementwiseObjective(n, src, param=None if k == 0 else (np.ones(n) if k == 1 else [None] * k), ctx=ctx)


def one_shot(cgo, ctx, model, probs, rows, m=None, scalars="own"):
    X0, params, sc = arrays(probs)
    cfg, ls = configs(probs, m)
    out = cgo.minimizeobjectivebatch_lbfgs_obj(model, X0, cfg, ls, params=params, scalars=sc if isinstance(scalars, str) else scalars, ctx=ctx, rows=rows)
    assert out.rows == rows
    return out


def on_handle(B, probs, m=None, scalars="own", active=None):
    X0, _, sc = arrays(probs)
    cfg, ls = configs(probs, m)
    return B.solve(X0, cfg, ls, scalars=sc if isinstance(scalars, str) else scalars, active=active)


def u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_result(a, b, tag):
    assert (a.status, a.iters_ran, a.total_fdf_evals) == (b.status, b.iters_ran, b.total_fdf_evals), tag
    assert np.array_equal(u64([a.objective]), u64([b.objective])), f"{tag}: objective"
    for f in ("minimizer", "gradient"):
        assert np.array_equal(u64(getattr(a, f)), u64(getattr(b, f))), f"{tag}: {f}"
    for f in ("objective", "grad_norm", "step_size"):
        assert np.array_equal(u64(getattr(a.trace, f)), u64(getattr(b.trace, f))), f"{tag}: trace.{f}"
    assert np.array_equal(a.trace.objective_evals, b.trace.objective_evals), f"{tag}: trace.objective_evals"


def same_batch(a, b, tag=""):
    assert len(a) == len(b) and (a.rows, a.launches, a.handed_back) == (b.rows, b.launches, b.handed_back), (tag, a.rows, a.launches, a.handed_back, b.rows, b.launches, b.handed_back)
    for i, (x, y) in enumerate(zip(a, b)):
        same_result(x, y, f"{tag} problem {i}")


def batches(cgo, rows):
    """the issue's batches; the loop shapes are the tier's own (pairs per lane and trip of ITS ring passes on three slots).  The
    LDS tier takes the last shape that fits a workgroup's LDS for m = 4 and three slots — one trip and a pair, n = 514, 515 —
    where the device tier takes two trips, a partial one and a pair (n = 1538, 1539)."""
    out = {"H2-64-m4": U.distinct("H2", 64, 4), "SH-513-m5": U.scalar_batch("SH", 513, 5), "Q4-513-m10": U.four_slots(),
           "H2-64-m4-wolfe-bisection": U.distinct_wolfe_bisection(), "SM-1-m1": U.scalar_batch("SM", 1, 1)}
    block, u = cgo.batch_lbfgs_shape_obj(3) if rows == "device" else cgo.batch_lbfgs_lds_shape(3)
    for which in (0, 1, 7 if rows == "device" else 6):
        for odd in (0, 1):
            out[f"Q3-loop{which}-{'odd' if odd else 'even'}"] = U.loop_batch("Q3", block, u, which, odd)
    return out


BATCH_NAMES = ["H2-64-m4", "SH-513-m5", "Q4-513-m10", "H2-64-m4-wolfe-bisection", "SM-1-m1"] + \
              [f"Q3-loop{w}-{p}" for w in ("0", "1", "last") for p in ("even", "odd")]


def batch_named(cgo, rows, name):
    return batches(cgo, rows)[name.replace("last", "7" if rows == "device" else "6")]


# ---- 1. the handle against the one-shot call ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BATCH_NAMES)
@pytest.mark.parametrize("rows", TIERS)
def test_handle_has_the_bits_of_the_one_shot_call(cgo, gpu_ctx, rows, name):
    probs = batch_named(cgo, rows, name)
    model = model_of(cgo, gpu_ctx, probs)
    try:
        ref = one_shot(cgo, gpu_ctx, model, probs, rows)
        _, params, _ = arrays(probs)
        with cgo.BatchLBFGS(model, params, len(probs), probs[0].m, rows=rows) as B:
            assert (B.rows, B.m) == (rows, probs[0].m)
            m = C.c_int32(0)
            assert cgo.lib().cgo_batch_lbfgs_m(B._h, C.byref(m)) == 0 and m.value == probs[0].m
            first = on_handle(B, probs)
            second = on_handle(B, probs)
        same_batch(first, ref, f"{name} on {rows}")
        same_batch(second, ref, f"{name} on {rows}, solved again")
        assert all(r.iters_ran > 0 for r in ref) and ref.handed_back == 0
    finally:
        model.close()


# ---- 2. nothing of a solve reaches the next -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", TIERS)
def test_no_state_leaks_between_solves(cgo, gpu_ctx, rows):
    """A, then B — other X0, other scalars, another line search, a smaller m, no trace — then A again; and a solve without scalars
    after one with them is the model's scalar for all"""
    probs = U.scalar_batch("SH", 513, 5)
    model = model_of(cgo, gpu_ctx, probs)
    try:
        X0, params, sc = arrays(probs)
        cfg, ls = configs(probs)
        cfg_b = cgo.setupCGConfig(1e-9, cgo.LBFGS(2), cgo.DisableTrace(), max_iters=9)
        ls_b = cgo.WolfeBisection(cgo.Wolfe(1e-3, 0.9), 100, 1e12, 50)
        X0_b, sc_b = np.roll(X0, 1, axis=0) * 0.75, sc[::-1] * 3.0
        model.set_scalar(0.75)
        with cgo.BatchLBFGS(model, params, len(probs), 5, rows=rows) as B:
            a1 = B.solve(X0, cfg, ls, scalars=sc)
            b1 = B.solve(X0_b, cfg_b, ls_b, scalars=sc_b)
            a2 = B.solve(X0, cfg, ls, scalars=sc)
            none = B.solve(X0, cfg, ls)
            a3 = B.solve(X0, cfg, ls, scalars=sc)
        same_batch(a1, a2, "A after B")
        same_batch(a1, a3, "A after a solve without scalars")
        same_batch(a1, one_shot(cgo, gpu_ctx, model, probs, rows), "A")
        same_batch(b1, cgo.minimizeobjectivebatch_lbfgs_obj(model, X0_b, cfg_b, ls_b, params=params, scalars=sc_b, ctx=gpu_ctx, rows=rows), "B")
        same_batch(none, one_shot(cgo, gpu_ctx, model, probs, rows, scalars=None), "no scalars")
        same_batch(none, one_shot(cgo, gpu_ctx, model, probs, rows, scalars=np.full(len(probs), 0.75)), "no scalars = the model's scalar for all")
        assert not np.array_equal(none[1].minimizer, a1[1].minimizer)
    finally:
        model.close()


# ---- 3. active -----------------------------------------------------------------------------------------------------------------
SENTINEL = -7.25


@pytest.mark.parametrize("rows", TIERS)
def test_active_leaves_inactive_problems_alone(cgo, gpu_ctx, rows):
    from cgo_amd import _lib
    probs = U.scalar_batch("SH", 513, 5)
    batch, n = len(probs), probs[0].n
    model = model_of(cgo, gpu_ctx, probs)
    try:
        X0, params, sc = arrays(probs)
        cfg, ls = configs(probs)
        full = one_shot(cgo, gpu_ctx, model, probs, rows)
        act = np.array([1, 0, 1, 1, 0, 1], dtype=bool)
        with cgo.BatchLBFGS(model, params, batch, 5, rows=rows) as B:
            part = B.solve(X0, cfg, ls, scalars=sc, active=act)
            # … and at the ctypes level, on sentinel-filled arrays: the rows of an inactive problem are not written
            cap = cfg.max_iters
            f, it, st, ev = np.full(batch, SENTINEL), np.full(batch, -7, dtype=np.int64), np.full(batch, -7, dtype=np.int32), np.full(batch, -7, dtype=np.int64)
            x, g = np.full((batch, n), SENTINEL), np.full((batch, n), SENTINEL)
            to, tg, ts = (np.full((batch, cap), SENTINEL) for _ in range(3))
            te = np.full((batch, cap), -7, dtype=np.int64)
            r = _lib.BatchResultsC()
            r.objective, r.iters_ran, r.status, r.total_fdf_evals = f.ctypes.data_as(_lib.dp), it.ctypes.data_as(_lib.i64p), st.ctypes.data_as(C.POINTER(C.c_int32)), ev.ctypes.data_as(_lib.i64p)
            r.minimizer, r.gradient = x.ctypes.data_as(_lib.dp), g.ctypes.data_as(_lib.dp)
            r.trace_objective, r.trace_grad_norm, r.trace_step_size = to.ctypes.data_as(_lib.dp), tg.ctypes.data_as(_lib.dp), ts.ctypes.data_as(_lib.dp)
            r.trace_objective_evals = te.ctypes.data_as(_lib.i64p)
            ac = act.astype(np.uint8)
            cc, lc = cfg._c(), ls._c()
            rc = cgo.lib().cgo_batch_lbfgs_solve(B._h, X0.ctypes.data_as(_lib.dp), sc.ctypes.data_as(_lib.dp), ac.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                 C.byref(cc), C.byref(lc), 0, C.byref(r))
            assert rc == 0, cgo.lib().cgo_last_error().decode()
            everything = B.solve(X0, cfg, ls, scalars=sc, active=np.ones(batch, dtype=bool))
        assert part.handed_back == 0 and part.launches == full.launches
        for b in range(batch):
            if not act[b]:
                assert part[b] is None
                assert f[b] == SENTINEL and it[b] == st[b] == ev[b] == -7 and np.all(x[b] == SENTINEL) and np.all(g[b] == SENTINEL)
                assert np.all(to[b] == SENTINEL) and np.all(tg[b] == SENTINEL) and np.all(ts[b] == SENTINEL) and np.all(te[b] == -7)
                continue
            same_result(part[b], full[b], f"active problem {b}")
            k = full[b].iters_ran
            assert np.array_equal(u64(x[b]), u64(full[b].minimizer)) and np.array_equal(u64(g[b]), u64(full[b].gradient)) and it[b] == k
            assert np.array_equal(u64(to[b, :k]), u64(full[b].trace.objective)) and np.all(to[b, k:] == SENTINEL)
        same_batch(everything, full, "all active")
    finally:
        model.close()


# ---- 4. m below m_max ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 4])
@pytest.mark.parametrize("rows", TIERS)
def test_m_below_m_max(cgo, gpu_ctx, rows, m):
    """a ring allocated for 10 pairs, strided for 11 slots, run with 1 and with 4: the bits of a one-shot call with that m — four
    slots at n = 513 (an odd tail), 12 iterations: the ring wraps"""
    probs = U.four_slots()
    model = model_of(cgo, gpu_ctx, probs)
    try:
        _, params, _ = arrays(probs)
        with cgo.BatchLBFGS(model, params, len(probs), 10, rows=rows) as B:
            got = on_handle(B, probs, m=m)
            ten = on_handle(B, probs)
            again = on_handle(B, probs, m=m)
        ref = one_shot(cgo, gpu_ctx, model, probs, rows, m=m)
        same_batch(got, ref, f"m = {m} on a handle of 10")
        same_batch(again, ref, f"m = {m} after m = 10")
        same_batch(ten, one_shot(cgo, gpu_ctx, model, probs, rows), "m = 10")
        assert not np.array_equal(ten[0].minimizer, got[0].minimizer)
    finally:
        model.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", TIERS)
def test_refusals_leave_the_handle_as_it_was(cgo, gpu_ctx, rows):
    probs = U.distinct("H2", 64, 4)
    batch = len(probs)
    model = model_of(cgo, gpu_ctx, probs)
    try:
        X0, params, _ = arrays(probs)
        cfg, ls = configs(probs)
        ref = one_shot(cgo, gpu_ctx, model, probs, rows)

        def config(beta):
            return cgo.setupCGConfig(1e-9, beta, cgo.EnableTrace(), max_iters=12)
        with cgo.BatchLBFGS(model, params, batch, 4, rows=rows) as B, cgo.Batch(model, params, batch, rows="device") as CG:
            same_batch(on_handle(B, probs), ref, "before")

            def refused(match, **kw):
                a = dict(X0=X0, config=cfg, linesearch_config=ls)
                a.update(kw)
                with pytest.raises(cgo.CgoError, match=match) as e:
                    B.solve(**a)
                assert e.value.code == 1   # CGO_EINVAL
                same_batch(on_handle(B, probs), ref, f"after the refusal of {match!r}")
            refused(r"m = 5 exceeds the m_max = 4", config=config(cgo.LBFGS(5)))
            refused(r"cgo_batch_lbfgs_max_m = 10", config=config(cgo.LBFGS(11)))
            for beta in (cgo.HagerZhang(), cgo.PolakRibiere(), cgo.BroydenFamily(0.5)):
                refused(r"CG flavours: cgo_batch_solve", config=config(beta))
            refused("Backtracking", linesearch_config=cgo.Backtracking(cgo.Armijo(1e-4), 0.5, 100, 50))
            refused(r"batched solves: scalars\[1\] is not finite", scalars=np.array([1.0, np.nan, 1.0, 1.0]))
            refused(r"batched solves: scalars\[3\] is not finite", scalars=np.array([1.0, 2.0, 1.0, np.inf]))
            refused("batched solves: active selects no problem", active=np.zeros(batch, dtype=bool))
            refused("slice_iters must be", slice_iters=-1)
            # the two kinds of handle do not mix
            from cgo_amd import _lib
            out, cc, lc = _lib.BatchResultsC(), cfg._c(), ls._c()
            out.launches = 7
            cg_cfg = config(cgo.HagerZhang())._c()
            assert cgo.lib().cgo_batch_solve(B._h, X0.ctypes.data_as(_lib.dp), None, None, C.byref(cg_cfg), C.byref(lc), 0, C.byref(out)) == 1
            assert "opened for L-BFGS: cgo_batch_lbfgs_solve" in cgo.lib().cgo_last_error().decode() and out.launches == 0
            out.launches = 7
            assert cgo.lib().cgo_batch_lbfgs_solve(CG._h, X0.ctypes.data_as(_lib.dp), None, None, C.byref(cc), C.byref(lc), 0, C.byref(out)) == 1
            assert "cgo_batch_solve" in cgo.lib().cgo_last_error().decode() and out.launches == 0
            m = C.c_int32(-1)
            assert cgo.lib().cgo_batch_lbfgs_m(CG._h, C.byref(m)) == 0 and m.value == 0
            with pytest.raises(cgo.CgoError, match="L-BFGS"):   # the CG handle refuses LBFGS in its own words, as before
                CG.solve(X0, cfg, ls)
            same_batch(on_handle(B, probs), ref, "after the other kind of handle")
            assert all(r.iters_ran > 0 for r in CG.solve(X0, config(cgo.HagerZhang()), ls))   # … and runs what it ran
        # open: m_max outside 1 … 10, and what the one-shot call refuses of params
        for m_max in (0, 11, -3):
            with pytest.raises(cgo.CgoError, match=r"m_max = %d lies outside 1 … cgo_batch_lbfgs_max_m = 10" % m_max) as e:
                cgo.BatchLBFGS(model, params, batch, m_max, rows=rows)
            assert e.value.code == 1
        with pytest.raises(cgo.CgoError, match="n_params = 1"):
            cgo.BatchLBFGS(model, params[:1], batch, 4, rows=rows)
        quad = cgo.QuadDiag(np.ones(64), ctx=gpu_ctx)
        try:
            with pytest.raises(ValueError, match="run-time compiled"):
                cgo.BatchLBFGS(quad, [], batch, 4, rows=rows)
        finally:
            quad.close()
    finally:
        model.close()


def test_lds_handle_is_refused_above_what_the_lds_holds_for_m_max(cgo, gpu_ctx):
    """the limit is m_max's, not the m of a solve: n fits for m = 1 and not for m = 10"""
    src, k = U.SOURCES["H2"]
    probe = cgo.ElementwiseObjective(4, src, param=[None] * k, ctx=gpu_ctx)
    try:
        top10, top1 = cgo.batch_lbfgs_max_n_obj(probe, m=10, rows="lds"), cgo.batch_lbfgs_max_n_obj(probe, m=1, rows="lds")
    finally:
        probe.close()
    n = top10 + 2
    assert 0 < top10 < n <= top1
    model = cgo.ElementwiseObjective(n, src, param=[None] * k, ctx=gpu_ctx)
    try:
        P = [np.ones((2, n)), np.full((2, n), 0.5)]
        with pytest.raises(cgo.CgoError, match=r"cgo_batch_lbfgs_max_n_obj_ex = %d" % top10) as e:
            cgo.BatchLBFGS(model, P, 2, 10, rows="lds")
        assert e.value.code == 1
        with cgo.BatchLBFGS(model, P, 2, 1, rows="lds") as B:
            assert B.rows == "lds"
        with cgo.BatchLBFGS(model, P, 2, 10, rows="auto") as B:
            assert B.rows == "device"   # the rule of include/cgo.h
    finally:
        model.close()


# ---- 6. hand-back --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["H2", "SH"])
@pytest.mark.parametrize("rows", TIERS)
def test_hand_back_reads_the_handles_rows_not_the_callers(cgo, gpu_ctx, rows, which):
    """mixed_h2 (six problems, two slots; five are handed back) and mixed_sh (the same with a scalar each): the arrays given to
    open are overwritten with NaN once it returns, so a hand-back fed from them would end in NaN.  H2 ends as
    MIXED_H2_EXPECT; under the scalars HANDBACK_SCALARS the problems whose scalar is exactly 1.0 (0, 2, 4) do, and all six end as the
    one-shot call ends them."""
    probs = U.mixed_h2() if which == "H2" else U.mixed_sh()
    model = model_of(cgo, gpu_ctx, probs)
    try:
        ref = one_shot(cgo, gpu_ctx, model, probs, rows)
        got_expect = [(r.status, r.iters_ran) for r in ref]
        for b in range(6) if which == "H2" else (0, 2, 4):
            assert got_expect[b] == U.MIXED_H2_EXPECT[b], (b, got_expect[b])
        assert ref.handed_back == sum(s not in ("success", "max_iters_reached") for s, _ in got_expect) >= 3
        _, params, _ = arrays(probs)
        mine = [np.array(v) for v in params]
        with cgo.BatchLBFGS(model, mine, len(probs), 4, rows=rows) as B:
            for v in mine:
                v[:] = np.nan
            got = on_handle(B, probs)
            again = on_handle(B, probs)
        print(f"{which} on {rows}: handed_back {got.handed_back} of {len(probs)}: {got_expect}")
        assert got.handed_back == ref.handed_back
        same_batch(got, ref, f"{which} on {rows}")
        same_batch(again, ref, f"{which} on {rows}, solved again")
        assert all(np.all(np.isfinite(r.minimizer)) for r in got)
    finally:
        model.close()


# ---- 7. memory -----------------------------------------------------------------------------------------------------------------------
def test_a_ring_beyond_free_memory_is_refused_before_anything_is_allocated(cgo, gpu_ctx):
    """sized from what the device reports free: (3 + 0 + 2·(10+1)) vectors of batch · n doubles at 1.5 times that.  (The model is
    R0, no slots: a model WITH slots of that size would itself allocate them.)"""
    import torch
    free, total = torch.cuda.mem_get_info(0)
    batch, vecs = 8, 3 + 0 + 2 * (10 + 1)
    n_big = int(1.5 * free // (8 * batch * vecs)) & ~1
    src, _ = U.SOURCES["R0"]
    big = cgo.ElementwiseObjective(n_big, src, ctx=gpu_ctx)
    try:
        assert n_big < cgo.batch_lbfgs_max_n_obj(big)
        with pytest.raises(cgo.CgoError, match="bytes of device memory") as e:
            cgo.BatchLBFGS(big, [], batch, 10)
        msg = str(e.value)
    finally:
        big.close()
    free_after, _ = torch.cuda.mem_get_info(0)
    print(f"free {free} of {total} bytes, {free_after} afterwards; refusal: {msg}")
    assert e.value.code == 6   # CGO_ENOMEM
    assert re.search(r"m = 10", msg) and f"{float(vecs) * batch * n_big * 8:.0f}"[:6] in msg
    assert free_after >= free - (1 << 30)   # nothing is left allocated
