"""CPU tier of the batched L-BFGS solves (tests/test_batch_lbfgs.py is the GPU tier): the exported symbols and the table row;
the scalar recursion of csrc/cgo_qn.hpp against a numpy two-loop recursion on explicit vectors; the device loop
res_iterate_qn (csrc/cgo_resident_qn.hpp) over plain loops (tests/hostsim/sim_batch_lbfgs.cpp, compiled here) against the
oracle at the GPU tier's bar; and, for EVERY problem the GPU tier uses, that the reference's two restatements (run_oracle,
run_numpy) agree to a tenth of that bar — the bar means something only where the reference itself is that well determined."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _batch_lbfgs_problems as Q
import _instances as I
from _cases import Out, _product_structs, rel, relf, run_numpy, run_oracle
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cgo_minimize_batch_lbfgs": 10, "cgo_batch_lbfgs_max_m": 0, "cgo_batch_lbfgs_max_n": 2, "cgo_batch_lbfgs_shape": 2}
MAX_M = 10


# ---- 1. the interface -----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_refuse_null_arguments(cgo):
    from cgo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cgo.h"), encoding="utf-8").read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    L = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name, nargs in NEW.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and getattr(L, name), name
        proto = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", flat)
        args = proto.group(1).strip()
        assert (0 if args in ("", "void") else len(args.split(","))) == nargs, name
        assert name in exported, name
    assert L.cgo_batch_lbfgs_max_m() == MAX_M == cgo.batch_lbfgs_max_m()
    assert L.cgo_minimize_batch_lbfgs(None, 0, 8, 2, None, None, None, None, 0, None) == 1
    assert "null argument" in L.cgo_last_error().decode()
    assert L.cgo_batch_lbfgs_max_n(None, 0) == 0
    L.cgo_batch_lbfgs_shape(None, None)   # as free(NULL)
    block, u = cgo.batch_lbfgs_shape()    # needs no device
    src = open(os.path.join(I.CSRC, "cgo_kernels_batch_lbfgs.hip.hpp")).read()
    assert block == Q.BLOCK and u == int(re.search(r"^#define CGO_BATCH_LBFGS_U (\d+)", src, re.M).group(1)) and 1 <= u <= 4
    for name in ("minimizeobjectivebatch_lbfgs", "batch_lbfgs_max_n"):
        assert callable(getattr(cgo, name))
        jl = open(os.path.join(ROOT, "conjugategradientoptim.jl_amd", "julia", "ConjugateGradientOptimAMD.jl"), encoding="utf-8").read()
        assert re.search(r"^(?:function )?" + name + r"\(", jl, re.M), name


def test_the_table_row_and_the_translation_units():
    assert I.rows("BATCH_LBFGS") == [(3,)]
    assert I.rows("BATCH") == [(3,)] and I.rows("BATCH_DEVROWS") == [(3,)]   # as they were
    tu = open(os.path.join(I.CSRC, "cgo_backend_batch_lbfgs.hip")).read()
    assert "CGO_BATCH_LBFGS_ROWS(ROW)" in tu and "k_batch_lbfgs<Obj, NPTS>" in tu
    assert "row_pick_for<BatchLbfgsRows>(obj_kind, npts)" in tu and "CGO_OBJ_ROWS(ROW)" in open(os.path.join(I.CSRC, "cgo_backend_internal.hpp")).read()   # (the switch over the objectives: once, for every tier)
    for other in ("cgo_backend_batch.hip", "cgo_backend_batch_rows.hip", "cgo_rtc.hip"):
        text = open(os.path.join(I.CSRC, other)).read()
        assert "cgo_kernels_batch_lbfgs.hip.hpp" not in text and "k_batch_lbfgs<" not in text, other
    # (the one unit of the module's further programs holds this tier's program too: no OTHER program lists the kernel)
    assert "k_batch_lbfgs<" not in open(os.path.join(I.CSRC, "cgo_rtc_batch.hip")).read()
    for prog in ("RTC_RESIDENT_PROBE", "RTC_BATCH", "RTC_BATCH_ROWS", "RTC_BATCH_PROBE"):
        assert not [k for k in I.rtc_program_kernels(prog) if k.startswith("k_batch_lbfgs")] and I.rtc_programs()[prog][2] == "RTC_TEXT_BASE", prog
    # the loop lives in a header of its own: the text of the run-time compiled modules does not carry it
    assert "res_iterate_qn" not in open(os.path.join(I.CSRC, "cgo_resident.hpp")).read()
    gen = open(os.path.join(I.CSRC, "gen_rtc_sources.py")).read()
    assert "cgo_resident_qn.hpp" not in gen and "cgo_qn.hpp" not in gen and "cgo_kernels_batch_lbfgs" not in gen
    code = re.sub(r"//.*", "", open(os.path.join(I.CSRC, "cgo_kernels_batch_lbfgs.hip.hpp")).read())
    assert "extern __shared__" not in code and "atomic" not in code and "__threadfence" not in code


def test_embedded_kernel_sources_do_not_see_the_new_declarations(tmp_path):
    import sys
    out = tmp_path / "cgo_rtc_sources.inc"
    subprocess.run([sys.executable, os.path.join(I.CSRC, "gen_rtc_sources.py"), str(out)], check=True)
    text = out.read_text(encoding="utf-8")
    assert "lbfgs_max_m" not in text and "CGO_HOST_ONLY" not in text and "cgo_batch_rows_shape" in text and "cgo_stop_status" in text


def test_python_arguments_are_checked_before_any_library_call(cgo, monkeypatch):
    from cgo_amd import _lib
    cfg = cgo.setupCGConfig(1e-9, cgo.LBFGS(4), cgo.EnableTrace(), max_iters=4)
    ls = cgo.setupStrongWolfeBisection(1e-5, 0.9)

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", no_library)
    model = cgo.DeviceObjective.__new__(cgo.DeviceObjective)
    with pytest.raises(ValueError, match="unknown objective kind"):
        cgo.minimizeobjectivebatch_lbfgs(model, np.ones((2, 8)), cfg, ls)
    with pytest.raises(ValueError, match="unknown objective kind"):
        cgo.minimizeobjectivebatch_lbfgs("cubic", np.ones((2, 8)), cfg, ls)
    with pytest.raises(ValueError, match=r"\[batch, n\]"):
        cgo.minimizeobjectivebatch_lbfgs("quad_diag", np.ones(8), cfg, ls, D=np.ones(8))
    with pytest.raises(ValueError, match="shape of X0"):
        cgo.minimizeobjectivebatch_lbfgs("quad_diag", np.ones((2, 8)), cfg, ls, D=np.ones((2, 7)))
    with pytest.raises(ValueError, match="unknown objective kind"):
        cgo.batch_lbfgs_max_n("cubic")


# ---- 2. the test double ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def simq(cgo, tmp_path_factory):
    from cgo_amd import _lib
    so = tmp_path_factory.mktemp("simq") / "libsim_batch_lbfgs.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unknown-pragmas", "-shared",
                    "-o", str(so), os.path.join(ROOT, "tests", "hostsim", "sim_batch_lbfgs.cpp")], check=True)
    L = C.CDLL(str(so))
    dp, i64p, i32p = _lib.dp, _lib.i64p, C.POINTER(C.c_int32)
    L.simq_solve.restype = C.c_int
    L.simq_solve.argtypes = [C.c_int, C.c_int64, dp, dp, C.POINTER(_lib.CGConfigC), C.POINTER(_lib.LSConfigC), C.c_int64, dp, dp, dp, i64p, i32p,
                             i64p, dp, dp, dp, i64p, i64p, i32p]
    L.simq_ring.restype = C.c_int
    L.simq_ring.argtypes = [C.c_int, C.c_int64, C.c_int, dp, dp, dp, i32p, i32p, i32p, dp, dp, dp, i32p]
    return L


def run_double(L, c, slice_iters=0):
    """the case through res_iterate_qn over plain loops → (Out, slices, handed)"""
    _, _lib, cfg, ls = _product_structs(c)
    dp, i64p = _lib.dp, _lib.i64p
    cap = max(c.max_iters, 1)
    x0 = np.ascontiguousarray(c.x0, dtype=np.float64)
    D = np.ascontiguousarray(c.D) if c.D is not None else None
    x, g, f = np.zeros(c.n), np.zeros(c.n), C.c_double(0)
    it, st, ev, sl, hb = C.c_int64(0), C.c_int32(-1), C.c_int64(0), C.c_int64(0), C.c_int32(0)
    to, tg, ts, te = np.zeros(cap), np.zeros(cap), np.zeros(cap), np.zeros(cap, dtype=np.int64)
    cc, lc = cfg._c(), ls._c()
    kind = {"quad_diag": 0, "rosenbrock_paired": 1, "booth": 2}[c.objective]
    rc = L.simq_solve(kind, c.n, x0.ctypes.data_as(dp), D.ctypes.data_as(dp) if D is not None else None, C.byref(cc), C.byref(lc), slice_iters,
                      x.ctypes.data_as(dp), g.ctypes.data_as(dp), C.byref(f), C.byref(it), C.byref(st), C.byref(ev), to.ctypes.data_as(dp),
                      tg.ctypes.data_as(dp), ts.ctypes.data_as(dp), te.ctypes.data_as(i64p), C.byref(sl), C.byref(hb))
    assert rc == 0
    k = int(it.value)
    e = np.zeros(0)
    out = Out(f.value, x, g, k, O.STATUS_NAMES[st.value] if not hb.value else "handed_back", to[:k], tg[:k], ts[:k], te[:k], e, e, e, int(ev.value))
    return out, int(sl.value), bool(hb.value)


def figures(got, ref):
    figs = {"minimizer": rel(got.minimizer, ref.minimizer), "objective": relf(got.objective, ref.objective), "gradient": rel(got.gradient, ref.gradient)}
    if abs(got.objective - ref.objective) <= 1e-290:
        figs["objective"] = 0.0
    if len(ref.trace_objective):
        figs["trace.objective"] = float(np.max(np.abs(got.trace_objective - ref.trace_objective) / np.maximum(np.abs(ref.trace_objective), 1e-300)))
        figs["trace.grad_norm"] = float(np.max(np.abs(got.trace_grad_norm - ref.trace_grad_norm) / np.maximum(np.abs(ref.trace_grad_norm), 1e-300)))
    return figs


def held(got, ref, name, scale=1.0):
    """tests/test_batch.py's assert_bar on `Out`s; scale = 0.1: a tenth of it"""
    assert got.status == ref.status, f"{name}: status {got.status} vs {ref.status}"
    assert got.iters_ran == ref.iters_ran, f"{name}: iters_ran {got.iters_ran} vs {ref.iters_ran}"
    assert np.array_equal(got.trace_objective_evals, ref.trace_objective_evals), f"{name}: evaluations per iteration differ"
    assert np.array_equal(got.trace_step_size, ref.trace_step_size), f"{name}: accepted steps differ"
    figs = figures(got, ref)
    for k, v in figs.items():
        assert v <= scale * (1e-9 if k == "gradient" else 1e-10), f"{name}: {k} rel diff {v:.3e}"
    return figs


_REF = {}


def refs(c):
    """(run_oracle, run_numpy) once per distinct problem"""
    key = (c.objective, c.n, c.x0.tobytes(), None if c.D is None else c.D.tobytes(), c.beta, c.m, c.ls, c.cond, c.c1, c.c2, c.eps, c.max_iters,
           c.zoom_max_iters, c.ls_max_iters)
    if key not in _REF:
        _REF[key] = (run_oracle(c), run_numpy(c))
    return _REF[key]


def every_batch(cgo):
    block, u = cgo.batch_lbfgs_shape()
    return Q.all_batches(block, u)


def test_problems_of_a_batch_are_pairwise_distinct(cgo):
    for batch in every_batch(cgo) + [Q.many_batch()]:
        keys = {(c.x0.tobytes(), None if c.D is None else c.D.tobytes()) for c in batch}
        assert len(keys) == len(batch), batch[0].name
        assert len({(c.objective, c.n, c.m, c.ls, c.c1, c.c2, c.eps, c.max_iters, c.zoom_max_iters) for c in batch}) == 1


def test_reference_restatements_agree_to_a_tenth_of_the_bar_on_every_gpu_problem(cgo):
    worst = {}
    for batch in every_batch(cgo):
        for c in batch:
            ref, alt = refs(c)
            for k, v in held(alt, ref, c.name, scale=0.1).items():
                if v > worst.get(k, (0.0, ""))[0]:
                    worst[k] = (v, c.name)
    print("run_numpy against run_oracle, worst: " + ", ".join(f"{k} {v:.1e} ({n})" for k, (v, n) in worst.items()))


def test_what_the_reference_does_with_the_mixed_batches(cgo):
    q = [refs(c)[0] for c in Q.mixed_quad()]
    assert [(r.status, r.iters_ran) for r in q] == [("success", 1), ("success", 0), ("success", 21)]
    z = [refs(c)[0] for c in Q.mixed_quad(2)]
    print("zoom_max_iters = 2:", [(r.status, r.iters_ran) for r in z])
    assert [(r.status, r.iters_ran) for r in z] == [("zoom_max_iters_reached", 0), ("zoom_max_iters_reached", 0), ("success", 1), ("success", 0)]
    r7, r8 = [refs(c)[0] for c in Q.mixed_rosen()]
    assert (r7.status, r7.iters_ran) == ("max_iters_reached", 8)
    print("seed 8:", r8.status, r8.iters_ran, r8.trace_objective_evals, r8.total_fdf_evals)
    assert (r8.status, r8.iters_ran) == ("zoom_max_iters_reached", 3)   # a hand-back MID-solve


def test_device_loop_over_plain_loops_meets_the_bar(cgo, simq):
    handed = 0
    for batch in every_batch(cgo):
        for c in batch:
            ref = refs(c)[0]
            got, _, hb = run_double(simq, c)
            if ref.status in ("success", "max_iters_reached"):
                assert not hb, c.name
                held(got, ref, c.name)
            else:   # the device loop gives such a problem back, before the iteration the reference stops in
                assert hb and got.iters_ran == ref.iters_ran, c.name
                handed += 1
    assert handed >= 2


def test_slices_of_the_device_loop_are_bit_for_bit_the_unsliced_run(cgo, simq):
    for batch in (Q.distinct_batches()[4], Q.distinct_batches()[-3], Q.wrap_batch(), Q.mixed_quad()):
        for c in batch[:2]:
            whole, n0, _ = run_double(simq, c)
            for sl in (1, 3):
                part, ns, _ = run_double(simq, c, sl)
                assert ns > n0 if whole.iters_ran > sl else ns >= n0
                assert (part.objective, part.iters_ran, part.status, part.total_fdf_evals) == (whole.objective, whole.iters_ran, whole.status, whole.total_fdf_evals)
                for f in ("minimizer", "gradient", "trace_objective", "trace_grad_norm", "trace_step_size", "trace_objective_evals"):
                    assert np.array_equal(getattr(part, f), getattr(whole, f)), (c.name, sl, f)


# ---- 3. the scalar recursion against a numpy two-loop recursion ---------------------------------------------------------------------
def two_loop(pairs, g):
    """Nocedal & Wright Alg. 7.4 on vectors.  pairs: (s, y) newest → oldest.  Returns u = −H·g and the coefficients of
    u = −γ·g + Σ cy_k·y_k + Σ cs_k·s_k."""
    if not pairs:
        return -g, 1.0, [], []
    q = g.copy()
    rho = [1.0 / float(s @ y) for s, y in pairs]
    alpha = []
    for (s, y), r in zip(pairs, rho):
        a = r * float(s @ q)
        alpha.append(a)
        q = q - a * y
    s0, y0 = pairs[0]
    gamma = float(s0 @ y0) / float(y0 @ y0)
    r_ = gamma * q
    cc = [0.0] * len(pairs)
    for k in range(len(pairs) - 1, -1, -1):
        s, y = pairs[k]
        b = rho[k] * float(y @ r_)
        cc[k] = alpha[k] - b
        r_ = r_ + cc[k] * s
    return -r_, gamma, [gamma * a for a in alpha], [-c for c in cc]


@pytest.mark.parametrize("m", [1, 4, 10])
def test_ring_and_recursion_against_numpy_two_loop(cgo, simq, m):
    from cgo_amd import _lib
    n, npush = 40, 2 * (m + 1) + 3   # the ring of m + 1 slots wraps twice
    rng = np.random.default_rng(100 + m)
    S = rng.standard_normal((npush, n))
    Y = S * (0.5 + rng.random((npush, n))) + 0.05 * rng.standard_normal((npush, n))
    G = rng.standard_normal((npush, n))
    drop = m + 2   # one candidate with s·y ≤ 0, after the ring has filled
    Y[drop] = -Y[drop]
    assert float(S[drop] @ Y[drop]) < 0 and all(float(S[t] @ Y[t]) > 0 for t in range(npush) if t != drop)
    dp, i32p = _lib.dp, C.POINTER(C.c_int32)
    kept, count, slot_of = (np.zeros(npush, dtype=np.int32) for _ in range(3))
    lst = np.zeros((npush, MAX_M), dtype=np.int32)
    gamma, cy, cs = np.zeros(npush), np.zeros((npush, MAX_M)), np.zeros((npush, MAX_M))
    assert simq.simq_ring(m, n, npush, S.ctypes.data_as(dp), Y.ctypes.data_as(dp), G.ctypes.data_as(dp), kept.ctypes.data_as(i32p),
                          count.ctypes.data_as(i32p), lst.ctypes.data_as(i32p), gamma.ctypes.data_as(dp), cy.ctypes.data_as(dp),
                          cs.ctypes.data_as(dp), slot_of.ctypes.data_as(i32p)) == 0
    stored = []   # candidate numbers, newest → oldest
    for t in range(npush):
        before = list(stored)
        if t != drop:
            stored = ([t] + stored)[:m]
        assert kept[t] == (t != drop) and count[t] == len(stored)
        # the slot list names the slots the stored candidates were written to — and a dropped candidate disturbed none of them
        assert [int(v) for v in lst[t, :count[t]]] == [int(slot_of[j]) for j in stored]
        assert slot_of[t] not in [int(slot_of[j]) for j in before[:m]] and 0 <= slot_of[t] <= m
        if t == drop:
            assert stored == before
        pairs = [(S[j], Y[j]) for j in stored]
        u_ref, g_ref, cy_ref, cs_ref = two_loop(pairs, G[t])
        assert gamma[t] == pytest.approx(g_ref, rel=1e-13)
        scale = max(np.max(np.abs(cy_ref)), np.max(np.abs(cs_ref)))
        assert np.max(np.abs(cy[t, :count[t]] - cy_ref)) <= 1e-13 * scale and np.max(np.abs(cs[t, :count[t]] - cs_ref)) <= 1e-13 * scale
        assert not cy[t, count[t]:].any() and not cs[t, count[t]:].any()
        u = -gamma[t] * G[t] + sum(cy[t, k] * Y[j] for k, j in enumerate(stored)) + sum(cs[t, k] * S[j] for k, j in enumerate(stored))
        assert rel(u, u_ref) <= 1e-12
    assert simq.simq_state_bytes() <= 2304   # ≈ 2.2 KB at m = 10: it lives in LDS during a launch
    with_wrap = [int(slot_of[t]) for t in range(npush)]
    assert with_wrap.count(with_wrap[0]) >= 2   # slot reuse: the ring wrapped
