"""CPU tier of the batched L-BFGS solves on run-time compiled objectives (tests/test_batch_lbfgs_user.py is the GPU tier): the
three entry points, the generated text of the fifth program, the Python argument checks, and — for EVERY problem the GPU tier
uses — that the reference's two restatements (run_oracle, run_numpy) agree bitwise on status, iterations, steps and evaluations
and within 1e-11 on x, f, ∇f/10 and the trace: a tenth of the GPU tier's bar."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _batch_lbfgs_user_problems as U
import _instances as I
from _cases import run_numpy, run_oracle
from test_batch_lbfgs_abi import held

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cgo_minimize_batch_lbfgs_obj": 11, "cgo_batch_lbfgs_max_n_obj": 1, "cgo_batch_lbfgs_shape_obj": 3}


# ---- 1. the interface -----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_host_only_exported_and_refuse_null_arguments(cgo):
    from cgo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cgo.h"), encoding="utf-8").read()
    host_only = "".join(re.findall(r"^/\* CGO_HOST_ONLY_BEGIN.*?^/\* CGO_HOST_ONLY_END \*/\n", hdr, flags=re.M | re.S))
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", host_only, flags=re.S))
    L = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name, nargs in NEW.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and getattr(L, name), name
        proto = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", flat)
        assert proto, f"{name} is not declared between the host-only markers"
        assert len(proto.group(1).strip().split(",")) == nargs, name
        assert name in exported, name
    assert L.cgo_minimize_batch_lbfgs_obj(None, None, 2, None, None, 0, None, None, None, 0, None) == 1
    assert "null argument" in L.cgo_last_error().decode()
    assert L.cgo_batch_lbfgs_max_n_obj(None) == 0
    L.cgo_batch_lbfgs_shape_obj(2, None, None)   # as free(NULL)
    jl = open(os.path.join(ROOT, "conjugategradientoptim.jl_amd", "julia", "ConjugateGradientOptimAMD.jl"), encoding="utf-8").read()
    for name in ("minimizeobjectivebatch_lbfgs_obj", "batch_lbfgs_max_n_obj", "batch_lbfgs_shape_obj"):
        assert callable(getattr(cgo, name))
        assert re.search(r"^(?:function )?" + name + r"\(", jl, re.M), name
        assert f":cgo_{'minimize_batch_lbfgs_obj' if name.startswith('minimize') else name}" in jl


def test_the_shape_needs_no_device_and_follows_the_slot_count(cgo):
    src = open(os.path.join(I.CSRC, "cgo_kernels_batch_lbfgs.hip.hpp")).read()
    u_max = int(re.search(r"^#define CGO_BATCH_LBFGS_U (\d+)", src, re.M).group(1))
    u_slots = int(re.search(r"^#define CGO_BATCH_LBFGS_U_SLOTS (\d+)", src, re.M).group(1))
    assert cgo.batch_lbfgs_shape() == (U.BLOCK, u_max)   # as it was
    for k in range(5):
        block, u = cgo.batch_lbfgs_shape_obj(k)
        assert block == U.BLOCK and 1 <= u <= u_max
        assert u == (u_max if k <= 1 else u_slots)
    # every ring pass takes its pairs per trip from the objective — the tier hands batch_lbfgs_u<Obj>() to the one template of
    # the ring passes, whose body names no constant of its own — and the header says why no bit depends on it
    code = re.sub(r"//.*", "", src)
    assert code.count("batch_lbfgs_u<Obj>()") == 1 and "constexpr int U = BATCH_LBFGS_U;" not in code
    assert re.search(r"using LbfgsDev = LbfgsRing<[^;]*\bbatch_lbfgs_u<Obj>\(\)[^;]*>;", code)
    ring = re.search(r"^struct LbfgsRing\b.*?^};", code, re.M | re.S).group(0)
    assert "BATCH_LBFGS_U" not in ring and "batch_lbfgs_u" not in ring and ring.count("U * BLOCK") == 4
    assert "in the same order for every U" in src


# ---- 2. the fifth program's text ---------------------------------------------------------------------------------------------------
def test_the_new_generator_embeds_the_kernel_and_the_old_one_does_not(tmp_path):
    new, old = tmp_path / "cgo_rtc_lbfgs_sources.inc", tmp_path / "cgo_rtc_sources.inc"
    subprocess.run([sys.executable, os.path.join(I.CSRC, "gen_rtc_sources.py"), str(new), "kRtcLbfgsSourceChunks",
                    "cgo_qn.hpp", "cgo_resident_qn.hpp", "cgo_kernels_batch_lbfgs.hip.hpp"], check=True)   # (the Makefile's rule)
    subprocess.run([sys.executable, os.path.join(I.CSRC, "gen_rtc_sources.py"), str(old)], check=True)
    text, was = new.read_text(encoding="utf-8"), old.read_text(encoding="utf-8")
    def code(t):   # (comments of the existing text name the kernel: its CODE must not carry it)
        return re.sub(r"//.*", "", re.sub(r"/\*.*?\*/", "", t, flags=re.S))
    assert "k_batch_lbfgs" in code(text) and "qn_update" in code(text) and "res_iterate_qn" in code(text)
    assert "k_batch_lbfgs" not in code(was) and "qn_update" not in code(was) and "res_iterate_qn" not in code(was)
    assert "qn_update" not in was and "k_batch_lbfgs<" not in was
    # stripped as the existing generator strips: no include survives, and nothing host-only
    assert "#include" not in text and "#pragma once" not in text and "CGO_HOST_ONLY" not in text and "std::" not in re.sub(r"//.*", "", text)
    assert I.rtc_program_kernels("RTC_BATCH_LBFGS") == ["k_batch_lbfgs<UserObjective, 3>", "k_batch_grad<UserObjective>"]
    assert ("RTC_BATCH_LBFGS", "batch_qn:", "k_batch_lbfgs", "CGO_BATCH_LBFGS_ROWS", 0) in I.rows("RTC_KERNEL")
    assert I.rtc_programs()["RTC_BATCH_LBFGS"][2] == "RTC_TEXT_LBFGS"
    tu = open(os.path.join(I.CSRC, "cgo_rtc_batch.hip")).read()
    assert "cgo_rtc_lbfgs_sources.inc" in tu and "kRtcLbfgsSourceChunks" in tu
    assert "std::lock_guard<std::mutex> lock(m.mu);" in I.rtc_compile_program_body() and "m.mods[prog]" in I.rtc_compile_program_body()
    mk = open(os.path.join(I.CSRC, "Makefile")).read()
    assert "cgo_rtc_batch.hip" in mk and "gen_rtc_sources.py $@ kRtcLbfgsSourceChunks cgo_qn.hpp cgo_resident_qn.hpp cgo_kernels_batch_lbfgs.hip.hpp" in mk
    assert new.read_text(encoding="utf-8").startswith("// generated by gen_rtc_sources.py") and "static const char *const kRtcLbfgsSourceChunks[] = {" in text
    assert I.every_program_module_is_unloaded()


# ---- 3. Python argument checks ------------------------------------------------------------------------------------------------------
def test_python_arguments_are_checked_before_any_library_call(cgo, monkeypatch):
    from cgo_amd import _lib
    cfg = cgo.setupCGConfig(1e-9, cgo.LBFGS(4), cgo.EnableTrace(), max_iters=4)
    ls = cgo.setupStrongWolfeBisection(1e-5, 0.9)

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", no_library)
    model = cgo.DeviceObjective.__new__(cgo.DeviceObjective)
    model.n_global, model.ctx = 8, None
    ok = np.ones((2, 8))
    with pytest.raises(ValueError, match="unknown objective kind.*minimizeobjectivebatch_lbfgs_obj"):
        cgo.minimizeobjectivebatch_lbfgs(model, ok, cfg, ls)   # the built-in call still refuses a model, and says where to go
    with pytest.raises(ValueError, match="run-time compiled"):
        cgo.minimizeobjectivebatch_lbfgs_obj("quad_diag", ok, cfg, ls)
    with pytest.raises(ValueError, match="run-time compiled"):
        cgo.batch_lbfgs_max_n_obj("quad_diag")
    with pytest.raises(ValueError, match=r"\[batch, n\]"):
        cgo.minimizeobjectivebatch_lbfgs_obj(model, np.ones(8), cfg, ls)
    with pytest.raises(ValueError, match=r"\[batch, 8\]"):
        cgo.minimizeobjectivebatch_lbfgs_obj(model, np.ones((2, 7)), cfg, ls)
    with pytest.raises(ValueError, match=r"params\[1\] must have the shape of X0"):
        cgo.minimizeobjectivebatch_lbfgs_obj(model, ok, cfg, ls, params=[ok, np.ones((2, 7))])
    with pytest.raises(ValueError, match=r"params\[0\] is None"):
        cgo.minimizeobjectivebatch_lbfgs_obj(model, ok, cfg, ls, params=[None])
    with pytest.raises(ValueError, match="scalars must be"):
        cgo.minimizeobjectivebatch_lbfgs_obj(model, ok, cfg, ls, params=[ok], scalars=np.ones(3))
    with pytest.raises(ValueError, match="scalars must be finite"):
        cgo.minimizeobjectivebatch_lbfgs_obj(model, ok, cfg, ls, params=[ok], scalars=np.array([1.0, np.inf]))
    with pytest.raises(ValueError, match="slice_iters"):
        cgo.minimizeobjectivebatch_lbfgs_obj(model, ok, cfg, ls, params=[ok], slice_iters=-1)


# ---- 4. the reference itself on every GPU problem ---------------------------------------------------------------------------------------
_REF = {}


def refs(p):
    """(run_oracle, run_numpy) once per distinct problem"""
    k = p.key()
    if k not in _REF:
        c = p.case()
        _REF[k] = (run_oracle(c), run_numpy(c))
    return _REF[k]


def every_batch(cgo):
    return U.all_batches(cgo.batch_lbfgs_shape_obj)


def test_problems_of_a_batch_are_pairwise_distinct(cgo):
    for batch in every_batch(cgo):
        assert len({(p.x0.tobytes(), tuple(v.tobytes() for v in p.slots), p.s0) for p in batch}) == len(batch), batch[0].case().name
        assert len({(p.name, p.n, p.m, tuple(sorted(p.kw.items()))) for p in batch}) == 1


def test_reference_restatements_agree_to_a_tenth_of_the_bar_on_every_gpu_problem(cgo):
    """bitwise on status, iterations, steps and evaluations; ≤ 1e-11 on x, f and the trace, ≤ 1e-10 on ∇f"""
    worst = {}
    for batch in every_batch(cgo):
        for p in batch:
            ref, alt = refs(p)
            for k, v in held(alt, ref, p.case().name, scale=0.1).items():
                if v > worst.get(k, (0.0, ""))[0]:
                    worst[k] = (v, p.case().name)
    print("run_numpy against run_oracle, worst: " + ", ".join(f"{k} {v:.1e} ({n})" for k, (v, n) in worst.items()))


def test_what_the_reference_does_with_the_mixed_batches(cgo):
    assert [(refs(p)[0].status, refs(p)[0].iters_ran) for p in U.mixed_h2()] == U.MIXED_H2_EXPECT
    assert [(refs(p)[0].status, refs(p)[0].iters_ran) for p in U.mixed_one()] == [("success", 1), ("success", 0), ("success", 21)]
    z = [(refs(p)[0].status, refs(p)[0].iters_ran) for p in U.mixed_one(2)]
    assert z == [("zoom_max_iters_reached", 0), ("zoom_max_iters_reached", 0), ("success", 1), ("success", 0)]
    # a scalar of exactly 1.0 changes no bit: problems 0, 2 and 4 of the scaled batch are H2's
    sh = [refs(p)[0] for p in U.mixed_sh()]
    for b in (0, 2, 4):
        h = refs(U.mixed_h2()[b])[0]
        assert (sh[b].status, sh[b].iters_ran, sh[b].objective) == (h.status, h.iters_ran, h.objective) and np.array_equal(sh[b].minimizer, h.minimizer)
    print("SH on the mixed batch:", [(r.status, r.iters_ran) for r in sh])
    assert sum(r.status not in ("success", "max_iters_reached") for r in sh) >= 2
    # every other batch stays on the device: its problems end max_iters_reached (or success) under the reference
    for batch in every_batch(cgo):
        if batch[0].kw.get("zoom_max_iters", 100) < 100:
            continue
        for p in batch:
            assert refs(p)[0].status in ("max_iters_reached", "success"), p.case().name
