"""CPU tier of the LDS tier of batched L-BFGS solves (tests/test_batch_lbfgs_lds.py is the GPU tier): the new entry points, the
table row and translation units, the generated program texts, the size helpers that need no device, and the Python argument
checks."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _instances as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cgo_minimize_batch_lbfgs_ex": 12, "cgo_minimize_batch_lbfgs_obj_ex": 13, "cgo_batch_lbfgs_max_n_ex": 4,
       "cgo_batch_lbfgs_max_n_obj_ex": 3, "cgo_batch_lbfgs_lds_rows": 2, "cgo_batch_lbfgs_lds_shape": 3}
BLOCK = 256
RING_PASSES = ("push_trip", "push_update", "combine_trip", "combine_trial")


def _code(name):
    return re.sub(r"//.*", "", open(os.path.join(I.CSRC, name)).read())


def ring_template_body():
    """the code of LbfgsRing, the one template of the ring passes of both tiers"""
    return re.search(r"^struct LbfgsRing\b.*?^};", _code("cgo_kernels_batch_lbfgs.hip.hpp"), re.M | re.S).group(0)


def ring_pass_definitions(code):
    """how often `code` DEFINES each of the four ring-pass functions (a call has no return type before the name)"""
    return {f: len(re.findall(r"\b(?:void|int) " + f + r"\(", code)) for f in RING_PASSES}


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
    assert L.cgo_minimize_batch_lbfgs_ex(None, 0, 8, 2, None, None, None, None, 0, None, None, None) == 1
    assert "null argument" in L.cgo_last_error().decode()
    assert L.cgo_minimize_batch_lbfgs_obj_ex(None, None, 2, None, None, 0, None, None, None, 0, None, None, None) == 1
    assert "null argument" in L.cgo_last_error().decode()
    assert L.cgo_batch_lbfgs_max_n_ex(None, 0, 5, None) == 0 and L.cgo_batch_lbfgs_max_n_obj_ex(None, 5, None) == 0
    pol = _lib.BatchPolicyC()
    L.cgo_batch_policy_init(pol)
    pol.rows = cgo.BATCH_ROWS["lds"]
    assert L.cgo_batch_lbfgs_max_n_ex(None, 0, 5, pol) == 0 and L.cgo_batch_lbfgs_max_n_obj_ex(None, 5, pol) == 0
    L.cgo_batch_lbfgs_lds_shape(0, None, None)   # as free(NULL)
    # the header states the policy rule, and that it differs from the CG _ex calls
    assert "DIFFERS FROM THE CG _ex CALLS ON PURPOSE" in hdr and "cgo_batch_lbfgs_max_n_ex" in hdr
    assert "an LDS tier on L-BFGS" not in hdr and "tier 3  k_batch_lbfgs_lds" in hdr
    jl = open(os.path.join(ROOT, "conjugategradientoptim.jl_amd", "julia", "ConjugateGradientOptimAMD.jl"), encoding="utf-8").read()
    for name in ("minimizeobjectivebatch_lbfgs", "minimizeobjectivebatch_lbfgs_obj", "batch_lbfgs_max_n", "batch_lbfgs_max_n_obj",
                 "batch_lbfgs_lds_rows", "batch_lbfgs_lds_shape"):
        assert callable(getattr(cgo, name))
        assert re.search(r"^(?:function )?" + name + r"\(", jl, re.M), name
    for sym in NEW:
        assert f":{sym}," in jl, sym
    assert "rows::Symbol = :device" in jl


def test_rows_and_shape_need_no_device(cgo):
    L = cgo.lib()
    for K in range(5):
        for m in range(1, 11):
            assert L.cgo_batch_lbfgs_lds_rows(K, m) == 2 + K + 2 * (m + 1) == cgo.batch_lbfgs_lds_rows(K, m)
    for K, m in ((-1, 5), (5, 5), (0, 0), (0, 11), (2, -3)):
        assert cgo.batch_lbfgs_lds_rows(K, m) == 0
    src = open(os.path.join(I.CSRC, "cgo_kernels_batch_lbfgs_lds.hip.hpp")).read()
    u_max = int(re.search(r"^#define CGO_BATCH_LBFGS_LDS_U (\d+)", src, re.M).group(1))
    u_slots = int(re.search(r"^#define CGO_BATCH_LBFGS_LDS_U_SLOTS (\d+)", src, re.M).group(1))
    for K in range(5):
        block, u = cgo.batch_lbfgs_lds_shape(K)
        assert block == BLOCK and u == (u_max if K <= 1 else u_slots) and 1 <= u <= 8
    # every ring pass takes its pairs per trip from the objective: the tier hands batch_lbfgs_lds_u<Obj>() to the one template
    # of the ring passes, once, and that template's body knows no other source of it; the header says why no bit depends on it
    code = re.sub(r"//.*", "", src)
    assert code.count("batch_lbfgs_lds_u<Obj>()") == 1
    assert re.search(r"using LbfgsLdsDev = LbfgsRing<[^;]*\bbatch_lbfgs_lds_u<Obj>\(\)[^;]*>;", code)
    ring = ring_template_body()
    for name in ("BATCH_LBFGS_U", "BATCH_LBFGS_LDS_U", "batch_lbfgs_u", "batch_lbfgs_lds_u"):
        assert name not in ring, name
    assert "in the same order for every U" in src
    assert "extern __shared__" in code and "__launch_bounds__(BLOCK, 1)" in code
    assert "atomic" not in code and "__threadfence" not in code
    assert "ResDev<Obj, NPTS, false, true>" in code and "res_iterate_qn(" in code and "batch_lbfgs_probe_script(" in code


# ---- 2. the table row and the translation units ----------------------------------------------------------------------------------
def test_the_table_row_and_the_translation_units():
    assert I.rows("BATCH_LBFGS_LDS") == [(3,)]
    assert I.rows("BATCH_LBFGS") == [(3,)] and I.rows("BATCH") == [(3,)] and I.rows("BATCH_DEVROWS") == [(3,)]   # as they were
    assert I.stray_uses() == []
    tu = open(os.path.join(I.CSRC, "cgo_backend_batch_lbfgs_lds.hip")).read()
    assert "CGO_BATCH_LBFGS_LDS_ROWS(ROW)" in tu and "k_batch_lbfgs_lds<Obj, NPTS>" in tu
    assert "row_pick_for<BatchLbfgsLdsRows>(obj_kind, npts)" in tu and "CGO_OBJ_ROWS(ROW)" in open(os.path.join(I.CSRC, "cgo_backend_internal.hpp")).read()   # (the switch over the objectives: once, for every tier)
    # the size arithmetic is the tier's; what the device gives a block and the kernel's static LDS are read once for both LDS
    # tiers (cgo_backend_batch.hip), the launch's dynamic LDS is allowed where the ring is allocated (cgo_backend_batch_lbfgs.hip)
    assert "- 512" in tu and "batch_tier_max_ld(ctx, BatchTier::LBFGS_LDS, obj_kind, m, rtc)" in tu
    shared = open(os.path.join(I.CSRC, "cgo_backend_batch.hip")).read()
    assert "hipDeviceAttributeMaxSharedMemoryPerBlock" in shared and "HipBackend::batch_lbfgs_lds_ld_of(max_lds, static_lds, t.lds_rows(nparams, m))" in shared
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in open(os.path.join(I.CSRC, "cgo_backend_batch_lbfgs.hip")).read()
    mk = open(os.path.join(I.CSRC, "Makefile")).read()
    for f in ("cgo_backend_batch_lbfgs_lds.hip", "cgo_rtc_batch.hip", "cgo_kernels_batch_lbfgs_lds.hip.hpp",
              "gen_rtc_sources.py $@ kRtcLbfgsLdsSourceChunks cgo_kernels_batch_lbfgs_lds.hip.hpp"):
        assert f in mk, f
    # the kernel is instantiated in its own unit, in the run-time compiled objectives' unit of the tier (by name) and, as PROBE
    # twins, in the probe unit: no other translation unit names it, and none of them includes its header
    own = {"cgo_backend_batch_lbfgs_lds.hip", "cgo_rtc_batch.hip", "cgo_backend_batch_probe.hip"}
    for name in sorted(os.listdir(I.CSRC)):
        if not (name.endswith(".hip") or name.endswith(".cpp")) or name in own:
            continue
        text = open(os.path.join(I.CSRC, name)).read()
        assert "k_batch_lbfgs_lds" not in re.sub(r"//.*", "", text) and "cgo_kernels_batch_lbfgs_lds.hip.hpp" not in text, name
    probe = open(os.path.join(I.CSRC, "cgo_backend_batch_probe.hip")).read()
    assert "k_batch_lbfgs_lds<Obj, NPTS, true>" in probe and "CGO_BATCH_LBFGS_LDS_ROWS(ROW)" in probe
    assert ", true>" not in tu
    # the device tier has no dynamic LDS
    dev = re.sub(r"//.*", "", open(os.path.join(I.CSRC, "cgo_kernels_batch_lbfgs.hip.hpp")).read())
    assert "extern __shared__" not in dev
    # … and it hands its own pairs per trip to the template of the ring passes, once; the four passes exist once in the two headers
    assert dev.count("batch_lbfgs_u<Obj>()") == 1
    assert re.search(r"using LbfgsDev = LbfgsRing<[^;]*\bbatch_lbfgs_u<Obj>\(\)[^;]*>;", dev)
    assert ring_pass_definitions(ring_template_body()) == dict.fromkeys(RING_PASSES, 1)
    assert ring_pass_definitions(dev + _code("cgo_kernels_batch_lbfgs_lds.hip.hpp")) == dict.fromkeys(RING_PASSES, 1)
    assert I.rtc_program_kernels("RTC_BATCH_LBFGS_LDS") == ["k_batch_lbfgs_lds<UserObjective, 3>"]   # that one kernel and nothing else
    assert I.rtc_programs()["RTC_BATCH_LBFGS_LDS"][2] == "RTC_TEXT_LBFGS_LDS"
    assert "std::lock_guard<std::mutex> lock(m.mu);" in I.rtc_compile_program_body() and "m.mods[prog]" in I.rtc_compile_program_body()
    assert I.every_program_module_is_unloaded()


# ---- 3. the generated texts --------------------------------------------------------------------------------------------------------
GENERATED = {   # the three texts, by the name each went by when a script of its own wrote it: the arguments of the one generator (the Makefile's rules)
    "gen_rtc_sources.py": (),
    "gen_rtc_lbfgs_sources.py": ("kRtcLbfgsSourceChunks", "cgo_qn.hpp", "cgo_resident_qn.hpp", "cgo_kernels_batch_lbfgs.hip.hpp"),
    "gen_rtc_lbfgs_lds_sources.py": ("kRtcLbfgsLdsSourceChunks", "cgo_kernels_batch_lbfgs_lds.hip.hpp"),
}


def _generate(csrc, name, out):
    subprocess.run([sys.executable, os.path.join(csrc, "gen_rtc_sources.py"), str(out), *GENERATED[name]], check=True)
    return out.read_text(encoding="utf-8")


def test_existing_generated_texts_are_unchanged_and_the_new_one_carries_the_kernel(tmp_path):
    new = _generate(I.CSRC, "gen_rtc_lbfgs_lds_sources.py", tmp_path / "cgo_rtc_lbfgs_lds_sources.inc")
    assert "k_batch_lbfgs_lds" in re.sub(r"//.*", "", new) and "#include" not in new and "#pragma once" not in new
    assert "kRtcLbfgsLdsSourceChunks" in new and "std::" not in re.sub(r"//.*", "", new)
    now = {g: _generate(I.CSRC, g, tmp_path / (g + ".now.inc")) for g in ("gen_rtc_sources.py", "gen_rtc_lbfgs_sources.py")}
    for g, text in now.items():
        assert "k_batch_lbfgs_lds" not in text and "LbfgsLdsDev" not in text, g
    # the ring passes of both tiers are the device tier's text: defined there once, and nowhere in what the LDS tier adds
    code = {g: re.sub(r"//.*", "", text) for g, text in dict(now, lds=new).items()}
    assert ring_pass_definitions(code["gen_rtc_lbfgs_sources.py"]) == dict.fromkeys(RING_PASSES, 1)
    assert ring_pass_definitions(code["lds"]) == dict.fromkeys(RING_PASSES, 0)
    assert ring_pass_definitions(code["gen_rtc_sources.py"]) == dict.fromkeys(RING_PASSES, 0)
    if shutil.which("git") is None:
        pytest.skip("git is absent: the parent commit's generators cannot be read")
    top = subprocess.run(["git", "-C", ROOT, "rev-parse", "--show-toplevel"], capture_output=True, text=True)
    if top.returncode != 0 or os.path.realpath(top.stdout.strip()) != os.path.realpath(ROOT):
        pytest.skip("not a git checkout: the parent commit's generators cannot be read")
    # the parent: the commit before the one that added this tier's header
    rel = "conjugategradientoptim.jl_amd/csrc"
    log = subprocess.run(["git", "-C", ROOT, "log", "--format=%H", "--diff-filter=A", "--", f"{rel}/cgo_kernels_batch_lbfgs_lds.hip.hpp"],
                         capture_output=True, text=True).stdout.split()
    parent = (log[-1] + "~") if log else "HEAD"   # (not committed yet: the checkout's HEAD is the parent)
    old = tmp_path / "parent" / rel
    os.makedirs(old)
    os.makedirs(tmp_path / "parent" / "include")
    names = subprocess.run(["git", "-C", ROOT, "ls-tree", "--name-only", parent, f"{rel}/", "include/"], capture_output=True, text=True)
    if names.returncode != 0:
        pytest.skip(f"the parent commit {parent} is not in this checkout's history")
    for path in names.stdout.split():
        blob = subprocess.run(["git", "-C", ROOT, "show", f"{parent}:{path}"], capture_output=True)
        if blob.returncode == 0:
            with open(tmp_path / "parent" / path, "wb") as f:
                f.write(blob.stdout)
    was = _generate(str(old), "gen_rtc_sources.py", tmp_path / "gen_rtc_sources.py.was.inc")
    assert was == now["gen_rtc_sources.py"], "gen_rtc_sources.py: the generated text changed"


# ---- 4. Python argument checks ------------------------------------------------------------------------------------------------------
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
    for rows in ("hbm", "LDS", None, 0):
        with pytest.raises(ValueError, match="rows must be one of"):
            cgo.minimizeobjectivebatch_lbfgs("quad_diag", ok, cfg, ls, D=ok, rows=rows)
        with pytest.raises(ValueError, match="rows must be one of"):
            cgo.minimizeobjectivebatch_lbfgs_obj(model, ok, cfg, ls, params=[ok], rows=rows)
        with pytest.raises(ValueError, match="rows must be one of"):
            cgo.batch_lbfgs_max_n("quad_diag", m=5, rows=rows)
        with pytest.raises(ValueError, match="rows must be one of"):
            cgo.batch_lbfgs_max_n_obj(model, m=5, rows=rows)
    with pytest.raises(ValueError, match="rows='lds' needs m"):
        cgo.batch_lbfgs_max_n("quad_diag", rows="lds")
    with pytest.raises(ValueError, match="rows='lds' needs m"):
        cgo.batch_lbfgs_max_n_obj(model, rows="lds")
    with pytest.raises(ValueError, match="m must be an integer"):
        cgo.batch_lbfgs_max_n("quad_diag", m=2.5, rows="lds")
    with pytest.raises(ValueError, match="unknown objective kind"):
        cgo.batch_lbfgs_max_n("cubic", m=5, rows="lds")
    with pytest.raises(ValueError, match="run-time compiled"):
        cgo.batch_lbfgs_max_n_obj("quad_diag", m=5, rows="lds")
    # the existing shape and scalar checks under the new keyword
    for rows in ("lds", "auto", "device"):
        with pytest.raises(ValueError, match="unknown objective kind.*minimizeobjectivebatch_lbfgs_obj"):
            cgo.minimizeobjectivebatch_lbfgs(model, ok, cfg, ls, rows=rows)
        with pytest.raises(ValueError, match=r"\[batch, n\]"):
            cgo.minimizeobjectivebatch_lbfgs("quad_diag", np.ones(8), cfg, ls, rows=rows)
        with pytest.raises(ValueError, match="D must have the shape of X0"):
            cgo.minimizeobjectivebatch_lbfgs("quad_diag", ok, cfg, ls, D=np.ones((2, 7)), rows=rows)
        with pytest.raises(ValueError, match="run-time compiled"):
            cgo.minimizeobjectivebatch_lbfgs_obj("quad_diag", ok, cfg, ls, rows=rows)
        with pytest.raises(ValueError, match=r"\[batch, n\]"):
            cgo.minimizeobjectivebatch_lbfgs_obj(model, np.ones(8), cfg, ls, rows=rows)
        with pytest.raises(ValueError, match=r"\[batch, 8\]"):
            cgo.minimizeobjectivebatch_lbfgs_obj(model, np.ones((2, 7)), cfg, ls, rows=rows)
        with pytest.raises(ValueError, match=r"params\[1\] must have the shape of X0"):
            cgo.minimizeobjectivebatch_lbfgs_obj(model, ok, cfg, ls, params=[ok, np.ones((2, 7))], rows=rows)
        with pytest.raises(ValueError, match=r"params\[0\] is None"):
            cgo.minimizeobjectivebatch_lbfgs_obj(model, ok, cfg, ls, params=[None], rows=rows)
        with pytest.raises(ValueError, match="scalars must be"):
            cgo.minimizeobjectivebatch_lbfgs_obj(model, ok, cfg, ls, params=[ok], scalars=np.ones(3), rows=rows)
        with pytest.raises(ValueError, match="scalars must be finite"):
            cgo.minimizeobjectivebatch_lbfgs_obj(model, ok, cfg, ls, params=[ok], scalars=np.array([1.0, np.inf]), rows=rows)
        with pytest.raises(ValueError, match="slice_iters"):
            cgo.minimizeobjectivebatch_lbfgs_obj(model, ok, cfg, ls, params=[ok], slice_iters=-1, rows=rows)
    with pytest.raises(ValueError, match="tier must be"):
        cgo.batch_probe("lbfgs_hbm", "quad_diag", np.ones((1, 4)), np.ones((1, 4)), [("init",)])
    assert cgo.BATCH_PROBE_TIERS["lbfgs_lds"] == 3


def test_the_default_is_the_call_without_a_policy(cgo, monkeypatch):
    """rows="device" reaches exactly the entry point it reached before the keyword existed; the others reach the _ex form"""
    from cgo_amd import _lib
    called = []

    class Spy:
        def __getattr__(self, name):
            def f(*a):
                called.append(name)
                return 0
            return f
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    cfg = cgo.setupCGConfig(1e-9, cgo.LBFGS(4), cgo.EnableTrace(), max_iters=4)
    ls = cgo.setupStrongWolfeBisection(1e-5, 0.9)
    ctx = cgo.Context.__new__(cgo.Context)
    ctx._h = None
    ok = np.ones((2, 8))
    for rows, want in (("device", "cgo_minimize_batch_lbfgs"), ("lds", "cgo_minimize_batch_lbfgs_ex"), ("auto", "cgo_minimize_batch_lbfgs_ex")):
        del called[:]
        try:
            cgo.minimizeobjectivebatch_lbfgs("quad_diag", ok, cfg, ls, D=ok, ctx=ctx, rows=rows)
        except Exception:
            pass   # (the spy returns no results to assemble)
        assert called and called[0] == want, (rows, called)
