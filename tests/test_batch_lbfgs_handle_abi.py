"""CPU tier of the batch handle for L-BFGS solves (tests/test_batch_lbfgs_handle.py is the GPU tier): the new entry points —
declared in the host-only region of include/cgo.h, exported, bound in _lib.py and in the Julia shim —, their null-argument
refusals, the Python argument checks that need no library, and that the texts of the kernels are what they were: the feature
adds no device code."""
import os
import re
import subprocess

import numpy as np
import pytest

import _instances as I
import test_batch_lbfgs_lds_abi as LDS
import test_julia_shim as JL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cgo_batch_lbfgs_open": 8, "cgo_batch_lbfgs_solve": 8, "cgo_batch_lbfgs_m": 2}


def test_symbols_are_declared_host_only_exported_and_refuse_null_arguments(cgo):
    from cgo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cgo.h"), encoding="utf-8").read()
    host_only = "".join(re.findall(r"^/\* CGO_HOST_ONLY_BEGIN.*?^/\* CGO_HOST_ONLY_END \*/\n", hdr, flags=re.M | re.S))
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", host_only, flags=re.S))
    outside = re.sub(r"/\*.*?\*/", "", hdr.replace(host_only, ""), flags=re.S)
    L = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name, nargs in NEW.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and getattr(L, name), name
        proto = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", flat)
        assert proto, f"{name} is not declared between the host-only markers"
        assert len(proto.group(1).strip().split(",")) == nargs, name
        assert name not in outside, f"{name} is named by code outside the host-only region"
        assert name in exported, name
    # the ctypes signatures, argument by argument
    import ctypes as C
    vp, dp = C.c_void_p, _lib.dp
    assert _lib.SIGNATURES["cgo_batch_lbfgs_open"] == (C.c_int, [vp, vp, C.c_int64, C.POINTER(dp), C.c_int32, C.c_int32, C.POINTER(_lib.BatchPolicyC), C.POINTER(vp)])
    assert _lib.SIGNATURES["cgo_batch_lbfgs_solve"] == _lib.SIGNATURES["cgo_batch_solve"]
    assert _lib.SIGNATURES["cgo_batch_lbfgs_m"] == (C.c_int, [vp, C.POINTER(C.c_int32)])
    # null arguments, and a NULL handle closes as before
    h = C.c_void_p()
    assert L.cgo_batch_lbfgs_open(None, None, 2, None, 0, 5, None, C.byref(h)) == 1 and "null argument" in L.cgo_last_error().decode()
    assert L.cgo_batch_lbfgs_open(None, None, 2, None, 0, 5, None, None) == 1
    assert L.cgo_batch_lbfgs_solve(None, None, None, None, None, None, 0, None) == 1 and "null argument" in L.cgo_last_error().decode()
    m = C.c_int32(7)
    assert L.cgo_batch_lbfgs_m(None, C.byref(m)) == 1 and m.value == 7
    assert L.cgo_batch_close(None) == 0
    # the header no longer says the handle is missing, and says what the two kinds of handle refuse of each other
    assert "Not built: the cgo_batch handle" not in hdr
    assert "cgo_batch_close and cgo_batch_rows serve both kinds" in hdr


def test_the_julia_shim_binds_the_new_calls():
    """every ccall names an exported symbol with the declared number of arguments (the shim's own test, unedited), and the three
    new symbols are among them"""
    JL.test_blocks_and_brackets_balance()
    JL.test_every_ccall_names_an_exported_symbol_with_the_declared_number_of_arguments()
    src = JL._strip(open(JL.JL, encoding="utf-8").read())
    for sym in NEW:
        assert re.search(r"ccall\(\(:" + sym + r", libcgo\)", src), sym
    assert re.search(r"^mutable struct BatchLBFGS\b", src, re.M)
    assert re.search(r"^function solve!\(out::CBatchResults, B::BatchLBFGS,", src, re.M)
    assert re.search(r"^function Base\.close\(B::BatchLBFGS\)", src, re.M)


def test_python_names_and_argument_checks_need_no_library(cgo, monkeypatch):
    from cgo_amd import _lib
    assert issubclass(cgo.BatchLBFGS, object) and callable(cgo.primalbarriermethodbatch_lbfgs)
    for f in (cgo.BatchLBFGS, cgo.BatchLBFGS.solve, cgo.primalbarriermethodbatch_lbfgs, cgo.primalbarriermethodbatch):
        assert f.__doc__
    assert "no `Batch` handle" not in cgo.minimizeobjectivebatch_lbfgs_obj.__doc__
    assert "BatchLBFGS" in cgo.primalbarriermethodbatch_lbfgs.__doc__ and "verifyt0" in cgo.primalbarriermethodbatch_lbfgs.__doc__
    lb5 = cgo.setupCGConfig(1e-2, cgo.LBFGS(5), cgo.EnableTrace(), max_iters=10)
    hz = cgo.setupCGConfig(1e-2, cgo.HagerZhang(), cgo.EnableTrace(), max_iters=10)
    br = cgo.setupCGConfig(1e-2, cgo.BroydenFamily(0.5), cgo.EnableTrace(), max_iters=10)
    wb = cgo.WolfeBisection(cgo.Wolfe(1e-3, 0.9), 100, 1e12, 50)
    bt = cgo.Backtracking(cgo.Armijo(1e-4), 0.5, 100, 50)
    bc = cgo.setupPrimalBarrierConfig(1e-2, 10.0, 3, 1.0)
    box = cgo.BoxConstraints(-1.0, 1.0)

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", no_library)
    model = cgo.DeviceObjective.__new__(cgo.DeviceObjective)
    model.n_global, model.ctx, model.kind, model._h = 8, None, "user", None
    ok = np.ones((2, 8))
    for rows in ("hbm", "LDS", None, 0):
        with pytest.raises(ValueError, match="rows must be one of"):
            cgo.BatchLBFGS(model, [ok], 2, 5, rows=rows)
        with pytest.raises(ValueError, match="rows must be one of"):
            cgo.primalbarriermethodbatch_lbfgs(cgo.BoxConstraints(-1.0, 1.0), "quad", ok * 0, None, None, None, rows=rows)
    with pytest.raises(ValueError, match="run-time compiled"):
        cgo.BatchLBFGS("quad_diag", [ok], 2, 5)
    with pytest.raises(ValueError, match="m must be an integer"):
        cgo.BatchLBFGS(model, [ok], 2, 2.5)
    with pytest.raises(ValueError, match="batch must be"):
        cgo.BatchLBFGS(model, [ok], 0, 5)
    with pytest.raises(ValueError, match=r"params\[0\] must be"):
        cgo.BatchLBFGS(model, [np.ones((2, 7))], 2, 5)
    # the barrier method's refusals come before any work: no objective is created, no library call made
    for stage in (hz, br):
        with pytest.raises(cgo.CgoError, match="primalbarriermethodbatch") as e:
            cgo.primalbarriermethodbatch_lbfgs(box, "quad", ok * 0, stage, wb, bc)
        assert e.value.code == 1
        with pytest.raises(cgo.CgoError, match="primalbarriermethodbatch"):
            cgo.primalbarriermethodbatch_lbfgs(box, "quad", ok * 0, lb5, wb, bc, (stage, wb))
    with pytest.raises(cgo.CgoError, match="Backtracking"):
        cgo.primalbarriermethodbatch_lbfgs(box, "quad", ok * 0, lb5, bt, bc)
    with pytest.raises(cgo.CgoError, match="Backtracking"):
        cgo.primalbarriermethodbatch_lbfgs(box, "quad", ok * 0, lb5, wb, bc, (lb5, bt))
    # … and primalbarriermethodbatch keeps refusing LBFGS in its own words
    with pytest.raises(cgo.CgoError, match="L-BFGS is not supported"):
        cgo.primalbarriermethodbatch(box, "quad", ok * 0, lb5, wb, bc)


def test_the_kernels_texts_stay_one_definition_each(tmp_path):
    """the one-definition checks of the LDS tier's CPU tests still hold: this feature adds no device code"""
    LDS.test_the_table_row_and_the_translation_units()
    LDS.test_existing_generated_texts_are_unchanged_and_the_new_one_carries_the_kernel(tmp_path)
    # neither kernel header names the handle; the reset that gives a solve its own m is host code
    for name in ("cgo_kernels_batch_lbfgs.hip.hpp", "cgo_kernels_batch_lbfgs_lds.hip.hpp"):
        assert "m_max" not in open(os.path.join(I.CSRC, name)).read(), name
    be = open(os.path.join(I.CSRC, "cgo_backend_batch_lbfgs.hip")).read()
    assert "int HipBackend::batch_lbfgs_reset(int m)" in be and "qn_init(q, m);" in be
    assert "L.ring_stride = (long long)(bat_m_ + 1) * bat_ld_;" in be   # the stride stays the allocated ring's
