"""CPU tier of the batched solves on run-time compiled objectives (tests/test_batch_user.py is the GPU tier): the two entry
points are declared and exported, refuse null arguments, compute nothing without a GPU; the table row is as it was and the
embedded kernel sources carry k_batch for the module's batch program."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _instances as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry_points(cgo):
    from cgo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cgo.h"), encoding="utf-8").read()
    flat = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("int cgo_minimize_batch_obj(cgo_ctx *ctx, cgo_objective *model, int64_t batch, const double *x0 , const double *const *params, "
            "int32_t n_params, const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t slice_iters , cgo_batch_results *out);") in flat
    assert "int64_t cgo_batch_max_n_obj(cgo_objective *model);" in flat
    assert "#define CGO_VERSION 100" in hdr and "kPairOnly = true needs an even n" in re.sub(r"\s+\*?\s*", " ", hdr)
    # the kind-based entry point keeps its signature
    assert "int cgo_minimize_batch(cgo_ctx *ctx, int32_t obj_kind, int64_t n, int64_t batch, const double *x0 , const double *param0 ," in flat
    L = _lib.lib()
    for name, nargs in (("cgo_minimize_batch_obj", 10), ("cgo_batch_max_n_obj", 1), ("cgo_minimize_batch", 10), ("cgo_batch_max_n", 2)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and getattr(L, name)
    assert _lib.SIGNATURES["cgo_batch_max_n_obj"][0] is C.c_int64
    assert L.cgo_version() == 100


def test_null_arguments_are_argument_errors(cgo):
    from cgo_amd import _lib
    L = _lib.lib()
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=4)
    ls = cgo.setupStrongWolfeBisection(1e-5, 0.1)
    out = _lib.BatchResultsC()
    cc, lc = cfg._c(), ls._c()
    x = np.ones(16)
    rows = (_lib.dp * 1)(x.ctypes.data_as(_lib.dp))
    assert L.cgo_minimize_batch_obj(None, None, 2, x.ctypes.data_as(_lib.dp), rows, 1, C.byref(cc), C.byref(lc), 0, C.byref(out)) == 1   # CGO_EINVAL
    assert "null argument" in L.cgo_last_error().decode()
    assert L.cgo_minimize_batch_obj(None, None, 2, None, None, 0, None, None, 0, None) == 1
    assert L.cgo_batch_max_n_obj(None) == 0


def test_no_cpu_fallback_for_batches_on_objectives(cgo):
    from cgo_amd import _lib
    cnt = C.c_int32(-1)
    assert _lib.lib().cgo_device_count(C.byref(cnt)) == 0
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=4)
    ls = cgo.setupStrongWolfeBisection(1e-5, 0.1)
    if cnt.value == 0:
        with pytest.raises(cgo.CgoError) as e:   # the model cannot even be made
            cgo.ElementwiseObjective(8, "gi = p*x; fi = 0.5*(gi*x);", param=np.ones(8))
        assert e.value.code == 4 and "no CPU fallback" in e.value.msg   # CGO_ENODEV
        # … and a stand-in for one, with no context of its own, gets the same answer from the call itself
        model = cgo.DeviceObjective.__new__(cgo.DeviceObjective)
        model.kind, model.n_global, model.ctx, model._h = "user", 8, None, C.c_void_p()
        with pytest.raises(cgo.CgoError) as e:
            cgo.minimizeobjectivebatch(model, np.ones((2, 8)), cfg, ls, params=[np.ones((2, 8))])
        assert e.value.code == 4 and "no CPU fallback" in e.value.msg
    # argument errors of the Python layer need no device; a kind name behaves as ever
    model = cgo.DeviceObjective.__new__(cgo.DeviceObjective)
    model.kind, model.n_global, model.ctx, model._h = "user", 8, None, C.c_void_p()
    with pytest.raises(ValueError):
        cgo.minimizeobjectivebatch(model, np.ones((2, 9)), cfg, ls, params=[np.ones((2, 9))])      # the model is of size 8
    with pytest.raises(ValueError):
        cgo.minimizeobjectivebatch(model, np.ones((2, 8)), cfg, ls, params=[np.ones((3, 8))])      # a slot of another shape
    with pytest.raises(ValueError):
        cgo.minimizeobjectivebatch(model, np.ones((2, 8)), cfg, ls, D=np.ones((2, 8)))             # D is the built-in quadratic's
    with pytest.raises(ValueError):
        cgo.minimizeobjectivebatch("quad_diag", np.ones((2, 8)), cfg, ls, params=[np.ones((2, 8))])
    with pytest.raises(ValueError):
        cgo.minimizeobjectivebatch("no_such_objective", np.ones((2, 8)), cfg, ls)


def test_the_batch_row_is_as_it_was_and_the_module_builds_it_in_a_program_of_its_own():
    assert I.rows("BATCH") == [(3,)]
    assert I.rows("RTC_RESIDENT") == [(3,)] and I.rows("OBJ") == [("CGO_OBJ_QUAD_DIAG", "ObjQuadDiag"), ("CGO_OBJ_ROSENBROCK_PAIRED", "ObjRosenPaired"),
                                                                  ("CGO_OBJ_BOOTH", "ObjBooth")]
    assert ("RTC_BATCH", "batch:", "k_batch", "CGO_BATCH_ROWS", 0) in I.rows("RTC_KERNEL") and "k_batch<UserObjective, 3>" in I.rtc_program_kernels("RTC_BATCH")
    assert "CGO_RTC_KERNEL_ROWS(ROW)" in open(os.path.join(I.CSRC, "cgo_rtc_batch.hip")).read()
    assert "k_batch" not in open(os.path.join(I.CSRC, "cgo_rtc.hip")).read()      # not in the program every objective compiles at creation
    assert "cgo_rtc_batch.hip" in open(os.path.join(I.CSRC, "Makefile")).read()
    assert I.stray_uses() == []


def test_embedded_kernel_sources_contain_k_batch(tmp_path):
    out = tmp_path / "cgo_rtc_sources.inc"
    subprocess.run([sys.executable, os.path.join(I.CSRC, "gen_rtc_sources.py"), str(out)], check=True)
    text = out.read_text(encoding="utf-8")
    # (the argument is BatchParams itself unless the PROBE flag of cgo_batch_probe is set: BatchArg<false>::type)
    assert "void k_batch(const typename BatchArg<PROBE>::type B)" in text
    assert "template <bool PROBE> struct BatchArg { using type = BatchParams; };" in text
    assert text.index("// ---- cgo_kernels_resident.hip.hpp") < text.index("// ---- cgo_kernels_batch.hip.hpp")
    assert '#include "' not in text.split("// ---- cgo_kernels_batch.hip.hpp")[1]


def test_batch_params_grow_at_their_end():
    """The kernarg offsets of the fields the three ahead-of-time instantiations read stay where they were: the pointers of
    slots 1–3 follow `budget`, the last field before them."""
    src = open(os.path.join(I.CSRC, "cgo_kernels_batch.hip.hpp")).read()
    body = src[src.index("struct BatchParams {"):]
    body = body[:body.index("};")]
    names = re.findall(r"\b(x|u|p0|st|recs|f_x0|n|ld|rec_stride|rec_abs|s0|cfg|budget|p1|p2|p3)\b(?=[,;])", re.sub(r"//.*", "", body))
    assert names == ["x", "u", "p0", "st", "recs", "f_x0", "n", "ld", "rec_stride", "rec_abs", "s0", "cfg", "budget", "p1", "p2", "p3"]
