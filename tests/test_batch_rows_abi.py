"""CPU tier of the batched solves' device-rows tier (tests/test_batch_rows.py is the GPU tier): the policy struct and its
defaults, the struct layout against the header, the exported _ex entry points, the table row and the translation units, and
the argument checks of the Python layer — none of which needs a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _instances as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = {"cgo_minimize_batch_ex": 12, "cgo_minimize_batch_obj_ex": 12, "cgo_batch_open_ex": 7, "cgo_batch_max_n_ex": 3,
      "cgo_batch_max_n_obj_ex": 2, "cgo_batch_policy_init": 1, "cgo_batch_rows": 2, "cgo_batch_rows_shape": 2}


def test_policy_init_sets_every_field_to_its_default(cgo):
    from cgo_amd import _lib
    pol = _lib.BatchPolicyC()
    C.memset(C.byref(pol), 0xFF, C.sizeof(pol))
    _lib.lib().cgo_batch_policy_init(C.byref(pol))
    assert pol.size == C.sizeof(_lib.BatchPolicyC) == 32
    assert pol.rows == 0 == cgo.BATCH_ROWS["lds"] and list(pol.reserved) == [0] * 6
    assert cgo.BATCH_ROWS == {"lds": 0, "device": 1, "auto": 2}
    _lib.lib().cgo_batch_policy_init(None)   # as free(NULL)


def test_policy_struct_layout_matches_header(cgo, tmp_path):
    from cgo_amd import _lib
    fields = [f for f, _ in _lib.BatchPolicyC._fields_]
    prog = tmp_path / "policy_layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cgo.h"\nint main(void){\n printf("%zu", sizeof(cgo_batch_policy));\n' +
                    "\n".join(f' printf(" %zu", offsetof(cgo_batch_policy, {f}));' for f in fields) +
                    '\n printf("\\n%d %d %d %d %zu\\n", CGO_BATCH_ROWS_LDS, CGO_BATCH_ROWS_DEVICE, CGO_BATCH_ROWS_AUTO, CGO_VERSION, sizeof(cgo_batch_results));\n return 0; }\n')
    exe = tmp_path / "policy_layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    l1, l2 = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    assert [int(v) for v in l1.split()] == [C.sizeof(_lib.BatchPolicyC)] + [getattr(_lib.BatchPolicyC, f).offset for f in fields]
    assert [int(v) for v in l2.split()] == [0, 1, 2, 100, C.sizeof(_lib.BatchResultsC)]   # additive: version and results struct as they were


def test_ex_symbols_are_declared_and_exported(cgo):
    from cgo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cgo.h"), encoding="utf-8").read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    L = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name, nargs in EX.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and getattr(L, name), name
        proto = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", flat)
        assert proto and len(proto.group(1).split(",")) == nargs, name
        assert name in exported, name
    assert _lib.SIGNATURES["cgo_batch_max_n_ex"][0] is C.c_int64 and _lib.SIGNATURES["cgo_batch_max_n_obj_ex"][0] is C.c_int64
    # null arguments are argument errors, a null policy is the call without one
    assert L.cgo_minimize_batch_ex(None, 0, 8, 2, None, None, None, None, 0, None, None, None) == 1
    assert L.cgo_minimize_batch_obj_ex(None, None, 2, None, None, 0, None, None, 0, None, None, None) == 1
    h = C.c_void_p()
    assert L.cgo_batch_open_ex(None, None, 2, None, 0, None, C.byref(h)) == 1 and not h.value
    assert L.cgo_batch_rows(None, None) == 1
    assert L.cgo_batch_max_n_ex(None, 0, None) == 0 and L.cgo_batch_max_n_obj_ex(None, None) == 0
    pol = _lib.BatchPolicyC()
    L.cgo_batch_policy_init(C.byref(pol))
    pol.size = 8   # a struct of another version
    cfg, ls = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=4)._c(), cgo.setupStrongWolfeBisection(1e-5, 0.1)._c()
    out, x = _lib.BatchResultsC(), np.ones(16)
    ctx = C.c_void_p(1)   # (never dereferenced: the policy is checked first)
    assert L.cgo_minimize_batch_ex(ctx, 0, 8, 2, x.ctypes.data_as(_lib.dp), x.ctypes.data_as(_lib.dp), C.byref(cfg), C.byref(ls), 0,
                                   C.byref(pol), C.byref(out), None) == 1
    assert "cgo_batch_policy.size" in L.cgo_last_error().decode()


def test_streaming_loop_shape_needs_no_device(cgo):
    block, u = cgo.batch_rows_shape()
    src = open(os.path.join(I.CSRC, "cgo_kernels_batch_rows.hip.hpp")).read()
    assert block == 256 and u == int(re.search(r"^#define CGO_BATCH_ROWS_U (\d+)", src, re.M).group(1)) and 1 <= u <= 8


def test_python_rows_argument_is_checked_before_any_library_call(cgo, monkeypatch):
    from cgo_amd import _lib
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=4)
    ls = cgo.setupStrongWolfeBisection(1e-5, 0.1)
    model = cgo.DeviceObjective.__new__(cgo.DeviceObjective)
    model.kind, model.n_global, model.ctx, model._h = "user", 8, None, C.c_void_p()

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", no_library)
    for bad in ("hbm", "LDS", 1, None):
        with pytest.raises(ValueError, match="rows must be"):
            cgo.minimizeobjectivebatch("quad_diag", np.ones((2, 8)), cfg, ls, D=np.ones((2, 8)), rows=bad)
        with pytest.raises(ValueError, match="rows must be"):
            cgo.Batch(model, [np.ones((2, 8))], 2, rows=bad)
        with pytest.raises(ValueError, match="rows must be"):
            cgo.batch_max_n("quad_diag", rows=bad)
        with pytest.raises(ValueError, match="rows must be"):
            cgo.primalbarriermethodbatch(cgo.BoxConstraints(0.0, 1.0), "ObjQuadDiag", np.full((2, 8), 0.5), cfg, ls,
                                         cgo.setupPrimalBarrierConfig(1e-2, 10.0, 5), params=[np.ones((2, 8))], rows=bad)


def test_the_table_row_and_the_translation_units():
    assert I.rows("BATCH_DEVROWS") == [(3,)] and I.rows("BATCH") == [(3,)]
    rows_tu = open(os.path.join(I.CSRC, "cgo_backend_batch_rows.hip")).read()
    assert "CGO_BATCH_DEVROWS_ROWS(ROW)" in rows_tu and "k_batch_rows<Obj, NPTS>" in rows_tu
    assert "row_pick_for<BatchDevRows>(obj_kind, npts)" in rows_tu and "CGO_OBJ_ROWS(ROW)" in open(os.path.join(I.CSRC, "cgo_backend_internal.hpp")).read()   # (the switch over the objectives: once, for every tier)
    # k_batch's translation unit does not see the new kernel (its device code stays what it was), nor does the program every
    # objective compiles at creation or the batch program's kernel list
    batch_tu = open(os.path.join(I.CSRC, "cgo_backend_batch.hip")).read()
    assert "cgo_kernels_batch_rows.hip.hpp" not in batch_tu and "k_batch_rows<" not in batch_tu
    assert "k_batch" not in open(os.path.join(I.CSRC, "cgo_rtc.hip")).read()
    # a program of its own, with a module handle of its own: the batch program compiles what it compiled
    assert I.rtc_program_kernels("RTC_BATCH_ROWS") == ["k_batch_rows<UserObjective, 3>"]
    assert '"<cgo::dev::UserObjective, "' in open(os.path.join(I.CSRC, "cgo_rtc_batch.hip")).read() and "m.mods[prog]" in I.rtc_compile_program_body()
    assert I.rtc_program_kernels("RTC_BATCH") == ["k_batch<UserObjective, 3>", "k_batch_grad<UserObjective>"]
    mk = open(os.path.join(I.CSRC, "Makefile")).read()
    assert "cgo_backend_batch_rows.hip" in mk and mk.count("cgo_kernels_batch_rows.hip.hpp") == 2


def test_embedded_kernel_sources_carry_the_rows_kernel_last(tmp_path):
    out = tmp_path / "cgo_rtc_sources.inc"
    subprocess.run([sys.executable, os.path.join(I.CSRC, "gen_rtc_sources.py"), str(out)], check=True)
    text = out.read_text(encoding="utf-8")
    # (the argument is BatchParams itself unless the PROBE flag of cgo_batch_probe is set: BatchArg<false>::type)
    assert "void k_batch_rows(const typename BatchArg<PROBE>::type B)" in text
    assert "template <bool PROBE> struct BatchArg { using type = BatchParams; };" in text
    assert text.index("// ---- cgo_kernels_batch.hip.hpp") < text.index("// ---- cgo_kernels_batch_rows.hip.hpp")
    assert '#include "' not in text.split("// ---- cgo_kernels_batch_rows.hip.hpp")[1]
    # the kernel takes BatchParams as it is, no dynamic LDS, and none of what the pool forbids for data exchange
    src = open(os.path.join(I.CSRC, "cgo_kernels_batch_rows.hip.hpp")).read()
    code = re.sub(r"//.*", "", src)
    assert "extern __shared__" not in code and "atomic" not in code and "struct BatchParams" not in code
