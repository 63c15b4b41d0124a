"""CPU tier of the batched solves (tests/test_batch.py is the GPU tier): the table row, the C ABI's struct, the one
status-from-state rule, and the refusal to compute anything without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _instances as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_table_has_one_batch_row_and_every_other_family_is_as_it_was():
    assert I.rows("BATCH") == [(3,)]
    assert I.rows("RESIDENT") == [(1,), (3,), (7,)] and I.rows("RESIDENT_CHAIN") == [(1,), (3,)] and I.rows("RTC_RESIDENT") == [(3,)]
    assert I.rows("OBJ") == [("CGO_OBJ_QUAD_DIAG", "ObjQuadDiag"), ("CGO_OBJ_ROSENBROCK_PAIRED", "ObjRosenPaired"), ("CGO_OBJ_BOOTH", "ObjBooth")]
    assert [len(I.rows(f)) for f in ("CG", "CG_LAG", "CG_REPLAY", "CG_LEAN", "CG_ARMED", "CHAIN", "FUSED_OBJ", "FUSED_FREE", "RTC_LBFGS")] == \
        [12, 4, 4, 2, 1, 10, 4, 6, 2]
    # the dispatch is expanded from the row, and the run-time compiled module does not build the kernel
    src = open(os.path.join(I.CSRC, "cgo_backend_batch.hip")).read()
    assert "CGO_BATCH_ROWS(ROW)" in src and "CGO_OBJ_ROWS(ROW)" in src
    assert "k_batch" not in open(os.path.join(I.CSRC, "cgo_rtc.hip")).read()
    assert I.stray_uses() == []


def test_batch_results_struct_layout_matches_header(cgo, tmp_path):
    from cgo_amd import _lib
    fields = [f for f, _ in _lib.BatchResultsC._fields_]
    prog = tmp_path / "batch_layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cgo.h"\nint main(void){\n printf("%zu", sizeof(cgo_batch_results));\n' +
                    "\n".join(f' printf(" %zu", offsetof(cgo_batch_results, {f}));' for f in fields) +
                    '\n printf("\\n%d %zu\\n", CGO_VERSION, sizeof(cgo_solver_policy));\n return 0; }\n')
    exe = tmp_path / "batch_layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    l1, l2 = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    assert [int(v) for v in l1.split()] == [C.sizeof(_lib.BatchResultsC)] + [getattr(_lib.BatchResultsC, f).offset for f in fields]
    assert [int(v) for v in l2.split()] == [100, C.sizeof(_lib.SolverPolicyC)]   # additive: the version and the policy keep their values


def test_status_follows_from_the_state_in_one_place(cgo):
    """optim.jl:53-80,162-169 — the rule Solver::iterate applies at the top of an iteration and a batched solve applies to a
    problem the device finished (stop_status, csrc/cgo_resident.hpp), through the ABI."""
    from cgo_amd import _lib
    L = _lib.lib()
    names = {L.cgo_status_name(i).decode(): i for i in range(20)}

    def rule(it, max_iters, f_x, norm, eps, f_x0):
        ran = C.c_int64(-7)
        return L.cgo_stop_status(it, max_iters, f_x, norm, eps, f_x0, C.byref(ran)), ran.value

    assert rule(16, 16, 3.0, 1.0, 1e-9, 5.0) == (names["max_iters_reached"], 16)        # it == max_iters, whatever the norm …
    assert rule(16, 16, 3.0, 1e-12, 1e-9, 5.0) == (names["max_iters_reached"], 16)      # … even a converged one: this test comes first
    assert rule(3, 16, 3.0, 1e-12, 1e-9, 5.0) == (names["success"], 3)                  # norm < ϵ, f_x ≤ f_x0
    assert rule(0, 16, 5.0, 0.0, 1e-9, 5.0) == (names["success"], 0)                    # (equality counts; x0 already stationary)
    assert rule(3, 16, 5.5, 1e-12, 1e-9, 5.0) == (names["increasing_objective"], 3)     # norm < ϵ, f_x > f_x0
    assert rule(3, 16, 3.0, 1e-9, 1e-9, 5.0)[0] == names["incomplete"]                  # norm == ϵ: the iteration runs
    assert rule(3, 16, float("nan"), 1e-12, 1e-9, 5.0)[0] == names["incomplete"]        # non-finite values never stop here
    assert rule(3, 16, 3.0, float("inf"), 1e-9, 5.0)[0] == names["incomplete"]
    assert rule(0, 0, 3.0, 1.0, 1e-9, 3.0) == (names["max_iters_reached"], 0)


def test_no_cpu_fallback_for_batches(cgo):
    from cgo_amd import _lib
    cnt = C.c_int32(-1)
    assert _lib.lib().cgo_device_count(C.byref(cnt)) == 0
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=4)
    ls = cgo.setupStrongWolfeBisection(1e-5, 0.1)
    if cnt.value == 0:
        with pytest.raises(cgo.CgoError) as e:
            cgo.minimizeobjectivebatch("quad_diag", np.ones((2, 8)), cfg, ls, D=np.ones((2, 8)))
        assert e.value.code == 4 and "no CPU fallback" in e.value.msg   # CGO_ENODEV
    with pytest.raises(ValueError):
        cgo.minimizeobjectivebatch("no_such_objective", np.ones((2, 8)), cfg, ls)
    with pytest.raises(ValueError):
        cgo.minimizeobjectivebatch("quad_diag", np.ones(8), cfg, ls, D=np.ones(8))   # X0 is [batch, n]
    # a null context is an argument error, not a crash
    out = _lib.BatchResultsC()
    cc, lc = cfg._c(), ls._c()
    assert _lib.lib().cgo_minimize_batch(None, 0, 8, 2, np.ones(16).ctypes.data_as(_lib.dp), None, C.byref(cc), C.byref(lc), 0, C.byref(out)) == 1
    assert _lib.lib().cgo_batch_max_n(None, 0) == 0
