"""CPU tier of the batched solves with a scalar per problem and of the batch that stays on the device (GPU tier:
tests/test_batch_scalars.py, tests/test_batch_barrier.py): the three entry points are declared and exported with the header's
argument counts and refuse null arguments; BatchParams grew at its end; the batch program builds k_batch_grad; and the
argument checks of the Python layer raise without a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _instances as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flat_header():
    hdr = open(os.path.join(ROOT, "include", "cgo.h"), encoding="utf-8").read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))


def test_header_declares_and_library_exports_the_entry_points(cgo):
    from cgo_amd import _lib
    flat = _flat_header()
    assert "typedef struct cgo_batch cgo_batch;" in flat
    assert ("int cgo_batch_open(cgo_ctx *ctx, cgo_objective *model, int64_t batch, const double *const *params, int32_t n_params, "
            "cgo_batch **handle);") in flat
    assert ("int cgo_batch_solve(cgo_batch *handle, const double *x0 , const double *scalars , const unsigned char *active , "
            "const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t slice_iters , cgo_batch_results *out);") in flat
    assert "int cgo_batch_close(cgo_batch *handle);" in flat
    # the one-shot entry points keep their signatures
    assert ("int cgo_minimize_batch_obj(cgo_ctx *ctx, cgo_objective *model, int64_t batch, const double *x0 , const double *const *params, "
            "int32_t n_params, const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t slice_iters , cgo_batch_results *out);") in flat
    L = _lib.lib()
    for name, nargs in (("cgo_batch_open", 6), ("cgo_batch_solve", 8), ("cgo_batch_close", 1), ("cgo_minimize_batch_obj", 10), ("cgo_minimize_batch", 10)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and getattr(L, name)
        proto = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", flat)
        assert proto and len(proto.group(1).split(",")) == nargs, name
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert {"cgo_batch_open", "cgo_batch_solve", "cgo_batch_close"} <= exported
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
    h = C.c_void_p()
    assert L.cgo_batch_open(None, None, 2, rows, 1, C.byref(h)) == 1 and "null argument" in L.cgo_last_error().decode()   # CGO_EINVAL
    assert not h.value
    assert L.cgo_batch_open(None, None, 2, None, 0, None) == 1
    assert L.cgo_batch_solve(None, x.ctypes.data_as(_lib.dp), None, None, C.byref(cc), C.byref(lc), 0, C.byref(out)) == 1
    assert "null argument" in L.cgo_last_error().decode()
    assert L.cgo_batch_close(None) == 0   # as free(NULL)


def test_batch_params_end_with_the_scalars():
    """The kernarg offsets of every field the kernels read before this one stay where they were: s0v follows p3."""
    src = open(os.path.join(I.CSRC, "cgo_kernels_batch.hip.hpp")).read()
    body = src[src.index("struct BatchParams {"):]
    body = body[:body.index("};")]
    names = re.findall(r"\b(x|u|p0|st|recs|f_x0|n|ld|rec_stride|rec_abs|s0|cfg|budget|p1|p2|p3|s0v)\b(?=[,;])", re.sub(r"//.*", "", body))
    assert names == ["x", "u", "p0", "st", "recs", "f_x0", "n", "ld", "rec_stride", "rec_abs", "s0", "cfg", "budget", "p1", "p2", "p3", "s0v"]
    assert "Q.s0 = B.s0v ? B.s0v[b] : B.s0;" in src
    # the resident kernel and the loop both kernels run do not know of it
    for f in ("cgo_kernels_resident.hip.hpp", "cgo_resident.hpp"):
        assert "s0v" not in open(os.path.join(I.CSRC, f)).read()


def test_the_gradient_kernel_is_built_ahead_of_time_and_in_the_batch_program(tmp_path):
    assert I.rows("BATCH") == [(3,)] and len(I.rows("OBJ")) == 3
    backend = open(os.path.join(I.CSRC, "cgo_backend_batch.hip")).read()
    assert re.search(r"#define ROW\(KIND, T\) case KIND: return \(const void \*\)k_batch_grad<T>;\s*CGO_OBJ_ROWS\(ROW\)", backend)
    assert ("RTC_BATCH", "batch:grad", "k_batch_grad") in I.rows("RTC_EXTRA") and "k_batch_grad<UserObjective>" in I.rtc_program_kernels("RTC_BATCH")
    assert "CGO_RTC_EXTRA_ROWS(ROW)" in open(os.path.join(I.CSRC, "cgo_rtc_batch.hip")).read()
    assert "k_batch_grad" not in open(os.path.join(I.CSRC, "cgo_rtc.hip")).read()   # not in the program every objective compiles at creation
    assert I.stray_uses() == []
    out = tmp_path / "cgo_rtc_sources.inc"
    subprocess.run([sys.executable, os.path.join(I.CSRC, "gen_rtc_sources.py"), str(out)], check=True)
    text = out.read_text(encoding="utf-8")
    assert "void k_batch_grad(const BatchGradParams G)" in text and "void k_batch(const typename BatchArg<PROBE>::type B)" in text
    assert "template <bool PROBE> struct BatchArg { using type = BatchParams; };" in text   # (BatchParams itself unless PROBE)


def _stand_in(cgo, n=8):
    model = cgo.DeviceObjective.__new__(cgo.DeviceObjective)
    model.kind, model.n_global, model.ctx, model._h = "user", n, None, C.c_void_p()
    return model


def test_python_argument_checks_need_no_device(cgo):
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=4)
    ls = cgo.setupStrongWolfeBisection(1e-5, 0.1)
    with pytest.raises(ValueError, match="reads no scalar"):
        cgo.minimizeobjectivebatch("quad_diag", np.ones((2, 8)), cfg, ls, D=np.ones((2, 8)), scalars=[1.0, 2.0])
    with pytest.raises(ValueError, match="reads no scalar"):
        cgo.minimizeobjectivebatch("rosenbrock_paired", np.ones((2, 8)), cfg, ls, scalars=[1.0, 2.0])
    model = _stand_in(cgo)
    with pytest.raises(ValueError, match="scalars"):
        cgo.minimizeobjectivebatch(model, np.ones((2, 8)), cfg, ls, params=[np.ones((2, 8))], scalars=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match=r"params\[0\]"):
        cgo.Batch(model, [np.ones((3, 8))], 2)
    with pytest.raises(ValueError, match=r"params\[1\]"):
        cgo.Batch(model, [np.ones((2, 8)), np.ones((2, 9))], 2)
    with pytest.raises(ValueError, match="batch must be"):
        cgo.Batch(model, [], 0)
    with pytest.raises(ValueError, match="run-time compiled"):
        cgo.Batch("quad_diag", [], 2)
    B = cgo.Batch.__new__(cgo.Batch)   # an open batch's shape checks come before the library is asked
    B._h, B.model, B.batch, B.n = C.c_void_p(1), model, 2, 8
    for kw in (dict(X0=np.ones((2, 9))), dict(X0=np.ones((3, 8))), dict(X0=np.ones((2, 8)), scalars=np.ones(3)), dict(X0=np.ones((2, 8)), active=[1, 0, 1])):
        with pytest.raises(ValueError):
            B.solve(kw.pop("X0"), cfg, ls, **kw)
    B._h = None
    with pytest.raises(ValueError, match="closed"):
        B.solve(np.ones((2, 8)), cfg, ls)


def test_barrier_batch_refusals_need_no_device(cgo):
    cfg = cgo.setupCGConfig(1e-5, cgo.HagerZhang(), cgo.EnableTrace(), max_iters=100)
    ls = cgo.WolfeBisection(cgo.Wolfe(1e-3, 0.9), 100, 1e12, 50)
    bc = cgo.setupPrimalBarrierConfig(1e-2, 10.0, 5)
    X0, rows = np.ones((2, 8)), np.ones((2, 8))
    box = cgo.BoxConstraints(np.zeros(8), np.full(8, 2.0))
    three = "struct BaseObjective { static constexpr int kParams = 3; static constexpr bool kPairOnly = false; };"
    with pytest.raises(AssertionError, match="no two slots"):   # K_base + 2 > 4
        cgo.primalbarriermethodbatch(box, three, X0, cfg, ls, bc, params=[rows, rows, rows])
    with pytest.raises(cgo.CgoError, match="Backtracking") as e:
        cgo.primalbarriermethodbatch(box, "ObjQuadDiag", X0, cfg, ls, bc, (cfg, cgo.Backtracking(cgo.Armijo(1e-3), 0.9, 300, 50)), params=[rows])
    assert e.value.code == 1
    with pytest.raises(cgo.CgoError, match="L-BFGS"):
        cgo.primalbarriermethodbatch(box, "ObjQuadDiag", X0, cgo.setupCGConfig(1e-5, cgo.LBFGS(5), cgo.EnableTrace()), ls, bc, params=[rows])
    with pytest.raises(cgo.CgoError, match="Broyden"):
        cgo.primalbarriermethodbatch(box, "ObjQuadDiag", X0, cfg, ls, bc, (cgo.setupCGConfig(1e-5, cgo.setupBroydenFamily(1.0, 8), cgo.EnableTrace()), ls),
                                     params=[rows])
    with pytest.raises(ValueError, match="X_initial"):
        cgo.primalbarriermethodbatch(box, "ObjQuadDiag", np.ones(8), cfg, ls, bc, params=[rows])
    with pytest.raises(ValueError, match=r"params\[0\]"):
        cgo.primalbarriermethodbatch(box, "ObjQuadDiag", X0, cfg, ls, bc, params=[np.ones((3, 8))])
    # the three forms of a bound: one float, one row for all, a row per problem
    lb, ub = cgo.BatchBoxConstraints(-1.0, np.arange(16.0).reshape(2, 8)).rows(2, 8)
    assert lb.shape == ub.shape == (2, 8) and np.all(lb == -1.0) and ub[1, 3] == 11.0
    lb, ub = cgo.BoxConstraints(np.arange(8.0), 9.0).rows(2, 8)
    assert np.array_equal(lb[0], lb[1]) and lb[1, 7] == 7.0 and np.all(ub == 9.0)
    with pytest.raises(AssertionError):
        cgo.BatchBoxConstraints(np.zeros((3, 8)), 1.0).rows(2, 8)
    # every problem infeasible at its start: the answer needs no device either
    out = cgo.primalbarriermethodbatch(cgo.BoxConstraints(0.0, 1.0), "ObjQuadDiag", np.full((2, 8), 1.0), cfg, ls, bc, params=[rows])
    assert [r.status for r in out] == ["infeasible_start"] * 2 and all(r.iters_ran == 0 and r.centering_results == [] for r in out)
