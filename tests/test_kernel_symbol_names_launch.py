"""GPU: kernel_symbol(kind) names the instantiation a launch of that kind runs.  bench.py matches a profile summary to the running
kernel through kernel_symbol, and the launch decides path, grid and instantiation on its own — both now ask the same plan
(HipBackend::r_plan, fused_symbol, csrc/cgo_launch_kinds.hpp), and this holds them together through the public API alone.

Kinds: those whose mode does not depend on the state of a solve (accept_dir_trial of the k_cg family alternates with the lazy /
replay launches).  n = 1026: pairs, more than one wave, an even count.  Every solver runs once with the policy's hbm_stream_bytes
below every launch's byte count, once between them (8·n·3.5: launches of up to three vectors stay grid-stride, the others stream)
and once above all, so both values of the pure-HBM bit are seen without a large allocation.  kernel_symbol is read before the
first probe: a probed solver is no longer eligible for the lazy direction."""
import numpy as np
import pytest

import _instances as I

B = I.BITS
N = 1026
THRESHOLDS = (1.0, 8.0 * N * 3.5, 1e15)
# kind → (default mode, trial steps of the probe: 0, 1, "max" = max_points, "max3" = min(max_points, 3))
CG_KINDS = {"init": (B["R_INIT"], 0), "trial": (B["R_TRIAL"], "max3"), "accept_dir": (B["R_ACCEPT"] | B["R_DIR"], 0),
            "accept_only": (B["R_ACCEPT"], 0), "reset_dir": (B["R_RESET"], 0), "upg_norm": (B["R_UPG"], 0),
            "dir_trial": (B["R_DIR"] | B["R_TRIAL"], "max"), "sys_project": (B["R_PROJ"], 1)}
FUSED_KINDS = {"init": 0, "trial": 1, "accept_dir_trial": 1, "accept_dir": 0, "accept_only": 0, "reset_dir": 0, "upg_norm": 0}
STEPS = [0.25, 0.125, 0.5, 0.0625, 0.375, 0.03125, 0.75]


def _vectors():
    rng = np.random.default_rng(1026)
    return {k: rng.uniform(-1.0, 1.0, N) for k in ("x", "u", "aux")}, rng.uniform(1.0, 2.0, N)


def _check(cgo, make_objective, beta, kinds, points, stored, seen):
    v, _ = _vectors()
    for thr in THRESHOLDS:
        o = make_objective()
        pol = cgo.SolverPolicy(stored_gradient=stored, resident=False, controller_depth=0, points=points, hbm_stream_bytes=thr)
        s = cgo.Solver(o, cgo.setupCGConfig(1e-9, beta, cgo.DisableTrace(), max_iters=5), cgo.setupStrongWolfeBisection(1e-5, 0.1), pol)
        try:
            named = {kind: s.kernel_symbol(kind) for kind in kinds}
            for kind, k in kinds.items():
                k = {"max": points, "max3": min(points or 1, 3)}.get(k, k)
                got = s.probe_launch(kind, 0, 0.5, 0.25, STEPS[:k], v["x"], v["u"], v["aux"])["symbol"]
                assert named[kind] and named[kind] == got, (kind, thr, named[kind], got)
                seen.setdefault(kind, set()).add(got.endswith("true>"))
        finally:
            s.close(); o.close()
    assert all(bits == {False, True} for bits in seen.values()), seen


@pytest.mark.gpu
@pytest.mark.parametrize("beta_name", ["PolakRibiere", "LBFGS"])
def test_stored_gradient_family(cgo, beta_name):
    """k_fused on ObjQuadDiag: policy stored_gradient under a CG β (trials carry the β sums), and L-BFGS (they do not)"""
    _, D = _vectors()
    _check(cgo, lambda: cgo.QuadDiag(D), getattr(cgo, beta_name)(), FUSED_KINDS, None, True, {})


@pytest.mark.gpu
def test_k_cg_family(cgo):
    _, D = _vectors()
    _check(cgo, lambda: cgo.QuadDiag(D), cgo.PolakRibiere(), {k: steps for k, (_, steps) in CG_KINDS.items()}, 7, False, {})


@pytest.mark.gpu
def test_k_chain_family(cgo):
    """the stencil objective: the kinds whose mode has a k_chain row (no dir_trial, no solvesystem); three points at most"""
    rows = {mode for mode, _ in I.rows("CHAIN")}
    kinds = {k: steps for k, (mode, steps) in CG_KINDS.items() if mode in rows}
    assert sorted(kinds) == ["accept_dir", "accept_only", "init", "reset_dir", "trial", "upg_norm"]
    _check(cgo, lambda: cgo.RosenbrockChained(N), cgo.PolakRibiere(), kinds, 3, False, {})
