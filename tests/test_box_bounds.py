"""Per-variable box bounds for primalbarriermethod: BoxConstraints(lb, ub) with length-D arrays (`lbs::Vector{T}`, `ubs::Vector{T}`
of examples/constrained.jl:22-31).  The bounds travel as the barrier objective's last two parameter vectors; the oracle's
make_boxhdh(lbs, ubs) has always taken vectors.  CPU tier: the generated source and the descriptor's validation; GPU tier: the
device objective against evalbarrier!, the whole method against the restatement, array bounds against scalar bounds."""
import math

import numpy as np
import pytest

from _cases import N, O
from test_primal_barrier import X0, _hold_centerings_to_the_restatement

LBS, UBS = np.array([-6.0, -9.0]), np.array([8.0, 14.0])        # each variable its own interval around X0 = (0.43, 1.23)

BASE2 = """
struct BaseObjective {                                         // ½ Σ w (x − b)², two parameter vectors of its own
    static constexpr int kParams = 2;
    static constexpr bool kPairOnly = false;
    __device__ static inline void eval1(double x, const double (&p)[2], double, double &f, double &g) {
        const double d = x - p[1];
        g = p[0]*d;
        f += 0.5*(g*d);
    }
    __device__ static inline void eval2(d2 x, const d2 (&p)[2], double s0, double &f, d2 &g) {
        const double pa[2] = {p[0].x, p[1].x}, pb[2] = {p[0].y, p[1].y};
        double g0, g1;
        eval1(x.x, pa, s0, f, g0);
        eval1(x.y, pb, s0, f, g1);
        g.x = g0; g.y = g1;
    }
};
"""
BASE3 = BASE2.replace("kParams = 2", "kParams = 3").replace("[2]", "[3]")


# ------------------------------------------------------------------------------------------- CPU tier
def test_scalar_bounds_keep_their_source(cgo):
    """Float bounds: the bounds are hex constants of the text, the functor has the one-slot interface — the text of before."""
    src = cgo.barrier_objective_source("ObjBooth", cgo.BoxConstraints(-10.0, 10.0))
    assert "kParams" not in src and "static constexpr bool kParam = B::kParam;" in src
    assert "const double hu = x - (0x1.4000000000000p+3), hl = (-0x1.4000000000000p+3) - x;" in src
    assert "eval1(double x, double p, double s0, double &f, double &g)" in src and "B::eval2(xx, pp, 0.0, f0, g0);" in src
    assert src == cgo.barrier_objective_source("ObjBooth", cgo.BoxConstraints(np.float64(-10.0), 10))
    assert not cgo.BoxConstraints(-10.0, 10.0).per_variable


def test_array_bounds_source_reads_the_last_two_slots(cgo):
    box = cgo.BoxConstraints(LBS, UBS)
    for base, kb in (("ObjBooth", 0), ("ObjQuadDiag", 1), (BASE2, 2)):
        src = cgo.barrier_objective_source(base, box)
        assert "0x1" not in src and "p+3" not in src                  # no baked bound constants
        assert "static constexpr int kParams = KB + 2;" in src and f"static_assert(KB == {kb}" in src
        assert "bar(x, p[KB], p[KB + 1], psi, dpsi);" in src and "const double hu = x - (ub), hl = (lb) - x;" in src
        assert "obj_eval2<B>(xx, pb, 0.0, f0, g0);" in src         # the base through the adaptor, old or new interface
        assert cgo.api.base_objective_params(base) == kb
    assert cgo.barrier_objective_source(BASE2, box).startswith(BASE2)
    with pytest.raises(AssertionError):
        cgo.barrier_objective_source(BASE3, box)                   # 3 + 2 > 4
    # the same bar() expression in both forms
    scalar = cgo.barrier_objective_source("ObjBooth", cgo.BoxConstraints(-10.0, 10.0))
    for line in ("const double cu = hu > 0.0 ? 0.0 : hu, cl = hl > 0.0 ? 0.0 : hl;", "psi = -(log(-cu) + log(-cl));",
                 "d -= 1.0 / cu;", "d -= -1.0 / cl;"):
        assert line in scalar and line in cgo.barrier_objective_source("ObjBooth", box)


def test_box_constraints_validation(cgo):
    box = cgo.BoxConstraints([-1.0, -2.0, -3.0], 4.0)              # one array, one float: the float holds for every variable
    assert box.per_variable and box.n_constraints(3) == 6
    lbs, ubs = box.vectors(3)
    assert np.array_equal(lbs, [-1.0, -2.0, -3.0]) and np.array_equal(ubs, [4.0, 4.0, 4.0]) and lbs.dtype == np.float64
    with pytest.raises(AssertionError):
        box.vectors(2)
    with pytest.raises(AssertionError):
        cgo.BoxConstraints([0.0, 0.0], [1.0, 1.0, 1.0])
    with pytest.raises(AssertionError):
        cgo.BoxConstraints(np.zeros((2, 2)), 1.0)
    cfg = cgo.setupCGConfig(1e-5, cgo.HagerZhang(), cgo.EnableTrace(), max_iters=10)
    ls = cgo.WolfeBisection(cgo.Wolfe(1e-3, 0.9), 100, 1e12, 50)
    bc = cgo.setupPrimalBarrierConfig(1e-8, 10.0, 3)
    with pytest.raises(AssertionError):                            # lengths differ from D: before anything touches a device
        cgo.primalbarriermethod(cgo.BoxConstraints(np.zeros(3), np.ones(3)), "ObjBooth", X0, cfg, ls, bc)
    with pytest.raises(AssertionError):                            # K_base + 2 > 4
        cgo.primalbarriermethod(cgo.BoxConstraints(LBS, UBS), BASE3, X0, cfg, ls, bc, param=[np.ones(2)] * 3)


def test_interface_is_declared(cgo):
    from cgo_amd import _lib
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/cgo.h", encoding="utf-8").read()
    for name in ("cgo_objective_create_from_source_ex", "cgo_objective_num_params", "cgo_objective_set_param_device"):
        assert f"int {name}(" in hdr and name in _lib.SIGNATURES


# ------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
def test_device_barrier_objective_with_array_bounds_matches_evalbarrier(cgo, gpu_ctx):
    """t·f0 + ψ with per-variable bounds from parameter slots 1 and 2 vs evalbarrier! over make_boxhdh(lbs, ubs)."""
    n = 1000
    D = O.fill_uniform(n, 5, 0.5, 3.0)
    lbs, ubs = O.fill_uniform(n, 8, -3.0, -2.0), O.fill_uniform(n, 9, 3.0, 5.0)
    src = cgo.barrier_objective_source("ObjQuadDiag", cgo.BoxConstraints(lbs, ubs))
    obj = cgo.ElementwiseObjective(n, src, param=[D, lbs, ubs])
    assert obj.n_params == 3
    con = N.CvxInequalityConstraint(2 * n, n)
    hdh = N.make_boxhdh(lbs, ubs)
    for seed, t in ((1, 1.0), (2, 37.5), (3, 1e6)):
        x = O.fill_uniform(n, seed, -1.9, 2.9)
        obj.set_scalar(t)
        g, g_ref = np.empty(n), np.empty(n)
        f = obj(g, x)
        f_ref = N.evalbarrier(con, g_ref, N.make_quad_diag(D), hdh, x, t)
        assert abs(f - f_ref) <= 1e-12 * abs(f_ref)
        assert np.allclose(g, g_ref, rtol=1e-14, atol=0)
    x = O.fill_uniform(n, 4, -1.9, 2.9)
    x[17] = ubs[17] + 0.5                         # outside ITS interval (inside its neighbours'): ψ = +Inf
    assert obj(np.empty(n), x) == math.inf
    obj.close()


def _configs(cgo):
    cfg = cgo.setupCGConfig(1e-5, cgo.HagerZhang(), cgo.EnableTrace(), max_iters=1000)
    lsW = cgo.WolfeBisection(cgo.Wolfe(1e-3, 0.9), 100, 1e12, 50)
    lsA = cgo.Backtracking(cgo.Armijo(1e-3), 0.9, 300, 50)
    cfgLS = cgo.setupCGConfig(1e-5, cgo.LiuStorrey(), cgo.EnableTrace(), max_iters=1000)
    cfgDFP = cgo.setupCGConfig(1e-5, cgo.setupBroydenFamily(1.0, 2), cgo.EnableTrace(), max_iters=1000)
    return cfg, lsW, ((cfgDFP, lsA), (cfgLS, lsW))


def _oracle_run(lbs, ubs):
    con = N.CvxInequalityConstraint(4, 2)
    cfg = N.CGConfig(1e-5, N.HagerZhang(), 1000)
    lsW = N.WolfeBisection(N.Wolfe(1e-3, 0.9), 100, 1e12, 50)
    lsA = N.Backtracking(N.Armijo(1e-3), 0.9, 300, 50)
    pairs = ((N.CGConfig(1e-5, N.BroydenFamily(1.0), 1000), lsA), (N.CGConfig(1e-5, N.LiuStorrey(), 1000), lsW))
    return N.primalbarriermethod(con, N.booth, N.make_boxhdh(lbs, ubs), X0, cfg, lsW, N.PrimalBarrierConfig(1e-8, 10.0, 100, math.nan), *pairs)


@pytest.mark.gpu
def test_primalbarriermethod_with_non_uniform_bounds(cgo, gpu_ctx):
    """The example problem (Booth, examples/constrained.jl) with every variable in its own interval: the device objective and the
    same solve through the closure contract, each held to the restatement centering by centering."""
    ref = _oracle_run(LBS, UBS)
    cfg, lsW, pairs = _configs(cgo)
    got = cgo.primalbarriermethod(cgo.BoxConstraints(LBS, UBS), "ObjBooth", X0, cfg, lsW, cgo.setupPrimalBarrierConfig(1e-8, 10.0, 100), *pairs)
    _hold_centerings_to_the_restatement(got.centering_results, ref)
    assert got.status in ("centering_step_issue", "success") and abs(got.iters_ran - ref.iters_ran) <= 2
    con = N.CvxInequalityConstraint(4, 2)
    hdh = N.make_boxhdh(LBS, UBS)
    t = N.booth(np.empty(2), np.array(X0)) * 10.0
    rets = []
    for _ in range(4):
        rets.append(cgo.minimizeobjectivererun(lambda g, x, t=t: N.evalbarrier(con, g, N.booth, hdh, x, t), np.array(X0), cfg, lsW, *pairs))
        t *= 10.0
    _hold_centerings_to_the_restatement(rets, ref)
    assert cgo.primalbarriermethod(cgo.BoxConstraints(LBS, UBS), "ObjBooth", [0.43, 14.0], cfg, lsW,
                                   cgo.setupPrimalBarrierConfig(1e-8, 10.0, 100)).status == "infeasible_start"


@pytest.mark.gpu
def test_arrays_of_equal_bounds_take_the_scalar_forms_steps(cgo, gpu_ctx):
    """Arrays filled with −10 / 10: the same bar() expression on loaded instead of literal bounds — the same statuses, iteration
    counts and step sequence as BoxConstraints(−10.0, 10.0)."""
    cfg, lsW, pairs = _configs(cgo)
    bc = cgo.setupPrimalBarrierConfig(1e-8, 10.0, 100)
    a = cgo.primalbarriermethod(cgo.BoxConstraints(-10.0, 10.0), "ObjBooth", X0, cfg, lsW, bc, *pairs)
    b = cgo.primalbarriermethod(cgo.BoxConstraints(np.full(2, -10.0), np.full(2, 10.0)), "ObjBooth", X0, cfg, lsW, bc, *pairs)
    assert a.status == b.status and a.iters_ran == b.iters_ran and a.t_final == b.t_final
    assert a.total_objective_evals == b.total_objective_evals
    for ra, rb in zip(a.centering_results, b.centering_results):
        assert [r.status for r in ra] == [r.status for r in rb] and [r.iters_ran for r in ra] == [r.iters_ran for r in rb]
        for x, y in zip(ra, rb):
            assert np.array_equal(x.trace.step_size, y.trace.step_size) and np.array_equal(x.trace.objective_evals, y.trace.objective_evals)


def _large_problem():
    n = 10001
    D = O.fill_uniform(n, 6, 1.0, 10.0)
    return n, D, O.fill_uniform(n, 7, 0.25, 0.75), O.fill_uniform(n, 8, 3.0, 5.0)


def _barrier_closure(D, lbs, ubs, t):
    """evalbarrier! (primal_barrier.jl:70-128) over make_boxhdh(lbs, ubs) without its dense 2D × D Jacobian: the same clamp, the
    same ψ and the same two terms of ∇ψ per coordinate, in O(D) — what lets the oracle's engine run this size."""
    def fdf(g, x):
        g0 = D * x
        f0 = float(np.sum(0.5 * (g0 * x)))
        hu, hl = x - ubs, lbs - x
        cu, cl = np.where(hu > 0.0, 0.0, hu), np.where(hl > 0.0, 0.0, hl)
        with np.errstate(divide="ignore", invalid="ignore"):
            psi = -float(np.sum(np.log(-cu) + np.log(-cl)))
            g[:] = t * g0 + (-(1.0 / cu) + 1.0 / cl)
        return t * f0 + psi
    return fdf


def _oracle_barrier_blocks(D, lbs, ubs, x, t, g, B=1000):
    """the restatement's own evalbarrier! — block by block, the objective being separable"""
    f = 0.0
    for lo in range(0, x.size, B):
        sl = slice(lo, min(lo + B, x.size))
        m = sl.stop - sl.start
        gb = np.empty(m)
        f += N.evalbarrier(N.CvxInequalityConstraint(2 * m, m), gb, N.make_quad_diag(D[sl]), N.make_boxhdh(lbs[sl], ubs[sl]), x[sl], t)
        g[sl] = gb
    return f


def test_large_problem_closure_is_the_oracles_evalbarrier():
    """CPU tier: the O(D) closure the large test hands the oracle's engine equals evalbarrier! over make_boxhdh, value and gradient."""
    n, D, lbs, ubs = _large_problem()
    for seed, t in ((1, 1.0), (2, 10.0)):
        x = lbs + (ubs - lbs) * O.fill_uniform(n, seed, 0.05, 0.95)
        g, g_ref = np.empty(n), np.empty(n)
        f, f_ref = _barrier_closure(D, lbs, ubs, t)(g, x), _oracle_barrier_blocks(D, lbs, ubs, x, t, g_ref)
        assert abs(f - f_ref) <= 1e-13 * abs(f_ref) and np.allclose(g, g_ref, rtol=1e-14, atol=0)


@pytest.mark.gpu
def test_primalbarriermethod_large_with_array_bounds(cgo, gpu_ctx):
    """ObjQuadDiag base (its D in slot 0, the bounds in slots 1 and 2) at n = 10⁴ + 1, every variable its own interval whose lower
    end (0.25 … 0.75) lies above the unconstrained minimiser 0.  Outcome class and final objective of every centering against the
    oracle's engine on the same barrier objective.  With the oracle: the first centre (t = 1) is a :success and a stationary point
    inside the box; the second (t = 10, restarted from x_initial = 1 like every one: primal_barrier.jl:172,214) ends after ONE
    iteration in :cannot_find_feasible_step — the steepest-descent step that is feasible for the variable nearest its bound
    no longer meets the Wolfe test — so the method returns :centering_step_issue after two centerings."""
    n, D, lbs, ubs = _large_problem()
    cfg = cgo.setupCGConfig(1e-5, cgo.HagerZhang(), cgo.EnableTrace(), max_iters=500)
    ls = cgo.WolfeBisection(cgo.Wolfe(1e-3, 0.9), 100, 1e12, 50)
    r = cgo.primalbarriermethod(cgo.BoxConstraints(lbs, ubs), "ObjQuadDiag", np.ones(n), cfg, ls,
                                cgo.setupPrimalBarrierConfig(1e-3, 10.0, 12, t_initial=1.0), param=D)
    refs, t = [], 1.0
    for _ in range(12):                                            # the method's loop (primal_barrier.jl:208-240) on the oracle's engine
        refs.append(N.minimizeobjective(_barrier_closure(D, lbs, ubs, t), np.ones(n), N.CGConfig(1e-5, N.HagerZhang(), 500),
                                        N.WolfeBisection(N.Wolfe(1e-3, 0.9), 100, 1e12, 50)))
        if refs[-1].status != "success" or 2 * n / t < 1e-3:
            break
        t *= 10.0
    ref_status = "centering_step_issue" if refs[-1].status != "success" else "success"
    assert refs[0].status == "success" and len(refs) == 2 and ref_status == "centering_step_issue"
    assert r.status == ref_status and r.iters_ran == len(refs) == len(r.centering_results)
    for k, ref in enumerate(refs):
        assert len(r.centering_results[k]) == 1
        res, t = r.centering_results[k][0], 10.0 ** k
        xs = res.minimizer
        assert res.status == ref.status and abs(res.iters_ran - ref.iters_ran) <= 2, (k, res.status, res.iters_ran, ref.status, ref.iters_ran)
        assert np.all(xs > lbs) and np.all(xs < ubs)
        assert abs(res.objective - ref.objective) <= 1e-10 * abs(ref.objective), k
        # (both stop at ‖∇‖ ≤ 1e-5 where ∇² ⪰ t·D ⪰ 1: each within 1e-5 of the centre, ‖x‖ ≈ 90 — 1e-6·‖x‖ ≈ 9e-5 covers the two)
        assert np.linalg.norm(xs - ref.minimizer) <= 1e-6 * np.linalg.norm(ref.minimizer), k
        f_at = _oracle_barrier_blocks(D, lbs, ubs, xs, t, np.empty(n))   # evalbarrier! itself at the device's centre
        assert abs(res.objective - f_at) <= 1e-10 * abs(f_at), k
    xs = r.centering_results[0][0].minimizer                       # the first centre: t·D·x = 1/(x − lb) − 1/(ub − x)
    resid = D * xs - (1.0 / (xs - lbs) - 1.0 / (ubs - xs))
    assert np.linalg.norm(resid) <= 1e-4 * max(1.0, np.linalg.norm(D * xs))
