"""The box-constrained problems of tests/test_batch_barrier.py (GPU tier) and tests/test_batch_barrier_oracle.py (CPU tier), and
their reference: N.primalbarriermethod (oracle/cgo_oracle_np.py) with N.make_boxhdh and the base objective as a closure, problem
by problem.

Base objectives, both separable quadratics, u = fill_uniform(n, 3 + 10b, 0.5, 4) and s_n = 1 / sqrt(40 n):
  QD   the built-in ObjQuadDiag, f0 = ½ Σ D x², D = 0.2 s_n u (K_base = 1) — with ONE box for all, [0.25, 3]: the unconstrained
       minimiser 0 lies below it, every lower bound is active at the optimum; x0 = fill_uniform(n, 4 + 10b, 0.5, 2.5);
  BQ2  f0 = ½ Σ p (x − p1)², p = 0.5 s_n u, as a `struct BaseObjective` with kParams = 2 — with per-variable bounds lb = fill_uniform(n,
       8 + 10b, −1.5, −1), ub = fill_uniform(n, 9 + 10b, 1, 1.5) and targets p1 = fill_uniform(n, 5 + 10b, −1.3, 1.3): the bounds of
       the variables whose target lies outside their interval are active, a few per problem; x0 = fill_uniform(n, 4 + 10b, −0.9, 0.9).
Why s_n.  Every centering step restarts from x_initial (primal_barrier.jl:172), and its line searches share ONE step among all
variables: with a weight t·p of a variable's quadratic against its barrier terms much above 100 the restart ends
:cannot_find_feasible_step sooner or later (tried on the restatement: t·p = 400 at n ≥ 64).  verifyt0 gives t = 10 f0(x0), which
grows with n for data of a fixed scale; with s_n it grows as sqrt(n) and t·p is the same at every n: ≤ 0.25 at the first
step, ≤ 25 at the third (with p = s_n u, t·p ≈ 90 at the third step of n = 513: two of five restarts failed on the restatement).

Configs: HagerZhang + WolfeBisection(Wolfe(1e-3, 0.9), 100, 1e12, 50) as examples/constrained.jl:81-86, 1000 iterations, ϵ = 1e-2.
Why not the example's ϵ = 1e-5: at a centre the gradient t ∇f0 + ∇ψ is a difference of terms of size up to 25 (and curvatures
up to ≈ 600) that cancel to below ϵ, so two runs whose x differ in the last bit differ in that gradient by ≈ 1e-14 — relative to
‖∇‖ < 1e-5 that is ≈ 1e-9, at the bar's 1e-9 for ∇f and above its 1e-10 for trace.grad_norm.  The existing primalbarriermethod,
one call per problem on the GPU, matched every status, count and step of the restatement at ϵ = 1e-5 and missed exactly those
two figures on 24 of 156 problems (1.1e-10 … 1e-8, once 3e-6 on a last gradient of norm ≈ 1e-8), and at ϵ = 1e-3 still on one
(∇f 1.4e-9 at n = 513, after 70 iterations); the problems were changed, not the bar.
barrier_growth_factor = 10; barrier_tol(problems) = 2n / (10^1.5 · the median t of the batch's first step): 2n / t < barrier_tol
first holds at the THIRD step for every problem whose first t lies within half a decade of the median — all of them for n ≥ 64;
a single variable's f0(x0) can be anything, so the small sizes take 2 to 5.  Fixed form: t_initial = 5.6 sqrt(n / 40) (QD: the same)."""
import math

import numpy as np

from _cases import N, O

BQ2 = """
struct BaseObjective {
    static constexpr int kParams = 2;
    static constexpr bool kParam = true;
    static constexpr bool kPairOnly = false;
    __device__ static inline void eval1(double x, const double (&p)[2], double, double &f, double &g) {
        const double d = x - p[1];
        g = p[0] * d;
        f += 0.5 * (g * d);
    }
    __device__ static inline void eval2(d2 x, const d2 (&p)[2], double, double &f, d2 &g) {
        const double d0 = x.x - p[1].x, d1 = x.y - p[1].y;
        g.x = p[0].x * d0;
        g.y = p[0].y * d1;
        f += 0.5 * (g.x * d0);
        f += 0.5 * (g.y * d1);
    }
};
"""
MU = 10.0
EPS = 1e-2   # the centering tolerance ‖∇(t f0 + ψ)‖ < ϵ (see the docstring)
FORMS = ("scalar", "shared", "rows")   # one box for all (floats) | one set of bounds for all (length-n) | [batch, n]
SIZES = (1, 2, 5, 64, 513)
BATCH = 5


class Prob:
    """one box-constrained problem: base source, its own rows, bounds (length-n arrays, whatever form they travel in), x0"""

    def __init__(self, form, n, b):
        self.form, self.n, self.b = form, n, b
        p = O.fill_uniform(n, 3 + 10 * b, 0.5, 4.0) / math.sqrt(40.0 * n)
        if form == "scalar":
            self.base, self.rows = "ObjQuadDiag", (0.2 * p,)
            self.lb, self.ub = np.full(n, 0.25), np.full(n, 3.0)
            self.x0 = O.fill_uniform(n, 4 + 10 * b, 0.5, 2.5)
        else:
            self.base, self.rows = BQ2, (0.5 * p, O.fill_uniform(n, 5 + 10 * b, -1.3, 1.3))
            bb = 0 if form == "shared" else b          # "shared": every problem has problem 0's bounds
            self.lb, self.ub = O.fill_uniform(n, 8 + 10 * bb, -1.5, -1.0), O.fill_uniform(n, 9 + 10 * bb, 1.0, 1.5)
            self.x0 = O.fill_uniform(n, 4 + 10 * b, -0.9, 0.9)

    def f0df0(self):
        r = self.rows
        if len(r) == 1:
            return N.make_quad_diag(r[0])

        def fdf(g, x):
            d = x - r[1]
            g[:] = r[0] * d
            return float(np.sum(0.5 * (g * d)))
        return fdf

    @property
    def name(self):
        return f"{self.form}-n{self.n}-b{self.b}"


# b = 3 of ("shared", 513) is left out for b = 5: with the fixed t its third centering step ends, after 70 iterations, on a
# gradient that the existing single-call primalbarriermethod on the GPU and the restatement give 1.3e-9 apart (ϵ = 1e-2; 1.4e-9
# at 1e-3) — every count and step equal, the bar's 1e-9 for ∇f missed by a third.  Changed the problem, not the bar.
INDICES = {("shared", 513): (0, 1, 2, 5, 4)}


def problems(form, n, batch=BATCH):
    return [Prob(form, n, b) for b in INDICES.get((form, n), range(BATCH))[:batch]]


def t_initial(tmode, n):
    return math.nan if tmode == "verifyt0" else 5.6 * math.sqrt(n / 40.0)


def first_t(p, tmode):
    return N.verifyt0(t_initial(tmode, p.n), p.x0, p.f0df0(), MU, 0.0)


def barrier_tol(probs, tmode):
    return 2.0 * probs[0].n / (10.0 ** 1.5 * float(np.median([first_t(p, tmode) for p in probs])))


def np_configs(max_iters=1000):
    return N.CGConfig(EPS, N.HagerZhang(), max_iters), N.WolfeBisection(N.Wolfe(1e-3, 0.9), 100, 1e12, 50)


def reference(p, t0, tol, barrier_max_iters=8, cfg_ls=None, reruns=()):
    """N.primalbarriermethod on problem p"""
    cfg, ls = cfg_ls or np_configs()
    con = N.CvxInequalityConstraint(2 * p.n, p.n)
    return N.primalbarriermethod(con, p.f0df0(), N.make_boxhdh(p.lb, p.ub), p.x0, cfg, ls, N.PrimalBarrierConfig(tol, MU, barrier_max_iters, t0), *reruns)


_REF = {}


def reference_of(p, tmode):
    """the problem as one of its batch problems(form, n): computed once per problem and t mode, shared between the tests, never changed"""
    key = (p.form, p.n, p.b, tmode)
    if key not in _REF:
        _REF[key] = reference(p, t_initial(tmode, p.n), barrier_tol(problems(p.form, p.n), tmode))
    return _REF[key]


# ---- mixed outcomes in one batch (n = 64, [batch, n] bounds, verifyt0) ---------------------------------------------------------
# Centering steps of at most MIXED_M = 40 iterations, ONE rerun tuple of at most MIXED_R = 3, three barrier iterations, the tolerance
# of problems("rows", 64).  On the restatement, with every step unlimited: the ordinary problems b = 1, 2 need ≤ 24 iterations a
# step and end :success in 3 steps without a rerun; b = 5 needs 44 in its second step — the rerun stage runs for it alone and
# finishes it in 2 more; b = 4 needs 47 in its third step and 3 more in the rerun stage, one more than that stage has (the stop
# test counts the iteration it is about to start, optim.jl:162): both stages end :max_iters_reached, :centering_step_issue;
# "halfway" (b = 0 started halfway to its targets: t = 0.96 against ≈ 3.3; ≤ 32 iterations a step) has not reached the tolerance
# after three steps, :max_iters_reached; "outside" starts with one variable above its upper bound, :infeasible_start.
# (A first choice for the exhausted problem, p spread over three decades, parted from the restatement in its evaluation counts
# on the GPU — in the existing single-call primalbarriermethod too: an ill-conditioned problem that never converges is knife-edge.)
MIXED_N, MIXED_M, MIXED_R, MIXED_BARRIER_ITERS = 64, 40, 3, 3
MIXED_EXPECT = {"b1": ("success", 3), "outside": ("infeasible_start", 0), "b5": ("success", 3), "b4": ("centering_step_issue", 3),
                "halfway": ("max_iters_reached", 3), "b2": ("success", 3)}


def mixed_problems():
    n = MIXED_N
    out = {"b1": Prob("rows", n, 1), "outside": Prob("rows", n, 6), "b5": Prob("rows", n, 5), "b4": Prob("rows", n, 4),
           "halfway": Prob("rows", n, 0), "b2": Prob("rows", n, 2)}
    out["outside"].x0[3] = out["outside"].ub[3] + 0.1
    q = out["halfway"]
    q.x0 = 0.5 * q.x0 + 0.5 * np.clip(q.rows[1], q.lb + 0.25, q.ub - 0.25)
    return out


def mixed_tol():
    return barrier_tol(problems("rows", MIXED_N), "verifyt0")


def mixed_reference(p):
    cfg, ls = np_configs(MIXED_M)
    return reference(p, math.nan, mixed_tol(), barrier_max_iters=MIXED_BARRIER_ITERS, cfg_ls=(cfg, ls),
                     reruns=((N.CGConfig(EPS, N.HagerZhang(), MIXED_R), ls),))
