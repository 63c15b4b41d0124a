"""The box-constrained problems of tests/test_batch_lbfgs_barrier.py (GPU tier) and tests/test_batch_lbfgs_barrier_oracle.py (CPU
tier): the problems of tests/_barrier_problems.py — the three bound forms, n ∈ (1, 2, 5, 64, 513), both t modes, five problems
a batch — under LBFGS(5) + WolfeBisection(Wolfe(1e-3, 0.9), 100, 1e12, 50) at ϵ = 1e-2, with that file's barrier_growth_factor,
barrier_tol rule and t_initial.  The reference is that file's: N.primalbarriermethod with N.make_boxhdh, problem by problem.

Replaced problems (the rule of tests/_barrier_problems.py: where the reference's own two restatements, or the existing single-call
primalbarriermethod on the GPU, miss the bar on a problem, the problem changes, not the bar; here at most one problem of any
(form, n, t mode) batch and at most 3 of the 150, each named with its measured miss — REPLACED below).  Both on the reference
alone, the numpy restatement against the C oracle, every status, count and accepted step equal, in the third centering step:
  ("shared", 513, "fixed")  b = 5 → b = 3.  b = 5 ends :success after 48 iterations there, with ∇f 1.2e-9, trace.grad_norm 5.5e-10
      and trace.objective 1.8e-11 apart, relative: the bar itself is missed on ∇f, a tenth of it (1e-10, 1e-11) on all three.
      b = 3 — the problem tests/_barrier_problems.py leaves out under Hager–Zhang — ends :success in 3 steps within the tenth.
  ("rows", 513, "fixed")    b = 2 → b = 5.  b = 2 ends :success after 63 iterations there, with ∇f 1.5e-10 and trace.grad_norm
      2.0e-11 apart: inside the bar, outside a tenth of it.  b = 5 ends :success in 3 steps within the tenth.
Under verifyt0 both batches stay tests/_barrier_problems.py's.

Six of the 150 do not end :success: their third centering step ends :cannot_find_feasible_step after 2 or 5 iterations, so the
problem ends :centering_step_issue — NOT_SUCCESS below.  They are kept: on the GPU the line-search outcome hands the problem
back to the host engine, with four slots and a scalar, from a handle whose slot rows are the only copy.

LBFGS(1): LBFGS1_BATCHES — n ≤ 64 only, and at n = 64 not the "rows" form.  Where the ring holds ONE pair the two restatements
part: at n = 513 by up to 2.8e-8 on x and 1.8e-3 on ∇f (shared b = 5, fixed t), on 13 of the 30 problems by more than a tenth of
the bar; at ("rows", 64) on three (b = 4 under verifyt0: ∇f 9.2e-10, trace.grad_norm 2.8e-10; b = 1 and b = 4 under the fixed t:
trace.grad_norm 1.5e-11 and 1.8e-11) — more than one problem of a batch, so the batch is left out, not patched.  On the batches
kept they agree to ≤ 3.3e-15 on x, ≤ 2.3e-11 on ∇f and ≤ 1.9e-12 on the trace.

Mixed outcomes in one batch (n = 64, [batch, n] bounds, verifyt0): tests/_barrier_problems.py's mixed_problems() and mixed_tol(),
centering stages of at most MIXED_M = 45 iterations, ONE rerun tuple of at most MIXED_R = 3, both LBFGS(5), three barrier
iterations — MIXED_EXPECT.  (At 40 iterations b4 fails too, and the batch loses its rerun-success case.)"""
import math
import types

import numpy as np

import _barrier_problems as P
from _cases import N

M = 5
INDICES = {("shared", 513, "fixed"): (0, 1, 2, 3, 4), ("rows", 513, "fixed"): (0, 1, 5, 3, 4)}
# (form, n, t mode): (the problem replaced, the figures of its third step that miss a tenth of the bar on the reference alone)
REPLACED = {("shared", 513, "fixed"): (5, ("gradient", "trace.grad_norm", "trace.objective")), ("rows", 513, "fixed"): (2, ("gradient", "trace.grad_norm"))}
# (form, n, t mode, b): :centering_step_issue in the third step, its stage :cannot_find_feasible_step after that many iterations
NOT_SUCCESS = {("shared", 513, "verifyt0", 5), ("shared", 513, "verifyt0", 4), ("shared", 513, "fixed", 0),
               ("rows", 513, "verifyt0", 1), ("rows", 513, "verifyt0", 2), ("rows", 513, "fixed", 0)}
TMODES = ("verifyt0", "fixed")
LBFGS1_BATCHES = [(form, n) for form in P.FORMS for n in (1, 2, 5, 64) if (form, n) != ("rows", 64)]


def problems(form, n, tmode, batch=P.BATCH):
    idx = INDICES.get((form, n, tmode))
    return P.problems(form, n, batch) if idx is None else [P.Prob(form, n, b) for b in idx[:batch]]


def np_configs(max_iters=1000, m=M):
    return N.CGConfig(P.EPS, N.LBFGS(m), max_iters), N.WolfeBisection(N.Wolfe(1e-3, 0.9), 100, 1e12, 50)


def as_out(r):
    """a `Results` of the numpy restatement with its traces as arrays, as assert_bar and `held` read them"""
    return types.SimpleNamespace(objective=r.objective, minimizer=r.minimizer, gradient=r.gradient, iters_ran=r.iters_ran, status=r.status,
                                 trace_objective=np.array(r.trace_objective, dtype=np.float64), trace_grad_norm=np.array(r.trace_grad_norm, dtype=np.float64),
                                 trace_step_size=np.array(r.trace_step_size, dtype=np.float64),
                                 trace_objective_evals=np.array(r.trace_objective_evals, dtype=np.int64))


_REF = {}


def reference_of(p, tmode, m=M):
    """the problem as one of its batch problems(form, n, tmode): once per problem, t mode and m, shared between the tests, never changed"""
    key = (p.form, p.n, p.b, tmode, m)
    if key not in _REF:
        _REF[key] = P.reference(p, P.t_initial(tmode, p.n), P.barrier_tol(problems(p.form, p.n, tmode), tmode), cfg_ls=np_configs(m=m))
    return _REF[key]


MIXED_M, MIXED_R, MIXED_BARRIER_ITERS = 45, 3, 3
MIXED_EXPECT = {"b1": ("centering_step_issue", 3), "outside": ("infeasible_start", 0), "b5": ("centering_step_issue", 3),
                "b4": ("success", 3), "halfway": ("max_iters_reached", 3), "b2": ("centering_step_issue", 3)}
_MIXED = {}


def mixed_reference(name, p, m_rerun=M):
    """(m_rerun: the rerun stage's own ring depth — the GPU tier runs a stage of m = 5 and one of m = 3 on one handle)"""
    if (name, m_rerun) not in _MIXED:
        cfg, ls = np_configs(MIXED_M)
        _MIXED[name, m_rerun] = P.reference(p, math.nan, P.mixed_tol(), barrier_max_iters=MIXED_BARRIER_ITERS, cfg_ls=(cfg, ls),
                                            reruns=((N.CGConfig(P.EPS, N.LBFGS(m_rerun), MIXED_R), ls),))
    return _MIXED[name, m_rerun]
