#!/usr/bin/env python3
"""Many small fits at once, on YOUR objective, with a quasi-Newton direction: 256 robust location fits of n = 1000 residuals,

    f_b(x) = Σ_i w_bi (sqrt(1 + (x_i − y_bi)²) − 1)        (pseudo-Huber; slot 0 = the weights w_b, slot 1 = the data y_b)

— the body of examples/batch_fit.py — under LBFGS(5) and StrongWolfeBisection(1e-5, 0.5) to ϵ = 1e-5, through

    model = ElementwiseObjective(n, BODY, param=[None, None])
    rets = minimizeobjectivebatch_lbfgs_obj(model, X0, config, linesearch_config, params=[W, Y])      # W, Y: [batch, n]

One workgroup per problem runs the outer loop, the line search and the two-loop recursion on the device
(k_batch_lbfgs<UserObjective, 3>: a program of its own of the model's compiled module, built by the first such call); the ring
of 2(m+1) rows per problem lives in device memory.  A problem the device loop does not finish is solved again from its own
start, with its own slot rows, by the ordinary engine (`rets.handed_back`).

Part 1 prints the one-off compile time, then the wall time of the batched call and of the loop it replaces — set the two
parameter vectors, call minimizeobjective, 256 times on the same objective — in one process: medians of REPS repetitions after
one untimed, with min … max.
It also prints the same batch on a handle, `BatchLBFGS(model, [W, Y], batch, m)`: the slot rows go up once and the rows and
the ring stay allocated, so a solve is the reset, the launches and the results — and returns the one-shot call's bits.
Part 2 sweeps a regularisation strength PER PROBLEM through `scalars`: the same 32 data sets under 8 strengths λ_b in one call,

    f_b(x) = Σ_i w_bi (sqrt(1 + (x_i − y_bi)²) − 1) + ½ λ_b x_i²             (λ_b = s0 of problem b)

— and, beside it, the form a sweep takes when the strengths are not known together: ONE BatchLBFGS of the 32 data sets, solved 8
times, each time with `scalars` = one strength for all; and 8 one-shot calls of 32 problems, which upload the 32 data sets 8 times.

    python examples/batch_lbfgs_fit.py [max_iters] [once] [--rows device|lds|auto] [--batch-only] [--no-loop]
    # --no-loop: everything but the loop of 256 single solves
    # needs an MI355X; `once`: the batched call alone, one run (for a kernel trace); --rows lds: the problem's rows and ring in LDS
    # during a launch (k_batch_lbfgs_lds<UserObjective, 3>, one more program of the source), same bits
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import cgo_amd as cgo

N, BATCH, REPS, M = 1000, 256, 7, 5
BODY = "const double d = x - p1; const double r = __builtin_sqrt(1.0 + d*d); gi = p*(d/r); fi = p*(r - 1.0);"
RIDGE = "const double d = x - p1; const double r = __builtin_sqrt(1.0 + d*d); gi = p*(d/r) + s0*x; fi = p*(r - 1.0) + 0.5*((s0*x)*x);"
ROWS = "device"
if "--rows" in sys.argv:
    i = sys.argv.index("--rows")
    ROWS = sys.argv[i + 1]
    del sys.argv[i:i + 2]
BATCH_ONLY = "--batch-only" in sys.argv      # (the batched call's timing alone, without the loop it replaces)
if BATCH_ONLY:
    sys.argv.remove("--batch-only")
NO_LOOP = "--no-loop" in sys.argv
if NO_LOOP:
    sys.argv.remove("--no-loop")
max_iters = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
config = cgo.setupCGConfig(1e-5, cgo.LBFGS(M), cgo.EnableTrace(), max_iters=max_iters)
ls = cgo.setupStrongWolfeBisection(1e-5, 0.5)

rng = np.random.default_rng(24)
W = 0.5 + 3.5 * rng.random((BATCH, N))
Y = 4.0 * rng.random((BATCH, N)) - 2.0
X0 = 4.0 * rng.random((BATCH, N)) - 2.0


def timed(f, reps=REPS):
    f()   # (once untimed: allocations, first launch of the kernel)
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), min(ts), max(ts), r


def report(name, t, rets):
    med, lo, hi, _ = t
    its = np.array([r.iters_ran for r in rets])
    print(f"{name}: {med * 1e3:9.3f} ms ({lo * 1e3:.3f} … {hi * 1e3:.3f}); iterations per problem {its.min()} … {its.max()}, median {int(np.median(its))}, "
          f"sum {its.sum()}; statuses {sorted(set(r.status for r in rets))}")


t = time.perf_counter()
model = cgo.ElementwiseObjective(N, BODY, param=[None, None])
t_create = time.perf_counter() - t
t = time.perf_counter()
rets = cgo.minimizeobjectivebatch_lbfgs_obj(model, X0, config, ls, params=[W, Y], rows=ROWS)   # the first such call on the source: compiles its program
t_first = time.perf_counter() - t
print(f"creating the objective (every kernel of a single solve): {t_create:.2f} s; the first batched L-BFGS call, which compiles the program once "
      f"per source: {t_first:.2f} s; pairs per lane and trip with two slots: {cgo.batch_lbfgs_shape_obj(2)[1]}")
if len(sys.argv) > 2 and sys.argv[2] == "once":
    rets = cgo.minimizeobjectivebatch_lbfgs_obj(model, X0, config, ls, params=[W, Y], rows=ROWS)
    print(f"one batched call (rows in {rets.rows}): {rets.launches} launch(es), {rets.handed_back} handed back, {sum(r.iters_ran for r in rets)} iterations")
    model.close()
    sys.exit(0)

# ---- part 1: the batch against the loop of single solves ---------------------------------------------------------------------
tb = timed(lambda: cgo.minimizeobjectivebatch_lbfgs_obj(model, X0, config, ls, params=[W, Y], rows=ROWS))
rets = tb[3]
report(f"batched LBFGS({M}), {BATCH} fits, rows in {rets.rows}", tb, rets)
print(f"    {rets.launches} launch(es), {rets.handed_back} handed back to the host engine")
if BATCH_ONLY:
    model.close()
    sys.exit(0)
with cgo.BatchLBFGS(model, [W, Y], BATCH, M, rows=ROWS) as handle:
    th = timed(lambda: handle.solve(X0, config, ls))
report(f"the same on a BatchLBFGS handle (rows uploaded once, ring kept), rows in {th[3].rows}", th, th[3])
bits = all(np.array_equal(a.minimizer, b.minimizer) and np.array_equal(a.gradient, b.gradient) and a.objective == b.objective and
           np.array_equal(a.trace.grad_norm, b.trace.grad_norm) for a, b in zip(th[3], rets))
print(f"    handle against the one-shot call: {tb[0] / th[0]:.2f} x; every minimizer, gradient, objective and trace bit for bit the same: {bits}")


def loop():
    out = []
    for b in range(BATCH):
        model.set_param(W[b], slot=0)
        model.set_param(Y[b], slot=1)
        out.append(cgo.minimizeobjective(model, X0[b], config, ls))
    return out


if not NO_LOOP:
    tl = timed(loop, reps=3)
    report(f"loop of {BATCH} minimizeobjective calls, LBFGS({M})", tl, tl[3])
    K = 5
    same = sum(np.array_equal(a.trace.step_size[:K], b.trace.step_size[:K]) for a, b in zip(rets, tl[3]))
    worst = max(float(np.max(np.abs(a.minimizer - b.minimizer))) for a, b in zip(rets, tl[3]))
    print(f"    batch against that loop: {tl[0] / tb[0]:.1f} x; the first {K} accepted steps are identical in {same} of {BATCH} fits; "
          f"largest |x_batch − x_loop|: {worst:.2e}")
model.close()

# ---- part 2: a regularisation strength per problem ---------------------------------------------------------------------------
SETS, LAMBDAS = 32, np.array([0.0, 1e-3, 1e-2, 0.1, 0.3, 1.0, 3.0, 10.0])
idx = np.repeat(np.arange(SETS), len(LAMBDAS))            # problem b fits data set idx[b] under strength lam[b]
lam = np.tile(LAMBDAS, SETS)
ridge = cgo.ElementwiseObjective(N, RIDGE, param=[None, None])
t = time.perf_counter()
sweep = cgo.minimizeobjectivebatch_lbfgs_obj(ridge, X0[idx], config, ls, params=[W[idx], Y[idx]], scalars=lam, rows=ROWS)
t_first = time.perf_counter() - t
ts = timed(lambda: cgo.minimizeobjectivebatch_lbfgs_obj(ridge, X0[idx], config, ls, params=[W[idx], Y[idx]], scalars=lam, rows=ROWS))
report(f"{SETS} data sets × {len(LAMBDAS)} strengths in one call (first call {t_first:.2f} s)", ts, ts[3])
print(f"    {ts[3].launches} launch(es), {ts[3].handed_back} handed back")
for j, l in enumerate(LAMBDAS):
    rs = [ts[3][b] for b in range(len(lam)) if lam[b] == l]
    print(f"    λ = {l:6.3f}: mean |x̂| {np.mean([np.mean(np.abs(r.minimizer)) for r in rs]):.4f}, mean iterations {np.mean([r.iters_ran for r in rs]):.1f}, "
          f"largest |∇f| {max(float(np.linalg.norm(r.gradient)) for r in rs):.2e}")


# … the same sweep as 8 solves of the 32 data sets on ONE handle, a strength for all per solve, and as 8 one-shot calls
def by_strength(solve):
    out = [None] * len(lam)
    for j, l in enumerate(LAMBDAS):
        for b, r in enumerate(solve(np.full(SETS, l))):
            out[b * len(LAMBDAS) + j] = r
    return out


X0s, Ws, Ys = X0[:SETS], W[:SETS], Y[:SETS]
with cgo.BatchLBFGS(ridge, [Ws, Ys], SETS, M, rows=ROWS) as handle:
    tsh = timed(lambda: by_strength(lambda sc: handle.solve(X0s, config, ls, scalars=sc)))
tso = timed(lambda: by_strength(lambda sc: cgo.minimizeobjectivebatch_lbfgs_obj(ridge, X0s, config, ls, params=[Ws, Ys], scalars=sc, rows=ROWS)))
report(f"{len(LAMBDAS)} solves of {SETS} problems on one BatchLBFGS", tsh, tsh[3])
report(f"{len(LAMBDAS)} one-shot calls of {SETS} problems", tso, tso[3])
bits = all(np.array_equal(a.minimizer, b.minimizer) and np.array_equal(a.trace.grad_norm, b.trace.grad_norm) for a, b in zip(tsh[3], ts[3]))
print(f"    one handle against the one call of {len(lam)}: {ts[0] / tsh[0]:.2f} x; against the {len(LAMBDAS)} one-shot calls: {tso[0] / tsh[0]:.2f} x; "
      f"every problem's minimizer and trace as in the one call, bit for bit: {bits}")
ridge.close()
