#!/usr/bin/env python3
"""Many small fits at once, on YOUR objective: 256 robust location fits of n = 1000 residuals each,

    f_b(x) = Σ_i w_bi (sqrt(1 + (x_i − y_bi)²) − 1)        (pseudo-Huber; slot 0 = the weights w_b, slot 1 = the data y_b)

written as an element-wise body, compiled at run time, and solved through

    model = ElementwiseObjective(n, BODY, param=[None, None])        # the compiled source; its own slots stay unused
    rets = minimizeobjectivebatch(model, X0, config, linesearch_config, params=[W, Y])      # W, Y: [batch, n]

One workgroup per problem runs the reference's outer loop and line search on the device (k_batch for the model's objective: a
second program of its compiled module, built by the first batched call); a problem whose next iteration the device loop does
not run is finished by the ordinary engine.

Prints the one-off compile time of the batch program, then the wall time of the batched call for 256 problems and of the loop
it replaces — set the two parameter vectors, call minimizeobjective, 256 times on the same objective — in one process:
medians of REPS repetitions after one untimed.

    python examples/batch_fit.py [iterations]      # needs an MI355X
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import cgo_amd as cgo

N, BATCH, REPS = 1000, 256, 7
BODY = "const double d = x - p1; const double r = __builtin_sqrt(1.0 + d*d); gi = p*(d/r); fi = p*(r - 1.0);"
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 15
config = cgo.setupCGConfig(1e-200, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=iters)
ls = cgo.setupStrongWolfeBisection(1e-5, 0.1)

rng = np.random.default_rng(24)
W = 0.5 + 3.5 * rng.random((BATCH, N))
Y = 4.0 * rng.random((BATCH, N)) - 2.0
X0 = 4.0 * rng.random((BATCH, N)) - 2.0


def median_time(f):
    f()   # (once untimed: allocations, first launch of the kernel)
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), r


t = time.perf_counter()
model = cgo.ElementwiseObjective(N, BODY, param=[None, None])
t_create = time.perf_counter() - t
t = time.perf_counter()
max_n = cgo.batch_max_n(model)   # the first batched use of the source: compiles its batch program
t_compile = time.perf_counter() - t
t = time.perf_counter()
cgo.batch_max_n(model)
t_again = time.perf_counter() - t
print(f"creating the objective (every kernel of a single solve): {t_create:.2f} s; the batch program, once per source: {t_compile:.2f} s "
      f"(asked again: {t_again * 1e3:.3f} ms); largest n of one problem with two slots: {max_n}")

dt_batch, rets = median_time(lambda: cgo.minimizeobjectivebatch(model, X0, config, ls, params=[W, Y]))
done = sum(r.iters_ran for r in rets)
print(f"batch {BATCH:5d}: {dt_batch * 1e3:9.3f} ms, {done} iterations = {done / dt_batch:11.0f} it/s in aggregate; {rets.launches} launch(es), "
      f"{rets.handed_back} finished by the host engine; statuses {sorted(set(r.status for r in rets))}")


def loop():
    out = []
    for b in range(BATCH):
        model.set_param(W[b], slot=0)
        model.set_param(Y[b], slot=1)
        out.append(cgo.minimizeobjective(model, X0[b], config, ls))
    return out


dt_loop, single = median_time(loop)
done = sum(r.iters_ran for r in single)
print(f"loop of {BATCH} minimizeobjective calls: {dt_loop * 1e3:9.3f} ms, {done} iterations = {done / dt_loop:11.0f} it/s")
print(f"batch of {BATCH} against that loop: {dt_loop / dt_batch:.1f} x")
same = all(a.status == b.status and a.iters_ran == b.iters_ran and np.array_equal(a.trace.step_size, b.trace.step_size) for a, b in zip(rets, single))
worst = max(float(np.max(np.abs(a.minimizer - b.minimizer))) for a, b in zip(rets, single))
print(f"same statuses, iteration counts and accepted steps as the loop: {same}; largest |x_batch − x_loop|: {worst:.2e}")
model.close()
