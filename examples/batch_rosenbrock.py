#!/usr/bin/env python3
"""Many small problems at once: 256 copies of BASELINE config 1 — paired Rosenbrock, n = 1000, Polak–Ribière,
StrongWolfeBisection(1e-5, 0.1) — from perturbed starts, through

    rets = minimizeobjectivebatch("rosenbrock_paired", X0, config, linesearch_config)

One workgroup per problem runs the reference's outer loop and line search on the device (k_batch); a problem whose next
iteration the device loop does not run is finished by the ordinary engine.  `rets` is a list of the `Results` that
minimizeobjective returns for each problem; `rets.launches` and `rets.handed_back` say how the batch was paid for.

Prints the wall time of the batched call for 1, 256 and 1024 problems and of the loop it replaces — minimizeobjective called
256 times — in one process: medians of REPS repetitions.

    python examples/batch_rosenbrock.py [iterations]      # needs an MI355X
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import cgo_amd as cgo

N, REPS = 1000, 7
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 15   # (plain PR leaves the descent cone after ≈ 25 iterations from this start)
config = cgo.setupCGConfig(1e-200, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=iters)
ls = cgo.setupStrongWolfeBisection(1e-5, 0.1)


def starts(batch):
    return np.tile([-1.2, 1.0], N // 2) + 0.01 * (2.0 * np.random.default_rng(24).random((batch, N)) - 1.0)


def median_time(f):
    f()   # (once untimed: allocations, first launch of the kernel)
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), r


times = {}
for batch in (1, 256, 1024):
    X0 = starts(batch)
    dt, rets = median_time(lambda: cgo.minimizeobjectivebatch("rosenbrock_paired", X0, config, ls))
    done = sum(r.iters_ran for r in rets)
    times[batch] = dt
    print(f"batch {batch:5d}: {dt * 1e3:9.3f} ms, {done} iterations = {done / dt:11.0f} it/s in aggregate; {rets.launches} launch(es), "
          f"{rets.handed_back} finished by the host engine; statuses {sorted(set(r.status for r in rets))}")

X0 = starts(256)
obj = cgo.RosenbrockPaired(N)


def loop():
    return [cgo.minimizeobjective(obj, x0, config, ls) for x0 in X0]


dt, rets = median_time(loop)
done = sum(r.iters_ran for r in rets)
print(f"loop of 256 minimizeobjective calls: {dt * 1e3:9.3f} ms, {done} iterations = {done / dt:11.0f} it/s")
print(f"batch of 256 against that loop: {dt / times[256]:.1f} x")
one = cgo.minimizeobjectivebatch("rosenbrock_paired", X0, config, ls)
same = all(a.status == b.status and a.iters_ran == b.iters_ran and np.array_equal(a.trace.step_size, b.trace.step_size) for a, b in zip(one, rets))
print("same statuses, iteration counts and accepted steps as the loop:", same)
obj.close()
