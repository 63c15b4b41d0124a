#!/usr/bin/env python3
"""Batched solves beyond one workgroup's LDS: 64 (then 256) quadratic problems of n = 50 000 — Polak–Ribière,
StrongWolfeBisection(1e-5, 0.1), 15 iterations each — through

    rets = minimizeobjectivebatch("quad_diag", X0, config, linesearch_config, D=D, rows="device")

rows="device" keeps every problem's rows of x, u and D in device memory and streams them in every pass of the device loop
(k_batch_rows), one workgroup per problem; rows="lds" (the default) holds them in the workgroup's LDS and ends at
batch_max_n("quad_diag") = 6 704.  `rets.rows` says which tier ran.

Prints, in one process, medians of REPS repetitions after one untimed run, with the spread (min … max):
  1. the batch of 64, and (l) the loop it replaces — 64 minimizeobjective calls on the same objectives — with whether statuses,
     iteration counts and accepted steps equal the loop's;
  2. the same batch at 256 problems (the rows then exceed what the Infinity Cache holds);
  3. what LDS buys: examples/batch_rosenbrock.py's 256 problems of n = 1000 under rows="lds" and rows="device".

    python examples/batch_rows.py [iterations] [parts, e.g. 1l or 12 or 3]      # needs an MI355X
"""
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import cgo_amd as cgo

N, REPS = 50000, 7
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 15
parts = sys.argv[2] if len(sys.argv) > 2 else "1l23"
config = cgo.setupCGConfig(1e-200, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=iters)
ls = cgo.setupStrongWolfeBisection(1e-5, 0.1)


def problems(batch):
    rng = np.random.default_rng(24)
    return 1.0 + 0.5 * rng.random((batch, N)), 1.0 + 999.0 * rng.random((batch, N))   # X0, the rows of D


def timed(f):
    f()   # (once untimed: allocations, first launch of the kernel)
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), min(ts), max(ts), r


def passes(rets):
    """passes over the rows, estimated from the evaluations: the initial one, one per iteration (accept + direction + the next
    line search's first three trial points) and one per further three trial points of a line search"""
    return sum(1 + r.iters_ran + sum(max(0, math.ceil((int(e) - 3) / 3)) for e in r.trace.objective_evals) for r in rets)


print(f"pairs per lane and trip of the streaming loop: {cgo.batch_rows_shape()[1]}; batch_max_n('quad_diag') = {cgo.batch_max_n('quad_diag')}")
t64 = None
for batch in [b for b, p in ((64, "1"), (256, "2")) if p in parts]:
    X0, D = problems(batch)
    dt, lo, hi, rets = timed(lambda: cgo.minimizeobjectivebatch("quad_diag", X0, config, ls, D=D, rows="device"))
    done, p = sum(r.iters_ran for r in rets), passes(rets)
    gb = p * N * 8 * 3 / 1e9 + done * N * 8 * 2 / 1e9   # x, u, D read per pass; x, u stored per accepted step
    print(f"rows={rets.rows} batch {batch:4d} of n = {N}: {dt * 1e3:9.3f} ms ({lo * 1e3:.3f} … {hi * 1e3:.3f}), {done} iterations = "
          f"{done / dt:9.0f} it/s in aggregate; {rets.launches} launch(es), {rets.handed_back} finished by the host engine; "
          f"≈ {p} passes, ≈ {gb:.2f} GB streamed by the kernel; statuses {sorted(set(r.status for r in rets))}")
    if batch == 64:
        t64, r64, X64, D64 = dt, rets, X0, D

if "1" in parts and "l" in parts:
    objs = [cgo.QuadDiag(d) for d in D64]
    dt, lo, hi, loop = timed(lambda: [cgo.minimizeobjective(o, x0, config, ls) for o, x0 in zip(objs, X64)])
    done = sum(r.iters_ran for r in loop)
    print(f"loop of 64 minimizeobjective calls: {dt * 1e3:9.3f} ms ({lo * 1e3:.3f} … {hi * 1e3:.3f}), {done} iterations = {done / dt:9.0f} it/s")
    print(f"batch of 64 with rows in device memory against that loop: {dt / t64:.1f} x")
    same = all(a.status == b.status and a.iters_ran == b.iters_ran and np.array_equal(a.trace.step_size, b.trace.step_size) for a, b in zip(r64, loop))
    print("same statuses, iteration counts and accepted steps as the loop:", same)
    for o in objs:
        o.close()

if "3" in parts:
    n = 1000
    X0 = np.tile([-1.2, 1.0], n // 2) + 0.01 * (2.0 * np.random.default_rng(24).random((256, n)) - 1.0)
    t = {}
    for rows in ("lds", "device", "lds", "device"):
        dt, lo, hi, rets = timed(lambda: cgo.minimizeobjectivebatch("rosenbrock_paired", X0, config, ls, rows=rows))
        t.setdefault(rows, []).append(dt)
        print(f"rows={rets.rows:6s} 256 paired Rosenbrocks of n = {n}: {dt * 1e3:9.3f} ms ({lo * 1e3:.3f} … {hi * 1e3:.3f})")
    print(f"what LDS buys at n = {n}: rows=\"device\" takes {min(t['device']) / min(t['lds']):.2f} x the time of rows=\"lds\"")
