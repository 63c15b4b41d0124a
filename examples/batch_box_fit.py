#!/usr/bin/env python3
"""Many small fits WITH BOUNDS at once: 256 box-constrained robust location fits of n = 1000 residuals each,

    minimise  f_b(x) = Σ_i w_bi (sqrt(1 + (x_i − y_bi)²) − 1)   subject to   lb_bi < x_i < ub_bi

(the pseudo-Huber objective of examples/batch_fit.py; every variable of every problem its own interval), by the primal barrier
method (primal_barrier.jl:156-255) on all problems together:

    outs = primalbarriermethodbatch(BatchBoxConstraints(LB, UB), BASE, X0, centering_config, linesearch_config, barrier_config,
                                    params=[W, Y])                                  # LB, UB, X0, W, Y: [batch, n]

The barrier weight t differs from problem to problem (verifyt0: t = 10 f0(x0)), so every centering step is ONE batched solve
with a scalar per problem (Batch.solve(..., scalars=t, active=…)); the rows of w, y, lb, ub go to the device once.

Prints the wall time of that call for 256 problems and of the loop it replaces — primalbarriermethod, 256 times, on the same
data — in one process: medians of REPS repetitions after one untimed, with the centering steps and launches taken.

    python examples/batch_box_fit.py      # needs an MI355X
"""
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import cgo_amd as cgo

N, BATCH, REPS = 1000, 256, 7
BASE = """
struct BaseObjective {
    static constexpr int kParams = 2;                                  // slot 0 = the weights w, slot 1 = the data y
    static constexpr bool kParam = true;
    static constexpr bool kPairOnly = false;
    __device__ static inline void eval1(double x, const double (&p)[2], double, double &f, double &g) {
        const double d = x - p[1];
        const double r = __builtin_sqrt(1.0 + d * d);
        g = p[0] * (d / r);
        f += p[0] * (r - 1.0);
    }
    __device__ static inline void eval2(d2 x, const d2 (&p)[2], double, double &f, d2 &g) {
        const double d0 = x.x - p[1].x, d1 = x.y - p[1].y;
        const double r0 = __builtin_sqrt(1.0 + d0 * d0), r1 = __builtin_sqrt(1.0 + d1 * d1);
        g.x = p[0].x * (d0 / r0);
        g.y = p[0].y * (d1 / r1);
        f += p[0].x * (r0 - 1.0);
        f += p[0].y * (r1 - 1.0);
    }
};
"""
config = cgo.setupCGConfig(1e-5, cgo.HagerZhang(), cgo.EnableTrace(), max_iters=1000)
ls = cgo.WolfeBisection(cgo.Wolfe(1e-3, 0.9), 100, 1e12, 50)             # examples/constrained.jl:81-86

rng = np.random.default_rng(24)
# weights scaled so that the barrier weight t·w of a variable is the same at every n (t = 10 f0(x0) grows as sqrt(n)): every
# centering step restarts from x_initial (primal_barrier.jl:172), and the restart is only well-conditioned while t·w stays moderate
W = (0.5 + 3.5 * rng.random((BATCH, N))) * 0.5 / math.sqrt(40.0 * N)
Y = 2.6 * rng.random((BATCH, N)) - 1.3                                    # a few targets per problem lie outside their interval
LB = -1.5 + 0.5 * rng.random((BATCH, N))
UB = 1.0 + 0.5 * rng.random((BATCH, N))
X0 = 1.8 * rng.random((BATCH, N)) - 0.9
f0 = np.sum(W * (np.sqrt(1.0 + (X0 - Y) ** 2) - 1.0), axis=1)
barrier_config = cgo.PrimalBarrierConfig(2.0 * N / (10.0 ** 1.5 * float(np.median(10.0 * f0))), 10.0, 8, math.nan, 0.0)   # the third step ends it


def median_time(f):
    f()   # (once untimed: compiles, allocations, first launches)
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), r


def launches(outs):
    """per problem: the launches of every stage it was part of — a batched stage counts once for each of its problems"""
    return [sum(r.total_launches for step in o.centering_results for r in step) for o in outs]


# one objective of each text kept alive: the library shares a compiled module between objectives of the same text while one of
# them lives, so neither the batched call nor the loop compiles anything in the timed repetitions
keep = [cgo.ElementwiseObjective(N, cgo.barrier_objective_source(BASE, cgo.BoxConstraints(LB[0], UB[0])), param=[None] * 4),
        cgo.ElementwiseObjective(N, cgo.api._base_objective_source(BASE), param=[None] * 2)]

dt_batch, outs = median_time(lambda: cgo.primalbarriermethodbatch(cgo.BatchBoxConstraints(LB, UB), BASE, X0, config, ls, barrier_config, params=[W, Y]))
steps = sum(o.iters_ran for o in outs)
stage_solves = sum(len(step) for step in max(outs, key=lambda o: o.iters_ran).centering_results)
print(f"batch {BATCH:5d}: {dt_batch * 1e3:9.3f} ms; {steps} centering steps in all ({min(o.iters_ran for o in outs)}–{max(o.iters_ran for o in outs)} per problem), "
      f"{sum(r.iters_ran for o in outs for s in o.centering_results for r in s)} iterations; ≈ {stage_solves} batched solves, "
      f"{max(launches(outs))} k_batch launches on the longest problem's path; statuses {sorted(set(o.status for o in outs))}")


def loop():
    return [cgo.primalbarriermethod(cgo.BoxConstraints(LB[b], UB[b]), BASE, X0[b], config, ls, barrier_config, param=[W[b], Y[b]]) for b in range(BATCH)]


dt_loop, single = median_time(loop)
print(f"loop of {BATCH} primalbarriermethod calls: {dt_loop * 1e3:9.3f} ms; {sum(o.iters_ran for o in single)} centering steps, "
      f"{sum(launches(single))} launches in all; statuses {sorted(set(o.status for o in single))}")
print(f"batch of {BATCH} against that loop: {dt_loop / dt_batch:.1f} x")
same = all(a.status == b.status and a.iters_ran == b.iters_ran and
           all(x.status == y.status and x.iters_ran == y.iters_ran and np.array_equal(x.trace.step_size, y.trace.step_size)
               for sa, sb in zip(a.centering_results, b.centering_results) for x, y in zip(sa, sb)) for a, b in zip(outs, single))
worst = max(float(np.max(np.abs(a.centering_results[-1][-1].minimizer - b.centering_results[-1][-1].minimizer))) for a, b in zip(outs, single))
print(f"same statuses, centering steps, iteration counts and accepted steps as the loop: {same}; largest |x_batch − x_loop|: {worst:.2e}")
for o in keep:
    o.close()
