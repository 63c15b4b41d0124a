#!/usr/bin/env python3
"""Many small fits WITH BOUNDS at once, with a quasi-Newton direction: the 256 box-constrained robust location fits of
examples/batch_box_fit.py (n = 1000 residuals each, every variable of every problem its own interval),

    minimise  f_b(x) = Σ_i w_bi (sqrt(1 + (x_i − y_bi)²) − 1)   subject to   lb_bi < x_i < ub_bi

by the primal barrier method (primal_barrier.jl:156-255) on all problems together, every centering step under LBFGS(5):

    outs = primalbarriermethodbatch_lbfgs(BatchBoxConstraints(LB, UB), BASE, X0, centering_config, linesearch_config, barrier_config,
                                          params=[W, Y])                            # LB, UB, X0, W, Y: [batch, n]

Every stage of every centering step is ONE BatchLBFGS.solve with scalars = t and active = the problems still running, on ONE
handle: the rows of w, y, lb, ub go to the device once, the ring of 2(m+1) rows per problem is allocated once.

Prints, in one process, medians of REPS repetitions after one untimed (min … max), each with its centering steps and iterations:
  1. that call;
  2. the loop it replaces — primalbarriermethod, 256 times, under the same LBFGS(5) (LOOP_REPS repetitions);
  3. primalbarriermethodbatch under Hager–Zhang on the same problems: the quasi-Newton direction is no promise of fewer
     iterations on these well-scaled fits;
  4. the same three on ONE ill-conditioned batch — the weights of each problem spread over three decades — reported whichever
     way it comes out (measured, DESIGN.md §2.14: every centering restart from x_initial fails there under either direction).

    python examples/batch_lbfgs_box_fit.py [--rows device|lds|auto] [--no-loop]      # needs an MI355X
"""
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import cgo_amd as cgo

N, BATCH, REPS, LOOP_REPS, M = 1000, 256, 3, 1, 5
ROWS = "device"
if "--rows" in sys.argv:
    i = sys.argv.index("--rows")
    ROWS = sys.argv[i + 1]
    del sys.argv[i:i + 2]
NO_LOOP = "--no-loop" in sys.argv
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
lbfgs = cgo.setupCGConfig(1e-5, cgo.LBFGS(M), cgo.EnableTrace(), max_iters=1000)
hz = cgo.setupCGConfig(1e-5, cgo.HagerZhang(), cgo.EnableTrace(), max_iters=1000)
ls = cgo.WolfeBisection(cgo.Wolfe(1e-3, 0.9), 100, 1e12, 50)             # examples/constrained.jl:81-86

rng = np.random.default_rng(24)
# (the data of examples/batch_box_fit.py: weights scaled so that the barrier weight t·w of a variable is the same at every n)
W = (0.5 + 3.5 * rng.random((BATCH, N))) * 0.5 / math.sqrt(40.0 * N)
Y = 2.6 * rng.random((BATCH, N)) - 1.3
LB = -1.5 + 0.5 * rng.random((BATCH, N))
UB = 1.0 + 0.5 * rng.random((BATCH, N))
X0 = 1.8 * rng.random((BATCH, N)) - 0.9
# the ill-conditioned batch: the same data, every problem's weights spread over three decades with the same geometric mean
W_ILL = W * 10.0 ** (3.0 * rng.random((BATCH, N)) - 1.5)


def barrier_config_of(Wv):
    f0 = np.sum(Wv * (np.sqrt(1.0 + (X0 - Y) ** 2) - 1.0), axis=1)
    return cgo.PrimalBarrierConfig(2.0 * N / (10.0 ** 1.5 * float(np.median(10.0 * f0))), 10.0, 8, math.nan, 0.0)   # the third step ends it


def timed(f, reps):
    f()   # (once untimed: compiles, allocations, first launches)
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), min(ts), max(ts), r


def report(name, t, outs):
    med, lo, hi, _ = t
    its = sum(r.iters_ran for o in outs for s in o.centering_results for r in s)
    stat = {s: sum(o.status == s for o in outs) for s in sorted(set(o.status for o in outs))}
    print(f"{name}: {med * 1e3:10.3f} ms ({lo * 1e3:.3f} … {hi * 1e3:.3f}); {sum(o.iters_ran for o in outs)} centering steps "
          f"({min(o.iters_ran for o in outs)}–{max(o.iters_ran for o in outs)} per problem), {its} iterations in all; statuses {stat}")
    return its


# one objective of each text kept alive: the library shares a compiled module between objectives of the same text while one of
# them lives, so nothing compiles in the timed repetitions
keep = [cgo.ElementwiseObjective(N, cgo.barrier_objective_source(BASE, cgo.BoxConstraints(LB[0], UB[0])), param=[None] * 4),
        cgo.ElementwiseObjective(N, cgo.api._base_objective_source(BASE), param=[None] * 2)]
box = cgo.BatchBoxConstraints(LB, UB)
for name, Wv in (("well-scaled weights", W), ("weights over three decades", W_ILL)):
    bc = barrier_config_of(Wv)
    print(f"---- {BATCH} fits of n = {N}, {name} ----")
    tq = timed(lambda: cgo.primalbarriermethodbatch_lbfgs(box, BASE, X0, lbfgs, ls, bc, params=[Wv, Y], rows=ROWS), REPS)
    iq = report(f"primalbarriermethodbatch_lbfgs, LBFGS({M}), rows in {ROWS}", tq, tq[3])
    tc = timed(lambda: cgo.primalbarriermethodbatch(box, BASE, X0, hz, ls, bc, params=[Wv, Y], rows="device" if ROWS == "device" else "auto"), REPS)
    ic = report("primalbarriermethodbatch, Hager–Zhang             ", tc, tc[3])
    print(f"    L-BFGS against Hager–Zhang, batched: {tc[0] / tq[0]:.2f} x in time, {iq} against {ic} iterations")
    if not NO_LOOP:
        tl = timed(lambda: [cgo.primalbarriermethod(cgo.BoxConstraints(LB[b], UB[b]), BASE, X0[b], lbfgs, ls, bc, param=[Wv[b], Y[b]]) for b in range(BATCH)], LOOP_REPS)
        report(f"loop of {BATCH} primalbarriermethod calls, LBFGS({M})  ", tl, tl[3])
        same = sum(a.status == b.status and a.iters_ran == b.iters_ran and
                   all(x.status == y.status and x.iters_ran == y.iters_ran for sa, sb in zip(a.centering_results, b.centering_results) for x, y in zip(sa, sb))
                   for a, b in zip(tq[3], tl[3]))
        ok = [(a, b) for a, b in zip(tq[3], tl[3]) if a.centering_results and b.centering_results]
        worst = max(float(np.max(np.abs(a.centering_results[-1][-1].minimizer - b.centering_results[-1][-1].minimizer))) for a, b in ok)
        print(f"    batch against that loop: {tl[0] / tq[0]:.1f} x; same statuses, centering steps and iteration counts in {same} of {BATCH} fits; "
              f"largest |x_batch − x_loop|: {worst:.2e}")
for o in keep:
    o.close()
