#!/usr/bin/env python3
"""Many small problems at once with a quasi-Newton direction: 256 paired-Rosenbrock problems of n = 1000 under LBFGS(5) and
StrongWolfeBisection(1e-5, 0.5), run to ϵ = 1e-5 from perturbed starts, through

    rets = minimizeobjectivebatch_lbfgs("rosenbrock_paired", X0, config, linesearch_config)

One workgroup per problem runs the outer loop, the line search and the two-loop recursion on the device (k_batch_lbfgs); the
ring of 2(m+1) rows per problem lives in device memory.  A problem the device loop does not finish is solved again from its
own start by the ordinary engine (`rets.handed_back`).

Times three things in one process — medians of REPS repetitions after one untimed run, with min … max:
    the batched call;
    the loop it replaces: minimizeobjective called 256 times with the same config;
    the existing batched Polak–Ribière solve of the same problems to the same ϵ (minimizeobjectivebatch).

    python examples/batch_lbfgs.py [max_iters] [once] [--rows device|lds|auto] [--batch-only] [--m M] [--n N]
    # needs an MI355X; `once`: the batched call alone, one run (for a kernel trace); --rows lds: the problem's rows and ring in LDS
    # during a launch (k_batch_lbfgs_lds; n ≤ batch_lbfgs_max_n(kind, m=M, rows="lds"), e.g. --m 3 --n 1800), same bits
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import cgo_amd as cgo

N, BATCH, REPS, M = 1000, 256, 7, 5


def option(name, default):
    """--name value, taken out of sys.argv"""
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return default


ROWS, M, N = option("--rows", "device"), int(option("--m", M)), int(option("--n", N))
BATCH_ONLY = "--batch-only" in sys.argv      # (the batched call's timing alone, without the loop it replaces)
if BATCH_ONLY:
    sys.argv.remove("--batch-only")
max_iters = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
config = cgo.setupCGConfig(1e-5, cgo.LBFGS(M), cgo.EnableTrace(), max_iters=max_iters)
config_pr = cgo.setupCGConfig(1e-5, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=max_iters)
ls = cgo.setupStrongWolfeBisection(1e-5, 0.5)
ls_pr = cgo.setupStrongWolfeBisection(1e-5, 0.1)   # (the curvature condition examples/batch_rosenbrock.py runs Polak–Ribière under)
X0 = np.tile([-1.2, 1.0], N // 2) + 0.01 * (2.0 * np.random.default_rng(24).random((BATCH, N)) - 1.0)


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


if len(sys.argv) > 2 and sys.argv[2] == "once":
    rets = cgo.minimizeobjectivebatch_lbfgs("rosenbrock_paired", X0, config, ls, rows=ROWS)
    print(f"one batched call (rows in {rets.rows}): {rets.launches} launch(es), {rets.handed_back} handed back, {sum(r.iters_ran for r in rets)} iterations")
    sys.exit(0)

tb = timed(lambda: cgo.minimizeobjectivebatch_lbfgs("rosenbrock_paired", X0, config, ls, rows=ROWS))
rets = tb[3]
report(f"batched LBFGS({M}), {BATCH} problems of n = {N}, rows in {rets.rows}", tb, rets)
print(f"    {rets.launches} launch(es), {rets.handed_back} handed back to the host engine; largest n with the rows and the ring in LDS for m = {M}: "
      f"{cgo.batch_lbfgs_max_n('rosenbrock_paired', m=M, rows='lds')}")
if BATCH_ONLY:
    sys.exit(0)

obj = cgo.RosenbrockPaired(N)
tl = timed(lambda: [cgo.minimizeobjective(obj, x0, config, ls) for x0 in X0], reps=3)
report(f"loop of {BATCH} minimizeobjective calls, LBFGS({M})", tl, tl[3])
obj.close()
# (the two run the same algorithm with differently ordered sums: over a hundred iterations of a line search that branches on ϕ and dϕ
#  the trajectories part, so only the first steps can be compared — the tests hold the batch to the reference over short horizons)
K = 10
same = sum(np.array_equal(a.trace.step_size[:K], b.trace.step_size[:K]) for a, b in zip(rets, tl[3]))
print(f"    batch against that loop: {tl[0] / tb[0]:.1f} x; the first {K} accepted steps are identical in {same} of {BATCH} problems")

for name, lsp in (("the same line search", ls), ("StrongWolfeBisection(1e-5, 0.1), this flavour's usual one", ls_pr)):
    tp = timed(lambda: cgo.minimizeobjectivebatch("rosenbrock_paired", X0, config_pr, lsp))
    report(f"batched Polak–Ribière (rows in LDS), {name}", tp, tp[3])
    print(f"    {tp[3].launches} launch(es), {tp[3].handed_back} handed back; wall time against the batched L-BFGS: {tp[0] / tb[0]:.2f} x")
