"""The problems of the batched L-BFGS tests, shared by the CPU tier (tests/test_batch_lbfgs_abi.py: the reference's own two
restatements must agree on every one of them to a tenth of the bar, and the CPU double of the device loop must meet the bar)
and the GPU tier (tests/test_batch_lbfgs.py).  Each entry of a list is one BATCH: cases of the same objective, size, config
and line search with their own x0 and D."""
import numpy as np

from _cases import Case, quad_D
from _suite import rosen_x0

QUAD_SIZES = (1, 2, 5, 64, 513, 1000)
QUAD_MS = (1, 4, 10)
ROSEN = ((2, 10), (32, 3), (64, 10), (1000, 3), (1000, 10))
BOOTH_STARTS = ([0.43, 1.23], [-2.0, 4.5], [3.0, 0.25])
BLOCK = 256   # lanes of a workgroup (cgo_batch_lbfgs_shape; asserted by both tiers)


def quad(n, b, m, **kw):
    """problem b of tests/test_batch.py's quad_problem recipe under LBFGS(m)"""
    kw = dict(dict(c2=0.9, eps=1e-9, max_iters=16), **kw)
    return Case(f"quad{n}-m{m}-b{b}", "quad_diag", n, np.ones(n) * (1 + b / 8), D=np.roll(quad_D(n), b) * 2.0 ** (b % 3 - 1), beta="LBFGS", m=m, **kw)


def rosen(n, b, m, **kw):
    """paired Rosenbrock from rosen_x0(n, seed = 7 + b), the jitter scaled with b (by 1 + b/16): seeds 8 and 10 give the same
    vector, so the plain recipe would put one problem into a batch twice"""
    kw = dict(dict(c2=0.5, max_iters=12), **kw)
    return Case(f"rosen{n}-m{m}-b{b}", "rosenbrock_paired", n, rosen_x0(n, jitter=0.01 * (1 + b / 16), seed=7 + b), beta="LBFGS", m=m, **kw)


def distinct_batches():
    out = [[quad(n, b, m) for b in range(4)] for n in QUAD_SIZES for m in QUAD_MS]
    out.append([quad(64, b, 5, max_iters=14, ls="WolfeBisection", cond="Wolfe", c1=1e-3, c2=0.9, ls_max_iters=100) for b in range(4)])
    out += [[rosen(n, b, m) for b in range(4)] for n, m in ROSEN]
    out.append([Case(f"booth-m3-b{b}", "booth", 2, np.array(x0), beta="LBFGS", m=3, max_iters=10) for b, x0 in enumerate(BOOTH_STARTS)])
    return out


def loop_pairs(block, u):
    return [1, block - 1, block, block + 1, u * block - 1, u * block, u * block + 1, 2 * u * block + block + 1]


def loop_batches(block, u):
    """every shape of the ring passes' loop, each with and without an odd tail: quadratics, m = 4, 8 iterations"""
    return [[quad(2 * p + odd, b, 4, max_iters=8) for b in range(3)] for p in loop_pairs(block, u) for odd in (0, 1)]


def wrap_batch():
    """m = 10 over 24 iterations: the ring of 11 slots wraps twice"""
    return [quad(64, b, 10, max_iters=24) for b in range(4)]


def many_batch():
    return [quad(5, b, 3, max_iters=8) for b in range(300)]


def mixed_quad(zoom_max_iters=100):
    """zoom_max_iters = 100: (ones, ones) lands on x = 0 with its first step, (zeros, D₀) starts at the minimizer, (ones, tile[1, 3])
    converges.  zoom_max_iters = 2: the two problems of tests/test_batch.py's mixed_hz whose FIRST line search gives up (the
    direction of iteration 1 is −g under any β) beside the first two"""
    n = 64
    D0 = quad_D(n)
    probs = [(np.ones(n), np.ones(n)), (np.zeros(n), D0), (np.ones(n), np.tile([1.0, 3.0], n // 2))]
    if zoom_max_iters == 2:
        probs = [(np.ones(n), D0), (3.0 * np.ones(n), np.roll(D0, 5))] + probs[:2]
    return [Case(f"mixed-quad-z{zoom_max_iters}-b{b}", "quad_diag", n, x0, D=D, beta="LBFGS", m=4, c2=0.9, eps=1e-5, max_iters=24, zoom_max_iters=zoom_max_iters)
            for b, (x0, D) in enumerate(probs)]


def mixed_rosen(max_iters=8):
    """seed 7 runs every iteration, seed 8's line search gives up in iteration 4 (:zoom_max_iters_reached).  8 iterations, not 12:
    after 12 the reference's own two restatements are 1.4e-11 apart on seed 7's trace, more than a tenth of the bar"""
    return [Case(f"mixed-rosen-seed{s}", "rosenbrock_paired", 64, rosen_x0(64, seed=s), beta="LBFGS", m=5, c2=0.1, zoom_max_iters=12, max_iters=max_iters)
            for s in (7, 8)]


def rows_batch():
    return [quad(513, b, 4) for b in range(4)]


def all_batches(block, u):
    return (distinct_batches() + loop_batches(block, u) + [wrap_batch(), many_batch()[:8], mixed_quad(), mixed_quad(2), mixed_rosen(), rows_batch()])
