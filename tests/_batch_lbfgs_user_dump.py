"""Solves the batches of tests/test_batch_lbfgs_user.py::ab_batches with the library CGO_LIB_PATH names and writes every
number of every result to an .npz — the other side of the test that the pairs per lane and trip change no bit.
usage: python _batch_lbfgs_user_dump.py OUT.npz"""
import sys

import numpy as np


def solve(cgo, ctx, probs, slice_iters=0):
    """the problems (one source, size, m and config) as ONE batched L-BFGS solve on a model of their source"""
    import _batch_lbfgs_user_problems as U
    from _cases import _product_structs
    p0 = probs[0]
    _, _, cfg, ls = _product_structs(p0.case())
    src, k = U.SOURCES[p0.name]
    param = None if k == 0 else (np.ones(p0.n) if k == 1 else [None] * k)   # (the model's own slots are neither read nor written)
    model = cgo.ElementwiseObjective(p0.n, src, param=param, ctx=ctx)
    try:
        X0 = np.stack([p.x0 for p in probs])
        params = [np.stack([p.slots[j] for p in probs]) for j in range(k)]
        scalars = None if p0.s0 is None else np.array([p.s0 for p in probs])
        return cgo.minimizeobjectivebatch_lbfgs_obj(model, X0, cfg, ls, params=params, scalars=scalars, ctx=ctx, slice_iters=slice_iters)
    finally:
        model.close()


def ab_batches():
    """two or more slots, sizes on both sides of every trip boundary of either pair count, a ring that wraps, a hand-back"""
    import _batch_lbfgs_user_problems as U
    out = [U.distinct("H2", 1000, 10), U.distinct("Q3", 513, 4), U.four_slots(), U.mixed_h2(), U.scalar_batch("SM", 513, 5)]
    out += [U.loop_batch("Q3", U.BLOCK, 2, which, 1) for which in (4, 6, 7)]
    return out


def flatten(out, tag, into):
    into[f"{tag}.counters"] = np.array([out.handed_back, len(out)])
    for b, r in enumerate(out):
        into[f"{tag}.{b}.scalars"] = np.array([r.objective, float(r.iters_ran), float(r.total_fdf_evals)])
        into[f"{tag}.{b}.status"] = np.array([r.status])
        into[f"{tag}.{b}.x"], into[f"{tag}.{b}.g"] = r.minimizer, r.gradient
        into[f"{tag}.{b}.tf"], into[f"{tag}.{b}.tg"] = r.trace.objective, r.trace.grad_norm
        into[f"{tag}.{b}.ta"], into[f"{tag}.{b}.te"] = r.trace.step_size, r.trace.objective_evals


def dump(cgo, ctx):
    into = {"shape": np.array(cgo.batch_lbfgs_shape_obj(2))}
    for i, probs in enumerate(ab_batches()):
        flatten(solve(cgo, ctx, probs), f"batch{i}", into)
    return into


if __name__ == "__main__":
    import cgo_amd
    np.savez(sys.argv[1], **dump(cgo_amd, cgo_amd.default_context()))
