"""Host-side mirror of ConjugateGradientOptim.jl's interface for the hot path.

Same names, argument meaning and error behaviour as the reference module
(src/ConjugateGradientOptim.jl:23-29 exports + the qualified names used by
examples/min.jl and examples/constrained.jl), so that parity tests read like
the reference's own usage:

    config = setupCGConfig(1e-5, HagerZhang(), EnableTrace(); max_iters=1000)
    ls     = setupStrongWolfeBisection(1e-5, 0.8; a_max_growth_factor=2.0, ...)
    ret    = minimizeobjective(fdf!, x0, config, ls)
    ret.minimizer, ret.objective, ret.status, ret.trace.objective_evals ...

The one deliberate difference: `fdf!` is a *device objective descriptor*
(QuadDiag, RosenbrockPaired, Booth, ...) instead of a host closure, because the
element-wise f/∇f runs inside the fused HIP kernels.  Passing a Python callable
raises TypeError — there is no CPU path in this package.

All numerical work happens in lib/libcgo_hip.so behind include/cgo.h; this file
only marshals arguments.  The Julia binding (julia/ConjugateGradientOptimAMD.jl)
is the same thin layer over the same symbols.
"""
from __future__ import annotations

import ctypes as C
import math
import re
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Union

import numpy as np

from . import _lib
from ._lib import BetaConfig, CGConfigC, LSConfigC, LSSConfigC, ResultsC, check, dp, i64p

# ---------------------------------------------------------------------------
# trace traits (src/types.jl:9-11)
# ---------------------------------------------------------------------------


class TraceTrait:
    pass


class EnableTrace(TraceTrait):
    def __repr__(self):
        return "EnableTrace()"


class DisableTrace(TraceTrait):
    def __repr__(self):
        return "DisableTrace()"


# ---------------------------------------------------------------------------
# βConfig subtypes (src/types.jl:5-7, src/cg_flavours.jl, src/qn_flavours.jl)
# ---------------------------------------------------------------------------


class βConfig:
    _kind = -1

    def _c(self) -> BetaConfig:
        return BetaConfig(self._kind, 0, 0.0)

    def __repr__(self):
        return type(self).__name__ + "()"


class CGβConfig(βConfig):
    pass


class QNβConfig(βConfig):
    pass


class HagerZhang(CGβConfig):  # cg_flavours.jl:83
    _kind = 0


class YuanWangSheng(CGβConfig):  # cg_flavours.jl:46-48
    _kind = 1

    def __init__(self, μ: float):
        self.μ = float(μ)

    def _c(self):
        return BetaConfig(self._kind, 0, self.μ)

    def __repr__(self):
        return f"YuanWangSheng({self.μ})"


class SallehAlhawarat(CGβConfig):  # cg_flavours.jl:130
    _kind = 2


class LiuStorrey(CGβConfig):  # cg_flavours.jl:154
    _kind = 3


class PolakRibiere(CGβConfig):  # new (stub at cg_flavours.jl:173-174)
    _kind = 4


class HestenesStiefel(CGβConfig):  # new (commented at cg_flavours.jl:110-127)
    _kind = 5


class DaiYuan(CGβConfig):  # new
    _kind = 6


class LBFGS(QNβConfig):  # new QNβConfig behind the contract of qn_flavours.jl:5-48
    _kind = 7

    def __init__(self, m: int = 10):
        self.m = int(m)

    def _c(self):
        return BetaConfig(self._kind, self.m, 0.0)

    def __repr__(self):
        return f"LBFGS({self.m})"


class BroydenFamily(QNβConfig):
    """BroydenFamily{T}(θ, B)  (src/qn_flavours.jl:53-66).  The reference's update computes s = B\\y first
    (:81), so Bs = y, sBs = s·y, v = 0 and B_new = B up to rounding (:83-87): B stays the identity it is
    initialised to and the direction B\\(−g) is steepest descent for every θ.  The engine therefore runs
    u = −g exactly (no n×n matrix, no O(n³) solves); the oracle carries the dense algebra."""
    _kind = 8

    def __init__(self, θ: float):
        self.θ = float(θ)

    def _c(self):
        return BetaConfig(self._kind, 0, self.θ)

    def __repr__(self):
        return f"BroydenFamily({self.θ})"


def setupBroydenFamily(θ: float, N: int) -> BroydenFamily:
    """setupBroydenFamily(θ, N)  (qn_flavours.jl:55-66): `@assert zero(T) <= θ`; the N×N matrix is never built."""
    if not (0.0 <= θ):
        raise AssertionError("AssertionError: zero(T) <= θ  (qn_flavours.jl:57)")
    return BroydenFamily(θ)


# ---------------------------------------------------------------------------
# CGConfig (src/types.jl:156-203)
# ---------------------------------------------------------------------------
@dataclass
class CGConfig:
    ϵ: float
    β_config: βConfig
    max_iters: int
    verbose: bool
    trace_status: TraceTrait

    def _c(self) -> CGConfigC:
        return CGConfigC(self.ϵ, self.β_config._c(), self.max_iters, int(self.verbose),
                         1 if isinstance(self.trace_status, EnableTrace) else 0)


def setupCGConfig(ϵ: float, β_config: βConfig, trace_status: TraceTrait, *, max_iters: int = 1000,
                  verbose: bool = False) -> CGConfig:
    """setupCGConfig(ϵ, β_config, trace_status; max_iters=1000, verbose=false)  (types.jl:171-203)."""
    cfg = CGConfig(float(ϵ), β_config, int(max_iters), bool(verbose), trace_status)
    c = cfg._c()
    check(_lib.lib().cgo_check_cg_config(C.byref(c)))  # @assert zero(T) < ϵ < one(T)
    return cfg


# ---------------------------------------------------------------------------
# line-search configs (src/linesearch/nocedal.jl:3-30, wolfe.jl:6-11,213-217,259-262)
# ---------------------------------------------------------------------------
class LineSearchConfig:
    pass


@dataclass
class StrongWolfeBisection(LineSearchConfig):
    c1: float
    c2: float
    a_max_growth_factor: float
    max_iters: int
    zoom_max_iters: int

    def _c(self) -> LSConfigC:
        return LSConfigC(0, 0, self.c1, self.c2, self.a_max_growth_factor, 0.0, 0.0,
                         self.max_iters, self.zoom_max_iters, 0, 0.0)


def setupStrongWolfeBisection(c1: float, c2: float, *, a_max_growth_factor: float = 2.0,
                              max_iters: int = 1000, zoom_max_iters: int = 100) -> StrongWolfeBisection:
    """setupStrongWolfeBisection(c1, c2; ...)  (nocedal.jl:14-30) incl. its @asserts."""
    ls = StrongWolfeBisection(float(c1), float(c2), float(a_max_growth_factor), int(max_iters),
                              int(zoom_max_iters))
    c = ls._c()
    check(_lib.lib().cgo_check_ls_config(C.byref(c)))
    return ls


@dataclass
class Wolfe:  # wolfe.jl:259-262
    c1: float
    c2: float


@dataclass
class YuanWeiLuWolfe:  # wolfe.jl:213-217
    c1: float
    c2: float
    δ1: float


@dataclass
class WolfeBisection(LineSearchConfig):
    """WolfeBisection(condition, max_iters, max_step_size, feasibility_max_iters)  (wolfe.jl:6-11).

    Like the reference's raw constructor this does not validate; the condition's
    @assert (wolfe.jl:233,278) fires when the solve starts."""
    condition: object
    max_iters: int
    max_step_size: float
    feasibility_max_iters: int

    def _c(self) -> LSConfigC:
        cond = self.condition
        if isinstance(cond, YuanWeiLuWolfe):
            return LSConfigC(1, 1, cond.c1, cond.c2, 2.0, cond.δ1, self.max_step_size,
                             self.max_iters, 0, self.feasibility_max_iters, 0.0)
        if isinstance(cond, Wolfe):
            return LSConfigC(1, 0, cond.c1, cond.c2, 2.0, 0.0, self.max_step_size, self.max_iters,
                             0, self.feasibility_max_iters, 0.0)
        raise TypeError("WolfeBisection.condition must be Wolfe or YuanWeiLuWolfe")


@dataclass
class Armijo:  # geometric.jl:159-162
    c1: float


@dataclass
class Backtracking(LineSearchConfig):
    """Backtracking(condition, discount_factor, max_iters, feasibility_max_iters)  (geometric.jl:15-20).

    Restated bug for bug (geometric.jl:77-78,141-144): on :success the previous (ϕ, a) is returned while
    the adopted iterate/gradient are those of the last, rejected trial — exactly what the reference does."""
    condition: Armijo
    discount_factor: float
    max_iters: int
    feasibility_max_iters: int

    def _c(self) -> LSConfigC:
        if not isinstance(self.condition, Armijo):
            raise TypeError("Backtracking.condition must be Armijo")
        return LSConfigC(2, 2, self.condition.c1, 0.0, 2.0, 0.0, 0.0, self.max_iters, 0,
                         self.feasibility_max_iters, self.discount_factor)


def evalwolfeconditions(condition, ϕ_a: float, dϕ_a: float, a: float, u, ϕ_0: float, dϕ_0: float):
    """evalwolfeconditions(condition, ϕ_a, dϕ_a, a, u, ϕ_0, dϕ_0) → (valid_large, valid_small)  (wolfe.jl:219-294).
    `u` is the search direction or — since only YuanWeiLuWolfe reads it, and only as dot(u,u) (:240) — that scalar."""
    uu = float(u) if np.isscalar(u) else float(np.dot(np.asarray(u, dtype=np.float64), np.asarray(u, dtype=np.float64)))
    ls = WolfeBisection(condition, 1, 1.0, 1)._c()
    v1, v2 = C.c_int32(0), C.c_int32(0)
    check(_lib.lib().cgo_evalwolfeconditions(C.byref(ls), ϕ_a, dϕ_a, a, uu, ϕ_0, dϕ_0, C.byref(v1), C.byref(v2)))
    return bool(v1.value), bool(v2.value)


def evalbacktrackcondition(condition: Armijo, ϕ_a: float, a: float, ϕ_0: float, dϕ_0: float) -> bool:
    """evalbacktrackcondition(::Armijo, ϕ_a, a, ϕ_0, dϕ_0)  (geometric.jl:164-186)."""
    ls = Backtracking(condition, 0.5, 1, 1)._c()
    v = C.c_int32(0)
    check(_lib.lib().cgo_evalbacktrackcondition(C.byref(ls), ϕ_a, a, ϕ_0, dϕ_0, C.byref(v)))
    return bool(v.value)


@dataclass
class LinesearchSolveSys:
    """LinesearchSolveSys{T}(ρ, σ, s, max_iters)  (solve_system.jl:6-11): the line search of
    solvesystem — eqn 18 of (Yuan 2019): first s·ρ^i with −g(z)ᵀu ≥ σ·a·‖g(z)‖·‖u‖²."""
    ρ: float
    σ: float
    s: float
    max_iters: int

    def _c(self) -> LSSConfigC:
        return LSSConfigC(self.ρ, self.σ, self.s, self.max_iters)


def setupLinesearchSolveSys(s: float, σ: float = 0.5, ρ: float = 0.95, max_iters: Optional[int] = None) -> LinesearchSolveSys:
    """setupLinesearchSolveSys(s; σ = 0.5, ρ = 0.95, max_iters = round(Int, log(ρ, 1e-6)))  (solve_system.jl:13-27)."""
    if max_iters is None:
        max_iters = int(_lib.lib().cgo_lss_default_max_iters(ρ)) if 0.0 < ρ < 1.0 else 0
    cfg = LinesearchSolveSys(ρ, σ, s, int(max_iters))
    c = cfg._c()
    check(_lib.lib().cgo_check_lss_config(C.byref(c)))   # the @assert's of solve_system.jl:21-23
    return cfg


# ---------------------------------------------------------------------------
# Results / TraceContainer (src/types.jl:17-23,107-114)
# ---------------------------------------------------------------------------
@dataclass
class TraceContainer:
    objective: np.ndarray
    grad_norm: np.ndarray
    step_size: np.ndarray
    objective_evals: np.ndarray
    status: TraceTrait


@dataclass
class Results:
    objective: float
    minimizer: np.ndarray
    gradient: np.ndarray
    iters_ran: int
    status: str  # the reference's Symbol, as text
    trace: TraceContainer
    total_fdf_evals: int = 0
    total_launches: int = 0


# ---------------------------------------------------------------------------
# device context
# ---------------------------------------------------------------------------
class Context:
    """One GPU = one shard.  `Context()` is a single-rank context on device 0."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        check(_lib.lib().cgo_ctx_create(device, C.byref(self._h)))
        self.device = device
        self.rank, self.world = 0, 1
        self._keep = []

    def set_default_policy(self, policy: "Optional[SolverPolicy]"):
        """The policy of every solver this context creates from now on — minimizeobjective / minimizeobjectivererun /
        solvesystem included (cgo_ctx_set_default_policy); None resets to the library's."""
        self._defpol_c = policy._c() if policy is not None else None
        check(_lib.lib().cgo_ctx_set_default_policy(self._h, C.byref(self._defpol_c) if self._defpol_c is not None else None))

    def set_comm_rccl(self, rank: int, world: int, unique_id: bytes):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        check(_lib.lib().cgo_ctx_set_comm_rccl(self._h, rank, world, buf))
        self.rank, self.world = rank, world

    def set_comm_callback(self, rank: int, world: int, allgather):
        """allgather(send: np.ndarray[count]) -> np.ndarray[world*count] (rank-major)."""
        def tramp(_user, send, recv, count):
            try:
                s = np.ctypeslib.as_array(send, shape=(count,)).copy()
                r = np.asarray(allgather(s), dtype=np.float64).reshape(-1)
                np.ctypeslib.as_array(recv, shape=(world * count,))[:] = r
                return 0
            except Exception:  # pragma: no cover - surfaced as CGO_ECOMM
                return 1
        cb = _lib.ALLGATHER_FN(tramp)
        self._keep.append(cb)
        check(_lib.lib().cgo_ctx_set_comm_callback(self._h, rank, world, cb, None))
        self.rank, self.world = rank, world

    def set_comm_shm(self, rank: int, world: int, name: str, create: bool):
        """Host shared-memory mailbox (one node).  Call on rank 0 with create=True, synchronise,
        call on the other ranks with create=False, synchronise, then rank 0 may shm_unlink(name)."""
        check(_lib.lib().cgo_ctx_set_comm_shm(self._h, rank, world, name.encode(), int(create)))
        self.rank, self.world = rank, world

    def connect_devices(self) -> bool:
        """COLLECTIVE (every rank, after all have attached with set_comm_shm): open the peers' device mailboxes over
        hipIpc / xGMI so that controller-armed launches exchange their blocks GPU to GPU.  False: host mailbox only."""
        ok = C.c_int32(0)
        check(_lib.lib().cgo_ctx_comm_connect_devices(self._h, C.byref(ok)))
        return bool(ok.value)

    def comm_info(self):
        """(transport, ranks_seen): 'none' | 'shm' | 'rccl' | 'callback', and how many ranks the transport itself
        reports (ncclCommCount / mailbox slots that have published / world)."""
        k, r, w, seen = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        check(_lib.lib().cgo_ctx_comm_info(self._h, C.byref(k), C.byref(r), C.byref(w), C.byref(seen)))
        return {0: "none", 1: "shm", 2: "rccl", 3: "callback"}[k.value], seen.value

    def exchange_stats(self, reset: bool = False):
        """(exchanges, peer_wait_us_total, device_exchange_us_mean) since the last reset — cgo_ctx_exchange_stats."""
        cnt, pw, dx = C.c_int64(), C.c_double(), C.c_double()
        check(_lib.lib().cgo_ctx_exchange_stats(self._h, C.byref(cnt), C.byref(pw), C.byref(dx), int(reset)))
        return cnt.value, pw.value, dx.value

    def close(self):
        if self._h:
            _lib.lib().cgo_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def build_id() -> str:
    """Digest of the sources libcgo_hip.so was built from (cgo_build_id)."""
    return _lib.lib().cgo_build_id().decode()


def rccl_available() -> bool:
    return _lib.lib().cgo_rccl_available() == 1


def shm_unlink(name: str) -> None:
    _lib.lib().cgo_shm_unlink(name.encode())


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    check(_lib.lib().cgo_comm_unique_id(buf))
    return buf.raw


_default_ctx: Optional[Context] = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def shard_extent(n_global: int, rank: int, world: int):
    """Contiguous, even-aligned shard [offset, offset+n_local) of rank `rank`."""
    pairs = n_global // 2
    base, rem = divmod(pairs, world)
    p0 = rank * base + min(rank, rem)
    p1 = p0 + base + (1 if rank < rem else 0)
    off, end = 2 * p0, 2 * p1
    if rank == world - 1:
        end = n_global  # odd tail element goes to the last rank
    return off, end - off


# ---------------------------------------------------------------------------
# device objective descriptors — the GPU-side `fdf!`
# ---------------------------------------------------------------------------
OBJ_KINDS = {"quad_diag": 0, "rosenbrock_paired": 1, "booth": 2, "lse": 3, "rosenbrock_chained": 6}
FILL_KINDS = {"constant": 0, "uniform": 1, "alternate": 2}


class DeviceObjective:
    """Descriptor of an element-wise objective evaluated inside the fused kernels."""

    def __init__(self, kind: str, n_global: int, ctx: Optional[Context] = None, source: Optional[str] = None,
                 has_param: bool = False, n_params: Optional[int] = None):
        self.ctx = ctx or default_context()
        self.kind = kind
        self.n_global = int(n_global)
        # Context.shard_fn: a host that partitions differently (uneven shards) supplies its own (n_global, rank, world) → extents
        shard = getattr(self.ctx, "shard_fn", None) or shard_extent
        self.offset, self.n_local = shard(self.n_global, self.ctx.rank, self.ctx.world)
        self._h = C.c_void_p()
        if source is not None:
            if n_params is None:   # zero or one parameter vector
                check(_lib.lib().cgo_objective_create_from_source(
                    self.ctx._h, source.encode(), int(has_param), self.n_global, self.offset, self.n_local,
                    C.byref(self._h)))
            else:                  # up to MAX_PARAM_SLOTS of them
                check(_lib.lib().cgo_objective_create_from_source_ex(
                    self.ctx._h, source.encode(), int(n_params), self.n_global, self.offset, self.n_local,
                    C.byref(self._h)))
            return
        check(_lib.lib().cgo_objective_create(self.ctx._h, OBJ_KINDS[kind], self.n_global,
                                              self.offset, self.n_local, C.byref(self._h)))

    def local(self, v: np.ndarray) -> np.ndarray:
        """This rank's shard of a global host vector."""
        return np.ascontiguousarray(v[self.offset:self.offset + self.n_local], dtype=np.float64)

    def set_param(self, v_global: np.ndarray, slot: int = 0):
        loc = self.local(np.asarray(v_global, dtype=np.float64))
        check(_lib.lib().cgo_objective_set_param_host(self._h, slot, loc.ctypes.data_as(dp)))

    def set_param_device(self, v, slot: int = 0):
        """Parameter vector `slot` from THIS rank's shard already on the GPU: a contiguous float64 torch tensor of
        n_local elements or a raw device pointer (int).  Device-to-device copy (cgo_objective_set_param_device)."""
        if v is None:
            raise TypeError("expected a torch.Tensor on the GPU or a raw device pointer")
        check(_lib.lib().cgo_objective_set_param_device(self._h, slot, _dev_ptr(v, self.n_local)))

    @property
    def n_params(self) -> int:
        """How many parameter vectors the objective's kernels read (cgo_objective_num_params)."""
        k = C.c_int32()
        check(_lib.lib().cgo_objective_num_params(self._h, C.byref(k)))
        return k.value

    def fill_param(self, fill: str, seed: int, lo: float, hi: float, slot: int = 0):
        check(_lib.lib().cgo_objective_fill_param(self._h, slot, FILL_KINDS[fill], seed, lo, hi))

    def set_scalar(self, value: float, slot: int = 0):
        check(_lib.lib().cgo_objective_set_scalar(self._h, slot, value))

    def __call__(self, g: np.ndarray, x: np.ndarray) -> float:
        """f = fdf!(g, x) on host vectors (one launch) — the reference's callback contract."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        f = C.c_double()
        check(_lib.lib().cgo_objective_eval_host(self._h, x.ctypes.data_as(dp), g.ctypes.data_as(dp),
                                                 C.byref(f)))
        return f.value

    def close(self):
        if self._h:
            _lib.lib().cgo_objective_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostObjective(DeviceObjective):
    """The reference's objective contract as it is: a host closure `f = fdf!(g, x)` that writes the gradient into `g`
    in place and returns the value (src/engine/optim.jl:25, src/cg_utils.jl:19; e.g. `boothfdf!`,
    examples/helpers/test_funcs.jl:3-12).  The solve still runs on the GPU engine — state, direction updates, dots,
    norms and the line-search state machine are the device ones; only x + a·u goes out and g comes back around each
    call of the closure (cgo_objective_create_callback).  `minimizeobjective(closure, …)` wraps a plain callable in
    one of these, so the reference's call `minimizeobjective(boothfdf!, x0, config, ls)` is a drop-in."""

    def __init__(self, fdf, n_global: int, ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()
        self.kind = "host"
        self.n_global = int(n_global)
        self.offset, self.n_local = shard_extent(self.n_global, self.ctx.rank, self.ctx.world)
        self._h = C.c_void_p()
        self._err = None

        def tramp(_user, gp, xp, n):
            try:
                g = np.ctypeslib.as_array(gp, shape=(n,))
                x = np.ctypeslib.as_array(xp, shape=(n,))
                return float(fdf(g, x))
            except BaseException as e:   # an exception cannot cross the C boundary: NaN stops the solve, re-raised after
                self._err = e
                return float("nan")
        self._cb = _lib.FDF_FN(tramp)
        self._fdf = fdf
        check(_lib.lib().cgo_objective_create_callback(self.ctx._h, self._cb, None, self.n_global, self.offset,
                                                       self.n_local, C.byref(self._h)))

    def reraise(self):
        if self._err is not None:
            e, self._err = self._err, None
            raise e


def QuadDiag(D: np.ndarray, ctx: Optional[Context] = None) -> DeviceObjective:
    """f(x) = ½ Σ D_i x_i²."""
    D = np.asarray(D, dtype=np.float64)
    o = DeviceObjective("quad_diag", D.size, ctx)
    o.set_param(D)
    return o


def QuadDiagRandom(n: int, seed: int = 24, lo: float = 1.0, hi: float = 1000.0,
                   ctx: Optional[Context] = None) -> DeviceObjective:
    """½ Σ D_i x_i² with D_i = lo + (hi−lo)·U(seed ⊕ i) generated on the device."""
    o = DeviceObjective("quad_diag", n, ctx)
    o.fill_param("uniform", seed, lo, hi)
    return o


def RosenbrockPaired(n: int, ctx: Optional[Context] = None) -> DeviceObjective:
    return DeviceObjective("rosenbrock_paired", n, ctx)


def RosenbrockChained(n: int, ctx: Optional[Context] = None) -> DeviceObjective:
    """f(x) = Σ_{i<n−1} (1 − x_i)² + 100 (x_{i+1} − x_i²)² — the chained form of examples/helpers/test_funcs.jl:50-57
    (value there; BASELINE config 1).  A 3-point stencil objective on the device (csrc/cgo_kernels_chain.hip.hpp):
    CG β kinds, every line search; shards exchange a 2-element halo inside the per-launch scalar block."""
    return DeviceObjective("rosenbrock_chained", n, ctx)


def LogSumExp(n: int, λ: float = 0.0, ctx: Optional[Context] = None) -> DeviceObjective:
    """f(x) = log Σ exp(x_i) + ½λ‖x‖² — not element-wise: two-phase kernels (trial statistics, then
    the gradient of the accepted step only)."""
    o = DeviceObjective("lse", n, ctx)
    o.set_scalar(float(λ))
    return o


MAX_PARAM_SLOTS = 4   # CGO_MAX_PARAM_SLOTS


def _param_list(param) -> Optional[list]:
    """`param=` of ElementwiseObjective / primalbarriermethod → None (one array or none: the one-slot form) or the list of
    slots of a sequence of arrays.  An entry that is None is a slot the caller sets later (fill_param, set_param_device)."""
    if param is None or isinstance(param, np.ndarray):
        return None
    if isinstance(param, (list, tuple)) and (len(param) == 0 or any(p is None or np.ndim(p) >= 1 for p in param)):
        return list(param)
    return None


def ElementwiseObjective(n: int, source: str, param=None,
                         ctx: Optional[Context] = None, cheap: bool = False) -> DeviceObjective:
    """A USER-SUPPLIED element-wise f/∇f — the GPU-side form of passing `minimizeobjective` your own
    `fdf!` closure.  `source` is HIP C++: the statements of an element-wise body setting `fi` and `gi`
    from `x`, `p`, `s0` (e.g. "gi = p*x; fi = 0.5*(gi*x);"), or a full `struct UserObjective {...}`
    functor for pair-coupled objectives.  Compiled at run time (hiprtc) into the fused kernels.

    `param` is one array (parameter slot 0, `p` in a body) or a sequence of up to 4 arrays: slots 0–3, `p`, `p1`, `p2`,
    `p3` in a body; a struct then declares `static constexpr int kParams = K` and takes `const double (&p)[K]` /
    `const d2 (&p)[K]` (include/cgo.h, cgo_objective_create_from_source_ex).  A None entry of the sequence reserves
    its slot for fill_param / set_param_device."""
    slots = _param_list(param)
    if slots is not None:
        assert len(slots) <= MAX_PARAM_SLOTS, f"at most {MAX_PARAM_SLOTS} parameter vectors"
        o = DeviceObjective("user", n, ctx, source=source, n_params=len(slots))
        for j, p in enumerate(slots):
            if p is not None:
                o.set_param(np.asarray(p, dtype=np.float64), slot=j)
        param = None
    else:
        o = DeviceObjective("user", n, ctx, source=source, has_param=param is not None)
    if param is not None:
        o.set_param(np.asarray(param, dtype=np.float64))
    if cheap:   # ≲ 10 flops per element for f and ∇f: seven speculative trial steps per launch
        check(_lib.lib().cgo_objective_set_cost_class(o._h, 1))
    return o


def Booth(ctx: Optional[Context] = None) -> DeviceObjective:
    """examples/helpers/test_funcs.jl:3-12."""
    return DeviceObjective("booth", 2, ctx)


def _dev_ptr(t, n: int):
    """torch tensor / raw pointer → void* (None → NULL); checks dtype, contiguity and length of tensors."""
    if t is None:
        return None
    if isinstance(t, int):
        return C.c_void_p(t)
    if hasattr(t, "data_ptr"):
        import torch
        if t.dtype != torch.float64 or not t.is_contiguous() or t.numel() != n or not t.is_cuda:
            raise ValueError(f"device vector must be a contiguous float64 GPU tensor of {n} elements")
        return C.c_void_p(t.data_ptr())
    raise TypeError("expected a torch.Tensor on the GPU or a raw device pointer")


# ---------------------------------------------------------------------------
# resumable solver (what minimizeobjective is built from)
# ---------------------------------------------------------------------------
LBFGS_FORMS = {"auto": 0, "one_pass": 1, "one_pass_own_update": 2, "gram": 3, "two_loop": 4}


@dataclass
class SolverPolicy:
    """cgo_solver_policy (include/cgo.h): HOW a solve runs, never WHAT it computes.  `None` = library policy for that
    field.  Precedence per field: Solver(..., policy=) > Context.set_default_policy > CGO_* experiment override > library."""
    points: Optional[int] = None               # trial steps per fused launch: 1 | 3 | 5 | 7
    resident: Optional[bool] = None            # resident solver on / off
    controller_depth: Optional[int] = None     # 0 host-driven, k armed rounds in flight
    controller_graph: Optional[bool] = None
    controller_fused: Optional[bool] = None
    stored_gradient: Optional[bool] = None     # True: the stored-gradient k_fused family
    fused_tail: Optional[bool] = None          # context-wide
    strict_tail: Optional[bool] = None         # context-wide: formally fenced hand-offs
    placement_search: Optional[bool] = None
    placement_stages: Optional[int] = None
    placement_max_bytes: Optional[int] = None  # cap on the search's transient device memory
    lbfgs_form: Optional[str] = None           # "one_pass" | "one_pass_own_update" | "gram" | "two_loop"
    lbfgs_fuse_grad: Optional[bool] = None
    lbfgs_fuse_trial: Optional[bool] = None
    lse_fixed_reference: Optional[bool] = None
    resident_points: Optional[int] = None
    resident_chunk: Optional[int] = None
    hbm_stream_bytes: Optional[float] = None   # launches moving more than this stream pure-HBM style (1: every launch)

    def _c(self) -> "_lib.SolverPolicyC":
        c = _lib.SolverPolicyC()
        _lib.lib().cgo_solver_policy_init(C.byref(c))
        tri = lambda v: -1 if v is None else (1 if v else 0)
        c.points = self.points or 0
        c.resident = tri(self.resident)
        c.controller_depth = -1 if self.controller_depth is None else int(self.controller_depth)
        c.controller_graph, c.controller_fused = tri(self.controller_graph), tri(self.controller_fused)
        c.stored_gradient = 1 if self.stored_gradient else 0
        c.fused_tail, c.strict_tail = tri(self.fused_tail), tri(self.strict_tail)
        c.placement_search = tri(self.placement_search)
        c.placement_stages = self.placement_stages or 0
        c.placement_max_bytes = int(self.placement_max_bytes or 0)
        c.lbfgs_form = LBFGS_FORMS[self.lbfgs_form or "auto"]
        c.lbfgs_fuse_grad, c.lbfgs_fuse_trial = tri(self.lbfgs_fuse_grad), tri(self.lbfgs_fuse_trial)
        c.lse_fixed_reference = tri(self.lse_fixed_reference)
        c.resident_points = self.resident_points or 0
        c.resident_chunk = self.resident_chunk or 0
        c.hbm_stream_bytes = float(self.hbm_stream_bytes or 0.0)
        return c


class Solver:
    def __init__(self, fdf: DeviceObjective, config: CGConfig, linesearch_config: LineSearchConfig,
                 policy: Optional[SolverPolicy] = None):
        if not isinstance(fdf, DeviceObjective):
            raise TypeError(
                "fdf! must be an objective descriptor: a device objective (QuadDiag, RosenbrockPaired, Booth, "
                "ElementwiseObjective, ...) or HostObjective(closure, n) — there is no CPU solver path in this package")
        self.obj, self.config, self.ls = fdf, config, linesearch_config
        self._cfg_c, self._ls_c = config._c(), linesearch_config._c()
        self._h = C.c_void_p()
        # a LinesearchSolveSys config selects solvesystem (solve_system.jl) instead of minimizeobjective
        create = (_lib.lib().cgo_solver_create_sys_ex if isinstance(linesearch_config, LinesearchSolveSys)
                  else _lib.lib().cgo_solver_create_ex)
        self._pol_c = policy._c() if policy is not None else None
        check(create(fdf.ctx._h, fdf._h, C.byref(self._cfg_c), C.byref(self._ls_c),
                     C.byref(self._pol_c) if self._pol_c is not None else None, C.byref(self._h)))

    def policy(self) -> dict:
        """The policy this solver actually runs with (cgo_solver_get_policy), as a dict of the C struct's fields."""
        c = _lib.SolverPolicyC()
        check(_lib.lib().cgo_solver_get_policy(self._h, C.byref(c)))
        return {n: getattr(c, n) for n, _ in c._fields_ if n not in ("size", "reserved")}

    def set_x0(self, x_initial_global: np.ndarray):
        loc = self.obj.local(np.asarray(x_initial_global, dtype=np.float64))
        check(_lib.lib().cgo_solver_set_x0_host(self._h, loc.ctypes.data_as(dp)))

    def set_x0_fill(self, fill: str, lo: float, hi: float = 0.0, seed: int = 0):
        check(_lib.lib().cgo_solver_set_x0_fill(self._h, FILL_KINDS[fill], seed, lo, hi))

    def set_x0_device(self, x0):
        """x_initial from memory that already lives on this GPU: a torch.Tensor (float64, contiguous, this rank's shard)
        or a raw device pointer (int).  Device-to-device copy, no PCIe (cgo_solver_set_x0_device)."""
        check(_lib.lib().cgo_solver_set_x0_device(self._h, _dev_ptr(x0, self.obj.n_local)))

    def results_device(self, minimizer=None, gradient=None):
        """Results.minimizer / Results.gradient into device buffers (torch tensors or raw pointers); scalars and traces
        come from results(vectors=False)."""
        check(_lib.lib().cgo_solver_results_device(self._h, _dev_ptr(minimizer, self.obj.n_local), _dev_ptr(gradient, self.obj.n_local)))

    def start(self):
        check(_lib.lib().cgo_solver_start(self._h))

    def iterate(self, iters: int) -> bool:
        fin = C.c_int32(0)
        check(_lib.lib().cgo_solver_iterate(self._h, iters, C.byref(fin)))
        return bool(fin.value)

    def enable_trial_log(self):
        cnt = C.c_int64()
        check(_lib.lib().cgo_solver_trial_log(self._h, -1, None, None, None, C.byref(cnt)))

    def trial_log(self):
        cnt = C.c_int64()
        check(_lib.lib().cgo_solver_trial_log(self._h, 0, None, None, None, C.byref(cnt)))
        k = cnt.value
        a, p, d = np.zeros(max(k, 1)), np.zeros(max(k, 1)), np.zeros(max(k, 1))
        check(_lib.lib().cgo_solver_trial_log(self._h, k, a.ctypes.data_as(dp), p.ctypes.data_as(dp),
                                              d.ctypes.data_as(dp), C.byref(cnt)))
        return a[:k], p[:k], d[:k]

    def kernel_family(self) -> str:
        return _lib.lib().cgo_solver_kernel_family(self._h).decode()

    def kernel_symbol(self, kind_name: str) -> str:
        """The kernel instantiation launches of kind `kind_name` ('accept_dir_trial', 'trial', …) use under the current
        policy, e.g. 'k_cg<ObjQuadDiag, 7, 7, true>' (cgo_solver_kernel_symbol)."""
        L = _lib.lib()
        buf = C.create_string_buffer(200)
        for k in range(L.cgo_num_kernel_kinds()):
            if L.cgo_kernel_kind_name(k).decode() == kind_name:
                check(L.cgo_solver_kernel_symbol(self._h, k, buf, 200))
                return buf.value.decode()
        return ""

    def set_lazy_direction(self, on: bool = True):
        """Force the lazy-direction launches on or off for this solver, before start() (cgo_solver_set_lazy_direction): on an
        eligible solver every second accept + direction + trial launch leaves u unstored and the next one rebuilds it."""
        check(_lib.lib().cgo_solver_set_lazy_direction(self._h, int(bool(on))))

    def set_replay_depth(self, d: int):
        """Replay depth of this solver, 1 … 16 (cgo_solver_set_replay_depth): on an eligible solver d − 1 of every d accept +
        direction + trial launches store neither x nor u and the d-th replays them and stores both; 1 = the lazy direction's
        alternation.  Above 8 (deep replay) where the cycle runs as path launches; any other solver runs it as 8.  Mid-solve,
        outstanding steps are stored first."""
        check(_lib.lib().cgo_solver_set_replay_depth(self._h, int(d)))

    def replay_stats(self):
        """dict(n=, s=, t=, m=, t_deep=, m_deep=, max_list=) of this solver (cgo_solver_replay_stats): launches N, S, T (a trial met
        with steps outstanding) and materialise passes M so far, the T and M that met more than seven outstanding steps, and the
        longest list a launch replayed."""
        v = [C.c_int64(0) for _ in range(6)]
        mx = C.c_int32(0)
        check(_lib.lib().cgo_solver_replay_stats(self._h, *[C.byref(q) for q in v], C.byref(mx)))
        return dict(zip(("n", "s", "t", "m", "t_deep", "m_deep"), (q.value for q in v)), max_list=mx.value)

    def set_lean_sums(self, on: bool):
        """Lean sums for this solver (cgo_solver_set_lean_sums): the replay cycle's launches N and S leave out the trial sums
        the solver's β flavour never reads, where the library has such kernels (Polak–Ribière); every number a solve returns
        stays bit for bit.  Takes effect at the next launch."""
        check(_lib.lib().cgo_solver_set_lean_sums(self._h, int(bool(on))))

    def set_path_prediction(self, on: bool):
        """Predicted path for this solver (cgo_solver_set_path_prediction): where the replay cycle's launches N and S would run
        their lean rows they evaluate only the steps the line search is predicted to ask for (separable quadratic, Polak–Ribière,
        a bisection search with the Wolfe conditions; any other solver keeps its rows).  Every number a solve returns stays bit
        for bit.  Takes effect at the next launch."""
        check(_lib.lib().cgo_solver_set_path_prediction(self._h, int(bool(on))))

    def path_stats(self):
        """dict(by_nact={points evaluated: path launches}, predicted=, tree=, misses=) of this solver (cgo_solver_path_stats)."""
        by = (C.c_int64 * 8)()
        p, t, m = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(_lib.lib().cgo_solver_path_stats(self._h, by, C.byref(p), C.byref(t), C.byref(m)))
        return dict(by_nact={j: int(by[j]) for j in (1, 2, 3, 4, 5, 7)}, predicted=p.value, tree=t.value, misses=m.value)

    def debug_set_path_skew(self, factor: float):
        """Tests only: a factor on the predicted path's curvature model (cgo_solver_debug_set_path_skew)."""
        check(_lib.lib().cgo_solver_debug_set_path_skew(self._h, float(factor)))

    def probe_launch(self, kind_name: str, variant: int, a_acc: float, beta: float, a: Sequence[float], x, u=None, aux=None,
                     beta_prev: Optional[float] = None, replay: Optional[Sequence] = None, path_nact: Optional[int] = None,
                     deep_trial: bool = False):
        """ONE launch of kind `kind_name` with mode bits `variant` on this rank's host vectors (cgo_solver_probe_launch): returns
        dict(sums=the whole reduced row, x=, u=, g= the vectors after the launch, symbol=the instantiation).  A test entry point:
        the solver is for probing only from the first call on.

        A stored-gradient solver (β = LBFGS on an element-wise objective, a HostObjective, policy stored_gradient) takes M_* bits
        and one trial step: init 16, trial 4 | 12, accept_dir_trial 15, accept_dir 3, accept_only 1, reset_dir 32, upg_norm 64
        (0: the kind's usual mode); `aux` is the stored gradient g the launch reads, g= the buffer holding g⁺ afterwards.  With a
        HostObjective init / trial / accept_dir_trial run k_trial_point, the closure and k_fused<…, 128> (init: then the reset
        launch; accept_dir_trial: accept_dir first), sums= their rows one after the other.  scaled_norm: variant = which
        (0 g, 1 g⁺, 3 u, 4 g⁺ − g; g⁺ is passed as `x` for 1 and 4), sums= the pass-0 row {max, #NaN, 0…} then, when it ran,
        the pass-1 row {Σ (v/max)², 0…}.  symbol joins the launches with " + "."""
        L = _lib.lib()
        kk = [L.cgo_kernel_kind_name(k).decode() for k in range(L.cgo_num_kernel_kinds())].index(kind_name)
        if beta_prev is not None:   # the lazy-direction variants (R_ULAG = 1024): u ← −∇f(x) + beta_prev·u on load
            check(L.cgo_solver_probe_set_beta_prev(self._h, float(beta_prev)))
        if replay is not None:      # the replay variants (R_REPLAY = 4096): the (a*, β) pairs replayed on load, oldest first
            ra = np.ascontiguousarray([p[0] for p in replay], dtype=np.float64)
            rb = np.ascontiguousarray([p[1] for p in replay], dtype=np.float64)
            check(L.cgo_solver_probe_set_replay(self._h, len(replay), ra.ctypes.data_as(dp), rb.ctypes.data_as(dp)))
        if path_nact is not None:   # a lean row as its path twin k_cg_path<…, path_nact, true> (this launch only)
            check(L.cgo_solver_probe_set_path(self._h, int(path_nact)))
        if deep_trial:              # launch T (variant 4100) as k_cg_trial_deep whatever the list's length (this launch only)
            check(L.cgo_solver_probe_set_deep_trial(self._h, 1))
        n = self.obj.n_local
        vec = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
        x, u, aux = vec(x), vec(u), vec(aux)
        for v in (x, u, aux):
            if v is not None and v.size != n:
                raise ValueError(f"probe vectors hold n_local = {n} elements")
        av = np.ascontiguousarray(a, dtype=np.float64) if len(a) else np.zeros(1)
        sums, ln = np.full(64, np.nan), C.c_int32(0)
        xo, uo, go = np.empty(n), np.empty(n), np.empty(n)
        sym = C.create_string_buffer(200)
        ptr = lambda v: None if v is None else v.ctypes.data_as(dp)
        check(L.cgo_solver_probe_launch(self._h, kk, int(variant), float(a_acc), float(beta), ptr(av), len(a), ptr(x), ptr(u),
                                        ptr(aux), ptr(sums), 64, C.byref(ln), ptr(xo), ptr(uo), ptr(go), sym, 200))
        return dict(sums=sums[:ln.value].copy(), x=xo, u=uo, g=go, symbol=sym.value.decode())

    LBFGS_PASSES = ("push", "push_gram", "direction_gram", "direction_trial", "push_lite", "loop")

    def probe_lbfgs(self, pass_name: str, x=None, u=None, g=None, gt=None, S=None, Y=None, **kw):
        """ONE L-BFGS pass on host vectors and whole rings (cgo_solver_probe_lbfgs; pass names and fields as in include/cgo.h).
        S, Y: (m + 1, n_local) arrays, NaN rows for absent slots; `list`, `cy`, `cs`, `spec_list`, `dots` (rows of 10),
        `alpha` are sequences, `stats` the log-sum-exp statistics (fields M, S), every other keyword a cgo_lbfgs_probe field.  Returns dict(sums=the whole reduced row, x=, xo=,
        u=, g=, gt=, S=, Y= after the pass, alpha=, symbols=[instantiations launched, in order], new_in_list=, spec_ok=,
        gram=[sy, yy, sgn, ygn, gtgt, then sjg, yjg, sjyn, yjsn, yjyn per pair] or None).  For probing only from the first call on."""
        n = self.obj.n_local
        P = self._cfg_c.beta.lbfgs_m + 1
        vec = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
        x, u, g, gt = vec(x), vec(u), vec(g), vec(gt)
        for v in (x, u, g, gt):
            if v is not None and v.size != n:
                raise ValueError(f"probe vectors hold n_local = {n} elements")
        S = None if S is None else np.ascontiguousarray(S, dtype=np.float64).reshape(P, n)
        Y = None if Y is None else np.ascontiguousarray(Y, dtype=np.float64).reshape(P, n)
        p = _lib.LbfgsProbeC()
        p.pass_ = self.LBFGS_PASSES.index(pass_name)
        dots = None
        for key, val in kw.items():
            if key in ("list", "spec_list"):
                getattr(p, key)[:len(val)] = [int(v) for v in val]
                setattr(p, "count" if key == "list" else "spec_count", len(val))
            elif key in ("cy", "cs", "alpha"):
                getattr(p, key)[:len(val)] = [float(v) for v in val]
            elif key == "stats":   # the log-sum-exp statistics (M, S): fields M, S
                p.M, p.S = float(val[0]), float(val[1])
            elif key == "dots":
                dots = np.ascontiguousarray(val, dtype=np.float64).reshape(-1, 10)
                p.dots, p.dot_count = dots.ctypes.data_as(dp), dots.shape[0]
            else:
                if not hasattr(p, key):
                    raise TypeError(f"probe_lbfgs: no field {key}")
                setattr(p, key, val)
        outs = {k: np.full(n, np.nan) for k in ("x", "xo", "u", "g", "gt")}
        So, Yo = np.full((P, n), np.nan), np.full((P, n), np.nan)
        ptr = lambda v: None if v is None else v.ctypes.data_as(dp)
        check(_lib.lib().cgo_solver_probe_lbfgs(self._h, C.byref(p), ptr(x), ptr(u), ptr(g), ptr(gt), ptr(S), ptr(Y),
                                                *[ptr(outs[k]) for k in ("x", "xo", "u", "g", "gt")], ptr(So), ptr(Yo)))
        sym = p.symbol.decode()
        return dict(sums=np.array(p.sums[:p.sums_len]), S=So, Y=Yo, alpha=np.array(p.alpha[:]), symbols=sym.split(" + ") if sym else [],
                    new_in_list=p.new_in_list, spec_ok=bool(p.spec_ok),
                    gram=np.array(p.gram[:5 + 5 * p.spec_count]) if p.spec_ok else None, **outs)

    def probe_resident(self, script, x, u):
        """A scripted sequence of resident passes in ONE launch (cgo_solver_probe_resident).  `script`: up to 32 tuples
        ("trial", a) or ("accept_dir_trial", a_acc, beta, a), a = the trial steps (k = len(a)).  Returns dict(rows=[per pass:
        (grid, width) array — the totals every workgroup holds], tail=[per pass: what lies behind the width in the 56-slot
        stride, (grid, 56 − width)], out=[per pass: dict(ts=(7, 7) array, gu=, uu=) as workgroup 0's member function returned
        them], grid=, chunk=, points=, round0=, wrote_back=, x=, u= (what the next slice would read), symbol=).  For probing
        only from the first call on."""
        n = self.obj.n_local
        x, u = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(u, dtype=np.float64)
        if x.size != n or u.size != n:
            raise ValueError(f"probe vectors hold n_local = {n} elements")
        p = _lib.ResidentProbeC()
        if len(script) > 32:
            raise ValueError("probe_resident: at most 32 passes")
        p.npass = len(script)
        for q, item in enumerate(script):
            c = p.pass_[q]
            if item[0] == "trial":
                c.kind, a = 0, item[1]
            elif item[0] == "accept_dir_trial":
                c.kind, c.a_acc, c.beta, a = 1, float(item[1]), float(item[2]), item[3]
            else:
                raise ValueError(f"probe_resident: no pass kind {item[0]!r}")
            if len(a) > 7:
                raise ValueError("probe_resident: at most 7 trial steps")
            c.k = len(a)
            c.a[:len(a)] = [float(v) for v in a]
        rows = np.full((max(p.npass, 1), 256, 56), np.nan)
        xo, uo = np.empty(n), np.empty(n)
        check(_lib.lib().cgo_solver_probe_resident(self._h, C.byref(p), x.ctypes.data_as(dp), u.ctypes.data_as(dp),
                                                   rows.ctypes.data_as(dp), rows.size, xo.ctypes.data_as(dp), uo.ctypes.data_as(dp)))
        g = p.grid
        got = rows.ravel()[:p.npass * g * 56].reshape(p.npass, g, 56)
        outs, rws, tails = [], [], []
        for q in range(p.npass):
            w = int(p.out[q].width)
            rws.append(got[q, :, :w].copy()); tails.append(got[q, :, w:].copy())
            outs.append(dict(ts=np.array([list(r) for r in p.out[q].ts]), gu=p.out[q].gu, uu=p.out[q].uu))
        return dict(rows=rws, tail=tails, out=outs, grid=g, chunk=p.chunk, points=p.points, round0=p.round0,
                    wrote_back=bool(p.wrote_back), x=xo, u=uo, symbol=p.symbol.decode())

    ARMED_FORMS = ("rounds", "graph", "controller")

    def probe_armed(self, state, rounds=1, form="rounds", x=None, u=None, max_iters=1 << 40, eps=None, row=None):
        """A batch of controller-armed rounds on host vectors (cgo_solver_probe_armed).  `state`: dict(f_x=, gg=, a_acc=, beta=,
        a=[1 … 7 trial steps, the last one repeated into the slots behind], npts= (default len(a)), go= (default 1), it=
        (default 0)) — the CtlState k_ctl_init writes; max_iters and eps (None: the solver's) complete the controller's
        config.  form "rounds": launched one by one, "graph": the engine's captured batches of 8 / 4 / 2, "controller":
        k_finalize_ctl alone on `row` (up to 56 sums), one round, x and u not needed.  Returns dict(records=[per round:
        dict(sums= all 56, a_acc=, beta=, a= all 7, npts=, accepted=, xwait=, bytes= the record as it was published)],
        st=, args= (dicts of the device block's state and argument block after the last round, each with bytes=), round=,
        out_dev= (56 slots), width=, maxp=, x=, u=, symbols=[every instantiation launched, in order]).  For probing only from
        the first call on."""
        n = self.obj.n_local
        p = _lib.ArmedProbeC()
        p.rounds, p.form = int(rounds), self.ARMED_FORMS.index(form)
        p.max_iters = int(max_iters)
        if eps is not None:
            p.use_eps, p.eps = 1, float(eps)
        a = [float(v) for v in state["a"]]
        if not 1 <= len(a) <= 7:
            raise ValueError("probe_armed: 1 to 7 trial steps")
        p.st.f_x, p.st.gg = float(state["f_x"]), float(state["gg"])
        p.st.a_acc, p.st.beta = float(state["a_acc"]), float(state["beta"])
        p.st.a[:] = a + [a[-1]] * (7 - len(a))
        p.st.npts, p.st.go, p.st.it = int(state.get("npts", len(a))), int(state.get("go", 1)), int(state.get("it", 0))
        if row is not None:
            r = [float(v) for v in row]
            p.row[:len(r)] = r
        vec = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
        x, u = vec(x), vec(u)
        for v in (x, u):
            if v is not None and v.size != n:
                raise ValueError(f"probe vectors hold n_local = {n} elements")
        xo, uo = np.full(n, np.nan), np.full(n, np.nan)
        ptr = lambda v: None if v is None else v.ctypes.data_as(dp)
        check(_lib.lib().cgo_solver_probe_armed(self._h, C.byref(p), ptr(x), ptr(u), ptr(xo), ptr(uo)))

        def block(c, names):
            d = {k: (np.array(getattr(c, k)[:]) if k in ("a", "sums") else getattr(c, k)) for k in names}
            d["bytes"] = bytes(c)
            return d
        recs = [block(p.rec[r], ("sums", "a_acc", "beta", "a", "npts", "accepted", "xwait")) for r in range(p.rounds)]
        sym = p.symbol.decode()
        return dict(records=recs, st=block(p.st_out, ("f_x", "gg", "a_acc", "beta", "a", "npts", "go", "it")),
                    args=block(p.args_out, ("a_acc", "beta", "a", "go")), round=int(p.round_out), out_dev=np.array(p.out_dev[:]),
                    width=p.width, maxp=p.maxp, x=xo, u=uo, symbols=sym.split(" + ") if sym else [])

    def placement_info(self):
        """(as_allocated_us, chosen_us, candidates) of the solver's placement search (cgo_solver_placement_info);
        candidates == 0: no search was made."""
        a, b, c = C.c_double(), C.c_double(), C.c_int32()
        check(_lib.lib().cgo_solver_placement_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def controller_launches(self) -> int:
        """Launches armed by the on-device controller instead of the host (csrc/cgo_ctl.hpp)."""
        return int(_lib.lib().cgo_solver_controller_launches(self._h))

    def resident_stats(self):
        """(slices, iterations): launches of the resident solver and the outer iterations completed inside them."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        check(_lib.lib().cgo_solver_resident_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        self.resident_gave_up = c.value   # slices handed back whole because their workgroups could not all run at once
        return a.value, b.value

    def lbfgs_stats(self):
        """(speculated, fused, plain): how the L-BFGS state updates of this solver were paid for (include/cgo.h)."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        check(_lib.lib().cgo_solver_lbfgs_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def profile(self, on: bool = True):
        check(_lib.lib().cgo_solver_profile_enable(self._h, int(on)))

    def profile_reset(self):
        check(_lib.lib().cgo_solver_profile_reset(self._h))

    def profile_get(self):
        L = _lib.lib()
        out = {}
        for k in range(L.cgo_num_kernel_kinds()):
            n, ms, b = C.c_int64(), C.c_double(), C.c_double()
            check(L.cgo_solver_profile_get(self._h, k, C.byref(n), C.byref(ms), C.byref(b)))
            if n.value:
                out[L.cgo_kernel_kind_name(k).decode()] = dict(
                    launches=n.value, total_ms=ms.value, bytes_per_launch=b.value)
        return out

    def results(self, vectors: bool = True) -> Results:
        n = self.obj.n_local
        cap = max(self.config.max_iters, 1)
        x = np.empty(n) if vectors else None
        g = np.empty(n) if vectors else None
        to, tg, ts = np.zeros(cap), np.zeros(cap), np.zeros(cap)
        te = np.zeros(cap, dtype=np.int64)
        r = ResultsC()
        r.minimizer = x.ctypes.data_as(dp) if vectors else None
        r.gradient = g.ctypes.data_as(dp) if vectors else None
        r.trace_objective, r.trace_grad_norm = to.ctypes.data_as(dp), tg.ctypes.data_as(dp)
        r.trace_step_size, r.trace_objective_evals = ts.ctypes.data_as(dp), te.ctypes.data_as(i64p)
        check(_lib.lib().cgo_solver_results(self._h, C.byref(r)))
        k = max(int(r.iters_ran), 0)
        if not isinstance(self.config.trace_status, EnableTrace):
            k = 0
        tr = TraceContainer(to[:k].copy(), tg[:k].copy(), ts[:k].copy(), te[:k].copy(),
                            self.config.trace_status)
        return Results(r.objective, x, g, int(r.iters_ran),
                       _lib.lib().cgo_status_name(r.status).decode(), tr,
                       int(r.total_fdf_evals), int(r.total_launches))

    def close(self):
        if self._h:
            _lib.lib().cgo_solver_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------
# the reference's two entry points
# ---------------------------------------------------------------------------
def minimizeobjective(fdf, x_initial: Sequence[float], config: CGConfig,
                      linesearch_config: LineSearchConfig, policy: Optional[SolverPolicy] = None) -> Results:
    """minimizeobjective(fdf!, x_initial, config, linesearch_config)  (src/engine/optim.jl:6-171).

    `x_initial` is the GLOBAL initial iterate (copied, never mutated — optim.jl:21);
    the returned minimizer/gradient are this rank's shard (the whole vector on one GPU).
    `fdf` is a device objective descriptor or — the reference's own form — a closure `fdf(g, x) -> f`
    (wrapped in a HostObjective: GPU engine, objective evaluated on the host)."""
    own = None
    if not isinstance(fdf, DeviceObjective) and callable(fdf):
        fdf = own = HostObjective(fdf, len(x_initial))
    s = Solver(fdf, config, linesearch_config, policy)
    try:
        s.set_x0(np.asarray(x_initial, dtype=np.float64))
        s.start()
        while not s.iterate(1 << 40):
            pass
        r = s.results()
        if isinstance(fdf, HostObjective):
            fdf.reraise()
        return r
    finally:
        s.close()
        if own is not None:
            own.close()


class BatchResults(list):
    """The `Results` of a batched solve, one per problem, plus the counters of the call: `launches` (k_batch launches),
    `handed_back` (problems the host engine finished) and `rows`, the tier that ran ("lds" or "device")."""
    launches: int = 0
    handed_back: int = 0
    rows: str = "lds"


BATCH_ROWS = {"lds": 0, "device": 1, "auto": 2}      # CGO_BATCH_ROWS_*
_BATCH_ROWS_NAMES = {v: k for k, v in BATCH_ROWS.items()}


def _batch_policy(rows) -> Optional["_lib.BatchPolicyC"]:
    """`rows` as a cgo_batch_policy — None for "lds", the calls without a policy.  An unknown value raises before any
    library call."""
    if not isinstance(rows, str) or rows not in BATCH_ROWS:
        raise ValueError(f"rows must be one of 'lds', 'device', 'auto', not {rows!r}")
    if rows == "lds":
        return None
    pol = _lib.BatchPolicyC()
    _lib.lib().cgo_batch_policy_init(C.byref(pol))
    pol.rows = BATCH_ROWS[rows]
    return pol


def batch_rows_shape():
    """(lanes per workgroup, pairs of elements per lane and trip) of the streaming loop of rows="device"."""
    blk, u = C.c_int32(0), C.c_int32(0)
    _lib.lib().cgo_batch_rows_shape(C.byref(blk), C.byref(u))
    return int(blk.value), int(u.value)


def batch_max_n(obj_or_kind, ctx: Optional[Context] = None, rows: str = "lds") -> int:
    """Largest n of one problem of a batched solve.  rows="lds": what one workgroup's LDS holds of x, u and the parameter
    vectors; "device" / "auto": the index range of a pass over rows in device memory (memory is the other limit, checked by
    the call).  A kind name for the built-in objectives; a run-time compiled `DeviceObjective` (kind "user") for its own — with
    rows="lds" the first call on its compiled module compiles the batch program."""
    pol = _batch_policy(rows)
    polp = C.byref(pol) if pol is not None else None
    if isinstance(obj_or_kind, DeviceObjective):
        return int(_lib.lib().cgo_batch_max_n_obj_ex(obj_or_kind._h, polp))
    ctx = ctx or default_context()
    return int(_lib.lib().cgo_batch_max_n_ex(ctx._h, OBJ_KINDS[obj_or_kind], polp))


class _BatchOut:
    """The caller-allocated arrays of a `cgo_batch_results` for [batch] problems of size n under `config`, and what they become."""

    def __init__(self, batch: int, n: int, config: CGConfig):
        self.batch, self.config = batch, config
        self.trace = isinstance(config.trace_status, EnableTrace)
        cap = max(config.max_iters, 1)
        self.f = np.zeros(batch)
        self.it = np.zeros(batch, dtype=np.int64)
        self.st = np.zeros(batch, dtype=np.int32)
        self.ev = np.zeros(batch, dtype=np.int64)
        self.x, self.g = np.zeros((batch, n)), np.zeros((batch, n))
        r = self.c = _lib.BatchResultsC()
        r.objective, r.iters_ran = self.f.ctypes.data_as(dp), self.it.ctypes.data_as(i64p)
        r.status, r.total_fdf_evals = self.st.ctypes.data_as(C.POINTER(C.c_int32)), self.ev.ctypes.data_as(i64p)
        r.minimizer, r.gradient = self.x.ctypes.data_as(dp), self.g.ctypes.data_as(dp)
        if self.trace:
            self.to, self.tg, self.ts = np.zeros((batch, cap)), np.zeros((batch, cap)), np.zeros((batch, cap))
            self.te = np.zeros((batch, cap), dtype=np.int64)
            r.trace_objective, r.trace_grad_norm = self.to.ctypes.data_as(dp), self.tg.ctypes.data_as(dp)
            r.trace_step_size, r.trace_objective_evals = self.ts.ctypes.data_as(dp), self.te.ctypes.data_as(i64p)

    def results(self, active=None, rows_used: int = 0) -> "BatchResults":
        r, config, trace = self.c, self.config, self.trace
        out = BatchResults()
        out.launches, out.handed_back, out.rows = int(r.launches), int(r.handed_back), _BATCH_ROWS_NAMES[int(rows_used)]
        empty, empty_i = np.zeros(0), np.zeros(0, dtype=np.int64)
        for b in range(self.batch):
            if active is not None and not active[b]:
                out.append(None)
                continue
            k = max(int(self.it[b]), 0) if trace else 0
            tr = (TraceContainer(self.to[b, :k].copy(), self.tg[b, :k].copy(), self.ts[b, :k].copy(), self.te[b, :k].copy(), config.trace_status)
                  if trace else TraceContainer(empty.copy(), empty.copy(), empty.copy(), empty_i.copy(), config.trace_status))
            out.append(Results(float(self.f[b]), self.x[b].copy(), self.g[b].copy(), int(self.it[b]),
                               _lib.lib().cgo_status_name(int(self.st[b])).decode(), tr, int(self.ev[b]), int(r.launches)))
        return out


def _batch_rows(name: str, v, shape, msg: Optional[str] = None) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float64))
    if a.shape != tuple(shape):
        raise ValueError(msg or f"{name} must be {list(shape)}")
    return a


def _batch_inputs(X0, params=None, n=None, none_ok=True):
    """X0 as a contiguous [batch, n] array and `params` as the list of slot rows of its shape (an entry that is None stays None
    where `none_ok`); `n`: the size X0's rows must have, a model's."""
    X0 = np.ascontiguousarray(np.asarray(X0, dtype=np.float64))
    if X0.ndim != 2:
        raise ValueError("X0 must be [batch, n]")
    if n is not None and X0.shape[1] != n:
        raise ValueError(f"X0 must be [batch, {n}], the size of the model objective")
    Pc = []
    for j, v in enumerate(params if params is not None else []):
        if v is None and not none_ok:
            raise ValueError(f"params[{j}] is None: every slot needs its [batch, n] rows")
        Pc.append(None if v is None else np.ascontiguousarray(np.asarray(v, dtype=np.float64)))
        if Pc[-1] is not None and Pc[-1].shape != X0.shape:
            raise ValueError(f"params[{j}] must have the shape of X0")
    return X0, Pc


def minimizeobjectivebatch(obj_or_kind, X0, config: CGConfig, linesearch_config: LineSearchConfig, D=None, params=None,
                           ctx: Optional[Context] = None, slice_iters: int = 0, scalars=None, rows: str = "lds") -> BatchResults:
    """`batch` independent minimizeobjective problems in ONE launch sequence, a workgroup each: X0 is [batch, n]; one config and
    one line search for all.  `obj_or_kind` is either one of "quad_diag" (D: [batch, n], the rows of the diagonal),
    "rosenbrock_paired" (n even) or "booth" (n = 2), or a run-time compiled `DeviceObjective` (ElementwiseObjective) of size n —
    the MODEL: its source, scalar and cost class are every problem's, its own parameter vectors are not touched — with `params`,
    a sequence of its n_params arrays [batch, n], the rows of slot 0, 1, ….  The first batched solve on a compiled source
    compiles its batch program (seconds); later ones find it.  Returns a list of `Results`, one per problem — what
    minimizeobjective returns for it — with the counters `launches` and `handed_back` as attributes.  Problems whose next
    iteration the device loop does not run are finished by the ordinary engine; anything the batched form does not cover
    raises CgoError (no loop of solves behind it).  slice_iters: outer iterations per problem and launch (0: the library's
    policy).  scalars: a [batch] array, every problem's OWN `s0` in place of the model's (a model only: the built-in kinds
    read no scalar) — one `Batch.solve`; a `Batch` kept open serves many such calls on the same data.
    rows: where a problem's rows live during the solve.  "lds" (the default): in its workgroup's LDS, n ≤ batch_max_n(…).
    "device": they stay in device memory and every pass streams them from there — n up to batch_max_n(…, rows="device") and
    what the device's memory holds; every number returned has the bits of the LDS tier, at the price of a round trip to
    memory per pass.  "auto": LDS where n fits, device rows beyond.  The returned list says which ran (`.rows`)."""
    pol = _batch_policy(rows)
    model = obj_or_kind if isinstance(obj_or_kind, DeviceObjective) else None
    if model is None and obj_or_kind not in OBJ_KINDS:
        raise ValueError(f"unknown objective kind {obj_or_kind!r}")
    X0, _ = _batch_inputs(X0)
    batch, n = X0.shape
    if scalars is not None and model is None:
        raise ValueError(f"scalars belongs to a run-time compiled objective: {obj_or_kind} reads no scalar")
    Dc = None
    if D is not None:
        if model is not None:
            raise ValueError("D belongs to the built-in quadratic: an objective takes params, one array per slot")
        Dc = _batch_rows("D", D, X0.shape, "D must have the shape of X0")
    if params is not None and model is None:
        raise ValueError("params belongs to a run-time compiled objective: the built-in quadratic takes D")
    _, Pc = _batch_inputs(X0, params)
    if model is not None:
        if n != model.n_global:
            raise ValueError(f"X0 must be [batch, {model.n_global}], the size of the model objective")
        ctx = ctx or model.ctx
    if scalars is not None:
        scalars = _batch_rows("scalars", scalars, (batch,))
        with Batch(model, Pc, batch, rows=rows) as B:
            return B.solve(X0, config, linesearch_config, scalars=scalars, slice_iters=slice_iters)
    ctx = ctx or default_context()
    o = _BatchOut(batch, n, config)
    cfg, ls = config._c(), linesearch_config._c()
    polp = C.byref(pol) if pol is not None else None
    used = C.c_int32(0)
    if model is not None:
        prows = (dp * max(len(Pc), 1))(*[v.ctypes.data_as(dp) if v is not None else None for v in Pc])
        check(_lib.lib().cgo_minimize_batch_obj_ex(ctx._h, model._h, batch, X0.ctypes.data_as(dp), prows, len(Pc), C.byref(cfg),
                                                   C.byref(ls), int(slice_iters), polp, C.byref(o.c), C.byref(used)))
    else:
        check(_lib.lib().cgo_minimize_batch_ex(ctx._h, OBJ_KINDS[obj_or_kind], n, batch, X0.ctypes.data_as(dp),
                                               Dc.ctypes.data_as(dp) if Dc is not None else None, C.byref(cfg), C.byref(ls),
                                               int(slice_iters), polp, C.byref(o.c), C.byref(used)))
    return o.results(rows_used=used.value)


BATCH_PROBE_TIERS = {"lds": 0, "device": 1, "lbfgs": 2, "lbfgs_lds": 3}
BATCH_PROBE_ROW = 64
NAN_PATTERN = 0x7FF87FF87FF87FF8   # what every probe buffer starts as


def batch_probe_qn_words() -> int:
    """8-byte words of one problem's quasi-Newton state (QnState, csrc/cgo_qn.hpp) as `batch_probe` takes and returns it."""
    return int(_lib.lib().cgo_batch_probe_qn_bytes()) // 8


def batch_probe(tier: str, obj_or_kind, X, U, script, params=None, scalars=None, skip=None, m: int = 0, S=None, Y=None, qn=None,
                gradient: bool = False, ctx: Optional[Context] = None) -> dict:
    """A scripted sequence of passes of a batched solve in ONE launch, a workgroup per problem (cgo_batch_probe).  tier: "lds"
    (k_batch), "device" (k_batch_rows), "lbfgs" (k_batch_lbfgs) or "lbfgs_lds" (k_batch_lbfgs_lds, tier 3: the inputs and outputs of
    "lbfgs", built-in kinds only).  `obj_or_kind` as in minimizeobjectivebatch; X, U [batch, n];
    params: the arrays [batch, n] of the slots the objective reads (the quadratic: [D]); scalars, skip: [batch] or None.
    "lbfgs": m, S and Y [batch, m + 1, n] (absent slots NaN) and qn, a uint64 array [batch, batch_probe_qn_words()].
    `script`: up to 32 tuples ("trial", a) | ("accept_dir_trial", a_acc, beta, a) | ("init",) | ("push", a_acc) |
    ("combine", a[, (count, gamma, cy, cs)]), a = the trial steps (k = len(a)).
    Returns dict(rows= uint64 [npass, batch, 64] (the bits of the row every workgroup holds after that pass; NAN_PATTERN where
    nothing was stored), width=, stored= [npass, batch], ts= [npass, batch, 7, 7], gu=, uu= [npass, batch], x=, u= [batch, ld],
    S=, Y= [batch, m + 1, ld], qn=, g= [batch, ld] (gradient=True), reason=, done=, passes= [batch], points=, ld=, symbol=)."""
    if tier not in BATCH_PROBE_TIERS:
        raise ValueError(f"tier must be one of {sorted(BATCH_PROBE_TIERS)}, not {tier!r}")
    model = obj_or_kind if isinstance(obj_or_kind, DeviceObjective) else None
    if model is None and obj_or_kind not in OBJ_KINDS:
        raise ValueError(f"unknown objective kind {obj_or_kind!r}")
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
    if X.ndim != 2:
        raise ValueError("X must be [batch, n]")
    batch, n = X.shape
    U = _batch_rows("U", U, X.shape)
    ld = n + (n & 1)
    keep = [X, U]
    p = _lib.BatchProbeC()
    p.tier, p.m, p.n, p.batch = BATCH_PROBE_TIERS[tier], int(m), n, batch
    p.obj_kind = 4 if model is not None else OBJ_KINDS[obj_or_kind]   # (4: CGO_OBJ_USER)
    p.model = model._h if model is not None else None
    p.x, p.u = X.ctypes.data_as(dp), U.ctypes.data_as(dp)
    Pc = [_batch_rows(f"params[{j}]", v, X.shape) for j, v in enumerate(params or [])]
    if len(Pc) > 4:
        raise ValueError("at most 4 parameter slots")
    keep += Pc
    p.n_params = len(Pc)
    for j, v in enumerate(Pc):
        p.params[j] = v.ctypes.data_as(dp)
    if scalars is not None:
        scalars = _batch_rows("scalars", scalars, (batch,))
        p.scalars = scalars.ctypes.data_as(dp)
    if skip is not None:
        skip = np.ascontiguousarray(np.asarray(skip, dtype=np.uint8))
        if skip.shape != (batch,):
            raise ValueError("skip must be [batch]")
        p.skip = skip.ctypes.data_as(C.POINTER(C.c_uint8))
    qw = batch_probe_qn_words()
    ring = tier in ("lbfgs", "lbfgs_lds")
    if ring:
        S = _batch_rows("S", S, (batch, m + 1, n))
        Y = _batch_rows("Y", Y, (batch, m + 1, n))
        qn = np.ascontiguousarray(np.asarray(qn, dtype=np.uint64))
        if qn.shape != (batch, qw):
            raise ValueError(f"qn must be [batch, {qw}] 8-byte words")
        p.S, p.Y, p.qn = S.ctypes.data_as(dp), Y.ctypes.data_as(dp), qn.ctypes.data_as(C.c_void_p)
    if len(script) > 32:
        raise ValueError("batch_probe: at most 32 passes")
    p.npass = len(script)
    for q, item in enumerate(script):
        c = p.pass_[q]
        a = []
        if item[0] == "trial":
            c.kind, a = 0, item[1]
        elif item[0] == "accept_dir_trial":
            c.kind, c.a_acc, c.beta, a = 1, float(item[1]), float(item[2]), item[3]
        elif item[0] == "init":
            c.kind = 2
        elif item[0] == "push":
            c.kind, c.a_acc = 3, float(item[1])
        elif item[0] == "combine":
            c.kind, a = 4, item[1]
            if len(item) > 2 and item[2] is not None:
                cnt, gamma, cy, cs = item[2]
                if len(cy) > 10 or len(cs) > 10:
                    raise ValueError("batch_probe: at most 10 coefficients")
                c.co_set, c.co_count, c.co_gamma = 1, int(cnt), float(gamma)
                c.co_cy[:len(cy)] = [float(v) for v in cy]
                c.co_cs[:len(cs)] = [float(v) for v in cs]
        else:
            raise ValueError(f"batch_probe: no pass kind {item[0]!r}")
        if len(a) > 7:
            raise ValueError("batch_probe: at most 7 trial steps")
        c.k = len(a)
        c.a[:len(a)] = [float(v) for v in a]
    npass = max(p.npass, 1)
    rows = np.full((npass, batch, BATCH_PROBE_ROW), NAN_PATTERN, dtype=np.uint64)
    out = (_lib.BatchPassOutC * (npass * batch))()
    xo, uo = np.empty((batch, ld)), np.empty((batch, ld))
    reason, done, passes = np.zeros(batch, dtype=np.int32), np.zeros(batch, dtype=np.int64), np.zeros(batch, dtype=np.int64)
    p.rows, p.out = rows.ctypes.data_as(dp), out
    p.x_out, p.u_out = xo.ctypes.data_as(dp), uo.ctypes.data_as(dp)
    p.reason, p.done, p.passes = reason.ctypes.data_as(C.POINTER(C.c_int32)), done.ctypes.data_as(i64p), passes.ctypes.data_as(i64p)
    go = So = Yo = qo = None
    if gradient:
        go = np.empty((batch, ld))
        p.g_out = go.ctypes.data_as(dp)
    if ring:
        So, Yo = np.empty((batch, m + 1, ld)), np.empty((batch, m + 1, ld))
        qo = np.zeros((batch, qw), dtype=np.uint64)
        p.S_out, p.Y_out, p.qn_out = So.ctypes.data_as(dp), Yo.ctypes.data_as(dp), qo.ctypes.data_as(C.c_void_p)
    ctx = ctx or (model.ctx if model is not None else default_context())   # (argument errors above need no device)
    check(_lib.lib().cgo_batch_probe(ctx._h, C.byref(p)))
    del keep
    o = np.frombuffer(out, dtype=np.float64).reshape(npass, batch, 53)
    return dict(rows=rows, width=o[:, :, 51].view(np.int64).copy(), stored=o[:, :, 52].view(np.int64).copy(),
                ts=o[:, :, :49].reshape(npass, batch, 7, 7).copy(), gu=o[:, :, 49].copy(), uu=o[:, :, 50].copy(),
                x=xo, u=uo, S=So, Y=Yo, qn=qo, g=go, reason=reason, done=done, passes=passes, points=int(p.points),
                ld=int(p.ld), symbol=p.symbol.decode())


def batch_lbfgs_shape():
    """(lanes per workgroup, pairs of elements per lane and trip) of the two ring passes of minimizeobjectivebatch_lbfgs."""
    blk, u = C.c_int32(0), C.c_int32(0)
    _lib.lib().cgo_batch_lbfgs_shape(C.byref(blk), C.byref(u))
    return int(blk.value), int(u.value)


def batch_lbfgs_max_m() -> int:
    """Largest history length m of a batched L-BFGS solve."""
    return int(_lib.lib().cgo_batch_lbfgs_max_m())


def _batch_lbfgs_policy(rows) -> Optional["_lib.BatchPolicyC"]:
    """`rows` of a batched L-BFGS call as a cgo_batch_policy — None for "device", the calls without a policy.  Checked and
    built without any library call."""
    if not isinstance(rows, str) or rows not in BATCH_ROWS:
        raise ValueError(f"rows must be one of 'device', 'lds', 'auto', not {rows!r}")
    if rows == "device":
        return None
    pol = _lib.BatchPolicyC()
    pol.size, pol.rows = C.sizeof(_lib.BatchPolicyC), BATCH_ROWS[rows]
    return pol


def _batch_lbfgs_m(m, rows: str) -> int:
    if rows == "lds" and m is None:
        raise ValueError("rows='lds' needs m: what one workgroup's LDS holds depends on the ring depth")
    if m is not None and (not isinstance(m, (int, np.integer)) or isinstance(m, bool)):
        raise ValueError("m must be an integer")
    return 1 if m is None else int(m)


def batch_lbfgs_max_n(kind: str, ctx: Optional[Context] = None, m: Optional[int] = None, rows: str = "device") -> int:
    """Largest n of one problem of minimizeobjectivebatch_lbfgs.  rows="device" (the default) / "auto": the index range of a
    pass (memory is the other limit, checked by the call).  rows="lds": what one workgroup's LDS holds of the problem's
    batch_lbfgs_lds_rows(K, m) rows — `m` is required; 0 for m outside 1 … batch_lbfgs_max_m()."""
    if kind not in OBJ_KINDS:
        raise ValueError(f"unknown objective kind {kind!r}")
    pol = _batch_lbfgs_policy(rows)
    mm = _batch_lbfgs_m(m, rows)
    ctx = ctx or default_context()
    if pol is None and m is None:
        return int(_lib.lib().cgo_batch_lbfgs_max_n(ctx._h, OBJ_KINDS[kind]))
    return int(_lib.lib().cgo_batch_lbfgs_max_n_ex(ctx._h, OBJ_KINDS[kind], mm, C.byref(pol) if pol is not None else None))


def batch_lbfgs_lds_rows(n_params: int, m: int) -> int:
    """Rows of n + n%2 doubles a problem of rows="lds" keeps in its workgroup's LDS: x, u, the n_params slots and the ring —
    2 + n_params + 2(m+1); 0 for n_params outside 0 … 4 or m outside 1 … 10.  Needs no device."""
    return int(_lib.lib().cgo_batch_lbfgs_lds_rows(int(n_params), int(m)))


def batch_lbfgs_lds_shape(n_params: int = 0):
    """(lanes per workgroup, pairs of elements per lane and trip) of the two ring passes of rows="lds" on an objective of
    `n_params` parameter slots (no bit of a result depends on it).  Needs no device."""
    blk, u = C.c_int32(0), C.c_int32(0)
    _lib.lib().cgo_batch_lbfgs_lds_shape(int(n_params), C.byref(blk), C.byref(u))
    return int(blk.value), int(u.value)


def minimizeobjectivebatch_lbfgs(kind: str, X0, config: CGConfig, linesearch_config: LineSearchConfig, D=None,
                                 ctx: Optional[Context] = None, slice_iters: int = 0, rows: str = "device") -> BatchResults:
    """minimizeobjectivebatch with a quasi-Newton direction: `config.β_config` is LBFGS(m), 1 ≤ m ≤ batch_lbfgs_max_m() = 10
    (minimizeobjectivebatch is the CG flavours' and refuses it).  kind: "quad_diag" (D: [batch, n]), "rosenbrock_paired" (n even)
    or "booth" (n = 2); StrongWolfeBisection or WolfeBisection.  One workgroup per problem; the rows of x, u, D and a ring of
    2(m+1) rows per problem stay in device memory — (3 + K + 2(m+1)) · batch · (n + n%2) · 8 bytes, checked against the device's
    free memory before anything is allocated.  Returns what minimizeobjectivebatch returns (`.rows`: the tier that ran).
    rows: "device" (the default): every pass streams the problem's rows and ring from device memory.  "lds": a workgroup keeps
    them in its LDS during a launch and writes back what it changed — n ≤ batch_lbfgs_max_n(kind, m=m, rows="lds"), refused
    beyond; every number returned has the bits of "device".  "auto": "device" at every n — the LDS tier did not beat the device tier by more than its spread at every
    measured shape, so it is reached by asking for it.  A problem
    the device loop does not finish is solved AGAIN from its own x0 by the ordinary engine — a whole solve — and counted in
    `handed_back`.  Anything not covered raises CgoError: Backtracking, m > 10, a multi-rank context.  Run-time compiled
    objectives, with parameter slots and a scalar per problem: minimizeobjectivebatch_lbfgs_obj."""
    if not isinstance(kind, str) or kind not in OBJ_KINDS:
        raise ValueError(f"unknown objective kind {kind!r} (a run-time compiled objective: minimizeobjectivebatch_lbfgs_obj)")
    pol = _batch_lbfgs_policy(rows)
    X0, _ = _batch_inputs(X0)
    batch, n = X0.shape
    Dc = None if D is None else _batch_rows("D", D, X0.shape, "D must have the shape of X0")
    ctx = ctx or default_context()
    o = _BatchOut(batch, n, config)
    cfg, ls = config._c(), linesearch_config._c()
    if pol is None:   # the default: exactly the call without a policy
        check(_lib.lib().cgo_minimize_batch_lbfgs(ctx._h, OBJ_KINDS[kind], n, batch, X0.ctypes.data_as(dp),
                                                  Dc.ctypes.data_as(dp) if Dc is not None else None, C.byref(cfg), C.byref(ls),
                                                  int(slice_iters), C.byref(o.c)))
        return o.results(rows_used=BATCH_ROWS["device"])
    used = C.c_int32(BATCH_ROWS["device"])
    check(_lib.lib().cgo_minimize_batch_lbfgs_ex(ctx._h, OBJ_KINDS[kind], n, batch, X0.ctypes.data_as(dp),
                                                 Dc.ctypes.data_as(dp) if Dc is not None else None, C.byref(cfg), C.byref(ls),
                                                 int(slice_iters), C.byref(pol), C.byref(o.c), C.byref(used)))
    return o.results(rows_used=used.value)


def batch_lbfgs_shape_obj(n_params: int):
    """(lanes per workgroup, pairs of elements per lane and trip) of the two ring passes of minimizeobjectivebatch_lbfgs_obj on a
    model of `n_params` parameter slots: fewer pairs per trip for two or more slots (no bit of a result depends on it)."""
    blk, u = C.c_int32(0), C.c_int32(0)
    _lib.lib().cgo_batch_lbfgs_shape_obj(int(n_params), C.byref(blk), C.byref(u))
    return int(blk.value), int(u.value)


def batch_lbfgs_max_n_obj(model: "DeviceObjective", m: Optional[int] = None, rows: str = "device") -> int:
    """Largest n of one problem of minimizeobjectivebatch_lbfgs_obj on `model` (0: not a run-time compiled, whole, single-rank
    objective).  rows="device" (the default) / "auto": the index range of a pass; compiles nothing.  rows="lds": what one
    workgroup's LDS holds of the problem's rows and ring for ring depth `m` (required) — the first such call on a compiled source
    compiles its program of that tier, as batch_max_n compiles the batch program."""
    if not isinstance(model, DeviceObjective):
        raise ValueError("model must be a run-time compiled DeviceObjective (ElementwiseObjective)")
    pol = _batch_lbfgs_policy(rows)
    mm = _batch_lbfgs_m(m, rows)
    if pol is None and m is None:
        return int(_lib.lib().cgo_batch_lbfgs_max_n_obj(model._h))
    return int(_lib.lib().cgo_batch_lbfgs_max_n_obj_ex(model._h, mm, C.byref(pol) if pol is not None else None))


def minimizeobjectivebatch_lbfgs_obj(model: "DeviceObjective", X0, config: CGConfig, linesearch_config: LineSearchConfig,
                                     params=None, scalars=None, ctx: Optional[Context] = None, slice_iters: int = 0,
                                     rows: str = "device") -> BatchResults:
    """minimizeobjectivebatch_lbfgs on a run-time compiled objective: `model` (ElementwiseObjective) as in minimizeobjectivebatch
    — its source, size, scalar and cost class are every problem's — with `params`, its n_params arrays [batch, n], the rows of
    slot 0, 1, …, and optionally `scalars`, a [batch] array of every problem's own `s0` (None: the model's for all).
    `config.β_config` is LBFGS(m), 1 ≤ m ≤ 10; StrongWolfeBisection or WolfeBisection.  The first call on a compiled source
    compiles its batched L-BFGS program (seconds); later ones find it.  Device memory: (3 + n_params + 2(m+1)) · batch ·
    (n + n%2) · 8 bytes, checked before anything is allocated.  rows: "device" | "lds" | "auto" as in minimizeobjectivebatch_lbfgs
    (the limit of "lds": batch_lbfgs_max_n_obj(model, m=m, rows="lds"); its kernel is one more program of the source, compiled by
    the first call that runs the tier).  Returns what minimizeobjectivebatch_lbfgs returns (`.rows`: the tier that ran); a problem the device loop does not finish is solved again from its own x0, with its own slot rows and scalar, by
    the ordinary engine and counted in `handed_back`.  Not covered (CgoError or ValueError): CG flavours and Broyden
    (minimizeobjectivebatch), Backtracking, m > 10, a multi-rank context.  A batch that stays on the device between such
    solves, with an `active` mask: `BatchLBFGS`; box-constrained fits on it: primalbarriermethodbatch_lbfgs."""
    if not isinstance(model, DeviceObjective):
        raise ValueError("model must be a run-time compiled DeviceObjective (ElementwiseObjective); built-in kinds: minimizeobjectivebatch_lbfgs")
    pol = _batch_lbfgs_policy(rows)
    X0, Pc = _batch_inputs(X0, params, n=model.n_global, none_ok=False)
    batch, n = X0.shape
    sc = None
    if scalars is not None:
        sc = _batch_rows("scalars", scalars, (batch,))
        if not np.all(np.isfinite(sc)):
            raise ValueError("scalars must be finite")
    if not isinstance(slice_iters, (int, np.integer)) or slice_iters < 0:
        raise ValueError("slice_iters must be an integer ≥ 0")
    ctx = ctx or model.ctx
    o = _BatchOut(batch, n, config)
    cfg, ls = config._c(), linesearch_config._c()
    prows = (dp * max(len(Pc), 1))(*[v.ctypes.data_as(dp) for v in Pc])
    if pol is None:   # the default: exactly the call without a policy
        check(_lib.lib().cgo_minimize_batch_lbfgs_obj(ctx._h, model._h, batch, X0.ctypes.data_as(dp), prows, len(Pc),
                                                      sc.ctypes.data_as(dp) if sc is not None else None, C.byref(cfg), C.byref(ls),
                                                      int(slice_iters), C.byref(o.c)))
        return o.results(rows_used=BATCH_ROWS["device"])
    used = C.c_int32(BATCH_ROWS["device"])
    check(_lib.lib().cgo_minimize_batch_lbfgs_obj_ex(ctx._h, model._h, batch, X0.ctypes.data_as(dp), prows, len(Pc),
                                                     sc.ctypes.data_as(dp) if sc is not None else None, C.byref(cfg), C.byref(ls),
                                                     int(slice_iters), C.byref(pol), C.byref(o.c), C.byref(used)))
    return o.results(rows_used=used.value)


class Batch:
    """`batch` problems of one run-time compiled objective that STAY ON THE DEVICE between solves (cgo_batch_open): `model` as
    in minimizeobjectivebatch, `params` its n_params arrays [batch, n], uploaded once.  `solve` then runs the batch any number
    of times — each call from its own X0, under its own config and line search, optionally with a scalar per problem and with
    only some of the problems.  rows: "lds" | "device" | "auto", as in minimizeobjectivebatch; `.rows` says which tier the open
    batch runs in.  A context manager; `close` frees the device rows."""

    _NAME, _SOLVE = "Batch", "cgo_batch_solve"   # the class in messages, the C symbol of `solve`

    def __init__(self, model: DeviceObjective, params, batch: int, rows: str = "lds"):
        self._h = None
        pol = _batch_policy(rows)
        polp = C.byref(pol) if pol is not None else None
        self._open(model, params, batch, lambda c, mh, b, pr, k, h: _lib.lib().cgo_batch_open_ex(c, mh, b, pr, k, polp, h))

    def _open(self, model, params, batch, open_call, m=None):
        """What both kinds of handle check and do to open: `open_call(ctx, model, batch, slot rows, n_params, handle)` is the C call;
        `m`: the ring depth of a BatchLBFGS (`.m`)."""
        if not isinstance(model, DeviceObjective) or model.kind != "user":
            raise ValueError(f"{self._NAME}: the model must be a run-time compiled objective (ElementwiseObjective)")
        if m is not None and (not isinstance(m, (int, np.integer)) or isinstance(m, bool)):
            raise ValueError(f"{self._NAME}: m must be an integer")
        self.model, self.batch, self.n = model, int(batch), int(model.n_global)
        if m is not None:
            self.m = int(m)
        if self.batch < 1:
            raise ValueError(f"{self._NAME}: batch must be ≥ 1")
        Pc = [_batch_rows(f"params[{j}]", v, (self.batch, self.n)) for j, v in enumerate(params or [])]
        prows = (dp * max(len(Pc), 1))(*[v.ctypes.data_as(dp) for v in Pc])
        h = C.c_void_p()
        ctx_h = model.ctx._h if model.ctx is not None else None
        check(open_call(ctx_h, model._h, self.batch, prows, len(Pc), C.byref(h)))
        self._h = h
        used = C.c_int32(0)
        check(_lib.lib().cgo_batch_rows(h, C.byref(used)))
        self._rows_used = int(used.value)
        self.rows = _BATCH_ROWS_NAMES[self._rows_used]

    def solve(self, X0, config: CGConfig, linesearch_config: LineSearchConfig, scalars=None, active=None,
              slice_iters: int = 0) -> BatchResults:
        """One batched solve from X0 ([batch, n]).  scalars: [batch], every problem's own `s0` (None: the model's for all — then
        every number is what the one-shot call returns).  active: [batch] booleans, the problems that run (None: all); the
        entry of an inactive problem in the returned list is None.  On a `BatchLBFGS`: `config.β_config` is LBFGS(m) with m ≤ `.m`;
        every ring starts empty with this solve's m, so nothing of an earlier solve is read, and every number has the bits of
        minimizeobjectivebatch_lbfgs_obj with the same inputs, rows and m.  A problem the device loop does not finish is solved
        again from its row of X0 by the ordinary engine, with the handle's slot rows and its own scalar, and counted in
        `handed_back`."""
        if self._h is None:
            raise ValueError(f"{self._NAME}: closed")
        X0 = _batch_rows("X0", X0, (self.batch, self.n))
        sc = None if scalars is None else _batch_rows("scalars", scalars, (self.batch,))
        ac = None
        if active is not None:
            ac = np.ascontiguousarray(np.asarray(active).astype(bool).astype(np.uint8))
            if ac.shape != (self.batch,):
                raise ValueError(f"active must be [{self.batch}]")
        o = _BatchOut(self.batch, self.n, config)
        cfg, ls = config._c(), linesearch_config._c()
        check(getattr(_lib.lib(), self._SOLVE)(self._h, X0.ctypes.data_as(dp), sc.ctypes.data_as(dp) if sc is not None else None,
                                               ac.ctypes.data_as(C.POINTER(C.c_uint8)) if ac is not None else None, C.byref(cfg),
                                               C.byref(ls), int(slice_iters), C.byref(o.c)))
        return o.results(ac, rows_used=self._rows_used)

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            _lib.lib().cgo_batch_close(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchLBFGS(Batch):
    """`Batch` for β = LBFGS(m) (cgo_batch_lbfgs_open): the slot rows of `params` go up once, and the rows of x, u, the gradient
    and a ring of 2(m+1) rows per problem stay allocated between solves — what minimizeobjectivebatch_lbfgs_obj allocates,
    uploads and frees on every call.  `m` is the largest history length a `solve` on the handle may ask for (1 …
    batch_lbfgs_max_m()); the device memory, (3 + n_params + 2(m+1)) · batch · (n + n%2) · 8 bytes, is checked against what is
    free before anything is allocated.  rows: "device" (the default) | "lds" | "auto", the rule of
    minimizeobjectivebatch_lbfgs — the limit of "lds" is batch_lbfgs_max_n_obj(model, m=m, rows="lds").  The tier's program of
    the model's source is compiled here, so a solve never compiles.  `.rows` says which tier the handle runs in, `.m` the m it
    was opened with.  A context manager; `close` frees the device rows."""

    _NAME, _SOLVE = "BatchLBFGS", "cgo_batch_lbfgs_solve"

    def __init__(self, model: DeviceObjective, params, batch: int, m: int, rows: str = "device"):
        self._h = None
        pol = _batch_lbfgs_policy(rows)
        polp = C.byref(pol) if pol is not None else None
        self._open(model, params, batch, lambda c, mh, b, pr, k, h: _lib.lib().cgo_batch_lbfgs_open(c, mh, b, pr, k, self.m, polp, h), m=m)


class UndefVarError(RuntimeError):
    """What the reference raises when solvesystem's line search finds no step (solve_system.jl:55 reads
    the loop variable `i` outside the loop)."""


def solvesystem(fdf, x_initial: Sequence[float], config: CGConfig, linesearch_config: LinesearchSolveSys,
                reference_throws: bool = False) -> Results:
    """solvesystem(fdf!, x_initial, config, linesearch_config)  (src/engine/solve_system.jl:64-237):
    the Hager–Zhang-type CG of (Yuan 2019) for g(x) = 0, where `fdf!` writes g(x) and returns any
    scalar to trace.  Restated bug for bug — see include/cgo.h, cgo_solver_create_sys.

    When no trial step passes the reference throws UndefVarError instead of returning its
    `:linesearch_failed` record; here that record (status "linesearch_failed", last good iterate) is
    returned, or the exception raised if `reference_throws=True`."""
    if not isinstance(linesearch_config, LinesearchSolveSys):
        raise TypeError("solvesystem takes a LinesearchSolveSys (setupLinesearchSolveSys)")
    s = Solver(fdf, config, linesearch_config)
    try:
        s.set_x0(np.asarray(x_initial, dtype=np.float64))
        s.start()
        while not s.iterate(1 << 40):
            pass
        r = s.results()
    finally:
        s.close()
    if reference_throws and r.status == "linesearch_failed":
        raise UndefVarError("UndefVarError: `i` not defined  (solve_system.jl:55)")
    return r


# ---------------------------------------------------------------------------
# primalbarriermethod! (src/engine/primal_barrier.jl) — a host-side CALLER of minimizeobjectivererun
# ---------------------------------------------------------------------------
@dataclass
class PrimalBarrierConfig:
    """PrimalBarrierConfig{T}  (primal_barrier.jl:130-136)."""
    barrier_tol: float
    barrier_growth_factor: float
    max_iters: int
    t_initial: float
    inf_f0_lb: float


def setupPrimalBarrierConfig(barrier_tol: float, barrier_growth_factor: float, max_iters: int,
                             t_initial: float = math.nan) -> PrimalBarrierConfig:
    """setupPrimalBarrierConfig(barrier_tol, barrier_growth_factor, max_iters; t_initial = NaN)  (:138-154)."""
    return PrimalBarrierConfig(barrier_tol, barrier_growth_factor, int(max_iters), t_initial, 0.0)


@dataclass
class PrimalBarrierResults:
    """PrimalBarrierResults{T,TrT}  (primal_barrier.jl:1-7)."""
    centering_results: List[List[Results]]
    status: str
    iters_ran: int
    t_final: float
    total_objective_evals: int


@dataclass
class BoxConstraints:
    """The box constraints lb ≤ x_d ≤ ub of examples/constrained.jl:18-48 (its `boxhdh!` + the
    `CvxInequalityConstraint` buffers, primal_barrier.jl:38-60) as a device-side descriptor: 2·D strict
    inequalities h(x) < 0, rows 1..D = x − ub, rows D+1..2D = lb − x.  The reference evaluates them as a
    dense 2D×D Jacobian on the host (O(D²) per call); here the log barrier ψ = −Σ log(−h_i) and its
    gradient (primal_barrier.jl:70-94) are element-wise terms inlined into the fused kernels.

    `lb`, `ub` are floats (one interval for every variable: the bounds are constants of the generated source) or
    length-D arrays (`lbs::Vector{T}`, `ubs::Vector{T}` of examples/constrained.jl:22-31: every variable its own
    interval; the bounds travel as the objective's last two parameter vectors).  One float and one array: the float
    is the same for every variable.  Every problem of a batch its own box: BatchBoxConstraints."""
    lb: Union[float, Sequence[float], np.ndarray]
    ub: Union[float, Sequence[float], np.ndarray]
    _NDIM = (1,)   # (a class attribute, not a field: the dimensions an array bound may have)

    def __post_init__(self):
        for name in ("lb", "ub"):
            v = getattr(self, name)
            if np.ndim(v) == 0:
                setattr(self, name, float(v))
            else:
                a = np.ascontiguousarray(v, dtype=np.float64)
                assert a.ndim in self._NDIM, f"BoxConstraints.{name}: a float or a one-dimensional array"
                setattr(self, name, a)
        if self.per_variable and np.ndim(self.lb) == 1 and np.ndim(self.ub) == 1:
            assert self.lb.size == self.ub.size, "BoxConstraints: lb and ub differ in length"

    @property
    def per_variable(self) -> bool:
        return np.ndim(self.lb) >= 1 or np.ndim(self.ub) >= 1

    def rows(self, batch: int, D: int):
        """(lbs, ubs) as [batch, D] arrays (primalbarriermethodbatch): a float or a length-D array is every problem's."""
        out = []
        for name in ("lb", "ub"):
            v = getattr(self, name)
            assert np.ndim(v) == 0 or v.shape in ((D,), (batch, D)), \
                f"BoxConstraints.{name} has shape {np.shape(v)} for {batch} problems of {D} variables"
            out.append(np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (batch, D))))
        return out[0], out[1]

    def vectors(self, D: int):
        """(lbs, ubs) as length-D arrays; AssertionError if an array bound has another length."""
        out = []
        for name in ("lb", "ub"):
            v = getattr(self, name)
            if np.ndim(v) == 0:
                v = np.full(D, float(v))
            assert v.size == D, f"BoxConstraints.{name} has {v.size} entries for {D} variables"
            out.append(v)
        return out[0], out[1]

    def n_constraints(self, D: int) -> int:
        return 2 * D


@dataclass
class BatchBoxConstraints(BoxConstraints):
    """BoxConstraints for primalbarriermethodbatch whose array bounds may also be [batch, D]: every problem its own set of bounds
    (a float or a length-D array is every problem's, as in BoxConstraints)."""
    _NDIM = (1, 2)


_BUILTIN_BASE_PARAMS = {"ObjQuadDiag": 1, "ObjRosenPaired": 0, "ObjBooth": 0}


def base_objective_params(base: str) -> int:
    """How many parameter vectors the base functor of barrier_objective_source reads."""
    if base.strip() in _BUILTIN_BASE_PARAMS:
        return _BUILTIN_BASE_PARAMS[base.strip()]
    m = re.search(r"\bkParams\s*=\s*(\d+)", base)
    if m:
        return int(m.group(1))
    m = re.search(r"\bkParam\s*=\s*(true|false)", base)
    assert m, "BaseObjective declares neither kParam nor kParams"
    return 1 if m.group(1) == "true" else 0


def barrier_objective_source(base: str, box: BoxConstraints) -> str:
    """HIP source of `t·f0(x) + ψ(x)` (evalbarrier!, primal_barrier.jl:111-128) around a base functor.
    `base` is the name of a built-in functor (ObjQuadDiag, ObjRosenPaired, ObjBooth) or the source of a
    `struct BaseObjective { kParam | kParams; kPairOnly; eval1; eval2 }`; t lives in the objective's scalar slot.
    Float bounds are constants of the source; array bounds are read from the two parameter slots after the base's own
    (lb, then ub), so the functor declares kParams = K_base + 2 (AssertionError if that exceeds 4)."""
    name = base.strip() if base.strip() in _BUILTIN_BASE_PARAMS else "BaseObjective"
    pre = "" if name != "BaseObjective" else base
    if box.per_variable:
        kb = base_objective_params(base)
        assert kb + 2 <= MAX_PARAM_SLOTS, f"the base objective reads {kb} parameter vectors: no two slots left for the bounds"
        return pre + f"""
struct UserObjective {{
    using B = {name};
    static constexpr int KB = obj_nparams<B>();                     // the base's own slots come first, then lb, then ub
    static_assert(KB == {kb}, "the base objective's parameter slots");
    static constexpr int kParams = KB + 2;
    static constexpr bool kParam = true;
    static constexpr bool kPairOnly = B::kPairOnly;
    __device__ static inline void bar(double x, double lb, double ub, double &psi, double &dpsi) {{
        const double hu = x - (ub), hl = (lb) - x;                   // fi_evals (examples/constrained.jl:31-32)
        const double cu = hu > 0.0 ? 0.0 : hu, cl = hl > 0.0 ? 0.0 : hl;  // clamp!(fi_evals, -Inf, 0)  (primal_barrier.jl:81)
        psi = -(log(-cu) + log(-cl));                                // ψ = −Σ log(−f_i)  (:82)
        double d = 0.0;
        d -= 1.0 / cu;                                               // dψ[d] −= df_i[d]/f_i  (:85-89), upper row
        d -= -1.0 / cl;                                              //                           lower row
        dpsi = d;
    }}
    __device__ static inline void eval1(double x, const double (&p)[kParams], double s0, double &f, double &g) {{
        double f0 = 0.0, g0 = 0.0, psi, dpsi;
        PS<B> pb;
        pb.v[0] = 0.0;
#pragma unroll
        for (int j = 0; j < KB; ++j) pb.v[j] = p[j];
        obj_eval1<B>(x, pb, 0.0, f0, g0);
        bar(x, p[KB], p[KB + 1], psi, dpsi);
        f += s0 * f0 + psi;                                          // t·f0 + ψ  (:127)
        g = s0 * g0 + dpsi;                                          // df = t·df0 + dψ  (:125)
    }}
    __device__ static inline void eval2(d2 xx, const d2 (&pp)[kParams], double s0, double &f, d2 &gg) {{
        double f0 = 0.0, psi0, psi1, d0, d1;
        d2 g0;
        PV<B> pb;
        pb.v[0] = d2{{0.0, 0.0}};
#pragma unroll
        for (int j = 0; j < KB; ++j) pb.v[j] = pp[j];
        obj_eval2<B>(xx, pb, 0.0, f0, g0);
        bar(xx.x, pp[KB].x, pp[KB + 1].x, psi0, d0);
        bar(xx.y, pp[KB].y, pp[KB + 1].y, psi1, d1);
        f += s0 * f0 + (psi0 + psi1);
        gg.x = s0 * g0.x + d0;
        gg.y = s0 * g0.y + d1;
    }}
}};
"""
    ub, lb = float(box.ub).hex(), float(box.lb).hex()
    return pre + f"""
struct UserObjective {{
    using B = {name};
    static constexpr bool kParam = B::kParam;
    static constexpr bool kPairOnly = B::kPairOnly;
    __device__ static inline void bar(double x, double &psi, double &dpsi) {{
        const double hu = x - ({ub}), hl = ({lb}) - x;              // fi_evals (examples/constrained.jl:31-32)
        const double cu = hu > 0.0 ? 0.0 : hu, cl = hl > 0.0 ? 0.0 : hl;  // clamp!(fi_evals, -Inf, 0)  (primal_barrier.jl:81)
        psi = -(log(-cu) + log(-cl));                                // ψ = −Σ log(−f_i)  (:82)
        double d = 0.0;
        d -= 1.0 / cu;                                               // dψ[d] −= df_i[d]/f_i  (:85-89), upper row
        d -= -1.0 / cl;                                              //                           lower row
        dpsi = d;
    }}
    __device__ static inline void eval1(double x, double p, double s0, double &f, double &g) {{
        double f0 = 0.0, g0 = 0.0, psi, dpsi;
        B::eval1(x, p, 0.0, f0, g0);
        bar(x, psi, dpsi);
        f += s0 * f0 + psi;                                          // t·f0 + ψ  (:127)
        g = s0 * g0 + dpsi;                                          // df = t·df0 + dψ  (:125)
    }}
    __device__ static inline void eval2(d2 xx, d2 pp, double s0, double &f, d2 &gg) {{
        double f0 = 0.0, psi0, psi1, d0, d1;
        d2 g0;
        B::eval2(xx, pp, 0.0, f0, g0);
        bar(xx.x, psi0, d0);
        bar(xx.y, psi1, d1);
        f += s0 * f0 + (psi0 + psi1);
        gg.x = s0 * g0.x + d0;
        gg.y = s0 * g0.y + d1;
    }}
}};
"""


def _base_objective_source(base: str) -> str:
    name = base.strip() if base.strip() in ("ObjQuadDiag", "ObjRosenPaired", "ObjBooth") else "BaseObjective"
    pre = "" if name != "BaseObjective" else base
    if base_objective_params(base) > 1:   # the array interface, as it is
        return pre + "\nstruct UserObjective : BaseObjective {};\n"
    return pre + f"""
struct UserObjective {{
    using B = {name};
    static constexpr bool kParam = B::kParam;
    static constexpr bool kPairOnly = B::kPairOnly;
    __device__ static inline void eval1(double x, double p, double s0, double &f, double &g) {{ B::eval1(x, p, s0, f, g); }}
    __device__ static inline void eval2(d2 xx, d2 pp, double s0, double &f, d2 &gg) {{ B::eval2(xx, pp, s0, f, gg); }}
}};
"""


def primalbarriermethod(constraints: BoxConstraints, f0df0: str, x_initial: Sequence[float],
                        centering_config: CGConfig, linesearch_config: LineSearchConfig,
                        barrier_config: PrimalBarrierConfig, *rerun_config_tuples,
                        param=None, ctx: Optional[Context] = None) -> PrimalBarrierResults:
    """primalbarriermethod!(constraints, f0df0!, hdh!, x_initial, centering_config, linesearch_config,
    barrier_config, rerun_config_tuples...)  (primal_barrier.jl:156-255; algorithm 11.1 of Boyd 2004).

    `(constraints, hdh!)` is a BoxConstraints descriptor and `f0df0` the base objective as device source
    (see barrier_objective_source); every centering step is one minimizeobjectivererun on the GPU.
    As in the reference, `x` is a copy of `x_initial` that is never updated (:172,:214-220): every centering
    step restarts from `x_initial`.  `param` holds the base objective's own parameter vectors: one array or a
    sequence of them.  Array bounds (BoxConstraints with length-D `lb` / `ub`) take two more slots."""
    x0 = np.ascontiguousarray(x_initial, dtype=np.float64)
    D = x0.size
    own = _param_list(param)
    if own is None:
        own = [] if param is None else [param]
    bar_param = base_param = param
    if constraints.per_variable:
        lbs, ubs = constraints.vectors(D)
        assert len(own) + 2 <= MAX_PARAM_SLOTS, f"{len(own)} parameter vectors of the base objective leave no two slots for the bounds"
        bar_param = own + [lbs, ubs]
        base_param = own if len(own) != 1 else own[0]
        if len(own) == 0:
            base_param = None
    bc = barrier_config
    rets: List[List[Results]] = []

    def assemble(status, it, t):                                    # assembleresults!  (:9-35)
        total = sum(int(e) for rr in rets[:it] for r in rr for e in r.trace.objective_evals)
        return PrimalBarrierResults(rets[:it], status, it, t, total)

    if np.any(x0 - constraints.ub >= 0.0) or np.any(constraints.lb - x0 >= 0.0):   # :178-191
        return assemble("infeasible_start", 0, bc.t_initial)
    obj = ElementwiseObjective(D, barrier_objective_source(f0df0, constraints), param=bar_param, ctx=ctx)
    try:
        t = bc.t_initial
        if not math.isfinite(t) or t < 0.0:                         # verifyt0  (:259-276)
            base = ElementwiseObjective(D, _base_objective_source(f0df0), param=base_param, ctx=ctx)   # f0 alone
            try:
                f_x0 = base(np.empty(D), x0)
            finally:
                base.close()
            t = (f_x0 - bc.inf_f0_lb) * bc.barrier_growth_factor
        for i in range(1, bc.max_iters + 1):                        # :208
            obj.set_scalar(t)
            rets.append(minimizeobjectivererun(obj, x0, centering_config, linesearch_config, *rerun_config_tuples))
            if rets[-1][-1].status != "success":
                return assemble("centering_step_issue", i, t)      # :215-223
            if constraints.n_constraints(D) / t < bc.barrier_tol:   # :229
                return assemble("success", i, t)
            t = bc.barrier_growth_factor * t                        # :240
        return assemble("max_iters_reached", bc.max_iters, t)
    finally:
        obj.close()


def _refuse_unbatched(config: CGConfig, linesearch_config: LineSearchConfig):
    """What the batched device loop does not run, in the library's words (check_batch_config) — before any work is done."""
    if isinstance(config.β_config, LBFGS):
        raise _lib.CgoError(1, "batched solves: β = L-BFGS is not supported (CG flavours only)")
    if isinstance(config.β_config, BroydenFamily):
        raise _lib.CgoError(1, "batched solves: β = Broyden family is not supported (CG flavours only)")
    if isinstance(linesearch_config, Backtracking):
        raise _lib.CgoError(1, "batched solves: the Backtracking line search is not supported (StrongWolfeBisection or WolfeBisection)")


def _primalbarrierbatch(open_batch, refuse, constraints: BoxConstraints, f0df0: str, X_initial, centering_config: CGConfig,
                        linesearch_config: LineSearchConfig, barrier_config: PrimalBarrierConfig, rerun_config_tuples,
                        params, ctx: Optional[Context]) -> List[PrimalBarrierResults]:
    """The loop of primalbarriermethodbatch and primalbarriermethodbatch_lbfgs.  `refuse(config, linesearch_config)` raises for a
    stage the handle does not run, before any work; `open_batch(model, rows, batch)` opens the handle — a `Batch` or a
    `BatchLBFGS` — every stage of every centering step, and the one evaluation of verifyt0, are solved on."""
    X0 = np.ascontiguousarray(np.asarray(X_initial, dtype=np.float64))
    if X0.ndim != 2:
        raise ValueError("X_initial must be [batch, D]")
    batch, D = X0.shape
    refuse(centering_config, linesearch_config)
    for tup in rerun_config_tuples:
        refuse(tup[0], tup[1])
    own = [_batch_rows(f"params[{j}]", v, (batch, D)) for j, v in enumerate(params or [])]
    bar_rows = list(own)
    if constraints.per_variable:
        assert len(own) + 2 <= MAX_PARAM_SLOTS, f"{len(own)} parameter vectors of the base objective leave no two slots for the bounds"
        lbs, ubs = constraints.rows(batch, D)
        bar_rows += [lbs, ubs]
    else:
        lbs, ubs = constraints.rows(batch, D)
    bc = barrier_config
    mu = bc.barrier_growth_factor
    stages = [(centering_config, linesearch_config)] + [(t[0], t[1]) for t in rerun_config_tuples]
    rets: List[List[List[Results]]] = [[] for _ in range(batch)]     # [problem][centering step][stage]

    def assemble(b, status, it, t):                                   # assembleresults!  (:9-35)
        total = sum(int(e) for rr in rets[b][:it] for r in rr for e in r.trace.objective_evals)
        return PrimalBarrierResults(rets[b][:it], status, it, float(t), total)

    out: List[Optional[PrimalBarrierResults]] = [None] * batch
    running = np.ones(batch, dtype=bool)
    infeasible = np.any(X0 - ubs >= 0.0, axis=1) | np.any(lbs - X0 >= 0.0, axis=1)      # :178-191
    for b in np.flatnonzero(infeasible):
        out[b] = assemble(b, "infeasible_start", 0, bc.t_initial)
        running[b] = False
    if not running.any():
        return out
    # (the models' own parameter vectors are never read by a batched solve: their slots stay reserved and unset)
    obj = ElementwiseObjective(D, barrier_objective_source(f0df0, constraints), param=[None] * len(bar_rows) if bar_rows else None, ctx=ctx)
    B = None
    try:
        t = np.full(batch, float(bc.t_initial))
        if not math.isfinite(bc.t_initial) or bc.t_initial < 0.0:     # verifyt0  (:259-276): f0(x_initial) of every problem, one launch
            base = ElementwiseObjective(D, _base_objective_source(f0df0), param=[None] * len(own) if own else None, ctx=ctx)
            try:
                with open_batch(base, own, batch) as B0:   # max_iters = 0: the initial evaluation (optim.jl:31) and nothing after it
                    c0 = CGConfig(centering_config.ϵ, centering_config.β_config, 0, False, DisableTrace())
                    r0 = B0.solve(np.where(running[:, None], X0, X0[np.flatnonzero(running)[0]]), c0, linesearch_config)
                f_x0 = np.array([r.objective for r in r0])
            finally:
                base.close()
            t = (f_x0 - bc.inf_f0_lb) * mu
        B = open_batch(obj, bar_rows, batch)
        for i in range(1, bc.max_iters + 1):                          # :208
            step: List[List[Results]] = [[] for _ in range(batch)]
            act, X = running.copy(), X0
            for k, (cfg_k, ls_k) in enumerate(stages):                # minimizeobjectivererun  (optim.jl:173-208)
                if k > 0:
                    act = act & np.array([bool(step[b]) and step[b][-1].status != "success" for b in range(batch)])
                    if not act.any():
                        break
                    X = np.array([step[b][-1].minimizer if act[b] else X0[b] for b in range(batch)])
                rs = B.solve(X, cfg_k, ls_k, scalars=np.where(running, t, 1.0), active=act)
                for b in np.flatnonzero(act):
                    step[b].append(rs[b])
            for b in np.flatnonzero(running):
                rets[b].append(step[b])
                if step[b][-1].status != "success":
                    out[b] = assemble(b, "centering_step_issue", i, t[b])   # :215-223
                elif constraints.n_constraints(D) / t[b] < bc.barrier_tol:   # :229
                    out[b] = assemble(b, "success", i, t[b])
                else:
                    t[b] = mu * t[b]                                  # :240
                    continue
                running[b] = False
            if not running.any():
                break
        for b in np.flatnonzero(running):
            out[b] = assemble(b, "max_iters_reached", bc.max_iters, t[b])
        return out
    finally:
        if B is not None:
            B.close()
        obj.close()


def primalbarriermethodbatch(constraints: BoxConstraints, f0df0: str, X_initial, centering_config: CGConfig,
                             linesearch_config: LineSearchConfig, barrier_config: PrimalBarrierConfig, *rerun_config_tuples,
                             params=None, ctx: Optional[Context] = None, rows: str = "lds") -> List[PrimalBarrierResults]:
    """primalbarriermethod for `batch` problems at once: X_initial is [batch, D], `params` the base objective's own [batch, D]
    rows (one array per slot), `constraints` one box for all (floats), one set of bounds for all (length-D arrays) or every
    problem's own ([batch, D] arrays: a BatchBoxConstraints).  The loop of primal_barrier.jl:156-255 with every scalar a [batch] array: t (verifyt0
    from ONE batched evaluation of f0), the status of the last stage, the stop tests.  Every stage of every centering step is
    ONE batched solve (`Batch.solve`) with scalars = t and active = the problems still running (for a rerun stage: those whose
    last status is not "success", from the previous stage's minimizers); `X_initial` is never updated, as in the reference.
    Returns what primalbarriermethod returns for each problem.  Configs the batched device loop does not run raise CgoError
    before any work (no loop of single solves).  rows: "lds" | "device" | "auto", passed on to every `Batch` (a box fit with
    per-variable bounds holds four slots: LDS ends at D = 3 352 there)."""
    _batch_policy(rows)
    return _primalbarrierbatch(lambda model, P, batch: Batch(model, P, batch, rows=rows), _refuse_unbatched, constraints, f0df0,
                               X_initial, centering_config, linesearch_config, barrier_config, rerun_config_tuples, params, ctx)


def _refuse_unbatched_lbfgs(config: CGConfig, linesearch_config: LineSearchConfig):
    """What a `BatchLBFGS` does not run, in the library's words (check_batch_lbfgs_call) — before any work is done."""
    if not isinstance(config.β_config, LBFGS):
        raise _lib.CgoError(1, "batched L-BFGS solves: β must be LBFGS(m) (CG flavours: primalbarriermethodbatch; the Broyden family has no batched form)")
    if isinstance(linesearch_config, Backtracking):
        raise _lib.CgoError(1, "batched L-BFGS solves: the Backtracking line search is not supported (StrongWolfeBisection or WolfeBisection)")


def primalbarriermethodbatch_lbfgs(constraints: BoxConstraints, f0df0: str, X_initial, centering_config: CGConfig,
                                   linesearch_config: LineSearchConfig, barrier_config: PrimalBarrierConfig, *rerun_config_tuples,
                                   params=None, ctx: Optional[Context] = None, rows: str = "device") -> List[PrimalBarrierResults]:
    """primalbarriermethodbatch with a quasi-Newton direction: the same loop, arguments and results, every stage of every
    centering step ONE `BatchLBFGS.solve` with scalars = t and active = the problems still running.  Every stage's β_config
    must be LBFGS(m) — each stage its own m; the handle is opened once with the largest — any other raises CgoError before any
    work and names primalbarriermethodbatch, and Backtracking is refused as there.  verifyt0 stays ONE batched evaluation of
    the base objective with max_iters = 0; it runs on a `BatchLBFGS` of its own on the base objective (the same rows and m as
    the fit's handle), under the centering stage's config.  rows: "device" (the default) | "lds" | "auto", the rule of
    minimizeobjectivebatch_lbfgs, passed on to both handles (with per-variable bounds a fit holds four slots: at m = 5 one
    workgroup's LDS then holds 18 rows of D + D%2 doubles)."""
    _batch_lbfgs_policy(rows)
    stages = [centering_config] + [t[0] for t in rerun_config_tuples]

    def open_batch(model, P, batch):   # (called after every stage has passed the refusal rule)
        return BatchLBFGS(model, P, batch, max(int(c.β_config.m) for c in stages), rows=rows)
    return _primalbarrierbatch(open_batch, _refuse_unbatched_lbfgs, constraints, f0df0, X_initial, centering_config,
                               linesearch_config, barrier_config, rerun_config_tuples, params, ctx)


def minimizeobjectivererun(fdf, x_initial, config: CGConfig, linesearch_config: LineSearchConfig,
                           *rerun_config_tuples) -> List[Results]:
    """minimizeobjectivererun(fdf!, x_initial, config, ls, rerun_config_tuples...)  (optim.jl:173-208).

    One call of cgo_minimize_rerun: every stage restarts from the previous stage's minimizer, which stays on the GPU
    (device-to-device copy between the stages).  On a sharded context every rank runs the chain on its own shard —
    `x_initial` is the GLOBAL vector, the returned minimizers / gradients are this rank's shards — and all ranks see the
    same statuses, hence the same number of stages."""
    if not isinstance(fdf, DeviceObjective):
        if not callable(fdf):
            raise TypeError("fdf! must be an objective descriptor or a closure fdf(g, x) -> f (no CPU solver path in this package)")
        host = HostObjective(fdf, len(x_initial))   # the reference's own call form: a closure
        try:
            rets = minimizeobjectivererun(host, x_initial, config, linesearch_config, *rerun_config_tuples)
            host.reraise()
            return rets
        finally:
            host.close()
    L = _lib.lib()
    npairs = len(rerun_config_tuples)
    n = fdf.n_local
    x0 = np.ascontiguousarray(fdf.local(np.asarray(x_initial, dtype=np.float64)), dtype=np.float64)
    cfgs = [config] + [t[0] for t in rerun_config_tuples]
    outs = (ResultsC * (1 + npairs))()
    bufs = []
    for i in range(1 + npairs):
        cap = max(cfgs[i].max_iters, 1)
        b = dict(x=np.empty(n), g=np.empty(n), to=np.zeros(cap), tg=np.zeros(cap), ts=np.zeros(cap),
                 te=np.zeros(cap, dtype=np.int64))
        outs[i].minimizer, outs[i].gradient = b["x"].ctypes.data_as(dp), b["g"].ctypes.data_as(dp)
        outs[i].trace_objective, outs[i].trace_grad_norm = b["to"].ctypes.data_as(dp), b["tg"].ctypes.data_as(dp)
        outs[i].trace_step_size = b["ts"].ctypes.data_as(dp)
        outs[i].trace_objective_evals = b["te"].ctypes.data_as(i64p)
        bufs.append(b)
    c0, l0 = config._c(), linesearch_config._c()
    rc = (CGConfigC * max(npairs, 1))(*[t[0]._c() for t in rerun_config_tuples])
    rl = (LSConfigC * max(npairs, 1))(*[t[1]._c() for t in rerun_config_tuples])
    nouts = C.c_int32(0)
    check(L.cgo_minimize_rerun(fdf.ctx._h, fdf._h, x0.ctypes.data_as(dp), C.byref(c0), C.byref(l0),
                               rc, rl, npairs, outs, C.byref(nouts)))
    rets = []
    for i in range(nouts.value):
        b, r = bufs[i], outs[i]
        k = int(r.iters_ran) if isinstance(cfgs[i].trace_status, EnableTrace) else 0
        tr = TraceContainer(b["to"][:k].copy(), b["tg"][:k].copy(), b["ts"][:k].copy(),
                            b["te"][:k].copy(), cfgs[i].trace_status)
        rets.append(Results(r.objective, b["x"], b["g"], int(r.iters_ran),
                            L.cgo_status_name(r.status).decode(), tr, int(r.total_fdf_evals),
                            int(r.total_launches)))
    return rets


# ---------------------------------------------------------------------------
# kernel-level entry points (generic dispatch functions of the reference)
# ---------------------------------------------------------------------------
def updatedir_(u: np.ndarray, df_x: np.ndarray, β: float, ctx: Optional[Context] = None):
    """updatedir!(u, df_x, β)  (cg_flavours.jl:2-15), in place; returns (g·u_new, u_new·u_new)."""
    ctx = ctx or default_context()
    assert u.shape == df_x.shape
    out = np.zeros(2)
    g = np.ascontiguousarray(df_x, dtype=np.float64)
    check(_lib.lib().cgo_kernel_dir(ctx._h, u.ctypes.data_as(dp), g.ctypes.data_as(dp), float(β),
                                    u.size, out.ctypes.data_as(dp)))
    return out[0], out[1]


def getβ(β_config: βConfig, g_next: np.ndarray, g: np.ndarray, u: np.ndarray,
         ctx: Optional[Context] = None) -> float:
    """getβ(β_config, g_next, g, u)::T  (cg_flavours.jl:46-170): one fused pass + scalar work."""
    ctx = ctx or default_context()
    gn = np.ascontiguousarray(g_next, dtype=np.float64)
    g = np.ascontiguousarray(g, dtype=np.float64)
    u = np.ascontiguousarray(u, dtype=np.float64)
    b = β_config._c()
    out = C.c_double()
    check(_lib.lib().cgo_getbeta(ctx._h, C.byref(b), gn.ctypes.data_as(dp), g.ctypes.data_as(dp),
                                 u.ctypes.data_as(dp), gn.size, C.byref(out)))
    return out.value


def beta_partials(g_next, g, u, ctx: Optional[Context] = None) -> np.ndarray:
    ctx = ctx or default_context()
    gn = np.ascontiguousarray(g_next, dtype=np.float64)
    g = np.ascontiguousarray(g, dtype=np.float64)
    u = np.ascontiguousarray(u, dtype=np.float64)
    out = np.zeros(9)
    check(_lib.lib().cgo_kernel_beta_partials(ctx._h, gn.ctypes.data_as(dp), g.ctypes.data_as(dp),
                                              u.ctypes.data_as(dp), gn.size, out.ctypes.data_as(dp)))
    return out


def evalϕdϕ(fdf: DeviceObjective, a: float, x: np.ndarray, u: np.ndarray):
    """evalϕdϕ!(xp, df_xp, fdf!, a, x, u)  (cg_utils.jl:4-23) → (ϕ, dϕ, df_xp)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    u = np.ascontiguousarray(u, dtype=np.float64)
    g = np.empty_like(x)
    out = np.zeros(2)
    check(_lib.lib().cgo_kernel_trial(fdf._h, x.ctypes.data_as(dp), u.ctypes.data_as(dp), float(a),
                                      g.ctypes.data_as(dp), out.ctypes.data_as(dp)))
    return out[0], out[1], g


def bench_stream_mix(n: int, reps: int = 9, ctx: Optional[Context] = None):
    """(median_us, best_us) of the accept+dir+trial read/write mix (R x,u,D / W x,u, 40 B/element) without its
    arithmetic, under the engine's pure-HBM streaming policy — the measured ceiling of the dominant launch on this box."""
    ctx = ctx or default_context()
    med, best = C.c_double(), C.c_double()
    check(_lib.lib().cgo_bench_stream_mix(ctx._h, int(n), int(reps), C.byref(med), C.byref(best)))
    return med.value, best.value


def bench_kernel(kind: int, n: int, reps: int = 20, fdf: Optional[DeviceObjective] = None,
                 ctx: Optional[Context] = None):
    ctx = ctx or (fdf.ctx if fdf else default_context())
    ms, b = C.c_double(), C.c_double()
    check(_lib.lib().cgo_bench_kernel(ctx._h, fdf._h if fdf else None, kind, n, reps, C.byref(ms),
                                      C.byref(b)))
    return ms.value, b.value
