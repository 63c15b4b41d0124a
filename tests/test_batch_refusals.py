"""What the batched entry points of the C API refuse, in which words, with which code and in which order: ONE table, read off
the library before its batched part became a translation unit of its own, and unchanged since.  A row is an entry point, the
wrong argument(s), the code and the full message.  Nothing is launched: every call ends at a refusal.

The order every entry point refuses in: null arguments, policy, objective, m_max (the L-BFGS open), config and call shape,
built-in shape rules or the model's params, scalars, active, tier, memory, remaining programs, allocation.  The rows of PAIRS
hold one pair of wrong arguments per adjacent pair of those phases and say which of the two errors is reported (active and
tier never meet in one entry point — a solve on a handle has no tier left to choose — so scalars meet the tier instead; a
program that does not compile needs another source, so the phases after memory have no pair)."""
import ctypes as C
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CG, LB, PR = "batched solves", "batched L-BFGS solves", "batch probe"
BODY = "const double d = x - p1; gi = p*d + s0*x; fi = 0.5*(p*d)*d + 0.5*((s0*x)*x);"
BATCH, N, M, GRID = 2, 4, 5, 0x7FFFFFFF
EINVAL, ENOMEM = 1, 6
QUAD, ROSEN, BOOTH, LSE = 0, 1, 2, 3
POLICY_SIZE = "cgo_batch_policy.size does not match this library (call cgo_batch_policy_init first)"
ROWS_ARE = "cgo_batch_policy.rows must be CGO_BATCH_ROWS_LDS, CGO_BATCH_ROWS_DEVICE or CGO_BATCH_ROWS_AUTO"
NOT_A_MODEL = (CG + ": the model must be a run-time compiled objective (cgo_objective_create_from_source[_ex]); built-in objectives: "
               "cgo_minimize_batch")
LBFGS_ON_CG = CG + ": β = L-BFGS is not supported (CG flavours only)"
BACKTRACKING = LB + ": the Backtracking line search is not supported (StrongWolfeBisection or WolfeBisection)"
M11 = " m = 11 exceeds cgo_batch_lbfgs_max_m = 10"


def cg_on_lbfgs(entry):
    return f"{LB}: β must be LBFGS(m) (CG flavours: {entry}; the Broyden family has no batched form)"


class Env:
    """One context, one model of two slots (run-time compiled once; the models of other sizes share its module), a handle
    of each kind, and every entry point as a function of keyword overrides of a CORRECT call."""

    def __init__(self, cgo):
        from cgo_amd import _lib
        self.cgo, self._lib, self.L = cgo, _lib, _lib.lib()
        self.dp = _lib.dp
        self.ctx = cgo.default_context()
        self.model = cgo.ElementwiseObjective(N, BODY, param=[None, None], ctx=self.ctx)
        self.builtin = cgo.QuadDiag(np.ones(N), ctx=self.ctx)
        self.keep = [np.ones((BATCH, N)) for _ in range(3)]
        self.x0, self.p0, self.p1 = (a.ctypes.data_as(self.dp) for a in self.keep)
        self.hz = cgo.setupCGConfig(1e-5, cgo.HagerZhang(), cgo.DisableTrace(), max_iters=10)._c()
        self.swb = cgo.setupStrongWolfeBisection(1e-5, 0.5)._c()
        self.bt = cgo.Backtracking(cgo.Armijo(1e-4), 0.5, 100, 50)._c()
        self.lds, self.device = self.policy(rows=0), self.policy(rows=1)
        self.models = {N: self.model}
        self.h_cg, self.h_lb = C.c_void_p(), C.c_void_p()
        assert self.call("open", handle=self.h_cg) == (0, "")
        assert self.call("lopen", handle=self.h_lb) == (0, "")
        # the limits the library itself reports (rows = lds; the L-BFGS ones for m = M)
        h, L, lds = self.ctx._h, self.L, C.byref(self.lds)
        self.lim = dict(cg=L.cgo_batch_max_n_ex(h, QUAD, lds), lb=L.cgo_batch_lbfgs_max_n_ex(h, QUAD, M, lds),
                        cgo=L.cgo_batch_max_n_obj_ex(self.model._h, lds), lbo=L.cgo_batch_lbfgs_max_n_obj_ex(self.model._h, M, lds),
                        cg_dev=L.cgo_batch_max_n_ex(h, ROSEN, C.byref(self.device)), lb_dev=L.cgo_batch_lbfgs_max_n(h, ROSEN))
        assert all(v >= 2 for v in self.lim.values()), self.lim

    def lbfgs(self, m=M):
        return self.cgo.setupCGConfig(1e-5, self.cgo.LBFGS(m), self.cgo.DisableTrace(), max_iters=10)._c()

    def policy(self, rows=0, size=None):
        p = self._lib.BatchPolicyC()
        self.L.cgo_batch_policy_init(C.byref(p))
        p.rows = rows
        if size is not None:
            p.size = size
        return p

    def model_of(self, n):
        if n not in self.models:
            self.models[n] = self.cgo.ElementwiseObjective(n, BODY, param=[None, None], ctx=self.ctx)
        return self.models[n]

    def close(self):
        self.L.cgo_batch_close(self.h_cg)
        self.L.cgo_batch_close(self.h_lb)
        for m in list(self.models.values()) + [self.builtin]:
            m.close()

    def call(self, entry, **kw):
        L, dp = self.L, self.dp
        lb = entry in ("lb", "lbo", "lopen", "lsolve")
        a = dict(ctx=self.ctx._h, kind=QUAD, n=N, batch=BATCH, x0=self.x0, param0=self.p0, cfg=self.lbfgs() if lb else self.hz,
                 ls=self.swb, slice_iters=0, pol=None, model=self.model._h, params=[self.p0, self.p1], n_params=2, scalars=None,
                 active=None, m_max=M, handle=None, h=self.h_lb if lb else self.h_cg, tier=0, m=0)
        a.update(kw)
        if "model_n" in a:
            a["model"] = self.model_of(a["model_n"])._h
        out, used = self._lib.BatchResultsC(), C.c_int32(0)
        cfg, ls = C.byref(a["cfg"]), C.byref(a["ls"])
        pol = C.byref(a["pol"]) if a["pol"] is not None else None
        params = (dp * 4)(*a["params"]) if a["params"] is not None else None
        sc = np.asarray(a["scalars"], dtype=np.float64) if a["scalars"] is not None else None
        scp = sc.ctypes.data_as(dp) if sc is not None else None
        ac = np.asarray(a["active"], dtype=np.uint8) if a["active"] is not None else None
        acp = ac.ctypes.data_as(C.POINTER(C.c_uint8)) if ac is not None else None
        if entry == "cg":
            rc = L.cgo_minimize_batch_ex(a["ctx"], a["kind"], a["n"], a["batch"], a["x0"], a["param0"], cfg, ls, a["slice_iters"], pol,
                                         C.byref(out), C.byref(used))
        elif entry == "lb":
            rc = L.cgo_minimize_batch_lbfgs_ex(a["ctx"], a["kind"], a["n"], a["batch"], a["x0"], a["param0"], cfg, ls, a["slice_iters"],
                                               pol, C.byref(out), C.byref(used))
        elif entry == "cgo":
            rc = L.cgo_minimize_batch_obj_ex(a["ctx"], a["model"], a["batch"], a["x0"], params, a["n_params"], cfg, ls, a["slice_iters"],
                                             pol, C.byref(out), C.byref(used))
        elif entry == "lbo":
            rc = L.cgo_minimize_batch_lbfgs_obj_ex(a["ctx"], a["model"], a["batch"], a["x0"], params, a["n_params"], scp, cfg, ls,
                                                   a["slice_iters"], pol, C.byref(out), C.byref(used))
        elif entry in ("open", "lopen"):
            h = a["handle"] if a["handle"] is not None else C.c_void_p()
            if entry == "open":
                rc = L.cgo_batch_open_ex(a["ctx"], a["model"], a["batch"], params, a["n_params"], pol, C.byref(h))
            else:
                rc = L.cgo_batch_lbfgs_open(a["ctx"], a["model"], a["batch"], params, a["n_params"], a["m_max"], pol, C.byref(h))
            if a["handle"] is None and h.value:   # a row of the table that is not refused: the assertion below reports it
                L.cgo_batch_close(h)
        elif entry in ("solve", "lsolve"):
            f = L.cgo_batch_solve if entry == "solve" else L.cgo_batch_lbfgs_solve
            rc = f(a["h"], a["x0"], scp, acp, cfg, ls, a["slice_iters"], C.byref(out))
        else:
            assert entry == "probe", entry
            p = self._lib.BatchProbeC()
            p.tier, p.obj_kind, p.m, p.n, p.batch = a["tier"], a["kind"], a["m"], a["n"], a["batch"]
            p.x, p.u, p.scalars = a["x0"], a["x0"], scp
            if a.get("on_model"):
                p.obj_kind, p.model, p.n_params = 4, a["model"], a["n_params"]
            for j, v in enumerate(a["params"] if a.get("on_model") else [a["param0"]]):
                p.params[j] = v
            p.npass = 1
            p.pass_[0].kind, p.pass_[0].k = 0, 1
            p.pass_[0].a[0] = 1.0
            rc = L.cgo_batch_probe(a["ctx"], C.byref(p))
        return rc, (L.cgo_last_error().decode() if rc else "")


@pytest.fixture(scope="module")
def env(cgo):
    e = Env(cgo)
    yield e
    e.close()


NAN1 = [1.0, float("nan")]
ONE_SHOT = ("cg", "lb", "cgo", "lbo")
PREFIX = dict(cg=CG, cgo=CG, open=CG, solve=CG, lb=LB, lbo=LB, lopen=LB, lsolve=LB)
CG_ENTRY = dict(lb="cgo_minimize_batch", lbo="cgo_minimize_batch_obj", lsolve="cgo_batch_solve")
TIERS = (0, 1, 2, 3)


def rows(e):
    """(name, entry, overrides, code, message); message: a string, or a compiled pattern where the text holds the free bytes"""
    lim = e.lim
    T = []

    def row(name, entry, code, msg, **kw):
        T.append((name, entry, kw, code, msg))
    # ---- one wrong argument ------------------------------------------------------------------------------------------------
    for en in ONE_SHOT + ("open", "lopen"):
        row("batch 0", en, EINVAL, PREFIX[en] + ": batch must be ≥ 1", batch=0)
        row("policy size", en, EINVAL, POLICY_SIZE, pol=e.policy(size=8))
        row("rows 7", en, EINVAL, PREFIX[en] + ": " + ROWS_ARE, pol=e.policy(rows=7))
    for en in ("cg", "lb"):
        row("odd Rosenbrock", en, EINVAL, PREFIX[en] + ": paired Rosenbrock needs an even n", kind=ROSEN, n=3)
        row("Booth at 4", en, EINVAL, PREFIX[en] + ": Booth is 2-dimensional (n = 2)", kind=BOOTH, n=4)
        row("no param0", en, EINVAL, PREFIX[en] + ": the quadratic needs param0, the [batch*n] rows of D", param0=None)
    for t in TIERS:
        m = M if t >= 2 else 0
        row("batch 0", "probe", EINVAL, PR + ": 1 ≤ batch ≤ the largest grid", tier=t, m=m, batch=0)
        row("odd Rosenbrock", "probe", EINVAL, PR + ": paired Rosenbrock needs an even n", tier=t, m=m, kind=ROSEN, n=3)
        row("Booth at 4", "probe", EINVAL, PR + ": Booth is 2-dimensional (n = 2)", tier=t, m=m, kind=BOOTH, n=4)
        row("no param0", "probe", EINVAL, PR + ": the quadratic needs params[0], the [batch*n] rows of D", tier=t, m=m, param0=None)
    for en in ("cgo", "lbo", "open", "lopen"):   # (the model's params are refused in the CG family's words everywhere)
        row("n_params off by one", en, EINVAL, CG + ": n_params = 1, the model reads 2 parameter slots", n_params=1)
        row("null params[1]", en, EINVAL, CG + ": params[1] is null (the [batch*n] rows of slot 1)", params=[e.p0, None])
    for t in (0, 1):
        row("n_params off by one", "probe", EINVAL, CG + ": n_params = 1, the model reads 2 parameter slots", tier=t, on_model=True, n_params=1)
        row("null params[1]", "probe", EINVAL, CG + ": params[1] is null (the [batch*n] rows of slot 1)", tier=t, on_model=True, params=[e.p0, None])
        row("scalars[1] = NaN", "probe", EINVAL, PR + ": scalars[1] is not finite", tier=t, on_model=True, scalars=NAN1)
    row("scalars[1] = NaN", "lbo", EINVAL, LB + ": scalars[1] is not finite", scalars=NAN1)
    for en in ("solve", "lsolve"):   # (the L-BFGS solve on a handle speaks with the CG family's prefix here)
        row("scalars[1] = NaN", en, EINVAL, CG + ": scalars[1] is not finite", scalars=NAN1)
        row("active all zero", en, EINVAL, CG + ": active selects no problem", active=[0, 0])
    for en in ("lb", "lbo", "lsolve"):
        row("CG flavour", en, EINVAL, cg_on_lbfgs(CG_ENTRY[en]), cfg=e.hz)
        row("Backtracking", en, EINVAL, BACKTRACKING, ls=e.bt)
        row("m = 11", en, EINVAL, LB + ":" + M11, cfg=e.lbfgs(11))
    for en in ("cg", "cgo", "solve"):
        row("LBFGS", en, EINVAL, LBFGS_ON_CG, cfg=e.lbfgs())
    for t in (2, 3):
        row("m = 11", "probe", EINVAL, PR + ":" + M11, tier=t, m=11)
    row("m_max = 0", "lopen", EINVAL, LB + ": m_max = 0 lies outside 1 … cgo_batch_lbfgs_max_m = 10", m_max=0)
    row("m > m_max", "lsolve", EINVAL, LB + ": m = 6 exceeds the m_max = 5 the handle was opened with", cfg=e.lbfgs(6))
    row("the other kind's handle", "lsolve", EINVAL, LB + ": the handle was opened for the CG flavours: cgo_batch_solve", h=e.h_cg)
    row("the other kind's handle", "solve", EINVAL, CG + ": the handle was opened for L-BFGS: cgo_batch_lbfgs_solve", h=e.h_lb)
    # n one above the LDS limit the library reports, rows = lds (the probe's tiers 0 and 3 are the LDS tiers)
    cg_lds = CG + ": n = {} exceeds what one workgroup's LDS holds ({} = {})"
    lb_lds = LB + ": n = {} exceeds what one workgroup's LDS holds of a problem's rows and ring ({} = {})"
    row("n above LDS", "cg", EINVAL, cg_lds.format(lim["cg"] + 1, "cgo_batch_max_n", lim["cg"]), n=lim["cg"] + 1, pol=e.lds)
    row("n above LDS", "probe", EINVAL, cg_lds.format(lim["cg"] + 1, "cgo_batch_max_n", lim["cg"]), n=lim["cg"] + 1, tier=0)
    row("n above LDS", "lb", EINVAL, lb_lds.format(lim["lb"] + 1, "cgo_batch_lbfgs_max_n_ex", lim["lb"]), n=lim["lb"] + 1, pol=e.lds)
    row("n above LDS", "probe", EINVAL, lb_lds.format(lim["lb"] + 1, "cgo_batch_lbfgs_max_n_ex", lim["lb"]), n=lim["lb"] + 1, tier=3, m=M)
    for en in ("cgo", "open"):
        row("n above LDS", en, EINVAL, cg_lds.format(lim["cgo"] + 1, "cgo_batch_max_n_obj", lim["cgo"]), model_n=lim["cgo"] + 1, pol=e.lds)
    row("n above LDS", "lbo", EINVAL, lb_lds.format(lim["lbo"] + 1, "cgo_batch_lbfgs_max_n_ex", lim["lbo"]), model_n=lim["lbo"] + 1, pol=e.lds)
    row("n above LDS", "lopen", EINVAL, lb_lds.format(lim["lbo"] + 1, "cgo_batch_lbfgs_max_n_obj_ex", lim["lbo"]), model_n=lim["lbo"] + 1, pol=e.lds)
    # per family, a byte count above the device's free memory, from the reported limits: refused before anything is allocated
    row("memory", "cg", ENOMEM, re.compile(CG + rf": the rows of {GRID} problems of n = {lim['cg_dev']} ask for \d+ bytes of device memory, \d+ are free"),
        kind=ROSEN, n=lim["cg_dev"], batch=GRID, pol=e.device)
    row("memory", "lb", ENOMEM, re.compile(LB + rf": the rows and rings \(m = {M}\) of {GRID} problems of n = {lim['lb_dev']} ask for \d+ bytes of device memory, \d+ are free"),
        kind=ROSEN, n=lim["lb_dev"], batch=GRID)
    # ---- PAIRS: two wrong arguments of adjacent phases, the earlier phase's error is reported ------------------------------------
    row("null | policy", "cg", EINVAL, "null argument", x0=None, pol=e.policy(size=8))
    row("policy | objective", "cg", EINVAL, CG + ": " + ROWS_ARE, pol=e.policy(rows=7), kind=LSE)
    row("policy | objective", "lbo", EINVAL, POLICY_SIZE, pol=e.policy(size=8), model=e.builtin._h)
    row("objective | m_max", "lopen", EINVAL, NOT_A_MODEL, model=e.builtin._h, m_max=0)
    row("m_max | call shape", "lopen", EINVAL, LB + ": m_max = 0 lies outside 1 … cgo_batch_lbfgs_max_m = 10", m_max=0, batch=0)
    row("objective | config", "lb", EINVAL, LB + ": the objective must be CGO_OBJ_QUAD_DIAG, CGO_OBJ_ROSENBROCK_PAIRED or CGO_OBJ_BOOTH", kind=LSE, cfg=e.hz)
    row("config | call shape", "lb", EINVAL, cg_on_lbfgs("cgo_minimize_batch"), cfg=e.hz, batch=0)
    row("call shape | built-in rules", "cg", EINVAL, CG + ": batch must be ≥ 1", batch=0, kind=ROSEN, n=3)
    row("call shape | params", "cgo", EINVAL, CG + ": batch must be ≥ 1", batch=0, n_params=1)
    row("params | scalars", "lbo", EINVAL, CG + ": n_params = 1, the model reads 2 parameter slots", n_params=1, scalars=NAN1)
    row("scalars | active", "solve", EINVAL, CG + ": scalars[1] is not finite", scalars=NAN1, active=[0, 0])
    row("scalars | active", "lsolve", EINVAL, CG + ": scalars[1] is not finite", scalars=NAN1, active=[0, 0])
    row("scalars | tier", "lbo", EINVAL, LB + ": scalars[1] is not finite", scalars=NAN1, model_n=lim["lbo"] + 1, pol=e.lds)
    row("built-in rules | tier", "cg", EINVAL, CG + ": the quadratic needs param0, the [batch*n] rows of D", param0=None, n=lim["cg"] + 1, pol=e.lds)
    row("tier | memory", "lb", EINVAL, lb_lds.format(lim["lb"] + 1, "cgo_batch_lbfgs_max_n_ex", lim["lb"]), n=lim["lb"] + 1, batch=GRID, pol=e.lds)
    row("probe: batch | built-in rules", "probe", EINVAL, PR + ": 1 ≤ batch ≤ the largest grid", batch=0, kind=ROSEN, n=3)
    return T


def test_every_refusal_keeps_its_code_its_words_and_its_place(env):
    table = rows(env)
    assert len(table) >= 100
    wrong = []
    for name, entry, kw, code, msg in table:
        rc, said = env.call(entry, **kw)
        same = msg.fullmatch(said) is not None if isinstance(msg, re.Pattern) else said == msg
        if rc != code or not same:
            what = {k: v for k, v in kw.items() if k in ("tier", "on_model", "n", "batch", "kind")}
            wrong.append(f"{entry} {what}, {name}: expected [{code}] {getattr(msg, 'pattern', msg)!r}, got [{rc}] {said!r}")
    assert not wrong, "\n".join(wrong)
    # the handles of the table still solve nothing by accident: neither was touched by a refused call
    used = C.c_int32(-1)
    assert env.L.cgo_batch_rows(env.h_cg, C.byref(used)) == 0 and used.value == 0
    assert env.L.cgo_batch_rows(env.h_lb, C.byref(used)) == 0 and used.value == 1
