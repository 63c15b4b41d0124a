"""Parameter vector slots 1–3 of run-time compiled objectives (cgo_objective_create_from_source_ex): every kernel family the
module instantiates reads K slots, through the C ABI and the Python interface.

One test objective with K = 3 whose three slots hold different data, so that a swapped, repeated or dropped slot shows:

    f = Σ ½ p (x − p1)² + p2·x          body: const double d = x - p1; gi = p*d + p2; fi = 0.5*((p*d)*d) + p2*x;

as an element-wise body, as a `kParams = 3` struct and as a numpy closure; K = 2 drops the p2 terms, K = 4 adds p3 like p2.

(1)–(3) hold every slot of every launch to exact dyadic sums with the models, data layout and comparison of
tests/test_kernel_sums.py, tests/test_stored_gradient_kernel_sums.py and tests/test_resident_kernel_sums.py: their cg_model /
fused_model call `obj.g2(x, p)` on a block of pairs and `obj.g1(x, p)` on the odd tail element, so the model here is an object
bound to its Data that looks the other slots up in the same block.  (4) the two source forms agree bit for bit, (5) whole
solves against the oracle run on the closure, (6) the ABI's behaviour.
"""
import threading

import numpy as np
import pytest

import test_kernel_sums as K
import test_resident_kernel_sums as R
import test_stored_gradient_kernel_sums as SG
from _cases import Case, O, Out, assert_parity, first_divergence, pin_points, rel, relf, run_oracle
from test_kernel_sums import A, M, S, Data, R_ACCEPT, R_DIR, R_GRAD, R_GRADT, R_INIT, R_PROJ, R_RESET, R_TRIAL, R_UPG, GRID_BIG

TOL = 1e-10

BODY = {2: "const double d = x - p1; gi = p*d; fi = 0.5*((p*d)*d);",
        3: "const double d = x - p1; gi = p*d + p2; fi = 0.5*((p*d)*d) + p2*x;",
        4: "const double d = x - p1; gi = (p*d + p2) + p3; fi = (0.5*((p*d)*d) + p2*x) + p3*x;"}
STRUCT3 = """
struct UserObjective {
    static constexpr int kParams = 3;
    static constexpr bool kPairOnly = false;
    __device__ static inline void eval1(double x, const double (&p)[3], double, double &f, double &g) {
        const double d = x - p[1];
        g = p[0]*d + p[2];
        f += 0.5*((p[0]*d)*d) + p[2]*x;
    }
    __device__ static inline void eval2(d2 x, const d2 (&p)[3], double s0, double &f, d2 &g) {
        const double pa[3] = {p[0].x, p[1].x, p[2].x}, pb[3] = {p[0].y, p[1].y, p[2].y};
        double g0, g1;
        eval1(x.x, pa, s0, f, g0);
        eval1(x.y, pb, s0, f, g1);
        g.x = g0; g.y = g1;
    }
};
"""
SLOT_KEYS = ("p", "p1", "p2", "p3")


class Slots:
    """The K-slot objective on one Data, in the shape of test_kernel_sums.Quad: g2 on the block of pairs, g1 on the odd tail."""
    name, kind, per_elem_f, param = "user_quad", "user_quad", True, True      # (name: the steps and scalars of the one-slot user body)

    def __init__(self, k, d):
        self.k, self.d = k, d

    def _eval(self, x, blk):
        dd = S(x, blk["p1"])
        pd = M(blk["p"], dd)
        g, f = pd, M(0.5, M(pd, dd))
        for key in SLOT_KEYS[2:self.k]:
            g = A(g, blk[key])
            f = A(f, M(blk[key], x))
        return f, g

    def g2(self, x, p):
        assert x.size == self.d.block["x"].size
        return self._eval(x, self.d.block)

    def g1(self, x, p):
        assert x.size == 1
        return self._eval(x, self.d.single)


_PERIOD = {}


def period():
    """The one-slot user body's exact period (x, u, p, x2, the stored g, gp) plus three more slots on x's grid."""
    if not _PERIOD:
        per = dict(SG.stored_period("user_quad"))
        rng = np.random.default_rng(2024)
        L = 2 * K.PERIOD_PAIRS
        per["p1"] = K._dy(rng, L, -4, 4, 0.25)
        per["p2"] = K._dy(rng, L, -3, 3, 0.5)
        per["p3"] = K._dy(rng, L, -2, 2, 0.25)
        _PERIOD.update(per)
    return _PERIOD


def slots_of(d, k):
    return [d.full[key] for key in SLOT_KEYS[:k]]


STEPS = K.STEPS["user_quad"]
A_ACC, BETA = K.SCAL["user_quad"]
ACC_T = R_ACCEPT | R_DIR | R_TRIAL
CG_LAUNCHES = [("init", R_INIT, 0), ("trial", R_TRIAL, 1), ("trial", R_TRIAL, 3), ("trial", R_TRIAL, 7), ("accept_dir_trial", ACC_T, 7),
               ("accept_dir", R_ACCEPT | R_DIR, 0), ("reset_dir", R_RESET, 0), ("upg_norm", R_UPG, 0), ("sys_project", R_PROJ, 1),
               ("scaled_norm", R_GRAD, 1), ("scaled_norm", R_GRADT, 1)]
FEW = [17, 513, 2 * (GRID_BIG * 8 + 1) + 1]                     # K = 2 and K = 4
RES_STATIC_LDS = R.STATIC_LDS[3]                               # k_resident<UserObjective, 3>


def res_keys(k):
    """(policy chunk, n): n = 2; 17 workgroups with one element in the last; 16 workgroups; 16 full workgroups and one element;
    the largest n the plan takes with 2 + k vectors in LDS."""
    return [(None, 2), (8, 129), (8, 128), (512, 16 * 512 + 1), (None, R.CUS * R.chunk_max(2 + k, RES_STATIC_LDS))]


def test_sizes_and_plans():
    """CPU tier: the resident sizes hit the edges they claim, and a slot costs the resident solver one LDS vector."""
    for k in (2, 3, 4):
        v = 2 + k
        assert R.plan(2, None, v, RES_STATIC_LDS) == (1, min(4096, R.chunk_max(v, RES_STATIC_LDS)))   # (five vectors and more: the default chunk no longer fits)
        assert R.plan(129, 8, v, RES_STATIC_LDS) == (17, 8) and R.last_chunk(129, 17, 8) == 1
        assert R.plan(128, 8, v, RES_STATIC_LDS) == (16, 8)
        assert R.plan(16 * 512 + 1, 512, v, RES_STATIC_LDS) == (17, 512)
        n = R.CUS * R.chunk_max(v, RES_STATIC_LDS)
        assert R.plan(n, None, v, RES_STATIC_LDS) == (256, R.chunk_max(v, RES_STATIC_LDS)) and R.plan(n + 1, None, v, RES_STATIC_LDS) is None
    assert R.chunk_max(5, RES_STATIC_LDS) == 3970 and R.chunk_max(5, RES_STATIC_LDS) < R.chunk_max(3, RES_STATIC_LDS)
    assert max(K.SIZES) <= 2 * (4096 * 16 + 1) + 1


def res_model_launch(model, npts, ks, ka):
    d = model.d
    script, rows = [], []
    for k in ks:
        script.append(("trial", STEPS[:k]))
        rows.append(R.expected_pass(model, d, npts, "trial", k, 0, 0)[0])
    x, u = d.full["x"], d.full["u"]
    if ka is not None:
        script.append(("accept_dir_trial", A_ACC, BETA, STEPS[:ka]))
        row, vec = R.expected_pass(model, d, npts, "accept", ka, A_ACC, BETA)
        rows.append(row)
        x, u = vec["x"], vec["u"]
    return script, rows, x, u


def test_exact_data_meet_their_preconditions():
    """CPU tier: every product exact, every slot's Σ|term| < 2⁵³ quanta, for every launch and size (1)–(3) run on the GPU."""
    for k, sizes in ((3, sorted(K.SIZES)[:6] + sorted(K.SIZES)[-4:]), (2, FEW), (4, FEW)):
        for n in sizes:
            d = Data(n, period())
            for kind, mode, kk in CG_LAUNCHES:
                K.expected_cg(Slots(k, d), d, mode, STEPS[:kk], A_ACC, BETA, with_u=K.needs_u(mode))
    for n in sorted(SG.S_SIZES)[:4] + sorted(SG.S_SIZES)[-5:]:
        d = Data(n, period())
        a_acc, beta, a = SG.SCAL["user_quad"]
        for _, mode in SG.LAUNCHES:
            SG.expected_fused(Slots(3, d), d, mode, a, a_acc, beta)
    for k in (2, 3, 4):
        for c, n in res_keys(k) if k == 3 else res_keys(k)[-1:]:
            d = Data(n, period())
            for ks, ka in R.launches_for(3):
                res_model_launch(Slots(k, d), 3, ks, ka)


def test_interface_is_declared():
    """CPU tier: the new functions are in the header and have ctypes signatures."""
    import cgo_amd
    from cgo_amd import _lib
    hdr = open(K.ROOT + "/include/cgo.h", encoding="utf-8").read()
    assert "#define CGO_MAX_PARAM_SLOTS 4" in hdr and cgo_amd.api.MAX_PARAM_SLOTS == 4
    for name in ("cgo_objective_create_from_source_ex", "cgo_objective_num_params", "cgo_objective_set_param_device"):
        assert f"int {name}(" in hdr and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["cgo_objective_create_from_source_ex"][1]) == 7
    assert len(_lib.SIGNATURES["cgo_objective_set_param_device"][1]) == 3


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def contexts(cgo):
    out = {name: cgo.Context(0) for name in K.TAILS}
    yield out
    for c in out.values():
        c.close()


@pytest.fixture(scope="module")
def modules(cgo, contexts):
    """Each distinct source compiled once for the whole file: the library shares a module between objectives of the same text
    while one of them is alive — these."""
    ctx = contexts["fused"]
    two = [np.ones(2)] * 4
    keep = [cgo.ElementwiseObjective(2, BODY[k], param=two[:k], ctx=ctx) for k in (2, 3, 4)]
    keep.append(cgo.ElementwiseObjective(2, STRUCT3, param=two[:3], ctx=ctx))
    yield keep
    for o in keep:
        o.close()


def _objective(cgo, k, d, ctx, source=None):
    return cgo.ElementwiseObjective(d.n, source or BODY[k], param=slots_of(d, k), ctx=ctx)


def _run_cg(cgo, contexts, k, n, tails, bigs=(False, True)):
    mism, cache = [], {}
    d = Data(n, period())
    model = Slots(k, d)
    for tail in tails:
        for big in bigs:
            o = _objective(cgo, k, d, contexts[tail])
            s = K._solver(cgo, o, tail, big)
            try:
                for kind, mode, kk in CG_LAUNCHES:
                    a = STEPS[:kk]
                    if (mode, kk) not in cache:
                        cache[(mode, kk)] = K.expected_cg(model, d, mode, a, A_ACC, BETA, with_u=K.needs_u(mode))
                    want_sums, want = cache[(mode, kk)]
                    got = s.probe_launch(kind, mode, A_ACC, BETA, a, d.full["x"], d.full["u"] if K.needs_u(mode) else None,
                                         d.full["x2"] if mode & R_PROJ else None)
                    tag = f"K={k} n={n} {tail} {'pure-HBM' if big else 'grid-stride'} {kind}/{mode} k={kk} [{got['symbol']}]"
                    if not got["symbol"].startswith(f"k_cg<UserObjective, {mode}, {K.npts_for(kk) if mode & R_TRIAL else 1}, "):
                        mism.append(f"{tag}: not the module's instantiation of this launch")
                    K._compare(tag, got, want_sums, want, mism)
            finally:
                s.close(); o.close()
    return mism


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(K.SIZES), ids=lambda n: f"n{n}")
def test_gradient_free_family_every_slot_exact(cgo, contexts, modules, n):
    """(1) k_cg<UserObjective, …> with K = 3: whole rows and x / u / g_out bit for bit, both streaming paths, three tails."""
    K._report(_run_cg(cgo, contexts, 3, n, tuple(K.TAILS)))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("n", FEW, ids=lambda n: f"n{n}")
def test_gradient_free_family_two_and_four_slots(cgo, contexts, modules, k, n):
    K._report(_run_cg(cgo, contexts, k, n, tuple(K.TAILS)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(SG.S_SIZES), ids=lambda n: f"n{n}")
def test_stored_gradient_family_every_slot_exact(cgo, contexts, modules, n):
    """(2) k_fused<UserObjective, …> (policy.stored_gradient) with K = 3, the row model of the stored-gradient suite."""
    mism, cache = [], {}
    d = Data(n, period())
    model = Slots(3, d)
    a_acc, beta, a = SG.SCAL["user_quad"]
    for tail in SG._tails(n):
        for big in (False, True):
            o = _objective(cgo, 3, d, contexts[tail])
            s = SG._solver(cgo, o, tail, big)
            try:
                for kind, mode in SG.LAUNCHES:
                    if mode not in cache:
                        cache[mode] = SG.expected_fused(model, d, mode, a, a_acc, beta)
                    want_sums, want = cache[mode]
                    got = s.probe_launch(kind, mode, a_acc, beta, [a] if mode & SG.M_TRIAL else [], d.full["x"],
                                         d.full["u"] if SG.reads_u(mode) else None, d.full["g"] if SG.reads_g(mode) else None)
                    tag = f"K=3 n={n} {tail} {'pure-HBM' if big else 'grid-stride'} {kind}/{mode} [{got['symbol']}]"
                    if got["symbol"] != SG.symbol_for("user_quad", mode, big):
                        mism.append(f"{tag}: expected {SG.symbol_for('user_quad', mode, big)}")
                    K._compare(tag, got, want_sums, want, mism)
            finally:
                s.close(); o.close()
    K._report(mism)


def _run_resident(cgo, ctx, k, key):
    chunk, n = key
    mism = []
    d = Data(n, period())
    model = Slots(k, d)
    o = _objective(cgo, k, d, ctx)
    s = R._solver(cgo, o, chunk, 3)
    try:
        rnd = 0
        for ks, ka in R.launches_for(3):
            script, rows, x, u = res_model_launch(model, 3, ks, ka)
            got = s.probe_resident(script, d.full["x"], d.full["u"])
            tag = f"K={k} n={n} chunk={chunk} grid={got['grid']}x{got['chunk']} round0={got['round0']} [{got['symbol']}]"
            assert (got["grid"], got["chunk"]) == R.plan(n, chunk, 2 + k, RES_STATIC_LDS), tag
            assert got["round0"] == rnd and got["points"] == 3 and "UserObjective" in got["symbol"], tag
            rnd += len(script)
            R.check_launch(tag, got, script, rows, x, u, 3, mism)
    finally:
        s.close(); o.close()
    return mism


@pytest.mark.gpu
@pytest.mark.parametrize("key", res_keys(3), ids=R._ids)
def test_resident_every_workgroup_exact(cgo, contexts, modules, key):
    """(3) k_resident<UserObjective, 3> with three parameter arrays in LDS: every workgroup's row of every pass."""
    R._report(_run_resident(cgo, contexts["fused"], 3, key))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 3, 4])
def test_resident_largest_size_shrinks_with_the_slots(cgo, contexts, modules, k):
    """The plan keeps 2 + K vectors in LDS: the largest n it takes runs exactly (K = 2, 4 here; K = 3 above), one element more
    is not the resident solver's: CGO_EINVAL."""
    n = R.CUS * R.chunk_max(2 + k, RES_STATIC_LDS)
    if k != 3:
        R._report(_run_resident(cgo, contexts["fused"], k, (None, n)))
    d = Data(n + 1, period())
    o = _objective(cgo, k, d, contexts["fused"])
    s = R._solver(cgo, o, None, 3)
    try:
        with pytest.raises(cgo.CgoError) as e:
            s.probe_resident([("trial", [0.25])], d.full["x"], d.full["u"])
        assert e.value.code == 1
    finally:
        s.close(); o.close()


# ---- whole solves --------------------------------------------------------------------------------------------------------------
def problem(n):
    p = O.fill_uniform(n, 3, 0.5, 4.0)
    p1 = O.fill_uniform(n, 5, -2.0, 2.0)
    p2 = O.fill_uniform(n, 6, -1.0, 1.0)
    x0 = O.fill_uniform(n, 4, -2.0, 2.0)

    def fdf(g, x):
        d = x - p1
        g[:] = p * d + p2
        return float(np.sum(0.5 * ((p * d) * d) + p2 * x))
    return (p, p1, p2), x0, fdf


def _solve(cgo, obj, x0, cfg, ls, policy=None):
    s = cgo.Solver(obj, cfg, ls, policy)
    try:
        s.enable_trial_log()
        s.set_x0(x0)
        s.start()
        while not s.iterate(1 << 40):
            pass
        r = s.results()
        la, lp, ld = s.trial_log()
    finally:
        s.close()
    return Out(r.objective, r.minimizer, r.gradient, r.iters_ran, r.status, r.trace.objective, r.trace.grad_norm, r.trace.step_size,
               r.trace.objective_evals, la, lp, ld, r.total_fdf_evals, r.total_launches)


@pytest.mark.gpu
def test_body_and_struct_forms_agree_bit_for_bit(cgo, gpu_ctx, modules, monkeypatch):
    """(4) the element-wise body and the kParams = 3 struct: the same bits, step logs and launch counts."""
    n = 4097
    slots, x0, _ = problem(n)
    ls = cgo.setupStrongWolfeBisection(1e-5, 0.1)
    a_obj = cgo.ElementwiseObjective(n, BODY[3], param=list(slots))
    b_obj = cgo.ElementwiseObjective(n, STRUCT3, param=list(slots))
    assert a_obj.n_params == b_obj.n_params == 3
    for pts in (3, 1, 7):
        pin_points(monkeypatch, pts)
        for beta in (cgo.PolakRibiere(), cgo.HagerZhang(), cgo.LBFGS(4)):
            cfg = cgo.setupCGConfig(1e-12, beta, cgo.EnableTrace(), max_iters=14)
            a, b = _solve(cgo, a_obj, x0, cfg, ls), _solve(cgo, b_obj, x0, cfg, ls)
            assert np.array_equal(a.log_a, b.log_a) and np.array_equal(a.log_phi, b.log_phi) and a.status == b.status
            assert a.iters_ran == b.iters_ran and a.total_launches == b.total_launches and a.objective == b.objective
            assert np.array_equal(a.minimizer, b.minimizer) and np.array_equal(a.gradient, b.gradient)
    a_obj.close(); b_obj.close()


CASES = [dict(beta="PolakRibiere", c2=0.1), dict(beta="DaiYuan", c2=0.8),
         dict(beta="HagerZhang", ls="WolfeBisection", cond="Wolfe", c1=1e-3, c2=0.9, ls_max_iters=100),
         dict(beta="LBFGS", m=5, c2=0.9), dict(beta="LBFGS", m=5, c2=0.9, env={"CGO_LBFGS_SPEC": "0"}),
         dict(beta="LBFGS", m=11, c2=0.9),
         # solvesystem: four iterations (≈ 300 trials).  Its step m comes out of differences of sums: at twelve iterations the two
         # CPU restatements of the reference (oracle/cgo_oracle.c, oracle/cgo_oracle_np.py) agree on this very problem only to
         # 9.5e-9 (n = 1001) with identical step logs — the reference's own rounding is then above the 1e-10 bar — and at six
         # to 4e-14; at four they agree to 1e-16: test_solvesystem_case_is_resolved_by_the_references.
         dict(beta="HagerZhang", ls="SolveSys", sys_s=0.25, max_iters=4)]


def _case(n, x0, fdf, kw, name):
    kw = {"max_iters": 12, **{k: v for k, v in kw.items() if k != "env"}}
    return Case(name, "closure", n, x0, eps=1e-12, extra={"fdf": fdf}, **kw)


def test_solvesystem_case_is_resolved_by_the_references():
    """CPU tier: on the solvesystem case of (5) the two independent restatements of the reference take the same steps and agree
    four orders of magnitude below the bar the device is held to."""
    from _cases import run_numpy
    for n in (1001, 4097):
        _, x0, fdf = problem(n)
        c = _case(n, x0, fdf, CASES[-1], "sys")
        a, b = run_oracle(c), run_numpy(c)
        assert np.array_equal(a.log_a, b.log_a) and rel(a.minimizer, b.minimizer) <= 1e-4 * TOL and relf(a.objective, b.objective) <= 1e-4 * TOL


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1001, 4097])
def test_solves_against_the_oracle_closure(cgo, gpu_ctx, modules, monkeypatch, n):
    """(5) the same expression as a numpy closure under the oracle: step logs and the 1e-10 bar."""
    from _cases import _product_structs
    slots, x0, fdf = problem(n)
    obj = cgo.ElementwiseObjective(n, BODY[3], param=list(slots))
    g, g_ref = np.zeros(n), np.zeros(n)
    f_dev, f_ref = obj(g, x0), fdf(g_ref, x0)
    assert np.array_equal(g, g_ref) and abs(f_dev - f_ref) <= 1e-13 * abs(f_ref)
    for i, kw in enumerate(CASES):
        for key, val in kw.get("env", {}).items():
            monkeypatch.setenv(key, val)
        c = _case(n, x0, fdf, kw, f"slots-{i}-{kw['beta']}")
        _, _, cfg, ls = _product_structs(c)
        ref = run_oracle(c)
        for resident in ((True, False) if kw["beta"] != "LBFGS" and kw.get("ls") != "SolveSys" else (None,)):
            pol = None if resident is None else cgo.SolverPolicy(resident=resident)
            assert_parity(_solve(cgo, obj, x0, cfg, ls, pol), ref, TOL, f"{c.name} resident={resident}")
        for key in kw.get("env", {}):
            monkeypatch.delenv(key)
    # a two-stage rerun chain: the second stage restarts from the first's minimizer, which stays on the device
    c1 = cgo.setupCGConfig(1e-12, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=4)
    c2 = cgo.setupCGConfig(1e-12, cgo.HagerZhang(), cgo.EnableTrace(), max_iters=8)
    ls = cgo.setupStrongWolfeBisection(1e-5, 0.1)
    rets = cgo.minimizeobjectivererun(obj, x0, c1, ls, (c2, ls))
    r1 = O.minimizeobjective(O.python_objective(fdf), x0, O.cg_config(1e-12, O.beta_config("PolakRibiere"), 4), O.strong_wolfe(1e-5, 0.1))
    r2 = O.minimizeobjective(O.python_objective(fdf), r1.minimizer, O.cg_config(1e-12, O.beta_config("HagerZhang"), 8), O.strong_wolfe(1e-5, 0.1))
    assert len(rets) == 2 and rets[0].status == r1.status and rets[1].status == r2.status and rets[1].iters_ran == r2.iters_ran
    assert np.array_equal(rets[1].trace.step_size, r2.trace_step_size)
    assert rel(rets[1].minimizer, r2.minimizer) <= TOL and relf(rets[1].objective, r2.objective) <= TOL
    obj.close()


def _uneven(W):
    def shard(n_global, rank, world):
        cuts = [0] + [2 * ((n_global * (r + 1) * (r + 2)) // (W * (W + 1)) // 2) for r in range(W - 1)] + [n_global]   # shares ∝ 1 : 2 : … : W, even offsets
        return cuts[rank], cuts[rank + 1] - cuts[rank]
    return shard


@pytest.mark.gpu
@pytest.mark.parametrize("W", [2, 8])
def test_virtual_ranks_pass_their_own_slice_of_every_slot(cgo, gpu_ctx, modules, W):
    """Uneven shards: slot 0 by fill_param (the device generator sees the shard's global offset), slot 1 from host memory,
    slot 2 device-to-device from a buffer of the shard on the GPU (a raw pointer from the HIP runtime the library already uses:
    a second runtime, as `import torch` after the library brings one, does not belong into this process)."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    n = 4097
    slots, x0, fdf = problem(n)
    shard = _uneven(W)
    assert all(shard(n, r, W)[0] % 2 == 0 and shard(n, r, W)[1] >= 1 for r in range(W)) and len({shard(n, r, W)[1] for r in range(W)}) == W
    ls = cgo.setupStrongWolfeBisection(1e-5, 0.1)
    for beta, name, m in ((cgo.PolakRibiere(), "PolakRibiere", 10), (cgo.LBFGS(4), "LBFGS", 4)):
        cfg = cgo.setupCGConfig(1e-12, beta, cgo.EnableTrace(), max_iters=10)
        ref = O.minimizeobjective(O.python_objective(fdf), x0, O.cg_config(1e-12, O.beta_config(name, m=m), 10), O.strong_wolfe(1e-5, 0.1), log_cap=10000)
        bar, cells, outs, errs = threading.Barrier(W), [None] * W, [None] * W, []

        def make_allgather(rank):
            def ag(send):
                cells[rank] = send.copy()
                bar.wait()
                out = np.concatenate(cells)
                bar.wait()
                return out
            return ag

        def worker(rank):
            try:
                ctx = cgo.Context(0)
                ctx.set_comm_callback(rank, W, make_allgather(rank))
                ctx.shard_fn = shard
                obj = cgo.ElementwiseObjective(n, BODY[3], param=[None, slots[1], None], ctx=ctx)
                obj.fill_param("uniform", 3, 0.5, 4.0, slot=0)
                loc, dev = obj.local(slots[2]), C.c_void_p()
                assert hip.hipMalloc(C.byref(dev), loc.nbytes) == 0 and hip.hipMemcpy(dev, loc.ctypes.data, loc.nbytes, 1) == 0   # 1: host to device
                obj.set_param_device(int(dev.value), slot=2)
                assert hip.hipFree(dev) == 0
                outs[rank] = _solve(cgo, obj, x0, cfg, ls)
                obj.close(); ctx.close()
            except Exception as e:  # pragma: no cover
                errs.append(e)
                bar.abort()
        ts = [threading.Thread(target=worker, args=(r,)) for r in range(W)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        assert not errs, errs
        for o in outs[1:]:
            assert o.objective == outs[0].objective and np.array_equal(o.log_phi, outs[0].log_phi)
        assert first_divergence(outs[0], ref) is None and outs[0].status == ref.status and outs[0].iters_ran == ref.iters_ran
        x = np.concatenate([o.minimizer for o in outs])
        assert rel(x, ref.minimizer) <= TOL and relf(outs[0].objective, ref.objective) <= TOL, name


# ---- ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_abi_behaviour(cgo, gpu_ctx, modules):
    """(6)"""
    import ctypes as C
    from cgo_amd import _lib
    L = _lib.lib()
    n = 1001
    slots, x0, _ = problem(n)
    ctx = cgo.default_context()

    def create(source, k, ex=True):
        h = C.c_void_p()
        fn = L.cgo_objective_create_from_source_ex if ex else L.cgo_objective_create_from_source
        return fn(ctx._h, source.encode(), k, n, 0, n, C.byref(h)), h

    def num(h):
        k = C.c_int32(-1)
        assert L.cgo_objective_num_params(h, C.byref(k)) == 0
        return k.value

    rc, h = create(BODY[3], 3)
    assert rc == 0 and num(h) == 3
    v = np.ascontiguousarray(slots[0])
    assert L.cgo_objective_set_param_host(h, 2, v.ctypes.data_as(_lib.dp)) == 0
    for bad in (3, 4, -1):
        assert L.cgo_objective_set_param_host(h, bad, v.ctypes.data_as(_lib.dp)) == 1           # CGO_EINVAL
        assert L.cgo_objective_fill_param(h, bad, 1, 3, 0.5, 4.0) == 1
        assert L.cgo_objective_set_param_device(h, bad, C.c_void_p(8)) == 1
    L.cgo_objective_destroy(h)
    rc, h = create(BODY[3], 5)
    assert rc == 1 and not h.value and "n_params" in L.cgo_last_error().decode()
    rc, h = create("gi = p*x; fi = 0.5*(gi*x);", 1, ex=False)                                   # the old entry: has_param = 1
    assert rc == 0 and num(h) == 1
    L.cgo_objective_destroy(h)
    rc, h = create("gi = x; fi = 0.5*(x*x);", 0, ex=False)
    assert rc == 0 and num(h) == 0
    L.cgo_objective_destroy(h)
    q = cgo.QuadDiag(np.ones(8))
    assert q.n_params == 1
    q.close()
    for k in (2, 4, 1, 0):                                                                      # kParams = 3 against another n_params
        rc, h = create(STRUCT3, k)
        assert rc == 1 and not h.value, k
        msg = L.cgo_last_error().decode()
        assert "kParams" in msg and "n_params" in msg, msg
    # slot 2 never set: the solve does not start, and the message names the slot
    obj = cgo.ElementwiseObjective(n, BODY[3], param=[slots[0], slots[1], None])
    cfg = cgo.setupCGConfig(1e-9, cgo.PolakRibiere(), cgo.EnableTrace(), max_iters=5)
    for pol in (None, cgo.SolverPolicy(stored_gradient=True), cgo.SolverPolicy(resident=False)):
        s = cgo.Solver(obj, cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), pol)
        s.set_x0(x0)
        with pytest.raises(cgo.CgoError) as e:
            s.start()
        assert e.value.code == 5 and "slot 2" in str(e.value), str(e.value)                     # CGO_ESTATE
        s.close()
    obj.set_param(slots[2], slot=2)
    # the profile's algorithmic bytes: (32 + 8·3) B per element for accept + direction + trial
    search = cgo.SolverPolicy(resident=False, controller_depth=0, placement_search=True, hbm_stream_bytes=1.0)   # every launch pure-HBM: the search runs at any n
    one = cgo.ElementwiseObjective(n, "gi = p*x; fi = 0.5*(gi*x);", param=slots[0])
    s = cgo.Solver(one, cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), search)
    assert s.placement_info()[2] > 0                                                            # one slot: (x, u, D) triples are timed
    s.close(); one.close()
    s = cgo.Solver(obj, cfg, cgo.setupStrongWolfeBisection(1e-5, 0.1), search)
    s.profile(True)
    s.set_x0(x0)
    s.start()
    while not s.iterate(1 << 40):
        pass
    prof = s.profile_get()
    assert prof["accept_dir_trial"]["launches"] > 0 and prof["accept_dir_trial"]["bytes_per_launch"] == (32 + 8 * 3) * n
    assert "trial" not in prof or prof["trial"]["bytes_per_launch"] == (16 + 8 * 3) * n
    assert s.placement_info()[2] == 0                                                           # no search over more than three streams
    s.close()
    obj.close()
