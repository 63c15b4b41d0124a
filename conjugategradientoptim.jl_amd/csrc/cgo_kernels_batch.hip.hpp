// cgo_kernels_batch.hip.hpp — k_batch: MANY small problems in one launch, a workgroup each, finished on the device.
//
// One small problem (BASELINE config 1: n = 1000) is latency-bound on the resident solver: one workgroup on one CU, the other
// 255 idle.  A user with n ≈ 1e3 has many of them — a parameter sweep, multi-start, one fit per pixel — and
// here blockIdx.x says WHICH PROBLEM, not which chunk:
//
//   * workgroup b loads row b of x, u and of every parameter slot the objective reads ([batch][ld] each, ld = n + (n & 1)) into
//     LDS — slot j at ps + j·ld, where ResDev looks for it — and its own ResState from st[b]; a problem that is already finished (RES_STOP, RES_HOST) costs its workgroup one load and a return;
//   * a problem that has not started (RES_FRESH) gets optim.jl:25-47 here: pass<R_INIT, 1> → u = −g, f_x, g·g;
//   * then res_iterate (cgo_resident.hpp) — the loop k_resident runs — over ResDev in its SOLO form: the passes, trial and
//     accept_dir_trial are ResDev's own (cgo_kernels_resident.hip.hpp), the workgroup's row is the total, its lane 0 the leader;
//   * when the slice ends: x, u back in place if an iteration completed, the state to st[b], the records of the completed
//     iterations (written by the leader as they completed) in recs[b].  (So a problem handed back before it completes an
//     iteration leaves its rows untouched.  The tier without LDS, k_batch_rows in cgo_kernels_batch_rows.hip.hpp, differs here:
//     its R_INIT pass has stored u = −g to the u row by then — a row the host solver does not read when st.it == 0.)
// The objective's scalar is the launch's (s0) or the problem's own (s0v[b]): a barrier weight, a regularisation strength, a
// temperature per problem.  With scalars per problem the results' gradient is k_batch_grad's (below), a workgroup per row too.
//
// Workgroups never wait for one another: no atomics, no polling, no read of another problem's rows.  More workgroups than CUs
// simply queue.  A launch is bounded by `budget` outer iterations per problem, each by the line search's own limits.
//
// PROBE (template flag, default false; cgo_batch_probe): the same kernel with a script of passes in place of res_iterate, every
// workgroup storing the row it holds after each pass — what tests/test_batch_kernel_sums.py compares.  Everything else — the
// early return, the LDS load, the vector-operations object, the write-back rule, the state store — is the code below.  The
// PROBE twins are instantiated in a translation unit of their own (cgo_backend_batch_probe.hip).
#pragma once

#include "cgo_kernels_resident.hip.hpp"

namespace cgo {
namespace dev {

struct BatchParams {
    double *x; double *u; const double *p0;   // [batch][ld]; the padding element of an odd n is never read by a pass
    ResState *st;                             // [batch]
    ResRecord *recs;                          // [batch][rec_stride]
    double *f_x0;                             // [batch]: f(x_initial), written with the initial evaluation (optim.jl:31)
    long long n, ld, rec_stride;
    int rec_abs;                              // 1: record of iteration it lives at [it − 1] (the trace); 0: at [its number in this slice]
    double s0;
    ResConfig cfg;
    long long budget;
    const double *p1, *p2, *p3;               // [batch][ld]: parameter slots 1–3 (run-time compiled objectives with kParams > 1 only)
    const double *s0v;                        // [batch]: every problem's own objective scalar; null: s0 is every problem's
};

// ---- cgo_batch_probe: the script of the PROBE twins of k_batch, k_batch_rows and k_batch_lbfgs ----------------------------------
constexpr int BATCH_PROBE_MAX_PASSES = 32;
constexpr int BATCH_PROBE_ROW = 64;       // stride of a stored row: the push row of k_batch_lbfgs (QN_SUMS), the widest there is
constexpr int BATCH_PROBE_MAX_M = 10;     // = QN_MAX_M (cgo_kernels_batch_lbfgs.hip.hpp asserts it)
static_assert(RES_WMAX <= BATCH_PROBE_ROW, "a stored row holds the widest row of totals");
// One pass: kind 0 trial(a, k) | 1 accept_dir_trial(a_acc, beta, a, k) | 2 pass<R_INIT, 1> | 3 push_update(a_acc) |
// 4 combine_trial(a, k) — with the coefficients the last push left, or (co_count ≥ 0) those given here.  a[] is padded by the
// host as the loops pad it (entries ≥ k repeat a[k − 1]).
struct BatchProbePass {
    int kind, k;
    double a[RES_MAXP];
    double a_acc, beta;
    int co_count, pad_;
    double co_gamma, co_cy[BATCH_PROBE_MAX_M], co_cs[BATCH_PROBE_MAX_M];
};
struct BatchProbeOut { TrialSums ts[RES_MAXP]; double gu, uu; long long width, stored; };
struct BatchProbe {
    const BatchProbePass *script; int npass;  // DEVICE [npass]
    double *rows;                             // DEVICE [npass][batch][BATCH_PROBE_ROW]: the row EVERY workgroup holds after each pass
    BatchProbeOut *out;                       // DEVICE [npass][batch]: what the member function returned in every problem
};
// (the PROBE twin's argument IS a BatchParams with the script behind it: the kernel text below reads B.… in both forms)
struct BatchProbeParams : BatchParams { BatchProbe pr; };
template <bool PROBE> struct BatchArg { using type = BatchParams; };
template <> struct BatchArg<true> { using type = BatchProbeParams; };

// after a member call: the workgroup's row (W slots of `row`, LDS) and, by lane 0, what the call returned
__device__ __forceinline__ void batch_probe_store(const BatchProbe &pr, int q, const double *row, int W, const TrialSums *out, double gu, double uu, int stored) {
    const size_t at = (size_t)q * gridDim.x + blockIdx.x;
    if ((int)threadIdx.x < W) pr.rows[at * BATCH_PROBE_ROW + threadIdx.x] = row[threadIdx.x];
    if (threadIdx.x == 0) {
        BatchProbeOut &o = pr.out[at];
        for (int j = 0; j < RES_MAXP; ++j) o.ts[j] = out[j];
        o.gu = gu; o.uu = uu; o.width = W; o.stored = stored;
    }
}

// The passes the CG loop (res_iterate) issues, through the member functions it calls.  An accepting pass counts as a completed
// iteration (s.done), so that k_batch's write-back runs as after a slice that completed one.  false: not one of them.
template <class V>
__device__ __forceinline__ bool batch_probe_cg_pass(const BatchProbe &pr, int q, const BatchProbePass &c, ResState &s, V &v, const double *tot) {
    constexpr int NPTS = V::kNpts, NT = NPTS < 3 ? NPTS : 3;
    TrialSums out[RES_MAXP] = {};
    double gu = 0.0, uu = 0.0;
    int rc = 0, W = 0;
    if (c.kind == 0) { rc = v.trial(c.a, c.k, out); W = RW<NT>::W; }
    else if (c.kind == 1) { rc = v.accept_dir_trial(c.a_acc, c.beta, c.a, c.k, out, gu, uu); W = c.k == 0 ? RW<1>::W : RW<NPTS>::W; if (!rc) s.done++; }
    else if (c.kind == 2) { double sums[RW<1>::W]; rc = v.template pass<R_INIT, 1>(0.0, 0.0, nullptr, 0, sums); W = RW<1>::W; }
    else return false;
    if (rc) { s.reason = RES_ERROR; return true; }
    s.passes++;
    batch_probe_store(pr, q, tot, W, out, gu, uu, 0);
    return true;
}
template <class V>
__device__ __forceinline__ void batch_probe_script(const BatchProbe &pr, ResState &s, V &v, const double *tot) {
    s.done = 0; s.log_len = 0; s.evals = 0; s.passes = 0; s.reason = RES_BUDGET;
    s.t_machine = 0; s.t_eval = 0; s.t_post = 0;
    for (int q = 0; q < pr.npass && s.reason == RES_BUDGET; ++q) {
        const BatchProbePass c = pr.script[q];
        if (!batch_probe_cg_pass(pr, q, c, s, v, tot)) s.reason = RES_ERROR;   // (the host refuses such a script)
    }
}

template <class Obj, int NPTS, bool PROBE = false>
__global__ __launch_bounds__(BLOCK, 1) void k_batch(const typename BatchArg<PROBE>::type B) {
    extern __shared__ __attribute__((aligned(16))) double res_lds[];
    __shared__ double tot[RES_WMAX];
    __shared__ double fs[BLOCK];
    __shared__ ResState s_out;
    const int tid = threadIdx.x;
    const long long b = blockIdx.x, lo = b * B.ld;
    ResState s = B.st[b];
    if (s.reason == RES_STOP || s.reason == RES_HOST) return;   // finished, on the device or for the host (the whole workgroup alike)
    double *xs = res_lds, *us = res_lds + B.ld, *ps = res_lds + 2 * B.ld;
    // (both row loops below have a UNIFORM trip count and a per-lane guard inside: a loop that lanes leave one by one ends with
    //  no lane active, and a per-lane value the register allocator parks right there — the row offset, kept for the write-back —
    //  is then never parked at all)
    for (long long i0 = 0; i0 < B.ld; i0 += BLOCK) {
        const long long i = i0 + tid;
        if (i < B.ld) {
            xs[i] = B.x[lo + i];
            us[i] = B.u[lo + i];
            constexpr int K = obj_nparams<Obj>();
            if constexpr (K > 0) ps[i] = B.p0[lo + i];
            if constexpr (K > 1) ps[B.ld + i] = B.p1[lo + i];
            if constexpr (K > 2) ps[2 * B.ld + i] = B.p2[lo + i];
            if constexpr (K > 3) ps[3 * B.ld + i] = B.p3[lo + i];
        }
    }
    __syncthreads();
    ResParams Q{};   // what ResDev reads of it in its SOLO form: the stride of the parameter slots, the objective's scalar, no clocks
    Q.n = B.n; Q.chunk = B.ld; Q.s0 = B.s0v ? B.s0v[b] : B.s0; Q.timing = 0;
    ResDev<Obj, NPTS, false, true> v{Q, xs, us, ps, (int)(B.n >> 1), (B.n & 1) != 0, 0ull, tot, fs, 0, 0, 0};
    ResConfig cfg = B.cfg;
    // (as k_resident: the loop state is FP64 arithmetic throughout — into VGPRs once, opaquely; see the note there)
#define RES_V(x) asm volatile("" : "+v"(x))
    RES_V(s.f_x); RES_V(s.gg); RES_V(s.norm); RES_V(s.dphi0); RES_V(s.uu); RES_V(s.a_initial); RES_V(s.last_a); RES_V(s.last_beta);
#pragma unroll
    for (int j = 0; j < RES_MAXP; ++j) {
        RES_V(s.ca[j]); RES_V(s.cs[j].f); RES_V(s.cs[j].gtu); RES_V(s.cs[j].gtgt); RES_V(s.cs[j].gtg); RES_V(s.cs[j].yy); RES_V(s.cs[j].uy); RES_V(s.cs[j].ygt);
    }
    RES_V(cfg.ls.c1); RES_V(cfg.ls.c2); RES_V(cfg.ls.a_max_growth_factor); RES_V(cfg.ls.delta1); RES_V(cfg.ls.max_step_size);
    RES_V(cfg.ls.discount_factor); RES_V(cfg.eps); RES_V(cfg.mu);
#undef RES_V
    bool go = true;
    if (s.reason == RES_FRESH) {   // optim.jl:25-47: f_x = fdf!(df_x, x); u = −df_x
        double sums[RW<1>::W];
        v.template pass<R_INIT, 1>(0.0, 0.0, nullptr, 0, sums);
        s.f_x = sums[RS_F]; s.gg = sums[RS_GTGT];
        s.dphi0 = -s.gg; s.uu = s.gg; s.dir_neg = 1;
        s.it = 0; s.ncache = 0;
        s.done = 0; s.log_len = 0; s.evals = 0; s.passes = 1;
        if (v.leader()) B.f_x0[b] = s.f_x;
        // LinearAlgebra.norm: sqrt(Σg²) in range; 0 when g IS the zero vector (u = −g lies in LDS: every element ±0 — a sum of
        // exactly 0 alone could be the underflow of tiny squares); everything else is the rare path, the host's from iteration 0
        int nz = 0;
        if (s.gg == 0.0) {
            for (long long i0 = 0; i0 < B.n; i0 += BLOCK) {
                const long long i = i0 + tid;
                if (i < B.n) nz |= (us[i] != 0.0);
            }
        }
        nz = __syncthreads_or(nz);
        if (sumsq_in_range(s.gg)) s.norm = __builtin_sqrt(s.gg);
        else if (s.gg == 0.0 && nz == 0) s.norm = 0.0;
        else { s.reason = RES_HOST; go = false; }
    }
    if (go) {
        ResRecord *recs = B.recs + b * B.rec_stride + (B.rec_abs ? s.it : 0);
        if constexpr (PROBE) batch_probe_script(B.pr, s, v, tot);
        else res_iterate(cfg, s, v, (int64_t)B.budget, recs, nullptr, 0);
    }
    s.t_total = 0; s.t_compute = 0; s.t_reduce = 0; s.t_exchange = 0; s.t_cycles = 0;
    __syncthreads();
    if (s.done > 0) {   // x, u of the last completed iteration (an iteration handed back never touched them)
        for (long long i0 = 0; i0 < B.n; i0 += BLOCK) {
            const long long i = i0 + tid;
            if (i < B.n) {
                B.x[lo + i] = xs[i];
                B.u[lo + i] = us[i];
            }
        }
    }
    constexpr int WS = sizeof(ResState) / 8;
    static_assert(sizeof(ResState) % 8 == 0 && WS <= BLOCK, "the state goes out as 8-byte words, one lane each");
    if (tid == 0) s_out = s;
    __syncthreads();
    if (tid < WS) reinterpret_cast<unsigned long long *>(B.st + b)[tid] = reinterpret_cast<const unsigned long long *>(&s_out)[tid];
}

// ∇f of every problem at its x, with the problem's own scalar: Results.gradient of a batched solve whose problems differ in
// s0 (without scalars per problem it is ONE ordinary R_GRAD launch over the concatenated rows, batch_results).  blockIdx.x = the
// problem; row b of x and of every slot the objective reads comes straight from HBM, row b of g goes back; the pair and odd-tail
// bodies are those of the R_GRAD launch (cg_pair, cg_single's line).  The padding element of an odd n is neither read nor written.
struct BatchGradParams {
    const double *x; double *g;               // [batch][ld]
    const double *p0, *p1, *p2, *p3;          // [batch][ld], the slots the objective reads
    const double *s0v;                        // [batch]
    long long n, ld;
};

template <class Obj>
__global__ __launch_bounds__(BLOCK) void k_batch_grad(const BatchGradParams G) {
    const int tid = threadIdx.x;
    const long long b = blockIdx.x, lo = b * G.ld;
    const double s0 = G.s0v[b];
    RParams rp;
    rp.a_acc = 0.0; rp.beta = 0.0; rp.s0 = s0; rp.n = 0; rp.nrep = 0;
#pragma unroll
    for (int j = 0; j < MAXP; ++j) rp.a[j] = 0.0;
    constexpr int K = obj_nparams<Obj>();
    const ParamPtrs pl{K > 0 ? G.p0 + lo : nullptr, K > 1 ? G.p1 + lo : nullptr, K > 2 ? G.p2 + lo : nullptr, K > 3 ? G.p3 + lo : nullptr};
    const double *xr = G.x + lo;
    double *gr = G.g + lo;
    const long long npairs = G.n >> 1;
    for (long long i0 = 0; i0 < npairs; i0 += BLOCK) {   // (uniform trip count, per-lane guard: k_batch's note)
        const long long i = i0 + tid;
        if (i < npairs) {
            d2 xa = ldg2<false>(xr, i), ua = d2{0.0, 0.0};
            const PV<Obj> pa = pv_load<Obj, false>(pl, i);
            double acc[RW<1>::W] = {};
            bool wx = false, wu = false;
            d2 g = d2{0.0, 0.0};
            cg_pair<Obj, R_GRAD, 1>(rp, xa, ua, pa, acc, wx, wu, g);
            stg2<false>(gr, i, g);
        }
    }
    if ((G.n & 1) && tid == 0) {   // the odd tail element, as cg_single's R_GRAD line forms it
        const long long i = G.n - 1;
        const PS<Obj> p = ps_load<Obj>(pl, i);
        double f0 = 0.0, g = 0.0;
        obj_eval1<Obj>(xr[i], p, s0, f0, g);
        gr[i] = g;
    }
}

}  // namespace dev
}  // namespace cgo
