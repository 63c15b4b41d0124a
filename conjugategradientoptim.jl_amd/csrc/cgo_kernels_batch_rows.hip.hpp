// cgo_kernels_batch_rows.hip.hpp — k_batch_rows: the batched solve's SECOND tier, for problems one workgroup's LDS does not hold.
//
// k_batch (cgo_kernels_batch.hip.hpp) keeps a problem's rows of x, u and the parameter slots in LDS, so a batch ends at
// cgo_batch_max_n (n ≤ 10 056 … 3 352 for 0 … 4 slots).  Nothing in the device loop depends on LDS: res_iterate is a template
// over a vector-operations object, and here that object (RowsDev) streams the rows from where they already are — the
// [batch][ld] rows of the concatenated backend — in every pass:
//
//   * still one workgroup per problem, the same BatchParams, states, records, hand-back and result assembly;
//   * no dynamic LDS, no load at entry, no write-back at exit: the accept pass stores x and u straight to their rows, the
//     R_INIT pass stores u = −g.  So — the opposite of what k_batch's header says of LDS — a problem handed back before it
//     completes an iteration HAS had its u row written (by R_INIT); the host solver starts such a problem itself (st.it == 0,
//     batch_export_row without u) and does not read that row;
//   * the lane → element assignment is ResDev's: lane tid owns pairs tid, tid + BLOCK, …, lane 0 the odd tail.  A lane only
//     ever re-reads what it wrote itself, in place, with plain global accesses (ldg2<false> / stg2<false>): a wave's own
//     read-after-write on one address is ordered, and there is no cross-lane hazard, no fence, no barrier for data;
//   * the pass bodies are cg_pair / cg_single, every lane accumulates its pairs in ascending index order into ONE
//     accumulator set, the workgroup reduction is wg_reduce_n and the row IS the total (the G == 1 branch of ResDev's
//     exchange): every sum, and with it every number of the solve, has the bits of the LDS tier.
//
// The streaming loop is this tier's hot path.  One workgroup of BLOCK lanes at one wave per SIMD is all a CU holds of a
// 512-VGPR kernel, so the bytes a CU keeps in flight are decided by the pairs per lane and trip alone: BATCH_ROWS_U of them,
// every 16-byte load of a trip issued before the arithmetic of its first pair.  Whole trips carry no guard; the last,
// partial trip loads from a clamped (in-row) index and guards arithmetic and stores per lane — trip counts are uniform
// (k_batch's note on the parked row offset applies here too).  U was chosen by measurement.
//
// No atomics, no polling, no read of another problem's rows; every loop is bounded by n or by the line search's own limits.
#pragma once

#include "cgo_kernels_batch.hip.hpp"

#ifndef CGO_BATCH_ROWS_U
#define CGO_BATCH_ROWS_U 4   // A/B builds: make EXTRA=-DCGO_BATCH_ROWS_U=… (ahead-of-time kernels only)
#endif

namespace cgo {
namespace dev {

constexpr int BATCH_ROWS_U = CGO_BATCH_ROWS_U;   // independent pairs per lane and trip
static_assert(BATCH_ROWS_U >= 1 && BATCH_ROWS_U <= 8, "pairs per lane and trip");
// A pass indexes the pairs of a row with an int, and its trip counter runs one trip past the last pair:
// npairs + U·BLOCK ≤ INT_MAX.  THE limit of this tier on n (cgo_batch_max_n_ex); memory is the other.
constexpr long long BATCH_ROWS_MAX_N = 2LL * (0x7FFFFFFFLL - (long long)BATCH_ROWS_U * BLOCK);

// What ResDev offers res_iterate in its SOLO form, over rows that stay in device memory.
template <class Obj, int NPTS>
struct RowsDev {
    double *xr, *ur;           // this problem's rows of x and u (device memory)
    ParamPtrs pl;              // … and of the parameter slots the objective reads (null beyond them)
    int npairs; bool odd;      // pairs of the row; has it an odd tail element (index 2·npairs)?
    double s0;
    double *tot;               // LDS [RES_WMAX]

    static constexpr int kNpts = NPTS;
    __device__ __forceinline__ bool leader() const { return threadIdx.x == 0; }
    __device__ __forceinline__ long long clock() const { return 0; }

    // U pairs of a trip: pairs i0 + j·BLOCK + tid, j < U.  All loads first, then the bodies in ascending pair order.
    template <int MODE, int NP, bool TAIL>
    __device__ __forceinline__ void trip(const RParams &rp, int i0, double (&acc)[RW<NP>::W]) {
        constexpr int U = BATCH_ROWS_U;
        constexpr bool rd_u = r_reads_u(MODE);
        d2 xv[U], uv[U];
        PV<Obj> pv[U];
        int idx[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            idx[j] = i0 + j * BLOCK + (int)threadIdx.x;
            const int il = (TAIL && idx[j] >= npairs) ? npairs - 1 : idx[j];   // (a lane past the end loads the row's last pair and drops it)
            xv[j] = ldg2<false>(xr, il);
            uv[j] = rd_u ? ldg2<false>(ur, il) : d2{0.0, 0.0};
            pv[j] = pv_load<Obj, false>(pl, il);
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
            if (!TAIL || idx[j] < npairs) {
                bool wx = false, wu = false;
                d2 g;
                cg_pair<Obj, MODE, NP>(rp, xv[j], uv[j], pv[j], acc, wx, wu, g);
                if (wx) stg2<false>(xr, idx[j], xv[j]);
                if (wu) stg2<false>(ur, idx[j], uv[j]);
            }
        }
    }

    // one pass over the row: the fused body of mode MODE with NP trial points, the workgroup's row of sums = the totals
    template <int MODE, int NP>
    __device__ __forceinline__ int pass(double a_acc, double beta, const double *a, int k, double (&sums)[RW<NP>::W]) {
        constexpr int W = RW<NP>::W;
        constexpr int U = BATCH_ROWS_U;
        const int tid = threadIdx.x;
        RParams rp;
        rp.a_acc = a_acc; rp.beta = beta; rp.s0 = s0; rp.n = 0;
#pragma unroll
        for (int j = 0; j < MAXP; ++j) rp.a[j] = (j < NP && k > 0) ? a[j] : 0.0;   // the caller pads a[] to NP entries
        double acc[W];
#pragma unroll
        for (int s = 0; s < W; ++s) acc[s] = 0.0;
        int i0 = 0;
        for (; i0 + U * BLOCK <= npairs; i0 += U * BLOCK) trip<MODE, NP, false>(rp, i0, acc);   // (uniform: npairs is the workgroup's)
        if (i0 < npairs) trip<MODE, NP, true>(rp, i0, acc);
        if (odd && tid == 0) {   // the odd tail element (objectives that are not pair-only)
            rp.x = xr; rp.u = ur; rp.p0 = pl.p0; rp.p1 = pl.p1; rp.p2 = pl.p2; rp.p3 = pl.p3; rp.xo = xr; rp.uo = ur; rp.gout = nullptr; rp.x2 = nullptr;
            cg_single<Obj, MODE, NP>(rp, 2LL * npairs, acc);
        }
        const double own = wg_reduce_n<W>(acc);
        if (tid < W) tot[tid] = own;   // (the G == 1 branch of ResDev::exchange)
        __syncthreads();
#pragma unroll
        for (int s = 0; s < W; ++s) sums[s] = tot[s];
        __syncthreads();   // tot is written again by the next pass
        return 0;
    }

    static __device__ TrialSums ts(const double *q) { return TrialSums{q[0], q[1], q[2], q[3], q[4], q[5], q[6]}; }

    // is ∇f(x + a·u) the zero vector, element by element? (ResDev::trial_gradient_is_zero: the same bodies, nothing written;
    // the rare path, one pair per lane and trip)
    static constexpr bool kZeroCheck = true;
    __device__ __forceinline__ bool trial_gradient_is_zero(double a) {
        const int tid = threadIdx.x;
        RParams rp;
        rp.a_acc = 0.0; rp.beta = 0.0; rp.s0 = s0; rp.n = 0;
#pragma unroll
        for (int j = 0; j < MAXP; ++j) rp.a[j] = (j == 0) ? a : 0.0;
        int nz = 0;
        for (int i0 = 0; i0 < npairs; i0 += BLOCK) {
            const int i = i0 + tid;
            if (i < npairs) {
                d2 xa = ldg2<false>(xr, i), ua = ldg2<false>(ur, i);
                const PV<Obj> pa = pv_load<Obj, false>(pl, i);
                double acc[RW<1>::W] = {};
                bool wx = false, wu = false;
                d2 g = d2{0.0, 0.0};
                cg_pair<Obj, R_GRADT, 1>(rp, xa, ua, pa, acc, wx, wu, g);
                nz |= (g.x != 0.0) | (g.y != 0.0);   // (a NaN counts as nonzero)
            }
        }
        if (odd && tid == 0) {   // the odd tail element, as cg_single's R_GRADT line forms it
            const long long i = 2LL * npairs;
            const PS<Obj> p = ps_load<Obj>(pl, i);
            double fd = 0.0, gg = 0.0;
            obj_eval1<Obj>(xr[i] + a * ur[i], p, s0, fd, gg);
            nz |= (gg != 0.0);
        }
        return __syncthreads_or(nz) == 0;
    }

    // is the stored direction the zero vector? (after R_INIT: u = −g.)  Every lane looks at the pairs it wrote itself.
    __device__ __forceinline__ bool direction_is_zero() {
        const int tid = threadIdx.x;
        int nz = 0;
        for (int i0 = 0; i0 < npairs; i0 += BLOCK) {
            const int i = i0 + tid;
            if (i < npairs) {
                const d2 ua = ldg2<false>(ur, i);
                nz |= (ua.x != 0.0) | (ua.y != 0.0);
            }
        }
        if (odd && tid == 0) nz |= (ur[2LL * npairs] != 0.0);
        return __syncthreads_or(nz) == 0;
    }

    __device__ __forceinline__ int trial(const double *a, int k, TrialSums *out) {
        constexpr int NT = NPTS < 3 ? NPTS : 3;
        double sums[RW<NT>::W];
        if (int rc = pass<R_TRIAL, NT>(0.0, 0.0, a, k, sums)) return rc;
#pragma unroll
        for (int j = 0; j < NT; ++j) out[j] = ts(sums + RS_PER_POINT * j);   // (all NT: a padded point repeats a real one)
        return 0;
    }
    __device__ __forceinline__ int accept_dir_trial(double a_acc, double beta, const double *a, int k, TrialSums *out, double &gu, double &uu) {
        if (k == 0) {
            double sums[RW<1>::W];
            if (int rc = pass<R_ACCEPT | R_DIR, 1>(a_acc, beta, a, 0, sums)) return rc;
            gu = sums[RW<1>::GU]; uu = sums[RW<1>::UU];
            return 0;
        }
        double sums[RW<NPTS>::W];
        if (int rc = pass<R_ACCEPT | R_DIR | R_TRIAL, NPTS>(a_acc, beta, a, k, sums)) return rc;
#pragma unroll
        for (int j = 0; j < NPTS; ++j) out[j] = ts(sums + RS_PER_POINT * j);
        gu = sums[RW<NPTS>::GU]; uu = sums[RW<NPTS>::UU];
        return 0;
    }
};

// PROBE: k_batch's note (cgo_batch_probe; the script in place of res_iterate, nothing else differs).
template <class Obj, int NPTS, bool PROBE = false>
__global__ __launch_bounds__(BLOCK, 1) void k_batch_rows(const typename BatchArg<PROBE>::type B) {
    __shared__ double tot[RES_WMAX];
    __shared__ ResState s_out;
    const int tid = threadIdx.x;
    const long long b = blockIdx.x, lo = b * B.ld;
    ResState s = B.st[b];
    if (s.reason == RES_STOP || s.reason == RES_HOST) return;   // finished, on the device or for the host (the whole workgroup alike)
    constexpr int K = obj_nparams<Obj>();
    RowsDev<Obj, NPTS> v{B.x + lo, B.u + lo,
                         ParamPtrs{K > 0 ? B.p0 + lo : nullptr, K > 1 ? B.p1 + lo : nullptr, K > 2 ? B.p2 + lo : nullptr, K > 3 ? B.p3 + lo : nullptr},
                         (int)(B.n >> 1), (B.n & 1) != 0, B.s0v ? B.s0v[b] : B.s0, tot};
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
    if (s.reason == RES_FRESH) {   // optim.jl:25-47: f_x = fdf!(df_x, x); u = −df_x (stored to the u row)
        double sums[RW<1>::W];
        v.template pass<R_INIT, 1>(0.0, 0.0, nullptr, 0, sums);
        s.f_x = sums[RS_F]; s.gg = sums[RS_GTGT];
        s.dphi0 = -s.gg; s.uu = s.gg; s.dir_neg = 1;
        s.it = 0; s.ncache = 0;
        s.done = 0; s.log_len = 0; s.evals = 0; s.passes = 1;
        if (v.leader()) B.f_x0[b] = s.f_x;
        // LinearAlgebra.norm, as k_batch has it: 0 only when g IS the zero vector (u = −g lies in the row: every element ±0)
        bool zero = false;
        if (s.gg == 0.0) zero = v.direction_is_zero();   // (uniform: the sums are the workgroup's)
        if (sumsq_in_range(s.gg)) s.norm = __builtin_sqrt(s.gg);
        else if (s.gg == 0.0 && zero) s.norm = 0.0;
        else { s.reason = RES_HOST; go = false; }
    }
    if (go) {
        ResRecord *recs = B.recs + b * B.rec_stride + (B.rec_abs ? s.it : 0);
        if constexpr (PROBE) batch_probe_script(B.pr, s, v, tot);
        else res_iterate(cfg, s, v, (int64_t)B.budget, recs, nullptr, 0);
    }
    s.t_total = 0; s.t_compute = 0; s.t_reduce = 0; s.t_exchange = 0; s.t_cycles = 0;
    constexpr int WS = sizeof(ResState) / 8;
    static_assert(sizeof(ResState) % 8 == 0 && WS <= BLOCK, "the state goes out as 8-byte words, one lane each");
    if (tid == 0) s_out = s;
    __syncthreads();
    if (tid < WS) reinterpret_cast<unsigned long long *>(B.st + b)[tid] = reinterpret_cast<const unsigned long long *>(&s_out)[tid];
}

}  // namespace dev
}  // namespace cgo
