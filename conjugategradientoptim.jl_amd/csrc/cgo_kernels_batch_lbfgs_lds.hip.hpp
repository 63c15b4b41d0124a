// cgo_kernels_batch_lbfgs_lds.hip.hpp — k_batch_lbfgs_lds: batched solves with β = LBFGS(m), one workgroup per problem, the rows
// AND the ring in LDS.
//
// k_batch_lbfgs (cgo_kernels_batch_lbfgs.hip.hpp) streams x, u, the parameter slots and the 2(m+1) ring rows of its problem from
// device memory in every pass; at n ≈ 1000 an iteration is bound by those dependent trips.  Here a problem's
// rows live in LDS for the whole launch, as k_batch (cgo_kernels_batch.hip.hpp) keeps x, u and the slots for the CG flavours:
//
//   * dynamic LDS, rows of ld doubles (ld even: every row 16-byte aligned): x | u | slot 0 … K−1 | S[0 … m] | Y[0 … m] —
//     2 + K + 2(m+1) rows (cgo_batch_lbfgs_lds_rows); the QnState, the coefficients and the two sum rows in static LDS;
//   * at entry: the problem's QnState → LDS, then x, u and the slots as k_batch loads them, then the ring slots that hold a
//     stored pair, q.list[0 … count) — a fresh problem loads none;
//   * the vector-operations object is k_batch's ResDev in its SOLO form over those rows: pass<R_INIT, 1>, trial, the zero check
//     of a trial gradient and leader() are ResDev's own.  push_update and combine_trial are the device tier's text: LbfgsRing
//     (cgo_kernels_batch_lbfgs.hip.hpp) over LbfgsLdsRows, which names the LDS rows as that template reads them, with int ring
//     offsets and a hook that notes the slot a push writes; the loop is res_iterate_qn, untouched;
//   * at exit, if an iteration completed (s.done > 0): x, u and every ring slot a push of THIS launch wrote go back to their
//     device rows — a slot that was only loaded is what device memory already holds.  A problem handed back before it completes an
//     iteration leaves its device rows untouched (k_batch's rule, not k_batch_rows's).  The QnState and ResState go out as in
//     k_batch_lbfgs.  The device ring stays allocated: a launch that ends on its slice budget and the launch that resumes it
//     produce together what one launch produces.
//
// EVERY NUMBER HAS THE BITS OF THE DEVICE TIER: the ring passes are one text for both tiers, and R_INIT and the trials are
// ResDev's, whose sums k_batch_rows reproduces bit for bit.  Pairs per lane and trip: batch_lbfgs_lds_u<Obj>()
// (CGO_BATCH_LBFGS_LDS_U for K ≤ 1, CGO_BATCH_LBFGS_LDS_U_SLOTS for K ≥ 2); every per-lane sum is formed over the same pairs
// in the same order for every U (the device tier's header says why).
//
// LDS access: pairs as 16-byte accesses (ds_read_b128 / ds_write_b128), consecutive lanes on consecutive pairs — no bank
// conflict.  No barrier for data beyond those the reductions and the recursion have (a lane only re-reads what it wrote itself).
// No atomics, no fences, no polling, no read of another problem's rows; every loop is bounded by n, m or the line search's limits.
#pragma once

#include "cgo_kernels_batch_lbfgs.hip.hpp"

#ifndef CGO_BATCH_LBFGS_LDS_U
#define CGO_BATCH_LBFGS_LDS_U 1   // A/B builds: make EXTRA=-DCGO_BATCH_LBFGS_LDS_U=…
#endif
#ifndef CGO_BATCH_LBFGS_LDS_U_SLOTS
#define CGO_BATCH_LBFGS_LDS_U_SLOTS 1   // objectives of two or more slots
#endif

namespace cgo {
namespace dev {

constexpr int BATCH_LBFGS_LDS_U = CGO_BATCH_LBFGS_LDS_U;   // independent pairs per lane and trip of the two ring passes over LDS
static_assert(BATCH_LBFGS_LDS_U >= 1 && BATCH_LBFGS_LDS_U <= 8, "pairs per lane and trip");
constexpr int BATCH_LBFGS_LDS_U_SLOTS = CGO_BATCH_LBFGS_LDS_U_SLOTS;
static_assert(BATCH_LBFGS_LDS_U_SLOTS >= 1 && BATCH_LBFGS_LDS_U_SLOTS <= BATCH_LBFGS_LDS_U, "an objective with slots takes no more pairs per trip than one without");
constexpr int batch_lbfgs_lds_u_of(int nparams) { return nparams >= 2 ? BATCH_LBFGS_LDS_U_SLOTS : BATCH_LBFGS_LDS_U; }
template <class Obj> constexpr int batch_lbfgs_lds_u() { return batch_lbfgs_lds_u_of(obj_nparams<Obj>()); }
constexpr int batch_lbfgs_lds_rows(int nparams, int m) { return 2 + nparams + 2 * (m + 1); }   // rows of ld doubles in dynamic LDS

// k_batch's ResDev in its SOLO form over the LDS rows, under the names LbfgsRing reads (cgo_kernels_batch_lbfgs.hip.hpp)
template <class Obj, int NPTS>
struct LbfgsLdsRows : ResDev<Obj, NPTS, false, true> {
    using R = ResDev<Obj, NPTS, false, true>;
    using Objective = Obj;
    __device__ __forceinline__ LbfgsLdsRows(const R &r) : R(r) {}
    __device__ __forceinline__ double *x_row() const { return this->xs; }
    __device__ __forceinline__ double *u_row() const { return this->us; }
    __device__ __forceinline__ ParamPtrs slot_ptrs() const {   // (addresses only: slots ≥ K are never read)
        return ParamPtrs{this->ps, this->ps + this->P.chunk, this->ps + 2 * this->P.chunk, this->ps + 3 * this->P.chunk};
    }
    __device__ __forceinline__ double scalar() const { return this->P.s0; }
};
// bit p: ring slot p was written by a push of this launch (the whole workgroup's alike)
struct RingPushDirty {
    unsigned dirty = 0u;
    __device__ __forceinline__ void operator()(int p) { dirty |= 1u << p; }
};

template <class Obj, int NPTS>
using LbfgsLdsDev = LbfgsRing<LbfgsLdsRows<Obj, NPTS>, int, batch_lbfgs_lds_u<Obj>(), RingPushDirty>;

// PROBE: k_batch's note (cgo_batch_probe, tier 3; the script of k_batch_lbfgs's twin in place of res_iterate_qn, nothing else differs).
template <class Obj, int NPTS, bool PROBE = false>
__global__ __launch_bounds__(BLOCK, 1) void k_batch_lbfgs_lds(const typename BatchLbfgsArg<PROBE>::type L) {
    extern __shared__ __attribute__((aligned(16))) double res_lds[];
    __shared__ double tot[RES_WMAX];
    __shared__ double qsum[QN_SUMS];
    __shared__ ResState s_out;
    __shared__ QnState s_q;
    __shared__ QnCoef s_co;
    const BatchParams &B = L.B;
    const int tid = threadIdx.x;
    const long long b = blockIdx.x, lo = b * B.ld;
    ResState s = B.st[b];
    if (s.reason == RES_STOP || s.reason == RES_HOST) return;   // finished, on the device or for the host (the whole workgroup alike)
    constexpr int QW = sizeof(QnState) / 8;
    for (int i = tid; i < QW; i += BLOCK)   // the problem's quasi-Newton state → LDS
        reinterpret_cast<unsigned long long *>(&s_q)[i] = reinterpret_cast<const unsigned long long *>(L.qn + b)[i];
    __syncthreads();
    constexpr int K = obj_nparams<Obj>();
    const int ld = (int)B.ld, slots_m = s_q.m + 1;
    double *xs = res_lds, *us = res_lds + ld, *ps = res_lds + 2 * ld;
    double *Ss = res_lds + (2 + K) * ld, *Ys = Ss + slots_m * ld;
    double *Sg = L.S + b * L.ring_stride, *Yg = L.Y + b * L.ring_stride;
    const int stored = s_q.count;
    // (uniform trip counts with a per-lane guard inside: k_batch's note)
    for (int i0 = 0; i0 < ld; i0 += BLOCK) {
        const int i = i0 + tid;
        if (i < ld) {
            xs[i] = B.x[lo + i];
            us[i] = B.u[lo + i];
            if constexpr (K > 0) ps[i] = B.p0[lo + i];
            if constexpr (K > 1) ps[ld + i] = B.p1[lo + i];
            if constexpr (K > 2) ps[2 * ld + i] = B.p2[lo + i];
            if constexpr (K > 3) ps[3 * ld + i] = B.p3[lo + i];
            for (int j = 0; j < stored; ++j) {   // the stored pairs only: a fresh problem loads none
                const int off = s_q.list[j] * ld + i;
                Ss[off] = Sg[off];
                Ys[off] = Yg[off];
            }
        }
    }
    __syncthreads();
    ResParams Q{};   // what ResDev reads of it in its SOLO form: the stride of the parameter slots, the objective's scalar, no clocks
    Q.n = B.n; Q.chunk = B.ld; Q.s0 = B.s0v ? B.s0v[b] : B.s0; Q.timing = 0;
    ResDev<Obj, NPTS, false, true> rows{Q, xs, us, ps, (int)(B.n >> 1), (B.n & 1) != 0, 0ull, tot, nullptr, 0, 0, 0};   // (fs: the exchange of more than one workgroup only)
    LbfgsLdsDev<Obj, NPTS> v(rows, Ss, Ys, ld, &s_q, &s_co, qsum);
    ResConfig cfg = B.cfg;
    CGO_BATCH_LBFGS_PIN(s, cfg);
    bool go = true;
    if (s.reason == RES_FRESH) {   // optim.jl:25-47: f_x = fdf!(df_x, x); u = −df_x
        double sums[RW<1>::W];
        v.template pass<R_INIT, 1>(0.0, 0.0, nullptr, 0, sums);
        s.f_x = sums[RS_F]; s.gg = sums[RS_GTGT];
        s.dphi0 = -s.gg; s.uu = s.gg; s.dir_neg = 1;
        s.it = 0; s.ncache = 0;
        s.done = 0; s.log_len = 0; s.evals = 0; s.passes = 1;
        if (v.leader()) B.f_x0[b] = s.f_x;
        // LinearAlgebra.norm, as k_batch has it: 0 only when g IS the zero vector (u = −g lies in LDS: every element ±0)
        int nz = 0;
        if (s.gg == 0.0) {
            for (int i0 = 0; i0 < (int)B.n; i0 += BLOCK) {
                const int i = i0 + tid;
                if (i < (int)B.n) nz |= (us[i] != 0.0);
            }
        }
        nz = __syncthreads_or(nz);
        if (sumsq_in_range(s.gg)) s.norm = __builtin_sqrt(s.gg);
        else if (s.gg == 0.0 && nz == 0) s.norm = 0.0;
        else { s.reason = RES_HOST; go = false; }
    }
    if (go) {
        ResRecord *recs = B.recs + b * B.rec_stride + (B.rec_abs ? s.it : 0);
        if constexpr (PROBE) batch_lbfgs_probe_script(L.pr, s, v);
        else res_iterate_qn(cfg, s, v, (int64_t)B.budget, recs);
    }
    s.t_total = 0; s.t_compute = 0; s.t_reduce = 0; s.t_exchange = 0; s.t_cycles = 0;
    __syncthreads();   // (also: lane 0's last recursion on s_q is complete)
    if (s.done > 0) {   // x, u of the last completed iteration and the ring slots this launch wrote (an iteration handed back never touched them)
        const int n = (int)B.n;
        const unsigned dirty = v.pushed.dirty;
        for (int i0 = 0; i0 < n; i0 += BLOCK) {
            const int i = i0 + tid;
            if (i < n) {
                B.x[lo + i] = xs[i];
                B.u[lo + i] = us[i];
                for (int p = 0; p < slots_m; ++p) {
                    if (dirty & (1u << p)) {   // (uniform)
                        const int off = p * ld + i;
                        Sg[off] = Ss[off];
                        Yg[off] = Ys[off];
                    }
                }
            }
        }
    }
    constexpr int WS = sizeof(ResState) / 8;
    static_assert(sizeof(ResState) % 8 == 0 && WS <= BLOCK, "the state goes out as 8-byte words, one lane each");
    if (tid == 0) s_out = s;
    __syncthreads();
    if (tid < WS) reinterpret_cast<unsigned long long *>(B.st + b)[tid] = reinterpret_cast<const unsigned long long *>(&s_out)[tid];
    for (int i = tid; i < QW; i += BLOCK)
        reinterpret_cast<unsigned long long *>(L.qn + b)[i] = reinterpret_cast<const unsigned long long *>(&s_q)[i];
}

}  // namespace dev
}  // namespace cgo
