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
//     of a trial gradient and leader() are ResDev's own.  push_update and combine_trial are added here with the contracts of
//     LbfgsDev, on the LDS rows; the scalar recursion (qn_update, qn_coefficients) runs in lane 0 between two barriers; the loop
//     is res_iterate_qn, untouched;
//   * at exit, if an iteration completed (s.done > 0): x, u and every ring slot a push of THIS launch wrote go back to their
//     device rows — a slot that was only loaded is what device memory already holds.  A problem handed back before it completes an
//     iteration leaves its device rows untouched (k_batch's rule, not k_batch_rows's).  The QnState and ResState go out as in
//     k_batch_lbfgs.  The device ring stays allocated: a launch that ends on its slice budget and the launch that resumes it
//     produce together what one launch produces.
//
// EVERY NUMBER HAS THE BITS OF THE DEVICE TIER.  Lane tid owns pairs tid, tid + BLOCK, … of every row, ring rows included, lane 0
// the odd tail; each lane adds its pairs in ascending index order into ONE accumulator set (QN_SUMS slots for the push, RW<NP>
// for the combine); the per-pair expressions are those of LbfgsDev::push_trip / combine_trip — obj_eval2, s = a·u, xp = x + s,
// y = g⁺ − g; u = −γ·g, then the cy terms j = 0 …, then the cs terms; cg_pair<Obj, R_TRIAL, NP> — the reduction is wg_reduce_n
// and the workgroup's row is the total.  Pairs per lane and trip: batch_lbfgs_lds_u<Obj>() (CGO_BATCH_LBFGS_LDS_U for K ≤ 1,
// CGO_BATCH_LBFGS_LDS_U_SLOTS for K ≥ 2).  The choice cannot change a bit of any result: a lane owns pairs tid, tid + BLOCK, …
// whatever U is, and within a trip it adds t = 0 … U−1 in ascending order into the same accumulators, so every per-lane sum is
// formed over the same pairs in the same order for every U; the reduction over lanes does not know U.
//
// LDS access: pairs as 16-byte accesses (ds_read_b128 / ds_write_b128), consecutive lanes on consecutive pairs — no bank
// conflict.  A lane only re-reads what it wrote itself: no barrier for data beyond those the reductions and the recursion have.
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

template <class Obj, int NPTS>
struct LbfgsLdsDev : ResDev<Obj, NPTS, false, true> {
    using R = ResDev<Obj, NPTS, false, true>;
    double *Sr, *Yr;           // this problem's ring (LDS), slot p at p·ld
    int ld;
    QnState *q;                // LDS
    QnCoef *co;                // LDS
    double *qsum;              // LDS [QN_SUMS]
    unsigned dirty = 0u;       // bit p: ring slot p was written by a push of this launch (the whole workgroup's alike)

    __device__ __forceinline__ LbfgsLdsDev(const R &r, double *S, double *Y, int ld_, QnState *q_, QnCoef *co_, double *qs)
        : R(r), Sr(S), Yr(Y), ld(ld_), q(q_), co(co_), qsum(qs) {}

    __device__ __forceinline__ ParamPtrs slots() const {   // (addresses only: slots ≥ K are never read)
        return ParamPtrs{this->ps, this->ps + this->P.chunk, this->ps + 2 * this->P.chunk, this->ps + 3 * this->P.chunk};
    }

    // ---- push -----------------------------------------------------------------------------------------------------------
    template <bool TAIL>
    __device__ __forceinline__ void push_trip(double a, int c, int i0, double (&acc)[QN_SUMS]) {
        constexpr int U = batch_lbfgs_lds_u<Obj>();
        const ParamPtrs pl = slots();
        d2 xv[U], uv[U], sv[QN_MAX_M][U], yv[QN_MAX_M][U];
        PV<Obj> pv[U];
        int idx[U], il[U];
#pragma unroll
        for (int t = 0; t < U; ++t) {
            idx[t] = i0 + t * BLOCK + (int)threadIdx.x;
            il[t] = (TAIL && idx[t] >= this->npairs) ? this->npairs - 1 : idx[t];   // (a lane past the end reads the row's last pair and drops it)
            xv[t] = ldg2<false>(this->xs, il[t]);
            uv[t] = ldg2<false>(this->us, il[t]);
            pv[t] = pv_load<Obj, false>(pl, il[t]);
        }
#pragma unroll
        for (int j = 0; j < QN_MAX_M; ++j) {
            if (j < c) {   // (wave-uniform: c is the workgroup's)
                const int off = q->list[j] * ld;
#pragma unroll
                for (int t = 0; t < U; ++t) { sv[j][t] = ldg2<false>(Sr + off, il[t]); yv[j][t] = ldg2<false>(Yr + off, il[t]); }
            }
        }
        const int offn = q->free_slot * ld;
#pragma unroll
        for (int t = 0; t < U; ++t) {
            if (!TAIL || idx[t] < this->npairs) {
                d2 g, gp, xp, s, y;
                double f0 = 0.0, f1 = 0.0;
                obj_eval2<Obj>(xv[t], pv[t], this->P.s0, f0, g);
                s.x = a * uv[t].x; s.y = a * uv[t].y;
                xp.x = xv[t].x + s.x; xp.y = xv[t].y + s.y;
                obj_eval2<Obj>(xp, pv[t], this->P.s0, f1, gp);
                y.x = gp.x - g.x; y.y = gp.y - g.y;
                stg2<false>(this->xs, idx[t], xp);
                stg2<false>(Sr + offn, idx[t], s);
                stg2<false>(Yr + offn, idx[t], y);
                acc[QS_SY] = dsum(acc[QS_SY], s.x, y.x); acc[QS_SY] = dsum(acc[QS_SY], s.y, y.y);
                acc[QS_YY] = dsum(acc[QS_YY], y.x, y.x); acc[QS_YY] = dsum(acc[QS_YY], y.y, y.y);
                acc[QS_SGN] = dsum(acc[QS_SGN], s.x, gp.x); acc[QS_SGN] = dsum(acc[QS_SGN], s.y, gp.y);
                acc[QS_YGN] = dsum(acc[QS_YGN], y.x, gp.x); acc[QS_YGN] = dsum(acc[QS_YGN], y.y, gp.y);
#pragma unroll
                for (int j = 0; j < QN_MAX_M; ++j) {
                    if (j < c) {
                        constexpr int P0 = QS_PAIR0;
                        const int b = P0 + QP_PER_PAIR * j;   // (a compile-time constant after unrolling)
                        const d2 sj = sv[j][t], yj = yv[j][t];
                        acc[b + QP_SJG] = dsum(acc[b + QP_SJG], sj.x, gp.x); acc[b + QP_SJG] = dsum(acc[b + QP_SJG], sj.y, gp.y);
                        acc[b + QP_YJG] = dsum(acc[b + QP_YJG], yj.x, gp.x); acc[b + QP_YJG] = dsum(acc[b + QP_YJG], yj.y, gp.y);
                        acc[b + QP_SJYN] = dsum(acc[b + QP_SJYN], sj.x, y.x); acc[b + QP_SJYN] = dsum(acc[b + QP_SJYN], sj.y, y.y);
                        acc[b + QP_YJSN] = dsum(acc[b + QP_YJSN], yj.x, s.x); acc[b + QP_YJSN] = dsum(acc[b + QP_YJSN], yj.y, s.y);
                        acc[b + QP_YJYN] = dsum(acc[b + QP_YJYN], yj.x, y.x); acc[b + QP_YJYN] = dsum(acc[b + QP_YJYN], yj.y, y.y);
                    }
                }
            }
        }
    }

    // the push pass, then the scalar recursion: returns the number of stored pairs (the whole workgroup's alike)
    __device__ __forceinline__ int push_update(double a) {
        constexpr int U = batch_lbfgs_lds_u<Obj>();
        const int tid = threadIdx.x;
        const int c = q->count, npairs = this->npairs;
        dirty |= 1u << q->free_slot;
        double acc[QN_SUMS];
#pragma unroll
        for (int s = 0; s < QN_SUMS; ++s) acc[s] = 0.0;
        int i0 = 0;
        for (; i0 + U * BLOCK <= npairs; i0 += U * BLOCK) push_trip<false>(a, c, i0, acc);   // (uniform: npairs is the workgroup's)
        if (i0 < npairs) push_trip<true>(a, c, i0, acc);
        if (this->odd && tid == 0) {   // the odd tail element (objectives that are not pair-only)
            const int i = 2 * npairs;
            const ParamPtrs pl = slots();
            const PS<Obj> p = ps_load<Obj>(pl, i);
            double f0 = 0.0, f1 = 0.0, g = 0.0, gp = 0.0;
            const double x = this->xs[i];
            obj_eval1<Obj>(x, p, this->P.s0, f0, g);
            const double s = a * this->us[i], xp = x + s;
            obj_eval1<Obj>(xp, p, this->P.s0, f1, gp);
            const double y = gp - g;
            const int offn = q->free_slot * ld;
            acc[QS_SY] = dsum(acc[QS_SY], s, y); acc[QS_YY] = dsum(acc[QS_YY], y, y);
            acc[QS_SGN] = dsum(acc[QS_SGN], s, gp); acc[QS_YGN] = dsum(acc[QS_YGN], y, gp);
#pragma unroll
            for (int j = 0; j < QN_MAX_M; ++j) {
                if (j < c) {
                    const int b = QS_PAIR0 + QP_PER_PAIR * j;
                    const int off = q->list[j] * ld;
                    const double sj = Sr[off + i], yj = Yr[off + i];
                    acc[b + QP_SJG] = dsum(acc[b + QP_SJG], sj, gp); acc[b + QP_YJG] = dsum(acc[b + QP_YJG], yj, gp);
                    acc[b + QP_SJYN] = dsum(acc[b + QP_SJYN], sj, y); acc[b + QP_YJSN] = dsum(acc[b + QP_YJSN], yj, s);
                    acc[b + QP_YJYN] = dsum(acc[b + QP_YJYN], yj, y);
                }
            }
            this->xs[i] = xp; Sr[offn + i] = s; Yr[offn + i] = y;
        }
        const double own = wg_reduce_n<QN_SUMS>(acc);
        if (tid < QN_SUMS) qsum[tid] = own;   // the workgroup's row is the total
        __syncthreads();
        if (tid == 0) {   // the scalar recursion, once; every lane then reads the same coefficients
            qn_update(*q, qsum);
            qn_coefficients(*q, *co);
        }
        __syncthreads();
        return co->count;
    }

    // ---- combine + the first trial points --------------------------------------------------------------------------------
    template <int NP, bool TAIL>
    __device__ __forceinline__ void combine_trip(const RParams &rp, int c, double ng, const double (&cy)[QN_MAX_M], const double (&cs)[QN_MAX_M],
                                                 int i0, double (&acc)[RW<NP>::W]) {
        constexpr int U = batch_lbfgs_lds_u<Obj>();
        const ParamPtrs pl = slots();
        d2 xv[U], sv[QN_MAX_M][U], yv[QN_MAX_M][U];
        PV<Obj> pv[U];
        int idx[U], il[U];
#pragma unroll
        for (int t = 0; t < U; ++t) {
            idx[t] = i0 + t * BLOCK + (int)threadIdx.x;
            il[t] = (TAIL && idx[t] >= this->npairs) ? this->npairs - 1 : idx[t];
            xv[t] = ldg2<false>(this->xs, il[t]);
            pv[t] = pv_load<Obj, false>(pl, il[t]);
        }
#pragma unroll
        for (int j = 0; j < QN_MAX_M; ++j) {
            if (j < c) {
                const int off = q->list[j] * ld;
#pragma unroll
                for (int t = 0; t < U; ++t) { sv[j][t] = ldg2<false>(Sr + off, il[t]); yv[j][t] = ldg2<false>(Yr + off, il[t]); }
            }
        }
#pragma unroll
        for (int t = 0; t < U; ++t) {
            if (!TAIL || idx[t] < this->npairs) {
                d2 g, u;
                double f0 = 0.0;
                obj_eval2<Obj>(xv[t], pv[t], this->P.s0, f0, g);
                u.x = ng * g.x; u.y = ng * g.y;
#pragma unroll
                for (int j = 0; j < QN_MAX_M; ++j) {
                    if (j < c) { u.x = u.x + cy[j] * yv[j][t].x; u.y = u.y + cy[j] * yv[j][t].y; }
                }
#pragma unroll
                for (int j = 0; j < QN_MAX_M; ++j) {
                    if (j < c) { u.x = u.x + cs[j] * sv[j][t].x; u.y = u.y + cs[j] * sv[j][t].y; }
                }
                stg2<false>(this->us, idx[t], u);
                acc[RW<NP>::GU] = dsum(acc[RW<NP>::GU], g.x, u.x); acc[RW<NP>::GU] = dsum(acc[RW<NP>::GU], g.y, u.y);
                acc[RW<NP>::UU] = dsum(acc[RW<NP>::UU], u.x, u.x); acc[RW<NP>::UU] = dsum(acc[RW<NP>::UU], u.y, u.y);
                bool wx = false, wu = false;
                d2 gout;
                cg_pair<Obj, R_TRIAL, NP>(rp, xv[t], u, pv[t], acc, wx, wu, gout);   // the trial sums, as a trial pass forms them
            }
        }
    }

    __device__ __forceinline__ int combine_trial(const double *a, int k, TrialSums *out, double &gu, double &uu) {
        constexpr int NP = NPTS;
        constexpr int W = RW<NP>::W;
        constexpr int U = batch_lbfgs_lds_u<Obj>();
        const int tid = threadIdx.x;
        const int c = co->count, npairs = this->npairs;
        const double ng = -co->gamma;
        double cy[QN_MAX_M], cs[QN_MAX_M];
#pragma unroll
        for (int j = 0; j < QN_MAX_M; ++j) { cy[j] = co->cy[j]; cs[j] = co->cs[j]; }   // (compile-time indices: registers)
        RParams rp;
        rp.a_acc = 0.0; rp.beta = 0.0; rp.s0 = this->P.s0; rp.n = 0;
#pragma unroll
        for (int j = 0; j < MAXP; ++j) rp.a[j] = (j < NP && k > 0) ? a[j] : 0.0;   // the caller pads a[] to NP entries
        double acc[W];
#pragma unroll
        for (int s = 0; s < W; ++s) acc[s] = 0.0;
        int i0 = 0;
        for (; i0 + U * BLOCK <= npairs; i0 += U * BLOCK) combine_trip<NP, false>(rp, c, ng, cy, cs, i0, acc);
        if (i0 < npairs) combine_trip<NP, true>(rp, c, ng, cy, cs, i0, acc);
        if (this->odd && tid == 0) {
            const int i = 2 * npairs;
            const ParamPtrs pl = slots();
            const PS<Obj> p = ps_load<Obj>(pl, i);
            double f0 = 0.0, g = 0.0;
            obj_eval1<Obj>(this->xs[i], p, this->P.s0, f0, g);
            double u = ng * g;
#pragma unroll
            for (int j = 0; j < QN_MAX_M; ++j) { if (j < c) u = u + cy[j] * Yr[q->list[j] * ld + i]; }
#pragma unroll
            for (int j = 0; j < QN_MAX_M; ++j) { if (j < c) u = u + cs[j] * Sr[q->list[j] * ld + i]; }
            this->us[i] = u;
            acc[RW<NP>::GU] = dsum(acc[RW<NP>::GU], g, u);
            acc[RW<NP>::UU] = dsum(acc[RW<NP>::UU], u, u);
            rp.x = this->xs; rp.u = this->us; rp.p0 = pl.p0; rp.p1 = pl.p1; rp.p2 = pl.p2; rp.p3 = pl.p3;
            rp.xo = this->xs; rp.uo = this->us; rp.gout = nullptr; rp.x2 = nullptr;
            cg_single<Obj, R_TRIAL, NP>(rp, i, acc);   // (reads back the u this lane stored just above)
        }
        const double own = wg_reduce_n<W>(acc);
        if (tid < W) this->tot[tid] = own;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NP; ++j) out[j] = R::ts(this->tot + RS_PER_POINT * j);
        gu = this->tot[RW<NP>::GU]; uu = this->tot[RW<NP>::UU];
        __syncthreads();   // tot is written again by the next pass
        return 0;
    }
};

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
        const unsigned dirty = v.dirty;
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
