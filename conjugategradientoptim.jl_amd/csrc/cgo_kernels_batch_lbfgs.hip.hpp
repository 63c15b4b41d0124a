// cgo_kernels_batch_lbfgs.hip.hpp — k_batch_lbfgs: batched solves with β = LBFGS(m), one workgroup per problem, the ring in
// device memory.
//
// k_batch_rows (cgo_kernels_batch_rows.hip.hpp) with a quasi-Newton direction.  The x, u and parameter rows are the [batch][ld]
// rows of the concatenated backend; beside them lie S[batch][m+1][ld] and Y[batch][m+1][ld], the ring of every problem, and one
// QnState per problem (cgo_qn.hpp: pair count, free slot, slot list, γ, ρ, the Gram blocks, s_j·g, y_j·g).  During a launch the
// QnState lives in LDS — the scalar recursion indexes it at run time, and a run-time index into private arrays would go to
// scratch memory.  There is no gradient row: g = ∇f(x) is recomputed from the stored x by the same expression, as in the CG family.
//
//   * R_INIT and the trial passes are RowsDev's own, unchanged (LbfgsDev derives from it);
//   * the two ring passes below are written ONCE, as LbfgsRing, for this tier and for the LDS tier
//     (cgo_kernels_batch_lbfgs_lds.hip.hpp): the tiers differ in where the rows lie, not in a pass's text;
//   * the PUSH pass, after the line search accepted a step a: per pair g, xp = x + a·u, g⁺ = ∇f(xp), s = a·u, y = g⁺ − g; x ← xp,
//     s and y into the free slot; 4 + 5c sums (those of k_lbfgs_push_gram) in a 64-slot row.  The loop over the c stored pairs is
//     unrolled to the compile-time maximum under wave-uniform `j < c` guards, so accumulator indices are compile-time constants
//     and the loads of absent pairs are skipped;
//   * the scalar recursion (qn_update, qn_coefficients) by lane 0 on the QnState in LDS; a barrier; every lane reads the same
//     coefficients;
//   * the COMBINE pass: u = −γ·g + Σ cy_j·Y_j + Σ cs_j·S_j with g recomputed from the new x; u stored; g·u, u·u and the first
//     trial points of the next line search (cg_pair's R_TRIAL block: the sums a trial pass would form).
// Lane tid owns pairs tid, tid + BLOCK, … in every pass and every row, ring rows included, lane 0 the odd tail: a lane only
// re-reads what it wrote itself, with plain loads and stores (global here, LDS in the LDS tier) — no fence and no barrier for
// data.  No atomics, no polling, no read of another problem's rows; every loop is bounded by n, m or the line search's own limits.
// The streaming loops follow RowsDev::trip: all 16-byte loads of a trip first, whole trips without a guard, the partial trip
// loading from a clamped in-row index, uniform trip counts.
// Pairs per lane and trip of the two ring passes: batch_lbfgs_u<Obj>(), a compile-time function of the objective's slot count K —
// BATCH_LBFGS_U for K ≤ 1 (the built-ins and one-slot bodies), BATCH_LBFGS_U_SLOTS for K ≥ 2, where a trip also holds K slot
// values per pair and two pairs per trip put the kernel into scratch memory.  The choice cannot change a bit of
// any result: a lane owns pairs tid, tid + BLOCK, … whatever U is, and within a trip it adds t = 0 … U−1 in ascending order into
// the same accumulators, so every per-lane sum is formed over the same pairs in the same order for every U; the reduction over
// lanes does not know U.
#pragma once

#include "cgo_kernels_batch_rows.hip.hpp"
#include "cgo_resident_qn.hpp"

#ifndef CGO_BATCH_LBFGS_U
#define CGO_BATCH_LBFGS_U 2   // A/B builds: make EXTRA=-DCGO_BATCH_LBFGS_U=…
#endif
#ifndef CGO_BATCH_LBFGS_U_SLOTS
#define CGO_BATCH_LBFGS_U_SLOTS 1   // objectives of two or more slots.  A/B builds: make EXTRA=-DCGO_BATCH_LBFGS_U_SLOTS=2
#endif

namespace cgo {
namespace dev {

constexpr int BATCH_LBFGS_U = CGO_BATCH_LBFGS_U;   // independent pairs per lane and trip of the two ring passes
static_assert(BATCH_LBFGS_U >= 1 && BATCH_LBFGS_U <= BATCH_ROWS_U, "pairs per lane and trip (the trial passes' index limit covers the ring passes')");
constexpr int BATCH_LBFGS_U_SLOTS = CGO_BATCH_LBFGS_U_SLOTS;   // … of an objective that reads two or more parameter slots
static_assert(BATCH_LBFGS_U_SLOTS >= 1 && BATCH_LBFGS_U_SLOTS <= BATCH_LBFGS_U, "an objective with slots takes no more pairs per trip than one without");
constexpr int batch_lbfgs_u_of(int nparams) { return nparams >= 2 ? BATCH_LBFGS_U_SLOTS : BATCH_LBFGS_U; }
template <class Obj> constexpr int batch_lbfgs_u() { return batch_lbfgs_u_of(obj_nparams<Obj>()); }
constexpr long long BATCH_LBFGS_MAX_N = BATCH_ROWS_MAX_N;   // the pass index limit: RowsDev's passes run here too

struct BatchLbfgsParams {
    BatchParams B;             // as k_batch_rows reads it
    double *S, *Y;             // [batch][m+1][ld]
    QnState *qn;               // [batch]
    long long ring_stride;     // (m+1)·ld: doubles between two problems' rings
};

// What the ring passes read of a tier's vector-operations object, under one set of names: x_row(), u_row(), slot_ptrs(),
// scalar().  This is RowsDev's form; the LDS tier's is in its own header.
template <class Obj, int NPTS>
struct LbfgsRows : RowsDev<Obj, NPTS> {
    using R = RowsDev<Obj, NPTS>;
    using Objective = Obj;
    __device__ __forceinline__ LbfgsRows(const R &r) : R(r) {}
    __device__ __forceinline__ double *x_row() const { return this->xr; }
    __device__ __forceinline__ double *u_row() const { return this->ur; }
    __device__ __forceinline__ ParamPtrs slot_ptrs() const { return this->pl; }
    __device__ __forceinline__ double scalar() const { return this->s0; }
};
struct RingPushNone { __device__ __forceinline__ void operator()(int) {} };   // device rows: a push stores straight to the ring

// The two ring passes of BOTH tiers: push_update and combine_trial, once.
//   Base    the tier's vector-operations object behind the four names above (R_INIT, the trial passes and the zero checks are its own);
//   Off     the type of a ring offset and of the odd tail's index: long long over device rows, int over LDS — the address
//           arithmetic is part of the device code, so each tier keeps its own;
//   U       pairs per lane and trip, from the objective's slot count (each tier passes its own function's value, once);
//   Pushed  called by a push with the free slot it is about to write.
// The per-pair expressions, the order of loads, stores and dsum calls, the `j < c` guards and the clamped tail index are the
// same text for both tiers, so every number of one tier has the bits of the other.
template <class Base, class Off, int U, class Pushed>
struct LbfgsRing : Base {
    using Obj = typename Base::Objective;
    static constexpr int NPTS = Base::kNpts;
    double *Sr, *Yr;           // this problem's ring, slot p at p·ld
    Off ld;
    QnState *q;                // LDS
    QnCoef *co;                // LDS
    double *qsum;              // LDS [QN_SUMS]
    Pushed pushed;

    __device__ __forceinline__ LbfgsRing(const typename Base::R &r, double *S, double *Y, Off ld_, QnState *q_, QnCoef *co_, double *qs)
        : Base(r), Sr(S), Yr(Y), ld(ld_), q(q_), co(co_), qsum(qs) {}

    // ---- push -----------------------------------------------------------------------------------------------------------
    template <bool TAIL>
    __device__ __forceinline__ void push_trip(double a, int c, int i0, double (&acc)[QN_SUMS]) {
        d2 xv[U], uv[U], sv[QN_MAX_M][U], yv[QN_MAX_M][U];
        PV<Obj> pv[U];
        int idx[U], il[U];
#pragma unroll
        for (int t = 0; t < U; ++t) {
            idx[t] = i0 + t * BLOCK + (int)threadIdx.x;
            il[t] = (TAIL && idx[t] >= this->npairs) ? this->npairs - 1 : idx[t];   // (a lane past the end reads the row's last pair and drops it)
            xv[t] = ldg2<false>(this->x_row(), il[t]);
            uv[t] = ldg2<false>(this->u_row(), il[t]);
            pv[t] = pv_load<Obj, false>(this->slot_ptrs(), il[t]);
        }
#pragma unroll
        for (int j = 0; j < QN_MAX_M; ++j) {
            if (j < c) {   // (wave-uniform: c is the workgroup's)
                const Off off = (Off)q->list[j] * ld;
#pragma unroll
                for (int t = 0; t < U; ++t) { sv[j][t] = ldg2<false>(Sr + off, il[t]); yv[j][t] = ldg2<false>(Yr + off, il[t]); }
            }
        }
        const Off offn = (Off)q->free_slot * ld;
#pragma unroll
        for (int t = 0; t < U; ++t) {
            if (!TAIL || idx[t] < this->npairs) {
                d2 g, gp, xp, s, y;
                double f0 = 0.0, f1 = 0.0;
                obj_eval2<Obj>(xv[t], pv[t], this->scalar(), f0, g);
                s.x = a * uv[t].x; s.y = a * uv[t].y;
                xp.x = xv[t].x + s.x; xp.y = xv[t].y + s.y;
                obj_eval2<Obj>(xp, pv[t], this->scalar(), f1, gp);
                y.x = gp.x - g.x; y.y = gp.y - g.y;
                stg2<false>(this->x_row(), idx[t], xp);
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
        const int tid = threadIdx.x;
        const int c = q->count, npairs = this->npairs;
        pushed(q->free_slot);
        double acc[QN_SUMS];
#pragma unroll
        for (int s = 0; s < QN_SUMS; ++s) acc[s] = 0.0;
        int i0 = 0;
        for (; i0 + U * BLOCK <= npairs; i0 += U * BLOCK) push_trip<false>(a, c, i0, acc);   // (uniform: npairs is the workgroup's)
        if (i0 < npairs) push_trip<true>(a, c, i0, acc);
        if (this->odd && tid == 0) {   // the odd tail element (objectives that are not pair-only)
            const Off i = (Off)2 * npairs;
            const PS<Obj> p = ps_load<Obj>(this->slot_ptrs(), i);
            double f0 = 0.0, f1 = 0.0, g = 0.0, gp = 0.0;
            const double x = this->x_row()[i];
            obj_eval1<Obj>(x, p, this->scalar(), f0, g);
            const double s = a * this->u_row()[i], xp = x + s;
            obj_eval1<Obj>(xp, p, this->scalar(), f1, gp);
            const double y = gp - g;
            const Off offn = (Off)q->free_slot * ld;
            acc[QS_SY] = dsum(acc[QS_SY], s, y); acc[QS_YY] = dsum(acc[QS_YY], y, y);
            acc[QS_SGN] = dsum(acc[QS_SGN], s, gp); acc[QS_YGN] = dsum(acc[QS_YGN], y, gp);
#pragma unroll
            for (int j = 0; j < QN_MAX_M; ++j) {
                if (j < c) {
                    const int b = QS_PAIR0 + QP_PER_PAIR * j;
                    const Off off = (Off)q->list[j] * ld;
                    const double sj = Sr[off + i], yj = Yr[off + i];
                    acc[b + QP_SJG] = dsum(acc[b + QP_SJG], sj, gp); acc[b + QP_YJG] = dsum(acc[b + QP_YJG], yj, gp);
                    acc[b + QP_SJYN] = dsum(acc[b + QP_SJYN], sj, y); acc[b + QP_YJSN] = dsum(acc[b + QP_YJSN], yj, s);
                    acc[b + QP_YJYN] = dsum(acc[b + QP_YJYN], yj, y);
                }
            }
            this->x_row()[i] = xp; Sr[offn + i] = s; Yr[offn + i] = y;
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
        d2 xv[U], sv[QN_MAX_M][U], yv[QN_MAX_M][U];
        PV<Obj> pv[U];
        int idx[U], il[U];
#pragma unroll
        for (int t = 0; t < U; ++t) {
            idx[t] = i0 + t * BLOCK + (int)threadIdx.x;
            il[t] = (TAIL && idx[t] >= this->npairs) ? this->npairs - 1 : idx[t];
            xv[t] = ldg2<false>(this->x_row(), il[t]);
            pv[t] = pv_load<Obj, false>(this->slot_ptrs(), il[t]);
        }
#pragma unroll
        for (int j = 0; j < QN_MAX_M; ++j) {
            if (j < c) {
                const Off off = (Off)q->list[j] * ld;
#pragma unroll
                for (int t = 0; t < U; ++t) { sv[j][t] = ldg2<false>(Sr + off, il[t]); yv[j][t] = ldg2<false>(Yr + off, il[t]); }
            }
        }
#pragma unroll
        for (int t = 0; t < U; ++t) {
            if (!TAIL || idx[t] < this->npairs) {
                d2 g, u;
                double f0 = 0.0;
                obj_eval2<Obj>(xv[t], pv[t], this->scalar(), f0, g);
                u.x = ng * g.x; u.y = ng * g.y;
#pragma unroll
                for (int j = 0; j < QN_MAX_M; ++j) {
                    if (j < c) { u.x = u.x + cy[j] * yv[j][t].x; u.y = u.y + cy[j] * yv[j][t].y; }
                }
#pragma unroll
                for (int j = 0; j < QN_MAX_M; ++j) {
                    if (j < c) { u.x = u.x + cs[j] * sv[j][t].x; u.y = u.y + cs[j] * sv[j][t].y; }
                }
                stg2<false>(this->u_row(), idx[t], u);
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
        const int tid = threadIdx.x;
        const int c = co->count, npairs = this->npairs;
        const double ng = -co->gamma;
        double cy[QN_MAX_M], cs[QN_MAX_M];
#pragma unroll
        for (int j = 0; j < QN_MAX_M; ++j) { cy[j] = co->cy[j]; cs[j] = co->cs[j]; }   // (compile-time indices: registers)
        RParams rp;
        rp.a_acc = 0.0; rp.beta = 0.0; rp.s0 = this->scalar(); rp.n = 0;
#pragma unroll
        for (int j = 0; j < MAXP; ++j) rp.a[j] = (j < NP && k > 0) ? a[j] : 0.0;   // the caller pads a[] to NP entries
        double acc[W];
#pragma unroll
        for (int s = 0; s < W; ++s) acc[s] = 0.0;
        int i0 = 0;
        for (; i0 + U * BLOCK <= npairs; i0 += U * BLOCK) combine_trip<NP, false>(rp, c, ng, cy, cs, i0, acc);
        if (i0 < npairs) combine_trip<NP, true>(rp, c, ng, cy, cs, i0, acc);
        if (this->odd && tid == 0) {
            const Off i = (Off)2 * npairs;
            const PS<Obj> p = ps_load<Obj>(this->slot_ptrs(), i);
            double f0 = 0.0, g = 0.0;
            obj_eval1<Obj>(this->x_row()[i], p, this->scalar(), f0, g);
            double u = ng * g;
#pragma unroll
            for (int j = 0; j < QN_MAX_M; ++j) { if (j < c) u = u + cy[j] * Yr[(Off)q->list[j] * ld + i]; }
#pragma unroll
            for (int j = 0; j < QN_MAX_M; ++j) { if (j < c) u = u + cs[j] * Sr[(Off)q->list[j] * ld + i]; }
            this->u_row()[i] = u;
            acc[RW<NP>::GU] = dsum(acc[RW<NP>::GU], g, u);
            acc[RW<NP>::UU] = dsum(acc[RW<NP>::UU], u, u);
            rp.x = this->x_row(); rp.u = this->u_row(); rp.p0 = this->slot_ptrs().p0; rp.p1 = this->slot_ptrs().p1; rp.p2 = this->slot_ptrs().p2; rp.p3 = this->slot_ptrs().p3;
            rp.xo = this->x_row(); rp.uo = this->u_row(); rp.gout = nullptr; rp.x2 = nullptr;
            cg_single<Obj, R_TRIAL, NP>(rp, i, acc);   // (reads back the u this lane stored just above)
        }
        const double own = wg_reduce_n<W>(acc);
        if (tid < W) this->tot[tid] = own;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NP; ++j) out[j] = Base::ts(this->tot + RS_PER_POINT * j);
        gu = this->tot[RW<NP>::GU]; uu = this->tot[RW<NP>::UU];
        __syncthreads();   // tot is written again by the next pass
        return 0;
    }
};

template <class Obj, int NPTS>
using LbfgsDev = LbfgsRing<LbfgsRows<Obj, NPTS>, long long, batch_lbfgs_u<Obj>(), RingPushNone>;

// ---- cgo_batch_probe: the passes the quasi-Newton loop (res_iterate_qn) issues, in its place -------------------------------------
static_assert(BATCH_PROBE_MAX_M == QN_MAX_M && BATCH_PROBE_ROW == QN_SUMS, "the probe's pass and row hold the largest ring's");
struct BatchLbfgsProbeParams : BatchLbfgsParams { BatchProbe pr; };   // (as BatchProbeParams: the kernel text reads L.… in both forms)
template <bool PROBE> struct BatchLbfgsArg { using type = BatchLbfgsParams; };
template <> struct BatchLbfgsArg<true> { using type = BatchLbfgsProbeParams; };

// trial and R_INIT are RowsDev's (batch_probe_cg_pass); a push counts as a completed iteration, as in res_iterate_qn.  A combine
// runs on the coefficients the last push left in LDS, or on those of its pass, written there by lane 0 as push_update writes them.
template <class V>
__device__ __forceinline__ void batch_lbfgs_probe_script(const BatchProbe &pr, ResState &s, V &v) {
    s.done = 0; s.log_len = 0; s.evals = 0; s.passes = 0; s.reason = RES_BUDGET;
    s.t_machine = 0; s.t_eval = 0; s.t_post = 0;
    for (int q = 0; q < pr.npass && s.reason == RES_BUDGET; ++q) {
        const BatchProbePass c = pr.script[q];
        TrialSums out[RES_MAXP] = {};
        if (c.kind == 3) {
            const int stored = v.push_update(c.a_acc);
            s.passes++; s.done++;
            batch_probe_store(pr, q, v.qsum, QN_SUMS, out, 0.0, 0.0, stored);
        } else if (c.kind == 4) {
            if (c.co_count >= 0) {
                if (threadIdx.x == 0) {
                    v.co->count = c.co_count; v.co->pad_ = 0; v.co->gamma = c.co_gamma;
                    for (int j = 0; j < QN_MAX_M; ++j) { v.co->cy[j] = c.co_cy[j]; v.co->cs[j] = c.co_cs[j]; }
                }
                __syncthreads();
            }
            double gu = 0.0, uu = 0.0;
            if (v.combine_trial(c.a, c.k, out, gu, uu)) { s.reason = RES_ERROR; break; }
            s.passes++;
            batch_probe_store(pr, q, v.tot, RW<V::kNpts>::W, out, gu, uu, v.co->count);
        } else if (c.kind == 1 || !batch_probe_cg_pass(pr, q, c, s, v, v.tot)) s.reason = RES_ERROR;   // (the host refuses such a script)
    }
}

// ---- what the kernels of both tiers share around the loop ------------------------------------------------------------------------
// (Only the pinning, and as a macro: the QnState copies, the fresh start and the state's write-out stay in the kernels — as
// __forceinline__ functions they change the kernels' instructions; DESIGN.md §2.14 has what was tried and measured.)
// As k_resident: the loop state is FP64 arithmetic throughout — into VGPRs once, opaquely; see the note there.
#define CGO_RES_V(x) asm volatile("" : "+v"(x))
#define CGO_BATCH_LBFGS_PIN(s, cfg) do { \
    CGO_RES_V(s.f_x); CGO_RES_V(s.gg); CGO_RES_V(s.norm); CGO_RES_V(s.dphi0); CGO_RES_V(s.uu); CGO_RES_V(s.a_initial); CGO_RES_V(s.last_a); CGO_RES_V(s.last_beta); \
    _Pragma("unroll") \
    for (int j = 0; j < RES_MAXP; ++j) { \
        CGO_RES_V(s.ca[j]); CGO_RES_V(s.cs[j].f); CGO_RES_V(s.cs[j].gtu); CGO_RES_V(s.cs[j].gtgt); CGO_RES_V(s.cs[j].gtg); CGO_RES_V(s.cs[j].yy); CGO_RES_V(s.cs[j].uy); CGO_RES_V(s.cs[j].ygt); \
    } \
    CGO_RES_V(cfg.ls.c1); CGO_RES_V(cfg.ls.c2); CGO_RES_V(cfg.ls.a_max_growth_factor); CGO_RES_V(cfg.ls.delta1); CGO_RES_V(cfg.ls.max_step_size); \
    CGO_RES_V(cfg.ls.discount_factor); CGO_RES_V(cfg.eps); CGO_RES_V(cfg.mu); \
} while (0)

template <class Obj, int NPTS, bool PROBE = false>
__global__ __launch_bounds__(BLOCK, 1) void k_batch_lbfgs(const typename BatchLbfgsArg<PROBE>::type L) {
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
    RowsDev<Obj, NPTS> rows{B.x + lo, B.u + lo,
                            ParamPtrs{K > 0 ? B.p0 + lo : nullptr, K > 1 ? B.p1 + lo : nullptr, K > 2 ? B.p2 + lo : nullptr, K > 3 ? B.p3 + lo : nullptr},
                            (int)(B.n >> 1), (B.n & 1) != 0, B.s0v ? B.s0v[b] : B.s0, tot};
    LbfgsDev<Obj, NPTS> v(rows, L.S + b * L.ring_stride, L.Y + b * L.ring_stride, B.ld, &s_q, &s_co, qsum);
    ResConfig cfg = B.cfg;
    CGO_BATCH_LBFGS_PIN(s, cfg);
    bool go = true;
    if (s.reason == RES_FRESH) {   // optim.jl:25-47: f_x = fdf!(df_x, x); u = −df_x (stored to the u row)
        double sums[RW<1>::W];
        v.template pass<R_INIT, 1>(0.0, 0.0, nullptr, 0, sums);
        s.f_x = sums[RS_F]; s.gg = sums[RS_GTGT];
        s.dphi0 = -s.gg; s.uu = s.gg; s.dir_neg = 1;
        s.it = 0; s.ncache = 0;
        s.done = 0; s.log_len = 0; s.evals = 0; s.passes = 1;
        if (v.leader()) B.f_x0[b] = s.f_x;
        // LinearAlgebra.norm, as k_batch_rows has it: 0 only when g IS the zero vector
        bool zero = false;
        if (s.gg == 0.0) zero = v.direction_is_zero();   // (uniform: the sums are the workgroup's)
        if (sumsq_in_range(s.gg)) s.norm = __builtin_sqrt(s.gg);
        else if (s.gg == 0.0 && zero) s.norm = 0.0;
        else { s.reason = RES_HOST; go = false; }
    }
    if (go) {
        ResRecord *recs = B.recs + b * B.rec_stride + (B.rec_abs ? s.it : 0);
        if constexpr (PROBE) batch_lbfgs_probe_script(L.pr, s, v);
        else res_iterate_qn(cfg, s, v, (int64_t)B.budget, recs);
    }
    s.t_total = 0; s.t_compute = 0; s.t_reduce = 0; s.t_exchange = 0; s.t_cycles = 0;
    constexpr int WS = sizeof(ResState) / 8;
    static_assert(sizeof(ResState) % 8 == 0 && WS <= BLOCK, "the state goes out as 8-byte words, one lane each");
    if (tid == 0) s_out = s;
    __syncthreads();   // (also: lane 0's last recursion on s_q is complete)
    if (tid < WS) reinterpret_cast<unsigned long long *>(B.st + b)[tid] = reinterpret_cast<const unsigned long long *>(&s_out)[tid];
    for (int i = tid; i < QW; i += BLOCK)
        reinterpret_cast<unsigned long long *>(L.qn + b)[i] = reinterpret_cast<const unsigned long long *>(&s_q)[i];
}

}  // namespace dev
}  // namespace cgo
