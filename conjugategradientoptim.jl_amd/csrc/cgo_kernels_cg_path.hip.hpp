// cgo_kernels_cg_path.hip.hpp — path launches (predicted path): launches N and S of the replay cycle, in their lean
// form, evaluating only the trial points the line search is predicted to ask for (cgo_path.hpp).
//
// k_cg_path<Obj, MODE, NACT, true> is k_cg<Obj, MODE, 7, true> (cgo_kernels_cg.hip.hpp) with two differences:
//   * of the seven trial points of the row only the first NACT are evaluated.  THE ROW KEEPS THE WIDTH AND SLOT POSITIONS OF THE
//     7-POINT ROW (RW<7>: 56 slots, the same wg_reduce_n<56>, the same k_finalize_one<56>); the accumulators of the other points
//     are never touched after their 0.0 and leave as +0.0 — the rule the lean rows follow for dropped sums.  An evaluated point's
//     accumulators run the chains of the 7-point launch over the same partition, so its sums, g·u and u·u have the bits the 7-point
//     lean launch gives for the same step: whole solves stay byte-identical;
//   * where the objective declares a constant Hessian (ObjCurv) every evaluated point also forms Σ g⁺·(H g⁺), in the slot of
//     Σ y·y, which the Polak–Ribière mask leaves unread.  No slot of any other row changes meaning;
//   * it replays up to RCAP = 15 accepted steps instead of RMAX = 7: those beyond the seventh arrive in a second kernel argument
//     (RDeep, below — deep replay), as they do for the deep trial launch k_cg_trial_deep at the end of this file.
//
// A header and a body of its own, not template arguments of cg_pair / cg_launch: the text of cgo_kernels_cg.hip.hpp is part of
// every run-time compiled module (gen_rtc_sources.py) and stays what it is.  The body below repeats, expression for expression
// and in the same order, what cg_pair / cg_single / cg_launch do for these modes — replay, accept, direction, trial, late f —
// and nothing else; tests/test_path_rows.py holds the two against each other bit for bit.  Built-in objectives only.
#pragma once

#include "cgo_kernels_cg.hip.hpp"

namespace cgo {
namespace dev {

// Constant Hessian: H v for an objective whose Hessian does not depend on x.  Declared for ObjQuadDiag only (H = diag D).
template <class Obj> struct ObjCurv { static constexpr bool declared = false; };
template <> struct ObjCurv<ObjQuadDiag> {
    static constexpr bool declared = true;
    __device__ static inline d2 apply2(d2 v, const PV<ObjQuadDiag> &p) { return d2{p.v[0].x * v.x, p.v[0].y * v.y}; }
    __device__ static inline double apply1(double v, const PS<ObjQuadDiag> &p) { return p.v[0] * v; }
};

// the modes a path row can have: launch N or S of the replay cycle with a mask that leaves the y·y slot free
constexpr bool path_mode(int mode) {
    return (r_base(mode) == (R_REPLAY | R_ACCEPT | R_DIR | R_TRIAL | R_NOWU | R_NOWX) || r_base(mode) == (R_REPLAY | R_ACCEPT | R_DIR | R_TRIAL)) &&
           (mode & R_NOYY) != 0;
}

// Deep replay: RParams holds the first RMAX accepted steps; a path launch and the deep trial launch take the steps
// beyond them — up to RDEEP more, replay depth up to RMAX + RDEEP + 1 = 16 — in a second kernel argument.  RParams, and with it the
// text of every run-time compiled module, stays what it is.  nrep2 > 0 only where P.nrep == RMAX.
constexpr int RDEEP = 8;
constexpr int RCAP = RMAX + RDEEP;   // most steps a path launch or the deep trial launch replays
struct RDeep {
    int nrep2;
    double ra2[RDEEP], rb2[RDEEP];
};
// How the deep steps reach the lanes.  Read as scalar operands like P.ra / P.rb, their 32 words are live across the streaming loop
// next to the ≈ 80 the loop already holds: past the scalar register file, so the register allocator parks words in lanes of a
// vector register and fetches them back inside the loop, several moves per replayed step.  Instead wave 0's first lane leaves the
// sixteen values in LDS once, before the loop, and a replayed step reads its pair from there: every lane the same address (a
// broadcast, no bank conflict), two vector registers for the length of the step.  LDS takes a run-time index, so the deep steps
// are a counted loop — one scalar counter instead of eight wave-uniform guards — kept rolled: unrolled, its reads would move out
// of the streaming loop and hold 32 vector registers across it.
struct RDeepLds { double a[RDEEP], b[RDEEP]; };
__device__ inline void rdeep_stage(const RDeep &Q, RDeepLds &L) {
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < RDEEP; ++j) { L.a[j] = Q.ra2[j]; L.b[j] = Q.rb2[j]; }
    }
    __syncthreads();
}

// R_REPLAY: steps 1 … RMAX from P (compile-time slot indices under a wave-uniform guard: see cg_pair), then steps RMAX + 1 … from
// LDS — the R_ACCEPT and R_DIR expressions of cg_pair, in its order
template <class Obj>
__device__ inline void replay_pair(const RParams &P, const RDeep &Q, const RDeepLds &L, d2 &x, d2 &u, const PV<Obj> &p) {
#pragma unroll
    for (int j = 0; j < RMAX; ++j) {
        if (j < P.nrep) {
            d2 gr;
            double fr = 0.0;
            x.x = x.x + P.ra[j] * u.x;
            x.y = x.y + P.ra[j] * u.y;
            obj_eval2<Obj>(x, p, P.s0, fr, gr);
            u.x = -gr.x + P.rb[j] * u.x; u.y = -gr.y + P.rb[j] * u.y;
        }
    }
#pragma nounroll
    for (int j = 0; j < Q.nrep2; ++j) {
        const double ra = L.a[j], rb = L.b[j];
        d2 gr;
        double fr = 0.0;
        x.x = x.x + ra * u.x;
        x.y = x.y + ra * u.y;
        obj_eval2<Obj>(x, p, P.s0, fr, gr);
        u.x = -gr.x + rb * u.x; u.y = -gr.y + rb * u.y;
    }
}
template <class Obj>
__device__ inline void replay_single(const RParams &P, const RDeep &Q, const RDeepLds &L, double &x, double &u, const PS<Obj> &p) {
#pragma unroll
    for (int j = 0; j < RMAX; ++j) {
        if (j < P.nrep) {
            double gr = 0.0, fr = 0.0;
            x = x + P.ra[j] * u;
            obj_eval1<Obj>(x, p, P.s0, fr, gr);
            u = -gr + P.rb[j] * u;
        }
    }
#pragma nounroll
    for (int j = 0; j < Q.nrep2; ++j) {
        const double ra = L.a[j], rb = L.b[j];
        double gr = 0.0, fr = 0.0;
        x = x + ra * u;
        obj_eval1<Obj>(x, p, P.s0, fr, gr);
        u = -gr + rb * u;
    }
}

template <class Obj, int MODE, int NACT>
__device__ inline void cg_path_pair(const RParams &P, const RDeep &Q, const RDeepLds &L, d2 &x, d2 &u, const PV<Obj> &p, double (&acc)[RW<MAXP>::W], bool &wx, bool &wu) {
    constexpr int R_GU = RW<MAXP>::GU, R_UU = RW<MAXP>::UU;
    replay_pair<Obj>(P, Q, L, x, u, p);   // R_REPLAY
    x.x = x.x + P.a_acc * u.x;   // R_ACCEPT
    x.y = x.y + P.a_acc * u.y;
    wx = r_writes_x(MODE);
    d2 g;
    double f0 = 0.0;
    obj_eval2<Obj>(x, p, P.s0, f0, g);
    {   // R_DIR
        d2 un;
        un.x = -g.x + P.beta * u.x; un.y = -g.y + P.beta * u.y;
        acc[R_GU] = dsum(acc[R_GU], g.x, un.x); acc[R_GU] = dsum(acc[R_GU], g.y, un.y);
        acc[R_UU] = dsum(acc[R_UU], un.x, un.x); acc[R_UU] = dsum(acc[R_UU], un.y, un.y);
        u = un;
        wu = r_writes_u(MODE);
    }
#pragma unroll
    for (int j = 0; j < NACT; ++j) {   // R_TRIAL, the first NACT points
        const int b = RS_PER_POINT * j;
        d2 xp, gt;
        xp.x = x.x + P.a[j] * u.x;
        xp.y = x.y + P.a[j] * u.y;
        obj_term2<Obj, LateF<Obj, MODE>::on>(xp, p, P.s0, acc[b + RS_F], gt);
        const double y0 = gt.x - g.x, y1 = gt.y - g.y;
        acc[b + RS_GTU] = dsum(acc[b + RS_GTU], gt.x, u.x);   acc[b + RS_GTU] = dsum(acc[b + RS_GTU], gt.y, u.y);
        acc[b + RS_GTGT] = dsum(acc[b + RS_GTGT], gt.x, gt.x); acc[b + RS_GTGT] = dsum(acc[b + RS_GTGT], gt.y, gt.y);
        if (!(MODE & R_NOGTG)) { acc[b + RS_GTG] = dsum(acc[b + RS_GTG], gt.x, g.x);   acc[b + RS_GTG] = dsum(acc[b + RS_GTG], gt.y, g.y); }
        if (!(MODE & R_NOUY)) { acc[b + RS_UY] = dsum(acc[b + RS_UY], u.x, y0);      acc[b + RS_UY] = dsum(acc[b + RS_UY], u.y, y1); }
        if (!(MODE & R_NOYGT)) { acc[b + RS_YGT] = dsum(acc[b + RS_YGT], y0, gt.x);    acc[b + RS_YGT] = dsum(acc[b + RS_YGT], y1, gt.y); }
        if constexpr (ObjCurv<Obj>::declared) {   // Σ g⁺·(H g⁺): the one sum the curvature model lacks
            const d2 hg = ObjCurv<Obj>::apply2(gt, p);
            acc[b + RS_YY] = dsum(acc[b + RS_YY], gt.x, hg.x); acc[b + RS_YY] = dsum(acc[b + RS_YY], gt.y, hg.y);
        }
    }
}

// odd tail element
template <class Obj, int MODE, int NACT>
__device__ inline void cg_path_single(const RParams &P, const RDeep &Q, const RDeepLds &L, long long i, double (&acc)[RW<MAXP>::W]) {
    constexpr int R_GU = RW<MAXP>::GU, R_UU = RW<MAXP>::UU;
    double x = P.x[i];
    double u = P.u[i];
    const PS<Obj> p = ps_load<Obj>(P, i);
    replay_single<Obj>(P, Q, L, x, u, p);
    x = x + P.a_acc * u;
    if (r_writes_x(MODE)) P.xo[i] = x;
    double g = 0.0, f0 = 0.0;
    obj_eval1<Obj>(x, p, P.s0, f0, g);
    const double un = -g + P.beta * u;
    acc[R_GU] = dsum(acc[R_GU], g, un); acc[R_UU] = dsum(acc[R_UU], un, un);
    if (r_writes_u(MODE)) P.uo[i] = un;
    u = un;
#pragma unroll
    for (int j = 0; j < NACT; ++j) {
        const int b = RS_PER_POINT * j;
        const double xp = x + P.a[j] * u;
        double gt;
        obj_term1<Obj, LateF<Obj, MODE>::on>(xp, p, P.s0, acc[b + RS_F], gt);
        const double y = gt - g;
        acc[b + RS_GTU] = dsum(acc[b + RS_GTU], gt, u); acc[b + RS_GTGT] = dsum(acc[b + RS_GTGT], gt, gt);
        if (!(MODE & R_NOGTG)) acc[b + RS_GTG] = dsum(acc[b + RS_GTG], gt, g);
        if (!(MODE & R_NOUY)) acc[b + RS_UY] = dsum(acc[b + RS_UY], u, y);
        if (!(MODE & R_NOYGT)) acc[b + RS_YGT] = dsum(acc[b + RS_YGT], y, gt);
        if constexpr (ObjCurv<Obj>::declared) acc[b + RS_YY] = dsum(acc[b + RS_YY], gt, ObjCurv<Obj>::apply1(gt, p));
    }
}

// the pure-HBM streaming loop of cg_launch (BIG): one chunk per workgroup, two independent 16-B groups per lane per trip
// (BIG: the streaming policy, as the last argument of every k_cg symbol — always true here)
template <class Obj, int MODE, int NACT, bool BIG>
__global__ __launch_bounds__(BLOCK) void k_cg_path(const RParams P, const RDeep Q) {
    static_assert(BIG, "path launches exist as pure-HBM streams only");
    static_assert(path_mode(MODE), "a path row is launch N or S of the replay cycle in a lean form that leaves the y·y slot free");
    static_assert(NACT >= 1 && NACT <= MAXP, "1 … 7 of the row's seven points");
    constexpr int W = RW<MAXP>::W;
    double acc[W];
#pragma unroll
    for (int s = 0; s < W; ++s) acc[s] = 0.0;
    __shared__ RDeepLds L;
    rdeep_stage(Q, L);
    const long long n2 = P.n >> 1;
    const long long per = big_chunk_pairs(n2, gridDim.x);
    long long i = per * blockIdx.x + threadIdx.x;
    const long long hi = (per * blockIdx.x + per < n2) ? per * blockIdx.x + per : n2;
    const long long step = BLOCK;
    for (; i + step < hi; i += 2 * step) {
        d2 xa = ldg2<true>(P.x, i), xb = ldg2<true>(P.x, i + step);
        d2 ua = ldg2<true>(P.u, i), ub = ldg2<true>(P.u, i + step);
        const PV<Obj> pa = pv_load<Obj, true>(P, i), pb = pv_load<Obj, true>(P, i + step);
        bool wxa = false, wua = false, wxb = false, wub = false;
        cg_path_pair<Obj, MODE, NACT>(P, Q, L, xa, ua, pa, acc, wxa, wua);
        cg_path_pair<Obj, MODE, NACT>(P, Q, L, xb, ub, pb, acc, wxb, wub);
        if (wxa) stg2<true>(P.xo, i, xa);
        if (wua) stg2<true>(P.uo, i, ua);
        if (wxb) stg2<true>(P.xo, i + step, xb);
        if (wub) stg2<true>(P.uo, i + step, ub);
    }
    if (i < hi) {
        d2 xa = ldg2<true>(P.x, i);
        d2 ua = ldg2<true>(P.u, i);
        const PV<Obj> pa = pv_load<Obj, true>(P, i);
        bool wxa = false, wua = false;
        cg_path_pair<Obj, MODE, NACT>(P, Q, L, xa, ua, pa, acc, wxa, wua);
        if (wxa) stg2<true>(P.xo, i, xa);
        if (wua) stg2<true>(P.uo, i, ua);
    }
    if ((P.n & 1) && blockIdx.x == 0 && threadIdx.x == 0) cg_path_single<Obj, MODE, NACT>(P, Q, L, P.n - 1, acc);
    if constexpr (LateF<Obj, MODE>::on) {   // the lane's sums of raw terms → its f sums, once
#pragma unroll
        for (int j = 0; j < NACT; ++j) acc[RS_PER_POINT * j + RS_F] *= ObjFScale<Obj>::scale;
    }
    store_partials_n<W, false>(acc, P.partials, P.tail);
}

// ---- the deep trial launch (T deep) ---------------------------------------------------------------------------------------------
// A trial-only launch met with more than RMAX steps outstanding: k_cg<Obj, R_REPLAY | R_TRIAL, NPTS, true> with the steps beyond
// its RMAX taken from the second argument.  Full rows — all seven sums of every point, RW<NPTS>, the same wg_reduce_n and finalize —
// and, expression for expression and in the same order, what cg_pair / cg_single / cg_launch do for that mode: from the same
// registers after the replay it leaves the row k_cg leaves (tests/test_deep_replay.py holds the two against each other bit for bit).
// Nothing is stored.
template <class Obj, int NPTS>
__device__ inline void cg_trial_points2(const RParams &P, const d2 &x, const d2 &u, const PV<Obj> &p, double (&acc)[RW<NPTS>::W]) {
    d2 g;
    double f0 = 0.0;
    obj_eval2<Obj>(x, p, P.s0, f0, g);
#pragma unroll
    for (int j = 0; j < NPTS; ++j) {
        const int b = RS_PER_POINT * j;
        d2 xp, gt;
        xp.x = x.x + P.a[j] * u.x;
        xp.y = x.y + P.a[j] * u.y;
        obj_term2<Obj, false>(xp, p, P.s0, acc[b + RS_F], gt);
        const double y0 = gt.x - g.x, y1 = gt.y - g.y;
        acc[b + RS_GTU] = dsum(acc[b + RS_GTU], gt.x, u.x);   acc[b + RS_GTU] = dsum(acc[b + RS_GTU], gt.y, u.y);
        acc[b + RS_GTGT] = dsum(acc[b + RS_GTGT], gt.x, gt.x); acc[b + RS_GTGT] = dsum(acc[b + RS_GTGT], gt.y, gt.y);
        acc[b + RS_GTG] = dsum(acc[b + RS_GTG], gt.x, g.x);   acc[b + RS_GTG] = dsum(acc[b + RS_GTG], gt.y, g.y);
        acc[b + RS_YY] = dsum(acc[b + RS_YY], y0, y0);       acc[b + RS_YY] = dsum(acc[b + RS_YY], y1, y1);
        acc[b + RS_UY] = dsum(acc[b + RS_UY], u.x, y0);      acc[b + RS_UY] = dsum(acc[b + RS_UY], u.y, y1);
        acc[b + RS_YGT] = dsum(acc[b + RS_YGT], y0, gt.x);    acc[b + RS_YGT] = dsum(acc[b + RS_YGT], y1, gt.y);
    }
}

template <class Obj, int NPTS, bool BIG>
__global__ __launch_bounds__(BLOCK) void k_cg_trial_deep(const RParams P, const RDeep Q) {
    static_assert(BIG, "replay launches exist as pure-HBM streams only");
    static_assert(NPTS == 1 || NPTS == 3 || NPTS == 5 || NPTS == 7, "a launch evaluates 1, 3, 5 or 7 trial points");
    constexpr int W = RW<NPTS>::W;
    double acc[W];
#pragma unroll
    for (int s = 0; s < W; ++s) acc[s] = 0.0;
    __shared__ RDeepLds L;
    rdeep_stage(Q, L);
    const long long n2 = P.n >> 1;
    const long long per = big_chunk_pairs(n2, gridDim.x);
    long long i = per * blockIdx.x + threadIdx.x;
    const long long hi = (per * blockIdx.x + per < n2) ? per * blockIdx.x + per : n2;
    const long long step = BLOCK;
    for (; i + step < hi; i += 2 * step) {
        d2 xa = ldg2<true>(P.x, i), xb = ldg2<true>(P.x, i + step);
        d2 ua = ldg2<true>(P.u, i), ub = ldg2<true>(P.u, i + step);
        const PV<Obj> pa = pv_load<Obj, true>(P, i), pb = pv_load<Obj, true>(P, i + step);
        replay_pair<Obj>(P, Q, L, xa, ua, pa);
        cg_trial_points2<Obj, NPTS>(P, xa, ua, pa, acc);
        replay_pair<Obj>(P, Q, L, xb, ub, pb);
        cg_trial_points2<Obj, NPTS>(P, xb, ub, pb, acc);
    }
    if (i < hi) {
        d2 xa = ldg2<true>(P.x, i);
        d2 ua = ldg2<true>(P.u, i);
        const PV<Obj> pa = pv_load<Obj, true>(P, i);
        replay_pair<Obj>(P, Q, L, xa, ua, pa);
        cg_trial_points2<Obj, NPTS>(P, xa, ua, pa, acc);
    }
    if ((P.n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // odd tail element
        const long long e = P.n - 1;
        double x = P.x[e];
        double u = P.u[e];
        const PS<Obj> p = ps_load<Obj>(P, e);
        replay_single<Obj>(P, Q, L, x, u, p);
        double g = 0.0, f0 = 0.0;
        obj_eval1<Obj>(x, p, P.s0, f0, g);
#pragma unroll
        for (int j = 0; j < NPTS; ++j) {
            const int b = RS_PER_POINT * j;
            const double xp = x + P.a[j] * u;
            double gt;
            obj_term1<Obj, false>(xp, p, P.s0, acc[b + RS_F], gt);
            const double y = gt - g;
            acc[b + RS_GTU] = dsum(acc[b + RS_GTU], gt, u); acc[b + RS_GTGT] = dsum(acc[b + RS_GTGT], gt, gt);
            acc[b + RS_GTG] = dsum(acc[b + RS_GTG], gt, g);
            acc[b + RS_YY] = dsum(acc[b + RS_YY], y, y);
            acc[b + RS_UY] = dsum(acc[b + RS_UY], u, y);
            acc[b + RS_YGT] = dsum(acc[b + RS_YGT], y, gt);
        }
    }
    store_partials_n<W, false>(acc, P.partials, P.tail);
}

}  // namespace dev
}  // namespace cgo
