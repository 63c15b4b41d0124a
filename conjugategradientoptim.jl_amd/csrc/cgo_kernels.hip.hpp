// cgo_kernels.hip.hpp — fused BLAS-1 streaming kernels for gfx950 (MI355X, CDNA4).
//
// One template, k_fused<Obj, MODE>, covers every vector pass of the reference's
// outer iteration (src/engine/optim.jl:50-160).  Which of the reference's
// separate loops / BLAS calls are folded into a launch is selected at compile
// time by MODE:
//
//   M_ACCEPT  x ← x + a·u                         (= x[:] = info.xp, optim.jl:136,140;
//                                                    the trial AXPY of cg_utils.jl:14-16)
//   M_DIR     u ← −g + β·u ; Σ g·u, Σ u·u          (updatedir!, cg_flavours.jl:10-12;
//                                                    dϕ₀ of nocedal.jl:56 / wolfe.jl:40;
//                                                    dot(u,u) of wolfe.jl:240)
//   M_TRIAL   xp = x + a·u ; g⁺ = ∇f(xp) ; Σ f, Σ g⁺·u, Σ g⁺·g⁺
//                                                  (evalϕdϕ!, cg_utils.jl:4-23; norm, optim.jl:107)
//   M_BETA    + Σ g⁺·g, Σ y·y, Σ u·y, Σ y·g⁺        (every dot of getβ, cg_flavours.jl:46-170)
//   M_INIT    g = ∇f(x) ; u = −g ; Σ f, Σ g·g      (optim.jl:25-26, cg_flavours.jl:29)
//   M_RESET   u = −g ; Σ g·u, Σ u·u                (wolfe.jl:129)
//   M_UPG     Σ (u+g)²                             (wolfe.jl:123)
//   M_BETAONLY partial sums of getβ from g⁺, g, u   (kernel-level entry point)
//
// Bandwidth-bound FP64 VALU work, no MFMA.  Design for CDNA4:
//   * every lane moves 16 B per access (dwordx4) on each of up to 4 input and 3
//     output streams; two independent 16-B groups per lane per loop trip keep
//     ≥ 8 loads in flight per lane; grid = min(work, 256 CUs × 8 workgroups);
//   * per-lane FP64 accumulators → 64-wide wavefront __shfl_down tree → LDS
//     across the 4 waves → one partial row per workgroup (plain stores) → a
//     one-workgroup k_finalize launch sums the rows in a fixed order.  Measured
//     on MI355X (scripts/tune): an in-kernel last-block ticket costs 12–16 µs
//     (one atomic word saturates at ≈88 arrivals/µs; an agent-scope release
//     fence per workgroup writes back the XCD L2 and costs ≈100 µs at n = 1e7),
//     the extra launch boundary ≈5 µs.  No float atomics: results are
//     bit-reproducible run to run for a given (n, grid).
//   * two streaming policies, chosen per launch by bytes moved (BIG):
//       BIG = false  grid-stride, default cache policy, ≤ 1024 workgroups —
//                    best while part of the working set lives in the 256 MiB
//                    Infinity Cache (n ≲ 3e7);
//       BIG = true   one contiguous chunk per workgroup, 4096 workgroups,
//                    non-temporal loads/stores — +9 % at n = 1e8 (5.97 TB/s).
//   * arithmetic is unfused (build with -ffp-contract=off) to round like the
//     Julia reference, which never contracts a*b+c.
#pragma once

#ifndef CGO_RTC  // the run-time (hiprtc) build of user objectives gets these from the hiprtc builtins
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif
#include "cgo_modes.hpp"   // M_*: the mode bits, and what a mode loads and stores

namespace cgo {
namespace dev {

typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int NS = 10;  // scalar slots per launch
enum Slot : int { S_F = 0, S_GTU, S_GTGT, S_GTG, S_YY, S_UY, S_YGT, S_GU, S_UU, S_GG };

constexpr int BLOCK = 256;      // 4 wavefronts of 64
constexpr int GRID_SMALL = 1024;  // grid-stride path: 256 CUs × 4 workgroups
constexpr int GRID_BIG = 4096;    // contiguous-chunk path
constexpr int MAX_GRID = 4096;    // partial-row capacity

struct KParams {
    double *x;          // current iterate (updated in place by M_ACCEPT)
    double *u;          // search direction (updated in place by M_DIR / M_INIT / M_RESET)
    const double *g;    // current gradient
    double *gt;         // trial gradient g⁺ (written by M_TRIAL / M_INIT)
    const double *p0;   // objective parameter vector (e.g. D)
    long long n;        // local length
    long long offset;   // global index of local element 0
    double a_acc, beta, a_trial;
    double s0;          // objective scalar (e.g. λ)
    double *partials;   // [gridDim.x][NS]
    double *out;        // [NS] local sums (written by k_finalize)
    const double *p1, *p2, *p3;   // parameter slots 1–3 (run-time compiled objectives with kParams > 1 only)
};

// ---- objective functors (device form of the `fdf!` contract) ---------------
// eval2: two consecutive elements (an aligned pair); eval1: odd tail element.
struct ObjQuadDiag {  // f = ½ Σ D_i x_i²
    static constexpr bool kParam = true;
    static constexpr bool kPairOnly = false;
    __device__ static inline void eval2(d2 x, d2 p, double, double &f, d2 &g) {
        g.x = p.x * x.x;
        g.y = p.y * x.y;
        f += 0.5 * (g.x * x.x);
        f += 0.5 * (g.y * x.y);
    }
    __device__ static inline void eval1(double x, double p, double, double &f, double &g) {
        g = p * x;
        f += 0.5 * (g * x);
    }
    // f = kFScale · Σ raw terms (ObjFScale below): the same g, the terms D_i x_i² without the factor
    static constexpr double kFScale = 0.5;
    __device__ static inline void eval2_raw(d2 x, d2 p, double, double &f, d2 &g) {
        g.x = p.x * x.x;
        g.y = p.y * x.y;
        f += g.x * x.x;
        f += g.y * x.y;
    }
    __device__ static inline void eval1_raw(double x, double p, double, double &f, double &g) {
        g = p * x;
        f += g * x;
    }
};

struct ObjRosenPaired {  // f = Σ_j 100 (x_{2j+1} − x_{2j}²)² + (1 − x_{2j})²   (0-based)
    static constexpr bool kParam = false;
    static constexpr bool kPairOnly = true;
    __device__ static inline void eval2(d2 x, d2, double, double &f, d2 &g) {
        const double t1 = x.y - x.x * x.x;
        const double t2 = 1.0 - x.x;
        f += 100.0 * (t1 * t1) + t2 * t2;
        g.x = -400.0 * (x.x * t1) - 2.0 * t2;
        g.y = 200.0 * t1;
    }
    __device__ static inline void eval1(double, double, double, double &, double &g) { g = 0.0; }
};

struct ObjBooth {  // examples/helpers/test_funcs.jl:3-12, n = 2
    static constexpr bool kParam = false;
    static constexpr bool kPairOnly = true;
    __device__ static inline void eval2(d2 p, d2, double, double &f, d2 &g) {
        const double t1 = p.x + 2 * p.y - 7, t2 = 2 * p.x + p.y - 5;
        f += t1 * t1 + t2 * t2;
        g.x = 2 * t1 + 2 * t2 * 2;
        g.y = 2 * t1 * 2 + 2 * t2;
    }
    __device__ static inline void eval1(double, double, double, double &, double &g) { g = 0.0; }
};

// ---- parameter slots ---------------------------------------------------------
// A functor reads K parameter vectors: K = kParam ? 1 : 0 with the scalar-`p` signatures above (every built-in), or — run-time
// compiled objectives only — `static constexpr int kParams = K` (2 ≤ K ≤ MAX_PARAM_SLOTS) with
//     eval1(double x, const double (&p)[K], double s0, double &f, double &g)
//     eval2(d2 x,     const d2     (&p)[K], double s0, double &f, d2 &g).
// The kernels hold an element's parameters in a PV / PS bundle (one register set per slot), fill it with pv_load / ps_load
// and evaluate through obj_eval1 / obj_eval2, which hand slot 0 to a scalar-`p` functor: no kernel body tells the two apart.
constexpr int MAX_PARAM_SLOTS = 4;   // = CGO_MAX_PARAM_SLOTS
template <class Obj, class = void> struct ObjParams { static constexpr int K = Obj::kParam ? 1 : 0; static constexpr bool array = false; };
template <class Obj> struct ObjParams<Obj, decltype((void)Obj::kParams)> {
    static constexpr int K = Obj::kParams; static constexpr bool array = true;
    static_assert(K >= 2 && K <= MAX_PARAM_SLOTS, "kParams must be 2, 3 or 4 (0 or 1 slot: kParam and the scalar-p signatures)");
};
template <class Obj> constexpr int obj_nparams() { return ObjParams<Obj>::K; }
template <class Obj> struct PV { d2 v[obj_nparams<Obj>() > 1 ? obj_nparams<Obj>() : 1]; };       // an aligned pair of every slot
template <class Obj> struct PS { double v[obj_nparams<Obj>() > 1 ? obj_nparams<Obj>() : 1]; };   // one element of every slot
template <class Obj> __device__ inline void obj_eval2(d2 x, const PV<Obj> &p, double s0, double &f, d2 &g) {
    if constexpr (ObjParams<Obj>::array) Obj::eval2(x, p.v, s0, f, g);
    else Obj::eval2(x, p.v[0], s0, f, g);
}
template <class Obj> __device__ inline void obj_eval1(double x, const PS<Obj> &p, double s0, double &f, double &g) {
    if constexpr (ObjParams<Obj>::array) Obj::eval1(x, p.v, s0, f, g);
    else Obj::eval1(x, p.v[0], s0, f, g);
}
// Late scaling.  A functor may declare `static constexpr double kFScale = c`, c a power of two, together with eval2_raw / eval1_raw
// (the scalar-`p` signatures): they form g exactly as eval2 / eval1 do and add the objective's terms to f WITHOUT the factor c, so
// that f = c · Σ raw terms.  Scaling by a power of two commutes with rounding — fl(c·a + c·b) = c · fl(a + b) — while no term or
// partial sum is subnormal and the unscaled sum stays finite, so a launch may accumulate the raw terms and scale each lane's sum
// once (the lean rows of k_cg: LateF, cgo_kernels_cg.hip.hpp).  Declared by ObjQuadDiag only.
template <class Obj, class = void> struct ObjFScale { static constexpr bool declared = false; static constexpr double scale = 1.0; };
template <class Obj> struct ObjFScale<Obj, decltype((void)Obj::kFScale)> {
    static constexpr bool declared = true; static constexpr double scale = Obj::kFScale;
    static_assert(!ObjParams<Obj>::array, "eval2_raw / eval1_raw take the scalar-p signatures");
};
template <class Obj, bool RAW> __device__ inline void obj_term2(d2 x, const PV<Obj> &p, double s0, double &f, d2 &g) {
    if constexpr (RAW) Obj::eval2_raw(x, p.v[0], s0, f, g);
    else obj_eval2<Obj>(x, p, s0, f, g);
}
template <class Obj, bool RAW> __device__ inline void obj_term1(double x, const PS<Obj> &p, double s0, double &f, double &g) {
    if constexpr (RAW) Obj::eval1_raw(x, p.v[0], s0, f, g);
    else obj_eval1<Obj>(x, p, s0, f, g);
}
// Slot J of an argument block that carries p0 … p3. J is a compile-time constant at every use: a run-time index into the
// argument copy would send the whole block to scratch (the note at cg_launch's reduction tail, cgo_kernels_cg.hip.hpp).
template <int J, class A> __device__ inline const double *param_slot(const A &P) {
    static_assert(J >= 0 && J < MAX_PARAM_SLOTS, "no such slot");
    if constexpr (J == 0) return P.p0;
    else if constexpr (J == 1) return P.p1;
    else if constexpr (J == 2) return P.p2;
    else return P.p3;
}
struct ParamPtrs { const double *p0, *p1, *p2, *p3; };

// One term of a dot product: acc + a·b with ONE rounding (v_fma_f64).  The reference's dots are BLAS calls
// (LinearAlgebra.dot → OpenBLAS ddot: FMA kernels, SIMD order — SURVEY.md §8a "Julia numerics facts"), so how a
// partial sum is rounded is not part of its contract, and the 7-point launches are short of FP64 issue slots, not of
// bytes (≈ 280 VALU instructions per element pair unfused, ≈ 190 fused).  Everything ELEMENT-WISE — xp, g⁺, u, y, f_i —
// stays unfused (-ffp-contract=off) and bit-identical to the oracle's.  -DCGO_PLAIN_SUMS restores mul + add (A/B).
__device__ inline double dsum(double acc, double a, double b) {
#ifdef CGO_PLAIN_SUMS
    return acc + a * b;
#else
    return __builtin_fma(a, b, acc);
#endif
}

// Where the LAST workgroup of a launch leaves the finished sums (fused reduction tail: finish_tail).
struct Tail {
    double *partials2;             // [≤ 64][N] one row per group of 64 workgroups (fused launches only: TAIL_EMPTY between launches)
    unsigned int *tickets;         // [64 + 1] arrival counters, zero between launches, then one error counter; nullptr = rows only (a finalize launch follows)
    double *out;                   // [N] device copy of the sums
    double *host_out;              // pinned host block / mailbox slot, or nullptr
    unsigned long long *host_seq;  // released with `seq` once host_out is complete
    unsigned long long seq;
    int strict;                    // 1: formal system-scope fence + release store for the host block
    // controller-armed launch (cgo_ctl.hpp): the finisher also runs ctl_step() on the sums and publishes the round's record
    void *ctl;                     // CtlDev* — config, state, the next launch's arguments, the round counter; nullptr = host-driven
    void *ctl_rec;                 // CtlRecord[PIPE_RING], pinned host memory
    unsigned long long *ctl_seq;   // [PIPE_RING] their words
    // multi-rank armed launch: every rank's device mailbox ([2][xw][XSLOT] doubles, cgo_comm.hip) as THIS device addresses it
    double *xmail[8];
    int xw, xme;                   // world size (0 / 1: no exchange), this rank
    unsigned long long xseq0;      // the solver's epoch on its context, shifted: block numbers never repeat between solvers
};
constexpr int XSLOT = 72;          // doubles per mailbox slot: 64 values + the check word + padding (= ShmComm::SLOT)
// The host block of a fused launch validates itself: its word is  seq·C + Σ_t bits(v_t)·K_t  (mod 2^64, K_t odd and
// different per slot), so the host accepts the block only when every one of its N values AND the word have arrived —
// in whatever order the writes cross the fabric.  (A release fence would order them, but at system scope it is a
// write-back + invalidate of the XCD's L2 on the critical path; finish_tail, T.strict.)
#ifdef CGO_RTC
#define CGO_TAIL_HD __device__
#else
#define CGO_TAIL_HD __host__ __device__
#endif
CGO_TAIL_HD inline unsigned long long tail_check_term(unsigned long long bits, int slot) {
    return bits * (0x9E3779B97F4A7C15ull * (unsigned long long)(2 * slot + 1));
}
CGO_TAIL_HD inline unsigned long long tail_check_seq(unsigned long long seq) { return seq * 0xD1B54A32D192ED03ull; }
constexpr int TAIL_GROUP = 64;     // workgroups per first-level group (= rows per block of the two-stage finalize)
// Distance between two slots of the L-BFGS ring (S and Y: one array of slots each), in doubles: the vector length rounded up to
// whole 128-B lines, so that every slot starts on a line like slot 0 does — with a stride of exactly n every slot of a ring whose
// n is not a multiple of 16 would have its wave accesses straddle lines (the effect described below, on 20 of 26 streams).
#ifdef CGO_RTC
__device__ inline size_t ring_ld(long long n) { return ((size_t)n + 15) & ~(size_t)15; }
#else
__host__ __device__ inline size_t ring_ld(long long n) { return ((size_t)n + 15) & ~(size_t)15; }
#endif
// Contiguous chunk of a pure-HBM (BIG) launch, in pairs of doubles per workgroup: a whole number of 128-B lines (8 pairs), so that
// every 1-KB wave access (64 lanes × 16 B) of every stream covers exactly eight lines.  With the plain ceiling a chunk starts
// wherever n / grid falls: at n = 1e7 (1 221 pairs per workgroup) each wave access straddled nine lines and the one-pass L-BFGS
// launch read 22.7 vectors where it needs 21 (PMC FETCH_SIZE) — 394–406 µs against 356–366 µs aligned; the accept + dir + trial
// launch at n = 7e7 took 632 µs against 538–547 µs.  n = 1e8 and 5e7 happened to be aligned already (12 208 / 6 104 pairs).
// Coarser alignment (16, 64 pairs) is no better and at n = 1e7 slightly worse (same box, alternating:
// profiles/r04_chunk_alignment.txt).
__device__ inline long long big_chunk_pairs(long long n2, unsigned int grid) {
    const long long per = (n2 + (long long)grid - 1) / (long long)grid;
    return (per + 7) & ~7LL;
}

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Workgroup partial sums → one row of P.partials (summed later by k_finalize).  Step-major: the NS cross-lane moves of a
// tree step are independent, so their ds_bpermute latencies overlap (slot-major order serialises 6·NS round trips).
__device__ inline void store_partials(double (&acc)[NS], const KParams &P) {
    __shared__ double sm[BLOCK / 64][NS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[s] += __shfl_down(acc[s], off, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < NS; ++s) sm[wave][s] = acc[s];
    }
    __syncthreads();
    if (tid < NS)
        P.partials[(size_t)blockIdx.x * NS + tid] = (sm[0][tid] + sm[1][tid]) + (sm[2][tid] + sm[3][tid]);
}

// One workgroup sums the partial rows in a fixed order.  The [rows][N] block is read FLAT — lane t
// owns slot t % N of rows t/N, t/N + G, … (G = THREADS/N row groups) — so every wavefront load is
// one contiguous 512-B run; a row-per-lane mapping (N strided 8-B loads per row) measured
// 8.5 µs (N = 10) and 41 µs (N = 24) at 4096 rows, this one ≈ 3 µs.
// With host_out != nullptr the sums are also published straight into pinned host memory
// followed by a system-scope release of `seq`, which the host spins on: no D2H copy, no
// stream synchronise on the per-trial latency path.
// One workgroup is limited to ≈ 25 GB/s (a single CU's latency-bound load stream): 786 KB of
// rows took 37 µs.  Large row blocks are therefore reduced in two stages — gridDim.x workgroups
// each sum `rows` consecutive rows into row blockIdx.x of `out`, then one workgroup sums those.
// G = how many interleaved row groups the N slots are summed in: part of the summation ORDER.  The k_cg family fixes it
// at BLOCK / N whatever kernel does the summing (a finalize launch or the launch's own last workgroup — finish_tail in
// cgo_kernels_cg.hip.hpp), so that both give the same bits.
template <int N, int THREADS, int G = THREADS / N>
__global__ __launch_bounds__(THREADS) void k_finalize_t(const double *partials_all, int rows_per_block, int rows_total,
                                                        double *out_all, double *host_out,
                                                        unsigned long long *host_seq, unsigned long long seq) {
    static_assert(G * N <= THREADS, "row groups need G·N lanes");
    __shared__ double sm[G][N];
    const int tid = threadIdx.x;
    const long long first = (long long)blockIdx.x * rows_per_block;
    long long rows = rows_total - first;
    if (rows > rows_per_block) rows = rows_per_block;
    if (rows < 0) rows = 0;
    const double *partials = partials_all + first * N;
    double *out = out_all + (size_t)blockIdx.x * N;
    if (tid < G * N) {
        double t = 0.0;
        const long long total = rows * N;
        // eight loads in flight per lane, added in index order (a dependent load per add made a 64-row block of 56-slot
        // rows 6.1 µs with 224 lanes against 4.2 µs with 728; + 0.0 for the slots past the end changes nothing: t starts at + 0.0)
        constexpr int U = 8;
        for (long long i = tid; i < total; i += (long long)U * G * N) {
            double v[U];
#pragma unroll
            for (int k = 0; k < U; ++k) { const long long j = i + (long long)k * G * N; v[k] = (j < total) ? partials[j] : 0.0; }
#pragma unroll
            for (int k = 0; k < U; ++k) t += v[k];
        }
        sm[tid / N][tid % N] = t;
    }
    __syncthreads();
    if (tid < N) {
        double v = 0.0;
#pragma unroll
        for (int g = 0; g < G; ++g) v += sm[g][tid];
        out[tid] = v;
        if (host_out) {
            host_out[tid] = v;
            __threadfence_system();
        }
    }
    if (host_out) {
        __syncthreads();
        if (tid == 0) __hip_atomic_store(host_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}


// Multi-rank contexts: after the all-gather, copy the [world][NS] block into pinned host memory
// and release the sequence word — replaces hipMemcpyAsync + hipStreamSynchronize on the
// per-launch latency path.
static __global__ void k_publish(const double *src, int count, double *host_out, unsigned long long *host_seq,
                          unsigned long long seq) {
    for (int i = threadIdx.x; i < count; i += blockDim.x) host_out[i] = src[i];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(host_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- the fused body ---------------------------------------------------------
// (which vectors a MODE loads: m_reads_x / _u / _g / _gt and m_evaluates, cgo_modes.hpp)
template <class Obj> struct Lanes { d2 x, u, g, gt; PV<Obj> p; };

template <bool NT> __device__ inline d2 ldg2(const double *base, long long i) {
    const d2 *q = reinterpret_cast<const d2 *>(base) + i;
    if (NT) return __builtin_nontemporal_load(q);
    return *q;
}
template <bool NT> __device__ inline void stg2(double *base, long long i, d2 v) {
    d2 *q = reinterpret_cast<d2 *>(base) + i;
    if (NT) __builtin_nontemporal_store(v, q);
    else *q = v;
}

// every parameter slot of the objective at pair i / element i (zero where it has none), with the policy of the launch's other streams
template <class Obj, bool NT, class A> __device__ inline PV<Obj> pv_load(const A &P, long long i) {
    constexpr int K = obj_nparams<Obj>();
    PV<Obj> r;
    r.v[0] = d2{0.0, 0.0};
    if constexpr (K > 0) r.v[0] = ldg2<NT>(param_slot<0>(P), i);
    if constexpr (K > 1) r.v[1] = ldg2<NT>(param_slot<1>(P), i);
    if constexpr (K > 2) r.v[2] = ldg2<NT>(param_slot<2>(P), i);
    if constexpr (K > 3) r.v[3] = ldg2<NT>(param_slot<3>(P), i);
    return r;
}
template <class Obj, class A> __device__ inline PS<Obj> ps_load(const A &P, long long i) {
    constexpr int K = obj_nparams<Obj>();
    PS<Obj> r;
    r.v[0] = 0.0;
    if constexpr (K > 0) r.v[0] = param_slot<0>(P)[i];
    if constexpr (K > 1) r.v[1] = param_slot<1>(P)[i];
    if constexpr (K > 2) r.v[2] = param_slot<2>(P)[i];
    if constexpr (K > 3) r.v[3] = param_slot<3>(P)[i];
    return r;
}

template <class Obj, int MODE, bool NT>
__device__ inline void load2(const KParams &P, long long i, Lanes<Obj> &v) {
    if (m_reads_x(MODE)) v.x = ldg2<NT>(P.x, i);
    if (m_reads_u(MODE)) v.u = ldg2<NT>(P.u, i);
    if (m_reads_g(MODE)) v.g = ldg2<NT>(P.g, i);
    if (m_reads_gt(MODE)) v.gt = ldg2<NT>(P.gt, i);
    if (m_evaluates(MODE) && obj_nparams<Obj>() > 0) v.p = pv_load<Obj, NT>(P, i);
}

template <class Obj, int MODE, bool NT>
__device__ inline void body2(const KParams &P, long long i, Lanes<Obj> &v, double (&acc)[NS]) {
    if (MODE & M_ACCEPT) {
        v.x.x = v.x.x + P.a_acc * v.u.x;
        v.x.y = v.x.y + P.a_acc * v.u.y;
        stg2<NT>(P.x, i, v.x);
    }
    if (MODE & (M_DIR | M_RESET)) {
        d2 un;
        if (MODE & M_DIR) {
            un.x = -v.g.x + P.beta * v.u.x;
            un.y = -v.g.y + P.beta * v.u.y;
        } else {
            un.x = -v.g.x;
            un.y = -v.g.y;
        }
        acc[S_GU] = dsum(acc[S_GU], v.g.x, un.x);
        acc[S_GU] = dsum(acc[S_GU], v.g.y, un.y);
        acc[S_UU] = dsum(acc[S_UU], un.x, un.x);
        acc[S_UU] = dsum(acc[S_UU], un.y, un.y);
        stg2<NT>(P.u, i, un);
        v.u = un;
    }
    if (MODE & M_TRIAL) {
        d2 xp, gt;
        xp.x = v.x.x + P.a_trial * v.u.x;
        xp.y = v.x.y + P.a_trial * v.u.y;
        obj_eval2<Obj>(xp, v.p, P.s0, acc[S_F], gt);
        stg2<NT>(P.gt, i, gt);
        acc[S_GTU] = dsum(acc[S_GTU], gt.x, v.u.x);
        acc[S_GTU] = dsum(acc[S_GTU], gt.y, v.u.y);
        acc[S_GTGT] = dsum(acc[S_GTGT], gt.x, gt.x);
        acc[S_GTGT] = dsum(acc[S_GTGT], gt.y, gt.y);
        if (MODE & M_BETA) {
            const double y0 = gt.x - v.g.x, y1 = gt.y - v.g.y;
            acc[S_GTG] = dsum(acc[S_GTG], gt.x, v.g.x);
            acc[S_GTG] = dsum(acc[S_GTG], gt.y, v.g.y);
            acc[S_YY] = dsum(acc[S_YY], y0, y0);
            acc[S_YY] = dsum(acc[S_YY], y1, y1);
            acc[S_UY] = dsum(acc[S_UY], v.u.x, y0);
            acc[S_UY] = dsum(acc[S_UY], v.u.y, y1);
            acc[S_YGT] = dsum(acc[S_YGT], y0, gt.x);
            acc[S_YGT] = dsum(acc[S_YGT], y1, gt.y);
        }
    }
    if (MODE & M_INIT) {
        d2 gt, un;
        obj_eval2<Obj>(v.x, v.p, P.s0, acc[S_F], gt);
        un.x = -gt.x;
        un.y = -gt.y;
        stg2<NT>(P.gt, i, gt);
        stg2<NT>(P.u, i, un);
        acc[S_GTGT] = dsum(acc[S_GTGT], gt.x, gt.x);
        acc[S_GTGT] = dsum(acc[S_GTGT], gt.y, gt.y);
    }
    if (MODE & M_UPG) {
        const double t0 = v.u.x + v.g.x, t1 = v.u.y + v.g.y;
        acc[S_UU] = dsum(acc[S_UU], t0, t0);
        acc[S_UU] = dsum(acc[S_UU], t1, t1);
    }
    if (MODE & M_BETAONLY) {
        const double y0 = v.gt.x - v.g.x, y1 = v.gt.y - v.g.y;
        acc[S_GTU] = dsum(acc[S_GTU], v.gt.x, v.u.x);   acc[S_GTU] = dsum(acc[S_GTU], v.gt.y, v.u.y);
        acc[S_GTGT] = dsum(acc[S_GTGT], v.gt.x, v.gt.x); acc[S_GTGT] = dsum(acc[S_GTGT], v.gt.y, v.gt.y);
        acc[S_GTG] = dsum(acc[S_GTG], v.gt.x, v.g.x);   acc[S_GTG] = dsum(acc[S_GTG], v.gt.y, v.g.y);
        acc[S_YY] = dsum(acc[S_YY], y0, y0);           acc[S_YY] = dsum(acc[S_YY], y1, y1);
        acc[S_UY] = dsum(acc[S_UY], v.u.x, y0);        acc[S_UY] = dsum(acc[S_UY], v.u.y, y1);
        acc[S_YGT] = dsum(acc[S_YGT], y0, v.gt.x);      acc[S_YGT] = dsum(acc[S_YGT], y1, v.gt.y);
        acc[S_GG] = dsum(acc[S_GG], v.g.x, v.g.x);     acc[S_GG] = dsum(acc[S_GG], v.g.y, v.g.y);
        acc[S_GU] = dsum(acc[S_GU], v.g.x, v.u.x);     acc[S_GU] = dsum(acc[S_GU], v.g.y, v.u.y);
        acc[S_UU] = dsum(acc[S_UU], v.u.x, v.u.x);     acc[S_UU] = dsum(acc[S_UU], v.u.y, v.u.y);
    }
}

// odd tail element (never taken for pair-only objectives: host validates n even)
template <class Obj, int MODE>
__device__ inline void body1(const KParams &P, long long i, double (&acc)[NS]) {
    double x = m_reads_x(MODE) ? P.x[i] : 0.0;
    double u = m_reads_u(MODE) ? P.u[i] : 0.0;
    const double g = m_reads_g(MODE) ? P.g[i] : 0.0;
    PS<Obj> p;
    p.v[0] = 0.0;
    if (m_evaluates(MODE) && obj_nparams<Obj>() > 0) p = ps_load<Obj>(P, i);
    if (MODE & M_ACCEPT) { x = x + P.a_acc * u; P.x[i] = x; }
    if (MODE & (M_DIR | M_RESET)) {
        const double un = (MODE & M_DIR) ? (-g + P.beta * u) : -g;
        acc[S_GU] = dsum(acc[S_GU], g, un);
        acc[S_UU] = dsum(acc[S_UU], un, un);
        P.u[i] = un;
        u = un;
    }
    if (MODE & M_TRIAL) {
        const double xp = x + P.a_trial * u;
        double gt;
        obj_eval1<Obj>(xp, p, P.s0, acc[S_F], gt);
        P.gt[i] = gt;
        acc[S_GTU] = dsum(acc[S_GTU], gt, u);
        acc[S_GTGT] = dsum(acc[S_GTGT], gt, gt);
        if (MODE & M_BETA) {
            const double y = gt - g;
            acc[S_GTG] = dsum(acc[S_GTG], gt, g); acc[S_YY] = dsum(acc[S_YY], y, y); acc[S_UY] = dsum(acc[S_UY], u, y); acc[S_YGT] = dsum(acc[S_YGT], y, gt);
        }
    }
    if (MODE & M_INIT) {
        double gt;
        obj_eval1<Obj>(x, p, P.s0, acc[S_F], gt);
        P.gt[i] = gt;
        P.u[i] = -gt;
        acc[S_GTGT] = dsum(acc[S_GTGT], gt, gt);
    }
    if (MODE & M_UPG) { const double t = u + g; acc[S_UU] = dsum(acc[S_UU], t, t); }
    if (MODE & M_BETAONLY) {
        const double gt = P.gt[i], y = gt - g;
        acc[S_GTU] = dsum(acc[S_GTU], gt, u); acc[S_GTGT] = dsum(acc[S_GTGT], gt, gt); acc[S_GTG] = dsum(acc[S_GTG], gt, g); acc[S_YY] = dsum(acc[S_YY], y, y);
        acc[S_UY] = dsum(acc[S_UY], u, y); acc[S_YGT] = dsum(acc[S_YGT], y, gt); acc[S_GG] = dsum(acc[S_GG], g, g);
        acc[S_GU] = dsum(acc[S_GU], g, u); acc[S_UU] = dsum(acc[S_UU], u, u);
    }
}

template <class Obj, int MODE, bool BIG>
__global__ __launch_bounds__(BLOCK) void k_fused(const KParams P) {
    double acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = 0.0;
    const long long n2 = P.n >> 1;
    if (BIG) {  // contiguous chunk per workgroup, streaming (non-temporal) accesses
        const long long per = big_chunk_pairs(n2, gridDim.x);
        const long long lo = per * blockIdx.x;
        const long long hi = (lo + per < n2) ? lo + per : n2;
        long long i = lo + threadIdx.x;
        for (; i + BLOCK < hi; i += 2 * BLOCK) {
            Lanes<Obj> a, b;
            load2<Obj, MODE, true>(P, i, a);
            load2<Obj, MODE, true>(P, i + BLOCK, b);
            body2<Obj, MODE, true>(P, i, a, acc);
            body2<Obj, MODE, true>(P, i + BLOCK, b, acc);
        }
        if (i < hi) {
            Lanes<Obj> a;
            load2<Obj, MODE, true>(P, i, a);
            body2<Obj, MODE, true>(P, i, a, acc);
        }
    } else {    // grid-stride
        const long long T = (long long)gridDim.x * BLOCK;
        long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
        for (; i + T < n2; i += 2 * T) {
            Lanes<Obj> a, b;
            load2<Obj, MODE, false>(P, i, a);
            load2<Obj, MODE, false>(P, i + T, b);
            body2<Obj, MODE, false>(P, i, a, acc);
            body2<Obj, MODE, false>(P, i + T, b, acc);
        }
        if (i < n2) {
            Lanes<Obj> a;
            load2<Obj, MODE, false>(P, i, a);
            body2<Obj, MODE, false>(P, i, a, acc);
        }
    }
    if ((P.n & 1) && blockIdx.x == 0 && threadIdx.x == 0) body1<Obj, MODE>(P, P.n - 1, acc);
    // host-closure objectives: this rank's f = fdf!(g, xp) was computed on the host; it joins the launch's sums here
    // so that it is reduced across ranks like every other scalar (a_trial is unused by this mode)
    if (MODE == M_BETAONLY && blockIdx.x == 0 && threadIdx.x == 0) acc[S_F] += P.a_trial;
    store_partials(acc, P);
}

// evalϕdϕ!'s trial point for a host closure (cg_utils.jl:14-16): out = x + a·u, unfused; u == nullptr → out = x.
// `out` is pinned host memory: the stores go straight over PCIe.
static __global__ __launch_bounds__(BLOCK) void k_trial_point(const double *x, const double *u, double a, double *out, long long n) {
    const long long T = (long long)gridDim.x * BLOCK;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += T)
        out[i] = u ? x[i] + a * u[i] : x[i];
}

// ---- the accept+dir+trial read/write mix with (next to) no arithmetic -------------------------------------------
// R x, u, D / W x, u in place, 16 B per lane, the BIG streaming policy of the engine (contiguous chunk per workgroup,
// non-temporal accesses, two groups per lane per trip).  What this delivers on the box at hand is the ceiling the
// engine's dominant launch is priced against beside the 8 TB/s pin peak (bench.py: roofline.frac_of_measured_mix);
// MI355X boxes differ by ±8 % on exactly this mix (scripts/tune/rw_mix.hip explores the other policies).
// BIG: the pure-HBM policy (contiguous chunk per workgroup, non-temporal accesses); otherwise the grid-stride, default-cache-
// policy form of the launches that still see part of their working set in the Infinity Cache (the 8-GPU shard of config 5).
template <bool HAS_D, bool BIG = true>
__global__ __launch_bounds__(BLOCK) void k_stream_mix(double *x, double *u, const double *d, long long n, double a, double b) {
    const long long n2 = n >> 1;
    long long i, hi, step;
    if (BIG) {
        const long long per = big_chunk_pairs(n2, gridDim.x);
        hi = (per * blockIdx.x + per < n2) ? per * blockIdx.x + per : n2;
        i = per * blockIdx.x + threadIdx.x;
        step = BLOCK;
    } else {
        i = (long long)blockIdx.x * BLOCK + threadIdx.x;
        hi = n2;
        step = (long long)gridDim.x * BLOCK;
    }
    auto body = [&](long long j, d2 xv, d2 uv, d2 dv) {
        d2 xn, un;
        xn.x = xv.x + a * uv.x; xn.y = xv.y + a * uv.y;
        un.x = b * uv.x - (dv.x * xn.x) * 1e-9; un.y = b * uv.y - (dv.y * xn.y) * 1e-9;
        stg2<BIG>(x, j, xn); stg2<BIG>(u, j, un);
    };
    const d2 one = d2{1.0, 1.0};
    for (; i + step < hi; i += 2 * step) {
        const d2 xa = ldg2<BIG>(x, i), xb = ldg2<BIG>(x, i + step);
        const d2 ua = ldg2<BIG>(u, i), ub = ldg2<BIG>(u, i + step);
        const d2 da = HAS_D ? ldg2<BIG>(d, i) : one, db = HAS_D ? ldg2<BIG>(d, i + step) : one;
        body(i, xa, ua, da); body(i + step, xb, ub, db);
    }
    if (i < hi) body(i, ldg2<BIG>(x, i), ldg2<BIG>(u, i), HAS_D ? ldg2<BIG>(d, i) : one);
}

// ---- LinearAlgebra.norm, rare path ---------------------------------------------------------
// PASS 0: row = [max|v_i|, #NaN];  PASS 1: row = [Σ (v_i/scale)²].  Rows are merged by
// k_finalize_maxsum (slot 0: max in pass 0 / sum in pass 1; slot 1: sum).
// w != nullptr: the vector is the difference v − w (y = g⁺ − g of getβ, never stored anywhere).
template <int PASS>
__global__ __launch_bounds__(BLOCK) void k_scaled_norm(const double *v, const double *w, long long n, double scale, double *partials) {
    __shared__ double sm[BLOCK / 64][2];
    double a0 = 0.0, a1 = 0.0;
    const long long T = (long long)gridDim.x * BLOCK;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += T) {
        const double x = w ? v[i] - w[i] : v[i];
        if (PASS == 0) { const double ax = fabs(x); if (ax > a0) a0 = ax; if (x != x) a1 += 1.0; }
        else { const double r = x / scale; a0 += r * r; }
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o0 = __shfl_down(a0, off, 64), o1 = __shfl_down(a1, off, 64);
        a0 = (PASS == 0) ? (o0 > a0 ? o0 : a0) : a0 + o0;
        a1 += o1;
    }
    if (lane == 0) { sm[wave][0] = a0; sm[wave][1] = a1; }
    __syncthreads();
    if (tid == 0) {
        double r0 = sm[0][0], r1 = sm[0][1];
        for (int w = 1; w < BLOCK / 64; ++w) {
            r0 = (PASS == 0) ? (sm[w][0] > r0 ? sm[w][0] : r0) : r0 + sm[w][0];
            r1 += sm[w][1];
        }
        double *row = partials + (size_t)blockIdx.x * NS;
        row[0] = r0; row[1] = r1;
#pragma unroll
        for (int s = 2; s < NS; ++s) row[s] = 0.0;
    }
}

template <int PASS>
__global__ void k_finalize_maxsum(const double *partials, int rows, double *out, double *host_out,
                                  unsigned long long *host_seq, unsigned long long seq) {
    if (threadIdx.x != 0) return;  // ≤ 1024 rows, rare path: one lane, fixed order
    double r0 = 0.0, r1 = 0.0;
    for (int b = 0; b < rows; ++b) {
        const double v = partials[(size_t)b * NS];
        r0 = (PASS == 0) ? (v > r0 ? v : r0) : r0 + v;
        r1 += partials[(size_t)b * NS + 1];
    }
    for (int s = 0; s < NS; ++s) { const double v = (s == 0) ? r0 : (s == 1 ? r1 : 0.0); out[s] = v; if (host_out) host_out[s] = v; }
    if (host_out) {
        __threadfence_system();
        __hip_atomic_store(host_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- L-BFGS (new QNβConfig; dispatch contract src/qn_flavours.jl:5-48) ------------------
// State update after an accepted step a* (the QN counterpart of getβ + the copies of
// optim.jl:130-140):  s = a*·u ; y = g⁺ − g ; x ← x + a*·u ; Σ s·y, Σ y·y, Σ s·g⁺.
// R x,u,g,g⁺ ; W x,s,y = 56 B/elt.
struct PushParams {
    double *x; const double *u; const double *g; const double *gt;
    double *s; double *y;
    long long n;
    double a;    // step of the accepted trial point: x ← x + a·u
    double a_s;  // step defining the curvature pair: s = a_s·u (= a except under Backtracking)
    double *partials;
};
enum PushSlot : int { PS_SY = 0, PS_YY = 1, PS_SGT = 2 };

template <bool BIG>
__global__ __launch_bounds__(BLOCK) void k_lbfgs_push(const PushParams P) {
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
    const long long n2 = P.n >> 1;
    long long i, hi, step;
    if (BIG) {
        const long long per = big_chunk_pairs(n2, gridDim.x);
        i = per * blockIdx.x + threadIdx.x;
        hi = (per * blockIdx.x + per < n2) ? per * blockIdx.x + per : n2;
        step = BLOCK;
    } else {
        i = (long long)blockIdx.x * BLOCK + threadIdx.x;
        hi = n2;
        step = (long long)gridDim.x * BLOCK;
    }
    for (; i < hi; i += step) {
        d2 x = ldg2<BIG>(P.x, i);
        const d2 u = ldg2<BIG>(P.u, i), g = ldg2<BIG>(P.g, i), gt = ldg2<BIG>(P.gt, i);
        d2 s, y;
        s.x = P.a_s * u.x; s.y = P.a_s * u.y;
        y.x = gt.x - g.x; y.y = gt.y - g.y;
        x.x = x.x + P.a * u.x; x.y = x.y + P.a * u.y;
        stg2<BIG>(P.x, i, x);
        stg2<BIG>(P.s, i, s);
        stg2<BIG>(P.y, i, y);
        acc[PS_SY] = dsum(acc[PS_SY], s.x, y.x);   acc[PS_SY] = dsum(acc[PS_SY], s.y, y.y);
        acc[PS_YY] = dsum(acc[PS_YY], y.x, y.x);   acc[PS_YY] = dsum(acc[PS_YY], y.y, y.y);
        acc[PS_SGT] = dsum(acc[PS_SGT], s.x, gt.x); acc[PS_SGT] = dsum(acc[PS_SGT], s.y, gt.y);
    }
    if ((P.n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const long long j = P.n - 1;
        const double u = P.u[j], s = P.a_s * u, y = P.gt[j] - P.g[j];
        P.x[j] = P.x[j] + P.a * u;
        P.s[j] = s; P.y[j] = y;
        acc[PS_SY] = dsum(acc[PS_SY], s, y); acc[PS_YY] = dsum(acc[PS_YY], y, y); acc[PS_SGT] = dsum(acc[PS_SGT], s, P.gt[j]);
    }
    KParams Q; Q.partials = P.partials;
    store_partials(acc, Q);
}

// ---- "vector-free" L-BFGS: every inner product of the two-loop recursion from ONE pass ------
// Fused with the state update of k_lbfgs_push.  With the candidate pair (sn, yn), the new
// gradient g⁺ and the `count` stored pairs j:   Σ sn·yn, yn·yn, sn·g⁺, yn·g⁺  and per j
// Σ s_j·g⁺, y_j·g⁺, s_j·yn, y_j·sn, y_j·yn.   The host keeps the Gram blocks (S·Y, Y·Y, S·g, Y·g),
// runs the recursion on scalars and asks for ONE linear-combination pass (k_lbfgs_combine).
// 2 launches and ≈ (4c+9)·8 B/elt per iteration instead of 2c+2 launches and (8c+7)·8 B/elt.
constexpr int GRAM_MAXC = 12;  // 4 + 5·12 = 64 sums
constexpr int NG = 64;
struct GramPushParams {
    double *x; const double *u; const double *g; const double *gt;
    double *S; double *Y;        // ring base, slot stride = n
    long long n;
    double a, a_s;
    int slot, count;
    int prev[GRAM_MAXC];
    double *partials;
};

// Wave-split form.  54 sums per lane (m = 10) is 108 accumulator VGPRs: with the 24 streams' data in
// flight on top, the first version ran at 2 waves/SIMD with its loads serialised behind their uses
// (533 µs, 4.06 TB/s at n = 1e7).  Here the four waves of a workgroup walk the SAME 64 element groups
// per trip and split the stored pairs between them (wave w owns pairs j ≡ w mod 4: ≤ 3 pairs, 15 sums);
// wave 0 also owns the state update and the four sums of the new pair.  u, g, g⁺ are read by all four
// waves (cache hits, default policy); S_j, Y_j stream through once (non-temporal).
constexpr int GRAM_PER_WAVE = (GRAM_MAXC + 3) / 4;

template <bool BIG>
__global__ __launch_bounds__(BLOCK) void k_lbfgs_push_gram(const GramPushParams P) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (scalar: owned pointers in SGPRs, wave tests are scalar branches)
    double base[4] = {0.0, 0.0, 0.0, 0.0};
    double acc[GRAM_PER_WAVE][5];
#pragma unroll
    for (int l = 0; l < GRAM_PER_WAVE; ++l)
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[l][q] = 0.0;
    const long long n2 = P.n >> 1;
    long long i, hi, step;
    if (BIG) {
        const long long per = big_chunk_pairs(n2, gridDim.x);
        i = per * blockIdx.x + lane;
        hi = (per * blockIdx.x + per < n2) ? per * blockIdx.x + per : n2;
        step = 64;
    } else {
        i = (long long)blockIdx.x * 64 + lane;
        hi = n2;
        step = (long long)gridDim.x * 64;
    }
    double *sn = P.S + (size_t)P.slot * ring_ld(P.n), *yn = P.Y + (size_t)P.slot * ring_ld(P.n);
    const double *Sj[GRAM_PER_WAVE], *Yj[GRAM_PER_WAVE];
    bool on[GRAM_PER_WAVE];
#pragma unroll
    for (int l = 0; l < GRAM_PER_WAVE; ++l) {
        const int j = l * 4 + wave;
        on[l] = j < P.count;
        const int slot = on[l] ? P.prev[j] : 0;
        Sj[l] = P.S + (size_t)slot * ring_ld(P.n);
        Yj[l] = P.Y + (size_t)slot * ring_ld(P.n);
    }
    for (; i < hi; i += step) {
        const d2 u = ldg2<false>(P.u, i), g = ldg2<false>(P.g, i), gt = ldg2<false>(P.gt, i);
        d2 sj[GRAM_PER_WAVE], yj[GRAM_PER_WAVE];
#pragma unroll
        for (int l = 0; l < GRAM_PER_WAVE; ++l)
            if (on[l]) { sj[l] = ldg2<BIG>(Sj[l], i); yj[l] = ldg2<BIG>(Yj[l], i); }
        d2 s, y;
        s.x = P.a_s * u.x; s.y = P.a_s * u.y;
        y.x = gt.x - g.x; y.y = gt.y - g.y;
        if (wave == 0) {
            d2 x = ldg2<BIG>(P.x, i);
            x.x = x.x + P.a * u.x; x.y = x.y + P.a * u.y;
            stg2<BIG>(P.x, i, x);
            stg2<BIG>(sn, i, s);
            stg2<BIG>(yn, i, y);
            base[0] = dsum(base[0], s.x, y.x);  base[0] = dsum(base[0], s.y, y.y);
            base[1] = dsum(base[1], y.x, y.x);  base[1] = dsum(base[1], y.y, y.y);
            base[2] = dsum(base[2], s.x, gt.x); base[2] = dsum(base[2], s.y, gt.y);
            base[3] = dsum(base[3], y.x, gt.x); base[3] = dsum(base[3], y.y, gt.y);
        }
#pragma unroll
        for (int l = 0; l < GRAM_PER_WAVE; ++l) {
            if (on[l]) {
                acc[l][0] = dsum(acc[l][0], sj[l].x, gt.x); acc[l][0] = dsum(acc[l][0], sj[l].y, gt.y);
                acc[l][1] = dsum(acc[l][1], yj[l].x, gt.x); acc[l][1] = dsum(acc[l][1], yj[l].y, gt.y);
                acc[l][2] = dsum(acc[l][2], sj[l].x, y.x);  acc[l][2] = dsum(acc[l][2], sj[l].y, y.y);
                acc[l][3] = dsum(acc[l][3], yj[l].x, s.x);  acc[l][3] = dsum(acc[l][3], yj[l].y, s.y);
                acc[l][4] = dsum(acc[l][4], yj[l].x, y.x);  acc[l][4] = dsum(acc[l][4], yj[l].y, y.y);
            }
        }
    }
    if ((P.n & 1) && blockIdx.x == 0 && lane == 0) {  // odd tail element: lane 0 of every wave, its own pairs
        const long long e = P.n - 1;
        const double u = P.u[e], gt = P.gt[e], s = P.a_s * u, y = gt - P.g[e];
        if (wave == 0) {
            P.x[e] = P.x[e] + P.a * u;
            sn[e] = s; yn[e] = y;
            base[0] = dsum(base[0], s, y); base[1] = dsum(base[1], y, y); base[2] = dsum(base[2], s, gt); base[3] = dsum(base[3], y, gt);
        }
#pragma unroll
        for (int l = 0; l < GRAM_PER_WAVE; ++l) {
            if (on[l]) {
                const double sje = Sj[l][e], yje = Yj[l][e];
                acc[l][0] = dsum(acc[l][0], sje, gt); acc[l][1] = dsum(acc[l][1], yje, gt); acc[l][2] = dsum(acc[l][2], sje, y);
                acc[l][3] = dsum(acc[l][3], yje, s);  acc[l][4] = dsum(acc[l][4], yje, y);
            }
        }
    }
    // every slot is owned by exactly one wave: wavefront tree → the row directly
    double *row = P.partials + (size_t)blockIdx.x * NG;
    if (wave == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double v = wave_sum(base[q]);
            if (lane == 0) row[q] = v;
        }
    }
#pragma unroll
    for (int l = 0; l < GRAM_PER_WAVE; ++l) {
        const int j = l * 4 + wave;
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const double v = wave_sum(acc[l][q]);
            if (lane == 0 && j < GRAM_MAXC) row[4 + 5 * j + q] = on[l] ? v : 0.0;
        }
    }
}

// The log-sum-exp objective's push forms g⁺ of the accepted trial itself (k_lbfgs_push_gram_lse, cgo_kernels_lse.hip.hpp):
// Σ g⁺² travels in row slot GRAM_GTGT — pair 11's last slot, free while count ≤ GRAM_MAXC_LSE.
constexpr int GRAM_GTGT = NG - 1;
constexpr int GRAM_MAXC_LSE = GRAM_MAXC - 1;
struct GramLseParams {
    double *xo;      // x + a·u goes here (never P.x): optim.jl:108-121 must be able to return the last good iterate
    double *gt_out;  // g⁺ goes here
    double M, S, lambda;
};

// u = cg·g + Σ_j ( cy_j·y_j + cs_j·s_j ) ; Σ g·u, Σ u·u.   R g, 2c vectors ; W u.
struct GramDirParams {
    const double *g; double *u; const double *S; const double *Y;
    long long n;
    int count;
    int slots[GRAM_MAXC];
    double cy[GRAM_MAXC], cs[GRAM_MAXC];
    double cg;
    double *partials;
};

// One pair of the combination (and, for a two-phase objective, of the first trial's statistics — CombineTrial below).
template <bool BIG>
__device__ inline d2 lbfgs_combine_pair(const GramDirParams &P, long long i, d2 g) {
    d2 yv[GRAM_MAXC], sv[GRAM_MAXC];
#pragma unroll
    for (int j = 0; j < GRAM_MAXC; ++j) {  // issue every load first: 2c+1 independent 16-B loads in flight
        if (j < P.count) {
            yv[j] = ldg2<BIG>(P.Y + (size_t)P.slots[j] * ring_ld(P.n), i);
            sv[j] = ldg2<BIG>(P.S + (size_t)P.slots[j] * ring_ld(P.n), i);
        }
    }
    d2 r;
    r.x = P.cg * g.x; r.y = P.cg * g.y;
#pragma unroll
    for (int j = 0; j < GRAM_MAXC; ++j) {
        if (j < P.count) {
            r.x = r.x + P.cy[j] * yv[j].x; r.y = r.y + P.cy[j] * yv[j].y;
            r.x = r.x + P.cs[j] * sv[j].x; r.y = r.y + P.cs[j] * sv[j].y;
        }
    }
    return r;
}
__device__ inline double lbfgs_combine_one(const GramDirParams &P, long long e, double g) {
    double r = P.cg * g;
    for (int j = 0; j < P.count; ++j) {
        r = r + P.cy[j] * P.Y[(size_t)P.slots[j] * ring_ld(P.n) + e];
        r = r + P.cs[j] * P.S[(size_t)P.slots[j] * ring_ld(P.n) + e];
    }
    return r;
}

template <bool BIG>
__global__ __launch_bounds__(BLOCK) void k_lbfgs_combine(const GramDirParams P) {
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
    const long long n2 = P.n >> 1;
    long long i, hi, step;
    if (BIG) {
        const long long per = big_chunk_pairs(n2, gridDim.x);
        i = per * blockIdx.x + threadIdx.x;
        hi = (per * blockIdx.x + per < n2) ? per * blockIdx.x + per : n2;
        step = BLOCK;
    } else {
        i = (long long)blockIdx.x * BLOCK + threadIdx.x;
        hi = n2;
        step = (long long)gridDim.x * BLOCK;
    }
    for (; i < hi; i += step) {
        const d2 g = ldg2<BIG>(P.g, i);
        const d2 r = lbfgs_combine_pair<BIG>(P, i, g);
        stg2<BIG>(P.u, i, r);
        acc[S_GU] = dsum(acc[S_GU], g.x, r.x); acc[S_GU] = dsum(acc[S_GU], g.y, r.y);
        acc[S_UU] = dsum(acc[S_UU], r.x, r.x); acc[S_UU] = dsum(acc[S_UU], r.y, r.y);
    }
    if ((P.n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const long long e = P.n - 1;
        const double g = P.g[e];
        const double r = lbfgs_combine_one(P, e, g);
        P.u[e] = r;
        acc[S_GU] = dsum(acc[S_GU], g, r); acc[S_UU] = dsum(acc[S_UU], r, r);
    }
    KParams Q; Q.partials = P.partials;
    store_partials(acc, Q);
}

// One step of the two-loop recursion (Nocedal & Wright Alg. 7.4), fused with the NEXT dot:
//   loop 1:  q ← q − α·v          α = ρ·dot_prev           (v = y_k)
//   loop 2:  r ← r + (α_k − ρ·dot_prev)·v                   (v = s_k)
//   last loop-1 step also scales r = γ·q ; the final loop-2 step writes u = −r, Σ g·u, Σ u·u.
// dot_prev is read from DEVICE memory (the sums k_finalize / the all-gather left there), so
// the 2m launches of one direction are enqueued back to back without a host round trip.
// R q,v,w ; W q = 32 B/elt per step.
struct LoopParams {
    const double *qin; double *qout; const double *v; const double *w;
    long long n;
    double rho, scale, dot_host;
    const double *dot_ptr;  // [dot_count][dot_stride] per-rank blocks (summed in rank order) or nullptr
    int dot_count, dot_stride, dot_slot;
    int mode;               // 0: loop 1, 1: loop 2, 2: dot only (no update)
    int final_step;         // write −r and the direction sums
    int apply_scale;        // multiply by `scale` after the update
    double *alpha; int k;   // α_k store (loop 1) / load (loop 2)
    double *partials;
};

template <bool BIG>
__global__ __launch_bounds__(BLOCK) void k_lbfgs_loop(const LoopParams P) {
    double dot = P.dot_host;
    if (P.dot_ptr) {
        dot = 0.0;
        for (int r = 0; r < P.dot_count; ++r) dot += P.dot_ptr[(size_t)r * P.dot_stride + P.dot_slot];
    }
    double coef = 0.0;
    if (P.mode == 0) {
        coef = P.rho * dot;  // α_k
        if (blockIdx.x == 0 && threadIdx.x == 0) P.alpha[P.k] = coef;
    } else if (P.mode == 1) {
        coef = P.alpha[P.k] - P.rho * dot;
    }
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
    const long long n2 = P.n >> 1;
    long long i, hi, step;
    if (BIG) {
        const long long per = big_chunk_pairs(n2, gridDim.x);
        i = per * blockIdx.x + threadIdx.x;
        hi = (per * blockIdx.x + per < n2) ? per * blockIdx.x + per : n2;
        step = BLOCK;
    } else {
        i = (long long)blockIdx.x * BLOCK + threadIdx.x;
        hi = n2;
        step = (long long)gridDim.x * BLOCK;
    }
    for (; i < hi; i += step) {
        d2 q = ldg2<BIG>(P.qin, i);
        const d2 w = ldg2<BIG>(P.w, i);
        if (P.mode != 2) {
            const d2 v = ldg2<BIG>(P.v, i);
            if (P.mode == 0) { q.x = q.x - coef * v.x; q.y = q.y - coef * v.y; }
            else             { q.x = q.x + coef * v.x; q.y = q.y + coef * v.y; }
            if (P.apply_scale) { q.x = P.scale * q.x; q.y = P.scale * q.y; }
            if (P.final_step) {
                q.x = -q.x; q.y = -q.y;
                acc[S_UU] = dsum(acc[S_UU], q.x, q.x); acc[S_UU] = dsum(acc[S_UU], q.y, q.y);
            }
            stg2<BIG>(P.qout, i, q);
        }
        acc[S_GU] = dsum(acc[S_GU], w.x, q.x); acc[S_GU] = dsum(acc[S_GU], w.y, q.y);  // next dot (or g·u on the final step)
    }
    if ((P.n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const long long j = P.n - 1;
        double q = P.qin[j];
        if (P.mode != 2) {
            q = (P.mode == 0) ? (q - coef * P.v[j]) : (q + coef * P.v[j]);
            if (P.apply_scale) q = P.scale * q;
            if (P.final_step) { q = -q; acc[S_UU] = dsum(acc[S_UU], q, q); }
            P.qout[j] = q;
        }
        acc[S_GU] = dsum(acc[S_GU], P.w[j], q);
    }
    KParams Q; Q.partials = P.partials;
    store_partials(acc, Q);
}

// ---- ONE pass over the ring per outer iteration (round 3) ------------------------------------------------------------
// The Gram form reads the 2c ring vectors twice per iteration: the push needs b·g⁺ for every stored vector b before the
// recursion's coefficients exist, the combination needs the coefficients.  But the first step of the next line search is
// known when the direction is formed (optim.jl:92) and is the step that gets accepted on all but a few iterations (config 4:
// 1.02 trials per iteration) — so the direction pass can ALSO leave every inner product the next push will need, taken at
// that first trial point xp = x + a₀·u.  For the log-sum-exp objective g⁺ = softmax(xp) + λ·xp is not known element by
// element before the pass has ended (it needs Σ), but with the statistics (M_r, S_r) of the CURRENT iterate as a fixed
// reference
//     e_i  = exp(xp_i − M_r)               S' = Σ e_i,  T' = Σ e_i·u_i  (plain sums: ϕ = M_r + log S' + ½λQ, dϕ = T'/S' + λR)
//     p_i  = e_i/S_r ,   g⁺_i = κ·p_i + λ·xp_i ,  κ = S_r/S'  (≈ 1)
//     y_i  = g⁺_i − g_i = ŷ_i + (κ − 1)·p_i ,  ŷ_i = (p_i + λ·xp_i) − g_i
// so with A_b = Σ b_i·ŷ_i and T_b = Σ b_i·p_i per stored vector b:  b·y = A_b + (κ − 1)·T_b — element-wise differences
// summed, no cancellation between two large sums — and b·g⁺ = b·g + b·y with b·g from the previous iteration.  Likewise
// y·y, s·y, y·g⁺, g⁺·g⁺ from six more sums (E0..E5 below).  If that trial is accepted, the push is a 56 B/element
// state update without sums (k_lbfgs_push_lite); if not, nothing is lost: the usual push runs on the accepted step.
// Per outer iteration: (2c + 3)·8 + 56 B/element and ONE host round trip, instead of (4c + 9)·8 + … and three.
// The fixed reference keeps the pass free of the running-max branch (and every slot of its row a plain sum); the host
// accepts the trial's statistics only while S' says the reference is still near the maximum (else: k_lse_stats, which
// takes the true maximum and becomes the next reference).
//
// Wave-split like k_lbfgs_push_gram: wave w owns the stored pairs j ≡ w (mod 4) — their loads, their share of the linear
// combination and their five sums each; the four partial combinations meet in LDS (one barrier per trip, two buffers on
// the trip's parity) and are added in wave order, so every wave holds the same u, xp, e, p.
// Row (NG = 64): [0] S' [1] T' [2] Q [3] R [4] Σĝ² · [5] g·u [6] u·u · [7..12] E0..E5 · [13 + 5j + q] pair j: s_j·ŷ, s_j·p, y_j·ŷ, y_j·p, y_j·u · [63] Σĝ·p,
// with ĝ = p + λ·xp (the gradient at the reference scaling: g⁺ = ĝ + (κ − 1)·p).  ‖g⁺‖² = Σĝ² + 2(κ − 1)·Σĝp + (κ − 1)²·Σp² is formed from
// THESE sums (round 4): expanded over Σp², Σp·xp, Σxp² it cancelled (‖p‖/‖g⁺‖)²-fold — the gradient norm in the trace, and the stop test
// that reads it, had lost ≈ 6 digits once ‖g‖ had fallen by 1e5 (found by the long-horizon comparison with the arbiter, config 4).
// ELEMENT-WISE objectives (separable quadratic, paired Rosenbrock) run the same pass with less algebra: g⁺ = ∇f(xp) is known
// in the pass, so y = g⁺ − g is exact there and every inner product is taken directly:
// Row: [0] f [1] g⁺·u [2] g⁺·g⁺ [3] y·g⁺ [4] u·y [5] g·u [6] u·u [7] y·y · [13 + 5j + q] pair j: s_j·g⁺, y_j·g⁺, s_j·y, y_j·y, y_j·u.
constexpr int SPEC_MAXC = 10;       // 13 + 5·10 = 63 slots
constexpr int SP_S = 0, SP_T = 1, SP_Q = 2, SP_R = 3, SP_GH2 = 4, SP_GU = 5, SP_UU = 6, SP_E0 = 7, SP_PAIR = 13, SP_GHP = 63;
constexpr int SE_F = 0, SE_GTU = 1, SE_GTGT = 2, SE_YGT = 3, SE_UY = 4, SE_YY = 7;
struct ObjLse { static constexpr bool kTwoPhase = true; static constexpr bool kParam = false; static constexpr bool kPairOnly = false; };
template <class Obj> struct SpecKind { static constexpr bool lse = false; };
template <> struct SpecKind<ObjLse> { static constexpr bool lse = true; };
struct SpecParams { double Mr, rSr, lambda; const double *p0, *p1, *p2, *p3; };   // log-sum-exp: reference maximum, 1/S_r, λ · element-wise: –, –, the objective's scalar, its parameter vector
// PUSH: the state update of the PREVIOUS iteration's accepted speculated trial rides in this pass instead of a launch of its
// own (k_lbfgs_push_lite): x ← x + a·u_old, g ← g⁺ (log-sum-exp: exp(x − M)/S + λ·x; element-wise: ∇f(x)), and the new pair
// s = a_s·u_old, y = g⁺ − g_old is FORMED in registers — written to its ring slot for the passes to come, used here by its
// owner (pair 0 = wave 0 when it joined the history: `new_in_list`) without being read.  Every wave forms x, g⁺ itself (≈ 35
// instructions per element, the pass is memory-bound).  R x, g, u_old, 2(c − 1) ring vectors · W x, g, u, s, y:
// (2c + 6)·8 B/element (+ 8 for a parameter vector) for the WHOLE iteration, and one launch.  x, g and u are updated in place:
// a trip's old values are consumed by every wave before the trip's barrier (explicit wait: a global load may otherwise
// still be in flight behind it) and written after it.
struct SpecPush { double *x, *g, *sn, *yn; double a, a_s, M, S; int new_in_list; };

template <class Obj, bool BIG, bool PUSH>
__global__ __launch_bounds__(BLOCK) void k_lbfgs_combine_spec(const GramDirParams P, const double *x, double a_trial, const SpecParams Q, const SpecPush U) {
    constexpr bool LSE = SpecKind<Obj>::lse;
    constexpr int W = BLOCK / 64, LPW = (SPEC_MAXC + W - 1) / W;
    __shared__ d2 pu[2][W][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (scalar: the owned pointers and coefficients live in SGPRs)
    const bool newp = PUSH && wave == 0 && U.new_in_list;   // this wave's pair l = 0 is the pair being formed
    const double *Sj[LPW], *Yj[LPW];
    double cy[LPW], cs[LPW];
    bool on[LPW];
    double acc[LPW][5];
#pragma unroll
    for (int l = 0; l < LPW; ++l) {
        const int j = l * W + wave;
        on[l] = j < P.count;
        const int slot = on[l] ? P.slots[j] : 0;
        Sj[l] = P.S + (size_t)slot * ring_ld(P.n);
        Yj[l] = P.Y + (size_t)slot * ring_ld(P.n);
        cy[l] = on[l] ? P.cy[j] : 0.0;
        cs[l] = on[l] ? P.cs[j] : 0.0;
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[l][q] = 0.0;
    }
    // designated sums — log-sum-exp: wave 0 g·u, u·u · wave 1 S', T', Q, R · wave 2 E0, E1, E2 · wave 3 E3, E4, E5
    //                   element-wise: wave 0 g·u, u·u · wave 1 f, g⁺·u, g⁺·g⁺, y·g⁺ · wave 2 u·y, y·y          (wave 0 also stores u)
    double d0 = 0.0, d1 = 0.0, d2s = 0.0, d3 = 0.0;
    auto elem_lse = [&](double xv, double g, double u, const double (&sv)[LPW], const double (&yv)[LPW]) {
        const double xp = xv + a_trial * u;
        const double e = exp(xp - Q.Mr);     // NaN input propagates; overflow → the host discards the speculation
        const double p = e * Q.rSr;
        const double gh = p + Q.lambda * xp;
        const double yh = gh - g;
        if (wave == 0) { d0 = dsum(d0, g, u); d1 = dsum(d1, u, u); d2s = dsum(d2s, gh, gh); d3 = dsum(d3, gh, p); }
        else if (wave == 1) { d0 += e; d1 = dsum(d1, e, u); d2s = dsum(d2s, xp, xp); d3 = dsum(d3, xp, u); }
        else if (wave == 2) { d0 = dsum(d0, yh, yh); d1 = dsum(d1, yh, p); d2s = dsum(d2s, p, p); }
        else { d0 = dsum(d0, u, yh); d1 = dsum(d1, p, xp); d2s = dsum(d2s, yh, xp); }
#pragma unroll
        for (int l = 0; l < LPW; ++l) {
            if (on[l]) {
                acc[l][0] = dsum(acc[l][0], sv[l], yh); acc[l][1] = dsum(acc[l][1], sv[l], p);
                acc[l][2] = dsum(acc[l][2], yv[l], yh); acc[l][3] = dsum(acc[l][3], yv[l], p);
                acc[l][4] = dsum(acc[l][4], yv[l], u);
            }
        }
    };
    auto sums_ew = [&](double g, double gt, double u, double fl, const double (&sv)[LPW], const double (&yv)[LPW]) {   // one element; fl: its share of f (the pair's f with the first)
        const double y = gt - g;
        if (wave == 0) { d0 = dsum(d0, g, u); d1 = dsum(d1, u, u); }
        else if (wave == 1) { d0 += fl; d1 = dsum(d1, gt, u); d2s = dsum(d2s, gt, gt); d3 = dsum(d3, y, gt); }
        else if (wave == 2) { d0 = dsum(d0, u, y); d1 = dsum(d1, y, y); }
#pragma unroll
        for (int l = 0; l < LPW; ++l) {
            if (on[l]) {
                acc[l][0] = dsum(acc[l][0], sv[l], gt); acc[l][1] = dsum(acc[l][1], yv[l], gt);
                acc[l][2] = dsum(acc[l][2], sv[l], y);  acc[l][3] = dsum(acc[l][3], yv[l], y);
                acc[l][4] = dsum(acc[l][4], yv[l], u);
            }
        }
    };
    auto pair = [&](d2 xv, d2 g, d2 u, const PV<Obj> &pv, const d2 (&sj)[LPW], const d2 (&yj)[LPW]) {
        double sx[LPW], sy[LPW], yx[LPW], yy[LPW];
#pragma unroll
        for (int l = 0; l < LPW; ++l) { sx[l] = sj[l].x; sy[l] = sj[l].y; yx[l] = yj[l].x; yy[l] = yj[l].y; }
        if constexpr (LSE) {
            elem_lse(xv.x, g.x, u.x, sx, yx);
            elem_lse(xv.y, g.y, u.y, sy, yy);
        } else {
            d2 xp, gt;
            xp.x = xv.x + a_trial * u.x; xp.y = xv.y + a_trial * u.y;
            double fl = 0.0;
            obj_eval2<Obj>(xp, pv, Q.lambda, fl, gt);
            sums_ew(g.x, gt.x, u.x, fl, sx, yx);
            sums_ew(g.y, gt.y, u.y, 0.0, sy, yy);
        }
    };
    auto push_pair = [&](d2 &xv, d2 &g, d2 uo, const PV<Obj> &pv, d2 &s, d2 &y) {   // k_lbfgs_push_lite's expressions
        xv.x = xv.x + U.a * uo.x; xv.y = xv.y + U.a * uo.y;
        d2 gt;
        if constexpr (LSE) {
            gt.x = exp(xv.x - U.M) / U.S + Q.lambda * xv.x;
            gt.y = exp(xv.y - U.M) / U.S + Q.lambda * xv.y;
        } else {
            double fl = 0.0;
            obj_eval2<Obj>(xv, pv, Q.lambda, fl, gt);
        }
        s.x = U.a_s * uo.x; s.y = U.a_s * uo.y;
        y.x = gt.x - g.x; y.y = gt.y - g.y;
        g = gt;
    };
    const long long n2 = P.n >> 1;
    long long i0, hi, step;
    if (BIG) {
        const long long per = big_chunk_pairs(n2, gridDim.x);
        i0 = per * blockIdx.x;
        hi = (i0 + per < n2) ? i0 + per : n2;
        step = 64;
    } else {
        i0 = (long long)blockIdx.x * 64;
        hi = n2;
        step = (long long)gridDim.x * 64;
    }
    int buf = 0;
    for (; i0 < hi; i0 += step, buf ^= 1) {   // (trip count is uniform over the workgroup: the barrier is reached by all)
        const long long i = i0 + lane;
        const bool valid = i < hi;
        d2 g{0.0, 0.0}, xv{0.0, 0.0}, sn{0.0, 0.0}, yn{0.0, 0.0}, sj[LPW], yj[LPW];
        PV<Obj> pv;
#pragma unroll
        for (int k = 0; k < (int)(sizeof(pv.v) / sizeof(pv.v[0])); ++k) pv.v[k] = d2{0.0, 0.0};
        d2 r{0.0, 0.0};
        if (valid) {
            g = ldg2<false>(P.g, i); xv = ldg2<false>(x, i);
            if (obj_nparams<Obj>() > 0) pv = pv_load<Obj, false>(Q, i);
            d2 uo{0.0, 0.0};
            if (PUSH) uo = ldg2<false>(P.u, i);
#pragma unroll
            for (int l = 0; l < LPW; ++l)
                if (on[l] && !(l == 0 && newp)) { yj[l] = ldg2<BIG>(Yj[l], i); sj[l] = ldg2<BIG>(Sj[l], i); }
            if (PUSH) {
                push_pair(xv, g, uo, pv, sn, yn);
                if (newp) { sj[0] = sn; yj[0] = yn; }
            }
            if (wave == 0) { r.x = P.cg * g.x; r.y = P.cg * g.y; }
#pragma unroll
            for (int l = 0; l < LPW; ++l) {
                if (on[l]) {
                    r.x = r.x + cy[l] * yj[l].x; r.y = r.y + cy[l] * yj[l].y;
                    r.x = r.x + cs[l] * sj[l].x; r.y = r.y + cs[l] * sj[l].y;
                }
            }
        }
        pu[buf][wave][lane] = r;
        if (PUSH) __builtin_amdgcn_s_waitcnt(0);   // every old x, g, u of this trip has arrived in every wave before any is overwritten
        __syncthreads();
        if (valid) {
            d2 u = pu[buf][0][lane];
#pragma unroll
            for (int w = 1; w < W; ++w) { const d2 t = pu[buf][w][lane]; u.x = u.x + t.x; u.y = u.y + t.y; }
            if (wave == 0) stg2<BIG>(P.u, i, u);
            if (PUSH) {
                if (wave == 1) stg2<BIG>(U.x, i, xv);
                else if (wave == 2) stg2<BIG>(U.g, i, g);
                else if (wave == 3) { stg2<BIG>(U.sn, i, sn); stg2<BIG>(U.yn, i, yn); }
            }
            pair(xv, g, u, pv, sj, yj);
        }
    }
    if ((P.n & 1) && blockIdx.x == 0) {   // odd tail element: lane 0 of every wave forms the same u (wave order) and takes its own sums
        const long long e = P.n - 1;
        double g = 0.0, xe = 0.0, u = 0.0, sne = 0.0, yne = 0.0;
        PS<Obj> pe;
#pragma unroll
        for (int k = 0; k < (int)(sizeof(pe.v) / sizeof(pe.v[0])); ++k) pe.v[k] = 0.0;
        double sv[LPW], yv[LPW];
        auto grad1 = [&](double xx, double &fl) {   // ∇f at one element
            double gt = 0.0;
            if constexpr (!LSE) obj_eval1<Obj>(xx, pe, Q.lambda, fl, gt);
            return gt;
        };
        if (lane == 0) {
            g = P.g[e]; xe = x[e];
            if (obj_nparams<Obj>() > 0) pe = ps_load<Obj>(Q, e);
            if (PUSH) {
                const double uo = P.u[e];
                xe = xe + U.a * uo;
                double fl = 0.0;
                const double gt = LSE ? exp(xe - U.M) / U.S + Q.lambda * xe : grad1(xe, fl);
                sne = U.a_s * uo; yne = gt - g; g = gt;
            }
            for (int w = 0; w < W; ++w) {
                double r = (w == 0) ? P.cg * g : 0.0;
                for (int l = 0; l < LPW; ++l) {
                    const int j = l * W + w;
                    if (j < P.count) {
                        const bool nw = PUSH && U.new_in_list && j == 0;
                        r = r + P.cy[j] * (nw ? yne : P.Y[(size_t)P.slots[j] * ring_ld(P.n) + e]);
                        r = r + P.cs[j] * (nw ? sne : P.S[(size_t)P.slots[j] * ring_ld(P.n) + e]);
                    }
                }
                u = (w == 0) ? r : u + r;
            }
            for (int l = 0; l < LPW; ++l) {
                const bool nw = newp && l == 0;
                sv[l] = on[l] ? (nw ? sne : Sj[l][e]) : 0.0; yv[l] = on[l] ? (nw ? yne : Yj[l][e]) : 0.0;
            }
        }
        if (PUSH) { __builtin_amdgcn_s_waitcnt(0); __syncthreads(); }   // (uniform branch) the old x, g, u of the element are in every wave's registers
        if (lane == 0) {
            if (wave == 0) P.u[e] = u;
            if (PUSH) {
                if (wave == 1) U.x[e] = xe;
                else if (wave == 2) U.g[e] = g;
                else if (wave == 3) { U.sn[e] = sne; U.yn[e] = yne; }
            }
            if constexpr (LSE) {
                elem_lse(xe, g, u, sv, yv);
            } else {
                double fl = 0.0;
                const double gt = grad1(xe + a_trial * u, fl);
                sums_ew(g, gt, u, fl, sv, yv);
            }
        }
    }
    double *row = P.partials + (size_t)blockIdx.x * NG;
    {
        const double v0 = wave_sum(d0), v1 = wave_sum(d1), v2 = wave_sum(d2s), v3 = wave_sum(d3);
        if (lane == 0) {
            if (LSE) {
                if (wave == 0) { row[SP_GU] = v0; row[SP_UU] = v1; row[SP_GH2] = v2; row[SP_GHP] = v3; }
                else if (wave == 1) { row[SP_S] = v0; row[SP_T] = v1; row[SP_Q] = v2; row[SP_R] = v3; }
                else if (wave == 2) { row[SP_E0] = v0; row[SP_E0 + 1] = v1; row[SP_E0 + 2] = v2; }
                else { row[SP_E0 + 3] = v0; row[SP_E0 + 4] = v1; row[SP_E0 + 5] = v2; }
            } else {
                if (wave == 0) { row[SP_GU] = v0; row[SP_UU] = v1; }
                else if (wave == 1) { row[SE_F] = v0; row[SE_GTU] = v1; row[SE_GTGT] = v2; row[SE_YGT] = v3; }
                else if (wave == 2) { row[SE_UY] = v0; row[SE_YY] = v1; }
                else { for (int q = 8; q < SP_PAIR; ++q) row[q] = 0.0; row[NG - 1] = 0.0; }
            }
        }
    }
#pragma unroll
    for (int l = 0; l < LPW; ++l) {
        const int j = l * W + wave;
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const double v = wave_sum(acc[l][q]);
            if (lane == 0 && j < SPEC_MAXC) row[SP_PAIR + 5 * j + q] = on[l] ? v : 0.0;
        }
    }
}

// The state update behind an accepted SPECULATED trial (k_lbfgs_combine_spec) when no direction pass follows that could
// carry it (the solve's last iteration, or something else touches x, g or the ring first): every sum the host needs is
// already there, so this pass only moves data — x ← x + a·u, g ← g⁺ (log-sum-exp: exp(xp − M)/S + λ·xp, k_lse_grad's
// expression; element-wise: ∇f(xp)), s = a_s·u, y = g⁺ − g into the free ring slot.  R x, u, g · W x, g, s, y = 56 B/element
// (+ 8 for a parameter vector); x and g in place (read and written by the same lane).  Launched only after the host has seen
// ‖g⁺‖ finite (optim.jl:107-121).
template <class Obj, bool BIG>
__global__ __launch_bounds__(BLOCK) void k_lbfgs_push_lite(double *x, const double *u, double *g, double *sn, double *yn, const double *p0, long long n,
                                                           double a, double a_s, double M, double S, double lambda,
                                                           const double *p1, const double *p2, const double *p3) {
    constexpr bool LSE = SpecKind<Obj>::lse;
    const ParamPtrs pp{p0, p1, p2, p3};
    const long long n2 = n >> 1;
    long long i, hi, step;
    if (BIG) {
        const long long per = big_chunk_pairs(n2, gridDim.x);
        i = per * blockIdx.x + threadIdx.x;
        hi = (per * blockIdx.x + per < n2) ? per * blockIdx.x + per : n2;
        step = BLOCK;
    } else {
        i = (long long)blockIdx.x * BLOCK + threadIdx.x;
        hi = n2;
        step = (long long)gridDim.x * BLOCK;
    }
    for (; i < hi; i += step) {
        d2 xv = ldg2<BIG>(x, i);
        const d2 gv = ldg2<BIG>(g, i), uv = ldg2<BIG>(u, i);
        const PV<Obj> pv = pv_load<Obj, BIG>(pp, i);
        xv.x = xv.x + a * uv.x; xv.y = xv.y + a * uv.y;
        d2 gt, s, y;
        if constexpr (LSE) {
            gt.x = exp(xv.x - M) / S + lambda * xv.x;
            gt.y = exp(xv.y - M) / S + lambda * xv.y;
        } else {
            double fl = 0.0;
            obj_eval2<Obj>(xv, pv, lambda, fl, gt);
        }
        s.x = a_s * uv.x; s.y = a_s * uv.y;
        y.x = gt.x - gv.x; y.y = gt.y - gv.y;
        stg2<BIG>(x, i, xv); stg2<BIG>(g, i, gt); stg2<BIG>(sn, i, s); stg2<BIG>(yn, i, y);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const long long e = n - 1;
        const double uv = u[e], xe = x[e] + a * uv;
        double gt = 0.0;
        if constexpr (LSE) gt = exp(xe - M) / S + lambda * xe;
        else { double fl = 0.0; obj_eval1<Obj>(xe, ps_load<Obj>(pp, e), lambda, fl, gt); }
        sn[e] = a_s * uv; yn[e] = gt - g[e];
        x[e] = xe; g[e] = gt;
    }
}

#ifndef CGO_RTC
// ---- device-side fills (counter-based RNG shared with the oracle) -----------
__device__ inline double uniform01(uint64_t seed, uint64_t index) {
    uint64_t z = (seed ^ index) + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z = z ^ (z >> 31);
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

static __global__ __launch_bounds__(BLOCK) void k_fill(double *v, long long n, long long offset, int kind,
                                                uint64_t seed, double lo, double hi) {
    const long long T = (long long)gridDim.x * BLOCK;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += T) {
        const uint64_t gi = (uint64_t)(offset + i);
        double r;
        if (kind == 1) r = lo + (hi - lo) * uniform01(seed, gi);
        else if (kind == 2) r = (gi & 1) ? hi : lo;
        else r = lo;
        v[i] = r;
    }
}

#endif  // CGO_RTC

}  // namespace dev
}  // namespace cgo
