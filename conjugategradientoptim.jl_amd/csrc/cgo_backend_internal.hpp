// cgo_backend_internal.hpp — what the translation units of the device backend share (round 4: cgo_hip_backend.hip split along its
// families): cgo_hip_backend.hip (context, reductions to the host, the stored-gradient k_fused launches, results, raw entry points),
// cgo_backend_cg.hip (k_cg / k_chain launches, reduction tails, on-device controller, resident solver), cgo_backend_lbfgs.hip
// (log-sum-exp + L-BFGS ring) and cgo_backend_place.hip (buffer placement search, stream-mix harness).
#pragma once

#include "cgo_hip_backend.hpp"
#include "cgo_instances.def"

#include <algorithm>
#include <cstdarg>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <type_traits>
#include <vector>

namespace cgo {

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e__ = (expr);                                                           \
        if (e__ != hipSuccess) {                                                           \
            set_error(std::string("HIP error: ") + hipGetErrorString(e__) + " at " #expr); \
            return CGO_EHIP;                                                               \
        }                                                                                  \
    } while (0)

static inline double now_ns() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e9 + (double)ts.tv_nsec;
}

// the probes' NaN slack (cgo_solver_probe_launch, cgo_solver_probe_lbfgs): both halves equal, so that hipMemsetD32 fills it;
// as a double a quiet NaN.  Buffers are padded to whole 128-B lines plus one more line.
constexpr unsigned PROBE_NAN32 = 0x7FF87FF8u;
static inline size_t probe_padded(size_t n) { return ((n + 15) & ~(size_t)15) + 16; }

// Row-width dispatch of the reduction launches: f(Width<N>) for the N of the list that equals `ns`; with `or_last`, the last N of
// the list for every other width.  false: none (each site lists the widths its kernels are instantiated for).
template <int N> using Width = std::integral_constant<int, N>;
template <int N, int... Rest, class F>
static inline bool with_width(int ns, bool or_last, F f) {
    if (ns == N || (or_last && sizeof...(Rest) == 0)) { f(Width<N>{}); return true; }
    if constexpr (sizeof...(Rest) > 0) return with_width<Rest...>(ns, or_last, f);
    else return false;
}

// ---- the tiers of batched solves ------------------------------------------------------------------------------------------------
// THE rule of a row family of cgo_instances.def with a row per point count: npts points get the last row with NPTS ≤ npts, the
// first row below that.  A translation unit that instantiates a family expands its rows into a RowPick once per objective,
//     template <class Obj> struct Rows { static RowPick at(int npts) { RowPick p;  CGO_…_ROWS(ROW)  return p; } };
//     with  #define ROW(NPTS) p.row(npts, NPTS, (const void *)k_…<Obj, NPTS>);
// and exports row_pick_for<Rows> as its one lookup, (obj_kind, npts) → kernel and the NPTS picked (nothing: no such objective).
struct RowPick {
    const void *fn = nullptr;
    int points = 0;
    void row(int npts, int row_npts, const void *kernel) { if (!fn || npts >= row_npts) { fn = kernel; points = row_npts; } }
};
namespace dev {
#define ROW(KIND, T) struct T;
CGO_OBJ_ROWS(ROW)
#undef ROW
}
template <template <class> class Rows, class... More>
static inline RowPick row_pick_for(int obj_kind, int npts, More... more) {   // (more: what a unit of several families picks among them by)
    switch (obj_kind) {
#define ROW(KIND, T) case KIND: return Rows<dev::T>::at(npts, more...);
    CGO_OBJ_ROWS(ROW)
#undef ROW
    default: return RowPick{};
    }
}
using RowLookup = RowPick (*)(int obj_kind, int npts);
RowPick batch_probe_kernel_for(BatchTier tier, int obj_kind, int npts);   // the PROBE twins of every tier (cgo_backend_batch_probe.hip)

// One row per tier (batch_tier_of, cgo_backend_batch.hip): everything the host side of a batch asks that depends on the tier.
// A tier's row stands in the translation unit that instantiates its kernels (tier_row_…), which names no other tier's.
struct BatchTierRow {
    const char *family;               // the kernel template as the probe reports it
    RowLookup aot;                    // the ahead-of-time instantiations: the unit's one lookup
    RtcProgram prog;                  // a run-time compiled objective's program of the tier and the key prefix of its kernels
    const char *key;                  // (CGO_RTC_KERNEL_ROWS, cgo_instances.def)
    RtcProgram probe_prog;            // … of their PROBE twins; RTC_NONE: the module builds none (cgo_batch_probe refuses a model there)
    const char *probe_key;
    bool qn;                          // β = LBFGS(m): a ring and a QnState per problem, BatchLbfgsParams
    int (*lds_rows)(int K, int m);    // rows of ld doubles a launch keeps in dynamic LDS, K parameter slots and m pairs
    const char *missing;              // the refusal where an objective has no ahead-of-time instantiation
};
const BatchTierRow &batch_tier_of(BatchTier tier);
const BatchTierRow &tier_row_lds();         // cgo_backend_batch.hip
const BatchTierRow &tier_row_rows();        // cgo_backend_batch_rows.hip
const BatchTierRow &tier_row_lbfgs();       // cgo_backend_batch_lbfgs.hip
const BatchTierRow &tier_row_lbfgs_lds();   // cgo_backend_batch_lbfgs_lds.hip
// a module's kernel of the tier for npts points (nullptr: no module, or the program is not compiled), its PROBE twin with `probe`
hipFunction_t batch_tier_module_kernel(const BatchTierRow &t, const RtcModule *rtc, int npts, bool probe = false);
// largest ld one workgroup's LDS holds of a problem of that tier, m pairs (batch_max_n, batch_lbfgs_lds_max_ld)
int64_t batch_tier_max_ld(HipCtx *ctx, BatchTier tier, int obj_kind, int m, const RtcModule *rtc);
// static LDS of an ahead-of-time kernel (fn) or else of a module's (mf); false: HIP refused, the error cleared
bool kernel_static_lds(const void *fn, hipFunction_t mf, int64_t &bytes);

// streaming policy and grids (cgo_hip_backend.hip)
double big_bytes_for(double forced, bool read_only = false);
double env_big_bytes();
bool is_big(int obj_kind, int mode, int64_t n, int n_params, double forced);
std::string fused_symbol(const char *obj_tname, int mode, bool big);   // a k_fused instantiation as rocprofv3 prints it minus namespaces
int grid_cg(int64_t n, int npts = 1);
// ALGORITHMIC bytes of a k_cg / k_chain launch (cgo_backend_cg.hip)
double bytes_r(int obj_kind, int mode, int64_t n, int n_params);
void unpack_r(const double *s, int k, Scal *out, bool dir, int npts = 0);
// host side of the publish protocols (cgo_hip_backend.hip)
int launch_module(hipFunction_t f, void *params, int grid, hipStream_t st);
int wait_word(HipCtx *ctx, unsigned long long *word, unsigned long long want);
int wait_checked(HipCtx *ctx, unsigned long long *word, unsigned long long want, const double *block, int ns, double *dst);

}  // namespace cgo
