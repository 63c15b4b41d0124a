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
