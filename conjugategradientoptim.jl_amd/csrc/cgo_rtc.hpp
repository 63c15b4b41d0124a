// cgo_rtc.hpp — run-time compilation of user-supplied element-wise objectives (hiprtc, gfx950).
#pragma once

#include <hip/hip_runtime.h>

#include <initializer_list>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace cgo {

// A loaded code object holding k_cg<UserObjective, …> and k_fused<UserObjective, …> instantiations.
struct RtcModule {
    hipModule_t mod = nullptr;
    std::map<std::string, hipFunction_t> fn;
    ~RtcModule();
    hipFunction_t cg(int mode, int npts, bool big) const;
    hipFunction_t fused(int mode, bool big) const;
    hipFunction_t resident(int npts) const;   // k_resident<UserObjective, npts> (npts = 3 only), or nullptr
    // k_resident<UserObjective, npts, true> (cgo_solver_probe_resident): NOT part of the module above — a second program,
    // compiled from the kept source on the first probe (rtc_compile_resident_probe), so that creating an objective costs
    // what it did before the probe existed
    hipFunction_t resident_probe(int npts) const;
    hipModule_t probe_mod = nullptr;
    // k_batch<UserObjective, npts> (batched solves, cgo_rtc_batch.hip): a program of its own as well, compiled on the first
    // batched solve on the objective (rtc_compile_batch) — an objective that never batches does not pay for it
    hipFunction_t batch(int npts) const;
    hipFunction_t batch_grad() const;         // k_batch_grad<UserObjective>, in the same program
    hipModule_t batch_mod = nullptr;
    // the batched solves' second tier (problem rows streamed from device memory, cgo_kernels_batch_rows.hip.hpp): a THIRD program,
    // compiled on the first solve of that tier (rtc_compile_batch_rows) — a user who never asks for the tier does not pay for it
    hipFunction_t batch_rows(int npts) const;
    hipModule_t rows_mod = nullptr;
    // the PROBE twins of k_batch and k_batch_rows (cgo_batch_probe): one more program, compiled from the kept source on the
    // first probe (rtc_compile_batch_probe) — creating an objective and its first batched solve cost what they did
    hipFunction_t batch_probe(bool device_rows, int npts) const;
    hipModule_t batch_probe_mod = nullptr;
    // the batched L-BFGS solves' kernel (cgo_rtc_batch_lbfgs.hip): a FIFTH program, compiled on the first batched L-BFGS solve on
    // the objective (rtc_compile_batch_lbfgs).  It carries a k_batch_grad of its own, so that the results' gradient of such a
    // solve with a scalar per problem does not compile the LDS tier's batch program: batch_grad() finds either.
    hipFunction_t batch_lbfgs(int npts) const;
    hipModule_t batch_lbfgs_mod = nullptr;
    // … and of their LDS tier (cgo_rtc_batch_lbfgs_lds.hip): one more program, holding k_batch_lbfgs_lds alone, compiled on the
    // first solve of that tier on the objective (rtc_compile_batch_lbfgs_lds)
    hipFunction_t batch_lbfgs_lds(int npts) const;
    hipModule_t batch_lbfgs_lds_mod = nullptr;
    std::string user_source;
    int n_params = 0;   // parameter slots the objective was created with (0 … CGO_MAX_PARAM_SLOTS)
    int device = 0;
    hipFunction_t spec(bool big, bool push) const;   // k_lbfgs_combine_spec<UserObjective, big, push>
    hipFunction_t lite(bool big) const;              // k_lbfgs_push_lite<UserObjective, big>
private:
    // the kernel filed under `prefix` + NPTS for the last of `rows` with NPTS ≤ npts, the first row below that (the rule of the
    // ahead-of-time dispatch); `rows` are the values of a row macro of cgo_instances.def, in its order
    hipFunction_t row_kernel(const std::string &prefix, std::initializer_list<int> rows, int npts) const;
};

// `source`: either a complete `struct UserObjective { … };` (functor interface of
// cgo_kernels.hip.hpp) or just the statements of an element-wise body that compute `fi` and
// `gi` from `x`, `p` (slot 0), `p1`, `p2`, `p3` (slots 1–3, as far as n_params goes), `s0`.  A struct that declares kParams
// must declare n_params of them.  Returns CGO_OK / CGO_EINVAL (compile log in `log`) / CGO_EHIP.
int rtc_compile_objective(int device, const std::string &source, int n_params,
                          std::shared_ptr<RtcModule> &out, std::string &log);
// the PROBE form of the module's resident kernel, compiled and loaded on first use; CGO_OK if it is there already
int rtc_compile_resident_probe(RtcModule &m, std::string &log);
// k_batch for the module's objective, one kernel per row of CGO_BATCH_ROWS, compiled and loaded on first use (cgo_rtc_batch.hip)
int rtc_compile_batch(RtcModule &m, std::string &log);
// the kernel of the batched solves' second tier for the module's objective, one per row of CGO_BATCH_DEVROWS_ROWS, likewise
int rtc_compile_batch_rows(RtcModule &m, std::string &log);
// the PROBE twins of both, one per row of CGO_BATCH_ROWS and of CGO_BATCH_DEVROWS_ROWS, in one program, likewise
int rtc_compile_batch_probe(RtcModule &m, std::string &log);
// the batched L-BFGS kernel for the module's objective, one per row of CGO_BATCH_LBFGS_ROWS, and k_batch_grad, likewise
int rtc_compile_batch_lbfgs(RtcModule &m, std::string &log);
// the kernel of the batched L-BFGS solves' LDS tier for the module's objective, one per row of CGO_BATCH_LBFGS_LDS_ROWS, likewise
int rtc_compile_batch_lbfgs_lds(RtcModule &m, std::string &log);
// the head of both programs' further text: this build's pairs per lane and trip of the device tier's ring passes, as #defines
std::string rtc_batch_lbfgs_defines();

// What a further program of a module is built from (cgo_rtc.hip): the embedded kernel templates + the user's objective as one
// translation unit, and one program → one loaded module: compiles `src` for the name expressions of `wants`, loads the code
// object as `mod` and files every kernel in `fn` under its key.  On failure `mod` is unloaded again and `fn` is as it was.
struct Want { std::string key, expr; };
std::string rtc_program_source(const std::string &source, int n_params);
// … with further headers (`more`) between the embedded templates and the user's objective
std::string rtc_program_source_with(const std::string &source, int n_params, const std::string &more);
int rtc_build(const std::string &src, const char *name, const std::vector<Want> &wants, hipModule_t &mod,
              std::map<std::string, hipFunction_t> &fn, std::string &log);

}  // namespace cgo
