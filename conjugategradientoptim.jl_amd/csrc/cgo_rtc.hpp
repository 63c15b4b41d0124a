// cgo_rtc.hpp — run-time compilation of user-supplied element-wise objectives (hiprtc, gfx950).
#pragma once

#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace cgo {

// The programs of a run-time compiled objective's module: the one compiled at creation, and the further ones, each compiled from
// the kept source on the first use of what it holds and kept on the RtcModule — creating an objective, and every use that needs
// none of them, costs what it did before they existed.  One row each in cgo_instances.def (CGO_RTC_PROGRAM_ROWS: file name,
// wording, text; CGO_RTC_KERNEL_ROWS / CGO_RTC_EXTRA_ROWS: kernels), in this order.
enum RtcProgram {
    RTC_NONE = -1,
    RTC_CREATE = 0,        // k_cg, k_fused, the per-objective L-BFGS kernels, k_resident (rtc_compile_objective)
    RTC_RESIDENT_PROBE,    // k_resident<…, true> (cgo_solver_probe_resident)
    RTC_BATCH,             // k_batch, k_batch_grad
    RTC_BATCH_ROWS,        // k_batch_rows
    RTC_BATCH_PROBE,       // k_batch<…, true>, k_batch_rows<…, true> (cgo_batch_probe)
    RTC_BATCH_LBFGS,       // k_batch_lbfgs, k_batch_grad
    RTC_BATCH_LBFGS_LDS,   // k_batch_lbfgs_lds
    RTC_PROGRAMS
};

// The loaded code objects of one objective text: mods[RTC_CREATE] always, the others once compiled (rtc_compile_program).
struct RtcModule {
    hipModule_t mods[RTC_PROGRAMS] = {};
    std::map<std::string, hipFunction_t> fn;   // every loaded kernel under its key
    // held while a further program is built and filed in `fn`: two first uses must not both build it, nor two programs write
    // `fn` at once (objectives of one text share the module).  Lookups take no lock: a kernel is looked up by those who compiled
    // its program, or after them.
    std::mutex mu;
    ~RtcModule();
    hipFunction_t cg(int mode, int npts, bool big) const;
    hipFunction_t fused(int mode, bool big) const;
    hipFunction_t resident(int npts) const;   // k_resident<UserObjective, npts> (npts = 3 only), or nullptr
    // the kernels of the further programs, nullptr before their program is compiled: the row of cgo_instances.def for npts
    hipFunction_t resident_probe(int npts) const;
    hipFunction_t batch(int npts) const;
    hipFunction_t batch_grad() const;         // k_batch_grad<UserObjective>: the batch program's, else the batched L-BFGS program's
    hipFunction_t batch_rows(int npts) const;
    hipFunction_t batch_probe(bool device_rows, int npts) const;
    hipFunction_t batch_lbfgs(int npts) const;
    hipFunction_t batch_lbfgs_lds(int npts) const;
    // … by program and key prefix (a row of CGO_RTC_KERNEL_ROWS): what a table of tiers names (cgo_backend_batch.hip)
    hipFunction_t kernel(RtcProgram prog, const char *prefix, int npts) const;
    std::string user_source;
    int n_params = 0;   // parameter slots the objective was created with (0 … CGO_MAX_PARAM_SLOTS)
    int device = 0;
    hipFunction_t spec(bool big, bool push) const;   // k_lbfgs_combine_spec<UserObjective, big, push>
    hipFunction_t lite(bool big) const;              // k_lbfgs_push_lite<UserObjective, big>
    // the kernel filed under `prefix` + NPTS for the last of `rows` with NPTS ≤ npts, the first row below that (the rule of the
    // ahead-of-time dispatch); `rows` are the values of a row macro of cgo_instances.def, in its order
    hipFunction_t row_kernel(const std::string &prefix, const std::vector<int> &rows, int npts) const;
};

// `source`: either a complete `struct UserObjective { … };` (functor interface of
// cgo_kernels.hip.hpp) or just the statements of an element-wise body that compute `fi` and
// `gi` from `x`, `p` (slot 0), `p1`, `p2`, `p3` (slots 1–3, as far as n_params goes), `s0`.  A struct that declares kParams
// must declare n_params of them.  Returns CGO_OK / CGO_EINVAL (compile log in `log`) / CGO_EHIP.
int rtc_compile_objective(int device, const std::string &source, int n_params,
                          std::shared_ptr<RtcModule> &out, std::string &log);
// One program as hiprtc gets it: the file name, the complete text, and the name expressions in order, each with the key its
// kernel is filed under in RtcModule::fn.
struct Want { std::string key, expr; };
struct RtcPlan { const char *name; std::string src; std::vector<Want> wants; };
// A further program of the module (any but RTC_CREATE), compiled and loaded on first use; CGO_OK if it is there already.
// THE one place that compiles them (cgo_rtc_batch.hip): rtc_program_plan, which touches no device, then rtc_build.
int rtc_compile_program(RtcModule &m, RtcProgram prog, std::string &log);
RtcPlan rtc_program_plan(RtcProgram prog, const std::string &source, int n_params);
std::vector<Want> rtc_create_wants();            // … the name expressions of RTC_CREATE, from the per-objective rows (cgo_rtc.hip)
const char *rtc_program_what(RtcProgram prog);   // the program in words: "user objective: <what> did not compile"
// the head of the batched L-BFGS programs' further text: this build's pairs per lane and trip of the device tier's ring passes, as #defines
std::string rtc_batch_lbfgs_defines();

// What a program is built from (cgo_rtc.hip): the embedded kernel templates + the user's objective as one translation unit …
std::string rtc_program_source(const std::string &source, int n_params);
// … with further headers (`more`) between the embedded templates and the user's objective
std::string rtc_program_source_with(const std::string &source, int n_params, const std::string &more);
// … and one program → one loaded module: compiles `src` for the name expressions of `wants`, loads the code object as `mod` and
// files every kernel in `fn` under its key.  On failure `mod` is unloaded again and `fn` is as it was.
int rtc_build(const std::string &src, const char *name, const std::vector<Want> &wants, hipModule_t &mod,
              std::map<std::string, hipFunction_t> &fn, std::string &log);

}  // namespace cgo
