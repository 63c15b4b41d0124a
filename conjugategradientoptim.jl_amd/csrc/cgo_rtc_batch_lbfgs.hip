// cgo_rtc_batch_lbfgs.hip — batched L-BFGS solves on a run-time compiled objective: k_batch_lbfgs<UserObjective, NPTS>
// (cgo_kernels_batch_lbfgs.hip.hpp) for the rows of CGO_BATCH_LBFGS_ROWS, as a FIFTH program of the objective's module, compiled
// from the kept source on the first batched L-BFGS solve and kept on the RtcModule, as the other further programs are
// (cgo_rtc_batch.hip).
//
// The text every other program is built from (gen_rtc_sources.py) carries neither the scalar recursion nor the quasi-Newton
// loop; this program adds cgo_qn.hpp, cgo_resident_qn.hpp and the kernel's header (gen_rtc_lbfgs_sources.py) between that text
// and the user's objective.  k_batch_grad<UserObjective> is instantiated here as well: the results' gradient of a solve with a
// scalar per problem needs it, and the LDS tier's 512-VGPR batch program is not compiled merely for that.
#include "cgo_rtc.hpp"

#include <mutex>

#include "cgo_hip_backend.hpp"
#include "cgo_instances.def"
#include "cgo_kernels_batch_lbfgs.hip.hpp"   // CGO_BATCH_LBFGS_U, CGO_BATCH_LBFGS_U_SLOTS: the program takes this build's
#include "cgo_rtc_lbfgs_sources.inc"

namespace cgo {

#define ROW_NPTS(NPTS) NPTS,
hipFunction_t RtcModule::batch_lbfgs(int npts) const { return row_kernel("batch_qn:", {CGO_BATCH_LBFGS_ROWS(ROW_NPTS)}, npts); }

#define CGO_STR2(x) #x
#define CGO_STR(x) CGO_STR2(x)

// (an A/B build's EXTRA reaches the program's text too)
std::string rtc_batch_lbfgs_defines() {
    return "\n#define CGO_BATCH_LBFGS_U " CGO_STR(CGO_BATCH_LBFGS_U) "\n#define CGO_BATCH_LBFGS_U_SLOTS " CGO_STR(CGO_BATCH_LBFGS_U_SLOTS) "\n";
}

int rtc_compile_batch_lbfgs(RtcModule &m, std::string &log) {
    static std::mutex mu;   // (as rtc_compile_batch)
    std::lock_guard<std::mutex> lock(mu);
    if (m.batch_lbfgs_mod) return CGO_OK;
    if (hipSetDevice(m.device) != hipSuccess) { log = "hipSetDevice failed"; return CGO_EHIP; }
    std::string more = rtc_batch_lbfgs_defines();   // the pairs per lane and trip this library was built with
    for (const char *c : kRtcLbfgsSourceChunks) more += c;
    std::vector<Want> wants;
#define ROW(NPTS) wants.push_back({"batch_qn:" #NPTS, "cgo::dev::k_batch_lbfgs<cgo::dev::UserObjective, " #NPTS ">"});
    CGO_BATCH_LBFGS_ROWS(ROW)
#undef ROW
    wants.push_back({"batch_qn:grad", "cgo::dev::k_batch_grad<cgo::dev::UserObjective>"});
    return rtc_build(rtc_program_source_with(m.user_source, m.n_params, more), "cgo_user_objective_batch_lbfgs.hip", wants, m.batch_lbfgs_mod, m.fn, log);
}

}  // namespace cgo
