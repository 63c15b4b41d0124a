// cgo_rtc_batch_lbfgs_lds.hip — the LDS tier of batched L-BFGS solves on a run-time compiled objective:
// k_batch_lbfgs_lds<UserObjective, NPTS> (cgo_kernels_batch_lbfgs_lds.hip.hpp) for the rows of CGO_BATCH_LBFGS_LDS_ROWS, as one
// more program of the objective's module, compiled from the kept source on the first solve of this tier and kept on the
// RtcModule, as the other further programs are (cgo_rtc_batch.hip, cgo_rtc_batch_lbfgs.hip).
//
// Its text is the device tier's program text (gen_rtc_sources.py, then gen_rtc_lbfgs_sources.py: the scalar recursion, the
// quasi-Newton loop, BatchLbfgsParams) with the new kernel's header behind it (gen_rtc_lbfgs_lds_sources.py).  It holds that one
// kernel and nothing else: the results' gradient with a scalar per problem is k_batch_grad's of whichever program has it
// (RtcModule::batch_grad), compiled by the backend where none has.
#include "cgo_rtc.hpp"

#include <mutex>

#include "cgo_hip_backend.hpp"
#include "cgo_instances.def"
#include "cgo_kernels_batch_lbfgs_lds.hip.hpp"   // the pairs per lane and trip of this build
#include "cgo_rtc_lbfgs_sources.inc"
#include "cgo_rtc_lbfgs_lds_sources.inc"

namespace cgo {

#define ROW_NPTS(NPTS) NPTS,
hipFunction_t RtcModule::batch_lbfgs_lds(int npts) const { return row_kernel("batch_qn_lds:", {CGO_BATCH_LBFGS_LDS_ROWS(ROW_NPTS)}, npts); }

#define CGO_STR2(x) #x
#define CGO_STR(x) CGO_STR2(x)

int rtc_compile_batch_lbfgs_lds(RtcModule &m, std::string &log) {
    static std::mutex mu;   // (as rtc_compile_batch)
    std::lock_guard<std::mutex> lock(mu);
    if (m.batch_lbfgs_lds_mod) return CGO_OK;
    if (hipSetDevice(m.device) != hipSuccess) { log = "hipSetDevice failed"; return CGO_EHIP; }
    // the pairs per lane and trip this library was built with (an A/B build's EXTRA reaches the program's text too)
    std::string more = rtc_batch_lbfgs_defines();
    more += "#define CGO_BATCH_LBFGS_LDS_U " CGO_STR(CGO_BATCH_LBFGS_LDS_U) "\n#define CGO_BATCH_LBFGS_LDS_U_SLOTS " CGO_STR(CGO_BATCH_LBFGS_LDS_U_SLOTS) "\n";
    for (const char *c : kRtcLbfgsSourceChunks) more += c;
    more += "\n";
    for (const char *c : kRtcLbfgsLdsSourceChunks) more += c;
    std::vector<Want> wants;
#define ROW(NPTS) wants.push_back({"batch_qn_lds:" #NPTS, "cgo::dev::k_batch_lbfgs_lds<cgo::dev::UserObjective, " #NPTS ">"});
    CGO_BATCH_LBFGS_LDS_ROWS(ROW)
#undef ROW
    return rtc_build(rtc_program_source_with(m.user_source, m.n_params, more), "cgo_user_objective_batch_lbfgs_lds.hip", wants, m.batch_lbfgs_lds_mod, m.fn, log);
}

}  // namespace cgo
