// cgo_rtc_batch.hip — batched solves on a run-time compiled objective: k_batch<UserObjective, NPTS> (cgo_kernels_batch.hip.hpp,
// embedded with the other kernel templates) for the rows of CGO_BATCH_ROWS, and k_batch_grad<UserObjective> beside them, as a
// SECOND program of the objective's module — and k_batch_rows<UserObjective, NPTS> (cgo_kernels_batch_rows.hip.hpp, the tier
// whose problem rows stay in device memory) as a THIRD, compiled on the first solve of that tier only.  The PROBE twins of both
// (cgo_batch_probe) are a FOURTH, compiled on the first probe only.
//
// k_batch is a 512-VGPR kernel that takes hiprtc about as long as k_resident: it is not part of the program every user
// objective compiles at creation (cgo_rtc.hip), but compiled from the kept source on the first batched solve and kept on
// the RtcModule — as the PROBE form of the resident kernel is (rtc_compile_resident_probe).  While one objective of the same
// text lives, every later batched solve finds it there.
#include "cgo_rtc.hpp"

#include <mutex>

#include "cgo_hip_backend.hpp"
#include "cgo_instances.def"

namespace cgo {

#define ROW_NPTS(NPTS) NPTS,   // (for the lookups: the values of a row macro)

hipFunction_t RtcModule::batch(int npts) const { return row_kernel("batch:", {CGO_BATCH_ROWS(ROW_NPTS)}, npts); }

hipFunction_t RtcModule::batch_grad() const {
    auto it = fn.find("batch:grad");
    if (it == fn.end()) it = fn.find("batch_qn:grad");   // (the same kernel in the batched quasi-Newton program, where only that one was compiled)
    return it != fn.end() ? it->second : nullptr;
}

int rtc_compile_batch(RtcModule &m, std::string &log) {
    static std::mutex mu;   // (objectives of one text share the module: two first batched solves must not both build it)
    std::lock_guard<std::mutex> lock(mu);
    if (m.batch_mod) return CGO_OK;
    if (hipSetDevice(m.device) != hipSuccess) { log = "hipSetDevice failed"; return CGO_EHIP; }
    std::vector<Want> wants;
#define ROW(NPTS) wants.push_back({"batch:" #NPTS, "cgo::dev::k_batch<cgo::dev::UserObjective, " #NPTS ">"});
    CGO_BATCH_ROWS(ROW)
#undef ROW
    wants.push_back({"batch:grad", "cgo::dev::k_batch_grad<cgo::dev::UserObjective>"});   // the results' gradient with a scalar per problem
    return rtc_build(rtc_program_source(m.user_source, m.n_params), "cgo_user_objective_batch.hip", wants, m.batch_mod, m.fn, log);
}

hipFunction_t RtcModule::batch_rows(int npts) const { return row_kernel("batch_rows:", {CGO_BATCH_DEVROWS_ROWS(ROW_NPTS)}, npts); }

int rtc_compile_batch_rows(RtcModule &m, std::string &log) {
    static std::mutex mu;   // (as rtc_compile_batch)
    std::lock_guard<std::mutex> lock(mu);
    if (m.rows_mod) return CGO_OK;
    if (hipSetDevice(m.device) != hipSuccess) { log = "hipSetDevice failed"; return CGO_EHIP; }
    std::vector<Want> wants;
#define ROW(NPTS) wants.push_back({"batch_rows:" #NPTS, "cgo::dev::k_batch_rows<cgo::dev::UserObjective, " #NPTS ">"});
    CGO_BATCH_DEVROWS_ROWS(ROW)
#undef ROW
    return rtc_build(rtc_program_source(m.user_source, m.n_params), "cgo_user_objective_batch_rows.hip", wants, m.rows_mod, m.fn, log);
}

// ---- the PROBE twins of both tiers (cgo_batch_probe): a FOURTH program, compiled on the first probe only ----------------------
hipFunction_t RtcModule::batch_probe(bool device_rows, int npts) const {
    return device_rows ? row_kernel("batch_rows_probe:", {CGO_BATCH_DEVROWS_ROWS(ROW_NPTS)}, npts) : row_kernel("batch_probe:", {CGO_BATCH_ROWS(ROW_NPTS)}, npts);
}

int rtc_compile_batch_probe(RtcModule &m, std::string &log) {
    static std::mutex mu;   // (as rtc_compile_batch)
    std::lock_guard<std::mutex> lock(mu);
    if (m.batch_probe_mod) return CGO_OK;
    if (hipSetDevice(m.device) != hipSuccess) { log = "hipSetDevice failed"; return CGO_EHIP; }
    std::vector<Want> wants;
#define ROW(NPTS) wants.push_back({"batch_probe:" #NPTS, "cgo::dev::k_batch<cgo::dev::UserObjective, " #NPTS ", true>"});
    CGO_BATCH_ROWS(ROW)
#undef ROW
#define ROW(NPTS) wants.push_back({"batch_rows_probe:" #NPTS, "cgo::dev::k_batch_rows<cgo::dev::UserObjective, " #NPTS ", true>"});
    CGO_BATCH_DEVROWS_ROWS(ROW)
#undef ROW
    return rtc_build(rtc_program_source(m.user_source, m.n_params), "cgo_user_objective_batch_probe.hip", wants, m.batch_probe_mod, m.fn, log);
}

}  // namespace cgo
