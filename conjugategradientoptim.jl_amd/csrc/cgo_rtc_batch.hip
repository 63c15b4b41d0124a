// cgo_rtc_batch.hip — the further programs of a run-time compiled objective's module (RtcProgram, cgo_rtc.hpp): the PROBE form of
// its resident kernel, and the kernels of batched solves on it — one program per tier and one for the PROBE twins of the two CG
// tiers.  What each program is called, how its failure reads, what text it adds and which kernels it holds are the rows of
// cgo_instances.def (CGO_RTC_PROGRAM_ROWS, CGO_RTC_KERNEL_ROWS, CGO_RTC_EXTRA_ROWS); this file expands them once, into the plan of a
// program (rtc_program_plan: no device needed), the one function that compiles it (rtc_compile_program) and the lookups.
//
// Why programs of their own: k_batch is a 512-VGPR kernel that takes hiprtc about as long as k_resident, and the others are no
// quicker.  None is part of the program every user objective compiles at creation (cgo_rtc.hip); each is compiled from the kept
// source on the first use of what it holds and kept on the RtcModule.  While one objective of the same text lives, every later
// use finds it there.
//
// The text every program is built from (gen_rtc_sources.py, one argument) carries neither the scalar recursion nor the
// quasi-Newton loop.  The batched L-BFGS program adds cgo_qn.hpp, cgo_resident_qn.hpp and its kernel's header
// (cgo_rtc_lbfgs_sources.inc) between that text and the user's objective; its LDS tier's program adds the tier's header behind
// those (cgo_rtc_lbfgs_lds_sources.inc).  Both start with this build's pairs per lane and trip as #defines, so that an A/B
// build's EXTRA reaches the program's text too.
#include "cgo_rtc.hpp"

#include <cstring>

#include "cgo_hip_backend.hpp"
#include "cgo_instances.def"
#include "cgo_kernels_batch_lbfgs.hip.hpp"       // CGO_BATCH_LBFGS_U, CGO_BATCH_LBFGS_U_SLOTS
#include "cgo_kernels_batch_lbfgs_lds.hip.hpp"   // CGO_BATCH_LBFGS_LDS_U, CGO_BATCH_LBFGS_LDS_U_SLOTS
#include "cgo_rtc_lbfgs_sources.inc"
#include "cgo_rtc_lbfgs_lds_sources.inc"

namespace cgo {

#define CGO_STR2(x) #x
#define CGO_STR(x) CGO_STR2(x)
#define ROW_NPTS(NPTS) NPTS,   // (the values of a row macro)

namespace {

enum RtcText { RTC_TEXT_BASE, RTC_TEXT_LBFGS, RTC_TEXT_LBFGS_LDS };
struct ProgramRow { RtcProgram prog; const char *name, *what; RtcText text; };
struct KernelRow { RtcProgram prog; const char *prefix, *kernel; std::vector<int> npts; bool probe; };
struct ExtraRow { RtcProgram prog; const char *key, *kernel; };

const ProgramRow kPrograms[] = {
#define ROW(PROG, NAME, WHAT, TEXT) {PROG, NAME, WHAT, TEXT},
    CGO_RTC_PROGRAM_ROWS(ROW)
#undef ROW
};
const std::vector<KernelRow> kKernels = {
#define ROW(PROG, PREFIX, KERNEL, ROWS, PROBE) {PROG, PREFIX, #KERNEL, {ROWS(ROW_NPTS)}, PROBE != 0},
    CGO_RTC_KERNEL_ROWS(ROW)
#undef ROW
};
const ExtraRow kExtras[] = {
#define ROW(PROG, KEY, KERNEL) {PROG, KEY, #KERNEL},
    CGO_RTC_EXTRA_ROWS(ROW)
#undef ROW
};
static_assert(sizeof kPrograms / sizeof kPrograms[0] == RTC_PROGRAMS, "one row of CGO_RTC_PROGRAM_ROWS per RtcProgram");

const ProgramRow &program_row(RtcProgram prog) {
    const ProgramRow &r = kPrograms[prog];   // (the rows are in the enum's order)
    return r.prog == prog ? r : kPrograms[RTC_CREATE];
}

// what follows the embedded kernel templates in a program's text
std::string program_text(RtcText text) {
    if (text == RTC_TEXT_BASE) return std::string();
    std::string more = rtc_batch_lbfgs_defines();
    if (text == RTC_TEXT_LBFGS_LDS) more += "#define CGO_BATCH_LBFGS_LDS_U " CGO_STR(CGO_BATCH_LBFGS_LDS_U) "\n#define CGO_BATCH_LBFGS_LDS_U_SLOTS " CGO_STR(CGO_BATCH_LBFGS_LDS_U_SLOTS) "\n";
    for (const char *c : kRtcLbfgsSourceChunks) more += c;
    if (text == RTC_TEXT_LBFGS_LDS) {
        more += "\n";
        for (const char *c : kRtcLbfgsLdsSourceChunks) more += c;
    }
    return more;
}

}  // namespace

std::string rtc_batch_lbfgs_defines() {
    return "\n#define CGO_BATCH_LBFGS_U " CGO_STR(CGO_BATCH_LBFGS_U) "\n#define CGO_BATCH_LBFGS_U_SLOTS " CGO_STR(CGO_BATCH_LBFGS_U_SLOTS) "\n";
}

const char *rtc_program_what(RtcProgram prog) { return program_row(prog).what; }

RtcPlan rtc_program_plan(RtcProgram prog, const std::string &source, int n_params) {
    const ProgramRow &row = program_row(prog);
    RtcPlan plan{row.name, rtc_program_source_with(source, n_params, program_text(row.text)), {}};
    if (prog == RTC_CREATE) { plan.wants = rtc_create_wants(); return plan; }
    for (const KernelRow &k : kKernels) {
        if (k.prog != prog) continue;
        for (int npts : k.npts) {
            const std::string n = std::to_string(npts);
            plan.wants.push_back({k.prefix + n, std::string("cgo::dev::") + k.kernel + "<cgo::dev::UserObjective, " + n + (k.probe ? ", true>" : ">")});
        }
    }
    for (const ExtraRow &e : kExtras)
        if (e.prog == prog) plan.wants.push_back({e.key, std::string("cgo::dev::") + e.kernel + "<cgo::dev::UserObjective>"});
    return plan;
}

int rtc_compile_program(RtcModule &m, RtcProgram prog, std::string &log) {
    if (prog <= RTC_CREATE || prog >= RTC_PROGRAMS) { log = "no such program of a run-time compiled objective"; return CGO_EINVAL; }
    std::lock_guard<std::mutex> lock(m.mu);
    if (m.mods[prog]) return CGO_OK;
    if (hipSetDevice(m.device) != hipSuccess) { log = "hipSetDevice failed"; return CGO_EHIP; }
    const RtcPlan plan = rtc_program_plan(prog, m.user_source, m.n_params);
    return rtc_build(plan.src, plan.name, plan.wants, m.mods[prog], m.fn, log);
}

// ---- the lookups: the row of the table for npts, by the rule of the ahead-of-time dispatch ------------------------------------
hipFunction_t RtcModule::kernel(RtcProgram prog, const char *prefix, int npts) const {
    for (const KernelRow &k : kKernels)
        if (k.prog == prog && !std::strcmp(k.prefix, prefix)) return row_kernel(k.prefix, k.npts, npts);
    return nullptr;
}
hipFunction_t RtcModule::resident_probe(int npts) const { return kernel(RTC_RESIDENT_PROBE, "resprobe:", npts); }
hipFunction_t RtcModule::batch(int npts) const { return kernel(RTC_BATCH, "batch:", npts); }
hipFunction_t RtcModule::batch_rows(int npts) const { return kernel(RTC_BATCH_ROWS, "batch_rows:", npts); }
hipFunction_t RtcModule::batch_probe(bool device_rows, int npts) const { return kernel(RTC_BATCH_PROBE, device_rows ? "batch_rows_probe:" : "batch_probe:", npts); }
hipFunction_t RtcModule::batch_lbfgs(int npts) const { return kernel(RTC_BATCH_LBFGS, "batch_qn:", npts); }
hipFunction_t RtcModule::batch_lbfgs_lds(int npts) const { return kernel(RTC_BATCH_LBFGS_LDS, "batch_qn_lds:", npts); }
hipFunction_t RtcModule::batch_grad() const {   // the first program of the table that has it loaded
    for (const ExtraRow &e : kExtras)
        if (auto it = fn.find(e.key); it != fn.end()) return it->second;
    return nullptr;
}

}  // namespace cgo
