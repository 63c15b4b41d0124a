// cgo_rtc.hip — "user-supplied element-wise f/∇f" on the GPU path.
//
// The reference takes an arbitrary Julia closure `f = fdf!(g, x)` (src/engine/optim.jl:25,
// src/cg_utils.jl:19).  A host closure cannot run inside a HIP kernel, so the device-side
// equivalent is SOURCE: the user hands over the element-wise body (or a full functor struct),
// and the same kernel templates that serve the built-in objectives (cgo_kernels.hip.hpp,
// cgo_kernels_cg.hip.hpp — embedded in this library as text) are instantiated for it at run time
// with hiprtc for gfx950, with the same flags as the ahead-of-time build (-ffp-contract=off).
#include "cgo_rtc.hpp"

#include <hip/hiprtc.h>

#include <mutex>
#include <tuple>
#include <vector>

#include "cgo_hip_backend.hpp"
#include "cgo_instances.def"
#include "cgo_kernels_cg.hip.hpp"   // the mode bits the rows of cgo_instances.def are written in
#include "cgo_rtc_sources.inc"

namespace cgo {

using namespace dev;

RtcModule::~RtcModule() {
    for (hipModule_t m : mods)
        if (m) (void)hipModuleUnload(m);
}

static std::string key_cg(int mode, int npts, bool big) {
    return "cg:" + std::to_string(mode) + ":" + std::to_string(npts) + ":" + (big ? "1" : "0");
}
static std::string key_fused(int mode, bool big) {
    return "fused:" + std::to_string(mode) + ":" + (big ? "1" : "0");
}
hipFunction_t RtcModule::cg(int mode, int npts, bool big) const {
    auto it = fn.find(key_cg(mode, npts, big));
    return it == fn.end() ? nullptr : it->second;
}
hipFunction_t RtcModule::resident(int npts) const {
    auto it = fn.find("res:" + std::to_string(npts));
    return it == fn.end() ? nullptr : it->second;
}
hipFunction_t RtcModule::spec(bool big, bool push) const {
    auto it = fn.find(std::string("spec:") + (big ? "1" : "0") + (push ? "1" : "0"));
    return it == fn.end() ? nullptr : it->second;
}
hipFunction_t RtcModule::lite(bool big) const {
    auto it = fn.find(std::string("lite:") + (big ? "1" : "0"));
    return it == fn.end() ? nullptr : it->second;
}
hipFunction_t RtcModule::fused(int mode, bool big) const {
    auto it = fn.find(key_fused(mode, big));
    return it == fn.end() ? nullptr : it->second;
}
hipFunction_t RtcModule::row_kernel(const std::string &prefix, const std::vector<int> &rows, int npts) const {
    hipFunction_t f = nullptr;
    for (int r : rows) {
        if (!f || npts >= r) { auto it = fn.find(prefix + std::to_string(r)); if (it != fn.end()) f = it->second; }
    }
    return f;
}

// the embedded kernel templates + the user's objective as one translation unit
std::string rtc_program_source(const std::string &source, int n_params) { return rtc_program_source_with(source, n_params, std::string()); }

// … with `more`, further headers a program of its own needs, between the embedded templates and the user's objective
std::string rtc_program_source_with(const std::string &source, int n_params, const std::string &more) {
    const bool has_param = n_params > 0;
    const std::string K = std::to_string(n_params);
    std::string src;
    for (const char *c : kRtcKernelSourceChunks) src += c;
    src += more;
    src += "\nnamespace cgo { namespace dev {\n";
    if (source.find("struct UserObjective") != std::string::npos) {
        src += source;
        // the slots the struct reads are the slots the objective holds (scalar-p structs: as ever, kParam is taken as given)
        src += "\nstatic_assert(!(ObjParams<UserObjective>::array || " + K + " > 1) || obj_nparams<UserObjective>() == " + K + ",\n"
               "              \"UserObjective: kParams does not match the n_params the objective was created with (" + K + ")\");\n";
    } else if (n_params > 1) {
        // element-wise body with more than one parameter slot: slot 0 is `p`, slots 1–3 are `p1`, `p2`, `p3`
        src += "struct UserObjective {\n";
        src += "    static constexpr int kParams = " + K + ";\n";
        src += "    static constexpr bool kParam = true;\n";
        src += "    static constexpr bool kPairOnly = false;\n";
        src += "    __device__ static inline void eval1(double x, const double (&pv)[" + K + "], double s0, double &f, double &g) {\n";
        src += "        const double p = pv[0]";
        for (int j = 1; j < n_params; ++j) src += ", p" + std::to_string(j) + " = pv[" + std::to_string(j) + "]";
        src += ";\n";
        for (int j = 1; j < n_params; ++j) src += "        (void)p" + std::to_string(j) + ";\n";
        src += "        (void)p;\n        double fi = 0.0, gi = 0.0;\n        {\n" + source + "\n        }\n        f += fi; g = gi;\n    }\n";
        src += "    __device__ static inline void eval2(d2 xx, const d2 (&pp)[" + K + "], double s0, double &f, d2 &gg) {\n";
        src += "        double g0, g1, pa[" + K + "], pb[" + K + "];\n";
        for (int j = 0; j < n_params; ++j) src += "        pa[" + std::to_string(j) + "] = pp[" + std::to_string(j) + "].x; pb[" + std::to_string(j) + "] = pp[" + std::to_string(j) + "].y;\n";
        src += "        eval1(xx.x, pa, s0, f, g0);\n        eval1(xx.y, pb, s0, f, g1);\n";
        src += "        gg.x = g0; gg.y = g1;\n    }\n};\n";
    } else {
        // element-wise body: statements computing `fi` (objective term) and `gi` (its derivative)
        // from `x` (the element), `p` (its parameter, 0 if none) and `s0` (a scalar)
        src += "struct UserObjective {\n";
        src += std::string("    static constexpr bool kParam = ") + (has_param ? "true" : "false") + ";\n";
        src += "    static constexpr bool kPairOnly = false;\n";
        src += "    __device__ static inline void eval1(double x, double p, double s0, double &f, double &g) {\n";
        src += "        double fi = 0.0, gi = 0.0;\n        {\n" + source + "\n        }\n        f += fi; g = gi;\n    }\n";
        src += "    __device__ static inline void eval2(d2 xx, d2 pp, double s0, double &f, d2 &gg) {\n";
        src += "        double g0, g1;\n        eval1(xx.x, pp.x, s0, f, g0);\n        eval1(xx.y, pp.y, s0, f, g1);\n";
        src += "        gg.x = g0; gg.y = g1;\n    }\n};\n";
    }
    src += "\n}}\n";
    return src;
}

// One program → one loaded module: compiles `src` for the name expressions of `wants`, loads the code object as `mod` and
// files every kernel in `fn` under its key.  On failure `mod` is unloaded again and `fn` is as it was.
int rtc_build(const std::string &src, const char *name, const std::vector<Want> &wants, hipModule_t &mod,
              std::map<std::string, hipFunction_t> &fn, std::string &log) {
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), name, 0, nullptr, nullptr) != HIPRTC_SUCCESS) { log = "hiprtcCreateProgram failed"; return CGO_EHIP; }
    for (auto &w : wants) hiprtcAddNameExpression(prog, w.expr.c_str());
    const char *opts[] = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17"};
    const hiprtcResult cr = hiprtcCompileProgram(prog, 4, opts);
    size_t logsz = 0;
    hiprtcGetProgramLogSize(prog, &logsz);
    if (logsz > 1) { log.resize(logsz); hiprtcGetProgramLog(prog, &log[0]); }
    if (cr != HIPRTC_SUCCESS) {
        hiprtcDestroyProgram(&prog);
        if (log.empty()) log = hiprtcGetErrorString(cr);
        return CGO_EINVAL;
    }
    size_t codesz = 0;
    hiprtcGetCodeSize(prog, &codesz);
    std::vector<char> code(codesz);
    hiprtcGetCode(prog, code.data());
    std::string err;
    std::vector<hipFunction_t> fs(wants.size(), nullptr);
    if (hipModuleLoadData(&mod, code.data()) != hipSuccess) { mod = nullptr; err = "hipModuleLoadData failed for the compiled user objective"; }
    for (size_t i = 0; err.empty() && i < wants.size(); ++i) {
        const char *lowered = nullptr;
        if (hiprtcGetLoweredName(prog, wants[i].expr.c_str(), &lowered) != HIPRTC_SUCCESS || !lowered) err = "no lowered name for " + wants[i].expr;
        else if (hipModuleGetFunction(&fs[i], mod, lowered) != hipSuccess) err = std::string("kernel not found in module: ") + lowered;
    }
    hiprtcDestroyProgram(&prog);
    if (!err.empty()) {
        if (mod) { (void)hipModuleUnload(mod); mod = nullptr; }
        log = err;
        return CGO_EHIP;
    }
    for (size_t i = 0; i < wants.size(); ++i) fn[wants[i].key] = fs[i];
    return CGO_OK;
}

// the name expressions of the program every objective compiles at creation (RTC_CREATE): every per-objective row of
// cgo_instances.def for UserObjective
std::vector<Want> rtc_create_wants() {
    std::vector<Want> wants;
    // k_cg and k_fused in both streaming policies
    const std::string uo = "<cgo::dev::UserObjective, ";
    auto tf = [](int b) { return b ? "true" : "false"; };
    for (int big = 0; big < 2; ++big) {
#define ROW(MODE, MAXPTS) \
        for (int npts = 1; npts <= MAXPTS; npts += 2) \
            wants.push_back({key_cg((MODE), npts, big), "cgo::dev::k_cg" + uo + std::to_string((int)(MODE)) + ", " + std::to_string(npts) + ", " + tf(big) + ">"});
        CGO_CG_ROWS(ROW)
#undef ROW
#define ROW(MODE) wants.push_back({key_fused((MODE), big), "cgo::dev::k_fused" + uo + std::to_string((int)(MODE)) + ", " + tf(big) + ">"});
        CGO_FUSED_OBJ_ROWS(ROW)
#undef ROW
    }
    // L-BFGS in one pass over the ring per outer iteration (k_lbfgs_combine_spec, k_lbfgs_push_lite) for this objective: every
    // combination of the kernel's bool arguments, the first argument the first digit of the key
#define ROW(KERNEL, KEY, NBOOLS) \
    for (int bits = 0; bits < (1 << NBOOLS); ++bits) { \
        Want w{KEY ":", "cgo::dev::" #KERNEL "<cgo::dev::UserObjective"}; \
        for (int j = NBOOLS - 1; j >= 0; --j) { w.key += "01"[(bits >> j) & 1]; w.expr += std::string(", ") + tf((bits >> j) & 1); } \
        w.expr += ">"; \
        wants.push_back(w); \
    }
    CGO_RTC_LBFGS_ROWS(ROW)
#undef ROW
    // the resident solver for this objective (cgo_kernels_resident.hip.hpp): whole outer iterations in one launch
#define ROW(NPTS) wants.push_back({"res:" #NPTS, "cgo::dev::k_resident" + uo + #NPTS ">"});
    CGO_RTC_RESIDENT_ROWS(ROW)
#undef ROW
    return wants;
}

int rtc_compile_objective(int device, const std::string &source, int n_params,
                          std::shared_ptr<RtcModule> &out, std::string &log) {
    if (hipSetDevice(device) != hipSuccess) { log = "hipSetDevice failed"; return CGO_EHIP; }
    // A module depends on (device, source, n_params) only, not on the objective's length, and its first program is never changed
    // once loaded: while an objective still holds the module of the same text, the next one shares it instead of compiling for
    // seconds again (the barrier method's two objectives per call, a sweep over sizes).  Not owned here: the last objective
    // unloads it.  (The further programs: rtc_compile_program, under the module's own mutex.)
    static std::mutex mu;
    static std::map<std::tuple<int, int, std::string>, std::weak_ptr<RtcModule>> live;
    const auto key = std::make_tuple(device, n_params, source);
    std::lock_guard<std::mutex> lock(mu);
    if (auto it = live.find(key); it != live.end()) {
        if (auto m = it->second.lock()) { out = m; return CGO_OK; }
        live.erase(it);
    }
    auto mod = std::make_shared<RtcModule>();
    const RtcPlan plan = rtc_program_plan(RTC_CREATE, source, n_params);
    if (int rc = rtc_build(plan.src, plan.name, plan.wants, mod->mods[RTC_CREATE], mod->fn, log)) return rc;
    mod->user_source = source; mod->n_params = n_params; mod->device = device;
    live[key] = mod;
    out = mod;
    return CGO_OK;
}

}  // namespace cgo
