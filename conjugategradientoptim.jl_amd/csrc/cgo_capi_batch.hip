// cgo_capi_batch.hip — the batched part of the extern "C" boundary (include/cgo.h): many small problems in one launch, a
// workgroup each.  Every rule an entry point refuses a call by is ONE function here and takes the words the refusal starts with
// (kCG, kLB or kPR); an entry point is the list of its phases, in the order that decides which error a doubly wrong call gets:
// null arguments, policy, objective, m_max, config and call shape, built-in shape rules or the model's params, scalars, active,
// tier (the LDS tier's program compiled just before its limit is read), memory, remaining programs, allocation.
// No kernel and no kernel header: the tiers live behind HipBackend (cgo_backend_batch*.hip).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>

#include "cgo_capi_internal.hpp"
#include "cgo_qn.hpp"

using namespace cgo;

static const char *const kCG = "batched solves", *const kLB = "batched L-BFGS solves", *const kPR = "batch probe";
static int refuse(int rc, const std::string &msg) { set_error(msg); return rc; }

// ---- the rules ---------------------------------------------------------------------------------------------------------------
static bool batch_kind(int32_t k) { return k == CGO_OBJ_QUAD_DIAG || k == CGO_OBJ_ROSENBROCK_PAIRED || k == CGO_OBJ_BOOTH; }
static int check_builtin_kind(const char *who, int32_t kind, bool or_model) {
    if (batch_kind(kind)) return CGO_OK;
    return refuse(CGO_EINVAL, std::string(who) + ": the objective must be CGO_OBJ_QUAD_DIAG, CGO_OBJ_ROSENBROCK_PAIRED" + (or_model ? ", CGO_OBJ_BOOTH or a model" : " or CGO_OBJ_BOOTH"));
}
// the built-in problem's shape; `d_name`: what the call names the rows of D
static int check_builtin_rules(const char *who, int32_t kind, int64_t n, const double *D, const char *d_name) {
    const std::string w(who);
    if (kind == CGO_OBJ_ROSENBROCK_PAIRED && n % 2 != 0) return refuse(CGO_EINVAL, w + ": paired Rosenbrock needs an even n");
    if (kind == CGO_OBJ_BOOTH && n != 2) return refuse(CGO_EINVAL, w + ": Booth is 2-dimensional (n = 2)");
    if (kind == CGO_OBJ_QUAD_DIAG && !D) return refuse(CGO_EINVAL, w + ": the quadratic needs " + d_name + ", the [batch*n] rows of D");
    return CGO_OK;
}
// … and its concatenated objective `cat`: n_local = batch · ld, the quadratic's slot allocated
static int builtin_cat(cgo_ctx *ctx, int32_t kind, int64_t n, int64_t batch, HipObjective &cat) {
    const int64_t ld = n + (n & 1);
    cat.ctx = &ctx->c; cat.kind = kind; cat.n_global = cat.n_local = batch * ld; cat.offset = 0;
    if (cat.uses_param()) { if (int rc = cat.p[0].alloc((size_t)(batch * ld))) return rc; }
    return CGO_OK;
}
static std::function<int(cgo_objective **)> builtin_hobj(cgo_ctx *ctx, int32_t kind, int64_t n) {
    return [=](cgo_objective **h) { return cgo_objective_create(ctx, kind, n, 0, n, h); };
}

// the rows a call asks for: a null policy is the call without one — `dflt`, the family's
static int batch_rows_asked(const cgo_batch_policy *pol, int dflt, const char *who, int &rows) {
    rows = dflt;
    if (!pol) return CGO_OK;
    REQUIRE(pol->size == (int32_t)sizeof(cgo_batch_policy), "cgo_batch_policy.size does not match this library (call cgo_batch_policy_init first)");
    if (pol->rows != CGO_BATCH_ROWS_LDS && pol->rows != CGO_BATCH_ROWS_DEVICE && pol->rows != CGO_BATCH_ROWS_AUTO)
        return refuse(CGO_EINVAL, std::string(who) + ": cgo_batch_policy.rows must be CGO_BATCH_ROWS_LDS, CGO_BATCH_ROWS_DEVICE or CGO_BATCH_ROWS_AUTO");
    rows = pol->rows;
    return CGO_OK;
}

static int check_one_rank(cgo_ctx *ctx, const char *who) {
    if (ctx->c.world() != 1) return refuse(CGO_EINVAL, std::string(who) + ": a multi-rank context is not supported (one rank only)");
    return CGO_OK;
}
// the shape of a call (an open has no slice: 0)
static int check_batch_shape(cgo_ctx *ctx, const char *who, int64_t n, int64_t batch, int64_t slice_iters) {
    const std::string w(who);
    if (int rc = check_one_rank(ctx, who)) return rc;
    if (batch < 1) return refuse(CGO_EINVAL, w + ": batch must be ≥ 1");
    if (batch > 0x7FFFFFFF) return refuse(CGO_EINVAL, w + ": batch exceeds the largest grid");
    if (slice_iters < 0) return refuse(CGO_EINVAL, w + ": slice_iters must be ≥ 0 (0 = the library's policy)");
    if (n < 1) return refuse(CGO_EINVAL, w + ": n must be ≥ 1");
    return CGO_OK;
}
static int check_lbfgs_m(const char *who, int m) {
    if (m > QN_MAX_M) return refuse(CGO_EINVAL, std::string(who) + ": m = " + std::to_string(m) + " exceeds cgo_batch_lbfgs_max_m = " + std::to_string(QN_MAX_M));
    return CGO_OK;
}
// What every solve refuses of a config and a call: a config the device loop does not run, then the shape.  `cg_entry`: null for
// the CG flavours' calls; for an L-BFGS call, where a CG flavour belongs instead.
static int check_batch_call(cgo_ctx *ctx, const char *cg_entry, const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t n, int64_t batch, int64_t slice_iters) {
    std::string why;
    if (int rc = check_cg_config(cfg, why)) return refuse(rc, why);
    if (int rc = check_ls_config(ls, why)) return refuse(rc, why);
    if (!cg_entry) {
        if (int rc = check_batch_config(*cfg, *ls, why)) return refuse(rc, why);
        return check_batch_shape(ctx, kCG, n, batch, slice_iters);
    }
    if (cfg->beta.kind != CGO_BETA_LBFGS) return refuse(CGO_EINVAL, std::string("batched L-BFGS solves: β must be LBFGS(m) (CG flavours: ") + cg_entry + "; the Broyden family has no batched form)");
    if (int rc = check_lbfgs_m(kLB, cfg->beta.lbfgs_m)) return rc;
    REQUIRE(ls->kind != CGO_LS_BACKTRACKING, "batched L-BFGS solves: the Backtracking line search is not supported (StrongWolfeBisection or WolfeBisection)");
    return check_batch_shape(ctx, kLB, n, batch, slice_iters);
}

static int check_scalars(const char *who, const double *scalars, int64_t batch) {
    for (int64_t b = 0; scalars && b < batch; ++b)
        if (!std::isfinite(scalars[b])) return refuse(CGO_EINVAL, std::string(who) + ": scalars[" + std::to_string(b) + "] is not finite");
    return CGO_OK;
}
static int check_active(const char *who, const unsigned char *active, int64_t batch) {
    if (!active) return CGO_OK;
    for (int64_t b = 0; b < batch; ++b) if (active[b] != 0) return CGO_OK;
    return refuse(CGO_EINVAL, std::string(who) + ": active selects no problem");
}

// `need` bytes of `what` (prefix and subject) of that shape against the device's free memory, before anything is allocated
static int check_device_memory(const std::string &what, int64_t batch, int64_t n, double need) {
    size_t free_b = 0, total_b = 0;
    HIPCHK2(hipMemGetInfo(&free_b, &total_b));
    if (need <= (double)free_b) return CGO_OK;
    char buf[160];
    std::snprintf(buf, sizeof buf, " of %lld problems of n = %lld ask for %.0f bytes of device memory, %zu are free", (long long)batch, (long long)n, need, free_b);
    return refuse(CGO_ENOMEM, what + buf);
}

// Is this a whole, single-rank, run-time compiled model?  (the limit queries answer 0 otherwise; check_batch_model says why)
static bool batch_model_whole(const cgo_objective *m) { return m->o.offset == 0 && m->o.n_local == m->o.n_global && m->o.ctx->world() == 1; }
static bool batch_model_ok(const cgo_objective *m) { return m && m->o.kind == CGO_OBJ_USER && m->o.rtc && batch_model_whole(m); }
static int check_batch_model(cgo_ctx *ctx, cgo_objective *model) {
    REQUIRE(model->o.kind == CGO_OBJ_USER && model->o.rtc,
            "batched solves: the model must be a run-time compiled objective (cgo_objective_create_from_source[_ex]); built-in objectives: cgo_minimize_batch");
    REQUIRE(model->o.ctx == &ctx->c, "batched solves: the model belongs to another context");
    REQUIRE(batch_model_whole(model), "batched solves: a sharded or multi-rank model is not supported (n_global = n_local = the size of ONE problem, one rank only)");
    return CGO_OK;
}
static int check_batch_model_params(cgo_objective *model, const double *const *params, int32_t n_params) {
    const int K = model->o.nparams();
    if (n_params != K) return refuse(CGO_EINVAL, "batched solves: n_params = " + std::to_string(n_params) + ", the model reads " + std::to_string(K) + " parameter slots");
    REQUIRE(K == 0 || params, "batched solves: params is null, the model reads parameter slots");
    for (int j = 0; j < K; ++j)
        if (!params[j]) return refuse(CGO_EINVAL, "batched solves: params[" + std::to_string(j) + "] is null (the [batch*n] rows of slot " + std::to_string(j) + ")");
    return CGO_OK;
}

// A batched program of a model's module (RtcProgram, cgo_rtc.hpp), compiled on the first use of its tier on the module
static int batch_program(cgo_objective *model, RtcProgram which) {
    std::string log;
    if (int rc = rtc_compile_program(*model->o.rtc, which, log)) return refuse(rc, std::string("user objective: ") + rtc_program_what(which) + " did not compile:\n" + log);
    return CGO_OK;
}

// what one workgroup's LDS holds of a built-in problem: its rows (m = 0) or its rows and a ring for m pairs (0: no context, kind
// or device, a bad m); Booth has two variables whatever fits
static int64_t builtin_lds_max_n(cgo_ctx *ctx, int32_t obj_kind, int32_t m) {
    if (!ctx || !batch_kind(obj_kind)) return 0;
    const int64_t ld = m > 0 ? HipBackend::batch_lbfgs_lds_max_ld(&ctx->c, obj_kind, m) : HipBackend::batch_max_n(&ctx->c, obj_kind);
    return obj_kind == CGO_OBJ_BOOTH ? std::min<int64_t>(ld, 2) : ld;
}

// (lanes per workgroup, pairs of elements per lane and trip) of a tier's streaming loop, to the pointers the caller gave
static void shape_out(int32_t *block, int32_t *pairs_per_trip, int b, int u) {
    if (block) *block = b;
    if (pairs_per_trip) *pairs_per_trip = u;
}

// ---- limits and shapes ---------------------------------------------------------------------------------------------------------
extern "C" {

int64_t cgo_batch_max_n(cgo_ctx *ctx, int32_t obj_kind) { return builtin_lds_max_n(ctx, obj_kind, 0); }

int32_t cgo_stop_status(int64_t it, int64_t max_iters, double f_x, double grad_norm, double eps, double f_x0, int64_t *iters_ran) {
    int64_t ran = 0;
    const int st = stop_status(it, max_iters, f_x, grad_norm, eps, f_x0, ran);
    if (iters_ran) *iters_ran = ran;
    return st;
}

// where a batch's rows live (cgo_batch_policy): LDS (k_batch) or device memory (k_batch_rows)
void cgo_batch_policy_init(cgo_batch_policy *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->size = (int32_t)sizeof(*p);
    p->rows = CGO_BATCH_ROWS_LDS;
}

void cgo_batch_rows_shape(int32_t *block, int32_t *pairs_per_trip) { shape_out(block, pairs_per_trip, HipBackend::batch_rows_block(), HipBackend::batch_rows_unroll()); }

int64_t cgo_batch_max_n_ex(cgo_ctx *ctx, int32_t obj_kind, const cgo_batch_policy *policy) {
    int rows = 0;
    if (batch_rows_asked(policy, CGO_BATCH_ROWS_LDS, kCG, rows)) return 0;
    const int64_t lds = cgo_batch_max_n(ctx, obj_kind);
    if (rows == CGO_BATCH_ROWS_LDS || lds == 0) return lds;
    return obj_kind == CGO_OBJ_BOOTH ? lds : HipBackend::batch_rows_max_n();
}

int64_t cgo_batch_max_n_obj(cgo_objective *model) {
    try {
        if (!batch_model_ok(model) || batch_program(model, RTC_BATCH)) return 0;
        return HipBackend::batch_max_n(model->o.ctx, CGO_OBJ_USER, model->o.rtc.get());
    } catch (...) { return 0; }
}

int64_t cgo_batch_max_n_obj_ex(cgo_objective *model, const cgo_batch_policy *policy) {
    try {
        int rows = 0;
        if (batch_rows_asked(policy, CGO_BATCH_ROWS_LDS, kCG, rows)) return 0;
        if (rows == CGO_BATCH_ROWS_LDS) return cgo_batch_max_n_obj(model);
        return batch_model_ok(model) ? HipBackend::batch_rows_max_n() : 0;   // (nothing is compiled for the answer)
    } catch (...) { return 0; }
}

// β = LBFGS(m): k_batch_lbfgs, the ring of every problem in device memory (k_batch_lbfgs_lds: in LDS)
int32_t cgo_batch_lbfgs_max_m(void) { return QN_MAX_M; }

void cgo_batch_lbfgs_shape(int32_t *block, int32_t *pairs_per_trip) { shape_out(block, pairs_per_trip, HipBackend::batch_lbfgs_block(), HipBackend::batch_lbfgs_unroll()); }
void cgo_batch_lbfgs_shape_obj(int32_t n_params, int32_t *block, int32_t *pairs_per_trip) {
    shape_out(block, pairs_per_trip, HipBackend::batch_lbfgs_block(), HipBackend::batch_lbfgs_unroll_for(n_params));
}
void cgo_batch_lbfgs_lds_shape(int32_t n_params, int32_t *block, int32_t *pairs_per_trip) {
    shape_out(block, pairs_per_trip, HipBackend::batch_lbfgs_block(), HipBackend::batch_lbfgs_lds_unroll_for(n_params));
}
int32_t cgo_batch_lbfgs_lds_rows(int32_t n_params, int32_t m) { return HipBackend::batch_lbfgs_lds_rows(n_params, m); }

int64_t cgo_batch_lbfgs_max_n(cgo_ctx *ctx, int32_t obj_kind) {
    const int64_t lds = cgo_batch_max_n(ctx, obj_kind);   // (0: no context, no such kind, no device)
    if (lds == 0) return 0;
    return obj_kind == CGO_OBJ_BOOTH ? lds : HipBackend::batch_lbfgs_max_n();
}

int64_t cgo_batch_lbfgs_max_n_obj(cgo_objective *model) {
    try {
        return batch_model_ok(model) ? HipBackend::batch_lbfgs_max_n() : 0;   // (nothing is compiled for the answer)
    } catch (...) { return 0; }
}

int64_t cgo_batch_lbfgs_max_n_ex(cgo_ctx *ctx, int32_t obj_kind, int32_t m, const cgo_batch_policy *policy) {
    try {
        int rows = 0;
        if (batch_rows_asked(policy, CGO_BATCH_ROWS_DEVICE, kLB, rows)) return 0;
        if (m < 1 || m > QN_MAX_M) return 0;
        if (rows == CGO_BATCH_ROWS_LDS) return builtin_lds_max_n(ctx, obj_kind, m);
        return cgo_batch_lbfgs_max_n(ctx, obj_kind);
    } catch (...) { return 0; }
}

int64_t cgo_batch_lbfgs_max_n_obj_ex(cgo_objective *model, int32_t m, const cgo_batch_policy *policy) {
    try {
        int rows = 0;
        if (batch_rows_asked(policy, CGO_BATCH_ROWS_DEVICE, kLB, rows)) return 0;
        if (m < 1 || m > QN_MAX_M) return 0;
        if (rows != CGO_BATCH_ROWS_LDS) return cgo_batch_lbfgs_max_n_obj(model);   // (nothing is compiled for the answer)
        // (as cgo_batch_max_n_obj compiles the batch program: the limit follows from the kernel's static LDS)
        if (!batch_model_ok(model) || batch_program(model, RTC_BATCH_LBFGS_LDS)) return 0;
        return HipBackend::batch_lbfgs_lds_max_ld(model->o.ctx, CGO_OBJ_USER, m, model->o.rtc.get());
    } catch (...) { return 0; }
}

}  // extern "C"

// ---- tiers ---------------------------------------------------------------------------------------------------------------------
// The tier a batch of problems of size n runs in.  lds_max: what one workgroup's LDS holds of this objective (`lds_name` reports
// it); beyond the LDS tier the limits are the pass index and the device's free memory.  (The probe reports these in a solve's words.)
static int batch_tier(int rows, int64_t n, int64_t batch, int nparams, int64_t lds_max, const char *lds_name, bool &device_rows) {
    device_rows = rows == CGO_BATCH_ROWS_DEVICE || (rows == CGO_BATCH_ROWS_AUTO && n > lds_max);
    if (!device_rows) {
        if (n > lds_max) return refuse(CGO_EINVAL, "batched solves: n = " + std::to_string(n) + " exceeds what one workgroup's LDS holds (" + lds_name + " = " + std::to_string(lds_max) + ")");
        return CGO_OK;
    }
    const int64_t max_n = HipBackend::batch_rows_max_n();
    if (n > max_n) return refuse(CGO_EINVAL, "batched solves: n = " + std::to_string(n) + " exceeds the index range of a pass over rows in device memory (cgo_batch_max_n_ex = " + std::to_string(max_n) + ")");
    return check_device_memory("batched solves: the rows", batch, n, HipBackend::batch_rows_bytes(batch, n, nparams));
}

// THE rule of CGO_BATCH_ROWS_AUTO for batched L-BFGS (stated in include/cgo.h): device rows.  "LDS where n fits" needed the LDS
// tier's kernel time below the device tier's by more than that tier's own spread at EVERY measured shape, and at n = 1000, m = 5
// it is not.  true: LDS where n fits for this m and slot count.
static constexpr bool kBatchLbfgsAutoTakesLds = false;
// the tier of a batched L-BFGS solve: lds_max = what one workgroup's LDS holds for this m and slot count
static int batch_lbfgs_tier(int rows, int64_t n, int64_t lds_max, bool &lds, const char *lds_name = "cgo_batch_lbfgs_max_n_ex") {
    lds = rows == CGO_BATCH_ROWS_LDS || (rows == CGO_BATCH_ROWS_AUTO && kBatchLbfgsAutoTakesLds && n <= lds_max);
    if (lds && n > lds_max)
        return refuse(CGO_EINVAL, "batched L-BFGS solves: n = " + std::to_string(n) + " exceeds what one workgroup's LDS holds of a problem's rows and ring (" + lds_name + " = " + std::to_string(lds_max) + ")");
    return CGO_OK;
}
// What a batched L-BFGS solve and its probe refuse of sizes alike: n beyond the pass index, and rows and rings the device's free
// memory does not hold — (3 + K + 2(m+1)) · batch · ld · 8 bytes against what is free, before anything is allocated.
static int batch_lbfgs_sizes_of(cgo_ctx *ctx, int64_t max_n, const char *max_name, int nparams, int64_t n, int64_t batch, int m) {
    HIPCHK2(hipSetDevice(ctx->c.device));
    if (n > max_n) return refuse(CGO_EINVAL, "batched L-BFGS solves: n = " + std::to_string(n) + " exceeds the index range of a pass (" + max_name + " = " + std::to_string(max_n) + ")");
    return check_device_memory("batched L-BFGS solves: the rows and rings (m = " + std::to_string(m) + ")", batch, n, HipBackend::batch_lbfgs_bytes(batch, n, nparams, m));
}
static int batch_lbfgs_sizes(cgo_ctx *ctx, int32_t obj_kind, int64_t n, int64_t batch, int m) {
    return batch_lbfgs_sizes_of(ctx, cgo_batch_lbfgs_max_n(ctx, obj_kind), "cgo_batch_lbfgs_max_n", obj_kind == CGO_OBJ_QUAD_DIAG ? 1 : 0, n, batch, m);
}
// The plan of an L-BFGS batch on a model, one-shot or kept: the tier (its program first: its static LDS decides the limit
// `lds_name` reports), the sizes, then the device tier's program — compiled here, so that a solve on a handle never compiles.
static int batch_lbfgs_model_plan(cgo_ctx *ctx, cgo_objective *model, int rows, int64_t batch, int m, const char *lds_name, bool &lds) {
    const int64_t n = model->o.n_local;
    lds = false;
    if (rows != CGO_BATCH_ROWS_DEVICE && (rows == CGO_BATCH_ROWS_LDS || kBatchLbfgsAutoTakesLds)) {
        HIPCHK2(hipSetDevice(ctx->c.device));
        if (int rc = batch_program(model, RTC_BATCH_LBFGS_LDS)) return rc;
        if (int rc = batch_lbfgs_tier(rows, n, HipBackend::batch_lbfgs_lds_max_ld(&ctx->c, CGO_OBJ_USER, m, model->o.rtc.get()), lds, lds_name)) return rc;
    }
    if (int rc = batch_lbfgs_sizes_of(ctx, cgo_batch_lbfgs_max_n_obj(model), "cgo_batch_lbfgs_max_n_obj", model->o.nparams(), n, batch, m)) return rc;
    return lds ? CGO_OK : batch_program(model, RTC_BATCH_LBFGS);
}

// ---- the batch itself ------------------------------------------------------------------------------------------------------------
// The concatenated problems: ONE objective `cat` (n_local = batch · ld, its parameter slots allocated) and backend whose x, u and
// parameter slots are the [batch][ld] rows.  A model's `cat` shares its compiled module, its scalar and its cost class; the slots
// are its own rows.
static int batch_model_cat_rows(cgo_ctx *ctx, cgo_objective *model, int64_t batch, HipObjective &cat) {
    const int64_t n = model->o.n_local, ld = n + (n & 1);
    const int K = model->o.nparams();
    cat.ctx = &ctx->c; cat.kind = CGO_OBJ_USER; cat.n_global = cat.n_local = batch * ld; cat.offset = 0;
    cat.rtc = model->o.rtc; cat.user_nparams = K; cat.s0 = model->o.s0; cat.user_cheap = model->o.user_cheap;
    for (int j = 0; j < K; ++j) { if (int rc = cat.p[j].alloc((size_t)(batch * ld))) return rc; }
    return CGO_OK;
}
// … of a CG batch on a model, from its params on: params, tier, memory, the device tier's program, the rows
static int batch_model_cat(cgo_ctx *ctx, cgo_objective *model, int64_t batch, const double *const *params, int32_t n_params, HipObjective &cat,
                           int rows, bool &device_rows) {
    if (int rc = check_batch_model_params(model, params, n_params)) return rc;
    HIPCHK2(hipSetDevice(ctx->c.device));
    // (rows in device memory, asked for outright: the batch program — the LDS tier's kernel — is neither needed nor compiled)
    int64_t lds_max = 0;
    if (rows != CGO_BATCH_ROWS_DEVICE) {
        if (int rc = batch_program(model, RTC_BATCH)) return rc;
        lds_max = HipBackend::batch_max_n(&ctx->c, CGO_OBJ_USER, model->o.rtc.get());
    }
    if (int rc = batch_tier(rows, model->o.n_local, batch, model->o.nparams(), lds_max, "cgo_batch_max_n_obj", device_rows)) return rc;
    if (device_rows) { if (int rc = batch_program(model, RTC_BATCH_ROWS)) return rc; }
    return batch_model_cat_rows(ctx, model, batch, cat);
}
// the objective of size n a handed-back problem of a model is finished on
static std::function<int(cgo_objective **)> batch_model_hobj(cgo_ctx *ctx, cgo_objective *model) {
    return [ctx, model](cgo_objective **h) {
        // (the module cache makes this free while the model lives: same device, text and n_params)
        const int64_t n = model->o.n_local;
        if (int rc = cgo_objective_create_from_source_ex(ctx, model->o.rtc->user_source.c_str(), model->o.nparams(), n, 0, n, h)) return rc;
        (*h)->o.s0 = model->o.s0; (*h)->o.user_cheap = model->o.user_cheap;
        return (int)CGO_OK;
    };
}
// the backend of `cat` with the slot rows uploaded; m > 0: the ring of a batched L-BFGS solve beside them
static int batch_backend_on(cgo_ctx *ctx, int64_t n, int64_t batch, const double *const *params, HipBackend &be, bool device_rows, int m = 0, bool lds = false) {
    cgo_solver_policy pol;
    { std::string pw; if (int rc = resolve_policy(ctx, nullptr, pol, pw)) return refuse(rc, pw); }
    be.set_policy(pol);
    be.set_rmode(true);
    if (int rc = be.alloc()) return rc;
    if (int rc = be.batch_alloc(batch, n, params, device_rows)) return rc;
    return m > 0 ? be.batch_lbfgs_alloc(m, lds) : CGO_OK;
}

// One solve.  `be`: the backend of a handle; null for a one-shot call, whose backend is made here on `cat` (device_rows, and for
// L-BFGS the ring of qn.m in qn.lds) and lives for the call.  `params`: the caller's slot rows — a one-shot call's; null on a handle,
// where they were valid during open only.  `make_hobj`: the objective of size n the handed-back problems are finished on.
// qn.m > 0: a batched L-BFGS solve — every ring empty at the start with THIS solve's m on a ring allocated for at least as much,
// and a handed-back problem is solved again by the host engine from its own x0 (the ring and Gram state of the device are not
// exported), with its row of the caller's x0 and of every slot of `params` (qn.nparams of them; a quasi-Newton solver keeps a
// stored gradient: not a backend batch_export_row serves) or, on a handle, of the batch's own device rows (batch_export_slots).
struct BatchSolve {
    cgo_ctx *ctx;
    HipBackend *be; HipObjective *cat; bool device_rows;
    int64_t n, batch;
    const double *x0; const double *const *params; const double *scalars; const unsigned char *active;
    const cgo_cg_config *cfg; const cgo_ls_config *ls; int64_t slice_iters;
    cgo_batch_results *out;
    std::function<int(cgo_objective **)> make_hobj;
    struct { int m, nparams; bool lds; } qn;
};

// Launched until every active problem is finished or handed back, then everything after the launch loop: statuses from
// stop_status, traces, and the hand-back of the problems the device loop does not finish to ONE ordinary solver on make_hobj's
// objective (created on the first hand-back), which takes the problem's own scalar where the call has them.
static int batch_solve_on(const BatchSolve &c) {
    const int64_t n = c.n, batch = c.batch;
    const cgo_cg_config *cfg = c.cfg;
    cgo_batch_results *out = c.out;
    std::unique_ptr<HipBackend> own;
    if (!c.be) {
        own.reset(new HipBackend(&c.ctx->c, c.cat));
        if (int rc = batch_backend_on(c.ctx, n, batch, c.params, *own, c.device_rows, c.qn.m, c.qn.lds)) return rc;
    }
    HipBackend &be = c.be ? *c.be : *own;
    auto on = [&](int64_t b) { return !c.active || c.active[b] != 0; };
    if (int rc = be.batch_reset(c.x0, c.scalars, c.active, cfg->max_iters, cfg->trace_enabled != 0)) return rc;
    if (c.qn.m > 0) { if (int rc = be.batch_lbfgs_reset(c.qn.m)) return rc; }
    BatchRun run;
    if (int rc = run_batch(&be, *cfg, *c.ls, batch, c.slice_iters, run)) { if (rc == CGO_ESTATE) set_error("internal: a batched launch left a problem in a state the driver does not know"); return rc; }
    out->launches = run.launches;
    // finished on the device: the status follows from the state (stop_status); minimizer and gradient of EVERY row from one
    // download — the rows the host engine finishes below are overwritten with its own
    if (int rc = be.batch_results(out->minimizer, out->gradient, c.active)) return rc;
    const bool trace = cfg->trace_enabled != 0;
    const int64_t mi = cfg->max_iters;
    std::vector<ResRecord> recs;
    const bool want_trace = trace && (out->trace_objective || out->trace_grad_norm || out->trace_step_size || out->trace_objective_evals);
    if (want_trace) { if (int rc = be.batch_records(-1, 1, recs)) return rc; }
    const int64_t stride = be.batch_rec_stride();
    for (int64_t b = 0; b < batch; ++b) {
        const ResState &s = run.st[(size_t)b];
        if (s.reason != RES_STOP || !on(b)) continue;
        int64_t ran = 0;
        const int st = stop_status(s.it, mi, s.f_x, s.norm, cfg->eps, run.f_x0[(size_t)b], ran);
        if (st == CGO_INCOMPLETE) { set_error("internal: a batched problem stopped on the device in a state that does not stop"); return CGO_ESTATE; }
        if (out->objective) out->objective[b] = s.f_x;
        if (out->iters_ran) out->iters_ran[b] = ran;
        if (out->status) out->status[b] = st;
        if (out->total_fdf_evals) out->total_fdf_evals[b] = 1 + run.evals[(size_t)b];
        if (want_trace)
            for (int64_t i = 0; i < s.it; ++i) {
                const ResRecord &r = recs[(size_t)(b * stride + i)];
                if (out->trace_objective) out->trace_objective[b * mi + i] = r.f;
                if (out->trace_grad_norm) out->trace_grad_norm[b * mi + i] = r.norm;
                if (out->trace_step_size) out->trace_step_size[b * mi + i] = r.a;
                if (out->trace_objective_evals) out->trace_objective_evals[b * mi + i] = r.evals;
            }
    }
    // handed back: the iteration at st.it + 1 is the host engine's — ONE ordinary solver (no resident slices), reused
    cgo_objective *hobj = nullptr;
    cgo_solver *hs = nullptr;
    int rc = CGO_OK;
    for (int64_t b = 0; b < batch && !rc; ++b) {
        const ResState &s = run.st[(size_t)b];
        if (s.reason != RES_HOST || !on(b)) continue;
        if (!hs) {
            if ((rc = c.make_hobj(&hobj))) break;
            cgo_solver_policy hp;
            cgo_solver_policy_init(&hp);
            hp.resident = 0;
            if ((rc = make_solver(c.ctx, hobj, cfg, c.ls, nullptr, &hp, &hs))) break;
        }
        if (c.scalars) { if ((rc = cgo_objective_set_scalar(hobj, 0, c.scalars[b]))) break; }   // (the call's own objective, never the model)
        if (c.qn.m > 0) {       // the whole solve, from the problem's own x0 (the device's row of x has moved on)
            if (!c.params) rc = be.batch_export_slots(b, *hs->be);
            for (int j = 0; c.params && j < c.qn.nparams && !rc; ++j)
                if (c.params[j]) rc = cgo_objective_set_param_host(hobj, j, c.params[j] + b * n);
            if (rc) break;
            if ((rc = hs->be->set_x0_host(c.x0 + b * n))) break;
            if ((rc = hs->sv->start())) break;
        } else if (s.it == 0) {   // nothing completed: the problem's own start, as a single solve has it
            if ((rc = be.batch_export_row(b, *hs->be, false))) break;
            if ((rc = hs->sv->start())) break;
        } else {
            if ((rc = be.batch_export_row(b, *hs->be, true))) break;
            std::vector<ResRecord> prefix;
            if ((rc = be.batch_records(b, s.it, prefix))) break;
            hs->sv->resume(run.f_x0[(size_t)b], run.evals[(size_t)b], s, prefix.data());
        }
        bool fin = false;
        while (!rc && !fin) rc = hs->sv->iterate(INT64_MAX / 2, fin);
        if (rc) break;
        cgo_results r{};
        r.minimizer = out->minimizer ? out->minimizer + b * n : nullptr;
        r.gradient = out->gradient ? out->gradient + b * n : nullptr;
        r.trace_objective = out->trace_objective ? out->trace_objective + b * mi : nullptr;
        r.trace_grad_norm = out->trace_grad_norm ? out->trace_grad_norm + b * mi : nullptr;
        r.trace_step_size = out->trace_step_size ? out->trace_step_size + b * mi : nullptr;
        r.trace_objective_evals = out->trace_objective_evals ? out->trace_objective_evals + b * mi : nullptr;
        if ((rc = cgo_solver_results(hs, &r))) break;
        if (out->objective) out->objective[b] = r.objective;
        if (out->iters_ran) out->iters_ran[b] = r.iters_ran;
        if (out->status) out->status[b] = r.status;
        if (out->total_fdf_evals) out->total_fdf_evals[b] = r.total_fdf_evals;
        out->handed_back++;
    }
    std::string keep = get_error();
    if (hs) cgo_solver_destroy(hs);
    if (hobj) cgo_objective_destroy(hobj);
    if (rc) set_error(keep);
    return rc;
}

// A batch that stays on the device between solves: the concatenated objective, its backend and the uploaded slot rows of the
// one-shot call on a model, kept.  m_max > 0: opened for L-BFGS, with a ring of m_max + 1 slots per problem — every solve empties
// every ring with ITS m ≤ m_max (batch_lbfgs_reset(m): the kernels lay the ring out from the QnState's own m, the stride between
// two problems' rings stays (m_max + 1) · ld).
struct cgo_batch {
    cgo_ctx *ctx = nullptr;
    cgo_objective *model = nullptr;   // a reference is held: its scalar and cost class are read at every solve
    int64_t n = 0, batch = 0;
    int m_max = 0;
    HipObjective cat;
    HipBackend *be = nullptr;
    ~cgo_batch() { delete be; }
};
// the open's last phase, `h->cat` made: the backend, the slot rows, the ring, the reference to the model
static int batch_open_on(std::unique_ptr<cgo_batch> &h, cgo_objective *model, const double *const *params, bool device_rows, int m_max, bool lds, cgo_batch **handle) {
    h->be = new HipBackend(&h->ctx->c, &h->cat);
    if (int rc = batch_backend_on(h->ctx, h->n, h->batch, params, *h->be, device_rows, m_max, lds)) return rc;
    h->m_max = m_max;
    h->model = model; model->refs++;
    *handle = h.release();
    return CGO_OK;
}
// a solve's phases from the scalars on (a handle speaks of both in the CG flavours' words, whichever kind it is)
static int batch_solve_handle(cgo_batch *h, const double *x0, const double *scalars, const unsigned char *active, const cgo_cg_config *cfg,
                              const cgo_ls_config *ls, int64_t slice_iters, cgo_batch_results *out) {
    if (int rc = check_scalars(kCG, scalars, h->batch)) return rc;
    if (int rc = check_active(kCG, active, h->batch)) return rc;
    HIPCHK2(hipSetDevice(h->ctx->c.device));
    h->cat.s0 = h->model->o.s0; h->cat.user_cheap = h->model->o.user_cheap;
    return batch_solve_on({h->ctx, h->be, nullptr, false, h->n, h->batch, x0, nullptr, scalars, active, cfg, ls, slice_iters, out,
                           batch_model_hobj(h->ctx, h->model), {h->m_max > 0 ? cfg->beta.lbfgs_m : 0, h->model->o.nparams(), false}});
}

// ---- the entry points ------------------------------------------------------------------------------------------------------------
extern "C" {

int cgo_minimize_batch(cgo_ctx *ctx, int32_t obj_kind, int64_t n, int64_t batch, const double *x0, const double *param0,
                       const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t slice_iters, cgo_batch_results *out) {
    return cgo_minimize_batch_ex(ctx, obj_kind, n, batch, x0, param0, cfg, ls, slice_iters, nullptr, out, nullptr);
}

int cgo_minimize_batch_ex(cgo_ctx *ctx, int32_t obj_kind, int64_t n, int64_t batch, const double *x0, const double *param0,
                          const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t slice_iters, const cgo_batch_policy *policy,
                          cgo_batch_results *out, int32_t *rows_used) {
    API_GUARD_BEGIN
    REQUIRE(ctx && x0 && cfg && ls && out, "null argument");
    out->launches = 0; out->handed_back = 0;
    int rows = 0;
    if (int rc = batch_rows_asked(policy, CGO_BATCH_ROWS_LDS, kCG, rows)) return rc;
    if (int rc = check_builtin_kind(kCG, obj_kind, false)) return rc;
    if (int rc = check_batch_call(ctx, nullptr, cfg, ls, n, batch, slice_iters)) return rc;
    if (int rc = check_builtin_rules(kCG, obj_kind, n, param0, "param0")) return rc;
    HIPCHK2(hipSetDevice(ctx->c.device));
    bool device_rows = false;
    if (int rc = batch_tier(rows, n, batch, obj_kind == CGO_OBJ_QUAD_DIAG ? 1 : 0, cgo_batch_max_n(ctx, obj_kind), "cgo_batch_max_n", device_rows)) return rc;
    if (rows_used) *rows_used = device_rows ? CGO_BATCH_ROWS_DEVICE : CGO_BATCH_ROWS_LDS;
    HipObjective cat;
    if (int rc = builtin_cat(ctx, obj_kind, n, batch, cat)) return rc;
    const double *params[1] = {param0};
    return batch_solve_on({ctx, nullptr, &cat, device_rows, n, batch, x0, params, nullptr, nullptr, cfg, ls, slice_iters, out,
                           builtin_hobj(ctx, obj_kind, n), {0, 0, false}});
    API_GUARD_END
}

int cgo_minimize_batch_lbfgs(cgo_ctx *ctx, int32_t obj_kind, int64_t n, int64_t batch, const double *x0, const double *param0,
                             const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t slice_iters, cgo_batch_results *out) {
    return cgo_minimize_batch_lbfgs_ex(ctx, obj_kind, n, batch, x0, param0, cfg, ls, slice_iters, nullptr, out, nullptr);
}

// … and their LDS tier (k_batch_lbfgs_lds): the call above with a policy.  A null policy is the call without one — device rows.
int cgo_minimize_batch_lbfgs_ex(cgo_ctx *ctx, int32_t obj_kind, int64_t n, int64_t batch, const double *x0, const double *param0,
                                const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t slice_iters, const cgo_batch_policy *policy,
                                cgo_batch_results *out, int32_t *rows_used) {
    API_GUARD_BEGIN
    REQUIRE(ctx && x0 && cfg && ls && out, "null argument");
    out->launches = 0; out->handed_back = 0;
    int rows = 0;
    if (int rc = batch_rows_asked(policy, CGO_BATCH_ROWS_DEVICE, kLB, rows)) return rc;
    if (int rc = check_builtin_kind(kLB, obj_kind, false)) return rc;
    if (int rc = check_batch_call(ctx, "cgo_minimize_batch", cfg, ls, n, batch, slice_iters)) return rc;
    if (int rc = check_builtin_rules(kLB, obj_kind, n, param0, "param0")) return rc;
    const int m = cfg->beta.lbfgs_m;
    bool lds = false;
    if (rows != CGO_BATCH_ROWS_DEVICE) {
        HIPCHK2(hipSetDevice(ctx->c.device));
        if (int rc = batch_lbfgs_tier(rows, n, builtin_lds_max_n(ctx, obj_kind, m), lds)) return rc;
    }
    if (int rc = batch_lbfgs_sizes(ctx, obj_kind, n, batch, m)) return rc;
    if (rows_used) *rows_used = lds ? CGO_BATCH_ROWS_LDS : CGO_BATCH_ROWS_DEVICE;
    HipObjective cat;
    if (int rc = builtin_cat(ctx, obj_kind, n, batch, cat)) return rc;
    const double *params[1] = {param0};
    return batch_solve_on({ctx, nullptr, &cat, true, n, batch, x0, params, nullptr, nullptr, cfg, ls, slice_iters, out,
                           builtin_hobj(ctx, obj_kind, n), {m, 1, lds}});
    API_GUARD_END
}

int cgo_minimize_batch_obj(cgo_ctx *ctx, cgo_objective *model, int64_t batch, const double *x0, const double *const *params,
                           int32_t n_params, const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t slice_iters,
                           cgo_batch_results *out) {
    return cgo_minimize_batch_obj_ex(ctx, model, batch, x0, params, n_params, cfg, ls, slice_iters, nullptr, out, nullptr);
}

int cgo_minimize_batch_obj_ex(cgo_ctx *ctx, cgo_objective *model, int64_t batch, const double *x0, const double *const *params,
                              int32_t n_params, const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t slice_iters,
                              const cgo_batch_policy *policy, cgo_batch_results *out, int32_t *rows_used) {
    API_GUARD_BEGIN
    REQUIRE(ctx && model && x0 && cfg && ls && out, "null argument");
    out->launches = 0; out->handed_back = 0;
    int rows = 0;
    if (int rc = batch_rows_asked(policy, CGO_BATCH_ROWS_LDS, kCG, rows)) return rc;
    if (int rc = check_batch_model(ctx, model)) return rc;
    const int64_t n = model->o.n_local;
    if (int rc = check_batch_call(ctx, nullptr, cfg, ls, n, batch, slice_iters)) return rc;
    HipObjective cat;
    bool device_rows = false;
    if (int rc = batch_model_cat(ctx, model, batch, params, n_params, cat, rows, device_rows)) return rc;
    if (rows_used) *rows_used = device_rows ? CGO_BATCH_ROWS_DEVICE : CGO_BATCH_ROWS_LDS;
    return batch_solve_on({ctx, nullptr, &cat, device_rows, n, batch, x0, params, nullptr, nullptr, cfg, ls, slice_iters, out,
                           batch_model_hobj(ctx, model), {0, 0, false}});
    API_GUARD_END
}

// Batched L-BFGS solves on a run-time compiled objective: k_batch_lbfgs<UserObjective, 3>, the fifth program of its module.  The
// model and params are checked as cgo_minimize_batch_obj checks them, the config as cgo_minimize_batch_lbfgs checks it; the batch
// is the device-rows tier's with the ring beside it.
int cgo_minimize_batch_lbfgs_obj(cgo_ctx *ctx, cgo_objective *model, int64_t batch, const double *x0, const double *const *params,
                                 int32_t n_params, const double *scalars, const cgo_cg_config *cfg, const cgo_ls_config *ls,
                                 int64_t slice_iters, cgo_batch_results *out) {
    return cgo_minimize_batch_lbfgs_obj_ex(ctx, model, batch, x0, params, n_params, scalars, cfg, ls, slice_iters, nullptr, out, nullptr);
}

int cgo_minimize_batch_lbfgs_obj_ex(cgo_ctx *ctx, cgo_objective *model, int64_t batch, const double *x0, const double *const *params,
                                    int32_t n_params, const double *scalars, const cgo_cg_config *cfg, const cgo_ls_config *ls,
                                    int64_t slice_iters, const cgo_batch_policy *policy, cgo_batch_results *out, int32_t *rows_used) {
    API_GUARD_BEGIN
    REQUIRE(ctx && model && x0 && cfg && ls && out, "null argument");
    out->launches = 0; out->handed_back = 0;
    int rows = 0;
    if (int rc = batch_rows_asked(policy, CGO_BATCH_ROWS_DEVICE, kLB, rows)) return rc;
    if (int rc = check_batch_model(ctx, model)) return rc;
    const int64_t n = model->o.n_local;
    if (int rc = check_batch_call(ctx, "cgo_minimize_batch_obj", cfg, ls, n, batch, slice_iters)) return rc;
    if (int rc = check_batch_model_params(model, params, n_params)) return rc;
    if (int rc = check_scalars(kLB, scalars, batch)) return rc;
    const int m = cfg->beta.lbfgs_m;
    bool lds = false;
    if (int rc = batch_lbfgs_model_plan(ctx, model, rows, batch, m, "cgo_batch_lbfgs_max_n_ex", lds)) return rc;
    if (rows_used) *rows_used = lds ? CGO_BATCH_ROWS_LDS : CGO_BATCH_ROWS_DEVICE;
    HipObjective cat;
    if (int rc = batch_model_cat_rows(ctx, model, batch, cat)) return rc;
    return batch_solve_on({ctx, nullptr, &cat, true, n, batch, x0, params, scalars, nullptr, cfg, ls, slice_iters, out,
                           batch_model_hobj(ctx, model), {m, model->o.nparams(), lds}});
    API_GUARD_END
}

int cgo_batch_open(cgo_ctx *ctx, cgo_objective *model, int64_t batch, const double *const *params, int32_t n_params, cgo_batch **handle) {
    return cgo_batch_open_ex(ctx, model, batch, params, n_params, nullptr, handle);
}

int cgo_batch_open_ex(cgo_ctx *ctx, cgo_objective *model, int64_t batch, const double *const *params, int32_t n_params,
                      const cgo_batch_policy *policy, cgo_batch **handle) {
    API_GUARD_BEGIN
    REQUIRE(ctx && model && handle, "null argument");
    *handle = nullptr;
    int rows = 0;
    if (int rc = batch_rows_asked(policy, CGO_BATCH_ROWS_LDS, kCG, rows)) return rc;
    if (int rc = check_batch_model(ctx, model)) return rc;
    if (int rc = check_batch_shape(ctx, kCG, model->o.n_local, batch, 0)) return rc;
    std::unique_ptr<cgo_batch> h(new cgo_batch);
    h->ctx = ctx; h->n = model->o.n_local; h->batch = batch;
    bool device_rows = false;
    if (int rc = batch_model_cat(ctx, model, batch, params, n_params, h->cat, rows, device_rows)) return rc;
    return batch_open_on(h, model, params, device_rows, 0, false, handle);
    API_GUARD_END
}

// … for β = LBFGS(m): the batch of cgo_minimize_batch_lbfgs_obj_ex, kept, with a ring for m_max pairs per problem
int cgo_batch_lbfgs_open(cgo_ctx *ctx, cgo_objective *model, int64_t batch, const double *const *params, int32_t n_params,
                         int32_t m_max, const cgo_batch_policy *policy, cgo_batch **handle) {
    API_GUARD_BEGIN
    REQUIRE(ctx && model && handle, "null argument");
    *handle = nullptr;
    int rows = 0;
    if (int rc = batch_rows_asked(policy, CGO_BATCH_ROWS_DEVICE, kLB, rows)) return rc;
    if (int rc = check_batch_model(ctx, model)) return rc;
    if (m_max < 1 || m_max > QN_MAX_M) return refuse(CGO_EINVAL, "batched L-BFGS solves: m_max = " + std::to_string(m_max) + " lies outside 1 … cgo_batch_lbfgs_max_m = " + std::to_string(QN_MAX_M));
    if (int rc = check_batch_shape(ctx, kLB, model->o.n_local, batch, 0)) return rc;
    if (int rc = check_batch_model_params(model, params, n_params)) return rc;
    bool lds = false;
    if (int rc = batch_lbfgs_model_plan(ctx, model, rows, batch, m_max, "cgo_batch_lbfgs_max_n_obj_ex", lds)) return rc;
    std::unique_ptr<cgo_batch> h(new cgo_batch);
    h->ctx = ctx; h->n = model->o.n_local; h->batch = batch;
    if (int rc = batch_model_cat_rows(ctx, model, batch, h->cat)) return rc;
    return batch_open_on(h, model, params, true, m_max, lds, handle);
    API_GUARD_END
}

int cgo_batch_rows(const cgo_batch *h, int32_t *rows_used) {
    API_GUARD_BEGIN
    REQUIRE(h && h->be && rows_used, "null argument");
    if (h->m_max > 0) *rows_used = h->be->batch_lbfgs_in_lds() ? CGO_BATCH_ROWS_LDS : CGO_BATCH_ROWS_DEVICE;   // (its rows are device rows in both tiers)
    else *rows_used = h->be->batch_device_rows() ? CGO_BATCH_ROWS_DEVICE : CGO_BATCH_ROWS_LDS;
    return CGO_OK;
    API_GUARD_END
}

int cgo_batch_lbfgs_m(const cgo_batch *h, int32_t *m_max) {
    API_GUARD_BEGIN
    REQUIRE(h && h->be && m_max, "null argument");
    *m_max = h->m_max;
    return CGO_OK;
    API_GUARD_END
}

int cgo_batch_solve(cgo_batch *h, const double *x0, const double *scalars, const unsigned char *active, const cgo_cg_config *cfg,
                    const cgo_ls_config *ls, int64_t slice_iters, cgo_batch_results *out) {
    API_GUARD_BEGIN
    REQUIRE(h && x0 && cfg && ls && out, "null argument");
    out->launches = 0; out->handed_back = 0;
    REQUIRE(h->m_max == 0, "batched solves: the handle was opened for L-BFGS: cgo_batch_lbfgs_solve");
    if (int rc = check_batch_call(h->ctx, nullptr, cfg, ls, h->n, h->batch, slice_iters)) return rc;
    return batch_solve_handle(h, x0, scalars, active, cfg, ls, slice_iters, out);
    API_GUARD_END
}

int cgo_batch_lbfgs_solve(cgo_batch *h, const double *x0, const double *scalars, const unsigned char *active, const cgo_cg_config *cfg,
                          const cgo_ls_config *ls, int64_t slice_iters, cgo_batch_results *out) {
    API_GUARD_BEGIN
    REQUIRE(h && x0 && cfg && ls && out, "null argument");
    out->launches = 0; out->handed_back = 0;
    REQUIRE(h->m_max > 0, "batched L-BFGS solves: the handle was opened for the CG flavours: cgo_batch_solve");
    if (int rc = check_batch_call(h->ctx, "cgo_batch_solve", cfg, ls, h->n, h->batch, slice_iters)) return rc;
    const int m = cfg->beta.lbfgs_m;
    if (m > h->m_max) return refuse(CGO_EINVAL, "batched L-BFGS solves: m = " + std::to_string(m) + " exceeds the m_max = " + std::to_string(h->m_max) + " the handle was opened with");
    return batch_solve_handle(h, x0, scalars, active, cfg, ls, slice_iters, out);
    API_GUARD_END
}

int cgo_batch_close(cgo_batch *h) {
    API_GUARD_BEGIN
    if (!h) return CGO_OK;
    cgo_ctx *c = h->ctx;
    cgo_objective *m = h->model;
    if (c) (void)hipSetDevice(c->c.device);
    delete h;            // (the backend before the model: its objective shares the model's module)
    obj_unref(m);
    return CGO_OK;
    API_GUARD_END
}

// ---- cgo_batch_probe: a script of passes of a batched solve in one launch (cgo_backend_batch_probe.hip) ------------------------------
// The batch is made as the solve of that tier makes it — the same rules for objectives, shapes and sizes, in the probe's own
// order and words, the same concatenated objective and backend — and lives for this one call.
int64_t cgo_batch_probe_qn_bytes(void) { return (int64_t)sizeof(QnState); }

int cgo_batch_probe(cgo_ctx *ctx, cgo_batch_probe_args *p) {
    API_GUARD_BEGIN
    REQUIRE(ctx && p, "null argument");
    p->points = 0; p->ld = 0; p->symbol[0] = 0;
    REQUIRE(p->tier >= 0 && p->tier <= 3, "batch probe: tier must be 0 (LDS), 1 (device rows), 2 (L-BFGS) or 3 (L-BFGS in LDS)");
    REQUIRE(p->npass >= 1 && p->npass <= CGO_BATCH_PROBE_MAX_PASSES, "batch probe: 1 … 32 passes");
    if (int rc = check_one_rank(ctx, kPR)) return rc;
    REQUIRE(p->batch >= 1 && p->batch <= 0x7FFFFFFF, "batch probe: 1 ≤ batch ≤ the largest grid");
    REQUIRE(p->x && p->u, "batch probe: x and u are required");
    const int64_t batch = p->batch;
    const int rows = p->tier == 0 ? CGO_BATCH_ROWS_LDS : CGO_BATCH_ROWS_DEVICE;
    bool device_rows = false;
    HipObjective cat;
    int64_t n = p->n;
    if (p->model) {
        REQUIRE(p->tier < 2, "batch probe: the batched L-BFGS kernels of a run-time compiled objective have no PROBE twin (tiers 0 and 1)");
        if (int rc = check_batch_model(ctx, p->model)) return rc;
        n = p->model->o.n_local;
        REQUIRE(p->n == n, "batch probe: n is not the size of the model objective");
        REQUIRE(n >= 1, "batch probe: n must be ≥ 1");
        if (int rc = check_scalars(kPR, p->scalars, batch)) return rc;
        if (int rc = batch_model_cat(ctx, p->model, batch, p->params, p->n_params, cat, rows, device_rows)) return rc;
    } else {
        const int32_t obj_kind = p->obj_kind;
        if (int rc = check_builtin_kind(kPR, obj_kind, true)) return rc;
        REQUIRE(n >= 1, "batch probe: n must be ≥ 1");
        REQUIRE(!p->scalars, "batch probe: scalars belong to a run-time compiled objective");
        if (int rc = check_builtin_rules(kPR, obj_kind, n, p->params[0], "params[0]")) return rc;
        HIPCHK2(hipSetDevice(ctx->c.device));
        if (p->tier >= 2) {
            REQUIRE(p->m >= 1, "batch probe: m must be ≥ 1");
            if (int rc = check_lbfgs_m(kPR, p->m)) return rc;
            if (p->tier == 3) { bool lds = false; if (int rc = batch_lbfgs_tier(CGO_BATCH_ROWS_LDS, n, builtin_lds_max_n(ctx, obj_kind, p->m), lds)) return rc; }
            if (int rc = batch_lbfgs_sizes(ctx, obj_kind, n, batch, p->m)) return rc;
            device_rows = true;
        } else {
            if (int rc = batch_tier(rows, n, batch, obj_kind == CGO_OBJ_QUAD_DIAG ? 1 : 0, cgo_batch_max_n(ctx, obj_kind), "cgo_batch_max_n", device_rows)) return rc;
        }
        if (int rc = builtin_cat(ctx, obj_kind, n, batch, cat)) return rc;
    }
    HipBackend be(&ctx->c, &cat);
    if (int rc = batch_backend_on(ctx, n, batch, p->params, be, device_rows, p->tier >= 2 ? p->m : 0, p->tier == 3)) return rc;
    return be.batch_probe(*p);
    API_GUARD_END
}

}  // extern "C"
