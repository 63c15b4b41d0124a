// cgo_backend_batch.hip — the host side of batched solves: many small problems in one launch, a workgroup each.  The backend's
// objective spans the concatenated problems (n_local = batch · ld), so x, u and every parameter slot ARE the [batch][ld] rows;
// the loop over launches is the engine's (run_batch, cgo_engine.cpp), the hand-back of a problem the device loop does not
// finish is the C API's (cgo_minimize_batch[_obj]), through batch_export_row below.
// Four tiers (BatchTier) share everything here — allocation, reset, THE launch, records, hand-back, results.  What differs is one
// row of batch_tier_of() below: the kernel family (ahead of time, or the program of a run-time compiled objective's module,
// cgo_rtc_batch.hip), whether it is a quasi-Newton tier, and the rows a launch keeps in dynamic LDS.  The instantiations of
// k_batch live here; those of every other tier in a translation unit of their own (cgo_backend_batch_rows.hip, _lbfgs.hip,
// _lbfgs_lds.hip; the PROBE twins of all four in _probe.hip), so that the device code of each unit is what it was before the
// next tier existed.
#include "cgo_backend_internal.hpp"
#include "cgo_kernels_batch.hip.hpp"

namespace cgo {

using namespace dev;

template <class Obj>
struct BatchRows {
    static RowPick at(int npts) {
        RowPick p;
#define ROW(NPTS) p.row(npts, NPTS, (const void *)k_batch<Obj, NPTS>);
        CGO_BATCH_ROWS(ROW)
#undef ROW
        return p;
    }
};
static RowPick batch_kernel_for(int obj_kind, int npts) { return row_pick_for<BatchRows>(obj_kind, npts); }

static int batch_vecs(int nparams, int = 0) { return 2 + nparams; }   // x, u and the parameter slots
// this tier's row of the table (batch_tier_of) (a table inside a function: a namespace-scope constant of a .hip unit is emitted for the device as well)
const BatchTierRow &tier_row_lds() {
    static const BatchTierRow row = {"k_batch", batch_kernel_for, RTC_BATCH, "batch:", RTC_BATCH_PROBE, "batch_probe:", false, [](int K, int) { return batch_vecs(K); },
                                     "batched solves: no k_batch instantiation for this objective"};
    return row;
}
// THE table of tiers: each row stands in the translation unit of its tier, beside the instantiations it names
const BatchTierRow &batch_tier_of(BatchTier tier) {
    switch (tier) {
    case BatchTier::LDS: return tier_row_lds();
    case BatchTier::ROWS: return tier_row_rows();
    case BatchTier::LBFGS: return tier_row_lbfgs();
    default: return tier_row_lbfgs_lds();
    }
}

hipFunction_t batch_tier_module_kernel(const BatchTierRow &t, const RtcModule *rtc, int npts, bool probe) {
    if (!rtc || (probe && t.probe_prog == RTC_NONE)) return nullptr;
    return probe ? rtc->kernel(t.probe_prog, t.probe_key, npts) : rtc->kernel(t.prog, t.key, npts);
}

bool kernel_static_lds(const void *fn, hipFunction_t mf, int64_t &bytes) {
    if (fn) {
        hipFuncAttributes fa;
        if (hipFuncGetAttributes(&fa, fn) != hipSuccess) { (void)hipGetLastError(); return false; }
        bytes = (int64_t)fa.sharedSizeBytes;
    } else {
        int v = 0;
        if (hipFuncGetAttribute(&v, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, mf) != hipSuccess) { (void)hipGetLastError(); return false; }
        bytes = v;
    }
    return true;
}

static const void *batch_grad_kernel_for(int obj_kind) {
    switch (obj_kind) {
#define ROW(KIND, T) case KIND: return (const void *)k_batch_grad<T>;
    CGO_OBJ_ROWS(ROW)
#undef ROW
    default: return nullptr;
    }
}
// res_plan's arithmetic for ONE workgroup that holds a whole problem: what the device gives a block, minus the kernel's static
// LDS, minus the same 512 bytes of slack, over 8 bytes × the rows the tier keeps there, rounded down to an even count (ld is even)
// — batch_lbfgs_lds_ld_of, for both LDS tiers.  (k_batch's limit was written out here before the tiers shared it: the same values,
// a negative remainder gave 0 there by the last line and gives 0 here by the first.)
// `rtc`: the module of a CGO_OBJ_USER objective, the tier's program loaded.  0: no kernel, no device, rows out of range.
int64_t batch_tier_max_ld(HipCtx *ctx, BatchTier tier, int obj_kind, int m, const RtcModule *rtc) {
    const BatchTierRow &t = batch_tier_of(tier);
    const void *fn = t.aot(obj_kind, 3).fn;
    const hipFunction_t mf = obj_kind == CGO_OBJ_USER ? batch_tier_module_kernel(t, rtc, 3) : nullptr;
    if (!fn && !mf) return 0;
    if (hipSetDevice(ctx->device) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int max_lds = 0;
    if (hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int64_t static_lds = 0;
    if (!kernel_static_lds(fn, mf, static_lds)) return 0;
    const int nparams = fn ? (obj_kind == CGO_OBJ_QUAD_DIAG ? 1 : 0) : rtc->n_params;
    return HipBackend::batch_lbfgs_lds_ld_of(max_lds, static_lds, t.lds_rows(nparams, m));
}
int64_t HipBackend::batch_max_n(HipCtx *ctx, int obj_kind, const RtcModule *rtc) { return batch_tier_max_ld(ctx, BatchTier::LDS, obj_kind, 0, rtc); }

// x, u, every slot and the results' gradient, [batch][ld] each; the states, f_x0 and a scalar per problem beside them
double HipBackend::batch_rows_bytes(int64_t batch, int64_t n, int nparams) {
    const double ld = (double)n + (double)(n & 1);
    return (double)batch * (ld * 8.0 * (double)(batch_vecs(nparams) + 1) + (double)sizeof(ResState) + 16.0);
}

// "allocate + slots": the rows of every parameter slot go up ONCE; the states, f_x0 and (where scalars per problem will come) s0v
// are allocated.  batch_reset below starts a solve on them, any number of times.
int HipBackend::batch_alloc(int64_t batch, int64_t n, const double *const *params, bool device_rows) {
    const int64_t ld = n + (n & 1);
    if (batch < 1 || n < 1 || obj_->n_local != batch * ld || !rmode_ || bat_st_) { set_error("internal: batched solve on a backend of another shape"); return CGO_ESTATE; }
    HIPCHK(hipSetDevice(ctx_->device));
    bat_count_ = batch; bat_n_ = n; bat_ld_ = ld;
    bat_tier_ = device_rows ? BatchTier::ROWS : BatchTier::LDS;
    const BatchTierRow &t = batch_tier_of(bat_tier_);
    bat_lds_ = (size_t)ld * 8 * (size_t)t.lds_rows(obj_->nparams(), 0);
    if (device_rows && n > batch_rows_max_n()) { set_error("internal: a batch beyond the pass index of the device-rows tier"); return CGO_ESTATE; }
    // rows padded to ld.  No pass reads the padding element (the odd tail is the workgroup's own element n − 1); the ONE
    // gradient launch over the concatenated rows (batch_results) does evaluate it.  Built-in objectives: zero in x, u and the
    // parameter vector, ∇f = D·x = 0 there.  A user's body is never evaluated on data the user did not supply — log(p), 1/p at
    // a zero would put a NaN into that launch — so there the padding of x and of every slot repeats element n − 1 of its row
    // (u stays zero).
    std::vector<double> rows((size_t)batch * (size_t)ld, 0.0);
    const size_t nb = rows.size() * sizeof(double);
    for (int j = 0; j < obj_->nparams(); ++j) {
        if (!params || !params[j]) { set_error("internal: batched solve without its parameter rows"); return CGO_ESTATE; }
        batch_fill_rows(rows, params[j]);
        HIPCHK(hipMemcpyAsync(obj_->p[j].p, rows.data(), nb, hipMemcpyHostToDevice, ctx_->stream));
        HIPCHK(hipStreamSynchronize(ctx_->stream));
        obj_->p_set[j] = true;
    }
    HIPCHK(hipMalloc((void **)&bat_st_, sizeof(ResState) * (size_t)batch));
    HIPCHK(hipMalloc((void **)&bat_fx0_, sizeof(double) * (size_t)batch));
    if (obj_->kind == CGO_OBJ_USER) {   // (a module's kernel takes its dynamic LDS as launched, as the resident solver's does)
        // (rows in device memory: the program of any tier whose rows are — batch_lbfgs_alloc may follow on and make the batch that tier's)
        bool compiled = false;
        for (int r = (int)bat_tier_; r < (device_rows ? BATCH_TIERS : 1); ++r) compiled = compiled || batch_tier_module_kernel(batch_tier_of((BatchTier)r), obj_->rtc.get(), 3);
        if (!compiled) { set_error("internal: batched solve before the objective's batch program was compiled"); return CGO_ESTATE; }
        return CGO_OK;
    }
    const void *fn = t.aot(obj_->kind, 3).fn;
    if (!fn) { set_error(t.missing); return CGO_EINVAL; }
    if (bat_lds_ > 48 * 1024) HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bat_lds_));
    return CGO_OK;
}

void HipBackend::batch_fill_rows(std::vector<double> &rows, const double *src) const {
    const bool user = obj_->kind == CGO_OBJ_USER;
    for (int64_t b = 0; b < bat_count_; ++b) {
        std::memcpy(rows.data() + (size_t)b * bat_ld_, src + (size_t)b * bat_n_, sizeof(double) * (size_t)bat_n_);
        if (bat_ld_ > bat_n_) rows[(size_t)b * bat_ld_ + bat_n_] = user ? src[(size_t)b * bat_n_ + bat_n_ - 1] : 0.0;
    }
}

// "reset for a solve": x ← x0, u ← 0, every ACTIVE problem's state fresh (optim.jl:47) and its f_x0 zero; an inactive problem
// (active[b] == 0) is preset RES_STOP, so that its workgroup returns at once and nothing of it is read afterwards.  scalars:
// every problem's own objective scalar for this solve (null: the objective's s0 for all).
int HipBackend::batch_reset(const double *x0, const double *scalars, const unsigned char *active, int64_t max_iters, bool trace) {
    if (!bat_st_) { set_error("internal: batch_reset before batch_alloc"); return CGO_ESTATE; }
    HIPCHK(hipSetDevice(ctx_->device));
    const int64_t batch = bat_count_;
    bat_trace_ = trace;
    if (trace) {   // (no trace: one slice's worth, sized by the first launch)
        const int64_t stride = std::max<int64_t>(max_iters, 1);
        if (int rc = batch_recs_reserve(stride)) return rc;
    }
    std::vector<double> rows((size_t)batch * (size_t)bat_ld_, 0.0);
    const size_t nb = rows.size() * sizeof(double);
    batch_fill_rows(rows, x0);
    HIPCHK(hipMemcpyAsync(xc_, rows.data(), nb, hipMemcpyHostToDevice, ctx_->stream));
    HIPCHK(hipMemsetAsync(uc_, 0, nb, ctx_->stream));
    HIPCHK(hipStreamSynchronize(ctx_->stream));
    std::vector<ResState> st((size_t)batch);
    for (int64_t b = 0; b < batch; ++b) {
        ResState &s = st[(size_t)b];
        std::memset(&s, 0, sizeof s);
        s.a_initial = NAN;   // optim.jl:47
        s.reason = (!active || active[b]) ? RES_FRESH : RES_STOP;
    }
    HIPCHK(hipMemcpy(bat_st_, st.data(), sizeof(ResState) * (size_t)batch, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(bat_fx0_, 0, sizeof(double) * (size_t)batch));
    bat_s0v_on_ = scalars != nullptr;
    if (scalars) {
        if (!bat_s0v_) HIPCHK(hipMalloc((void **)&bat_s0v_, sizeof(double) * (size_t)batch));
        HIPCHK(hipMemcpy(bat_s0v_, scalars, sizeof(double) * (size_t)batch, hipMemcpyHostToDevice));
    }
    return CGO_OK;
}

// the records: [batch][stride], grown when a solve needs a longer row
int HipBackend::batch_recs_reserve(int64_t stride) {
    const size_t need = (size_t)bat_count_ * (size_t)stride;
    if (bat_recs_ && bat_recs_cap_ < need) { HIPCHK(hipFree(bat_recs_)); bat_recs_ = nullptr; bat_recs_cap_ = 0; }
    if (!bat_recs_) { HIPCHK(hipMalloc((void **)&bat_recs_, sizeof(ResRecord) * need)); bat_recs_cap_ = need; }
    bat_rec_stride_ = stride;
    return CGO_OK;
}

void HipBackend::batch_fill_params(BatchParams &B, const ResConfig &c, int64_t budget) const {
    B.x = xc_; B.u = uc_; B.p0 = obj_->p[0].p; B.p1 = obj_->p[1].p; B.p2 = obj_->p[2].p; B.p3 = obj_->p[3].p;
    B.st = bat_st_; B.recs = bat_recs_; B.f_x0 = bat_fx0_;
    B.n = bat_n_; B.ld = bat_ld_; B.rec_stride = bat_rec_stride_; B.rec_abs = bat_trace_ ? 1 : 0;
    B.s0 = obj_->s0; B.s0v = bat_s0v_on_ ? bat_s0v_ : nullptr;
    B.cfg = c; B.cfg.npts = 3; B.cfg.log_on = 0;
    B.budget = budget;
}

// the fork every launch of a batch takes, a workgroup per problem
int HipBackend::batch_launch_kernel(const void *fn, hipFunction_t mf, const char *missing, void **args, size_t lds) {
    if (obj_->kind == CGO_OBJ_USER) {   // (a module's kernel takes its dynamic LDS as launched, as the resident solver's does)
        if (!mf) { set_error("internal: kernel missing from the run-time compiled objective module"); return CGO_EINVAL; }
        HIPCHK(hipModuleLaunchKernel(mf, (unsigned)bat_count_, 1, 1, BLOCK, 1, 1, (unsigned)lds, ctx_->stream, args, nullptr));
    } else {
        if (!fn) { set_error(missing); return CGO_EINVAL; }
        HIPCHK(hipLaunchKernel(fn, dim3((unsigned)bat_count_), dim3(BLOCK), args, lds, ctx_->stream));
    }
    total_launches_++;
    return CGO_OK;
}

// … of the tier's own kernel on its parameter block (BatchParams; BatchLbfgsParams for a quasi-Newton tier)
int HipBackend::batch_launch_tier(void *params) {
    const BatchTierRow &t = batch_tier_of(bat_tier_);
    const bool user = obj_->kind == CGO_OBJ_USER;
    void *args[] = {params};
    return batch_launch_kernel(user ? nullptr : t.aot(obj_->kind, 3).fn, user ? batch_tier_module_kernel(t, obj_->rtc.get(), 3) : nullptr, t.missing, args, bat_lds_);
}

int HipBackend::batch_launch(const ResConfig &c, int64_t budget, std::vector<ResState> &st, std::vector<double> &f_x0) {
    if (!bat_st_) { set_error("internal: batch_launch before batch_alloc"); return CGO_ESTATE; }
    HIPCHK(hipSetDevice(ctx_->device));
    if (budget < 1) budget = 1;
    if (!bat_trace_) {   // nobody reads the records: the leader still writes one per completed iteration of the slice
        if (int rc = batch_recs_reserve(budget)) return rc;
    }
    if (batch_tier_of(bat_tier_).qn) {   // the parameter block with the ring: cgo_backend_batch_lbfgs.hip
        if (int rc = batch_lbfgs_launch_tier(c, budget)) return rc;
    } else {
        BatchParams B{};
        batch_fill_params(B, c, budget);
        if (int rc = batch_launch_tier(&B)) return rc;
    }
    st.resize((size_t)bat_count_); f_x0.resize((size_t)bat_count_);
    HIPCHK(hipMemcpyAsync(st.data(), bat_st_, sizeof(ResState) * (size_t)bat_count_, hipMemcpyDeviceToHost, ctx_->stream));
    HIPCHK(hipMemcpyAsync(f_x0.data(), bat_fx0_, sizeof(double) * (size_t)bat_count_, hipMemcpyDeviceToHost, ctx_->stream));
    HIPCHK(hipStreamSynchronize(ctx_->stream));
    return CGO_OK;
}

int HipBackend::batch_records(int64_t b, int64_t count, std::vector<ResRecord> &out) {
    out.clear();
    if (!bat_trace_ || count <= 0) return CGO_OK;
    if (b >= bat_count_ || count > bat_rec_stride_) { set_error("internal: batch_records out of range"); return CGO_ESTATE; }
    if (b < 0) { b = 0; count = bat_count_ * bat_rec_stride_; }   // every problem's row, batch_rec_stride() apart
    out.resize((size_t)count);
    HIPCHK(hipSetDevice(ctx_->device));
    HIPCHK(hipMemcpyAsync(out.data(), bat_recs_ + (size_t)b * (size_t)bat_rec_stride_, sizeof(ResRecord) * (size_t)count, hipMemcpyDeviceToHost, ctx_->stream));
    HIPCHK(hipStreamSynchronize(ctx_->stream));
    return CGO_OK;
}

int HipBackend::batch_export_row(int64_t b, HipBackend &dst, bool with_u) {
    if (b < 0 || b >= bat_count_ || dst.obj_->n_local != bat_n_ || dst.obj_->kind != obj_->kind || !dst.rmode_) { set_error("internal: batch_export_row to a solver of another shape"); return CGO_ESTATE; }
    if (int rc = dst.set_x0_device(xc_ + (size_t)b * (size_t)bat_ld_)) return rc;   // (ends whatever the last problem left pending there)
    const size_t nb = sizeof(double) * (size_t)bat_n_;
    if (with_u) HIPCHK(hipMemcpyAsync(dst.uc_, uc_ + (size_t)b * (size_t)bat_ld_, nb, hipMemcpyDeviceToDevice, ctx_->stream));
    return batch_export_slots(b, dst);
}

// … the slots alone: what a handed-back problem of a batched L-BFGS solve on a handle takes from the batch (its x0 is the
// caller's, and a quasi-Newton solver forms its own u and stored gradient at its start)
int HipBackend::batch_export_slots(int64_t b, HipBackend &dst) {
    if (b < 0 || b >= bat_count_ || dst.obj_->n_local != bat_n_ || dst.obj_->kind != obj_->kind) { set_error("internal: batch_export_slots to a solver of another shape"); return CGO_ESTATE; }
    if (dst.obj_->nparams() != obj_->nparams()) { set_error("internal: batch_export_slots to an objective of other parameter slots"); return CGO_ESTATE; }
    HIPCHK(hipSetDevice(ctx_->device));
    const size_t nb = sizeof(double) * (size_t)bat_n_;
    for (int j = 0; j < obj_->nparams(); ++j) {
        HIPCHK(hipMemcpyAsync(dst.obj_->p[j].p, obj_->p[j].p + (size_t)b * (size_t)bat_ld_, nb, hipMemcpyDeviceToDevice, ctx_->stream));
        dst.obj_->p_set[j] = true;
    }
    HIPCHK(hipStreamSynchronize(ctx_->stream));
    return CGO_OK;
}

// ∇f of every row with its problem's own scalar → ga_ (k_batch_grad): what the R_GRAD launch of download() is without them
int HipBackend::batch_grad_rows() {
    if (int rc = ensure_ga()) return rc;
    BatchGradParams G{};
    G.x = xc_; G.g = ga_.p; G.p0 = obj_->p[0].p; G.p1 = obj_->p[1].p; G.p2 = obj_->p[2].p; G.p3 = obj_->p[3].p;
    G.s0v = bat_s0v_; G.n = bat_n_; G.ld = bat_ld_;
    void *args[] = {&G};
    hipFunction_t mf = nullptr;
    if (obj_->kind == CGO_OBJ_USER && obj_->rtc) {
        if (!obj_->rtc->batch_grad()) {   // (a batch opened on rows in device memory never compiled the batch program, where this kernel lives)
            std::string log;
            if (int rc = rtc_compile_program(*obj_->rtc, RTC_BATCH, log)) { set_error(std::string("user objective: ") + rtc_program_what(RTC_BATCH) + " did not compile:\n" + log); return rc; }
        }
        mf = obj_->rtc->batch_grad();
    }
    return batch_launch_kernel(batch_grad_kernel_for(obj_->kind), mf, "batched solves: no k_batch_grad instantiation for this objective", args, 0);
}

int HipBackend::batch_results(double *x, double *g, const unsigned char *active) {
    if (!x && !g) return CGO_OK;
    const size_t rows = (size_t)bat_count_ * (size_t)bat_ld_;
    std::vector<double> xr(x ? rows : 0), gr(g ? rows : 0);
    if (bat_s0v_on_) {   // a scalar per problem: a workgroup per row, each with its own
        HIPCHK(hipSetDevice(ctx_->device));
        if (g) { if (int rc = batch_grad_rows()) return rc; }
        if (x) HIPCHK(hipMemcpyAsync(xr.data(), xc_, sizeof(double) * rows, hipMemcpyDeviceToHost, ctx_->stream));
        if (g) HIPCHK(hipMemcpyAsync(gr.data(), ga_.p, sizeof(double) * rows, hipMemcpyDeviceToHost, ctx_->stream));
        HIPCHK(hipStreamSynchronize(ctx_->stream));
    } else {
        if (int rc = download(x ? xr.data() : nullptr, g ? gr.data() : nullptr)) return rc;   // ONE gradient launch over every row
    }
    for (int64_t b = 0; b < bat_count_; ++b) {
        if (active && !active[b]) continue;   // an inactive problem's rows of the output stay as the caller left them
        if (x) std::memcpy(x + (size_t)b * bat_n_, xr.data() + (size_t)b * bat_ld_, sizeof(double) * (size_t)bat_n_);
        if (g) std::memcpy(g + (size_t)b * bat_n_, gr.data() + (size_t)b * bat_ld_, sizeof(double) * (size_t)bat_n_);
    }
    return CGO_OK;
}

}  // namespace cgo
