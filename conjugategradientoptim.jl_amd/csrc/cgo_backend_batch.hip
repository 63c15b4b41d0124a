// cgo_backend_batch.hip — the host side of batched solves: many small problems in one launch, a workgroup each (k_batch,
// cgo_kernels_batch.hip.hpp).  The backend's objective spans the concatenated problems (n_local = batch · ld), so x, u and the
// parameter vector ARE the [batch][ld] rows; the loop over launches is the engine's (run_batch, cgo_engine.cpp), the hand-back
// of a problem the device loop does not finish is the C API's (cgo_minimize_batch), through batch_export_row below.
#include "cgo_backend_internal.hpp"
#include "cgo_kernels_batch.hip.hpp"

namespace cgo {

using namespace dev;

// The rows of cgo_instances.def: the last row with NPTS ≤ npts, the first row below that.
template <class Obj>
static const void *batch_kernel(int npts) {
    const void *fn = nullptr;
#define ROW(NPTS) if (!fn || npts >= NPTS) fn = (const void *)k_batch<Obj, NPTS>;
    CGO_BATCH_ROWS(ROW)
#undef ROW
    return fn;
}
static const void *batch_kernel_for(int obj_kind, int npts) {
    switch (obj_kind) {
#define ROW(KIND, T) case KIND: return batch_kernel<T>(npts);
    CGO_OBJ_ROWS(ROW)
#undef ROW
    default: return nullptr;
    }
}
static int batch_vecs(int obj_kind) { return 2 + (obj_kind == CGO_OBJ_QUAD_DIAG ? 1 : 0); }   // x, u and the parameter vector

// res_plan's arithmetic for ONE workgroup that holds a whole problem: what the device gives a block, minus the kernel's static
// LDS, minus the same 512 bytes of slack, over 8 bytes × the vectors, rounded down to an even count (ld is even).
int64_t HipBackend::batch_max_n(HipCtx *ctx, int obj_kind) {
    const void *fn = batch_kernel_for(obj_kind, 3);
    if (!fn) return 0;
    if (hipSetDevice(ctx->device) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int max_lds = 0;
    if (hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device) != hipSuccess) { (void)hipGetLastError(); return 0; }
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, fn) != hipSuccess) { (void)hipGetLastError(); return 0; }
    const int64_t avail = (int64_t)max_lds - (int64_t)fa.sharedSizeBytes - 512;
    const int64_t ld_max = (avail / (8 * batch_vecs(obj_kind))) & ~1LL;
    return ld_max < 2 ? 0 : ld_max;
}

int HipBackend::batch_begin(int64_t batch, int64_t n, const double *x0, const double *param0, int64_t max_iters, bool trace) {
    const int64_t ld = n + (n & 1);
    if (batch < 1 || n < 1 || obj_->n_local != batch * ld || !rmode_) { set_error("internal: batched solve on a backend of another shape"); return CGO_ESTATE; }
    HIPCHK(hipSetDevice(ctx_->device));
    bat_count_ = batch; bat_n_ = n; bat_ld_ = ld; bat_trace_ = trace;
    bat_rec_stride_ = trace ? std::max<int64_t>(max_iters, 1) : 0;   // (no trace: one slice's worth, sized by the first launch)
    bat_lds_ = (size_t)ld * 8 * (size_t)batch_vecs(obj_->kind);
    // rows padded to ld: the padding element is zero in x, u and the parameter vector — no pass reads it (the odd tail is the
    // workgroup's own element n − 1), and the gradient launch over the concatenated rows gets ∇f = D·x = 0 there
    std::vector<double> rows((size_t)batch * (size_t)ld, 0.0);
    const size_t nb = rows.size() * sizeof(double);
    for (int64_t b = 0; b < batch; ++b) std::memcpy(rows.data() + (size_t)b * ld, x0 + (size_t)b * n, sizeof(double) * (size_t)n);
    HIPCHK(hipMemcpyAsync(xc_, rows.data(), nb, hipMemcpyHostToDevice, ctx_->stream));
    HIPCHK(hipMemsetAsync(uc_, 0, nb, ctx_->stream));
    HIPCHK(hipStreamSynchronize(ctx_->stream));
    if (obj_->uses_param()) {
        if (!param0) { set_error("internal: batched solve without its parameter rows"); return CGO_ESTATE; }
        for (int64_t b = 0; b < batch; ++b) {
            std::memcpy(rows.data() + (size_t)b * ld, param0 + (size_t)b * n, sizeof(double) * (size_t)n);
            if (ld > n) rows[(size_t)b * ld + n] = 0.0;
        }
        HIPCHK(hipMemcpyAsync(obj_->p[0].p, rows.data(), nb, hipMemcpyHostToDevice, ctx_->stream));
        HIPCHK(hipStreamSynchronize(ctx_->stream));
        obj_->p_set[0] = true;
    }
    std::vector<ResState> st((size_t)batch);
    for (auto &s : st) { std::memset(&s, 0, sizeof s); s.a_initial = NAN; s.reason = RES_FRESH; }   // optim.jl:47
    HIPCHK(hipMalloc((void **)&bat_st_, sizeof(ResState) * (size_t)batch));
    HIPCHK(hipMalloc((void **)&bat_fx0_, sizeof(double) * (size_t)batch));
    HIPCHK(hipMemcpy(bat_st_, st.data(), sizeof(ResState) * (size_t)batch, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(bat_fx0_, 0, sizeof(double) * (size_t)batch));
    if (trace) HIPCHK(hipMalloc((void **)&bat_recs_, sizeof(ResRecord) * (size_t)batch * (size_t)bat_rec_stride_));
    const void *fn = batch_kernel_for(obj_->kind, 3);
    if (!fn) { set_error("batched solves: no k_batch instantiation for this objective"); return CGO_EINVAL; }
    if (bat_lds_ > 48 * 1024) HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bat_lds_));
    return CGO_OK;
}

int HipBackend::batch_launch(const ResConfig &c, int64_t budget, std::vector<ResState> &st, std::vector<double> &f_x0) {
    if (!bat_st_) { set_error("internal: batch_launch before batch_begin"); return CGO_ESTATE; }
    HIPCHK(hipSetDevice(ctx_->device));
    if (budget < 1) budget = 1;
    if (!bat_trace_) {   // nobody reads the records: the leader still writes one per completed iteration of the slice
        if (bat_recs_ && bat_rec_stride_ < budget) { HIPCHK(hipFree(bat_recs_)); bat_recs_ = nullptr; }
        if (!bat_recs_) { bat_rec_stride_ = budget; HIPCHK(hipMalloc((void **)&bat_recs_, sizeof(ResRecord) * (size_t)bat_count_ * (size_t)budget)); }
    }
    BatchParams B{};
    B.x = xc_; B.u = uc_; B.p0 = obj_->p[0].p;
    B.st = bat_st_; B.recs = bat_recs_; B.f_x0 = bat_fx0_;
    B.n = bat_n_; B.ld = bat_ld_; B.rec_stride = bat_rec_stride_; B.rec_abs = bat_trace_ ? 1 : 0;
    B.s0 = obj_->s0;
    B.cfg = c; B.cfg.npts = 3; B.cfg.log_on = 0;
    B.budget = budget;
    const void *fn = batch_kernel_for(obj_->kind, 3);
    void *args[] = {&B};
    HIPCHK(hipLaunchKernel(fn, dim3((unsigned)bat_count_), dim3(BLOCK), args, bat_lds_, ctx_->stream));
    total_launches_++;
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
    if (obj_->uses_param()) {
        HIPCHK(hipMemcpyAsync(dst.obj_->p[0].p, obj_->p[0].p + (size_t)b * (size_t)bat_ld_, nb, hipMemcpyDeviceToDevice, ctx_->stream));
        dst.obj_->p_set[0] = true;
    }
    HIPCHK(hipStreamSynchronize(ctx_->stream));
    return CGO_OK;
}

int HipBackend::batch_results(double *x, double *g) {
    if (!x && !g) return CGO_OK;
    const size_t rows = (size_t)bat_count_ * (size_t)bat_ld_;
    std::vector<double> xr(x ? rows : 0), gr(g ? rows : 0);
    if (int rc = download(x ? xr.data() : nullptr, g ? gr.data() : nullptr)) return rc;   // ONE gradient launch over every row
    for (int64_t b = 0; b < bat_count_; ++b) {
        if (x) std::memcpy(x + (size_t)b * bat_n_, xr.data() + (size_t)b * bat_ld_, sizeof(double) * (size_t)bat_n_);
        if (g) std::memcpy(g + (size_t)b * bat_n_, gr.data() + (size_t)b * bat_ld_, sizeof(double) * (size_t)bat_n_);
    }
    return CGO_OK;
}

}  // namespace cgo
