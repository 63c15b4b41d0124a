// cgo_backend_batch_lbfgs_lds.hip — the ahead-of-time instantiations of k_batch_lbfgs_lds (cgo_kernels_batch_lbfgs_lds.hip.hpp),
// batched solves with β = LBFGS(m) whose rows and ring live in LDS during a launch, and the host side of what the tier adds to a
// batch of batched L-BFGS (cgo_backend_batch_lbfgs.hip): the size arithmetic, the dynamic LDS of the launch, the launch itself.
// Rows, ring, states, reset, records, results and the hand-back are the device tier's — the device ring stays where it is, a
// launch writes back what it changed.  A translation unit of its own, so that the device code of every other one is what it was.
#include "cgo_backend_internal.hpp"
#include "cgo_kernels_batch_lbfgs_lds.hip.hpp"

namespace cgo {

using namespace dev;

// The rows of cgo_instances.def: the last row with NPTS ≤ npts, the first row below that.
template <class Obj>
static const void *batch_lbfgs_lds_kernel(int npts) {
    const void *fn = nullptr;
#define ROW(NPTS) if (!fn || npts >= NPTS) fn = (const void *)k_batch_lbfgs_lds<Obj, NPTS>;
    CGO_BATCH_LBFGS_LDS_ROWS(ROW)
#undef ROW
    return fn;
}
static const void *batch_lbfgs_lds_kernel_for(int obj_kind, int npts) {
    switch (obj_kind) {
#define ROW(KIND, T) case KIND: return batch_lbfgs_lds_kernel<T>(npts);
    CGO_OBJ_ROWS(ROW)
#undef ROW
    default: return nullptr;
    }
}

int HipBackend::batch_lbfgs_lds_unroll_for(int nparams) { return batch_lbfgs_lds_u_of(nparams); }
int HipBackend::batch_lbfgs_lds_rows(int nparams, int m) {
    if (nparams < 0 || nparams > MAX_PARAM_SLOTS || m < 1 || m > QN_MAX_M) return 0;
    return dev::batch_lbfgs_lds_rows(nparams, m);
}
// batch_max_n's arithmetic over the tier's rows: (bytes a block may use − static LDS − slack) / (8 · rows), down to even
int64_t HipBackend::batch_lbfgs_lds_ld_of(int64_t max_lds, int64_t static_lds, int rows) {
    if (rows < 1) return 0;
    const int64_t avail = max_lds - static_lds - 512;
    if (avail < 0) return 0;
    const int64_t ld_max = (avail / (8 * (int64_t)rows)) & ~1LL;
    return ld_max < 2 ? 0 : ld_max;
}

// largest ld of one problem of (kind | module, m) on this device; 0: no kernel, no device, a bad m
int64_t HipBackend::batch_lbfgs_lds_max_ld(HipCtx *ctx, int obj_kind, int m, const RtcModule *rtc) {
    if (m < 1 || m > QN_MAX_M) return 0;
    const void *fn = batch_lbfgs_lds_kernel_for(obj_kind, 3);
    const hipFunction_t mf = (obj_kind == CGO_OBJ_USER && rtc) ? rtc->batch_lbfgs_lds(3) : nullptr;
    if (!fn && !mf) return 0;
    if (hipSetDevice(ctx->device) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int max_lds = 0;
    if (hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int64_t static_lds = 0;
    if (fn) {
        hipFuncAttributes fa;
        if (hipFuncGetAttributes(&fa, fn) != hipSuccess) { (void)hipGetLastError(); return 0; }
        static_lds = (int64_t)fa.sharedSizeBytes;
    } else {
        int v = 0;
        if (hipFuncGetAttribute(&v, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, mf) != hipSuccess) { (void)hipGetLastError(); return 0; }
        static_lds = v;
    }
    const int nparams = fn ? (obj_kind == CGO_OBJ_QUAD_DIAG ? 1 : 0) : rtc->n_params;
    return batch_lbfgs_lds_ld_of(max_lds, static_lds, batch_lbfgs_lds_rows(nparams, m));
}

// after batch_lbfgs_alloc: this batch's launches are the LDS tier's
int HipBackend::batch_lbfgs_lds_on() {
    if (!bat_qn_ || bat_m_ < 1 || bat_qn_lds_) { set_error("internal: the LDS tier of batched L-BFGS on a batch of another shape"); return CGO_ESTATE; }
    const bool user = obj_->kind == CGO_OBJ_USER;
    const void *fn = user ? nullptr : batch_lbfgs_lds_kernel_for(obj_->kind, 3);
    if (user) {
        if (!obj_->rtc || !obj_->rtc->batch_lbfgs_lds(3)) { set_error("internal: batched L-BFGS solve in LDS before the objective's program of that tier was compiled"); return CGO_ESTATE; }
    } else if (!fn) { set_error("batched L-BFGS solves: no k_batch_lbfgs_lds instantiation for this objective"); return CGO_EINVAL; }
    const int64_t ld_max = batch_lbfgs_lds_max_ld(ctx_, obj_->kind, bat_m_, obj_->rtc.get());
    if (bat_ld_ > ld_max) { set_error("internal: a batch beyond what one workgroup's LDS holds of a batched L-BFGS problem"); return CGO_ESTATE; }
    HIPCHK(hipSetDevice(ctx_->device));
    bat_lds_ = (size_t)bat_ld_ * 8 * (size_t)batch_lbfgs_lds_rows(obj_->nparams(), bat_m_);
    if (fn && bat_lds_ > 48 * 1024) HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bat_lds_));
    bat_qn_lds_ = true;
    return CGO_OK;
}

int HipBackend::batch_lbfgs_lds_launch(const BatchLbfgsParams &L) {
    void *args[] = {(void *)&L};
    if (obj_->kind == CGO_OBJ_USER) {   // (a module's kernel takes its dynamic LDS as launched)
        const hipFunction_t mf = obj_->rtc ? obj_->rtc->batch_lbfgs_lds(3) : nullptr;
        if (!mf) { set_error("internal: kernel missing from the run-time compiled objective module"); return CGO_EINVAL; }
        HIPCHK(hipModuleLaunchKernel(mf, (unsigned)bat_count_, 1, 1, BLOCK, 1, 1, (unsigned)bat_lds_, ctx_->stream, args, nullptr));
    } else {
        const void *fn = batch_lbfgs_lds_kernel_for(obj_->kind, 3);
        if (!fn) { set_error("batched L-BFGS solves: no k_batch_lbfgs_lds instantiation for this objective"); return CGO_EINVAL; }
        HIPCHK(hipLaunchKernel(fn, dim3((unsigned)bat_count_), dim3(BLOCK), args, bat_lds_, ctx_->stream));
    }
    return CGO_OK;
}

}  // namespace cgo
