// cgo_backend_batch_lbfgs.hip — the ahead-of-time instantiations of k_batch_lbfgs (cgo_kernels_batch_lbfgs.hip.hpp), batched
// solves with β = LBFGS(m), and the host side of what they add to a batch of the device-rows tier: the ring of 2(m+1) rows
// and the QnState per problem, their reset, and the launch.  Allocation of the rows, reset of the states, records, results and
// the hand-back are cgo_backend_batch.hip's; this file exists so that the translation units of k_batch and k_batch_rows compile
// to what they compiled to before.  A run-time compiled objective brings its own kernel: the batched L-BFGS program of its
// module (cgo_rtc_batch_lbfgs.hip), compiled by the caller before batch_lbfgs_alloc.
#include "cgo_backend_internal.hpp"
#include "cgo_kernels_batch_lbfgs.hip.hpp"

namespace cgo {

using namespace dev;

// The rows of cgo_instances.def: the last row with NPTS ≤ npts, the first row below that.
template <class Obj>
static const void *batch_lbfgs_kernel(int npts) {
    const void *fn = nullptr;
#define ROW(NPTS) if (!fn || npts >= NPTS) fn = (const void *)k_batch_lbfgs<Obj, NPTS>;
    CGO_BATCH_LBFGS_ROWS(ROW)
#undef ROW
    return fn;
}
static const void *batch_lbfgs_kernel_for(int obj_kind, int npts) {
    switch (obj_kind) {
#define ROW(KIND, T) case KIND: return batch_lbfgs_kernel<T>(npts);
    CGO_OBJ_ROWS(ROW)
#undef ROW
    default: return nullptr;
    }
}

int64_t HipBackend::batch_lbfgs_max_n() { return (int64_t)BATCH_LBFGS_MAX_N; }
int HipBackend::batch_lbfgs_unroll() { return BATCH_LBFGS_U; }
int HipBackend::batch_lbfgs_unroll_for(int nparams) { return batch_lbfgs_u_of(nparams); }
int HipBackend::batch_lbfgs_block() { return BLOCK; }

// x, u, every slot, the results' gradient and the ring, [batch][ld] each; the states beside them
double HipBackend::batch_lbfgs_bytes(int64_t batch, int64_t n, int nparams, int m) {
    const double ld = (double)n + (double)(n & 1);
    return (double)batch * (ld * 8.0 * (double)(3 + nparams + 2 * (m + 1)) + (double)sizeof(ResState) + (double)sizeof(QnState) + 16.0);
}

int HipBackend::batch_lbfgs_alloc(int m, bool lds) {
    if (!bat_st_ || !bat_rows_ || bat_qn_ || m < 1 || m > QN_MAX_M) { set_error("internal: batched L-BFGS on a batch of another shape"); return CGO_ESTATE; }
    if (obj_->kind == CGO_OBJ_USER) {   // (lds: the kernel is the LDS tier's program's, checked by batch_lbfgs_lds_on)
        if (!obj_->rtc || !(lds ? obj_->rtc->batch_lbfgs_lds(3) : obj_->rtc->batch_lbfgs(3))) { set_error("internal: batched L-BFGS solve before the objective's batched L-BFGS program was compiled"); return CGO_ESTATE; }
    } else if (!batch_lbfgs_kernel_for(obj_->kind, 3)) { set_error("batched L-BFGS solves: no k_batch_lbfgs instantiation for this objective"); return CGO_EINVAL; }
    if (bat_n_ > batch_lbfgs_max_n()) { set_error("internal: a batch beyond the pass index of the batched L-BFGS solves"); return CGO_ESTATE; }
    HIPCHK(hipSetDevice(ctx_->device));
    const size_t ring = (size_t)bat_count_ * (size_t)(m + 1) * (size_t)bat_ld_ * sizeof(double);
    HIPCHK(hipMalloc((void **)&bat_S_, ring));
    HIPCHK(hipMalloc((void **)&bat_Y_, ring));
    HIPCHK(hipMalloc((void **)&bat_qn_, sizeof(QnState) * (size_t)bat_count_));
    bat_m_ = m;
    return lds ? batch_lbfgs_lds_on() : (int)CGO_OK;   // (cgo_backend_batch_lbfgs_lds.hip)
}

// every problem's ring empty.  (The ring rows need no clearing: a pass reads the slots of stored pairs only, and the padding
// element of an odd n is never read.)  m: the ring depth of the solve that starts — the kernels lay a problem's ring out from its
// QnState's own m, inside the (bat_m_ + 1) rows the ring was allocated with, whose stride stays (a batch that outlives a solve:
// cgo_batch_lbfgs_solve).
int HipBackend::batch_lbfgs_reset(int m) {
    if (!bat_qn_) { set_error("internal: batch_lbfgs_reset before batch_lbfgs_alloc"); return CGO_ESTATE; }
    if (m == 0) m = bat_m_;
    if (m < 1 || m > bat_m_) { set_error("internal: batch_lbfgs_reset with a ring deeper than the one allocated"); return CGO_ESTATE; }
    HIPCHK(hipSetDevice(ctx_->device));
    QnState q;
    std::memset(&q, 0, sizeof q);
    qn_init(q, m);
    std::vector<QnState> qs((size_t)bat_count_, q);
    HIPCHK(hipMemcpy(bat_qn_, qs.data(), sizeof(QnState) * (size_t)bat_count_, hipMemcpyHostToDevice));
    return CGO_OK;
}

void HipBackend::batch_lbfgs_fill_params(BatchLbfgsParams &L, const ResConfig &c, int64_t budget) const {
    batch_fill_params(L.B, c, budget);
    L.S = bat_S_; L.Y = bat_Y_; L.qn = bat_qn_;
    L.ring_stride = (long long)(bat_m_ + 1) * bat_ld_;
}

int HipBackend::batch_lbfgs_launch(const ResConfig &c, int64_t budget, std::vector<ResState> &st, std::vector<double> &f_x0) {
    if (!bat_qn_) { set_error("internal: batched L-BFGS launch on a batch of another shape"); return CGO_ESTATE; }
    HIPCHK(hipSetDevice(ctx_->device));
    if (budget < 1) budget = 1;
    if (!bat_trace_) {   // nobody reads the records: the leader still writes one per completed iteration of the slice
        if (int rc = batch_recs_reserve(budget)) return rc;
    }
    BatchLbfgsParams L{};
    batch_lbfgs_fill_params(L, c, budget);
    void *args[] = {&L};
    if (bat_qn_lds_) {   // rows and ring in LDS during the launch: k_batch_lbfgs_lds (cgo_backend_batch_lbfgs_lds.hip)
        if (int rc = batch_lbfgs_lds_launch(L)) return rc;
    } else if (obj_->kind == CGO_OBJ_USER) {
        const hipFunction_t mf = obj_->rtc ? obj_->rtc->batch_lbfgs(3) : nullptr;
        if (!mf) { set_error("internal: kernel missing from the run-time compiled objective module"); return CGO_EINVAL; }
        HIPCHK(hipModuleLaunchKernel(mf, (unsigned)bat_count_, 1, 1, BLOCK, 1, 1, 0, ctx_->stream, args, nullptr));
    } else {
        const void *fn = batch_lbfgs_kernel_for(obj_->kind, 3);
        if (!fn) { set_error("batched L-BFGS solves: no k_batch_lbfgs instantiation for this objective"); return CGO_EINVAL; }
        HIPCHK(hipLaunchKernel(fn, dim3((unsigned)bat_count_), dim3(BLOCK), args, 0, ctx_->stream));
    }
    total_launches_++;
    st.resize((size_t)bat_count_); f_x0.resize((size_t)bat_count_);
    HIPCHK(hipMemcpyAsync(st.data(), bat_st_, sizeof(ResState) * (size_t)bat_count_, hipMemcpyDeviceToHost, ctx_->stream));
    HIPCHK(hipMemcpyAsync(f_x0.data(), bat_fx0_, sizeof(double) * (size_t)bat_count_, hipMemcpyDeviceToHost, ctx_->stream));
    HIPCHK(hipStreamSynchronize(ctx_->stream));
    return CGO_OK;
}

}  // namespace cgo
