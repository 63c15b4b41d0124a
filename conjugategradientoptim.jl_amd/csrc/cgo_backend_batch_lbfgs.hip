// cgo_backend_batch_lbfgs.hip — the ahead-of-time instantiations of k_batch_lbfgs (cgo_kernels_batch_lbfgs.hip.hpp), batched
// solves with β = LBFGS(m) (BatchTier::LBFGS), and the host side of what the quasi-Newton tiers add to a batch of the device-rows
// tier: the ring of 2(m+1) rows and the QnState per problem, their reset, and the ring's part of a launch's parameter block.
// Allocation of the rows, reset of the states, the launch, records, results and the hand-back are cgo_backend_batch.hip's; this
// file exists so that the translation units of k_batch and k_batch_rows compile to what they compiled to before.  A run-time
// compiled objective brings its own kernel: the program of the tier of its module (cgo_rtc_batch.hip), compiled by the caller
// before batch_lbfgs_alloc.
#include "cgo_backend_internal.hpp"
#include "cgo_kernels_batch_lbfgs.hip.hpp"

namespace cgo {

using namespace dev;

template <class Obj>
struct BatchLbfgsRows {
    static RowPick at(int npts) {
        RowPick p;
#define ROW(NPTS) p.row(npts, NPTS, (const void *)k_batch_lbfgs<Obj, NPTS>);
        CGO_BATCH_LBFGS_ROWS(ROW)
#undef ROW
        return p;
    }
};
static RowPick batch_lbfgs_kernel_for(int obj_kind, int npts) { return row_pick_for<BatchLbfgsRows>(obj_kind, npts); }
// this tier's row of the table (batch_tier_of): no dynamic LDS, and no PROBE twin in a module
const BatchTierRow &tier_row_lbfgs() {
    static const BatchTierRow row = {"k_batch_lbfgs", batch_lbfgs_kernel_for, RTC_BATCH_LBFGS, "batch_qn:", RTC_NONE, nullptr, true, [](int, int) { return 0; },
                                     "batched L-BFGS solves: no k_batch_lbfgs instantiation for this objective"};
    return row;
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

// lds: the launches keep the rows and the ring in LDS (BatchTier::LBFGS_LDS) — the same allocation, the device ring stays where
// it is and a launch writes back what it changed
int HipBackend::batch_lbfgs_alloc(int m, bool lds) {
    if (!bat_st_ || bat_tier_ != BatchTier::ROWS || bat_qn_ || m < 1 || m > QN_MAX_M) { set_error("internal: batched L-BFGS on a batch of another shape"); return CGO_ESTATE; }
    const BatchTierRow &t = batch_tier_of(lds ? BatchTier::LBFGS_LDS : BatchTier::LBFGS);
    const bool user = obj_->kind == CGO_OBJ_USER;
    const void *fn = user ? nullptr : t.aot(obj_->kind, 3).fn;
    if (user) {
        if (!batch_tier_module_kernel(t, obj_->rtc.get(), 3)) { set_error("internal: batched L-BFGS solve before the objective's batched L-BFGS program was compiled"); return CGO_ESTATE; }
    } else if (!fn) { set_error(t.missing); return CGO_EINVAL; }
    if (bat_n_ > batch_lbfgs_max_n()) { set_error("internal: a batch beyond the pass index of the batched L-BFGS solves"); return CGO_ESTATE; }
    if (lds && bat_ld_ > batch_lbfgs_lds_max_ld(ctx_, obj_->kind, m, obj_->rtc.get())) { set_error("internal: a batch beyond what one workgroup's LDS holds of a batched L-BFGS problem"); return CGO_ESTATE; }
    HIPCHK(hipSetDevice(ctx_->device));
    const size_t ring = (size_t)bat_count_ * (size_t)(m + 1) * (size_t)bat_ld_ * sizeof(double);
    HIPCHK(hipMalloc((void **)&bat_S_, ring));
    HIPCHK(hipMalloc((void **)&bat_Y_, ring));
    HIPCHK(hipMalloc((void **)&bat_qn_, sizeof(QnState) * (size_t)bat_count_));
    bat_m_ = m;
    bat_lds_ = (size_t)bat_ld_ * 8 * (size_t)t.lds_rows(obj_->nparams(), m);
    if (fn && bat_lds_ > 48 * 1024) HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bat_lds_));
    bat_tier_ = lds ? BatchTier::LBFGS_LDS : BatchTier::LBFGS;
    return CGO_OK;
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

int HipBackend::batch_lbfgs_launch_tier(const ResConfig &c, int64_t budget) {
    BatchLbfgsParams L{};
    batch_lbfgs_fill_params(L, c, budget);
    return batch_launch_tier(&L);
}

}  // namespace cgo
