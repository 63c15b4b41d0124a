// cgo_backend_batch_lbfgs_lds.hip — the ahead-of-time instantiations of k_batch_lbfgs_lds (cgo_kernels_batch_lbfgs_lds.hip.hpp),
// batched solves with β = LBFGS(m) whose rows and ring live in LDS during a launch (BatchTier::LBFGS_LDS), and the tier's size
// arithmetic.  Everything else of such a batch is the device tier's (cgo_backend_batch_lbfgs.hip) and cgo_backend_batch.hip's.
// A translation unit of its own, so that the device code of every other one is what it was.
#include "cgo_backend_internal.hpp"
#include "cgo_kernels_batch_lbfgs_lds.hip.hpp"

namespace cgo {

using namespace dev;

template <class Obj>
struct BatchLbfgsLdsRows {
    static RowPick at(int npts) {
        RowPick p;
#define ROW(NPTS) p.row(npts, NPTS, (const void *)k_batch_lbfgs_lds<Obj, NPTS>);
        CGO_BATCH_LBFGS_LDS_ROWS(ROW)
#undef ROW
        return p;
    }
};
static RowPick batch_lbfgs_lds_kernel_for(int obj_kind, int npts) { return row_pick_for<BatchLbfgsLdsRows>(obj_kind, npts); }
// this tier's row of the table (batch_tier_of): no PROBE twin in a module
const BatchTierRow &tier_row_lbfgs_lds() {
    static const BatchTierRow row = {"k_batch_lbfgs_lds", batch_lbfgs_lds_kernel_for, RTC_BATCH_LBFGS_LDS, "batch_qn_lds:", RTC_NONE, nullptr, true, HipBackend::batch_lbfgs_lds_rows,
                                     "batched L-BFGS solves: no k_batch_lbfgs_lds instantiation for this objective"};
    return row;
}

int HipBackend::batch_lbfgs_lds_unroll_for(int nparams) { return batch_lbfgs_lds_u_of(nparams); }
int HipBackend::batch_lbfgs_lds_rows(int nparams, int m) {
    if (nparams < 0 || nparams > MAX_PARAM_SLOTS || m < 1 || m > QN_MAX_M) return 0;
    return dev::batch_lbfgs_lds_rows(nparams, m);
}
// THE size arithmetic of both LDS tiers (batch_tier_max_ld): (bytes a block may use − static LDS − 512 of slack) / (8 · rows), down to even
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
    return batch_tier_max_ld(ctx, BatchTier::LBFGS_LDS, obj_kind, m, rtc);
}

}  // namespace cgo
