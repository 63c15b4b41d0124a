// cgo_backend_batch_rows.hip — the ahead-of-time instantiations of k_batch_rows (cgo_kernels_batch_rows.hip.hpp), the batched
// solves' tier whose problem rows stay in device memory (BatchTier::ROWS), and the facts of its streaming loop.  Everything else
// of a batched solve is cgo_backend_batch.hip's for every tier; this file exists so that k_batch's translation unit compiles to
// what it compiled to before this tier.
#include "cgo_backend_internal.hpp"
#include "cgo_kernels_batch_rows.hip.hpp"

namespace cgo {

using namespace dev;

template <class Obj>
struct BatchDevRows {
    static RowPick at(int npts) {
        RowPick p;
#define ROW(NPTS) p.row(npts, NPTS, (const void *)k_batch_rows<Obj, NPTS>);
        CGO_BATCH_DEVROWS_ROWS(ROW)
#undef ROW
        return p;
    }
};
static RowPick batch_rows_kernel_for(int obj_kind, int npts) { return row_pick_for<BatchDevRows>(obj_kind, npts); }
// this tier's row of the table (batch_tier_of): no dynamic LDS
const BatchTierRow &tier_row_rows() {
    static const BatchTierRow row = {"k_batch_rows", batch_rows_kernel_for, RTC_BATCH_ROWS, "batch_rows:", RTC_BATCH_PROBE, "batch_rows_probe:", false, [](int, int) { return 0; },
                                     "batched solves: no k_batch instantiation for this objective"};
    return row;
}

int64_t HipBackend::batch_rows_max_n() { return (int64_t)BATCH_ROWS_MAX_N; }
int HipBackend::batch_rows_unroll() { return BATCH_ROWS_U; }
int HipBackend::batch_rows_block() { return BLOCK; }

}  // namespace cgo
