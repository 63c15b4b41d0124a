// cgo_backend_batch_rows.hip — the ahead-of-time instantiations of k_batch_rows (cgo_kernels_batch_rows.hip.hpp), the batched
// solves' tier whose problem rows stay in device memory, and the facts of its streaming loop.  Everything else of a batched
// solve — allocation, reset, the launch, records, hand-back, results — is cgo_backend_batch.hip's for both tiers; this file
// exists so that k_batch's translation unit compiles to what it compiled to before this tier.
#include "cgo_backend_internal.hpp"
#include "cgo_kernels_batch_rows.hip.hpp"

namespace cgo {

using namespace dev;

// The rows of cgo_instances.def: the last row with NPTS ≤ npts, the first row below that.
template <class Obj>
static const void *batch_rows_kernel(int npts) {
    const void *fn = nullptr;
#define ROW(NPTS) if (!fn || npts >= NPTS) fn = (const void *)k_batch_rows<Obj, NPTS>;
    CGO_BATCH_DEVROWS_ROWS(ROW)
#undef ROW
    return fn;
}
const void *batch_rows_kernel_for(int obj_kind, int npts) {
    switch (obj_kind) {
#define ROW(KIND, T) case KIND: return batch_rows_kernel<T>(npts);
    CGO_OBJ_ROWS(ROW)
#undef ROW
    default: return nullptr;
    }
}

int64_t HipBackend::batch_rows_max_n() { return (int64_t)BATCH_ROWS_MAX_N; }
int HipBackend::batch_rows_unroll() { return BATCH_ROWS_U; }
int HipBackend::batch_rows_block() { return BLOCK; }

}  // namespace cgo
