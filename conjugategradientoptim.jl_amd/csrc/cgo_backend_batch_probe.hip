// cgo_backend_batch_probe.hip — cgo_batch_probe: the PROBE twins of k_batch, k_batch_rows, k_batch_lbfgs and k_batch_lbfgs_lds (the rows of
// cgo_instances.def × the objectives, each with the template's PROBE flag set) and the host side of a probe.  A translation unit
// of its own, for the reason cgo_backend_batch_rows.hip and cgo_backend_batch_lbfgs.hip exist: the device code of the product
// units is what it was before the probe.  Which twin a batch takes, what the probe calls it and whether a run-time compiled
// objective has one is the batch's row of batch_tier_of() (cgo_backend_batch.hip).
//
// A probe runs on a batch that batch_alloc (and batch_lbfgs_alloc) made, and its launch arguments are batch_fill_params' /
// batch_lbfgs_fill_params' — the product's ld, slot pointers, s0 / s0v, ring stride and record stride.  What the probe replaces
// is DATA: every buffer is re-allocated with NaN slack behind its used part, the padding element of an odd n is the NaN
// pattern in every row, and the states are the caller's.  Every index a kernel will use is checked here first.
#include "cgo_backend_internal.hpp"
#include "cgo_kernels_batch_lbfgs_lds.hip.hpp"

namespace cgo {

using namespace dev;

static_assert(sizeof(BatchProbePass) == sizeof(cgo_batch_pass) && sizeof(BatchProbeOut) == sizeof(cgo_batch_pass_out), "C ABI twins");
static_assert(BATCH_PROBE_MAX_PASSES == CGO_BATCH_PROBE_MAX_PASSES && BATCH_PROBE_ROW == 64 && RES_MAXP == 7 && QN_MAX_M == 10, "include/cgo.h states them");

// The PROBE twins of every tier's rows, picked as the product's dispatch picks (RowPick).  One expansion per objective holds
// all four tiers, in tier order: the order the kernels were instantiated in before the tiers had a table.
template <class Obj>
struct ProbeRows {
    static RowPick at(int npts, BatchTier tier) {
        RowPick p[BATCH_TIERS];
#define ROW(NPTS) p[(int)BatchTier::LDS].row(npts, NPTS, (const void *)k_batch<Obj, NPTS, true>);
        CGO_BATCH_ROWS(ROW)
#undef ROW
#define ROW(NPTS) p[(int)BatchTier::ROWS].row(npts, NPTS, (const void *)k_batch_rows<Obj, NPTS, true>);
        CGO_BATCH_DEVROWS_ROWS(ROW)
#undef ROW
#define ROW(NPTS) p[(int)BatchTier::LBFGS].row(npts, NPTS, (const void *)k_batch_lbfgs<Obj, NPTS, true>);
        CGO_BATCH_LBFGS_ROWS(ROW)
#undef ROW
#define ROW(NPTS) p[(int)BatchTier::LBFGS_LDS].row(npts, NPTS, (const void *)k_batch_lbfgs_lds<Obj, NPTS, true>);
        CGO_BATCH_LBFGS_LDS_ROWS(ROW)
#undef ROW
        return p[(int)tier];
    }
};
RowPick batch_probe_kernel_for(BatchTier tier, int obj_kind, int npts) { return row_pick_for<ProbeRows>(obj_kind, npts, tier); }

namespace {
// a device buffer of `used` bytes with one 128-B line of the NaN pattern behind it
struct SlackBuf { void *p; size_t used; const char *name; };
constexpr size_t SLACK = 128;
int slack_alloc(std::vector<SlackBuf> &all, void **out, size_t used, const char *name, hipStream_t st) {
    const size_t padded = (used + 7) & ~(size_t)7;
    void *p = nullptr;
    HIPCHK(hipMalloc(&p, padded + SLACK));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)p, (int)PROBE_NAN32, (padded + SLACK) / 4, st));
    all.push_back({p, padded, name});
    *out = p;
    return CGO_OK;
}
// [batch][rows][n] → [batch][rows][ld], the padding element of an odd n the NaN pattern
std::vector<double> padded_rows(const double *src, int64_t rows, int64_t n, int64_t ld) {
    std::vector<double> v((size_t)rows * (size_t)ld);
    unsigned long long nanw = ((unsigned long long)PROBE_NAN32 << 32) | PROBE_NAN32;
    for (int64_t r = 0; r < rows; ++r) {
        std::memcpy(v.data() + (size_t)r * ld, src + (size_t)r * n, sizeof(double) * (size_t)n);
        if (ld > n) std::memcpy(v.data() + (size_t)r * ld + n, &nanw, 8);
    }
    return v;
}
}  // namespace

int HipBackend::batch_probe(cgo_batch_probe_args &p) {
    if (!bat_st_) { set_error("internal: batch_probe before batch_alloc"); return CGO_ESTATE; }
    const int tier = p.tier;
    const bool user = obj_->kind == CGO_OBJ_USER;
    const int64_t batch = bat_count_, n = bat_n_, ld = bat_ld_;
    const int m = bat_m_, K = obj_->nparams();
    if (tier != (int)bat_tier_) { set_error("internal: batch_probe on a batch of another tier"); return CGO_ESTATE; }
    const BatchTierRow &t = batch_tier_of(bat_tier_);
    const bool qnt = t.qn;   // the two tiers of batched L-BFGS: the ring in device memory (2) or, with the rows, in LDS (3)
    // ---- the script: what this tier's loop issues, for the points of the instantiation a solve of this tier launches (npts = 3)
    // (a module's rows are the table's: the points the built-in dispatch picks)
    const RowPick twin = user ? RowPick{nullptr, t.aot(CGO_OBJ_QUAD_DIAG, 3).points} : batch_probe_kernel_for(bat_tier_, obj_->kind, 3);
    const int picked = twin.points, npts = picked, nt = npts < 3 ? npts : 3;
    if (p.npass < 1 || p.npass > CGO_BATCH_PROBE_MAX_PASSES) { set_error("batch probe: 1 … 32 passes"); return CGO_EINVAL; }
    std::vector<BatchProbePass> script((size_t)p.npass);
    bool pushed = false;
    for (int q = 0; q < p.npass; ++q) {
        const cgo_batch_pass &c = p.pass[q];
        bool known = false, k_ok = true;
        switch (c.kind) {
        case 0: known = true; k_ok = c.k >= 1 && c.k <= nt; break;
        case 1: known = !qnt; k_ok = c.k >= 0 && c.k <= npts; break;
        case 2: known = true; break;
        case 3: known = qnt; pushed = pushed || known; break;
        case 4: known = qnt; k_ok = c.k >= 0 && c.k <= npts; break;
        default: break;
        }
        if (!known) { set_error("batch probe: pass " + std::to_string(q) + " (kind " + std::to_string(c.kind) + ") is not one the loop of tier " + std::to_string(tier) + " issues"); return CGO_EINVAL; }
        if (!k_ok) { set_error("batch probe: pass " + std::to_string(q) + " asks for k = " + std::to_string(c.k) + " trial points, the instantiation evaluates " + std::to_string(c.kind == 0 ? nt : npts)); return CGO_EINVAL; }
        BatchProbePass &d = script[(size_t)q];
        std::memset(&d, 0, sizeof d);
        d.kind = c.kind; d.k = c.k; d.a_acc = c.a_acc; d.beta = c.beta;
        double lastp = 0.0;
        for (int j = 0; j < RES_MAXP; ++j) { if (j < c.k) lastp = c.a[j]; d.a[j] = lastp; }   // padded as the loops pad it
        d.co_count = -1;
        if (c.kind == 4) {
            if (c.co_set) {
                if (c.co_count < 0 || c.co_count > m) { set_error("batch probe: pass " + std::to_string(q) + " overrides the coefficients of " + std::to_string(c.co_count) + " pairs, the ring holds m = " + std::to_string(m)); return CGO_EINVAL; }
                d.co_count = c.co_count; d.co_gamma = c.co_gamma;
                for (int j = 0; j < QN_MAX_M; ++j) { d.co_cy[j] = c.co_cy[j]; d.co_cs[j] = c.co_cs[j]; }
            } else if (!pushed) { set_error("batch probe: pass " + std::to_string(q) + " combines before any push of the script and without coefficients of its own"); return CGO_EINVAL; }
        }
    }
    if (!p.x || !p.u) { set_error("batch probe: x and u are required"); return CGO_EINVAL; }
    for (int j = 0; j < K; ++j)
        if (!p.params[j]) { set_error("batch probe: params[" + std::to_string(j) + "] is null, the objective reads " + std::to_string(K) + " parameter slots"); return CGO_EINVAL; }
    std::vector<QnState> qn;
    if (qnt) {
        if (!p.S || !p.Y || !p.qn) { set_error("batch probe: tiers 2 and 3 need S, Y and the quasi-Newton states"); return CGO_EINVAL; }
        qn.resize((size_t)batch);
        std::memcpy(qn.data(), p.qn, sizeof(QnState) * (size_t)batch);
        for (int64_t b = 0; b < batch; ++b) {   // every index the kernel takes from the state
            const QnState &s = qn[(size_t)b];
            bool ok = s.m == m && s.count >= 0 && s.count <= m && s.free_slot >= 0 && s.free_slot <= m;
            for (int j = 0; j <= QN_SLOTS && ok; ++j) ok = s.list[j] >= 0 && s.list[j] <= m;
            if (!ok) { set_error("batch probe: the quasi-Newton state of problem " + std::to_string(b) + " names a slot outside the ring (m, count, free_slot, list against m = " + std::to_string(m) + ")"); return CGO_EINVAL; }
        }
    } else if (p.scalars && !user) { set_error("batch probe: scalars belong to a run-time compiled objective"); return CGO_EINVAL; }
    if (qnt && p.scalars) { set_error("batch probe: the batched L-BFGS solves take no scalar per problem"); return CGO_EINVAL; }

    // ---- the kernel: the PROBE twin
    const void *fn = twin.fn;
    hipFunction_t mf = nullptr;
    if (user && t.probe_prog != RTC_NONE) {
        if (!obj_->rtc) { set_error("internal: a run-time compiled objective without its module"); return CGO_ESTATE; }
        std::string log;
        if (int rc = rtc_compile_program(*obj_->rtc, t.probe_prog, log)) { set_error(std::string("batch probe: ") + rtc_program_what(t.probe_prog) + " did not compile:\n" + log); return rc; }
        mf = batch_tier_module_kernel(t, obj_->rtc.get(), 3, true);
    }
    if (!fn && !mf) { set_error("batch probe: no PROBE instantiation for this objective"); return CGO_EINVAL; }
    HIPCHK(hipSetDevice(ctx_->device));
    hipStream_t st = ctx_->stream;
    {   // the batch was sized for the product instantiation: the twin must fit the same launch
        int max_lds = 0;
        int64_t static_lds = 0;
        HIPCHK(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx_->device));
        if (!kernel_static_lds(fn, mf, static_lds)) { set_error("batch probe: the static LDS of the PROBE instantiation cannot be read"); return CGO_EHIP; }
        if ((size_t)static_lds + bat_lds_ > (size_t)max_lds) { set_error("batch probe: the PROBE instantiation does not fit the launch of the batch"); return CGO_ESTATE; }
        if (fn && bat_lds_ > 48 * 1024) HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bat_lds_));
    }

    // ---- the data: NaN slack behind everything, the padding element of every row the NaN pattern
    if (int rc = probe_prepare()) return rc;   // x, u, the gradient buffers and the parameter slots: whole lines + one line of NaN
    std::vector<SlackBuf> own;
    const size_t rows_n = (size_t)p.npass * (size_t)batch * BATCH_PROBE_ROW, row_b = (size_t)batch * (size_t)ld * sizeof(double);
    void *d_script = nullptr, *d_rows = nullptr, *d_out = nullptr, *d_st = nullptr, *d_fx0 = nullptr, *d_s0v = nullptr, *d_S = nullptr, *d_Y = nullptr, *d_qn = nullptr;
    struct Freer { std::vector<SlackBuf> &v; void *keep[6]; ~Freer() { for (auto &e : v) { bool k = false; for (void *q : keep) k = k || (q && q == e.p); if (!k) (void)hipFree(e.p); } } } freer{own, {}};
    if (int rc = slack_alloc(own, &d_script, sizeof(BatchProbePass) * (size_t)p.npass, "the script", st)) return rc;
    if (int rc = slack_alloc(own, &d_rows, sizeof(double) * rows_n, "the probe's rows", st)) return rc;
    if (int rc = slack_alloc(own, &d_out, sizeof(BatchProbeOut) * (size_t)p.npass * (size_t)batch, "the probe's results", st)) return rc;
    if (int rc = slack_alloc(own, &d_st, sizeof(ResState) * (size_t)batch, "the states", st)) return rc;
    if (int rc = slack_alloc(own, &d_fx0, sizeof(double) * (size_t)batch, "f_x0", st)) return rc;
    if (p.scalars) { if (int rc = slack_alloc(own, &d_s0v, sizeof(double) * (size_t)batch, "the scalars", st)) return rc; }
    if (qnt) {
        const size_t ring = row_b * (size_t)(m + 1);
        if (int rc = slack_alloc(own, &d_S, ring, "the ring S", st)) return rc;
        if (int rc = slack_alloc(own, &d_Y, ring, "the ring Y", st)) return rc;
        if (int rc = slack_alloc(own, &d_qn, sizeof(QnState) * (size_t)batch, "the quasi-Newton states", st)) return rc;
    }
    // the batch's own buffers of these make way (the backend frees what it holds when it goes)
    HIPCHK(hipStreamSynchronize(st));
    (void)hipFree(bat_st_); bat_st_ = (ResState *)d_st; freer.keep[0] = d_st;
    (void)hipFree(bat_fx0_); bat_fx0_ = (double *)d_fx0; freer.keep[1] = d_fx0;
    if (d_s0v) { if (bat_s0v_) (void)hipFree(bat_s0v_); bat_s0v_ = (double *)d_s0v; freer.keep[2] = d_s0v; }
    bat_s0v_on_ = d_s0v != nullptr;
    if (qnt) {
        (void)hipFree(bat_S_); bat_S_ = (double *)d_S; freer.keep[3] = d_S;
        (void)hipFree(bat_Y_); bat_Y_ = (double *)d_Y; freer.keep[4] = d_Y;
        (void)hipFree(bat_qn_); bat_qn_ = (QnState *)d_qn; freer.keep[5] = d_qn;
    }
    bat_trace_ = false;
    if (int rc = batch_recs_reserve(1)) return rc;

    {
        std::vector<double> v = padded_rows(p.x, batch, n, ld);
        HIPCHK(hipMemcpy(xc_, v.data(), row_b, hipMemcpyHostToDevice));
        v = padded_rows(p.u, batch, n, ld);
        HIPCHK(hipMemcpy(uc_, v.data(), row_b, hipMemcpyHostToDevice));
        for (int j = 0; j < K; ++j) {
            v = padded_rows(p.params[j], batch, n, ld);
            HIPCHK(hipMemcpy(obj_->p[j].p, v.data(), row_b, hipMemcpyHostToDevice));
        }
        if (qnt) {
            v = padded_rows(p.S, batch * (m + 1), n, ld);
            HIPCHK(hipMemcpy(bat_S_, v.data(), row_b * (size_t)(m + 1), hipMemcpyHostToDevice));
            v = padded_rows(p.Y, batch * (m + 1), n, ld);
            HIPCHK(hipMemcpy(bat_Y_, v.data(), row_b * (size_t)(m + 1), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(bat_qn_, qn.data(), sizeof(QnState) * (size_t)batch, hipMemcpyHostToDevice));
        }
        if (p.scalars) HIPCHK(hipMemcpy(bat_s0v_, p.scalars, sizeof(double) * (size_t)batch, hipMemcpyHostToDevice));
    }
    std::vector<ResState> hst((size_t)batch);
    for (int64_t b = 0; b < batch; ++b) {   // batch_reset's state, but under way (the script's own R_INIT is a pass like the others)
        ResState &s = hst[(size_t)b];
        std::memset(&s, 0, sizeof s);
        s.a_initial = NAN;
        s.reason = (p.skip && p.skip[b]) ? RES_STOP : RES_BUDGET;
    }
    HIPCHK(hipMemcpy(bat_st_, hst.data(), sizeof(ResState) * (size_t)batch, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(bat_fx0_, 0, sizeof(double) * (size_t)batch));
    HIPCHK(hipMemcpy(d_script, script.data(), sizeof(BatchProbePass) * (size_t)p.npass, hipMemcpyHostToDevice));

    // ---- the launch: the product's arguments, the script behind them
    BatchProbe pr{};
    pr.script = (const BatchProbePass *)d_script; pr.npass = p.npass; pr.rows = (double *)d_rows; pr.out = (BatchProbeOut *)d_out;
    ResConfig cfg;
    std::memset(&cfg, 0, sizeof cfg);   // (the script reads none of it)
    BatchProbeParams A{};
    BatchLbfgsProbeParams AL{};
    void *args[1];
    if (qnt) { batch_lbfgs_fill_params(AL, cfg, 1); AL.pr = pr; args[0] = &AL; }
    else { batch_fill_params(A, cfg, 1); A.pr = pr; args[0] = &A; }
    p.points = picked; p.ld = ld;
    snprintf(p.symbol, sizeof p.symbol, "%s<%s, %d, true>", t.family, obj_tname(), picked);
    if (int rc = batch_launch_kernel(fn, mf, "batch probe: no PROBE instantiation for this objective", args, bat_lds_)) return rc;
    HIPCHK(hipStreamSynchronize(st));

    // ---- what it left
    HIPCHK(hipMemcpy(hst.data(), bat_st_, sizeof(ResState) * (size_t)batch, hipMemcpyDeviceToHost));
    for (int64_t b = 0; b < batch; ++b) {
        const ResState &s = hst[(size_t)b];
        if (p.reason) p.reason[b] = s.reason;
        if (p.done) p.done[b] = s.done;
        if (p.passes) p.passes[b] = s.passes;
    }
    if (p.rows) HIPCHK(hipMemcpy(p.rows, d_rows, sizeof(double) * rows_n, hipMemcpyDeviceToHost));
    if (p.out) HIPCHK(hipMemcpy(p.out, d_out, sizeof(BatchProbeOut) * (size_t)p.npass * (size_t)batch, hipMemcpyDeviceToHost));
    if (p.x_out) HIPCHK(hipMemcpy(p.x_out, xc_, row_b, hipMemcpyDeviceToHost));
    if (p.u_out) HIPCHK(hipMemcpy(p.u_out, uc_, row_b, hipMemcpyDeviceToHost));
    if (qnt) {
        if (p.S_out) HIPCHK(hipMemcpy(p.S_out, bat_S_, row_b * (size_t)(m + 1), hipMemcpyDeviceToHost));
        if (p.Y_out) HIPCHK(hipMemcpy(p.Y_out, bat_Y_, row_b * (size_t)(m + 1), hipMemcpyDeviceToHost));
        if (p.qn_out) HIPCHK(hipMemcpy(p.qn_out, bat_qn_, sizeof(QnState) * (size_t)batch, hipMemcpyDeviceToHost));
    }
    for (int64_t b = 0; b < batch; ++b) {
        const ResState &s = hst[(size_t)b];
        const bool skipped = p.skip && p.skip[b];
        if (skipped ? (s.reason != RES_STOP) : (s.reason != RES_BUDGET || s.passes != p.npass)) {
            set_error("batch probe: problem " + std::to_string(b) + " ran " + std::to_string((long long)s.passes) + " of " + std::to_string(p.npass) + " passes (reason " + std::to_string(s.reason) + ")");
            return CGO_ESTATE;
        }
    }
    if (p.g_out) {   // the results' gradient, by the path batch_results takes
        if (bat_s0v_on_) {
            // (k_batch_grad must leave the padding element alone: the buffer starts as the NaN pattern)
            if (int rc = ensure_ga()) return rc;
            HIPCHK(hipMemsetD32Async((hipDeviceptr_t)ga_.p, (int)PROBE_NAN32, (size_t)batch * (size_t)ld * 2, st));
            if (int rc = batch_grad_rows()) return rc;
            HIPCHK(hipMemcpyAsync(p.g_out, ga_.p, row_b, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        } else {
            if (int rc = download(nullptr, p.g_out)) return rc;
        }
    }
    if (int rc = probe_slack_intact()) return rc;
    std::vector<unsigned> h;
    for (const SlackBuf &e : own) {
        h.assign(SLACK / 4, 0u);
        HIPCHK(hipMemcpy(h.data(), (const char *)e.p + e.used, SLACK, hipMemcpyDeviceToHost));
        for (size_t w = 0; w < h.size(); ++w)
            if (h[w] != PROBE_NAN32) { set_error(std::string("batch probe: the launch wrote past the end of ") + e.name + " (byte " + std::to_string(e.used + 4 * w) + ")"); return CGO_ESTATE; }
    }
    return CGO_OK;
}

}  // namespace cgo
