// cgo_backend_cg.hip — the gradient-free multi-point CG family on the device: k_cg / k_chain launches and their reduction tails,
// the on-device line-search controller (armed rounds), the resident solver.
#include "cgo_backend_internal.hpp"

#include "cgo_kernels.hip.hpp"
#include "cgo_kernels_cg.hip.hpp"
#include "cgo_kernels_cg_path.hip.hpp"
#include "cgo_kernels_chain.hip.hpp"
#include "cgo_kernels_lse.hip.hpp"
#include "cgo_kernels_resident.hip.hpp"

namespace cgo {

using namespace dev;

// ---- gradient-free multi-point CG family (cgo_kernels_cg.hip.hpp) ---------------------------
double bytes_r(int obj_kind, int mode, int64_t n, int n_params) {
    const int p = std::max(obj_kind == CGO_OBJ_QUAD_DIAG ? 1 : 0, n_params);
    return 8.0 * (double)n * (double)r_vectors(mode, p);   // reads + writes of the mode (cgo_modes.hpp): a new row needs no edit here
}

// The point ladder, written once: f(Pts<N>) for the odd N ≤ MAXPTS a launch of `npts` points takes.  A count that is none of
// them takes the largest where that is 7 (k_cg), 1 otherwise (k_chain: anything but 3).
template <int N> using Pts = std::integral_constant<int, N>;
template <int MAXPTS, class F>
static inline void with_points(int npts, F f) {
    static_assert(MAXPTS == 1 || MAXPTS == 3 || MAXPTS == 5 || MAXPTS == 7, "a launch evaluates 1, 3, 5 or 7 trial points");
    if constexpr (MAXPTS >= 3) { if (npts == 3) return f(Pts<3>{}); }
    if constexpr (MAXPTS >= 5) { if (npts == 5) return f(Pts<5>{}); }
    if constexpr (MAXPTS >= 7) { if (npts != 1) return f(Pts<7>{}); }
    return f(Pts<1>{});
}

// the rows of cgo_instances.def; -1: no such row
template <class Obj, bool BIG>
static int launch_cg(int mode, int npts, const RParams &P, int grid, hipStream_t st) {
    // a whole controller round in this launch (never BIG: pipe_fused)
#define ROW(MODE, MAXPTS) if (mode == (MODE) && P.tail.ctl) { with_points<MAXPTS>(npts, [&](auto n) { k_cg_armed<Obj, decltype(n)::value><<<grid, BLOCK, 0, st>>>(P); }); return 0; }
    CGO_CG_ARMED_ROWS(ROW)
#undef ROW
    switch (mode) {
#define ROW(MODE, MAXPTS) case (MODE): with_points<MAXPTS>(npts, [&](auto n) { k_cg<Obj, (MODE), decltype(n)::value, BIG><<<grid, BLOCK, 0, st>>>(P); }); return 0;
    CGO_CG_ROWS(ROW)
#undef ROW
    default: break;
    }
    if constexpr (BIG) {   // the lazy-direction and replay rows: pure-HBM streaming only
        switch (mode) {
#define ROW(MODE, MAXPTS) case (MODE): with_points<MAXPTS>(npts, [&](auto n) { k_cg<Obj, (MODE), decltype(n)::value, true><<<grid, BLOCK, 0, st>>>(P); }); return 0;
        CGO_CG_LAG_ROWS(ROW)
        CGO_CG_REPLAY_ROWS(ROW)
        CGO_CG_LEAN_ROWS(ROW)
#undef ROW
        default: break;
        }
    }
    return -1;
}

// the path rows of cgo_instances.def (k_cg_path: pure-HBM streaming, the 7-point row, `nact` points evaluated); -1: no such row
template <class Obj>
static int launch_cg_path(int mode, int nact, const RParams &P, const RDeep &Q, int grid, hipStream_t st) {
#define ROW(MODE, NACT) if (mode == (MODE) && nact == (NACT)) { k_cg_path<Obj, (MODE), (NACT), true><<<grid, BLOCK, 0, st>>>(P, Q); return 0; }
    CGO_CG_PATH_ROWS(ROW)
#undef ROW
    return -1;
}
// the deep trial rows of cgo_instances.def (k_cg_trial_deep: launch T with more than RMAX steps outstanding); -1: no such row
template <class Obj>
static int launch_cg_deep_t(int npts, const RParams &P, const RDeep &Q, int grid, hipStream_t st) {
#define ROW(NPTS) if (npts == (NPTS)) { k_cg_trial_deep<Obj, (NPTS), true><<<grid, BLOCK, 0, st>>>(P, Q); return 0; }
    CGO_CG_DEEP_T_ROWS(ROW)
#undef ROW
    return -1;
}
static inline bool path_row(int mode, int nact) {
#define ROW(MODE, NACT) if (mode == (MODE) && nact == (NACT)) return true;
    CGO_CG_PATH_ROWS(ROW)
#undef ROW
    return false;
}
static inline bool path_objective(int kind) {   // the objectives that declare a constant Hessian (ObjCurv)
#define ROW(KIND, T) if (kind == KIND) return true;
    CGO_OBJ_CURV_ROWS(ROW)
#undef ROW
    return false;
}
// Predicted path: launches N and S of this solver run as path launches — where the switch is on, the replay
// cycle runs, and both would otherwise run their lean rows.
bool HipBackend::deep_trial(int mode) const {
    return mode == (R_REPLAY | R_TRIAL) && !path_nact_ && path_objective(obj_->kind) && (rep_n_ > RMAX || deep_t_);
}
bool HipBackend::path_rows() const {
    if (!path_on_ || !path_objective(obj_->kind) || replay_depth_ < 2 || !lazy_eligible()) return false;
    const int mode_n = r_mode_of(KK_ACCEPT_TRIAL_NOSTORE), mode_s = R_REPLAY | R_ADT;
    return path_row(mode_n | lean_for(mode_n), MAXP) && path_row(mode_s | lean_for(mode_s), MAXP);
}

// Lean sums: the R_NO… bits to or into `mode` — those of the solver's β flavour where the table has that row.
static inline bool lean_row(int mode) {
#define ROW(MODE, MAXPTS) if (mode == (MODE)) return true;
    CGO_CG_LEAN_ROWS(ROW)
#undef ROW
    return false;
}
int HipBackend::lean_for(int mode) const { return (lean_bits_ && lean_row(mode | lean_bits_)) ? lean_bits_ : 0; }

// a row of an `npts`-point launch (0: npts_for(k)) → the scalars of its first k trial points and, with `dir`, the direction sums
void unpack_r(const double *s, int k, Scal *out, bool dir, int npts) {
    if (npts == 0) npts = npts_for(k);
    for (int j = 0; j < k; ++j) {
        const double *q = s + RS_PER_POINT * j;
        out[j].f = q[RS_F]; out[j].gtu = q[RS_GTU]; out[j].gtgt = q[RS_GTGT]; out[j].gtg = q[RS_GTG];
        out[j].yy = q[RS_YY]; out[j].uy = q[RS_UY]; out[j].ygt = q[RS_YGT];
    }
    if (dir) { out[0].gu = s[RS_PER_POINT * npts]; out[0].uu = s[RS_PER_POINT * npts + 1]; }
}

// stencil launches carry one or three trial points: three only where the mode evaluates trials at all
static inline int chain_npts(int mode, int npts) { return ((mode & R_TRIAL) && npts >= 3) ? 3 : 1; }

// What a launch of (mode, npts) is for this solver — decided HERE for the launch, its profile entry and kernel_symbol.  Pure-HBM: the
// rows that exist in that form only, or above the threshold for what the mode does.  (The stencil objective has no parameter slots.)
RPlan HipBackend::r_plan(int mode, int npts) const {
    const double bytes = bytes_r(obj_->kind, mode, obj_->n_local, obj_->nparams());
    const bool big = r_big_only(mode) || bytes > big_bytes(r_read_only(mode));
    return {big, big ? GRID_BIG : grid_cg(obj_->n_local, chain() ? 1 : npts), chain() ? chain_npts(mode, npts) : npts, bytes};
}
bool HipBackend::adt_is_big() const { return bytes_r(obj_->kind, R_ADT, obj_->n_local, obj_->nparams()) > big_bytes(false); }

int HipBackend::launch_r(int kk, int mode, double a_acc, double beta, const double *a, int k, bool fetch,
                         double *sums) {
    if (int rc = pipe_drain()) return rc;
    pipe_streak_ = 0;  // a host-driven launch: the streak of controller-eligible launches ends
    // A launch that does not rebuild the lagged direction itself: one that reads u gets it stored first, one that overwrites
    // u without reading it (R_INIT, R_RESET) simply ends the lag.  (accept_dir_trial / trial choose the lag modes; a probe
    // never meets the flag.)
    if (u_lag_ && !(mode & R_ULAG)) {
        if (r_reads_u(mode)) { if (int rc = materialize_u()) return rc; }
        else if (mode & (R_INIT | R_RESET)) u_lag_ = false;
    }
    // Steps outstanding (replay): x lags too, and every launch reads x — R_RESET and R_INIT included.  Any launch but N / S / T
    // gets both vectors stored first.
    if (rep_n_ > 0 && !(mode & R_REPLAY)) { if (int rc = materialize_lag()) return rc; }
    // More steps outstanding than RParams holds (deep replay): a path launch and the deep trial launch take the rest in their second
    // argument, every other replay launch gets the pair stored first and starts from an empty list.
    if (rep_n_ > RMAX && (mode & R_REPLAY) && r_base(mode) != R_REPLAY && !path_nact_ && !deep_trial(mode)) { if (int rc = materialize_lag()) return rc; }
    RPlan plan;
    const int npts = path_nact_ ? MAXP : npts_for(k);   // a path launch fills the 7-point row whatever k
    if (int rc = launch_r_kernel(kk, mode, a_acc, beta, a, k, npts, nullptr, &plan)) return rc;
    const int grid = plan.grid;
    total_launches_++;
    const bool has_sums = r_has_sums(mode);
    const bool fused = has_sums && tail_fused(grid);   // the launch's last workgroup already left the sums (finish_tail)
    if (has_sums && chain()) {   // 24- or 32-slot rows: the sums + this rank's eight edge values (cgo_kernels_chain.hip.hpp)
        const bool three = plan.npts == 3;
        const int W = three ? NRC3 : NRC, edge = three ? RC3_EDGE : RC_EDGE, nsums = three ? NR : NR1;
        if (!fused) { if (int rc = finalize_rows(ctx_, grid, W, true)) return rc; }
        const int Wd = ctx_->world(), me = ctx_->rank();
        std::vector<double> raw((size_t)W * Wd);
        double all[NRC3];
        if (int rc = fetch_sums(ctx_, all, MERGE_SUM, W, raw.data())) return rc;
        if (sums) std::memcpy(sums, all, sizeof(double) * nsums);
        if (me > 0) {           // left neighbour's LAST two elements
            const double *e = raw.data() + (size_t)(me - 1) * W + edge + 4;
            halo_xl_[0] = e[0]; halo_xl_[1] = e[1]; halo_ul_[0] = e[2]; halo_ul_[1] = e[3];
        }
        if (me < Wd - 1) {       // right neighbour's FIRST two elements
            const double *e = raw.data() + (size_t)(me + 1) * W + edge;
            halo_xr_[0] = e[0]; halo_xr_[1] = e[1]; halo_ur_[0] = e[2]; halo_ur_[1] = e[3];
        }
        if (probe_) { std::memcpy(probe_row_, all, sizeof(double) * W); probe_len_ = W; }
    } else if (has_sums) {
        if (!fused) { if (int rc = finalize_rows(ctx_, grid, rows_for(npts), true)) return rc; }
        if (fetch) {
            if (int rc = fetch_sums(ctx_, sums, MERGE_SUM, rows_for(npts))) return rc;
        }
        if (probe_ && fetch) { std::memcpy(probe_row_, sums, sizeof(double) * rows_for(npts)); probe_len_ = rows_for(npts); }
    }
    if (prof_on_) prof_commit(kk, plan.bytes);
    return CGO_OK;
}

// ---- lazy direction -------------------------------------------------------------------------------------
// Eligible: the pure-HBM, host-driven launches of a built-in element-wise objective, updated in place.  The lag launches exist
// as BIG instantiations only, and lazy on must compute bit for bit what lazy off computes, so both the plain accept + dir +
// trial launch and the plain trial launch of this solver have to be BIG ones (same partition, same order of additions).
bool HipBackend::lazy_eligible() const {
    if (!lazy_on_ || !rmode_ || chain() || sys_on_ || probe_ || pingpong_ == 1) return false;
    bool aot = false;   // the objectives with ahead-of-time kernels
#define ROW(KIND, T) aot = aot || obj_->kind == KIND;
    CGO_OBJ_ROWS(ROW)
#undef ROW
    if (!aot) return false;
    if (const char *e = getenv("CGO_PINGPONG")) { if (e[0] == '1') return false; }
    if (ctl_depth() > 0) return false;
    return adt_is_big() && r_plan(R_TRIAL, 1).big;
}

// Every reader of the stored direction other than the lag launches: store u_{k+1} = −∇f(x_{k+1}) + β_k·u_k now.  Not a launch
// the solve asked for (total_launches stays); the profile shows it under its own kind.
int HipBackend::materialize_u() {
    if (!u_lag_) return CGO_OK;
    const int64_t asked = total_launches_;
    const int nact = path_nact_;   // (met on the way to a path launch: this pass is not one)
    path_nact_ = 0;
    const int rc = launch_rk(KK_MATERIALIZE_U, 0.0, 0.0, nullptr, 0, false, nullptr);
    path_nact_ = nact;
    total_launches_ = asked;
    if (rc) return rc;
    u_lag_ = false;
    return CGO_OK;
}

// Replay: memory holds (x_k, u_k) and rep_a_ / rep_b_ the (a*, β) of the rep_n_ steps accepted since.  Every
// reader of x or u other than the replay launches: store the current pair now (after a one-step lag of u, if any).  Like
// materialize_u not a launch the solve asked for; the profile shows it under its own kind.
int HipBackend::materialize_lag() {
    if (int rc = materialize_u()) return rc;
    const int64_t asked = total_launches_;
    const int nact = path_nact_;
    path_nact_ = 0;
    int rc = CGO_OK;
    // the pass replays RMAX steps at most: a longer list (deep replay) goes in chunks — store the pair after the first RMAX steps,
    // shift the list, again.  Rare (the end of a solve, a mode switch), so no kernel of its own.
    while (rep_n_ > 0 && rc == CGO_OK) {
        const int all = rep_n_, take = std::min(all, (int)RMAX);
        rep_n_ = take;
        rc = launch_rk(KK_MATERIALIZE_XU, 0.0, 0.0, nullptr, 0, false, nullptr);
        rep_n_ = all;
        if (rc) break;
        rstats_.m++;
        if (all > RMAX) rstats_.m_deep++;
        for (int j = take; j < all; ++j) { rep_a_[j - take] = rep_a_[j]; rep_b_[j - take] = rep_b_[j]; }
        rep_n_ = all - take;
    }
    path_nact_ = nact;
    total_launches_ = asked;
    return rc;
}

int HipBackend::set_replay_depth_now(int d) {
    if (d < 1 || d > RCAP + 1) { set_error("replay depth: 1 … 16"); return CGO_EINVAL; }
    if (d != replay_depth_) { if (int rc = materialize_lag()) return rc; }   // mid-solve: a cycle of the old depth ends first
    replay_depth_ = d;
    return CGO_OK;
}

void HipBackend::set_probe_replay(int nrep, const double *a, const double *beta) {
    probe_rep_n_ = std::max(0, std::min(nrep, (int)RCAP));   // (more than RMAX: path rows and the deep trial launch only — probe_launch refuses the others)
    for (int j = 0; j < probe_rep_n_; ++j) { probe_rep_a_[j] = a[j]; probe_rep_b_[j] = beta[j]; }
}

// accept + direction + trial and trial of the k_cg family.  Where eligible: depth d ≥ 2 — d − 1 launches that store nothing
// (N), then one that replays them and stores both vectors (S); depth 1 — alternating between the two lag launches.
int HipBackend::accept_dir_trial_r(double a_acc, double beta, const double *a, int k, double *s) {
    if (!lazy_eligible()) return launch_rk(KK_ACCEPT_DIR_TRIAL, a_acc, beta, a, k, true, s);
    if (replay_depth_ >= 2) {
        if (int rc = materialize_u()) return rc;
        // launch N while the list is short of the depth and of what the launch about to run replays: a path launch takes RCAP steps
        // (deep replay), any other RMAX — a solver without path rows runs a depth above 8 as depth 8
        if (rep_n_ < replay_depth_ - 1 && rep_n_ < (path_nact_ ? RCAP : RMAX)) {   // launch N: the new pair in registers only
            const int mode_n = r_mode_of(KK_ACCEPT_TRIAL_NOSTORE);
            if (int rc = launch_r(KK_ACCEPT_TRIAL_NOSTORE, mode_n | lean_for(mode_n), a_acc, beta, a, k, true, s)) return rc;
            if (path_nact_) { path_last_n_ = path_nact_; path_count_[path_nact_]++; }
            rep_a_[rep_n_] = a_acc; rep_b_[rep_n_] = beta; rep_n_++;
            rstats_.n++;
            return CGO_OK;
        }
        // launch S: replays the outstanding steps, then today's launch
        const int mode_s = R_REPLAY | R_ADT;
        if (int rc = launch_r(KK_ACCEPT_DIR_TRIAL, mode_s | lean_for(mode_s), a_acc, beta, a, k, true, s)) return rc;
        if (path_nact_) { path_last_s_ = path_nact_; path_count_[path_nact_]++; }
        rep_n_ = 0;
        rstats_.s++;
        return CGO_OK;
    }
    if (!u_lag_) {   // launch A: x ← x + a·u, the new direction in registers only
        if (int rc = launch_rk(KK_ACCEPT_TRIAL_LAZY, a_acc, beta, a, k, true, s)) return rc;
        u_lag_ = true; beta_lag_ = beta;
        return CGO_OK;
    }
    // launch B: rebuilds the direction A left unstored, then today's launch
    if (int rc = launch_r(KK_ACCEPT_DIR_TRIAL, R_ULAG | R_ADT, a_acc, beta, a, k, true, s)) return rc;
    u_lag_ = false;
    return CGO_OK;
}
int HipBackend::trial_r(const double *a, int k, double *s) {
    if (rep_n_ > 0 && lazy_eligible()) {   // launch T — 24 B: nothing stored, steps still outstanding
        rstats_.t++;
        if (rep_n_ > RMAX) rstats_.t_deep++;
        return launch_r(KK_TRIAL, R_REPLAY | R_TRIAL, 0, 0, a, k, true, s);
    }
    if (u_lag_ && lazy_eligible()) return launch_r(KK_TRIAL, R_ULAG | R_TRIAL, 0, 0, a, k, true, s);   // 24 B: nothing stored, still lagged
    return launch_rk(KK_TRIAL, 0, 0, a, k, true, s);
}

// Fused reduction tail (finish_tail): a host-driven launch of the k_cg / k_chain family takes the next sequence number
// itself and publishes where a finalize launch would have.
// Only where the launch is short: at 4096 workgroups the ≈ 0.5 M slot and ticket atomics and the finisher's chain cost the
// pure-HBM launch what the two finalize launches did (n = 1e8: 671 → 683 µs, 1 236 vs 1 230 it/s; gpurun_out/r02_ft).
// A controller-armed round as ONE launch (tail_ctl): wherever the fused tail applies, except for run-time compiled
// objectives, whose kernels carry no controller code.
bool HipBackend::pipe_fused(int grid) const {
    return tail_fused(grid) && obj_->kind != CGO_OBJ_USER && !chain() && ctl_fused_;
}
bool HipBackend::tail_fused(int grid) const {
    static const int cap = [] { const char *e = getenv("CGO_FUSED_TAIL_MAX_GRID"); int v = e ? atoi(e) : 0; return v > 0 ? v : 1024; }();
    return ctx_->fused_tail && grid <= cap && grid <= TAIL_GROUP * TAIL_GROUP;
}
Tail HipBackend::make_tail(bool on) {
    Tail t{};
    if (!on) return t;
    ctx_->seq++;
    t.partials2 = ctx_->partials2_f; t.tickets = ctx_->tickets; t.out = ctx_->out_dev;
    t.strict = ctx_->tail_strict ? 1 : 0;
    ctx_->pub_target(&t.host_out, &t.host_seq);
    ctx_->pub_checked = (t.host_out != nullptr) && !ctx_->tail_strict;
    t.seq = ctx_->seq;
    return t;
}

// the k_cg launch itself (bracketed by the profiling events); `ctl` non-null = controller-armed
int HipBackend::launch_r_kernel(int kk, int mode, double a_acc, double beta, const double *a, int k, int npts,
                                const CtlArgs *ctl, RPlan *plan_out) {
    HIPCHK(hipSetDevice(ctx_->device));
    if (obj_->unset_slot() >= 0) return param_unset_error(obj_->unset_slot());
    const int64_t n = obj_->n_local;
    if (mode & (R_GRAD | R_GRADT)) { if (int rc = ensure_ga()) return rc; }
    const bool has_sums = r_has_sums(mode);
    const RPlan plan = *plan_out = r_plan(mode, npts);
    const bool big = plan.big; const int grid = plan.grid;
    const bool deep_t = deep_trial(mode);
    last_mode_ = mode; last_npts_ = plan.npts; last_big_ = big; last_nact_ = deep_t ? -1 : path_nact_;
    if (path_nact_ && (chain() || !big || ctl || !path_row(mode, path_nact_) || !path_objective(obj_->kind))) { set_error("internal: not a path row"); return CGO_EINVAL; }
    if (chain()) {
        if (int rc = prof_begin(kk)) return rc;
        if (int rc = launch_chain_kernel(mode, a_acc, beta, a, k, plan.npts, big, grid, make_tail(has_sums && !ctl && tail_fused(grid)))) return rc;
        return prof_end();
    }
    RParams P;
    P.x = xc_; P.u = uc_; P.gout = ga_.p; obj_->param_args(P); P.n = n;
    P.xo = xc_; P.uo = uc_;
    P.a_acc = a_acc; P.beta = beta; P.s0 = obj_->s0; P.partials = ctx_->partials;
    P.beta_prev = beta_lag_;
    const int nrep = (mode & R_REPLAY) ? rep_n_ : 0;
    if (nrep > RCAP || (nrep > RMAX && !path_nact_ && !deep_t)) { set_error("internal: more replayed steps than the launch takes"); return CGO_ESTATE; }
    P.nrep = std::min(nrep, (int)RMAX);
    for (int j = 0; j < RMAX; ++j) { P.ra[j] = j < P.nrep ? rep_a_[j] : 0.0; P.rb[j] = j < P.nrep ? rep_b_[j] : 0.0; }
    RDeep Q;   // the steps beyond RMAX (path launches and the deep trial launch)
    Q.nrep2 = nrep - P.nrep;
    for (int j = 0; j < RDEEP; ++j) { Q.ra2[j] = j < Q.nrep2 ? rep_a_[RMAX + j] : 0.0; Q.rb2[j] = j < Q.nrep2 ? rep_b_[RMAX + j] : 0.0; }
    rstats_.max_list = std::max(rstats_.max_list, nrep);
    P.ctl = ctl;
    P.x2 = xn_;
    for (int j = 0; j < MAXP; ++j) P.a[j] = (a && j < k) ? a[j] : ((a && k > 0) ? a[k - 1] : 0.0);
    P.tail = make_tail(has_sums && !ctl && tail_fused(grid));
    if (ctl && pipe_fused(grid)) {
        P.tail.partials2 = ctx_->partials2_f; P.tail.tickets = ctx_->tickets; P.tail.out = ctx_->out_dev;
        P.tail.strict = ctx_->tail_strict ? 1 : 0;
        P.tail.ctl = ctl_dev_; P.tail.ctl_rec = ctl_rec_; P.tail.ctl_seq = ctl_seq_;
        if (!ctx_->single()) {   // the finisher exchanges its block with the peers' GPUs itself (tail_exchange)
            P.tail.xw = ctx_->world(); P.tail.xme = ctx_->rank(); P.tail.xseq0 = epoch_ << 40;
            for (int r = 0; r < P.tail.xw && r < 8; ++r) P.tail.xmail[r] = ctx_->comm->dev_mailbox(r);
        }
    }
    if (P.tail.tickets) P.partials = ctx_->partials_f;
    const bool wr_x = r_writes_x(mode), wr_u = r_writes_u(mode);
    const bool pp = big && !ctl && (wr_x || wr_u) && !(mode & R_PROJ) && pingpong_ready();
    if (pp && wr_x) P.xo = xalt_;
    if (pp && wr_u) P.uo = ualt_;
    if (mode == R_PROJ && !xn_) { set_error("internal: no second iterate buffer"); return CGO_ESTATE; }
    hipStream_t st = ctx_->stream;
    if (int rc = prof_begin(kk)) return rc;
    int r = -2;
    if (path_nact_) {
        switch (obj_->kind) {
#define ROW(KIND, T) case KIND: r = launch_cg_path<T>(mode, path_nact_, P, Q, grid, st); break;
        CGO_OBJ_CURV_ROWS(ROW)
#undef ROW
        default: break;
        }
    } else if (deep_t) {
        if (!big) { set_error("internal: not a deep trial row"); return CGO_EINVAL; }
        switch (obj_->kind) {
#define ROW(KIND, T) case KIND: r = launch_cg_deep_t<T>(plan.npts, P, Q, grid, st); break;
        CGO_OBJ_CURV_ROWS(ROW)
#undef ROW
        default: break;
        }
    } else switch (obj_->kind) {
#define ROW(KIND, T) case KIND: r = big ? launch_cg<T, true>(mode, npts, P, grid, st) : launch_cg<T, false>(mode, npts, P, grid, st); break;
    CGO_OBJ_ROWS(ROW)
#undef ROW
    case CGO_OBJ_USER:
        if (!obj_->rtc) { set_error("user objective has no compiled module"); return CGO_EINVAL; }
        if (r_big_only(mode)) break;   // built-in objectives only: r stays −2
        if (int rc = launch_module(obj_->rtc->cg(mode, npts, big), &P, grid, st)) return rc;
        r = 0;
        break;
    default: break;
    }
    if (r) { set_error("internal: CG kernel mode not instantiated"); return CGO_EINVAL; }
    HIPCHK(hipGetLastError());
    if (pp && wr_x) std::swap(xc_, xalt_);
    if (pp && wr_u) std::swap(uc_, ualt_);
    return prof_end();
}

// ---- chained Rosenbrock: the stencil launches (cgo_kernels_chain.hip.hpp) ----------------------------------------
template <bool BIG>
static int launch_chain(int mode, int npts, const ChainParams &P, int grid, hipStream_t st) {
    switch (mode) {
#define ROW(MODE, MAXPTS) case (MODE): with_points<MAXPTS>(npts, [&](auto n) { k_chain<(MODE), decltype(n)::value, BIG><<<grid, BLOCK, 0, st>>>(P); }); return 0;
    CGO_CHAIN_ROWS(ROW)
#undef ROW
    default: return -1;
    }
}

int HipBackend::launch_chain_kernel(int mode, double a_acc, double beta, const double *a, int k, int npts, bool big, int grid, const Tail &tail) {
    ChainParams P;
    P.tail = tail;
    for (int j = 0; j < 3; ++j) P.a[j] = (a && j < k) ? a[j] : ((a && k > 0) ? a[k - 1] : 0.0);
    P.x = xc_; P.u = uc_; P.xo = xc_; P.uo = uc_; P.gout = ga_.p;
    P.odd = (int)(obj_->n_local & 1);
    P.n = obj_->n_local + P.odd; P.a_acc = a_acc; P.beta = beta; P.partials = tail.tickets ? ctx_->partials_f : ctx_->partials;
    for (int j = 0; j < 2; ++j) { P.hxl[j] = halo_xl_[j]; P.hul[j] = halo_ul_[j]; P.hxr[j] = halo_xr_[j]; P.hur[j] = halo_ur_[j]; }
    // the global vector ends where this rank's shard touches its ends
    P.has_left = obj_->offset > 0 ? 1 : 0;
    P.has_right = obj_->offset + obj_->n_local < obj_->n_global ? 1 : 0;
    const bool wr_x = r_writes_x(mode), wr_u = r_writes_u(mode);
    if (wr_x) P.xo = xalt_;
    if (wr_u) P.uo = ualt_;
    const int r = big ? launch_chain<true>(mode, npts, P, grid, ctx_->stream) : launch_chain<false>(mode, npts, P, grid, ctx_->stream);
    if (r) { set_error("internal: chain kernel mode not instantiated"); return CGO_EINVAL; }
    HIPCHK(hipGetLastError());
    if (wr_x) std::swap(xc_, xalt_);
    if (wr_u) std::swap(uc_, ualt_);
    return CGO_OK;
}

// A k_cg / k_chain instantiation as rocprofv3 prints it minus namespaces.
std::string HipBackend::r_symbol(int mode, int npts, bool big, int nact) const {
    char buf[160];
    if (chain()) snprintf(buf, sizeof buf, "k_chain<%d, %d, %s>", mode, npts, big ? "true" : "false");
    else if (nact < 0) snprintf(buf, sizeof buf, "k_cg_trial_deep<%s, %d, true>", obj_tname(), npts);   // (nact −1: the deep trial launch)
    else if (nact) snprintf(buf, sizeof buf, "k_cg_path<%s, %d, %d, true>", obj_tname(), mode, nact);
    else snprintf(buf, sizeof buf, "k_cg<%s, %d, %d, %s>", obj_tname(), mode, npts, big ? "true" : "false");
    return buf;
}

// The instantiation a launch of kind `kk` uses under the current policy, as rocprofv3 prints it minus namespaces: the kind's mode and point
// rule (cgo_launch_kinds.hpp), the plan the launch itself asks for (r_plan) and, next to them, which lazy / replay kinds this solver issues.
std::string HipBackend::kernel_symbol(int kk) const {
    if (!rmode_) {
        if (obj_->two_phase() || kk == KK_LBFGS_PUSH || kk == KK_LBFGS_LOOP || kk == KK_LBFGS_FINAL) return lbfgs_symbol(kk);
        const int mode = fused_mode(kk);
        return mode < 0 ? "" : fused_symbol(obj_tname(), mode, is_big(obj_->kind, mode, obj_->n_local, obj_->nparams(), pol_.hbm_stream_bytes));
    }
    const RKind *rk = r_kind(kk);
    if (!rk) return "";
    int mode = rk->mode;
    const bool lazy = lazy_eligible();
    switch (kk) {
    case KK_ACCEPT_DIR_TRIAL: if (lazy) mode |= replay_depth_ >= 2 ? R_REPLAY : R_ULAG; break;   // launch S / launch B
    case KK_ACCEPT_TRIAL_LAZY: case KK_MATERIALIZE_U: if (!lazy || replay_depth_ >= 2) return ""; break;
    case KK_ACCEPT_TRIAL_NOSTORE: case KK_MATERIALIZE_XU: if (!lazy || replay_depth_ < 2) return ""; break;
    default: break;
    }
    if (kk == KK_TRIAL && lazy && rep_n_ > RMAX) mode |= R_REPLAY;   // launch T with a deep list outstanding: what runs next
    const RPlan plan = r_plan(mode, rk->pts == PTS_ONE ? 1 : npts_for(rk->pts == PTS_MAX ? max_points() : std::min(max_points(), 3)));
    if ((mode & R_REPLAY) && (mode & R_ACCEPT)) mode |= lean_for(mode);   // N and S: the lean row where that is what runs
    if ((mode & R_REPLAY) && (mode & R_ACCEPT) && path_rows()) {   // … or the path row that last ran for the kind (none yet: the tree's)
        const int last = kk == KK_ACCEPT_TRIAL_NOSTORE ? path_last_n_ : path_last_s_;
        return r_symbol(mode, plan.npts, plan.big, last ? last : MAXP);
    }
    if (kk == KK_TRIAL && deep_trial(mode)) return r_symbol(mode, plan.npts, plan.big, -1);
    return r_symbol(mode, plan.npts, plan.big);
}

// ---- on-device controller (cgo_ctl.hpp) ------------------------------------------------------
// Device block: the controller's config and state, and the argument block the armed launches read.
// `round` numbers the rounds of a solve on the DEVICE: the reduce/controller kernel derives its record slot and its
// sequence word from it, so that a round's kernels carry no per-round host argument at all and whole batches of
// rounds replay from one instantiated hipGraph (pipe_launch_graph).
// (struct CtlDev: cgo_kernels_cg.hip.hpp — the armed launches' own finisher reads and writes it too)

__global__ void k_ctl_init(CtlDev *d, const CtlConfig cfg, const CtlState st, unsigned long long round) {
    d->cfg = cfg;
    d->st = st;
    d->round = round;
    d->args = ctl_args_of(st);
}

// Final reduction stage of a controller-armed launch + the controller itself: rows → sums →
// ctl_step() → arguments of the next launch (device memory) and the round's record (pinned host
// memory, released with a sequence word the host polls).
// One lane running scalar code is the slow part of this kernel (a dependent global load costs ≈ 1–2 µs, a
// PCIe store ≈ 0.2 µs): the device block is staged into LDS and the results are written back — state and
// arguments to HBM, the 30-word record to pinned host memory — by as many lanes as there are words.


template <int N, int THREADS>
__global__ __launch_bounds__(THREADS) void k_finalize_ctl(const double *partials, int rows, double *out, CtlDev *d,
                                                          CtlRecord *rec_ring, unsigned long long *seq_ring) {
    constexpr int G = BLOCK / N;   // the k_cg family's summation order (finalize_rows canon, finish_tail)
    constexpr int WD = sizeof(CtlDev) / 8, WR = sizeof(CtlRecord) / 8;
    __shared__ double sm[G][N];
    __shared__ double fin[CTL_NSUMS];
    __shared__ CtlDev sd;
    __shared__ CtlRecord sr;
    const int tid = threadIdx.x;
    if (tid < WD) ((unsigned long long *)&sd)[tid] = ((const unsigned long long *)d)[tid];
    if (tid < CTL_NSUMS) fin[tid] = 0.0;
    __syncthreads();
    const bool go = sd.st.go != 0;
    const unsigned long long round = sd.round, seq = round + 1;
    CtlRecord *rec_host = rec_ring + (round % PIPE_RING);
    unsigned long long *seq_host = seq_ring + (round % PIPE_RING);
    if (go) {  // same summation order as k_finalize_t: the record must hold what a host-driven launch would
        if (tid < G * N) {
            double t = 0.0;
            const long long total = (long long)rows * N;
            for (long long i = tid; i < total; i += G * N) t += partials[i];
            sm[tid / N][tid % N] = t;
        }
        __syncthreads();
        if (tid < N) {
            double v = 0.0;
#pragma unroll
            for (int g = 0; g < G; ++g) v += sm[g][tid];
            out[tid] = v;
            fin[tid] = v;
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (go) {
            ctl_step(sd.cfg, sd.st, fin, sr);
            sd.args = ctl_args_of(sd.st);
        } else ctl_idle_record(sr);
        sd.round = round + 1;
    }
    __syncthreads();
    if (go && tid < WD) ((unsigned long long *)d)[tid] = ((const unsigned long long *)&sd)[tid];
    if (!go && tid == 0) d->round = round + 1;
    if (tid < WR) {
        ((unsigned long long *)rec_host)[tid] = ((const unsigned long long *)&sr)[tid];
        __threadfence_system();
    }
    __syncthreads();
    if (tid == 0) __hip_atomic_store(seq_host, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Armed rounds: one rank — or several whose GPUs exchange their blocks themselves (device mailboxes, cgo_comm.hip), which only
// the single-launch form of a round does (tail_ctl): built-in objective, grid-stride launch with a fused tail.
int HipBackend::ctl_depth() const {
    if (!(rmode_ && ctx_->host_publish && !obj_->two_phase())) return 0;
    if (ctx_->single()) return ctl_depth_;
    if (!ctx_->dev_exchange() || ctx_->force_gather) return 0;
    return (!adt_is_big() && pipe_fused(grid_cg(obj_->n_local, policy_points()))) ? ctl_depth_ : 0;
}

int HipBackend::pipe_alloc() {
    if (ctl_dev_) return CGO_OK;
    HIPCHK(hipMalloc(&ctl_dev_, sizeof(CtlDev)));
    HIPCHK(hipHostMalloc((void **)&ctl_rec_, sizeof(CtlRecord) * PIPE_RING, hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void **)&ctl_seq_, sizeof(unsigned long long) * PIPE_RING, hipHostMallocDefault));
    std::memset(ctl_rec_, 0, sizeof(CtlRecord) * PIPE_RING);
    std::memset(ctl_seq_, 0, sizeof(unsigned long long) * PIPE_RING);
    pipe_prof_.assign(PIPE_RING, {-1, 0u});
    return CGO_OK;
}

// At solver creation: the controller's blocks, and ONE armed round with the controller stopped — a no-op that files an idle
// record — so that the first launches of k_ctl_init and of the armed kernel (≈ 60 µs each of code-object set-up) do not
// fall into the first armed iteration (BASELINE config 1 runs 25 iterations in all: 14.4k vs 16.5k it/s).
int HipBackend::prepare_controller() {
    if (ctl_depth() <= 0) return CGO_OK;
    if (int rc = pipe_alloc()) return rc;
    if (obj_->unset_slot() >= 0) return CGO_OK;   // nothing to launch on yet
    HIPCHK(hipSetDevice(ctx_->device));
    CtlConfig cc{};
    CtlState st{};
    st.go = 0;
    pipe_npts_ = max_points();
    k_ctl_init<<<1, 1, 0, ctx_->stream>>>((CtlDev *)ctl_dev_, cc, st, pipe_enq_);
    HIPCHK(hipGetLastError());
    if (int rc = pipe_enqueue_round()) return rc;
    return pipe_drain();
}

// the kernels of one controller-armed round: k_cg reading its scalars from the device block, then reduce + controller.
// No argument depends on the round (record slot and sequence number come from CtlDev::round), so the same launches can
// be captured into a hipGraph.
int HipBackend::pipe_round_kernels() {
    RPlan plan;
    const int npts = pipe_npts_, ns = rows_for(npts);
    CtlDev *d = (CtlDev *)ctl_dev_;
    if (int rc = launch_r_kernel(KK_ACCEPT_DIR_TRIAL, R_ADT, 0.0, 0.0, nullptr, 0, npts, &d->args, &plan)) return rc;
    const int grid = plan.grid;
    pipe_checked_ = pipe_fused(grid) && !ctx_->tail_strict;
    if (pipe_fused(grid)) {   // the launch's own finisher reduced, ran the controller and published the record
        if (probe_) probe_note(nullptr, 0, "k_cg_armed<%s, %d>", obj_tname(), last_npts_);
        return CGO_OK;
    }
    if (probe_) probe_note(nullptr, 0, "%s", r_symbol(last_mode_, last_npts_, last_big_).c_str());
    hipStream_t st = ctx_->stream;
    const double *src = ctx_->partials;
    int nrows = grid;
    if (grid > TAIL_GROUP) {
        const int nb = (grid + TAIL_GROUP - 1) / TAIL_GROUP;
        with_width<NR, NR5, NR7, NS>(ns, true, [&](auto w) { k_finalize_t<decltype(w)::value, BLOCK><<<nb, BLOCK, 0, st>>>(ctx_->partials, TAIL_GROUP, grid, ctx_->partials2, nullptr, nullptr, 0); });
        HIPCHK(hipGetLastError());
        if (probe_) probe_note(nullptr, 0, "k_finalize_t<%d>", ns);
        src = ctx_->partials2;
        nrows = nb;
    }
    return pipe_finalize_ctl(src, nrows, ns);
}

// the last kernel of an un-fused round: `nrows` rows of width `ns` → sums → ctl_step → state, arguments, record
int HipBackend::pipe_finalize_ctl(const double *src, int nrows, int ns) {
    CtlDev *d = (CtlDev *)ctl_dev_;
    CtlRecord *rec = (CtlRecord *)ctl_rec_;
    hipStream_t st = ctx_->stream;
    with_width<NR, NR5, NR7, NS>(ns, true, [&](auto w) { constexpr int N = decltype(w)::value, T = N == NS ? BLOCK : 768; k_finalize_ctl<N, T><<<1, T, 0, st>>>(src, nrows, ctx_->out_dev, d, rec, ctl_seq_); });
    HIPCHK(hipGetLastError());
    if (probe_) probe_note(nullptr, 0, "k_finalize_ctl<%d>", ns);
    return CGO_OK;
}

// one round, launched kernel by kernel (with a HIP-event sample when the profiler picks it)
int HipBackend::pipe_enqueue_round() {
    if (int rc = pipe_round_kernels()) return rc;
    const int idx = (int)(pipe_enq_ % PIPE_RING);
    pipe_prof_[idx] = {prof_cur_ ? ring_used_ - 1 : -1, prof_gen_};
    prof_cur_ = false;
    pipe_enq_++;
    return CGO_OK;
}

// `rounds` rounds as ONE hipGraphLaunch: the per-launch host cost (≈ 3.5 µs per kernel, two or three kernels per round)
// is what kept the device waiting for the host at small n although the controller needs no host decision
// (DESIGN.md §2.7).  Instantiated once per (rounds, row width, buffers) and replayed.
int HipBackend::pipe_launch_graph(int rounds) {
    HIPCHK(hipSetDevice(ctx_->device));
    PipeGraph *g = nullptr;
    for (auto &c : graphs_)
        if (c.rounds == rounds && c.npts == pipe_npts_ && c.x == xc_ && c.u == uc_ && c.p0 == obj_->p[0].p && c.n == obj_->n_local) { g = &c; break; }
    if (!g) {
        hipStream_t st = ctx_->stream;
        hipGraph_t graph = nullptr;
        capturing_ = true;
        const size_t syms0 = probe_syms_.size();   // (a probed solver: what the captured rounds launch, for every replay's report)
        hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
        int rc = CGO_OK;
        if (e == hipSuccess) {
            for (int r = 0; r < rounds && rc == CGO_OK; ++r) rc = pipe_round_kernels();
            hipError_t e2 = hipStreamEndCapture(st, &graph);
            if (e2 != hipSuccess) e = e2;
        }
        capturing_ = false;
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (e != hipSuccess || !graph) { set_error(std::string("hipGraph capture of controller rounds failed: ") + hipGetErrorString(e)); (void)hipGetLastError(); return CGO_EHIP; }
        hipGraphExec_t exec = nullptr;
        e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { set_error(std::string("hipGraphInstantiate failed: ") + hipGetErrorString(e)); return CGO_EHIP; }
        graphs_.push_back(PipeGraph{exec, rounds, pipe_npts_, xc_, uc_, obj_->p[0].p, obj_->n_local, {}});
        g = &graphs_.back();
        if (probe_) { g->syms = probe_syms_.substr(syms0 ? syms0 + 3 : 0); probe_syms_.resize(syms0); }
    }
    if (probe_ && !g->syms.empty()) { if (!probe_syms_.empty()) probe_syms_ += " + "; probe_syms_ += g->syms; }
    HIPCHK(hipGraphLaunch((hipGraphExec_t)g->exec, ctx_->stream));
    for (int r = 0; r < rounds; ++r) {
        pipe_prof_[(int)(pipe_enq_ % PIPE_RING)] = {-1, prof_gen_};
        pipe_enq_++;
    }
    graph_rounds_ += rounds;
    return CGO_OK;
}

// enqueue `count` more rounds: graphs of 8 / 4 / 2 rounds where possible.  With the profiler on, every 4th batch goes
// kernel by kernel so that the HIP-event samples of the armed launches keep coming.
int HipBackend::pipe_enqueue(int64_t count) {
    const bool eager = !graph_on_ || (prof_on_ && ((pipe_batches_++ & 3) == 0));
    while (count > 0) {
        int c = 1;
        if (!eager) { c = 8; while (c > count) c >>= 1; }
        if (c == 1) { if (int rc = pipe_enqueue_round()) return rc; }
        else if (int rc = pipe_launch_graph(c)) return rc;
        count -= c;
    }
    return CGO_OK;
}

// wait for the record of global round `id` (0-based)
int HipBackend::pipe_wait(unsigned long long id, CtlRecord &rec) {
    const int idx = (int)(id % PIPE_RING);
    if (pipe_checked_) {   // fused rounds: the record validates itself (tail_publish_record)
        static_assert(sizeof(CtlRecord) % 8 == 0, "record = 8-byte words");
        constexpr int WR = (int)(sizeof(CtlRecord) / 8);
        double words[WR];
        if (int rc = wait_checked(ctx_, ctl_seq_ + idx, id + 1, reinterpret_cast<const double *>(ctl_rec_) + (size_t)idx * WR, WR, words)) return rc;
        std::memcpy(&rec, words, sizeof(CtlRecord));
        if (rec.npts >= 0 && !ctx_->single()) {   // the round exchanged its block between the GPUs: its cost, for cgo_ctx_exchange_stats
            ctx_->xch_count++; ctx_->xch_dev_ms += (double)rec.xwait * 1e-5; ctx_->xch_dev_n++;
        }
        return CGO_OK;
    }
    if (int rc = wait_word(ctx_, ctl_seq_ + idx, id + 1)) return rc;
    rec = ((CtlRecord *)ctl_rec_)[idx];
    return CGO_OK;
}

// Before any launch that is not controller-armed: every round still in flight must be a no-op
// (the controller stops exactly where the host-side state machine leaves the fast path).
int HipBackend::pipe_drain() {
    while (pipe_done_ < pipe_enq_) {
        CtlRecord rec;
        if (int rc = pipe_wait(pipe_done_, rec)) return rc;
        pipe_done_++;
        if (rec.npts >= 0) {
            set_error("internal: the on-device controller ran a launch the host state machine did not ask for");
            return CGO_ESTATE;
        }
    }
    return CGO_OK;
}

int HipBackend::accept_dir_trial_ctl(const CtlConfig &cc, const CtlState &s0, int64_t rounds, Scal *out) {
    if (ctl_depth() <= 0) return accept_dir_trial(s0.a_acc, s0.beta, s0.a, s0.npts, out);
    if (int rc = pipe_alloc()) return rc;
    // how far to run ahead: one more round per first trial accepted in a row (host-observed)
    const int64_t ahead = std::min<int64_t>(std::min<int64_t>(ctl_depth_, pipe_streak_), rounds - 1);
    if (pipe_done_ == pipe_enq_) {  // idle: arm a new batch from the host's state
        if (ahead <= 0) { pipe_streak_++; return accept_dir_trial_keep_streak(s0, out); }
        HIPCHK(hipSetDevice(ctx_->device));
        pipe_npts_ = cc.maxp;
        k_ctl_init<<<1, 1, 0, ctx_->stream>>>((CtlDev *)ctl_dev_, cc, s0, pipe_enq_);
        HIPCHK(hipGetLastError());
        pipe_stopped_ = false;
        if (int rc = pipe_enqueue(1 + ahead)) return rc;
    }
    CtlRecord rec;
    const unsigned long long id = pipe_done_;
    if (int rc = pipe_wait(id, rec)) return rc;
    pipe_done_++;
    if (rec.npts < 0) {  // the controller had stopped before this round: the host drives it
        if (int rc = pipe_drain()) return rc;
        pipe_streak_++;
        return accept_dir_trial_keep_streak(s0, out);
    }
    if (std::memcmp(&rec.a_acc, &s0.a_acc, 8) || std::memcmp(&rec.beta, &s0.beta, 8) || rec.npts != s0.npts ||
        std::memcmp(rec.a, s0.a, 8 * (size_t)s0.npts)) {
        set_error("internal: the on-device controller and the host state machine disagree on a launch");
        return CGO_ESTATE;
    }
    unpack_r(rec.sums, s0.npts, out, true, pipe_npts_);
    total_launches_++;
    pipe_served_++;
    pipe_streak_++;
    const auto &pp = pipe_prof_[(int)(id % PIPE_RING)];
    if (prof_on_) {
        prof_cnt_[KK_ACCEPT_DIR_TRIAL]++;
        prof_bytes_[KK_ACCEPT_DIR_TRIAL] = bytes_r(obj_->kind, R_ADT, obj_->n_local, obj_->nparams());
        if (pp.first >= 0 && pp.second == prof_gen_ && pp.first < ring_used_) {
            ring_[pp.first].kk = KK_ACCEPT_DIR_TRIAL;
            ring_[pp.first].bytes = prof_bytes_[KK_ACCEPT_DIR_TRIAL];
        }
    }
    if (!rec.accepted) pipe_stopped_ = true;
    if (!pipe_stopped_) {  // keep the device `ahead` rounds in front of the host
        // top the run-ahead up in batches (half the depth at a time) so that graph replays stay worth their launch
        const int64_t want = std::min<int64_t>(std::min<int64_t>(ctl_depth_, pipe_streak_), rounds - 1);
        const int64_t have = (int64_t)(pipe_enq_ - pipe_done_);
        if (have < want && (want - have >= (want + 1) / 2 || have == 0))
            if (int rc = pipe_enqueue(want - have)) return rc;
    }
    return CGO_OK;
}

// host-driven accept+dir+trial that does not reset the first-trial streak counter
int HipBackend::accept_dir_trial_keep_streak(const CtlState &s0, Scal *out) {
    const int64_t keep = pipe_streak_;
    const int rc = accept_dir_trial(s0.a_acc, s0.beta, s0.a, s0.npts, out);
    pipe_streak_ = keep;
    return rc;
}


// ---- one launch on host vectors (cgo_solver_probe_launch) ------------------------------------------------------------
// Every buffer a launch of this solver can touch — x, u, their ping-pong partners, both gradient buffers (the second one is
// solvesystem's x2) and the parameter vector — is re-allocated to whole 128-B lines plus one more line, and everything behind
// the elements in use is a NaN pattern: a launch that reads past n_local sums a NaN, one that writes past it is caught by
// probe_slack_intact.  Elements in use: n_local (the stencil objective: its one phantom element of padding too, kept at zero).

int HipBackend::probe_prepare() {
    if (probe_) return CGO_OK;
    if (int rc = pipe_drain()) return rc;
    u_lag_ = false; rep_n_ = 0;   // the probes upload x and u
    HIPCHK(hipSetDevice(ctx_->device));
    HIPCHK(hipStreamSynchronize(ctx_->stream));
    (void)pingpong_ready();   // the engine's own decision, taken now: it would allocate its pair unpadded on the first pure-HBM launch
    const size_t n = (size_t)obj_->n_local, na = n + (chain() ? (n & 1) : 0), np = probe_padded(na);
    DevBuf *bufs[] = {&x_, &u_, &x2_, &u2_, &ga_, &gb_};
    for (DevBuf *b : bufs) {
        if (b == &x2_ || b == &u2_) { if (pingpong_ != 1) continue; }
        if (int rc = b->alloc(np)) return rc;
        HIPCHK(hipMemsetAsync(b->p, 0, na * sizeof(double), ctx_->stream));
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(b->p + na), (int)PROBE_NAN32, (np - na) * 2, ctx_->stream));
    }
    for (int j = 0; j < obj_->nparams(); ++j) {   // the objective's parameter vectors, contents kept
        if (!obj_->p_set[j]) continue;
        DevBuf p;
        if (int rc = p.alloc(np)) return rc;
        HIPCHK(hipMemcpyAsync(p.p, obj_->p[j].p, n * sizeof(double), hipMemcpyDeviceToDevice, ctx_->stream));
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(p.p + n), (int)PROBE_NAN32, (np - n) * 2, ctx_->stream));
        HIPCHK(hipStreamSynchronize(ctx_->stream));
        std::swap(p.p, obj_->p[j].p); std::swap(p.n, obj_->p[j].n);
    }
    HIPCHK(hipStreamSynchronize(ctx_->stream));
    xc_ = x_.p; uc_ = u_.p; xalt_ = x2_.p; ualt_ = u2_.p;
    g_ = ga_.p; gt_ = gb_.p; xn_ = gb_.p;
    lse_have_ = false;
    probe_ = true;
    return CGO_OK;
}

// CGO_OK while every slack word of every buffer still holds the NaN pattern
int HipBackend::probe_slack_intact() {
    const size_t n = (size_t)obj_->n_local, na = n + (chain() ? (n & 1) : 0);
    struct { const DevBuf *b; const char *name; size_t used; int slot; } v[] = {
        {&x_, "x", na, -1}, {&u_, "u", na, -1}, {&x2_, "x (ping-pong)", na, -1}, {&u2_, "u (ping-pong)", na, -1},
        {&ga_, "gradient A", na, -1}, {&gb_, "gradient B / x2", na, -1}, {&obj_->p[0], "parameter vector", n, 0},
        {&obj_->p[1], "parameter vector 1", n, 1}, {&obj_->p[2], "parameter vector 2", n, 2}, {&obj_->p[3], "parameter vector 3", n, 3}};
    std::vector<unsigned> h;
    for (const auto &e : v) {
        if (!e.b->p || (e.slot >= 0 && !(e.slot < obj_->nparams() && obj_->p_set[e.slot]))) continue;
        const size_t words = (e.b->n - e.used) * 2;
        h.assign(words, 0u);
        HIPCHK(hipMemcpyAsync(h.data(), e.b->p + e.used, words * 4, hipMemcpyDeviceToHost, ctx_->stream));
        HIPCHK(hipStreamSynchronize(ctx_->stream));
        for (size_t w = 0; w < words; ++w)
            if (h[w] != PROBE_NAN32) {
                set_error(std::string("probe: the launch wrote past the ") + std::to_string(e.used) + " elements of " + e.name +
                          " (element " + std::to_string(e.used + w / 2) + ")");
                return CGO_ESTATE;
            }
    }
    return CGO_OK;
}

int HipBackend::probe_launch(int kk, int variant, double a_acc, double beta, const double *a, int k, const double *x,
                             const double *u, const double *aux, double *sums, int sums_cap, int *sums_len, double *x_out,
                             double *u_out, double *g_out, std::string &symbol) {
    *sums_len = 0;
    const int want_nact = probe_nact_;   // a lean row as its path twin (cgo_solver_probe_set_path): asked once, for this call
    probe_nact_ = 0;
    const bool want_deep = probe_deep_t_;   // launch T as the deep trial launch (cgo_solver_probe_set_deep_trial): asked once, for this call
    probe_deep_t_ = false;
    const bool lse = obj_->two_phase();
    if (k < 0 || k > MAXP || (k > 0 && !a)) { set_error("probe: 0 ≤ k ≤ 7 trial steps"); return CGO_EINVAL; }
    if (!rmode_ && !lse) return probe_launch_stored(kk, variant, a_acc, beta, a, k, x, u, aux, sums, sums_cap, sums_len, x_out, u_out, g_out, symbol);
    int mode = -1;
    if (lse) {
        if (kk == KK_LSE_STATS && (variant == 0 || variant == LM_NOU || variant == (LM_ACCEPT | LM_DIR))) mode = variant;
        if (kk == KK_LSE_GRAD && variant >= 0 && variant <= 2) mode = variant;   // 0 g⁺ only, 1 + the getβ sums, 2 init (u = −g)
        if (kk == KK_LSE_STATS && mode != LM_NOU && k < 1) mode = -1;
        if (kk == KK_LSE_GRAD && mode != 2 && k < 1) mode = -1;
    } else {
        // the kind's default mode, or one of those its row allows (cgo_launch_kinds.hpp); beside the table: the lean rows of launches
        // N and S, the stencil objective's edge pass, and scaled_norm_parts' two materialise passes (a kind kernel_symbol does not name)
        static constexpr RKind norm_passes{KK_SCALED_NORM, R_GRAD, PTS_ONE, {R_GRADT, 0}};
        const RKind *rk = kk == KK_SCALED_NORM ? &norm_passes : r_kind(kk);
        if (rk && (variant & R_LEAN)) {
            const int full = kk == KK_ACCEPT_DIR_TRIAL ? (R_REPLAY | R_ADT) : (kk == KK_ACCEPT_TRIAL_NOSTORE ? rk->mode : -1);
            if (lean_row(variant) && (variant & ~R_LEAN) == full) mode = variant;
        } else if (rk) {
            const int m = variant ? variant : rk->mode;
            if (r_kind_allows(*rk, m) || (kk == KK_INIT && chain() && m == R_EDGES)) mode = m;
        }
        if (mode > 0 && (mode & (R_TRIAL | R_GRADT | R_PROJ)) && k < 1) mode = -1;
        if (mode > 0 && chain() && k > 3) mode = -1;
        if (mode > 0 && r_big_only(mode) && (chain() || obj_->kind == CGO_OBJ_USER)) mode = -1;
    }
    if (mode < 0) { set_error("probe: kernel kind / variant / trial steps not a launch this solver's engine issues"); return CGO_EINVAL; }
    if (int rc = probe_prepare()) return rc;
    HIPCHK(hipSetDevice(ctx_->device));
    hipStream_t st = ctx_->stream;
    const size_t n = (size_t)obj_->n_local, nb = n * sizeof(double);
    double *ub = lse ? u_.p : uc_;
    double *gb = lse ? gt_ : ga_.p;              // where a gradient is written (R_GRAD, R_GRADT; k_lse_grad: g⁺)
    double *auxb = lse ? g_ : xn_;               // the stored gradient (log-sum-exp) / solvesystem's x2 (R_PROJ)
    // inputs; every buffer the launch may write (or must not read) starts as NaN, so that a dropped element shows
    auto put = [&](double *dst, const double *src) -> int {
        if (src) HIPCHK(hipMemcpyAsync(dst, src, nb, hipMemcpyHostToDevice, st));
        else HIPCHK(hipMemsetD32Async((hipDeviceptr_t)dst, (int)PROBE_NAN32, n * 2, st));
        return CGO_OK;
    };
    if (int rc = put(xc_, x)) return rc;
    if (int rc = put(ub, u)) return rc;
    if (int rc = put(auxb, aux)) return rc;
    if (gb != auxb) { if (int rc = put(gb, nullptr)) return rc; }
    if (!lse && pingpong_ == 1) {
        if (int rc = put(xalt_, nullptr)) return rc;
        if (int rc = put(ualt_, nullptr)) return rc;
    }
    HIPCHK(hipStreamSynchronize(st));
    probe_len_ = 0;
    last_mode_ = -1;
    beta_lag_ = probe_beta_prev_;   // what a launch with R_ULAG reads as β_prev (cgo_solver_probe_set_beta_prev)
    rep_n_ = (!lse && (mode & R_REPLAY)) ? probe_rep_n_ : 0;   // … and one with R_REPLAY as its list (cgo_solver_probe_set_replay)
    for (int j = 0; j < rep_n_; ++j) { rep_a_[j] = probe_rep_a_[j]; rep_b_[j] = probe_rep_b_[j]; }
    int rc = CGO_OK;
    char buf[160];
    if (lse) {
        Scal o;
        if (kk == KK_LSE_STATS) {
            lse_have_ = false;   // the running-maximum form: a probe has no earlier point on the line
            rc = lse_stats(mode, a_acc, beta, k ? a[0] : 0.0, o, mode == (LM_ACCEPT | LM_DIR));
            snprintf(buf, sizeof buf, "k_lse_stats<%d, %s, %s>", last_mode_, last_big_ ? "true" : "false", last_npts_ ? "true" : "false");
        } else {   // (max, Σ) of the trial point: those the last LSE_STATS probe of this solver left, as in the engine
            const bool nb0 = need_beta_;
            need_beta_ = mode == 1;
            rc = lse_grad(mode == 2, k ? a[0] : 0.0, o);
            need_beta_ = nb0;
            snprintf(buf, sizeof buf, "k_lse_grad<%s, %s, %s>", last_mode_ == 1 ? "true" : "false", last_mode_ == 2 ? "true" : "false",
                     last_big_ ? "true" : "false");
        }
        if (rc) return rc;
        symbol = buf;
    } else {
        double s[64];
        if (want_deep && (mode != (R_REPLAY | R_TRIAL) || want_nact || !path_objective(obj_->kind))) { rep_n_ = 0; set_error("probe: not a deep trial launch of this solver"); return CGO_EINVAL; }
        if (rep_n_ > RMAX && !want_nact && !(mode == (R_REPLAY | R_TRIAL) && path_objective(obj_->kind))) {
            rep_n_ = 0; set_error("probe: more than 7 replayed steps: path rows and the deep trial launch only"); return CGO_EINVAL;
        }
        deep_t_ = want_deep;
        if (want_nact) {
            if (!path_row(mode, want_nact) || !path_objective(obj_->kind) || k > want_nact) { rep_n_ = 0; set_error("probe: not a path row of this solver, or more steps than it evaluates"); return CGO_EINVAL; }
            path_nact_ = want_nact;
        }
        rc = launch_r(kk, mode, a_acc, beta, a, k, true, s);
        path_nact_ = 0;
        deep_t_ = false;
        rep_n_ = 0;
        if (rc) return rc;
        symbol = r_symbol(last_mode_, last_npts_, last_big_, last_nact_);
    }
    HIPCHK(hipStreamSynchronize(st));
    if (x_out) HIPCHK(hipMemcpyAsync(x_out, xc_, nb, hipMemcpyDeviceToHost, st));
    if (u_out) HIPCHK(hipMemcpyAsync(u_out, lse ? u_.p : uc_, nb, hipMemcpyDeviceToHost, st));
    if (g_out) HIPCHK(hipMemcpyAsync(g_out, mode == R_PROJ && !lse ? xn_ : gb, nb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (int rc2 = probe_slack_intact()) return rc2;
    *sums_len = probe_len_;
    if (probe_len_ > sums_cap) { set_error("probe: sums_cap smaller than the launch's row"); return CGO_EINVAL; }
    if (probe_len_) std::memcpy(sums, probe_row_, sizeof(double) * probe_len_);
    return CGO_OK;
}

// The same for a solver of the stored-gradient family (k_fused; the host-closure objective: k_trial_point, the closure, then
// k_fused<…, M_BETAONLY>; scaled_norm: k_scaled_norm + k_finalize_maxsum).  The probe calls what the engine calls — trial,
// accept_dir_trial, accept_dir, accept_only, reset_dir, upg_sumsq, host_trial, scaled_norm_parts, and launch itself for M_INIT —
// so that grid, streaming path, finalize form, publication and the g / g⁺ swap of the accepting entry points are the solve's own;
// launch, host_trial and scaled_norm_parts note every instantiation and append every fetched row while probe_stored_ is set.
// `aux` is the vector the launch reads as g: it goes where the entry point's swap will have put g by the time it launches.
// g⁺ for scaled_norm 1 / 4 travels in `x`, which no norm pass reads.  g_out is the buffer that holds g⁺ after the call.
void HipBackend::probe_append(const double *row, int len) {
    if (probe_len_ + len > (int)(sizeof probe_row_ / sizeof probe_row_[0])) return;
    std::memcpy(probe_row_ + probe_len_, row, sizeof(double) * len);
    probe_len_ += len;
}

int HipBackend::probe_launch_stored(int kk, int variant, double a_acc, double beta, const double *a, int k, const double *x,
                                    const double *u, const double *aux, double *sums, int sums_cap, int *sums_len, double *x_out,
                                    double *u_out, double *g_out, std::string &symbol) {
    if (ctx_->world() != 1) { set_error("probe: a single-rank solver"); return CGO_EINVAL; }
    const bool host = obj_->host_closure();
    int mode = -1;
    if (const MKind *mk = m_kind(kk)) {   // the mode this solver's entry point launches, or the other one of the kind's row
        const int m = variant ? variant : (host ? mk->host : fused_mode(kk));
        if (host ? m == mk->host : (m == mk->mode || (mk->alt && m == mk->alt))) mode = m;
    } else if (kk == KK_SCALED_NORM) {
        mode = (variant == 0 || variant == 1 || variant == 3 || variant == 4) ? variant : -1;
    }
    const bool trial_step = kk == KK_TRIAL || kk == KK_ACCEPT_DIR_TRIAL;
    if (mode >= 0 && trial_step && k != 1) mode = -1;   // one trial step per launch in this family
    if (mode < 0) { set_error("probe: kernel kind / variant / trial steps not a launch this solver's engine issues"); return CGO_EINVAL; }
    if (int rc = probe_prepare()) return rc;
    HIPCHK(hipSetDevice(ctx_->device));
    hipStream_t st = ctx_->stream;
    const size_t n = (size_t)obj_->n_local, nb = n * sizeof(double);
    auto put = [&](double *dst, const double *src) -> int {
        if (src) HIPCHK(hipMemcpyAsync(dst, src, nb, hipMemcpyHostToDevice, st));
        else HIPCHK(hipMemsetD32Async((hipDeviceptr_t)dst, (int)PROBE_NAN32, n * 2, st));
        return CGO_OK;
    };
    const bool norm = kk == KK_SCALED_NORM;
    const bool gt_in_x = norm && (mode == 1 || mode == 4);
    const bool swaps = kk == KK_ACCEPT_DIR_TRIAL || kk == KK_ACCEPT_DIR || kk == KK_ACCEPT_ONLY;   // std::swap(g_, gt_) before the launch
    if (int rc = put(xc_, gt_in_x ? nullptr : x)) return rc;
    if (int rc = put(u_.p, u)) return rc;
    if (int rc = put(swaps ? gt_ : g_, aux)) return rc;
    if (int rc = put(swaps ? g_ : gt_, gt_in_x ? x : nullptr)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    probe_len_ = 0;
    probe_syms_.clear();
    probe_stored_ = true;
    int rc = CGO_OK;
    Scal o[MAXP];
    switch (kk) {
    case KK_INIT: {
        double s[NS];
        rc = host ? host_trial(0.0, true, o[0]) : launch_k(KK_INIT, 0, 0, 0, true, s);
        break;
    }
    case KK_TRIAL: {
        const bool nb0 = need_beta_;
        need_beta_ = mode == m_mode_of(KK_TRIAL);
        rc = trial(a, 1, o);
        need_beta_ = nb0;
        break;
    }
    case KK_ACCEPT_DIR_TRIAL: rc = accept_dir_trial(a_acc, beta, a, 1, o); break;
    case KK_ACCEPT_DIR: rc = accept_dir(a_acc, beta, o[0]); break;
    case KK_ACCEPT_ONLY: rc = accept_only(a_acc); break;
    case KK_RESET_DIR: rc = reset_dir(o[0]); break;
    case KK_UPG_NORM: { double uu; rc = upg_sumsq(uu); break; }
    default: { double mx, ss; bool nan; rc = scaled_norm_parts(mode, 0.0, mx, ss, nan); break; }
    }
    probe_stored_ = false;
    if (rc) return rc;
    symbol = probe_syms_;
    HIPCHK(hipStreamSynchronize(st));
    if (x_out) HIPCHK(hipMemcpyAsync(x_out, xc_, nb, hipMemcpyDeviceToHost, st));
    if (u_out) HIPCHK(hipMemcpyAsync(u_out, u_.p, nb, hipMemcpyDeviceToHost, st));
    if (g_out) HIPCHK(hipMemcpyAsync(g_out, gt_, nb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (int rc2 = probe_slack_intact()) return rc2;
    *sums_len = probe_len_;
    if (probe_len_ > sums_cap) { set_error("probe: sums_cap smaller than the launch's rows"); return CGO_EINVAL; }
    if (probe_len_) std::memcpy(sums, probe_row_, sizeof(double) * probe_len_);
    return CGO_OK;
}

// ---- a batch of controller-armed rounds on host vectors (cgo_solver_probe_armed) --------------------------------------------
// What accept_dir_trial_ctl does when it arms a batch — k_ctl_init from the caller's state, pipe_enqueue, pipe_wait per round —
// with every record handed out whole instead of being replayed into the host state machine, then the device block itself.
// Form 2 launches the controller kernel of an un-fused round alone (pipe_finalize_ctl) on a row the caller supplies.
static_assert(sizeof(cgo_ctl_state) == sizeof(CtlState) && sizeof(cgo_ctl_args) == sizeof(CtlArgs) && sizeof(cgo_ctl_record) == sizeof(CtlRecord),
              "include/cgo.h repeats the controller's blocks word for word");
static_assert(offsetof(cgo_ctl_state, npts) == offsetof(CtlState, npts) && offsetof(cgo_ctl_state, it) == offsetof(CtlState, it) &&
              offsetof(cgo_ctl_args, go) == offsetof(CtlArgs, go) && offsetof(cgo_ctl_record, a_acc) == offsetof(CtlRecord, a_acc) &&
              offsetof(cgo_ctl_record, npts) == offsetof(CtlRecord, npts) && offsetof(cgo_ctl_record, xwait) == offsetof(CtlRecord, xwait),
              "include/cgo.h repeats the controller's blocks word for word");

int HipBackend::probe_armed(const cgo_cg_config &cfg, const cgo_ls_config &ls, cgo_armed_probe &p, const double *x, const double *u,
                            double *x_out, double *u_out) {
    p.symbol[0] = 0;
    if (ctx_->world() != 1) { set_error("probe: a single-rank solver"); return CGO_EINVAL; }
    if (ctl_depth() <= 0) { set_error("probe: this solver's engine arms no rounds (controller depth 0)"); return CGO_EINVAL; }
    if (p.form < 0 || p.form > 2 || p.rounds < 1 || p.rounds > CGO_ARMED_PROBE_MAX_ROUNDS || (p.form == 2 && p.rounds != 1)) {
        set_error("probe: form 0 | 1 | 2, 1 ≤ rounds ≤ 32, the controller alone (form 2) runs one round"); return CGO_EINVAL;
    }
    if (p.st.npts < 0 || p.st.npts > CTL_MAXP) { set_error("probe: 0 ≤ npts ≤ 7 trial steps"); return CGO_EINVAL; }
    if (p.form != 2 && !(x && u)) { set_error("probe: armed rounds read x and u"); return CGO_EINVAL; }
    if (int rc = probe_prepare()) return rc;
    if (int rc = pipe_drain()) return rc;
    if (int rc = pipe_alloc()) return rc;
    HIPCHK(hipSetDevice(ctx_->device));
    hipStream_t st = ctx_->stream;
    const size_t nb = (size_t)obj_->n_local * sizeof(double);
    CtlConfig cc;
    cc.ls = ls; cc.eps = p.use_eps ? p.eps : cfg.eps; cc.mu = cfg.beta.mu;
    cc.beta_kind = cfg.beta.kind; cc.maxp = max_points();
    cc.max_iters = p.max_iters;
    CtlState s0;
    std::memcpy(&s0, &p.st, sizeof s0);
    const int ns = rows_for(cc.maxp);
    if (x) HIPCHK(hipMemcpyAsync(xc_, x, nb, hipMemcpyHostToDevice, st));
    if (u) HIPCHK(hipMemcpyAsync(uc_, u, nb, hipMemcpyHostToDevice, st));
    if (p.form == 2) HIPCHK(hipMemcpyAsync(ctx_->partials, p.row, sizeof(double) * ns, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    u_lag_ = false; rep_n_ = 0;
    pipe_npts_ = cc.maxp;
    probe_syms_.clear();
    const unsigned long long first = pipe_enq_;
    k_ctl_init<<<1, 1, 0, st>>>((CtlDev *)ctl_dev_, cc, s0, pipe_enq_);
    HIPCHK(hipGetLastError());
    pipe_stopped_ = false;
    int rc = CGO_OK;
    if (p.form == 2) {
        pipe_checked_ = false;   // k_finalize_ctl releases the plain sequence number
        rc = pipe_finalize_ctl(ctx_->partials, 1, ns);
        if (!rc) { pipe_prof_[(int)(pipe_enq_ % PIPE_RING)] = {-1, prof_gen_}; pipe_enq_++; }
    } else {
        const bool graph0 = graph_on_;
        graph_on_ = p.form == 1;
        rc = pipe_enqueue(p.rounds);
        graph_on_ = graph0;
    }
    for (unsigned long long id = first; !rc && id < pipe_enq_; ++id) {
        CtlRecord rec;
        rc = pipe_wait(id, rec);
        if (!rc) { std::memcpy(&p.rec[id - first], &rec, sizeof rec); pipe_done_++; }
    }
    if (rc) {   // nothing is retried: the stream is left to finish what it holds, the pipe counts as drained
        (void)hipStreamSynchronize(st);
        pipe_done_ = pipe_enq_;
        return rc == CGO_EINVAL ? rc : CGO_ESTATE;
    }
    HIPCHK(hipStreamSynchronize(st));
    CtlDev d;
    double od[CTL_NSUMS] = {};
    HIPCHK(hipMemcpyAsync(&d, ctl_dev_, sizeof d, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(od, ctx_->out_dev, sizeof(double) * ns, hipMemcpyDeviceToHost, st));
    if (x_out) HIPCHK(hipMemcpyAsync(x_out, xc_, nb, hipMemcpyDeviceToHost, st));
    if (u_out) HIPCHK(hipMemcpyAsync(u_out, uc_, nb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::memcpy(&p.st_out, &d.st, sizeof d.st);
    std::memcpy(&p.args_out, &d.args, sizeof d.args);
    p.round_out = d.round;
    std::memcpy(p.out_dev, od, sizeof od);
    p.width = ns; p.maxp = cc.maxp;
    if (int rc2 = probe_slack_intact()) return rc2;
    if (probe_syms_.size() >= sizeof p.symbol) { set_error("probe: the symbol list does not fit"); return CGO_ESTATE; }
    std::snprintf(p.symbol, sizeof p.symbol, "%s", probe_syms_.c_str());
    return CGO_OK;
}

// ---- resident solver (cgo_resident.hpp, cgo_kernels_resident.hip.hpp) -------------------------------------------------
// Which shards: the built-in element-wise objectives under a CG β and one of the two bisection line searches, on one rank,
// while x, u (and the parameter vector) fit the LDS of the chip's CUs — one workgroup per CU at most, so that every
// workgroup of the launch is resident and their all-gather can complete.  CGO_RESIDENT=0 switches it off,
// CGO_RES_CHUNK sets the elements per workgroup (default 4096: n = 1e6 → 245 workgroups; n ≤ 4096 → ONE workgroup and no
// exchange at all), CGO_RES_POINTS the trial steps per pass (default 3).
constexpr int64_t RES_REC_CAP = 4096;     // iterations per slice at most
constexpr int64_t RES_LOG_CAP = 1 << 16;  // trial-log entries per slice

// The rows of cgo_instances.def, PROBE = the twins cgo_solver_probe_resident launches (the script in place of res_iterate):
// the last row with NPTS ≤ npts, the first row below that.
template <class Obj, bool PROBE>
static const void *res_kernel(int npts) {
    const void *fn = nullptr;
#define ROW(NPTS) if (!fn || npts >= NPTS) fn = (const void *)k_resident<Obj, NPTS, PROBE>;
    CGO_RESIDENT_ROWS(ROW)
#undef ROW
    return fn;
}
template <bool PROBE>
static const void *res_kernel_for(int obj_kind, int npts) {
    switch (obj_kind) {
    case CGO_OBJ_ROSENBROCK_CHAINED: {   // ONE workgroup
        const void *fn = nullptr;
#define ROW(NPTS) if (!fn || npts >= NPTS) fn = (const void *)k_resident_chain<NPTS, PROBE>;
        CGO_RESIDENT_CHAIN_ROWS(ROW)
#undef ROW
        return fn;
    }
#define ROW(KIND, T) case KIND: return res_kernel<T, PROBE>(npts);
    CGO_OBJ_ROWS(ROW)
#undef ROW
    default: return nullptr;
    }
}

int HipBackend::res_plan() {
    if (res_grid_ != 0) return res_grid_ > 0 ? res_grid_ : 0;
    res_grid_ = -1;   // decided: does not fit, unless the plan below completes
    const int64_t want = pol_.resident_chunk >= 2 ? (int64_t)(pol_.resident_chunk & ~1) : (int64_t)4096;
    const int pts = (pol_.resident_points == 1 || pol_.resident_points == 3 || pol_.resident_points == 7) ? pol_.resident_points : 3;
    res_npts_ = pts;
    const void *fn = res_kernel_for<false>(obj_->kind, res_npts_);
    // a run-time compiled objective carries its own copy of the kernel (k_resident<UserObjective, 3>, cgo_rtc.hip)
    hipFunction_t mf = (obj_->kind == CGO_OBJ_USER && obj_->rtc) ? obj_->rtc->resident(res_npts_) : nullptr;
    if (!fn && !mf) return 0;
    const int64_t n = obj_->n_local;
    const int vecs = chain() ? 4 : 2 + obj_->nparams();   // x, u and every parameter slot (the stencil objective: two LDS copies of x and of u)
    if (chain() && res_npts_ > 3) res_npts_ = 3;
    int max_lds = 0;
    if (hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx_->device) != hipSuccess) { (void)hipGetLastError(); return 0; }
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
    const int64_t avail = (int64_t)max_lds - static_lds - 512;
    int64_t chunk_max = (avail / (8 * vecs)) & ~1LL;
    if (chunk_max < 2) return 0;
    const int cus = std::min(ctx_->num_cu > 0 ? ctx_->num_cu : 256, RES_GSIZE * RES_GROUPS);   // (the two-level exchange holds 16 groups of 16)
    int64_t chunk = std::min<int64_t>(want, chunk_max);
    if (chain()) {   // the whole (padded) vector in ONE workgroup, or not at all
        chunk = n + (n & 1);
        if (chunk > chunk_max) return 0;
    }
    int64_t grid = (n + chunk - 1) / chunk;
    if (grid > cus) {   // more elements per workgroup, up to what the LDS holds
        chunk = (((n + cus - 1) / cus) + 1) & ~1LL;
        if (chunk > chunk_max) return 0;
        grid = (n + chunk - 1) / chunk;
    }
    const size_t lds = (size_t)chunk * 8 * vecs;
    if (fn && lds > 48 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int per_cu = 0;
    if (fn) { if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, BLOCK, lds) != hipSuccess || per_cu < 1) { (void)hipGetLastError(); return 0; } }
    else if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, mf, BLOCK, lds) != hipSuccess || per_cu < 1) { (void)hipGetLastError(); return 0; }
    if (grid > (int64_t)cus * per_cu) return 0;   // every workgroup must be resident: they wait for one another
    res_chunk_ = chunk; res_lds_ = lds; res_grid_ = (int)grid;
    return res_grid_;
}

bool HipBackend::resident_ready(const cgo_cg_config &cfg, const cgo_ls_config &ls) const {
    if (!res_on_ || !rmode_ || sys_on_ || !ctx_->single()) return false;
    if (cfg.beta.kind == CGO_BETA_LBFGS) return false;
    if (ls.kind != CGO_LS_STRONG_WOLFE_BISECTION && ls.kind != CGO_LS_WOLFE_BISECTION) return false;
    return const_cast<HipBackend *>(this)->res_plan() > 0;
}

int HipBackend::res_alloc() {
    if (res_state_) return CGO_OK;
    HIPCHK(hipSetDevice(ctx_->device));
    HIPCHK(hipHostMalloc((void **)&res_state_, sizeof(ResState), hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void **)&res_recs_, sizeof(ResRecord) * RES_REC_CAP, hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void **)&res_done_, 64, hipHostMallocDefault));
    *res_done_ = 0;
    const size_t xb = sizeof(double) * RES_XBUFS * ((size_t)res_grid_ + RES_GROUPS) * RES_WMAX;   // workgroup rows, then group rows
    HIPCHK(hipMalloc((void **)&res_xbuf_, xb));
    HIPCHK(hipMemsetD32((hipDeviceptr_t)res_xbuf_, (int)(TAIL_EMPTY & 0xFFFFFFFFull), xb / 4));
    HIPCHK(hipMalloc((void **)&res_recs_dev_, sizeof(ResRecord) * RES_REC_CAP));
    HIPCHK(hipMalloc((void **)&res_err_, 64));     // [0] error flags, [1] workgroups that have reported in
    HIPCHK(hipMemset(res_err_, 0, 64));
    if (res_grid_ > 1) {   // a multi-workgroup slice leaves x, u in these; swapped in on a good global verdict only
        if (int rc = res_xo_.alloc((size_t)obj_->n_local)) return rc;
        if (int rc = res_uo_.alloc((size_t)obj_->n_local)) return rc;
    }
    HIPCHK(hipDeviceSynchronize());
    res_round_ = 0;
    return CGO_OK;
}

// The host bookkeeping of a resident launch, shared by resident_run and probe_resident: where the launch leaves x, u (OTHER
// buffers when it has more than one workgroup), the kernel arguments that do not depend on what the launch computes, the swap
// after a good GLOBAL verdict, and the reset after a launch whose exchange gave up.
void HipBackend::res_out_buffers(double *&xo, double *&uo) const {
    const bool oop = res_grid_ > 1;
    xo = oop ? ((xc_ == res_xo_.p) ? res_xin_ : res_xo_.p) : xc_;
    uo = oop ? ((uc_ == res_uo_.p) ? res_uin_ : res_uo_.p) : uc_;
}

void HipBackend::res_fill_params(ResParams &P, double *xo, double *uo) {
    P.x = xc_; P.u = uc_; obj_->param_args(P); P.n = obj_->n_local; P.chunk = res_chunk_; P.s0 = obj_->s0;
    P.xo = xo; P.uo = uo; P.arrive = res_err_ + 1;
    P.inject = -1;
    P.st_out = res_state_; P.recs = res_recs_dev_;
    P.recs_host = res_recs_; P.log_host = res_log_;
    P.xbuf = res_xbuf_; P.round0 = res_round_; P.err = res_err_;
    P.done_seq = res_done_; P.seq = ++res_seq_;
}

void HipBackend::res_swap_in(double *xo, double *uo) {
    res_xin_ = xc_; res_uin_ = uc_;
    xc_ = xo; uc_ = uo;
}

int HipBackend::res_error_reset() {
    HIPCHK(hipStreamSynchronize(ctx_->stream));
    const size_t xb = sizeof(double) * RES_XBUFS * ((size_t)res_grid_ + RES_GROUPS) * RES_WMAX;
    HIPCHK(hipMemsetD32((hipDeviceptr_t)res_xbuf_, (int)(TAIL_EMPTY & 0xFFFFFFFFull), xb / 4));
    HIPCHK(hipMemset(res_err_, 0, 64));
    res_round_ = 0;
    return CGO_OK;
}

int HipBackend::resident_run(const ResConfig &c, ResState &s, int64_t budget, std::vector<ResRecord> &recs, std::vector<ResLog> &log) {
    if (int rc = pipe_drain()) return rc;
    pipe_streak_ = 0;
    if (int rc = materialize_lag()) return rc;   // the slice loads the stored iterate and direction
    if (res_plan() <= 0) { set_error("internal: resident slice on a shard that does not fit"); return CGO_ESTATE; }
    if (obj_->unset_slot() >= 0) return param_unset_error(obj_->unset_slot());
    if (int rc = res_alloc()) return rc;
    HIPCHK(hipSetDevice(ctx_->device));
    if (c.log_on && !res_log_) {
        HIPCHK(hipHostMalloc((void **)&res_log_, sizeof(ResLog) * RES_LOG_CAP, hipHostMallocDefault));
        HIPCHK(hipMalloc((void **)&res_log_dev_, sizeof(ResLog) * RES_LOG_CAP));
    }
    ResParams P{};
    const bool oop = res_grid_ > 1;
    double *xo, *uo;
    res_out_buffers(xo, uo);
    res_fill_params(P, xo, uo);
    if (res_slices_ == 0) { if (const char *e = getenv("CGO_RES_INJECT_GIVEUP")) P.inject = atoi(e); }   // test hook: first slice only
    P.cfg = c; P.cfg.npts = res_npts_;
    P.st = s;
    if (P.st.ncache > res_npts_) P.st.ncache = res_npts_;   // (a wider host launch left more trial results than a pass of this width keeps)
    P.budget = std::min<int64_t>(budget, RES_REC_CAP);
    P.log = res_log_dev_; P.log_cap = c.log_on ? RES_LOG_CAP : 0;
    static const bool timing = getenv("CGO_RES_TIMING") != nullptr;
    P.timing = timing ? 1 : 0;
    const void *fn = res_kernel_for<false>(obj_->kind, res_npts_);
    void *args[] = {&P};
    const double h0 = timing ? now_ns() : 0.0;
    if (int rc = prof_begin(KK_RESIDENT)) return rc;
    if (fn) HIPCHK(hipLaunchKernel(fn, dim3(res_grid_), dim3(BLOCK), args, res_lds_, ctx_->stream));
    else HIPCHK(hipModuleLaunchKernel(obj_->rtc->resident(res_npts_), res_grid_, 1, 1, BLOCK, 1, 1, (unsigned)res_lds_, ctx_->stream, args, nullptr));
    if (int rc = prof_end()) return rc;
    total_launches_++;
    const double h1 = timing ? now_ns() : 0.0;
    if (int rc = wait_word(ctx_, res_done_, res_seq_)) return rc;
    const double h2 = timing ? now_ns() : 0.0;
    if (timing) fprintf(stderr, "[cgo resident] host: enqueue %.1f us, wait for the slice %.1f us\n", (h1 - h0) * 1e-3, (h2 - h1) * 1e-3);
    s = *res_state_;
    res_round_ += (unsigned long long)s.passes;
    res_slices_++;
    {
        if (timing) fprintf(stderr, "[cgo resident] slice: %lld iterations, %lld passes, grid %d x %lld elements, reason %d: %.1f us in all; per pass compute %.2f, "
                                 "workgroup reduce %.2f, exchange %.2f us; outside the passes %.2f us per iteration (machine %.2f, evals incl. passes %.2f, post %.2f); shader clock %.0f MHz\n",
                         (long long)s.done, (long long)s.passes, res_grid_, (long long)res_chunk_, (int)s.reason, s.t_total * 1e-2,
                         s.t_compute * 1e-2 / std::max<double>(s.passes, 1), s.t_reduce * 1e-2 / std::max<double>(s.passes, 1),
                         s.t_exchange * 1e-2 / std::max<double>(s.passes, 1),
                         (s.t_total - s.t_compute - s.t_reduce - s.t_exchange) * 1e-2 / std::max<double>(s.done, 1),
                         s.t_machine * 1e-2 / std::max<double>(s.done, 1), s.t_eval * 1e-2 / std::max<double>(s.done, 1), s.t_post * 1e-2 / std::max<double>(s.done, 1),
                         (double)s.t_cycles / std::max<double>((double)s.t_total * 1e-2, 1e-9));
    }
    if (s.reason == RES_ERROR) {
        // The exchange gave up: some workgroup of the launch was not running while the others waited for its row.  That
        // happens when ANOTHER process's kernels hold CUs (two persistent launches can each be partially resident and wait
        // for workgroups the other one's keep out).  Nothing is lost: a slice writes x, u back only when it ends well, so
        // the state is still that of the slice's start — hand the whole slice to the launch-per-trial engine and keep this
        // solver off the resident path from here on (correct under any sharing of the GPU, at the old speed).
        if (int rc = res_error_reset()) return rc;
        res_on_ = false;
        res_gave_up_++;
        s = P.st;   // the state the slice started from
        s.done = 0; s.log_len = 0; s.evals = 0; s.passes = 0; s.reason = RES_HOST;
        recs.clear(); log.clear();
        return CGO_OK;
    }
    if (oop && s.done > 0) res_swap_in(xo, uo);   // a good slice, by the verdict of ALL its workgroups: its x, u become the iterate
    res_iters_ += s.done;
    recs.assign(res_recs_, res_recs_ + s.done);
    if (c.log_on) log.assign(res_log_, res_log_ + s.log_len); else log.clear();
    // state moved once per slice: load x, u (+ D) and store x, u
    if (prof_on_) prof_commit(KK_RESIDENT, 8.0 * (double)obj_->n_local * (double)(2 + obj_->nparams() + (s.done > 0 ? 2 : 0)));
    return CGO_OK;
}

// ---- a script of resident passes in one launch (cgo_solver_probe_resident) ---------------------------------------------
// Everything but the kernel's PROBE flag is resident_run's: the plan, res_alloc's buffers, the out-of-place rule and its
// swap, round0 and the rounds added afterwards.  x, u, xo, uo and the parameter vector carry NaN slack (probe_prepare; xo, uo
// here).  Buffers a good launch must write start as NaN, so that an element it drops shows.
int HipBackend::probe_resident(const cgo_cg_config &cfg, const cgo_ls_config &ls, cgo_resident_probe &p, const double *x, const double *u,
                               double *rows, int64_t rows_cap, double *x_out, double *u_out) {
    static_assert(sizeof(ResProbePass) == sizeof(cgo_resident_pass) && sizeof(ResProbeOut) == sizeof(cgo_resident_pass_out), "C ABI twins");
    static_assert(RES_MAXP == 7 && RES_WMAX == 56, "include/cgo.h states them");
    p.grid = 0; p.points = 0; p.chunk = 0; p.round0 = 0; p.err_word = 0; p.wrote_back = 0; p.symbol[0] = 0;
    if (!resident_ready(cfg, ls)) { set_error("probe: this solver's engine would not run the resident solver (objective, β, line search, size or policy)"); return CGO_EINVAL; }
    if (obj_->unset_slot() >= 0) return param_unset_error(obj_->unset_slot());
    if (p.npass < 1 || p.npass > CGO_RESIDENT_PROBE_MAX_PASSES) { set_error("probe: 1 … 32 passes"); return CGO_EINVAL; }
    const int npts = res_npts_, nt = npts < 3 ? npts : 3;
    for (int q = 0; q < p.npass; ++q) {
        const cgo_resident_pass &c = p.pass[q];
        const bool ok = c.kind == 0 ? (c.k >= 1 && c.k <= nt) : (c.kind == 1 && c.k >= 0 && c.k <= npts);
        if (!ok) { set_error("probe: pass " + std::to_string(q) + " is not one the resident loop of this width issues"); return CGO_EINVAL; }
    }
    if (rows_cap < (int64_t)p.npass * res_grid_ * RES_WMAX) { set_error("probe: rows_cap smaller than npass · grid · 56"); return CGO_EINVAL; }
    if (int rc = probe_prepare()) return rc;
    if (int rc = res_alloc()) return rc;
    HIPCHK(hipSetDevice(ctx_->device));
    hipStream_t st = ctx_->stream;
    const size_t n = (size_t)obj_->n_local, nb = n * sizeof(double);
    const bool oop = res_grid_ > 1;
    const size_t rows_n = (size_t)CGO_RESIDENT_PROBE_MAX_PASSES * res_grid_ * RES_WMAX;
    if (!res_pr_ready_) {
        if (oop) {   // the out-of-place partners: whole lines + one line of NaN, as probe_prepare gives x and u
            const size_t np = probe_padded(n);
            if (int rc = res_xo_.alloc(np)) return rc;
            if (int rc = res_uo_.alloc(np)) return rc;
            HIPCHK(hipMemsetD32Async((hipDeviceptr_t)res_xo_.p, (int)PROBE_NAN32, np * 2, st));
            HIPCHK(hipMemsetD32Async((hipDeviceptr_t)res_uo_.p, (int)PROBE_NAN32, np * 2, st));
        }
        HIPCHK(hipMalloc(&res_pr_script_, sizeof(ResProbePass) * CGO_RESIDENT_PROBE_MAX_PASSES));
        HIPCHK(hipMalloc(&res_pr_out_, sizeof(ResProbeOut) * CGO_RESIDENT_PROBE_MAX_PASSES));
        HIPCHK(hipMalloc((void **)&res_pr_rows_, sizeof(double) * rows_n));
        HIPCHK(hipStreamSynchronize(st));
        res_xin_ = nullptr; res_uin_ = nullptr;
        res_pr_ready_ = true;
    }
    // the script, padded as res_iterate / ResEval pad it: the spare points repeat the last real step
    ResProbePass script[CGO_RESIDENT_PROBE_MAX_PASSES] = {};
    for (int q = 0; q < p.npass; ++q) {
        const cgo_resident_pass &c = p.pass[q];
        script[q].kind = c.kind; script[q].k = c.k; script[q].a_acc = c.a_acc; script[q].beta = c.beta;
        double lastp = 0.0;
        for (int j = 0; j < RES_MAXP; ++j) { if (j < c.k) lastp = c.a[j]; script[q].a[j] = lastp; }
    }
    double *xo, *uo;
    res_out_buffers(xo, uo);
    HIPCHK(hipMemcpyAsync(res_pr_script_, script, sizeof script, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)res_pr_rows_, (int)PROBE_NAN32, rows_n * 2, st));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)res_pr_out_, (int)PROBE_NAN32, sizeof(ResProbeOut) * CGO_RESIDENT_PROBE_MAX_PASSES / 4, st));
    HIPCHK(hipMemcpyAsync(xc_, x, nb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(uc_, u, nb, hipMemcpyHostToDevice, st));
    if (oop) {
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)xo, (int)PROBE_NAN32, n * 2, st));
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)uo, (int)PROBE_NAN32, n * 2, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    ResParams P{};
    res_fill_params(P, xo, uo);
    P.cfg.ls = ls; P.cfg.eps = cfg.eps; P.cfg.npts = res_npts_;
    P.budget = 0;
    P.log = nullptr; P.log_cap = 0;
    P.timing = 0;
    P.pr_script = (const ResProbePass *)res_pr_script_; P.pr_n = p.npass; P.pr_rows = res_pr_rows_; P.pr_out = (ResProbeOut *)res_pr_out_;
    const void *fn = res_kernel_for<true>(obj_->kind, res_npts_);
    hipFunction_t mf = nullptr;
    if (!fn && obj_->kind == CGO_OBJ_USER && obj_->rtc && obj_->rtc->resident(res_npts_)) {   // compiled on the first probe, not with the objective
        std::string log;
        if (int rc = rtc_compile_program(*obj_->rtc, RTC_RESIDENT_PROBE, log)) { set_error("probe: " + log); return rc; }
        mf = obj_->rtc->resident_probe(res_npts_);
    }
    if (!fn && !mf) { set_error("probe: no PROBE instantiation of this solver's resident kernel"); return CGO_EINVAL; }
    // the plan was made for the product instantiation: this one has the same static LDS and no more registers, checked here
    int per_cu = 0;
    if (fn) {
        if (res_lds_ > 48 * 1024) HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)res_lds_));
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, BLOCK, res_lds_));
    } else {
        HIPCHK(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, mf, BLOCK, res_lds_));
    }
    const int cus = std::min(ctx_->num_cu > 0 ? ctx_->num_cu : 256, RES_GSIZE * RES_GROUPS);
    if (per_cu < 1 || res_grid_ > cus * per_cu) { set_error("probe: the PROBE instantiation does not fit the engine's plan"); return CGO_ESTATE; }
    p.grid = res_grid_; p.points = res_npts_; p.chunk = res_chunk_; p.round0 = (int64_t)res_round_;
    if (chain()) snprintf(p.symbol, sizeof p.symbol, "k_resident_chain<%d, true>", res_npts_);
    else snprintf(p.symbol, sizeof p.symbol, "k_resident<%s, %d, true>", obj_tname(), res_npts_);
    void *args[] = {&P};
    if (fn) HIPCHK(hipLaunchKernel(fn, dim3(res_grid_), dim3(BLOCK), args, res_lds_, st));
    else HIPCHK(hipModuleLaunchKernel(mf, res_grid_, 1, 1, BLOCK, 1, 1, (unsigned)res_lds_, st, args, nullptr));
    total_launches_++;
    if (int rc = wait_word(ctx_, res_done_, res_seq_)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    const ResState s = *res_state_;
    if (s.reason == RES_ERROR) {   // as resident_run: buffers and counters back to their start; here the caller is told, nothing is retried
        unsigned int e[2] = {0, 0};
        HIPCHK(hipMemcpy(e, res_err_, sizeof e, hipMemcpyDeviceToHost));
        p.err_word = e[0];
        if (int rc = res_error_reset()) return rc;
        set_error("probe: a workgroup of the resident launch gave up waiting for a row (error word " + std::to_string(e[0]) + ", " +
                  std::to_string(e[1]) + " of " + std::to_string(res_grid_ - 1) + " workgroups reported in)");
        return CGO_ESTATE;
    }
    res_round_ += (unsigned long long)s.passes;
    res_slices_++;
    if (oop && s.done > 0) res_swap_in(xo, uo);
    p.wrote_back = s.done > 0 ? 1 : 0;
    if (s.passes != p.npass) { set_error("probe: the launch ran " + std::to_string((long long)s.passes) + " of " + std::to_string(p.npass) + " passes"); return CGO_ESTATE; }
    HIPCHK(hipMemcpyAsync(rows, res_pr_rows_, sizeof(double) * (size_t)p.npass * res_grid_ * RES_WMAX, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(p.out, res_pr_out_, sizeof(ResProbeOut) * p.npass, hipMemcpyDeviceToHost, st));
    if (x_out) HIPCHK(hipMemcpyAsync(x_out, xc_, nb, hipMemcpyDeviceToHost, st));
    if (u_out) HIPCHK(hipMemcpyAsync(u_out, uc_, nb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (int rc = probe_slack_intact()) return rc;
    if (oop) {
        const DevBuf *bs[2] = {&res_xo_, &res_uo_};
        std::vector<unsigned> h;
        for (int b = 0; b < 2; ++b) {
            const size_t words = (bs[b]->n - n) * 2;
            h.assign(words, 0u);
            HIPCHK(hipMemcpy(h.data(), bs[b]->p + n, words * 4, hipMemcpyDeviceToHost));
            for (size_t w = 0; w < words; ++w)
                if (h[w] != PROBE_NAN32) {
                    set_error(std::string("probe: the launch wrote past the ") + std::to_string(n) + " elements of the out-of-place " + (b ? "u" : "x") +
                              " (element " + std::to_string(n + w / 2) + ")");
                    return CGO_ESTATE;
                }
        }
    }
    return CGO_OK;
}

}  // namespace cgo

#ifdef CGO_STAMPS
// diagnostic build: the per-workgroup stamps of the last k_cg launch (cgo_kernels_cg.hip.hpp); the caller has synchronised
extern "C" int cgo_debug_stamps(unsigned long long *out, int words) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(cgo::dev::cgo_stamps), (size_t)words * 8, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
