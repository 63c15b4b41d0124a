// cgo_hip_backend.hpp — the product's only VecBackend: device-resident solver
// state in HBM + the fused gfx950 launches of cgo_kernels.hip.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "cgo_engine.hpp"
#include "cgo_launch_kinds.hpp"
#include "cgo_rtc.hpp"

namespace cgo {

// Where a batch's rows (and ring) live during a launch, and which solver runs on them: the kernel family of its launches.  The
// numbers are the C ABI's cgo_batch_probe_args.tier (include/cgo.h); one row each in batch_tier_of() (cgo_backend_internal.hpp).
enum class BatchTier : int { LDS = 0, ROWS = 1, LBFGS = 2, LBFGS_LDS = 3 };
constexpr int BATCH_TIERS = 4;
struct BatchTierRow;

namespace dev { struct CtlArgs; struct Tail; struct LoopParams; struct ResParams; struct BatchParams; struct BatchLbfgsParams; }

void set_error(const std::string &msg);
const char *get_error();

// RAII device allocation
struct DevBuf {
    double *p = nullptr;
    size_t n = 0;
    DevBuf() {}
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int alloc(size_t count);
    void release();
};

struct HipCtx {
    int device = -1;
    hipStream_t stream = nullptr;
    std::unique_ptr<Comm> comm;  // null = single rank
    // reduction scratch shared by every launch on this ctx (one solve at a time)
    double *partials = nullptr;      // [MAX_GRID][NR]
    double *partials2 = nullptr;     // [MAX_GRID/64][NR]  second-stage rows
    double *out_dev = nullptr;       // [NS] local sums
    unsigned int *tickets = nullptr; // [64 + 1] arrival counters of the fused reduction tail (zero between launches) + 1 error counter
    double *partials_f = nullptr;    // [MAX_GRID][NR7] rows of fused launches: every slot holds TAIL_EMPTY between launches
    double *partials2_f = nullptr;   // [64][NR7] their group rows, likewise
    bool pub_checked = false;        // the last publisher was a fused launch: its host block validates itself (tail_check_term)
    bool tail_strict = false;        // CGO_TAIL_STRICT=1: formal system-scope fence for the host block (finish_tail)
    bool fused_tail = true;          // k_cg / k_chain launches finish their own sums (CGO_FUSED_TAIL=0: finalize launches)
    double *gather_dev = nullptr;    // [world][NS]
    double *host_pinned = nullptr;   // [max(world,1)][NS]
    unsigned long long *host_seq = nullptr;  // pinned; k_finalize publishes the launch sequence number here
    unsigned long long seq = 0;      // sequence number of the last launch that produced sums
    bool host_publish = true;        // poll pinned memory instead of D2H copy + stream sync
    // exchange diagnostics (cgo_ctx_exchange_stats)
    long long xch_count = 0;         // launches whose sums crossed ranks
    double xch_peer_wait_ns = 0;     // mailbox: own block visible → last peer's block visible
    hipEvent_t xev0 = nullptr, xev1 = nullptr;  // device-side duration of all-gather + publish, every 4th exchange
    bool xev_pending = false;
    double xch_dev_ms = 0; long long xch_dev_n = 0;
    void xch_collect();              // fold a pending event pair into xch_dev_ms
    bool force_gather = false;       // debug (CGO_FORCE_GATHER=1): run the multi-rank exchange path even with one rank
    unsigned long long solver_epoch = 0;   // solvers created on this context so far (the same on every rank: replicated control flow)
    bool dev_exchange() const { return comm && world() > 1 && comm->dev_mailbox(0) != nullptr; }   // device mailboxes connected
    bool single() const { return world() == 1 && !force_gather; }
    bool shm() const { return comm && comm->shm_slot_host(0, 0) != nullptr; }
    // where the finalize kernel of launch `seq` publishes (nullptr = no host publish for this launch)
    void pub_target(double **out, unsigned long long **seqw);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // the (x, u) buffers the last solver's placement search kept, parked here when that solver goes so that the next solver
    // of the same size (a rerun chain, the next centering step) takes them over instead of searching again
    DevBuf placed_x, placed_u;
    int64_t placed_n = 0;
    double placed_first_us = 0.0, placed_best_us = 0.0;
    int placed_candidates = 0;
    std::string arch;
    int num_cu = 0;
    ~HipCtx();
    int init(int device);
    int ensure_gather();
    int rank() const { return comm ? comm->rank : 0; }
    int world() const { return comm ? comm->world : 1; }
};

struct HipObjective {
    HipCtx *ctx = nullptr;
    int kind = 0;
    int64_t n_global = 0, offset = 0, n_local = 0;
    DevBuf p[CGO_MAX_PARAM_SLOTS];   // parameter vectors, slots 0 … nparams() − 1
    bool p_set[CGO_MAX_PARAM_SLOTS] = {};
    double s0 = 0.0;
    std::shared_ptr<RtcModule> rtc;  // CGO_OBJ_USER: the run-time compiled kernels
    int user_nparams = 0;     // CGO_OBJ_USER: parameter slots its kernels read (0 … CGO_MAX_PARAM_SLOTS)
    bool user_cheap = false;  // cgo_objective_set_cost_class: seven trial steps per launch
    int users = 0;            // live solvers on this objective (the placement search moves the parameter vector only for a sole user)
    // CGO_OBJ_HOST: the reference's closure contract f = fdf!(g, x) on host vectors (cgo_objective_create_callback)
    cgo_fdf_fn host_fn = nullptr;
    void *host_user = nullptr;
    double *host_x = nullptr, *host_g = nullptr;   // pinned staging, n_local doubles each
    bool host_closure() const { return kind == CGO_OBJ_HOST; }
    ~HipObjective();
    int nparams() const { return kind == CGO_OBJ_QUAD_DIAG ? 1 : (kind == CGO_OBJ_USER ? user_nparams : 0); }
    bool uses_param() const { return nparams() > 0; }
    int unset_slot() const { for (int j = 0; j < nparams(); ++j) if (!p_set[j]) return j; return -1; }   // −1: every slot is set
    template <class A> void param_args(A &P) const { P.p0 = p[0].p; P.p1 = p[1].p; P.p2 = p[2].p; P.p3 = p[3].p; }   // KParams, RParams, SpecParams, ResParams
    bool two_phase() const { return kind == CGO_OBJ_LSE; }
};

struct RPlan { bool big; int grid, npts; double bytes; };   // a k_cg / k_chain launch: streaming path, grid, points as launched, algorithmic bytes

struct QnState;   // cgo_qn.hpp
class HipBackend : public VecBackend {
  public:
    HipBackend(HipCtx *ctx, HipObjective *obj);
    ~HipBackend() override;
    int alloc();
    int place();   // placement search for HBM-bound sizes (after the launch policy is set)
    int64_t n_local() const override { return obj_->n_local; }
    int set_x0_host(const double *x0) override;
    int set_x0_device(const double *x0_dev);
    int download_device(double *x_dev, double *g_dev);
    int tail_errors();
    int set_x0_fill(int kind, uint64_t seed, double lo, double hi) override;
    int init_eval(Scal &out) override;
    // 3-point launches pay a 24-slot reduction: worth it once a saved launch is worth more than
    // that (measured: n = 1e6 loses 20 %, n = 1e7 gains 70 %)
    // Trial steps per launch (policy set by the C API from the objective's cost class; measured in
    // scripts/ab_points.sh, ab_small.sh, ab_small2.sh).  The on-device controller understands 3-point rows.
    int max_points() const override {
        if (!rmode_ || obj_->n_local < multi_min_n_) return 1;
        return policy_points();
    }
    int policy_points() const {
        if (!rmode_ || obj_->n_local < multi_min_n_) return 1;
        if (obj_->n_local >= band3_lo_ && obj_->n_local < band3_hi_) return 3;
        if (obj_->n_local >= multi7_min_n_) return 7;
        return obj_->n_local >= multi5_min_n_ ? 5 : 3;
    }
    int trial(const double *a, int k, Scal *out) override;
    int accept_dir_trial(double a_acc, double beta, const double *a, int k, Scal *out) override;
    int ctl_depth() const override;
    int accept_dir_trial_ctl(const CtlConfig &cc, const CtlState &s0, int64_t rounds, Scal *out) override;
    void set_ctl_depth(int d) { ctl_depth_ = d < 0 ? 0 : (d > 32 ? 32 : d); }
    void set_policy(const cgo_solver_policy &p);          // the resolved policy (before alloc())
    const cgo_solver_policy &policy() const { return pol_; }
    double big_bytes(bool read_only = false) const;       // pure-HBM streaming threshold of this solver
    int prepare_controller();   // its device / pinned blocks and the first launch of its kernels, outside the first armed iteration
    int64_t ctl_served() const { return pipe_served_; }
    int64_t ctl_graph_rounds() const { return graph_rounds_; }
    void placement_info(double *first_us, double *best_us, int *candidates) const { *first_us = place_first_us_; *best_us = place_best_us_; *candidates = place_candidates_; }
    double placement_cap_bytes() const { return place_cap_bytes_; }
    void set_ctl_graph(bool on) { graph_on_ = on; }
    // resident solver (cgo_kernels_resident.hip.hpp): whole iterations in one launch while the shard fits the LDS of the chip
    bool resident_ready(const cgo_cg_config &cfg, const cgo_ls_config &ls) const override;
    int resident_run(const ResConfig &c, ResState &s, int64_t budget, std::vector<ResRecord> &recs, std::vector<ResLog> &log) override;
    void set_resident(bool on) { res_on_ = on; }
    bool resident_enabled() const { return res_on_; }
    int ctl_depth_setting() const { return ctl_depth_; }
    int64_t resident_iters() const { return res_iters_; }
    int64_t resident_slices() const { return res_slices_; }
    int64_t resident_gave_up() const { return res_gave_up_; }
    // Batched solves (cgo_backend_batch.hip; k_batch, cgo_kernels_batch.hip.hpp).  The backend's objective spans the
    // CONCATENATED problems — n_local = batch · ld, ld = n + (n & 1) — so that x, u and every parameter slot are the
    // [batch][ld] rows and the ordinary gradient launch (download) serves every problem at once.
    // largest n one workgroup's LDS holds of x, u and the slots (res_plan's arithmetic); 0: no kernel.  CGO_OBJ_USER: `rtc` with its batch program
    static int64_t batch_max_n(HipCtx *ctx, int obj_kind, const RtcModule *rtc = nullptr);
    // params[j], j < nparams(): the [batch·n] rows of slot j
    // … in its two halves, for a batch that stays on the device between solves (cgo_batch_open / cgo_batch_solve): the slot rows
    // once; then per solve x0, the states, and optionally a scalar per problem (scalars, [batch]) and which problems run
    // (active, [batch] bytes; null: all — an inactive problem's workgroup returns at once)
    // device_rows: the second tier (k_batch_rows, cgo_kernels_batch_rows.hip.hpp) — the rows are streamed from where they are in every
    // pass: no dynamic LDS, n up to batch_rows_max_n() and what the device's memory holds (batch_rows_bytes)
    int batch_alloc(int64_t batch, int64_t n, const double *const *params, bool device_rows = false);
    static int64_t batch_rows_max_n();         // the limit of the tier's pass index on n
    static int batch_rows_unroll();            // pairs per lane and trip of its streaming loop
    static int batch_rows_block();             // lanes of its workgroup
    static double batch_rows_bytes(int64_t batch, int64_t n, int nparams);   // device bytes a batch of that shape asks for
    bool batch_device_rows() const { return bat_tier_ != BatchTier::LDS; }   // (the L-BFGS tiers' rows are device rows too)
    int batch_reset(const double *x0, const double *scalars, const unsigned char *active, int64_t max_iters, bool trace);
    int batch_launch(const ResConfig &c, int64_t budget, std::vector<ResState> &st, std::vector<double> &f_x0) override;
    int batch_records(int64_t b, int64_t count, std::vector<ResRecord> &out);     // the trace records of problem b's first `count` iterations (b < 0: every row)
    int64_t batch_rec_stride() const { return bat_rec_stride_; }
    int batch_export_row(int64_t b, HipBackend &dst, bool with_u);                // row b of x (u), and of every parameter slot → dst
    int batch_export_slots(int64_t b, HipBackend &dst);                           // row b of every parameter slot alone → dst's objective
    // dense rows; each may be nullptr; rows of inactive problems are not written.  With a scalar per problem the gradient is
    // k_batch_grad's (a workgroup per row), otherwise the ordinary gradient launch over the concatenated rows
    int batch_results(double *x /*[batch·n]*/, double *g /*[batch·n]*/, const unsigned char *active = nullptr);
    // Batched solves with β = LBFGS(m) (cgo_backend_batch_lbfgs.hip; k_batch_lbfgs, cgo_kernels_batch_lbfgs.hip.hpp): a batch
    // allocated with device_rows gets a ring of 2(m+1) rows and a QnState per problem beside its rows; batch_launch then runs
    // k_batch_lbfgs.  batch_lbfgs_reset after every batch_reset: every problem's ring empty.  A run-time compiled objective runs
    // the kernel of its module's batched L-BFGS program (RTC_BATCH_LBFGS), which the caller compiles first.
    int batch_lbfgs_alloc(int m, bool lds = false);
    int batch_lbfgs_reset(int m = 0);          // m: this solve's ring depth, 1 … the allocated one (0: the allocated one) — the ring keeps its stride
    int batch_lbfgs_m() const { return bat_m_; }   // the ring depth allocated (0: not a batched L-BFGS batch)
    static int64_t batch_lbfgs_max_n();        // the limit of the pass index on n
    static int batch_lbfgs_unroll();           // pairs per lane and trip of the two ring passes
    static int batch_lbfgs_unroll_for(int nparams);   // … for an objective of that many parameter slots (run-time compiled ones)
    static int batch_lbfgs_block();            // lanes of the workgroup
    static double batch_lbfgs_bytes(int64_t batch, int64_t n, int nparams, int m);   // device bytes a batch of that shape asks for
    // … with the problem's rows and ring in LDS during a launch (cgo_backend_batch_lbfgs_lds.hip; k_batch_lbfgs_lds,
    // cgo_kernels_batch_lbfgs_lds.hip.hpp): batch_lbfgs_alloc(m, true) — the same allocation, the launches take
    // 8 · ld · batch_lbfgs_lds_rows(K, m) bytes of dynamic LDS.  A run-time compiled objective runs the kernel of its module's
    // program of this tier (RTC_BATCH_LBFGS_LDS), which the caller compiles first.
    static int batch_lbfgs_lds_rows(int nparams, int m);        // 2 + K + 2(m+1); 0: K or m out of range
    static int batch_lbfgs_lds_unroll_for(int nparams);         // pairs per lane and trip of the two ring passes over LDS
    static int64_t batch_lbfgs_lds_ld_of(int64_t max_lds, int64_t static_lds, int rows);   // the size arithmetic alone
    // largest ld (even) one workgroup's LDS holds of a problem's rows and ring; 0: none.  CGO_OBJ_USER: `rtc` with that program
    static int64_t batch_lbfgs_lds_max_ld(HipCtx *ctx, int obj_kind, int m, const RtcModule *rtc = nullptr);
    bool batch_lbfgs_in_lds() const { return bat_tier_ == BatchTier::LBFGS_LDS; }
    // Test entry point (cgo_batch_probe, cgo_backend_batch_probe.hip): a script of passes in ONE launch of the PROBE twin of this
    // batch's kernel, on host vectors; the batch is one batch_alloc (and batch_lbfgs_alloc) made, the launch arguments are
    // batch_fill_params' / batch_lbfgs_fill_params'.  Every buffer of the batch gets NaN slack: a probed batch is for probing only.
    int batch_probe(cgo_batch_probe_args &p);
    int64_t push_count(int kind) const { return push_counts_[kind]; }   // 0 speculated, 1 fused (g⁺ formed in the push), 2 plain
    bool sys_supported() const override { return rmode_; }
    int sys_begin() override;
    int sys_project(double a, double m, Scal &out) override;
    int sys_commit() override;
    int dir_trial(double beta, const double *a, int k, Scal *out) override;
    int accept_dir(double a_acc, double beta, Scal &out) override;
    int accept_only(double a_acc) override;
    int reset_dir(Scal &out) override;
    int upg_sumsq(double &out) override;
    int lbfgs_alloc(int slots) override;
    int lbfgs_gram_max_pairs() const override { return gram_on_ ? 12 : 0; }
    int lbfgs_push_gram(double a_x, double a_s, int slot, const int *prev, int count, GramOut &out) override;
    bool lbfgs_push_materializes(double a_x) override;
    bool lbfgs_push_spec(double a_x, double a_s, int slot, const int *prev, int count, GramOut &out) override;
    int lbfgs_push_commit(bool direction_follows) override;
    int lbfgs_direction_gram(const int *slots, const double *cy, const double *cs, int count, double cg,
                             Scal &out) override;
    bool lbfgs_direction_gram_can_fuse_trial() const override;
    int lbfgs_direction_gram_trial(const int *slots, const double *cy, const double *cs, int count, double cg, double a_trial,
                                   Scal &dir, Scal &trial) override;
    int lbfgs_push(double a_x, double a_s, int slot, double &sy, double &yy) override;
    int lbfgs_direction(const int *slots, const double *rho, int count, double gamma,
                        Scal &out) override;
    bool two_phase() const override { return obj_->two_phase(); }
    int materialize(Scal &out) override;
    void discard_pending() override { push_pending_ = false; push_lite_pending_ = false; lite_deferred_ = false; spec_valid_ = false; spec_unmat_ = false; }
    int download(double *x, double *g) override;
    int scaled_norm_parts(int which, double a_trial, double &maxabs, double &scaled_ss, bool &has_nan) override;
    void profile_enable(bool on) override;
    void profile_reset() override;
    void profile_get(int kind, int64_t *launches, double *ms, double *bytes) override;
    int64_t launches() const override { return total_launches_; }
    void set_need_beta(bool b) { need_beta_ = b; }
    // gradient-free multi-point CG kernels (cgo_kernels_cg.hip.hpp): element-wise objective + CG β
    void set_rmode(bool on) { rmode_ = on; }
    void set_multi_min_n(int64_t n) { multi_min_n_ = n; }
    void set_multi5_min_n(int64_t n) { multi5_min_n_ = n; }
    void set_multi7_min_n(int64_t n) { multi7_min_n_ = n; }
    void set_three_point_band(int64_t lo, int64_t hi) { band3_lo_ = lo; band3_hi_ = hi; }
    bool rmode() const { return rmode_; }
    // Lazy direction: every second accept + dir + trial launch of an eligible solver leaves u unstored.
    void set_lazy_direction(bool on) { lazy_on_ = on; }
    bool lazy_direction() const { return lazy_on_; }
    int set_lazy_direction_now(bool on) { if (!on) { if (int rc = materialize_lag()) return rc; } lazy_on_ = on; return 0; }   // (mid-solve: the lag ends first)
    void set_probe_beta_prev(double b) { probe_beta_prev_ = b; }
    // Replay: of every d accepting launches of an eligible solver d − 1 store nothing and the d-th stores x and u.
    // d = 1: the lazy direction's alternation.
    // d ≤ 16 where launches N and S run as path launches, which take the steps beyond the seventh in a second kernel argument (deep
    // replay); every other solver runs a larger request as depth 8.
    void set_replay_depth(int d) { replay_depth_ = d < 1 ? 1 : (d > 16 ? 16 : d); }
    int replay_depth() const { return replay_depth_; }
    int set_replay_depth_now(int d);   // (mid-solve: outstanding steps are stored first)
    void set_probe_replay(int nrep, const double *a, const double *beta);
    void set_probe_deep_trial(bool on) { probe_deep_t_ = on; }   // the next probe_launch of launch T runs as k_cg_trial_deep whatever its list
    // launches N, S, T (a trial met with steps outstanding) and M (a materialise pass) so far; the T and M among them that met more
    // than seven outstanding steps; the longest list a launch replayed
    struct ReplayStats { int64_t n = 0, s = 0, t = 0, m = 0, t_deep = 0, m_deep = 0; int max_list = 0; };
    const ReplayStats &replay_stats() const { return rstats_; }
    // Lean sums: launches N and S without the trial sums the solver's β flavour never reads (beta_unread_sums),
    // where cgo_instances.def has rows for that mask.  The stored state is the same either way: no pass is needed to switch.
    void set_beta_unread(int bits) { lean_mask_ = bits; if (lean_bits_) lean_bits_ = bits; }
    void set_lean_sums(bool on) { lean_bits_ = on ? lean_mask_ : 0; }
    bool lean_sums() const { return lean_bits_ != 0; }
    // Predicted path: where launches N and S would run their lean rows, they run as path launches (k_cg_path) —
    // the first k trial points of the 7-point row and the curvature sums.  Objectives with a constant Hessian only (ObjCurv); the
    // stored state is the same either way.
    void set_path_prediction(bool on) { path_on_ = on; }
    bool path_prediction() const { return path_on_; }
    bool path_rows() const override;
    int accept_dir_trial_path(double a_acc, double beta, const double *a, int k, Scal *out) override;
    int64_t path_launches(int nact) const { return (nact >= 1 && nact <= 7) ? path_count_[nact] : 0; }
    void set_probe_path(int nact) { probe_nact_ = nact; }   // the next probe_launch of a lean row runs as that path row (0: the lean row)
    std::string kernel_symbol(int kernel_kind) const;
    // Test entry point (cgo_solver_probe_launch): the vectors → this solver's device state, ONE launch of kind `kernel_kind`
    // with mode bits `variant` through the engine's own launch path, the whole reduced row and the vectors back.  The first
    // probe re-allocates the solver's buffers with NaN slack behind n_local: a probed solver is for probing only.
    int probe_launch(int kernel_kind, int variant, double a_acc, double beta, const double *a, int k, const double *x,
                     const double *u, const double *aux, double *sums, int sums_cap, int *sums_len, double *x_out,
                     double *u_out, double *g_out, std::string &symbol);
    bool probed() const { return probe_; }
    int probe_launch_stored(int kernel_kind, int variant, double a_acc, double beta, const double *a, int k, const double *x,
                            const double *u, const double *aux, double *sums, int sums_cap, int *sums_len, double *x_out,
                            double *u_out, double *g_out, std::string &symbol);   // the stored-gradient family's half of it
    // Test entry point (cgo_solver_probe_lbfgs): ONE L-BFGS pass of this solver (β = LBFGS(m)) on host vectors and rings,
    // through the entry point the engine uses for it; the rings get NaN slack as well.
    int probe_lbfgs(int m, cgo_lbfgs_probe &p, const double *x, const double *u, const double *g, const double *gt, const double *S,
                    const double *Y, double *x_out, double *xo_out, double *u_out, double *g_out, double *gt_out, double *S_out,
                    double *Y_out);

    // Test entry point (cgo_solver_probe_resident): a script of resident passes in ONE launch of the PROBE instantiation of this
    // solver's resident kernel, under the engine's own plan, exchange buffers, write-back rule and round bookkeeping.
    int probe_resident(const cgo_cg_config &cfg, const cgo_ls_config &ls, cgo_resident_probe &p, const double *x, const double *u,
                       double *rows, int64_t rows_cap, double *x_out, double *u_out);

    // Test entry point (cgo_solver_probe_armed): a batch of controller-armed rounds on host vectors through k_ctl_init,
    // pipe_enqueue and pipe_wait — every record whole, the device block and the vectors back.
    int probe_armed(const cgo_cg_config &cfg, const cgo_ls_config &ls, cgo_armed_probe &p, const double *x, const double *u,
                    double *x_out, double *u_out);

    // raw single-launch helpers used by the kernel-level C entry points
    static int run_dir(HipCtx *ctx, double *u_host, const double *g_host, double beta, int64_t n,
                       double *out2);
    static int run_beta_partials(HipCtx *ctx, const double *gn, const double *g, const double *u,
                                 int64_t n, double *out9);
    static int run_trial(HipObjective *obj, const double *x, const double *u, double a,
                         double *gn_out, double *out2);
    static int run_eval(HipObjective *obj, const double *x, double *g_out, double *f);
    static int bench_kernel(HipCtx *ctx, HipObjective *obj, int kernel_kind, int64_t n, int reps,
                            double *ms, double *bytes);
    static int bench_stream_mix(HipCtx *ctx, int64_t n, int reps, double *median_us, double *best_us);

  private:
    int launch(int kk, int mode, double a_acc, double beta, double a_trial, bool fetch,
               double *sums /*[NS] global*/);
    int launch_k(int kk, double a_acc, double beta, double a_trial, bool fetch, double *sums) { return launch(kk, fused_mode(kk), a_acc, beta, a_trial, fetch, sums); }
    HipCtx *ctx_;
    HipObjective *obj_;
    DevBuf x_, u_, ga_, gb_;
    // Ping-pong iterate/direction buffers of the gradient-free family's pure-HBM (BIG) launches: such a launch
    // writes the updated x / u into the OTHER buffer of the pair and the pointers swap — reading and writing the same
    // arrays in one stream costs ≈ 10 % of HBM bandwidth.  Allocated on first use, only if they fit.
    DevBuf x2_, u2_;
    double *uc_ = nullptr;                     // current direction (u_.p or u2_.p)
    double *xalt_ = nullptr, *ualt_ = nullptr; // the other buffer of each pair
    int pingpong_ = -1;                        // −1: not decided yet, 0: in place, 1: ping-pong
    bool sys_on_ = false;                      // solvesystem owns a second iterate buffer of its own: in place
    // chained Rosenbrock (stencil objective, cgo_kernels_chain.hip.hpp): x / u always advance out of place, and the
    // two elements beyond each shard boundary travel in the scalar block (slots 10–17 of every rank's row)
    bool chain() const { return obj_->kind == CGO_OBJ_ROSENBROCK_CHAINED; }
    // probe_launch: the buffers carry NaN slack, the last launch's reduced row is kept, and so is what the last k_cg / k_chain
    // launch instantiated (mode, points, pure-HBM)
    bool probe_ = false;
    double probe_row_[64] = {};
    int probe_len_ = 0;
    int last_mode_ = -1, last_npts_ = 0;
    bool last_big_ = false;
    int probe_prepare();
    int probe_slack_intact();
    std::string r_symbol(int mode, int npts, bool big, int nact = 0) const;
    std::string probe_syms_;   // probe_lbfgs: every instantiation its pass launched (probe_note)
    void probe_note(const double *row, int len, const char *fmt, ...);
    int probe_ring_slack_intact();
    // probe_launch on a stored-gradient solver: launch, host_trial and scaled_norm_parts note what they launch and append
    // every row they fetch (several launches per probe: the host closure's init, scaled_norm's two passes)
    bool probe_stored_ = false;
    void probe_append(const double *row, int len);
    const char *obj_tname() const;
    int launch_loop(const dev::LoopParams &P, int kk, double nvec, bool big, int grid);
    double halo_xl_[2] = {0, 0}, halo_ul_[2] = {0, 0}, halo_xr_[2] = {0, 0}, halo_ur_[2] = {0, 0};
    int launch_chain_kernel(int mode, double a_acc, double beta, const double *a, int k, int npts, bool big, int grid, const dev::Tail &tail);
    bool tail_fused(int grid) const;
    bool pipe_fused(int grid) const;
    dev::Tail make_tail(bool on);
    bool pingpong_ready();
    // placement search for pure-HBM problem sizes: which physical buffers x, u (and D) live in
    int tune_placement();
    double place_first_us_ = 0.0, place_best_us_ = 0.0;   // the mix on the buffers as allocated / on the chosen ones
    int place_candidates_ = 0;
    double place_cap_bytes_ = 0.0;          // transient memory the placement search may use (policy.placement_max_bytes or a quarter of the free memory)
    bool placed_ = false;
    int ensure_ga();   // gradient buffer A on first use
    int ensure_gb();   // gradient buffer B / solvesystem's second iterate on first use
    double *xc_ = nullptr, *xn_ = nullptr;  // current iterate / solvesystem's x_next (swapped by sys_commit)
    double *g_ = nullptr, *gt_ = nullptr;  // rotate between ga_/gb_ (kills optim.jl:139's copy)
    bool need_beta_ = true;
    bool rmode_ = false;
    int64_t multi_min_n_ = 3000000;
    int64_t multi5_min_n_ = INT64_MAX;
    int64_t multi7_min_n_ = INT64_MAX;
    int64_t band3_lo_ = 0, band3_hi_ = 0;  // sizes inside [lo, hi) stay at three points
    int launch_r(int kk, int mode, double a_acc, double beta, const double *a, int k, bool fetch, double *sums);
    int launch_rk(int kk, double a_acc, double beta, const double *a, int k, bool fetch, double *sums) { return launch_r(kk, r_mode_of(kk), a_acc, beta, a, k, fetch, sums); }
    RPlan r_plan(int mode, int npts) const;   // asked by the launch itself, its byte accounting and kernel_symbol
    bool adt_is_big() const;                  // is this solver's accept + direction + trial launch a pure-HBM one?
    // the k_fused mode this solver's entry point of kind kk launches (−1: none): a trial whose β sums nobody reads takes the row without them
    int fused_mode(int kk) const { const MKind *mk = m_kind(kk); return !mk ? -1 : ((kk == KK_TRIAL && !need_beta_) ? mk->alt : mk->mode); }
    std::string lbfgs_symbol(int kk) const;   // kernel_symbol's half for the L-BFGS and log-sum-exp launches (cgo_backend_lbfgs.hip)
    // lazy direction: memory holds (x_{k+1}, u_k) while u_lag_ is set, and beta_lag_ = β_k rebuilds u_{k+1} from them
    bool lazy_on_ = false, u_lag_ = false;
    double beta_lag_ = 0.0, probe_beta_prev_ = 0.0;
    bool lazy_eligible() const;
    int materialize_u();   // store the rebuilt direction for any reader but the lag launches; clears u_lag_
    // replay: memory holds (x_k, u_k); rep_a_[j], rep_b_[j] = (a*, β) of the rep_n_ steps accepted since, oldest first
    int replay_depth_ = 1, rep_n_ = 0, probe_rep_n_ = 0;
    double rep_a_[15] = {}, rep_b_[15] = {}, probe_rep_a_[15] = {}, probe_rep_b_[15] = {};
    bool probe_deep_t_ = false, deep_t_ = false;   // deep T whatever the list: asked for by a probe; in force for the probe's launch
    bool deep_trial(int mode) const;   // this launch runs as k_cg_trial_deep: launch T with more than seven steps outstanding (or the probe's request)
    ReplayStats rstats_;
    int materialize_lag();   // … and the replayed pair (x, u) likewise; clears u_lag_ and rep_n_
    int lean_mask_ = 0, lean_bits_ = 0;   // the flavour's R_NO… bits; those in force (0: full rows)
    int lean_for(int mode) const;         // … for this mode: lean_bits_ where a lean row exists, else 0
    // predicted path: the switch; NACT of the path launch being issued (0: an ordinary launch) and of the last launch; the last
    // path row launches N and S ran as; launches by NACT
    bool path_on_ = false;
    int path_nact_ = 0, last_nact_ = 0, probe_nact_ = 0;
    int path_last_n_ = 0, path_last_s_ = 0;
    int64_t path_count_[8] = {};
    int accept_dir_trial_r(double a_acc, double beta, const double *a, int k, double *s);
    int trial_r(const double *a, int k, double *s);
    int launch_r_kernel(int kk, int mode, double a_acc, double beta, const double *a, int k, int npts,
                        const struct dev::CtlArgs *ctl, RPlan *plan_out);
    // on-device controller (cgo_ctl.hpp): rounds armed on the device ahead of the host
    int ctl_depth_ = 0;  // set by the C API per objective class / CGO_CTL_DEPTH
    unsigned long long epoch_ = 0;          // this solver's number on its context (device-mailbox block numbers carry it)
    void *ctl_dev_ = nullptr;               // CtlDev in HBM
    void *ctl_rec_ = nullptr;               // CtlRecord[PIPE_RING], pinned host
    unsigned long long *ctl_seq_ = nullptr; // [PIPE_RING], pinned host
    unsigned long long pipe_enq_ = 0, pipe_done_ = 0;  // rounds enqueued / consumed (global counters)
    bool pipe_stopped_ = false;
    bool pipe_checked_ = false;             // rounds in flight publish self-validating records (fused rounds, not CGO_TAIL_STRICT)
    bool ctl_fused_ = true;                 // policy.controller_fused = 0: armed rounds keep their reduce + controller launches
    cgo_solver_policy pol_;                 // resolved policy of this solver (set_policy)
    int pipe_npts_ = 1;                     // kernel variant (1, 3, 5, 7 trial points) of the rounds in flight
    int64_t pipe_streak_ = 0;               // accept+dir+trial launches in a row = first trials accepted in a row
    int64_t pipe_served_ = 0;
    std::vector<std::pair<int, unsigned>> pipe_prof_;  // profiling slot (index, generation) of each round
    unsigned prof_gen_ = 0;
    int pipe_alloc();
    int pipe_round_kernels();
    int pipe_finalize_ctl(const double *src, int nrows, int ns);
    int pipe_enqueue_round();
    int pipe_launch_graph(int rounds);
    int pipe_enqueue(int64_t count);
    struct PipeGraph { void *exec; int rounds, npts; double *x, *u; const double *p0; int64_t n; std::string syms; };   // (armed rounds: built-in objectives, one slot)
    std::vector<PipeGraph> graphs_;      // instantiated hipGraphs of 2 / 4 / 8 controller rounds
    bool graph_on_ = false;              // CGO_CTL_GRAPH=1: batches of armed rounds replay from instantiated hipGraphs (measured 3–8 % slower than kernel-by-kernel enqueue)
    bool capturing_ = false;
    unsigned long long pipe_batches_ = 0;
    int64_t graph_rounds_ = 0;
    int pipe_wait(unsigned long long id, CtlRecord &rec);
    int pipe_drain();
    int accept_dir_trial_keep_streak(const CtlState &s0, Scal *out);
    // resident solver state
    bool res_on_ = true;
    int res_grid_ = 0, res_npts_ = 3;
    int64_t res_chunk_ = 0;
    size_t res_lds_ = 0;
    int res_plan();                          // grid, chunk, LDS bytes for this shard; 0 workgroups = does not fit
    int res_alloc();
    // shared by resident_run and probe_resident (cgo_backend_cg.hip)
    void res_out_buffers(double *&xo, double *&uo) const;
    void res_fill_params(dev::ResParams &P, double *xo, double *uo);
    void res_swap_in(double *xo, double *uo);
    int res_error_reset();
    ResState *res_state_ = nullptr;          // pinned
    ResRecord *res_recs_ = nullptr;          // pinned [RES_REC_CAP]
    ResLog *res_log_ = nullptr;              // pinned [RES_LOG_CAP], allocated when a log is first asked for
    ResRecord *res_recs_dev_ = nullptr;      // device twins: the kernel's leader writes here, workgroup 0 copies out at the end
    ResLog *res_log_dev_ = nullptr;
    double *res_xbuf_ = nullptr;             // device
    unsigned int *res_err_ = nullptr;        // device: [0] error flags of the exchange, [1] workgroups that have reported in
    DevBuf res_xo_, res_uo_;                 // where a multi-workgroup slice leaves x, u (swapped in on a good GLOBAL verdict only)
    double *res_xin_ = nullptr, *res_uin_ = nullptr;   // the pair those were swapped against (the next slice's output)
    unsigned long long *res_done_ = nullptr; // pinned
    unsigned long long res_seq_ = 0, res_round_ = 0;
    // probe_resident: script, per-workgroup rows and member-function results on the device; xo / uo with NaN slack
    void *res_pr_script_ = nullptr, *res_pr_out_ = nullptr;
    double *res_pr_rows_ = nullptr;
    bool res_pr_ready_ = false;
    int64_t res_iters_ = 0, res_slices_ = 0, res_gave_up_ = 0;
    // batched solves
    int64_t bat_count_ = 0, bat_n_ = 0, bat_ld_ = 0, bat_rec_stride_ = 0;
    bool bat_trace_ = false;
    size_t bat_lds_ = 0;
    BatchTier bat_tier_ = BatchTier::LDS;    // batch_alloc: LDS or ROWS; batch_lbfgs_alloc turns ROWS into LBFGS or LBFGS_LDS
    ResState *bat_st_ = nullptr;             // device [batch]
    ResRecord *bat_recs_ = nullptr;          // device [batch][bat_rec_stride_]
    double *bat_fx0_ = nullptr;              // device [batch]
    double *bat_s0v_ = nullptr;              // device [batch]: the scalars of the solve under way (bat_s0v_on_)
    bool bat_s0v_on_ = false;
    size_t bat_recs_cap_ = 0;                // records allocated
    void batch_fill_rows(std::vector<double> &rows, const double *src) const;
    int batch_recs_reserve(int64_t stride);
    int batch_grad_rows();
    // ONE launch of a batch's kernel, a workgroup per problem: the ahead-of-time instantiation `fn`, or for a run-time compiled
    // objective its module's `mf`; `missing`: the refusal where a built-in objective has no instantiation
    int batch_launch_kernel(const void *fn, hipFunction_t mf, const char *missing, void **args, size_t lds);
    int batch_launch_tier(void *params);                               // … of this batch's tier on its parameter block
    int batch_lbfgs_launch_tier(const ResConfig &c, int64_t budget);   // … a quasi-Newton tier's: batch_lbfgs_fill_params, then that
    // what a launch reads of the batch — ld, the slot pointers, s0 / s0v, the record stride: batch_launch's and the probe's alike
    void batch_fill_params(dev::BatchParams &B, const ResConfig &c, int64_t budget) const;
    void batch_lbfgs_fill_params(dev::BatchLbfgsParams &L, const ResConfig &c, int64_t budget) const;   // … and the ring, its stride, the states
    int bat_m_ = 0;                          // > 0: a batched L-BFGS solve of that ring depth (batch_lbfgs_alloc)
    double *bat_S_ = nullptr, *bat_Y_ = nullptr;   // device [batch][m+1][ld]
    QnState *bat_qn_ = nullptr;             // device [batch]
    bool prof_on_ = false;
    struct ProfSlot { hipEvent_t e0 = nullptr, e1 = nullptr; int kk = -1; double bytes = 0; };
    std::vector<ProfSlot> ring_;
    int ring_used_ = 0;
    int prof_slot(hipEvent_t *e0, hipEvent_t *e1);
    int prof_begin(int kk);
    int prof_end();
    void prof_commit(int kk, double bytes);
    void prof_flush();
    bool prof_pick(int kk);             // is the launch about to be issued one of the timed ones?
    int prof_every_ = 4;                // below n_local = 3e7: time every 4th launch, count all
    int64_t prof_tick_[KK_COUNT] = {};
    bool prof_cur_ = false;
    int64_t prof_cnt_[KK_COUNT] = {};   // launches (all)
    int64_t prof_n_[KK_COUNT] = {};     // launches timed
    double prof_ms_[KK_COUNT] = {};
    double prof_bytes_[KK_COUNT] = {};
    int64_t total_launches_ = 0;
    // L-BFGS ring in HBM
    int qn_m_ = 0;
    bool gram_on_ = true;   // CGO_LBFGS_TWO_LOOP=1: chained two-loop launches instead of the Gram form
    DevBuf qn_S_, qn_Y_;
    double *qn_alpha_dev_ = nullptr;
    double qn_sgt_ = 0.0;   // Σ s·g⁺ of the last push (global)
    int qn_sgt_slot_ = -1;
    bool push_pending_ = false, fuse_grad_ = true;   // fused push of the log-sum-exp objective: x', g⁺ written, pointers not swapped yet
    double *push_xo_ = nullptr;
    // one ring pass per iteration: the sums the direction pass took at its speculated first trial (lbfgs_direction_spec)
    bool spec_on_ = false, spec_valid_ = false, push_lite_pending_ = false;
    bool spec_fuse_push_ = true, lite_deferred_ = false, spec_unmat_ = false;   // the state update of an accepted speculated trial left to the next direction pass
    int flush_lite();
    double spec_s_[64] = {}, spec_Mr_ = 0.0, spec_Sr_ = 1.0, spec_a_ = 0.0, spec_dphi_ = 0.0;
    int64_t spec_refreshed_ = 0;   // speculated trials whose statistics were taken again with the true maximum
    int spec_count_ = 0, spec_slots_[16] = {};
    double lite_a_ = 0.0, lite_as_ = 0.0, lite_M_ = 0.0, lite_S_ = 1.0;
    int lite_slot_ = 0;
    int64_t push_counts_[3] = {0, 0, 0};
    int lbfgs_direction_spec(const int *slots, const double *cy, const double *cs, int count, double cg, double a_trial, Scal &dir, Scal &trial);
    int lbfgs_push_lite();
    int chain_sums(int grid, int slot, const double **dot_ptr, int *dot_count, double *dot_host);
    // two-phase (LSE) state of the most recent trial
    double lse_a_ = 0.0, lse_M_ = 0.0, lse_S_ = 1.0;
    bool lse_have_ = false;   // (lse_M_, lse_S_) are the statistics of a point on the current line: usable as a fixed reference
    int lse_stats(int mode, double a_acc, double beta, double a_trial, Scal &out, bool dir);
    int lse_grad(bool init, double a, Scal &out);
    // host-closure objective: xp → pinned host, fdf!, g⁺ → device, then the getβ sums kernel (f rides in its S_F slot)
    int host_trial(double a, bool init, Scal &out);
};

// low-level launcher shared by the backend and the raw helpers
int launch_fused(HipCtx *ctx, int obj_kind, int mode, const void *kparams, int64_t n,
                 bool timed = false, const HipObjective *obj = nullptr, hipEvent_t e0 = nullptr,
                 hipEvent_t e1 = nullptr, double big_forced = -1.0 /* < 0: no solver — the CGO_BIG_BYTES experiment override, else the library's thresholds */);
int grid_for(int64_t n);
double bytes_for(int obj_kind, int mode, int64_t n, int n_params = 0);
int param_unset_error(int slot);   // CGO_ESTATE, the message names the slot
enum MergeKind { MERGE_SUM = 0, MERGE_LSE = 1, MERGE_MAX0 = 2 };
int fetch_sums(HipCtx *ctx, double *sums, int merge = MERGE_SUM, int ns = 10, double *raw = nullptr);  // raw: every rank's block, [world][ns]
int finalize_launch(HipCtx *ctx, int grid, bool lse);
int finalize_rows(HipCtx *ctx, int rows, int ns, bool canon = false);
int fill_device(HipCtx *ctx, double *v, int64_t n, int64_t offset, int kind, uint64_t seed, double lo,
                double hi);

Comm *make_rccl_comm(HipCtx *ctx, int rank, int world, const void *unique_id128);
Comm *make_callback_comm(int rank, int world, cgo_allgather_fn fn, void *user);
Comm *make_shm_comm(HipCtx *ctx, int rank, int world, const char *name, int create);
int rccl_unique_id(void *out128);
bool rccl_available();

}  // namespace cgo
