/*
 * cgo.h — C ABI of the MI355X-native inner-iteration engine for
 * ConjugateGradientOptim.jl's nonlinear-CG / quasi-Newton hot path.
 *
 * This is the drop-in boundary: a Julia host (`ccall`), or any other FFI,
 * binds exactly these symbols.  Plain pointers and sizes only; no C++ or torch
 * types; no exceptions cross it.  Every entry point names the reference
 * interface it replaces (paths relative to the reference repository).
 *
 * Conventions
 *   - return value: 0 = CGO_OK, otherwise an API error (bad argument, failed
 *     config assertion, HIP/RCCL error); cgo_last_error() has the message.
 *     The reference throws only on config @asserts; numerical outcomes are
 *     status symbols.  Same here: the numerical outcome is cgo_results.status.
 *   - all vectors are Float64, contiguous.  "local" sizes refer to this
 *     rank's contiguous shard [offset, offset + n_local) of the n_global state.
 *   - host buffers are caller-owned; device memory is owned by the ctx.
 *   - one solve per ctx at a time; distinct ctx may be used concurrently.
 *   - there is NO CPU fallback: without a usable HIP device cgo_ctx_create
 *     fails with CGO_ENODEV.
 */
#ifndef CGO_H
#define CGO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGO_VERSION 100

/* ---- API error codes --------------------------------------------------- */
enum {
    CGO_OK = 0,
    CGO_EINVAL = 1,  /* bad argument, or a reference @assert would have fired */
    CGO_EHIP = 2,    /* HIP runtime error */
    CGO_ECOMM = 3,   /* RCCL / communicator error */
    CGO_ENODEV = 4,  /* no usable gfx950 device */
    CGO_ESTATE = 5,  /* call sequence error (e.g. iterate before start) */
    CGO_ENOMEM = 6
};

/* ---- numerical outcome: one integer per reference status Symbol -------- */
enum {
    CGO_INCOMPLETE = 0,                                /* src/engine/optim.jl:39  */
    CGO_SUCCESS = 1,                                   /* src/engine/optim.jl:64  */
    CGO_INCREASING_OBJECTIVE = 2,                      /* src/engine/optim.jl:76  */
    CGO_NON_FINITE_OBJECTIVE_OR_GRADIENT_PROPOSED = 3, /* src/engine/optim.jl:118 */
    CGO_MAX_ITERS_REACHED = 4,                         /* src/engine/optim.jl:168 */
    CGO_NON_DESCENT_SEARCH_DIRECTION = 5,              /* src/linesearch/nocedal.jl:62, wolfe.jl:42 */
    CGO_LINESEARCH_A_MAX_OVERFLOW = 6,                 /* src/linesearch/nocedal.jl:148 */
    CGO_LINESEARCH_MAX_ITERS_REACHED = 7,              /* nocedal.jl:157, wolfe.jl:164 */
    CGO_ZOOM_MAX_ITERS_REACHED = 8,                    /* nocedal.jl:208 */
    CGO_ACCEPTED_NON_FINITE_ITERATE = 9,               /* wolfe.jl:37  */
    CGO_CANNOT_FIND_INITIAL_FEASIBLE_STEP = 10,        /* wolfe.jl:64  */
    CGO_MAX_STEP_LENGTH_REACHED = 11,                  /* wolfe.jl:111 */
    CGO_CANNOT_FIND_FEASIBLE_STEP = 12,                /* wolfe.jl:157 */
    CGO_STEP_BRACKET_PRECISION_ISSUE = 13,             /* wolfe.jl:131 (unreachable in the reference) */
    CGO_BISECTION_LOWER_BOUND_LARGER_THAN_PROPOSED_STEP = 14, /* wolfe.jl:187 */
    CGO_FEASIBLE = 15,                                 /* wolfe.jl:197 */
    CGO_INFEASIBLE = 16,                               /* wolfe.jl:206 */
    CGO_NON_FINITE_STEP_PROPOSED = 17,                 /* geometric.jl:129 */
    CGO_PROPOSED_STEP_SAME_AS_CURRENT_STEP = 18,       /* geometric.jl:133 */
    CGO_LINESEARCH_FAILED = 19,                        /* solve_system.jl:139 — where the reference itself
                                                        * throws UndefVarError (solve_system.jl:55) */
    CGO_NUM_STATUS = 20
};

/* ---- βConfig subtypes (src/types.jl:5-7; src/cg_flavours.jl) ----------- */
enum {
    CGO_BETA_HAGER_ZHANG = 0,      /* HagerZhang            cg_flavours.jl:83-108  */
    CGO_BETA_YUAN_WANG_SHENG = 1,  /* YuanWangSheng{T}(μ)   cg_flavours.jl:46-79   */
    CGO_BETA_SALLEH_ALHAWARAT = 2, /* SallehAlhawarat       cg_flavours.jl:130-151 */
    CGO_BETA_LIU_STORREY = 3,      /* LiuStorrey            cg_flavours.jl:154-170 */
    CGO_BETA_POLAK_RIBIERE = 4,    /* new CGβConfig (stub at cg_flavours.jl:173-174) */
    CGO_BETA_HESTENES_STIEFEL = 5, /* new CGβConfig (commented at cg_flavours.jl:110-127) */
    CGO_BETA_DAI_YUAN = 6,         /* new CGβConfig */
    CGO_BETA_LBFGS = 7,            /* new QNβConfig; dispatch contract src/qn_flavours.jl:5-48 */
    CGO_BETA_BROYDEN_FAMILY = 8    /* BroydenFamily{T}(θ, B) — src/qn_flavours.jl:53-90.  Its update solves
                                    * s = B\y first (:81), hence Bs = y, sBs = s·y, v = 0 and B_new = B up to
                                    * rounding (:83-87): B stays the identity it is initialised/reset to (:13-15,
                                    * :33-36) and u = B\(−g) is steepest descent for every θ.  The engine takes
                                    * u = −g exactly, without the dense n×n matrix and its O(n³) solves; the oracle
                                    * carries the dense algebra and agrees to ≈ 1e-15. */
};

/* ---- LineSearchConfig subtypes (src/types.jl:1) ------------------------ */
enum {
    CGO_LS_STRONG_WOLFE_BISECTION = 0, /* StrongWolfeBisection{T}  nocedal.jl:3-11 */
    CGO_LS_WOLFE_BISECTION = 1,        /* WolfeBisection{T,CT}     wolfe.jl:6-11   */
    CGO_LS_BACKTRACKING = 2            /* Backtracking{T,CT}       geometric.jl:15-20 (restated bug for bug) */
};
enum {
    CGO_COND_WOLFE = 0,        /* Wolfe{T}(c1,c2)              wolfe.jl:259-262 */
    CGO_COND_YUAN_WEI_LU = 1,  /* YuanWeiLuWolfe{T}(c1,c2,δ1)  wolfe.jl:213-217 */
    CGO_COND_ARMIJO = 2        /* Armijo{T}(c1)                geometric.jl:159-162 */
};

/* ---- device objective descriptors (replace the `fdf!` closure of
 *      src/engine/optim.jl:25 and src/cg_utils.jl:19 on the GPU path) ----- */
enum {
    CGO_OBJ_QUAD_DIAG = 0,         /* f = ½ Σ D_i x_i²; param vector slot 0 = D     */
    CGO_OBJ_ROSENBROCK_PAIRED = 1, /* f = Σ_j 100(x_{2j}−x_{2j−1}²)² + (1−x_{2j−1})² */
    CGO_OBJ_BOOTH = 2,             /* examples/helpers/test_funcs.jl:3-12 (n = 2)   */
    CGO_OBJ_LSE = 3,               /* f = log Σ e^{x_i} + ½λ‖x‖²; scalar slot 0 = λ  */
    CGO_OBJ_USER = 4,              /* user-supplied element-wise source, see cgo_objective_create_from_source */
    CGO_OBJ_HOST = 5,              /* a host closure f = fdf!(g, x), see cgo_objective_create_callback */
    CGO_OBJ_ROSENBROCK_CHAINED = 6 /* f = Σ_{i<N−1} (1−x_i)² + 100(x_{i+1}−x_i²)² — examples/helpers/test_funcs.jl:50-57 (value;
                                    * BASELINE config 1's second form).  A 3-point STENCIL objective: neighbours are
                                    * re-read from cache, x/u advance out of place, and shard boundaries carry a 2-element
                                    * halo inside the per-launch scalar block.  Any N ≥ 2.
                                    * LAUNCH POLICY, fenced (round 4): this objective runs host-driven launches of ONE or THREE
                                    * trial points — cgo_solver_policy.points > 3 is clamped to 3, controller_depth is ignored (no
                                    * on-device controller), CG β kinds only; the resident solver takes it in ONE workgroup, i.e.
                                    * up to ≈ 4 800 elements on a single rank (x, u in two LDS copies each) — larger or sharded
                                    * stencil problems keep a launch per line-search step.  5/7-point stencil launches and a
                                    * multi-workgroup resident form (halos between workgroups) are NOT built. */
};

/* initial-iterate fills done on the device (global index aware) */
enum {
    CGO_FILL_CONSTANT = 0,   /* v_i = lo                                  */
    CGO_FILL_UNIFORM = 1,    /* v_i = lo + (hi−lo)·U(seed ⊕ i), splitmix64 */
    CGO_FILL_ALTERNATE = 2   /* v_i = (i even) ? lo : hi   (Rosenbrock −1.2, 1) */
};

typedef struct cgo_beta_config {
    int32_t kind;
    int32_t lbfgs_m; /* history length for CGO_BETA_LBFGS */
    double mu;       /* YuanWangSheng μ, 0 < μ < 1 */
} cgo_beta_config;

/* CGConfig{T,BT,ET} (src/types.jl:156-169) built by setupCGConfig (:171-203) */
typedef struct cgo_cg_config {
    double eps;            /* ϵ, asserted 0 < ϵ < 1 (types.jl:187) */
    cgo_beta_config beta;  /* β_config */
    int64_t max_iters;
    int32_t verbose;       /* stored, not functional (as in the reference) */
    int32_t trace_enabled; /* EnableTrace / DisableTrace (types.jl:9-11) */
} cgo_cg_config;

/* union of StrongWolfeBisection (nocedal.jl:3-30),
 * WolfeBisection{Wolfe|YuanWeiLuWolfe} (wolfe.jl:6-11,213-217,259-262) and
 * Backtracking{Armijo} (geometric.jl:15-20,159-162) */
typedef struct cgo_ls_config {
    int32_t kind;
    int32_t cond_kind;
    double c1, c2;
    double a_max_growth_factor;
    double delta1;
    double max_step_size;
    int64_t max_iters;
    int64_t zoom_max_iters;
    int64_t feasibility_max_iters;
    double discount_factor;          /* Backtracking.discount_factor */
} cgo_ls_config;

/* Results{T,TrT} (src/types.jl:107-114) + TraceContainer{T,ET} (:17-23).
 * All pointers are caller-allocated host buffers and may be NULL to skip. */
typedef struct cgo_results {
    double objective;
    double *minimizer;              /* [n_local] this rank's shard */
    double *gradient;               /* [n_local] */
    int64_t iters_ran;
    int32_t status;
    int32_t _pad;
    double *trace_objective;        /* [max_iters]; valid [0, iters_ran) */
    double *trace_grad_norm;
    double *trace_step_size;
    int64_t *trace_objective_evals;
    int64_t total_fdf_evals;        /* engine counter: objective evaluations incl. the initial one */
    int64_t total_launches;         /* engine counter: kernel launches */
} cgo_results;

typedef struct cgo_ctx cgo_ctx;
typedef struct cgo_objective cgo_objective;
typedef struct cgo_solver cgo_solver;

/* cross-rank exchange hook for hosts that bring their own communicator
 * (e.g. MPI.jl): gather `count` doubles from every rank, rank-major, into
 * recv[world*count].  Must return 0 on success. */
typedef int (*cgo_allgather_fn)(void *user, const double *send, double *recv, int32_t count);

/* ---- library ----------------------------------------------------------- */
int cgo_version(void);
/* hex digest of the sources this binary was built from (the .hip / .hpp files of csrc and this header): lets a
 * measurement (the PMC summaries under profiles/) be tied to the exact kernels it was taken on */
const char *cgo_build_id(void);
const char *cgo_last_error(void);
const char *cgo_status_name(int32_t status);   /* the reference's Symbol text */
int cgo_device_count(int32_t *count);

/* config validation = the reference's @assert sites:
 * types.jl:187; nocedal.jl:22-26; wolfe.jl:233,278; geometric.jl:169 */
int cgo_check_cg_config(const cgo_cg_config *cfg);
int cgo_check_ls_config(const cgo_ls_config *ls);

/* ---- context: one GPU, one shard --------------------------------------- */
int cgo_ctx_create(int32_t device, cgo_ctx **out);
int cgo_ctx_destroy(cgo_ctx *ctx);
/* RCCL communicator over xGMI for the scalar exchange. unique_id: 128 bytes
 * from cgo_comm_unique_id on rank 0, broadcast by the host. */
int cgo_comm_unique_id(void *out128);
int cgo_ctx_set_comm_rccl(cgo_ctx *ctx, int32_t rank, int32_t world, const void *unique_id128);
int cgo_ctx_set_comm_callback(cgo_ctx *ctx, int32_t rank, int32_t world, cgo_allgather_fn fn,
                              void *user);
/* Single-node, lowest latency: a POSIX shared-memory mailbox.  Rank 0 calls with create = 1 first,
 * the host synchronises, the other ranks call with create = 0, the host synchronises again and rank
 * 0 may cgo_shm_unlink(name).  Every rank's finalize kernel then stores its ≤ 64-double block and a
 * sequence word directly into its slot of the segment (registered with HIP); all ranks read all
 * slots from host memory: no collective call per launch. */
int cgo_ctx_set_comm_shm(cgo_ctx *ctx, int32_t rank, int32_t world, const char *name, int32_t create);
int cgo_shm_unlink(const char *name);
/* Device mailboxes for the shared-memory communicator (SURVEY.md §8(e) "fast path"): COLLECTIVE — every rank calls it once,
 * after all ranks have attached to the segment.  Each rank exported a small block of its own HBM through the segment
 * (hipIpcGetMemHandle); this call opens every peer's (hipIpcOpenMemHandle: over xGMI between GPUs of a node) and agrees
 * with the others on whether everybody could.  *connected = 1: the finisher of a controller-armed launch now stores its
 * block straight into its peers' GPUs and sums the world's blocks itself, so armed rounds (csrc/cgo_ctl.hpp) work across
 * ranks without the host; host-driven launches keep publishing into the host slots.  *connected = 0 (more than 8 ranks, IPC
 * refused, CGO_NO_DEVICE_MAILBOX set): nothing changes.  Never an error for that reason. */
int cgo_ctx_comm_connect_devices(cgo_ctx *ctx, int32_t *connected);
/* Diagnostics of the scalar exchange (the reference has no counterpart: SURVEY.md §5 "Distributed
 * communication backend: none").  kind: 0 = single rank, 1 = shared-memory mailbox, 2 = RCCL, 3 = host callback.
 * ranks_seen: how many ranks the transport itself reports — ncclCommCount for RCCL, the number of mailbox slots
 * that have published at least one launch for the mailbox, `world` for a callback. */
int cgo_ctx_comm_info(cgo_ctx *ctx, int32_t *kind, int32_t *rank, int32_t *world, int32_t *ranks_seen);
/* Exchange cost since the last reset.  exchanges: launches whose sums crossed ranks.  peer_wait_us: host time
 * between this rank's own block being visible and the LAST peer's block being visible (mailbox: skew + PCIe
 * latency; 0 for the other transports).  device_exchange_us: mean duration on the GPU of the all-gather +
 * publish of a sampled launch (RCCL and forced-gather paths; HIP events around every 4th exchange; 0 otherwise).
 * reset != 0 zeroes the counters after reading them. */
int cgo_ctx_exchange_stats(cgo_ctx *ctx, int64_t *exchanges, double *peer_wait_us, double *device_exchange_us,
                           int32_t reset);
/* 1 if librccl can be loaded in this process (cgo_ctx_set_comm_rccl is a collective call: check first) */
int cgo_rccl_available(void);

/* ---- objective descriptor ---------------------------------------------- */
int cgo_objective_create(cgo_ctx *ctx, int32_t kind, int64_t n_global, int64_t offset,
                         int64_t n_local, cgo_objective **out);
/* "User-supplied element-wise f/∇f": the device-side form of handing `minimizeobjective` an
 * arbitrary `fdf!` closure (src/engine/optim.jl:25).  `source` is HIP C++ text compiled at run
 * time (hiprtc, gfx950, -ffp-contract=off) into the same fused kernel templates the built-in
 * objectives use.  Either
 *   - the statements of an element-wise body that set `fi` (the term f_i) and `gi` (∂f_i/∂x_i)
 *     from `x` (the element), `p` (its entry of parameter vector slot 0, if has_param) and `s0`
 *     (scalar slot 0), e.g.  "gi = p*x; fi = 0.5*(gi*x);"   or
 *   - a complete `struct UserObjective { kParam; kPairOnly; eval2(); eval1(); };` (the functor
 *     interface of csrc/cgo_kernels.hip.hpp) for objectives coupling the two elements of a pair.
 * On a compile error returns CGO_EINVAL; cgo_last_error() holds the hiprtc log.
 * has_param != 0 means one parameter vector (n_params = 1 of the _ex form below). */
int cgo_objective_create_from_source(cgo_ctx *ctx, const char *source, int32_t has_param,
                                     int64_t n_global, int64_t offset, int64_t n_local,
                                     cgo_objective **out);
/* The same with up to CGO_MAX_PARAM_SLOTS parameter vectors (per-element data: weights, targets, bounds …), each of
 * n_local doubles, read by every kernel the objective is compiled into.
 *   - An element-wise body sees slot 0 as `p` and slots 1, 2, 3 as `p1`, `p2`, `p3`, e.g. (n_params = 3)
 *       "const double d = x - p1; gi = p*d + p2; fi = 0.5*((p*d)*d) + p2*x;"
 *   - A `struct UserObjective` that reads more than one slot declares `static constexpr int kParams = K;` (2 ≤ K ≤ 4)
 *     instead of relying on kParam, and takes the slots as arrays:
 *       eval1(double x, const double (&p)[K], double s0, double &f, double &g)
 *       eval2(d2 x,     const d2     (&p)[K], double s0, double &f, d2 &g)
 *     A struct whose kParams differs from n_params (or that declares none while n_params > 1) does not compile:
 *     CGO_EINVAL, the message in cgo_last_error().
 * Every slot must be set (cgo_objective_set_param_host / _device / cgo_objective_fill_param) before a solve starts:
 * CGO_ESTATE otherwise, naming the first slot that is missing.  Built-in objectives keep their 0 or 1 slot.
 * Each slot adds 8 B per element to every launch that evaluates the objective (accept + direction + trial:
 * (32 + 8·n_params) B, trial: (16 + 8·n_params) B), and one vector to what the resident solver keeps in LDS, so the
 * largest shard it takes shrinks by the factor 3/(2 + n_params) against a one-slot objective.  The placement search
 * (cgo_solver_placement_info) times a three-stream mix and does not run for n_params > 1. */
#define CGO_MAX_PARAM_SLOTS 4
int cgo_objective_create_from_source_ex(cgo_ctx *ctx, const char *source, int32_t n_params /* 0 … CGO_MAX_PARAM_SLOTS */,
                                        int64_t n_global, int64_t offset, int64_t n_local,
                                        cgo_objective **out);
/* how many parameter slots the objective reads (built-in: 0 or 1) */
int cgo_objective_num_params(cgo_objective *obj, int32_t *n_params);
/* The reference's objective contract itself: `f = fdf!(g, x)` (src/engine/optim.jl:25, src/cg_utils.jl:19; exemplar
 * examples/helpers/test_funcs.jl:3-12) as a C callback — what Julia's `@cfunction` of an existing `fdf!` closure
 * produces, so that `minimizeobjective(boothfdf!, x0, config, ls)` (examples/min.jl:41) is a drop-in without rewriting
 * the objective as device code.  This is still the GPU engine: x, u, both gradients, every AXPY / direction update /
 * dot / norm / getβ sum and the line-search state machine stay where they are for the built-in objectives; per trial the
 * engine forms xp = x + a·u on the device straight into pinned host memory, calls `fn` there (it writes g, returns f)
 * and moves g back.  One trial step per launch, no on-device controller; CG β kinds, L-BFGS, all three line searches.
 * The callback sees this rank's shard [offset, offset + n_local) and returns this rank's part of f (the parts are summed
 * across ranks) — only separable objectives shard.  Throughput is PCIe-bound (16 B/element per trial): the device
 * objectives above are the fast path. */
typedef double (*cgo_fdf_fn)(void *user, double *g_local, const double *x_local, int64_t n_local);
int cgo_objective_create_callback(cgo_ctx *ctx, cgo_fdf_fn fn, void *user, int64_t n_global, int64_t offset,
                                  int64_t n_local, cgo_objective **out);
int cgo_objective_destroy(cgo_objective *obj);
int cgo_objective_set_param_host(cgo_objective *obj, int32_t slot, const double *host_local);
int cgo_objective_fill_param(cgo_objective *obj, int32_t slot, int32_t fill_kind, uint64_t seed,
                             double lo, double hi);
/* The same for a vector that already lives in THIS GPU's memory: n_local doubles, copied device-to-device like
 * cgo_solver_set_x0_device.  All three setters take slot < cgo_objective_num_params (CGO_EINVAL otherwise). */
int cgo_objective_set_param_device(cgo_objective *obj, int32_t slot, const double *dev_local);
int cgo_objective_set_scalar(cgo_objective *obj, int32_t slot, double value);
/* Cost class of a user objective: how many speculative trial steps a fused launch evaluates.
 * 0 (default for cgo_objective_create_from_source): heavier than a few flops per element — one step per launch
 * below n_local = 3e6, three above, on-device controller on.  1: cheap (f and ∇f cost ≲ 10 flops per element,
 * like the built-in quadratic) — seven steps per launch.  Built-in objectives carry their own class. */
int cgo_objective_set_cost_class(cgo_objective *obj, int32_t cost_class);
/* U2: f = fdf!(g, x) for host vectors (H2D, one launch, D2H) — KAT entry */
int cgo_objective_eval_host(cgo_objective *obj, const double *x_local, double *g_local,
                            double *f_global);

/* ---- solver policy -------------------------------------------------------
 * HOW a solve runs — never WHAT it computes: every setting below changes launch counts, kernels or hand-off protocols,
 * not the step sequence (the parity tests hold each of them to the same oracle).  A field left at its "library policy"
 * value (what cgo_solver_policy_init writes) is decided by the library from the objective, the problem size and the
 * context; the CGO_* environment variables of earlier rounds remain as overrides FOR EXPERIMENTS and apply only to fields
 * left at "library policy" (an explicit field always wins).  No counterpart in the reference (it has one code path).
 * Order of precedence per field: cgo_solver_create_ex argument > cgo_ctx_set_default_policy > environment > library. */
typedef struct cgo_solver_policy {
    int32_t size;                 /* sizeof(cgo_solver_policy), written by cgo_solver_policy_init (versioning) */
    int32_t points;               /* trial steps per fused launch: 0 library policy | 1 | 3 | 5 | 7   */
    int32_t resident;             /* resident solver (§2.12): -1 library policy | 0 off | 1 on where objective and size allow */
    int32_t controller_depth;     /* on-device line-search controller (§2.7): -1 library policy | 0 host-driven | k armed rounds in flight */
    int32_t controller_graph;     /* armed rounds replayed from hipGraphs: -1 library policy (off) | 0 | 1 */
    int32_t controller_fused;     /* an armed round as ONE launch: -1 library policy (on) | 0 reduce + controller launches | 1 */
    int32_t stored_gradient;      /* 0 library policy (gradient-free k_cg family where it applies) | 1 stored-gradient k_fused family */
    int32_t fused_tail;           /* a launch sums its own rows (§2.4): -1 keep the context's setting | 0 finalize launches | 1 fused.  CONTEXT-WIDE */
    int32_t strict_tail;          /* hand-offs by __threadfence_system + release store instead of self-validating blocks (§2.4):
                                     -1 keep the context's setting (off) | 0 | 1.  CONTEXT-WIDE: applies to later solvers of the ctx too */
    int32_t placement_search;     /* buffer placement search at pure-HBM sizes (§2.5; a measured HEURISTIC: it finds a faster
                                     (x, u, D) buffer triple in 5 of 8 processes, none in the others; 10–450 ms and up to
                                     placement_max_bytes of transient memory per solver): -1 library policy (OFF: opt-in) | 0 off | 1 on */
    int32_t placement_stages;     /* 0 library policy (3) | 1..3: stages of 8 spare vectors the search may allocate */
    int64_t placement_max_bytes;  /* cap on the search's TRANSIENT device memory: 0 library policy (min(24 vectors, a quarter of the
                                     free memory)) | bytes.  Below 8 vectors' worth the search does not run */
    int32_t lbfgs_form;           /* 0 library policy | 1 one ring pass per iteration, state update riding in the next pass (§2.3) |
                                     2 one ring pass + a state-update launch of its own | 3 Gram form, two passes | 4 chained two-loop */
    int32_t lbfgs_fuse_grad;      /* the log-sum-exp push forms g⁺ itself: -1 library policy (on) | 0 | 1 */
    int32_t lbfgs_fuse_trial;     /* first trial of the next line search in the direction pass: -1 library policy (on) | 0 | 1 */
    int32_t lse_fixed_reference;  /* log-sum-exp statistics against a fixed reference instead of a running maximum: -1 (on) | 0 | 1 */
    int32_t resident_points;      /* 0 library policy (3) | 1 | 3 | 7: trial steps per pass of the resident solver */
    int32_t resident_chunk;       /* 0 library policy (4096) | even number of elements per workgroup of the resident solver */
    double hbm_stream_bytes;      /* a launch moving more than this streams pure-HBM style (contiguous chunks, non-temporal; §2.5):
                                     0 library policy (1.4e9 read-write, 4.5e8 read-only) | bytes (1 = every launch) */
    int32_t reserved[8];          /* zero */
} cgo_solver_policy;
void cgo_solver_policy_init(cgo_solver_policy *p);                               /* every field = library policy */
int cgo_ctx_set_default_policy(cgo_ctx *ctx, const cgo_solver_policy *policy);   /* for every solver this context creates from now on,
                                                                                    the one-shot entry points included; NULL resets */
/* what a solver actually runs with, after the precedence above (reporting; tests) */
int cgo_solver_get_policy(cgo_solver *s, cgo_solver_policy *out);

/* ---- solver: resumable form of minimizeobjective (optim.jl:6-171) ------
 * Memory: x and u (16 B per local element; the k_cg family keeps no gradient vector) — plus two gradient buffers for the
 * stored-gradient families (quasi-Newton flavours, host closures, log-sum-exp), the 2(m + 1) vectors of the L-BFGS ring,
 * and a second iterate buffer for L-BFGS on log-sum-exp (the fused push advances x out of place).
 * Creation time: with cgo_solver_policy.placement_search = 1 (opt-in since round 4; bench.py opts in) and a pure-HBM problem
 * size (the dominant launch moves more than 1.4 GB: n_local ≳ 3.5e7 for the quadratic) creating a solver runs the placement
 * search of DESIGN.md §2.5: up to 24 spare n-vectors — never more than placement_max_bytes, by default a quarter of the free
 * device memory — are allocated transiently and up to ≈ 190 short launches timed — 10–150 ms at n = 1e8 (≤ 450 ms observed) —
 * and the parameter vector of the objective may be moved to another buffer (only while this solver is the objective's sole
 * user).  The pair (x, u) it kept is parked in the context when the solver is destroyed and taken over by the next solver of
 * the same size (rerun chains, centering steps); parked buffers of another size are released before a new solver allocates. */
int cgo_solver_create_ex(cgo_ctx *ctx, cgo_objective *obj, const cgo_cg_config *cfg, const cgo_ls_config *ls,
                         const cgo_solver_policy *policy /* NULL = the context's default */, cgo_solver **out);
int cgo_solver_create(cgo_ctx *ctx, cgo_objective *obj, const cgo_cg_config *cfg,
                      const cgo_ls_config *ls, cgo_solver **out);
int cgo_solver_destroy(cgo_solver *s);
int cgo_solver_set_x0_host(cgo_solver *s, const double *x0_local);
int cgo_solver_set_x0_fill(cgo_solver *s, int32_t fill_kind, uint64_t seed, double lo, double hi);
/* The same for callers whose vectors already live in THIS GPU's memory (a ROCArray, a torch tensor): x0_dev is a
 * device pointer to n_local doubles, copied device-to-device (optim.jl:21 copies x_initial too).  No PCIe traffic:
 * at n = 1e8 the host form moves 0.8 GB in (and cgo_solver_results 1.6 GB out) ≈ 50 ms, against 0.9 ms per iteration. */
int cgo_solver_set_x0_device(cgo_solver *s, const double *x0_dev);
/* optim.jl:25-47: initial fdf!, ‖g‖, u = −g */
int cgo_solver_start(cgo_solver *s);
/* optim.jl:50-160: run at most `iters` further outer iterations;
 * *finished = 1 once a terminal status was reached */
int cgo_solver_iterate(cgo_solver *s, int64_t iters, int32_t *finished);
/* optim.jl:162-170 / updateresult! (types.jl:134-151).  Also where a reduction that gave up on a partial-row slot
 * (it leaves a NaN in that launch's sums) surfaces: CGO_EHIP instead of a record that blames the objective. */
int cgo_solver_results(cgo_solver *s, cgo_results *out);
/* Results.minimizer / Results.gradient (types.jl:107-114) into DEVICE buffers of n_local doubles each (either may be
 * NULL); everything else of the record through cgo_solver_results with NULL vector pointers. */
int cgo_solver_results_device(cgo_solver *s, double *minimizer_dev, double *gradient_dev);
/* branch log of every evalϕdϕ! (cg_utils.jl:4-23): (a, ϕ, dϕ); returns count */
int cgo_solver_trial_log(cgo_solver *s, int64_t cap, double *a, double *phi, double *dphi,
                         int64_t *count);
/* per-kernel-kind HIP-event timings accumulated since start / last reset */
int cgo_solver_profile_enable(cgo_solver *s, int32_t on);
int cgo_solver_profile_reset(cgo_solver *s);
int cgo_solver_profile_get(cgo_solver *s, int32_t kernel_kind, int64_t *launches,
                           double *total_ms, double *bytes_per_launch);
const char *cgo_kernel_kind_name(int32_t kernel_kind);
/* which kernel family the solver launches: "k_cg (gradient-free, N-point)" with N = 1, 3, 5 or 7 trial steps per launch,
 * "k_fused (stored gradient)", "k_lse (two-phase)"; L-BFGS adds "+ k_lbfgs" */
const char *cgo_solver_kernel_family(cgo_solver *s);
/* Launches that were armed by the on-device controller (csrc/cgo_ctl.hpp) instead of the host:
 * streaks of outer iterations whose line search accepts its first trial (nocedal.jl:78-110,
 * wolfe.jl:51-78) run device-side; the host replays them from published records.  Depth of the
 * run-ahead: env CGO_CTL_DEPTH (0 = the host drives every launch; default 4 for objectives whose
 * launches carry at most three trial steps, 0 for the cheap built-in ones — DESIGN.md §2.7). */
int64_t cgo_solver_controller_launches(cgo_solver *s);
/* Resident solver (csrc/cgo_resident.hpp): for cache-sized shards — x, u and the parameter vector fit the LDS of the chip,
 * n ≲ 1.6e6 with a parameter vector — of the built-in element-wise objectives under a CGβConfig and StrongWolfeBisection /
 * WolfeBisection on one rank, cgo_solver_iterate runs a whole slice of outer iterations (optim.jl:50-160: line search,
 * getβ, updatedir!) inside ONE launch; iterations it cannot complete (any outcome other than :success, rare-path norms)
 * are run by the host-driven path as before.  Reports the slices launched, the iterations completed inside them, and how
 * often a slice was given up because its workgroups could not all run at once (another process holding CUs): such a slice
 * changes nothing, the launch-per-trial engine redoes it, and the solver stays off the resident path afterwards.
 * Environment: CGO_RESIDENT=0 switches it off; CGO_RES_CHUNK (elements per workgroup), CGO_RES_POINTS (1 | 3 | 7). */
int cgo_solver_resident_stats(cgo_solver *s, int64_t *slices, int64_t *iterations, int64_t *gave_up);
/* L-BFGS (Gram form, m ≤ 10) on the log-sum-exp, separable-quadratic, paired-Rosenbrock and user-compiled objectives: how the state updates
 * ("pushes") of this solver were paid for.
 * `speculated`: the direction pass had already taken every inner product at the step that was then accepted — one pass
 * over the ring for that iteration (k_lbfgs_combine_spec; the 56 B/element state update rides in the NEXT direction
 * pass, or runs as k_lbfgs_push_lite when none follows); `fused`: the push read the ring and formed g⁺ itself
 * (k_lbfgs_push_gram_lse; log-sum-exp only); `plain`: k_lbfgs_push_gram on a gradient a launch of its own wrote.
 * Environment: CGO_LBFGS_SPEC=0 (1: the state update always as its own launch), CGO_LBFGS_FUSE_GRAD=0 switch the first two off. */
int cgo_solver_lbfgs_stats(cgo_solver *s, int64_t *speculated, int64_t *fused, int64_t *plain);
int cgo_num_kernel_kinds(void);
/* Lazy direction.  u_{k+1} = −∇f(x_{k+1}) + β_k·u_k is recoverable, bit for bit, from the stored x_{k+1},
 * the stored u_k and the host scalar β_k, so on an eligible solver — a built-in element-wise objective whose launches are
 * pure-HBM streams driven by the host, updated in place — every second accept + direction + trial launch does not store u
 * (kernel kind "accept_trial_lazy", 8n(2+p+1) bytes) and the next one rebuilds it on load ("accept_dir_trial", R_ULAG
 * instantiation, 8n(2+p+2) bytes); any other reader of u gets it stored first ("materialize_u", not counted in
 * total_launches).  Results are those of the plain launches bit for bit.  Library policy: on for the separable quadratic;
 * env CGO_LAZY_DIR=0|1 forces it for every built-in objective; this call has the last word for one solver.  Meant to be
 * called before cgo_solver_start; later it takes effect at the next launch (switching off stores a lagged u first). */
int cgo_solver_set_lazy_direction(cgo_solver *s, int32_t on);
/* Replay.  The iterate is recoverable as well: x_{k+1} = x_k + a*_k·u_k with the host scalar a*_k.  At replay
 * depth d ≥ 2 an eligible solver (as above) stores NOTHING in d − 1 of every d accept + direction + trial launches (kernel kind
 * "accept_trial_nostore", 8n(2+p) bytes): each rebuilds the current (x, u) in registers from the stored pair and the list of
 * (a*, β) of the steps accepted since, and the d-th ("accept_dir_trial", R_REPLAY instantiation, 8n(2+p+2) bytes) stores both.
 * Any other reader of x or u gets both stored first ("materialize_xu", not counted in total_launches).  Results are those of
 * the plain launches bit for bit.  d = 1 is the lazy direction's alternation.  Library policy: d > 1 only for the separable
 * quadratic where an accepting launch exceeds the library's own pure-HBM threshold (1.4 GB); env CGO_REPLAY_DEPTH=1…16 forces
 * it; this call has the last word for one solver (1 ≤ d ≤ 16; mid-solve, outstanding steps are stored first).
 * Deep replay: d > 8 takes effect where launches N and S run as path launches (below), which take the steps beyond the seventh
 * in a second kernel argument; a trial-only launch met with more than seven steps outstanding runs "k_cg_trial_deep<Obj, NPTS,
 * true>", "materialize_xu" stores a longer list in passes of seven steps, and any other solver runs d > 8 as d = 8.
 * cgo_solver_set_lazy_direction(s, 0) and CGO_LAZY_DIR=0 switch all of it off. */
int cgo_solver_set_replay_depth(cgo_solver *s, int32_t d);
/* What the replay cycle of this solver has launched so far: launches N, S, T (a trial-only launch met with steps outstanding) and M
 * ("materialize_xu" passes); how many of the T and of the M met more than seven outstanding steps; the longest list a launch
 * replayed.  Any pointer may be null. */
int cgo_solver_replay_stats(cgo_solver *s, int64_t *n, int64_t *s_launches, int64_t *t, int64_t *m, int64_t *t_deep, int64_t *m_deep,
                            int32_t *max_list);
/* Lean sums.  A β flavour reads only some of the seven sums a trial point delivers (Polak–Ribière: f, g⁺·u,
 * g⁺·g⁺ and y·g⁺); the seven-point launches are short of FP64 issue slots, not of bytes.  With lean sums on, launches N and S of
 * the replay cycle run instantiations that do not form the sums the solver's flavour never reads (R_NOGTG = 16384,
 * R_NOYY = 32768, R_NOUY = 65536, R_NOYGT = 131072 in the reported symbol): those slots of the row come back +0.0, every other
 * slot, x and u bit for bit as before; kernel kinds and bytes per launch are unchanged.  Kernels exist for Polak–Ribière's mask;
 * a solver of any other flavour keeps the full rows whatever is asked.  Library policy: on where the replay depth's own default
 * is > 1; env CGO_LEAN_SUMS=0|1 forces it for every built-in objective and size; this call has the last word for one solver
 * and takes effect at the next launch (the stored state is the same either way). */
int cgo_solver_set_lean_sums(cgo_solver *s, int32_t on);
/* The kernel instantiation a launch of `kernel_kind` uses under the solver's current policy, as the profiler
 * prints it without namespaces — e.g. "k_cg<ObjQuadDiag, 7, 7, true>" (objective, mode bits, trial points, pure-HBM
 * streaming policy).  Written NUL-terminated into buf[cap]. */
int cgo_solver_kernel_symbol(cgo_solver *s, int32_t kernel_kind, char *buf, int32_t cap);

/* ---- the line-search conditions as scalar functions ------------------------------------------------
 * evalwolfeconditions(condition, ϕ_a, dϕ_a, a, u, ϕ_0, dϕ_0) → (valid_large, valid_small) — wolfe.jl:219-294
 * (Wolfe: :264-294, YuanWeiLuWolfe: :219-251; `uu` = dot(u,u), which the YWL form reads at :240) — and
 * evalbacktrackcondition(::Armijo, ϕ_a, a, ϕ_0, dϕ_0) — geometric.jl:164-186.  The same code the engine and
 * the on-device controller run (csrc/cgo_ctl.hpp).  `ls` supplies cond_kind, c1, c2, delta1. */
int cgo_evalwolfeconditions(const cgo_ls_config *ls, double phi_a, double dphi_a, double a, double uu,
                            double phi_0, double dphi_0, int32_t *valid_large, int32_t *valid_small);
int cgo_evalbacktrackcondition(const cgo_ls_config *ls, double phi_a, double a, double phi_0, double dphi_0,
                               int32_t *valid);

/* ---- solvesystem (src/engine/solve_system.jl; exported at ConjugateGradientOptim.jl:28) ---- */
/* LinesearchSolveSys{T} + setupLinesearchSolveSys — solve_system.jl:6-27 (eqn 18 of Yuan 2019) */
typedef struct {
    double rho;        /* 0 < ρ < 1 (asserted, solve_system.jl:21-22): step shrink factor */
    double sigma;      /* σ (default 0.5; the reference never checks it) */
    double s;          /* s > 0 (asserted, :23): the first trial step */
    int64_t max_iters; /* default round(Int, log(ρ, 1e-6)) = cgo_lss_default_max_iters(ρ) */
} cgo_lss_config;
int cgo_check_lss_config(const cgo_lss_config *ls);
int64_t cgo_lss_default_max_iters(double rho);
/* A solver running solvesystem(fdf!, x_initial, config, linesearch_config) — solve_system.jl:64-237 —
 * instead of minimizeobjective; every other cgo_solver_* call applies unchanged.  CG β kinds and
 * element-wise objectives only.  Restated bug for bug: the projection step is
 * added to the x_next buffer, i.e. to the iterate of two iterations ago (:172-178,:194);
 * trace.objective_evals holds the 0-based index of the accepted trial (:52); status
 * CGO_LINESEARCH_FAILED marks the point where the reference throws UndefVarError (:55). */
int cgo_solver_create_sys(cgo_ctx *ctx, cgo_objective *obj, const cgo_cg_config *cfg,
                          const cgo_lss_config *ls, cgo_solver **out);
int cgo_solver_create_sys_ex(cgo_ctx *ctx, cgo_objective *obj, const cgo_cg_config *cfg, const cgo_lss_config *ls,
                             const cgo_solver_policy *policy /* NULL = the context's default */, cgo_solver **out);
int cgo_solvesystem(cgo_ctx *ctx, cgo_objective *obj, const double *x0_local,
                    const cgo_cg_config *cfg, const cgo_lss_config *ls, cgo_results *out);

/* ---- one-shot drop-ins -------------------------------------------------- */
/* minimizeobjective(fdf!, x_initial, config, linesearch_config)  optim.jl:6-11 */
int cgo_minimize(cgo_ctx *ctx, cgo_objective *obj, const double *x0_local,
                 const cgo_cg_config *cfg, const cgo_ls_config *ls, cgo_results *out);
/* minimizeobjectivererun(fdf!, x_initial, config, ls, rerun_config_tuples...)
 * optim.jl:173-208.  outs has capacity 1 + npairs; *nouts = runs performed.  A stage restarts from the previous
 * stage's minimizer (optim.jl:195-200), which stays on the GPU between the stages (device-to-device copy): the
 * minimizer / gradient buffers of ANY outs[k] may be NULL where the host does not want that stage's vectors.
 * Sharded contexts: every rank calls this with its own shard; all ranks see the same statuses and stage count. */
int cgo_minimize_rerun(cgo_ctx *ctx, cgo_objective *obj, const double *x0_local,
                       const cgo_cg_config *cfg, const cgo_ls_config *ls,
                       const cgo_cg_config *rerun_cfgs, const cgo_ls_config *rerun_ls,
                       int32_t npairs, cgo_results *outs, int32_t *nouts);

/* ---- batched solves: many small problems in one launch, a workgroup each ---------------------------------
 * `batch` independent minimizeobjective problems of the same objective kind and size n under ONE config and line search: a
 * parameter sweep, multi-start, one small fit per pixel.  Each problem occupies one workgroup (k_batch), which runs the
 * reference's outer loop and line search on the device until its stop test fires; a problem whose next iteration the device
 * loop does not run (any line-search outcome other than :success, non-finite values, a rare-path norm, WolfeBisection's
 * bracket collapse) is finished by the ordinary engine, one at a time, with the reference's status and iters_ran.
 * Objectives: CGO_OBJ_QUAD_DIAG (param0 = the [batch*n] rows of D), CGO_OBJ_ROSENBROCK_PAIRED (n even), CGO_OBJ_BOOTH (n = 2).
 * CGO_EINVAL, with a message naming the reason, for any other objective, β = L-BFGS / Broyden, Backtracking, a multi-rank
 * context, batch < 1, n > cgo_batch_max_n, and a missing param0 — there is no fallback to a loop of solves. */
typedef struct cgo_batch_results {      /* every pointer caller-allocated, each may be NULL */
    double  *objective;                 /* [batch] */
    int64_t *iters_ran;                 /* [batch] */
    int32_t *status;                    /* [batch] */
    int64_t *total_fdf_evals;           /* [batch] */
    double  *minimizer, *gradient;      /* [batch * n], row-major, dense */
    double  *trace_objective, *trace_grad_norm, *trace_step_size;   /* [batch * max_iters], row b valid in [0, iters_ran[b]) */
    int64_t *trace_objective_evals;
    int64_t launches, handed_back;      /* out: k_batch launches; problems the host engine finished */
} cgo_batch_results;
int cgo_minimize_batch(cgo_ctx *ctx, int32_t obj_kind, int64_t n, int64_t batch,
                       const double *x0 /* [batch*n] */, const double *param0 /* [batch*n]; NULL unless the objective has a parameter vector */,
                       const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t slice_iters /* 0 = library policy */,
                       cgo_batch_results *out);
int64_t cgo_batch_max_n(cgo_ctx *ctx, int32_t obj_kind);   /* largest n one workgroup's LDS holds (same arithmetic as the resident plan); 0: none */
/* The same for a RUN-TIME COMPILED objective: the caller's own element-wise body or `struct UserObjective`, with its up to
 * CGO_MAX_PARAM_SLOTS per-element data vectors given per problem.
 * `model`: an objective from cgo_objective_create_from_source[_ex] on a single-rank ctx whose n_global = n_local = n is the size of
 * ONE problem; it supplies the compiled source, n_params, scalar slot 0 (shared by all problems) and the cost class.  Its own
 * parameter slots are neither read nor written.  params[j] (j < n_params) = the [batch*n] rows of slot j.
 * The kernel (k_batch for the model's objective) is a second program of the model's compiled module: the first batched call on
 * a module — cgo_batch_max_n_obj included — compiles it (seconds), every later one on an objective of the same text finds it.
 * One workgroup holds 2 + n_params vectors of a problem: cgo_batch_max_n_obj shrinks with the slots.  A `struct
 * UserObjective` with kPairOnly = true needs an even n; that stays the caller's matter, as for a single solve.  Where n is odd
 * the rows are padded by one element on the device; that element of x and of every slot repeats element n − 1 of its row, so
 * the body is never evaluated on data the caller did not supply.
 * CGO_EINVAL, with a message naming the reason, for a model that is not run-time compiled (those: cgo_minimize_batch), a
 * sharded or multi-rank model, n_params other than the model's, a null params[j], n > cgo_batch_max_n_obj, and everything
 * cgo_minimize_batch refuses of a config. */
int cgo_minimize_batch_obj(cgo_ctx *ctx, cgo_objective *model, int64_t batch, const double *x0 /* [batch*n] */,
                           const double *const *params, int32_t n_params,
                           const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t slice_iters /* 0 = library policy */,
                           cgo_batch_results *out);
int64_t cgo_batch_max_n_obj(cgo_objective *model);   /* 0: none */
/* A batch that STAYS ON THE DEVICE between solves: the concatenated problems of cgo_minimize_batch_obj, their slot rows uploaded
 * once, solved any number of times — each time from its own x0, under its own config and line search, optionally with
 *   scalars [batch]: every problem's OWN scalar slot 0 for this solve (a barrier weight t, a regularisation strength per
 *                    problem) — NULL: the model's, for all, and every number is what cgo_minimize_batch_obj returns;
 *   active  [batch] bytes: nonzero = the problem runs.  An inactive problem costs its workgroup one load and a return, and its
 *                    entries of every array of `out` are left untouched — NULL: all run.
 * The model's scalar and cost class are read at every solve; the handle holds a reference on the model.  With scalars,
 * Results.gradient comes from a kernel of the batch program that evaluates every row with its own scalar (k_batch_grad), and a
 * problem the host engine finishes is finished under its own scalar.
 * cgo_batch_open refuses what cgo_minimize_batch_obj refuses of a model, a batch and params; cgo_batch_solve what it refuses of a
 * config, and a non-finite entry of scalars and an `active` that selects no problem (CGO_EINVAL, the reason in the message). */
typedef struct cgo_batch cgo_batch;
int cgo_batch_open(cgo_ctx *ctx, cgo_objective *model, int64_t batch, const double *const *params, int32_t n_params,
                   cgo_batch **handle);
int cgo_batch_solve(cgo_batch *handle, const double *x0 /* [batch*n] */, const double *scalars /* [batch] or NULL */,
                    const unsigned char *active /* [batch] or NULL */, const cgo_cg_config *cfg, const cgo_ls_config *ls,
                    int64_t slice_iters /* 0 = library policy */, cgo_batch_results *out);
int cgo_batch_close(cgo_batch *handle);
/* WHERE A PROBLEM'S ROWS LIVE during a batched solve — the size limit of the calls above lifted, as an explicitly chosen way to
 * run a batch.  Above, every workgroup keeps its problem's rows of x, u and the parameter slots in LDS, so n ends at
 * cgo_batch_max_n[_obj] (10 056 … 3 352 for 0 … 4 slots).  With rows = CGO_BATCH_ROWS_DEVICE the rows stay where they are —
 * the [batch][n] rows in device memory — and every pass of the device loop streams them from there (k_batch_rows): still one
 * workgroup per problem, the same loop, hand-back and results, and every number returned has the BITS of the LDS tier (same
 * bodies, same order of every sum).  Its limits: the index type of a pass, n ≤ cgo_batch_max_n_ex(…DEVICE…) ≈ 4.29e9, and
 * the device's free memory — a batch asks for (3 + n_params) · batch · (n + n%2) · 8 bytes (x, u, the slots, the results'
 * gradient) and is refused with CGO_ENOMEM, the bytes in the message and nothing left allocated, when that exceeds what is free.
 * A pass costs a round trip to device memory where the LDS tier pays none: where n fits, LDS is the faster tier, and
 * CGO_BATCH_ROWS_AUTO takes it there and the device rows beyond.  For a run-time compiled objective the tier's kernel is a
 * third program of the module, compiled on the first call that runs this tier (cgo_batch_max_n_obj_ex compiles nothing for it).
 * A NULL policy, or rows = CGO_BATCH_ROWS_LDS, makes every _ex call the call it extends — refusals included (n >
 * cgo_batch_max_n[_obj] with that name in the message).  Any other value of rows: CGO_EINVAL. */
enum { CGO_BATCH_ROWS_LDS = 0, CGO_BATCH_ROWS_DEVICE = 1, CGO_BATCH_ROWS_AUTO = 2 };
typedef struct cgo_batch_policy {
    int32_t size;                 /* sizeof(cgo_batch_policy), written by cgo_batch_policy_init (versioning) */
    int32_t rows;                 /* CGO_BATCH_ROWS_*; default CGO_BATCH_ROWS_LDS */
    int32_t reserved[6];          /* zero */
} cgo_batch_policy;
void cgo_batch_policy_init(cgo_batch_policy *p);                                  /* every field = its default */
/* rows_used (may be NULL): the tier that ran, CGO_BATCH_ROWS_LDS or CGO_BATCH_ROWS_DEVICE */
int cgo_minimize_batch_ex(cgo_ctx *ctx, int32_t obj_kind, int64_t n, int64_t batch, const double *x0, const double *param0,
                          const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t slice_iters,
                          const cgo_batch_policy *policy, cgo_batch_results *out, int32_t *rows_used);
int cgo_minimize_batch_obj_ex(cgo_ctx *ctx, cgo_objective *model, int64_t batch, const double *x0,
                              const double *const *params, int32_t n_params,
                              const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t slice_iters,
                              const cgo_batch_policy *policy, cgo_batch_results *out, int32_t *rows_used);
int cgo_batch_open_ex(cgo_ctx *ctx, cgo_objective *model, int64_t batch, const double *const *params, int32_t n_params,
                      const cgo_batch_policy *policy, cgo_batch **handle);
int cgo_batch_rows(const cgo_batch *handle, int32_t *rows_used);                  /* the tier an open batch runs in */
/* largest n under `policy` (NULL: cgo_batch_max_n[_obj]); DEVICE and AUTO: the limit of the pass index.  0: none */
int64_t cgo_batch_max_n_ex(cgo_ctx *ctx, int32_t obj_kind, const cgo_batch_policy *policy);
int64_t cgo_batch_max_n_obj_ex(cgo_objective *model, const cgo_batch_policy *policy);
/* The streaming loop of the device-rows tier: lanes per workgroup and pairs of elements per lane and trip (needs no device). */
void cgo_batch_rows_shape(int32_t *block, int32_t *pairs_per_trip);
/* CGO_HOST_ONLY_BEGIN: declarations the run-time compiled modules do not need — csrc/gen_rtc_sources.py leaves the lines from
 * here to CGO_HOST_ONLY_END out of their text, which so stays what it was */
/* BATCHED SOLVES WITH A QUASI-NEWTON DIRECTION: β = LBFGS(m), 1 ≤ m ≤ cgo_batch_lbfgs_max_m() = 10.  Every call above is a CG
 * flavour and refuses LBFGS; this one is the batch for it — a call of its own because it allocates a ring of 2(m+1) rows per
 * problem and runs another kernel (k_batch_lbfgs): one workgroup per problem, the rows of x, u and the parameter vector and the
 * ring S, Y [batch][m+1][n + n%2] in device memory, the Gram form of the two-loop recursion on the device between a push pass
 * and a combine pass.  Arguments and results as cgo_minimize_batch; `launches` and `handed_back` keep their meaning.
 *   Objectives: CGO_OBJ_QUAD_DIAG, CGO_OBJ_ROSENBROCK_PAIRED, CGO_OBJ_BOOTH.  Line searches: StrongWolfeBisection, WolfeBisection.
 *   Device memory: (3 + K + 2(m+1)) · batch · (n + n%2) · 8 bytes (K = 1 for the quadratic, else 0), compared with what is
 *   free BEFORE anything is allocated: a batch that does not fit is CGO_ENOMEM with the bytes in the message.
 *   Hand-back: a problem whose next iteration the device loop does not run (a line-search outcome other than :success, a
 *   non-finite value, the rare-path norms, WolfeBisection's bracket collapse) is SOLVED AGAIN FROM ITS OWN x0 by one ordinary
 *   solver under the same config — it costs a whole solve, and its results and trace replace the device's.
 * CGO_EINVAL, with the reason in the message: a CG flavour or the Broyden family (those: cgo_minimize_batch), m > 10,
 * Backtracking, any other objective kind (CGO_OBJ_USER included: run-time compiled objectives, with parameter slots and a
 * scalar per problem, are cgo_minimize_batch_lbfgs_obj's, below), a multi-rank context, batch < 1,
 * n > cgo_batch_lbfgs_max_n, and what cgo_minimize_batch refuses of shapes (odd n for paired Rosenbrock, n ≠ 2 for Booth, a
 * missing param0). */
int cgo_minimize_batch_lbfgs(cgo_ctx *ctx, int32_t obj_kind, int64_t n, int64_t batch, const double *x0, const double *param0,
                             const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t slice_iters, cgo_batch_results *out);
int32_t cgo_batch_lbfgs_max_m(void);                                              /* 10 */
int64_t cgo_batch_lbfgs_max_n(cgo_ctx *ctx, int32_t obj_kind);                    /* the limit of the pass index, as cgo_batch_max_n_ex(…DEVICE…); 0: none */
void cgo_batch_lbfgs_shape(int32_t *block, int32_t *pairs_per_trip);              /* of the two ring passes; needs no device */
/* … on a RUN-TIME COMPILED objective with parameter slots: cgo_minimize_batch_obj with a quasi-Newton direction.  `model`,
 * `params` and `n_params` as there — every problem has the model's source, size, scalar and cost class and its own row of every
 * slot; `scalars`: every problem's own s0 for this solve, or NULL for the model's.  The kernel is k_batch_lbfgs<UserObjective, 3>
 * in a program of its own of the model's module, compiled on the FIRST batched L-BFGS solve on that module (seconds) and kept
 * while an objective of the same text lives.  Its two ring passes take cgo_batch_lbfgs_shape_obj(n_params) pairs per lane and
 * trip — fewer for two or more slots, which changes no bit of any result.
 *   Device memory: (3 + K + 2(m+1)) · batch · (n + n%2) · 8 bytes with K = n_params, checked against what is free before
 *   anything is allocated (CGO_ENOMEM, the bytes in the message).
 *   Hand-back: as above — the problem is solved again from its own x0 by one ordinary solver on an objective of the model's
 *   source with the problem's row of every slot and its own scalar.
 * CGO_EINVAL: what cgo_minimize_batch_obj refuses of a model and of params (a model that is not run-time compiled, of another
 * context, sharded or multi-rank; n_params other than the model's; a null params[j]), what cgo_minimize_batch_lbfgs refuses of a
 * config (a CG flavour or the Broyden family — those: cgo_minimize_batch_obj —, m > 10, Backtracking, a multi-rank context,
 * batch < 1), a scalars[b] that is not finite, n > cgo_batch_lbfgs_max_n_obj.
 * A batch that stays on the device between such solves, with an `active` mask: cgo_batch_lbfgs_open, below.
 * Not built: PROBE twins of this kernel (cgo_batch_probe's tiers 2 and 3 stay the built-in objectives'). */
int cgo_minimize_batch_lbfgs_obj(cgo_ctx *ctx, cgo_objective *model, int64_t batch, const double *x0 /* [batch*n] */,
                                 const double *const *params /* n_params × [batch*n] */, int32_t n_params,
                                 const double *scalars /* [batch] or NULL: the model's s0 for all */,
                                 const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t slice_iters, cgo_batch_results *out);
int64_t cgo_batch_lbfgs_max_n_obj(cgo_objective *model);        /* the pass-index limit; 0: none; compiles nothing */
void cgo_batch_lbfgs_shape_obj(int32_t n_params, int32_t *block, int32_t *pairs_per_trip);   /* needs no device */
/* AN LDS TIER FOR BATCHED L-BFGS: the two calls above with a cgo_batch_policy and rows_used.  Under CGO_BATCH_ROWS_LDS a
 * workgroup keeps its problem's x, u, parameter slots AND ring in LDS during a launch (k_batch_lbfgs_lds) —
 * cgo_batch_lbfgs_lds_rows(K, m) = 2 + K + 2(m+1) rows of n + n%2 doubles, loaded at entry (the ring: the stored pairs only) and
 * written back at exit if an iteration completed (the ring: the slots a push of that launch wrote).  Device memory is allocated
 * exactly as above, the ring included: launches resume from it.  Every number returned has the BITS of the device tier: the same
 * per-pair expressions, every lane's pairs in the same order into the same sums, the same reduction.
 * THE POLICY RULE DIFFERS FROM THE CG _ex CALLS ON PURPOSE, because the call these extend runs on device rows:
 *   NULL, CGO_BATCH_ROWS_DEVICE  the call it extends (k_batch_lbfgs), refusals included;
 *   CGO_BATCH_ROWS_LDS           the LDS tier; n above what one workgroup's LDS holds for this m and slot count is CGO_EINVAL,
 *                                with cgo_batch_lbfgs_max_n_ex and its value in the message;
 *   CGO_BATCH_ROWS_AUTO          DEVICE ROWS, at every n.  The rule: AUTO takes "LDS where n fits for this m and slot count" only
 *                                if the LDS tier's summed kernel time is below the device tier's by more than the device tier's
 *                                own run-to-run spread at EVERY measured shape.  It is at n = 1800, m = 3 (4.54 against 5.06 ms)
 *                                and on a two-slot objective at n = 1000, m = 5 (0.47 against 0.53 ms per launch), but not on
 *                                paired Rosenbrock at n = 1000, m = 5 (4.10 … 4.13 against 4.13 … 4.18 ms: inside the spread),
 *                                so the tier is reached by asking for it;
 *   any other value              CGO_EINVAL.
 * rows_used (may be NULL): CGO_BATCH_ROWS_LDS or CGO_BATCH_ROWS_DEVICE, the tier that ran.  For a run-time compiled objective
 * the LDS tier's kernel is one more program of the module (k_batch_lbfgs_lds<UserObjective, 3> alone), compiled on the first
 * solve of this tier on that module. */
int cgo_minimize_batch_lbfgs_ex(cgo_ctx *ctx, int32_t obj_kind, int64_t n, int64_t batch, const double *x0, const double *param0,
                                const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t slice_iters,
                                const cgo_batch_policy *policy, cgo_batch_results *out, int32_t *rows_used);
int cgo_minimize_batch_lbfgs_obj_ex(cgo_ctx *ctx, cgo_objective *model, int64_t batch, const double *x0,
                                    const double *const *params, int32_t n_params, const double *scalars,
                                    const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t slice_iters,
                                    const cgo_batch_policy *policy, cgo_batch_results *out, int32_t *rows_used);
/* largest n under `policy` for ring depth m: LDS — what one workgroup's LDS holds (the device's bytes per block minus the kernel's
 * static LDS and 512 bytes of slack, over 8 · cgo_batch_lbfgs_lds_rows, down to even); DEVICE, AUTO, NULL — the pass-index limit.
 * 0: no context, kind or model, or m outside 1 … 10.  The _obj form under LDS compiles the module's program of the tier if it
 * is not there, as cgo_batch_max_n_obj compiles the batch program; under the other policies it compiles nothing. */
int64_t cgo_batch_lbfgs_max_n_ex(cgo_ctx *ctx, int32_t obj_kind, int32_t m, const cgo_batch_policy *policy);
int64_t cgo_batch_lbfgs_max_n_obj_ex(cgo_objective *model, int32_t m, const cgo_batch_policy *policy);
int32_t cgo_batch_lbfgs_lds_rows(int32_t n_params, int32_t m);   /* 2 + K + 2(m+1); 0 for K outside 0 … 4 or m outside 1 … 10; needs no device */
void cgo_batch_lbfgs_lds_shape(int32_t n_params, int32_t *block, int32_t *pairs_per_trip);   /* of the two ring passes over LDS; needs no device */
/* A BATCH THAT STAYS ON THE DEVICE between L-BFGS solves: cgo_batch_open / cgo_batch_solve for β = LBFGS(m).  The handle is a
 * cgo_batch — cgo_batch_close and cgo_batch_rows serve both kinds — but the two kinds do not mix: cgo_batch_solve on a handle
 * opened here, and cgo_batch_lbfgs_solve on a handle of cgo_batch_open[_ex], are CGO_EINVAL with the other call's name in the message.
 *   open   allocates what cgo_minimize_batch_lbfgs_obj_ex allocates for ring depth m_max (1 … cgo_batch_lbfgs_max_m(), else
 *          CGO_EINVAL) — x, u, the gradient row, the K slot rows (uploaded here, once: `params` is not read afterwards) and 2(m_max+1)
 *          ring rows per problem, checked against the free device memory before anything is allocated (CGO_ENOMEM, the bytes in the
 *          message, nothing left allocated) — and compiles the tier's program of the model's module, so that a solve never compiles.
 *          policy: the L-BFGS rule above (NULL / DEVICE: device rows; LDS: the LDS tier, refused with CGO_EINVAL above
 *          cgo_batch_lbfgs_max_n_obj_ex(model, m_max, policy), that name and its value in the message; AUTO: device rows).  It
 *          refuses what cgo_minimize_batch_lbfgs_obj_ex refuses of a model, params, batch, n, policy and context; the handle holds
 *          a reference on the model, whose scalar and cost class are read at every solve.
 *   solve  cfg->beta must be LBFGS(m) with 1 ≤ m ≤ m_max (a larger m: CGO_EINVAL naming both; a CG flavour or Broyden: CGO_EINVAL
 *          pointing to cgo_batch_solve; Backtracking refused as in the one-shot call); x0, scalars and active as cgo_batch_solve
 *          has them, refusals included.  Every solve starts every ring EMPTY with this solve's m: nothing of an earlier solve is
 *          read, the ring keeps the stride of m_max, and the LDS tier launches with the dynamic LDS of m_max.  Every number
 *          returned has the BITS of cgo_minimize_batch_lbfgs_obj_ex with the same inputs, tier and m.  After a refusal the
 *          handle is what it was.
 *   Hand-back: as in the one-shot call the problem is solved again from its own row of this solve's x0 by one ordinary solver,
 *          under its own scalar where the solve has them, else the model's; its slot rows are copied device to device from the
 *          handle's rows.  (The ring is not exported: a handed-back problem does not resume where it stands.)
 *   cgo_batch_lbfgs_m: the m_max a handle was opened with; 0 for a handle of cgo_batch_open[_ex]. */
int cgo_batch_lbfgs_open(cgo_ctx *ctx, cgo_objective *model, int64_t batch, const double *const *params, int32_t n_params,
                         int32_t m_max, const cgo_batch_policy *policy /* NULL: device rows */, cgo_batch **handle);
int cgo_batch_lbfgs_solve(cgo_batch *handle, const double *x0 /* [batch*n] */, const double *scalars /* [batch] or NULL */,
                          const unsigned char *active /* [batch] or NULL */, const cgo_cg_config *cfg, const cgo_ls_config *ls,
                          int64_t slice_iters /* 0 = library policy */, cgo_batch_results *out);
int cgo_batch_lbfgs_m(const cgo_batch *handle, int32_t *m_max);
/* A scripted sequence of passes of a BATCHED solve in ONE launch, a workgroup per problem, on host vectors — for tests that check
 * every slot of every pass in EVERY workgroup (tests/test_batch_kernel_sums.py).  The batch is allocated as a solve allocates it
 * and the launch arguments are filled by the code that fills them for a solve (ld, the slot pointers, s0 / s0v, the ring stride,
 * the record stride); the kernel is the product kernel instantiated with its PROBE flag: in place of the scalar loop
 * (res_iterate / res_iterate_qn) it runs pass[0..npass) through the member functions that loop calls —
 *   tier 0  k_batch        rows in LDS                 tier 1  k_batch_rows   rows streamed from device memory
 *   tier 2  k_batch_lbfgs  tier 1 with the ring S, Y [batch][m+1][ld] and a quasi-Newton state per problem
 *   tier 3  k_batch_lbfgs_lds  tier 2 with the rows and the ring in LDS during the launch: same inputs, outputs and kinds
 *   kind 0  trial(a, k, out)                              1 ≤ k ≤ 3                     tiers 0, 1, 2, 3
 *   kind 1  accept_dir_trial(a_acc, beta, a, k, …)        0 ≤ k ≤ 3                     tiers 0, 1
 *   kind 2  pass<R_INIT, 1>                               u = −g, f, g·g                tiers 0, 1, 2, 3
 *   kind 3  push_update(a_acc)                            x ← x + a_acc·u, the pair into the free slot, the scalar recursion   tiers 2, 3
 *   kind 4  combine_trial(a, k, …)                        0 ≤ k ≤ 3                     tiers 2, 3
 * — a[k..) repeating a[k − 1] as the loops pad them (done here).  A combine runs on the coefficients the last push of the script
 * left, or (co_set) on count = co_count, γ = co_gamma, co_cy, co_cs, written into the workgroup's coefficient block; a combine
 * with neither is refused.  An accepting pass or a push counts as a completed iteration, so tier 0 writes its rows back as after
 * a slice that completed one; a script without one leaves them alone.
 * In: obj_kind (a built-in kind; tiers 0, 1, 2, 3) or model (a run-time compiled objective, obj_kind = CGO_OBJ_USER; tiers 0, 1 —
 * its PROBE kernels are one more program of its module, compiled on the first probe); x, u [batch][n]; params[j] [batch][n] for
 * every slot the objective reads; scalars [batch] or NULL (tiers 0, 1; a model only); skip [batch] or NULL — a flagged problem
 * is preset finished (RES_STOP) and its workgroup returns at once; tiers 2, 3: m, S and Y [batch][m+1][n] (an absent slot: NaN rows)
 * and qn, every problem's QnState (csrc/cgo_qn.hpp) as cgo_batch_probe_qn_bytes() bytes each — list, count and free_slot are
 * checked against m here, before any of them indexes the ring.
 * Out (each pointer may be NULL): rows [npass][batch][64] — the row every workgroup holds after that pass, out[…].width slots of
 * it (64 after a push), the rest still the NaN pattern 0x7FF87FF87FF87FF8 the buffer starts with; out [npass][batch] what the
 * member function returned there (stored: push_update's pair count; for a combine the count it ran on); x_out, u_out, g_out
 * [batch][ld] and S_out, Y_out [batch][m+1][ld] with ld = n + n%2, i.e. WITH the padding element of an odd n, which is uploaded as
 * the NaN pattern in every row; g_out = the results' gradient formed after the script by the backend's own path (k_batch_grad with
 * scalars — which leaves the padding element alone — else the gradient launch over the concatenated rows, which evaluates it);
 * qn_out; reason, done, passes [batch] of every ResState; points, ld; symbol, e.g. "k_batch_rows<ObjQuadDiag, 3, true>".
 * Every device buffer of the batch carries NaN slack behind its used part (rows, parameter slots, ring, states, quasi-Newton
 * states, scalars, the probe's own rows), checked after the launch: CGO_ESTATE if a word of it changed, or if a problem that
 * was not skipped ran another number of passes.  CGO_EINVAL: a kind the tier's loop never issues, k beyond the instantiation's
 * points, more than 32 passes, a multi-rank context, and what the solve of that tier refuses of objectives and sizes
 * (n > cgo_batch_max_n* of the tier); CGO_ENOMEM as the solve. */
#define CGO_BATCH_PROBE_MAX_PASSES 32
typedef struct cgo_batch_pass {
    int32_t kind, k;
    double a[7];
    double a_acc, beta;
    int32_t co_set, co_count;
    double co_gamma, co_cy[10], co_cs[10];
} cgo_batch_pass;
typedef struct cgo_batch_pass_out {
    double ts[7][7];          /* per point: f, gtu, gtgt, gtg, yy, uy, ygt */
    double gu, uu;
    int64_t width, stored;
} cgo_batch_pass_out;
typedef struct cgo_batch_probe_args {
    int32_t tier, obj_kind, m, n_params;
    cgo_objective *model;
    int64_t n, batch;
    const double *x, *u;
    const double *params[4];
    const double *scalars;
    const unsigned char *skip;
    const double *S, *Y;
    const void *qn;
    int32_t npass, reserved;
    cgo_batch_pass pass[CGO_BATCH_PROBE_MAX_PASSES];
    /* out */
    double *rows;
    cgo_batch_pass_out *out;
    double *x_out, *u_out, *g_out, *S_out, *Y_out;
    void *qn_out;
    int32_t *reason;
    int64_t *done, *passes;
    int32_t points, reserved2;
    int64_t ld;
    char symbol[128];
} cgo_batch_probe_args;
int cgo_batch_probe(cgo_ctx *ctx, cgo_batch_probe_args *p);
int64_t cgo_batch_probe_qn_bytes(void);                                           /* sizeof(QnState): what a mirror of it must measure */
/* Predicted path.  For an objective with a constant Hessian the curvature along the NEXT direction is known
 * before the launch that forms it — from sums the accepting launch returns plus one more, g⁺ᵀH g⁺ — and the line search run over
 * the parabola ϕ(a) = f + a·dϕ₀ + ½a²·c lists the steps the real search will ask for.  With prediction on, launches N and S of the
 * replay cycle run as path launches ("k_cg_path<Obj, mode, NACT, true>" in the reported symbol) wherever they would run their lean rows:
 * the 7-point row with only the first NACT points evaluated — the steps of the predicted path that the seven-point tree holds —
 * the other points' slots +0.0, g⁺ᵀH g⁺ in the slot of y·y.  An evaluated point has the bits the seven-point launch gives it and
 * every decision is taken on sums a launch formed, so a solve returns what it returns with prediction off, bit for bit; a search
 * that asks for a step of the tree the launch left out gets the whole tree from one trial launch (counted as a miss).  Kernel
 * kinds and bytes per launch are unchanged.  It takes effect for the separable quadratic, Polak–Ribière and StrongWolfeBisection or
 * WolfeBisection with the Wolfe conditions; any other solver keeps its rows whatever is asked.  Library policy: on exactly where
 * lean sums are on by the library's own default; env CGO_PATH_PREDICT=0|1 forces the switch; this call has the last word for one
 * solver and takes effect at the next launch. */
int cgo_solver_set_path_prediction(cgo_solver *s, int32_t on);
/* by_nact[8]: path launches by points evaluated (index 1 … 5, 7); predicted / tree: launches that evaluated a predicted path / the
 * whole tree on a path row; misses: line searches answered by a trial launch of the tree.  Any pointer may be null. */
int cgo_solver_path_stats(cgo_solver *s, int64_t *by_nact, int64_t *predicted, int64_t *tree, int64_t *misses);
/* The NEXT cgo_solver_probe_launch of a lean row (launch N or S of the replay cycle, variant with the R_NO… bits) runs as its path
 * twin k_cg_path<Obj, mode, nact, true> (cgo_solver_set_path_prediction): nact = 1 … 5 or 7 active points, at most nact trial steps.
 * 0 takes the request back.  Asked once per launch. */
int cgo_solver_probe_set_path(cgo_solver *s, int32_t nact);
/* Tests only: a factor on the curvature of the predicted path's model (1.0: the model as it is), so that predictions go wrong. */
int cgo_solver_debug_set_path_skew(cgo_solver *s, double factor);
/* CGO_HOST_ONLY_END */
/* The stop test at the top of iteration it + 1 (optim.jl:53-80,162-169) as a function of the loop state — the one rule the
 * engine and the problems a batch finishes on the device share: the terminal status (CGO_INCOMPLETE: the iteration runs) and
 * Results.iters_ran. */
int32_t cgo_stop_status(int64_t it, int64_t max_iters, double f_x, double grad_norm, double eps, double f_x0, int64_t *iters_ran);

/* ---- kernel-level entry points on host vectors (KATs / micro-benchmarks)
 *      each: H2D, ONE fused launch, D2H ---------------------------------- */
/* updatedir!(u, df_x, β) (cg_flavours.jl:2-15) fused with the next dϕ₀ = g·u
 * (nocedal.jl:56, wolfe.jl:40) and u·u (wolfe.jl:240): out2 = {g·u_new, u_new·u_new} */
int cgo_kernel_dir(cgo_ctx *ctx, double *u, const double *g, double beta, int64_t n,
                   double *out2);
/* one-pass partial sums for getβ (cg_flavours.jl:46-170):
 * out9 = {g⁺·u, g⁺·g⁺, g⁺·g, y·y, u·y, y·g⁺, g·g, g·u, u·u}, y = g⁺ − g */
int cgo_kernel_beta_partials(cgo_ctx *ctx, const double *g_next, const double *g,
                             const double *u, int64_t n, double *out9);
/* getβ(β_config, g_next, g, u)::T evaluated from those partials (scalar work) */
int cgo_getbeta(cgo_ctx *ctx, const cgo_beta_config *b, const double *g_next, const double *g,
                const double *u, int64_t n, double *beta);
/* evalϕdϕ!(xp, df_xp, fdf!, a, x, u) (cg_utils.jl:4-23): out2 = {ϕ, dϕ}; g_next_out = df_xp */
int cgo_kernel_trial(cgo_objective *obj, const double *x, const double *u, double a,
                     double *g_next_out, double *out2);
/* ONE launch of the solver's gradient-free family (k_cg / k_chain; the log-sum-exp objective: k_lse_stats / k_lse_grad) on
 * host vectors, for tests that check every slot of a launch's reduced row.  x, u and aux (n_local doubles each) go into the
 * solver's own device state and the launch goes through the engine's own path: the solver's resolved policy and its context's
 * tail setting pick the instantiation (points, pure-HBM or not, reduction tail).  `kernel_kind` is a KK kind the engine
 * issues such launches for, `variant` its mode bits (0: the kind's usual mode):
 *   init: R_INIT 8 | R_GRAD 64 | R_EDGES 512 (stencil)   trial: R_TRIAL 4   accept_dir_trial: 7   accept_dir: 3   accept_only: 1
 *   reset_dir: 16   upg_norm: 32   dir_trial: R_DIR 2 | R_DIR|R_TRIAL 6   sys_project: R_PROJ 256   scaled_norm: R_GRAD | R_GRADT 128
 *   lse_stats: 0 (trial at a[0]) | 4 (at x itself) | 3 (accept a_acc + direction β, then the trial)
 *   lse_grad: 0 (g⁺ at a[0]) | 1 (+ the getβ sums) | 2 (initial: at x, u = −g); the (max, Σ) are those the last lse_stats
 *             probe of this solver left, as in the engine.
 * a[0..k) are the trial steps (k ≤ 7; a launch for more points than k repeats a[k−1]).  u may be NULL where the mode does not
 * read it, aux is solvesystem's x2 (sys_project) or the stored gradient (lse_stats 3, lse_grad 1), else NULL; what is NULL
 * reaches the device as NaN.  Out: the WHOLE reduced row (padding points and padding slots included; sums_len = its width,
 * 0 for a mode without sums), x / u after the launch, g_out = the gradient the mode wrote (x2 for sys_project); any of them
 * may be NULL.  symbol = the instantiation, as cgo_solver_kernel_symbol prints it (the log-sum-exp kernels with their template
 * arguments).  The first probe re-allocates the solver's buffers to whole 128-B lines plus one line with NaN behind n_local
 * (the objective's parameter vector too, contents kept) and checks after every launch that that slack is untouched
 * (CGO_ESTATE otherwise): a probed solver is for probing only — cgo_solver_start / cgo_solver_iterate refuse it.  The
 * parameter vector is the OBJECTIVE's: its old buffer is freed, so the objective of a probed solver must not be shared with
 * another solver in use (one that has started, or keeps a captured graph or a resident slice on it).
 * CGO_EINVAL for every other kind (the L-BFGS passes: cgo_solver_probe_lbfgs; the resident solver: cgo_solver_probe_resident;
 * armed rounds — the on-device controller's finisher, k_cg_armed and k_finalize_ctl — cgo_solver_probe_armed).
 *
 * A solver of the stored-gradient family (k_fused: β = LBFGS(m) on an element-wise objective, a host-closure objective,
 * policy.stored_gradient) is probed through the same entry point, single rank only, one trial step (k = 1) where the kind
 * takes one.  `variant` holds M_* bits (0: the kind's usual mode):
 *   init: M_INIT 16   trial: M_TRIAL 4 | M_TRIAL|M_BETA 12   accept_dir_trial: 15   accept_dir: 3   accept_only: 1
 *   reset_dir: M_RESET 32   upg_norm: M_UPG 64
 *   scaled_norm: variant = which, 0 g | 1 g⁺ | 3 u | 4 g⁺ − g: k_scaled_norm<0>, then k_scaled_norm<1> unless the first pass
 *             found a NaN, a zero vector or an infinity.  sums = the pass-0 row {max|v|, #NaN, 0 …} followed by the pass-1
 *             row {Σ (v/max)², 0 …} when that pass ran: sums_len = 20 or 10.  For which = 1 and 4, g⁺ is passed in `x`
 *             (no norm pass reads x, which reaches the device as NaN then).
 *   host-closure objective: init and trial (variant 0 or M_BETAONLY 128) run k_trial_point → the closure → k_fused<…, 128>,
 *             whose S_F slot carries the closure's f; init zeroes g and u first and is followed by the reset launch
 *             (k_fused<…, 32>, u = −g), its row appended (sums_len = 20).  accept_dir_trial (variant 0 or 3) runs accept_dir,
 *             then the trial: rows of k_fused<…, 3> and k_fused<…, 128>.
 * aux is the vector the launch reads as the stored gradient g (the accepting kinds swap g and g⁺ before they launch: aux
 * lands where that swap puts g).  g_out is the buffer that holds g⁺ after the call — what the launch wrote, what the
 * closure returned, NaN where the mode writes no g⁺; after a host-closure init it is the zeroed former g, the closure's
 * gradient having become g.  symbol joins the instantiations launched with " + ", e.g.
 * "k_trial_point + k_fused<ObjQuadDiag, 128, false>" or "k_scaled_norm<0> + k_scaled_norm<1>" (the objective-free modes
 * are instantiated for ObjQuadDiag only).  Multi-rank solvers are refused (CGO_EINVAL). */
/* The lazy-direction instantiations (pure-HBM form only, built-in objectives) are probed through cgo_solver_probe_launch too:
 *   accept_dir_trial: R_ULAG|7 = 1031   accept_trial_lazy: 7|R_NOWU = 2055   trial: R_ULAG|R_TRIAL = 1028   materialize_u: R_ULAG 1024
 * R_ULAG rebuilds u ← −∇f(x) + β_prev·u on load; β_prev is what this call set last (0 until then). */
int cgo_solver_probe_set_beta_prev(cgo_solver *s, double beta_prev);
/* The replay instantiations likewise (R_REPLAY = 4096, R_NOWX = 8192):
 *   accept_trial_nostore: 4096|7|2048|8192 = 14343   accept_dir_trial: 4096|7 = 4103   trial: 4096|4 = 4100   materialize_xu: 4096
 * R_REPLAY does, on load, for j < nrep: x ← x + a[j]·u ; u ← −∇f(x) + beta[j]·u.  The list is what this call set last (empty
 * until then; 0 ≤ nrep ≤ 15: more than 7 for a path row (cgo_solver_probe_set_path) and for "trial", which then runs as
 * "k_cg_trial_deep<Obj, NPTS, true>" — cgo_solver_probe_launch refuses a longer list for any other launch).
 * cgo_solver_probe_set_deep_trial(s, 1): the NEXT probe of "trial" with variant 4100 runs as k_cg_trial_deep whatever the list.
 * Lean N and S (Polak–Ribière's mask 16384|32768|65536 = 114688 or-ed in): accept_trial_nostore 129031, accept_dir_trial 118791. */
int cgo_solver_probe_set_replay(cgo_solver *s, int32_t nrep, const double *a, const double *beta);
int cgo_solver_probe_set_deep_trial(cgo_solver *s, int32_t on);
int cgo_solver_probe_launch(cgo_solver *s, int32_t kernel_kind, int32_t variant, double a_acc, double beta,
                            const double *a, int32_t k,
                            const double *x, const double *u, const double *aux,
                            double *sums, int32_t sums_cap, int32_t *sums_len,
                            double *x_out, double *u_out, double *g_out,
                            char *symbol, int32_t symbol_cap);
/* ONE L-BFGS pass of a single-rank solver whose β is LBFGS(m), on host vectors (cgo_solver_probe_lbfgs), through the backend's
 * own entry point for that pass, so that the engine picks the instantiation, grid and streaming path:
 *   0 push              lbfgs_push (k_lbfgs_push): a, a_s, slot
 *   1 push_gram         lbfgs_push_gram (k_lbfgs_push_gram, or k_lbfgs_push_gram_lse where the engine fuses g⁺ into the push:
 *                       the log-sum-exp objective, M, S = the accepted trial's statistics, out of place into xo_out)
 *   2 direction_gram    lbfgs_direction_gram (k_lbfgs_combine): list, count, cg, cy, cs
 *   3 direction_trial   lbfgs_direction_gram_trial (k_lbfgs_combine_lse, or k_lbfgs_combine_spec where the one-pass form is on;
 *                       M, S = the iterate's statistics; deferred_push: the state update of a_lite, a_s_lite, M_lite, S_lite
 *                       into lite_slot rides along — new_in_list is the engine's own decision, list[0] == lite_slot, and out)
 *                       then, with spec_check, lbfgs_push_spec(spec_a_x, spec_a_s, spec_slot, spec_list, spec_count): spec_ok
 *                       and gram = {sy, yy, sgn, ygn, gtgt, then per pair j: sjg, yjg, sjyn, yjsn, yjyn}
 *   4 push_lite         lbfgs_push_lite (k_lbfgs_push_lite): a, a_s, slot, M, S
 *   5 loop              ONE k_lbfgs_loop launch: loop_mode (0 loop 1, 1 loop 2, 2 dot only), final_step, apply_scale, k, rho,
 *                       scale; q from g (q_from_g) or u, out to u; v and w are ring vectors (ring 0 S, 1 Y) or g (ring 2);
 *                       the dot from dot_host (dot_count 0) or summed over dot_count rows of 10 (dots, rank order) on the
 *                       device; alpha[64] is the device α vector before (in) and after (out) the launch.
 * x, u, g (the stored gradient), gt (g⁺) hold n_local doubles, S and Y the whole rings: m + 1 slots of n_local, slot-major;
 * what is NULL reaches the device as NaN (an absent ring slot: NaN rows).  Out (each may be NULL): the vectors and both rings
 * after the launch; sums / sums_len the whole reduced row of the pass's last reducing launch (padding slots included);
 * symbol every instantiation launched, in order, joined by " + ".  As cgo_solver_probe_launch, the first probe gives every
 * vector NaN slack, the rings too (the ring_ld padding behind every slot and one line behind the last), and every launch is
 * checked not to have written into it (CGO_ESTATE): a probed solver is for probing only.  CGO_EINVAL for a solver that is
 * not single-rank L-BFGS, and for a pass its engine would not issue. */
typedef struct cgo_lbfgs_probe {
    int32_t pass, slot, count, list[16];
    double a, a_s, a_trial, cg, M, S;
    double cy[16], cs[16];
    int32_t deferred_push, lite_slot;
    double a_lite, a_s_lite, M_lite, S_lite;
    int32_t loop_mode, final_step, apply_scale, k, q_from_g, v_ring, v_slot, w_ring, w_slot, dot_count;
    double rho, scale, dot_host;
    const double *dots;
    double alpha[64];
    int32_t spec_check, spec_slot, spec_count, spec_list[16];
    double spec_a_x, spec_a_s;
    int32_t spec_ok, new_in_list, sums_len, reserved;   /* out */
    double gram[85];                                     /* out */
    double sums[64];                                     /* out */
    char symbol[256];                                    /* out */
} cgo_lbfgs_probe;
int cgo_solver_probe_lbfgs(cgo_solver *s, cgo_lbfgs_probe *p,
                           const double *x, const double *u, const double *g, const double *gt, const double *S, const double *Y,
                           double *x_out, double *xo_out, double *u_out, double *g_out, double *gt_out, double *S_out, double *Y_out);
/* A scripted sequence of passes of the RESIDENT solver (k_resident / k_resident_chain) in ONE launch, on host vectors, for
 * tests that check every slot of every pass in EVERY workgroup.  The launch is the engine's own: its plan (grid, chunk, LDS
 * bytes, points per pass from SolverPolicy.resident_chunk / resident_points), its exchange buffers, the out-of-place write-back
 * and its swap, and the exchange round carried from one launch to the next — two probes in a row continue the buffer rotation
 * where the first stopped.  The kernel is the product kernel instantiated with its PROBE flag: in place of the scalar loop
 * (res_iterate) it runs pass[0..npass) through the member functions that loop calls —
 *   kind 0  trial(a, k, out)                               1 ≤ k ≤ min(points, 3)
 *   kind 1  accept_dir_trial(a_acc, beta, a, k, out, gu, uu)   0 ≤ k ≤ points
 * — with a[k..) repeating a[k − 1] as the loop pads them (done here, the caller fills a[0..k)).  An accepting pass counts as a
 * completed iteration: x, u are written back and swapped in as after a good slice; a script of trials leaves them alone.
 * Out: rows[pass][workgroup][56] = the totals every workgroup holds after that pass (out[pass].width slots, the padding
 * slots of a row included; what lies behind the width is left as it was), rows_cap its capacity in doubles
 * (≥ npass · grid · 56; npass · 256 · 56 always suffices); out[pass] what the member function returned in workgroup 0;
 * grid, chunk, points, round0 (the exchange round the launch started at); x_out / u_out (may be NULL) what the next slice
 * would read; symbol the instantiation.  As with cgo_solver_probe_launch the first probe gives x, u, their out-of-place
 * partners and the parameter vector NaN slack, checked after every launch (CGO_ESTATE), and the solver is for probing only.
 * CGO_EINVAL where the engine would not run the resident solver (objective, β, line search, size, policy) and for a pass it
 * cannot issue.  If a workgroup's bounded poll gives up: CGO_ESTATE, err_word = the launch's error word — nothing is retried. */
#define CGO_RESIDENT_PROBE_MAX_PASSES 32
typedef struct cgo_resident_pass {
    int32_t kind, k;
    double a[7];
    double a_acc, beta;
} cgo_resident_pass;
typedef struct cgo_resident_pass_out {
    double ts[7][7];          /* per point: f, gtu, gtgt, gtg, yy, uy, ygt */
    double gu, uu;
    int64_t width;
} cgo_resident_pass_out;
typedef struct cgo_resident_probe {
    int32_t npass, reserved;
    cgo_resident_pass pass[CGO_RESIDENT_PROBE_MAX_PASSES];
    /* out */
    int32_t grid, points;
    int64_t chunk, round0;
    uint32_t err_word;
    int32_t wrote_back;
    cgo_resident_pass_out out[CGO_RESIDENT_PROBE_MAX_PASSES];
    char symbol[128];
} cgo_resident_probe;
int cgo_solver_probe_resident(cgo_solver *s, cgo_resident_probe *p, const double *x, const double *u,
                              double *rows, int64_t rows_cap, double *x_out, double *u_out);
/* A batch of CONTROLLER-ARMED rounds (csrc/cgo_ctl.hpp) of a single-rank solver on host vectors, through the
 * engine's own path: k_ctl_init writes the device block from `st` and the solver's configuration (line search, β kind, μ and the
 * row layout — trial points per launch — are the solver's; max_iters, and eps where use_eps is set, are given here), the rounds
 * are enqueued as the engine enqueues them, and every record is awaited with the engine's bounded wait.  The solver's policy
 * and its context's tail setting pick the form of a round: ONE launch (k_cg_armed, whose finisher runs the controller) where
 * the fused tail applies, else k_cg reading its scalars from the device block + k_finalize_t above 64 rows + k_finalize_ctl.
 *   form 0  rounds launched one by one
 *        1  as captured graphs, the engine's own split into batches of 8, 4 and 2 rounds (a remaining round goes by itself)
 *        2  the controller alone: `row` is placed as a single row of partials and k_finalize_ctl<width> is launched on it,
 *           rounds = 1, no vector is read or written (x, u may be NULL) — for sums no vector data produces on demand
 * 1 ≤ rounds ≤ CGO_ARMED_PROBE_MAX_ROUNDS.  The three structs below are the controller's own (CtlState, CtlArgs, CtlRecord),
 * word for word.  Out: rec[0..rounds) whole; st_out, args_out, round_out = the device block after the last round (round
 * counts on from probe to probe); out_dev = the device copy of the last reduced row (width slots, +0.0 behind them); x_out /
 * u_out (may be NULL) the vectors after the last round; symbol = every instantiation launched, in order, joined by " + ", e.g.
 * "k_cg_armed<ObjQuadDiag, 7>" or "k_cg<ObjBooth, 7, 3, false> + k_finalize_ctl<24>".  As with cgo_solver_probe_launch the
 * first probe gives every buffer NaN slack, every call checks it and drains the controller's pipe before it returns, and the
 * solver is for probing only.  A record that does not validate, or the bounded wait running out: CGO_ESTATE, never a hang.
 * CGO_EINVAL where the engine would arm no round (controller depth 0: multi-rank without device mailboxes, two-phase and
 * stencil objectives, the stored-gradient family), for a multi-rank solver, and for bad arguments. */
#define CGO_ARMED_PROBE_MAX_ROUNDS 32
typedef struct cgo_ctl_state {
    double f_x, gg, a_acc, beta, a[7];
    int32_t npts, go;
    int64_t it;
} cgo_ctl_state;
typedef struct cgo_ctl_args {
    double a_acc, beta, a[7];
    int64_t go;
} cgo_ctl_args;
typedef struct cgo_ctl_record {
    double sums[56], a_acc, beta, a[7];
    int32_t npts, accepted;
    int64_t xwait;
} cgo_ctl_record;
typedef struct cgo_armed_probe {
    int32_t rounds, form, use_eps, reserved;
    int64_t max_iters;
    double eps;
    cgo_ctl_state st;
    double row[56];                                       /* form 2 */
    /* out */
    int32_t width, maxp;
    uint64_t round_out;
    cgo_ctl_state st_out;
    cgo_ctl_args args_out;
    double out_dev[56];
    cgo_ctl_record rec[CGO_ARMED_PROBE_MAX_ROUNDS];
    char symbol[4096];
} cgo_armed_probe;
int cgo_solver_probe_armed(cgo_solver *s, cgo_armed_probe *p, const double *x, const double *u, double *x_out, double *u_out);
/* device-resident micro-benchmark of the fused kernels: allocates vectors of
 * n doubles on the ctx, runs `reps` launches of `kernel_kind`, returns the mean
 * HIP-event time per launch (ms) and the algorithmic bytes per launch */
int cgo_bench_kernel(cgo_ctx *ctx, cgo_objective *obj, int32_t kernel_kind, int64_t n,
                     int32_t reps, double *ms_per_launch, double *bytes_per_launch);

/* What the box at hand delivers for the READ/WRITE MIX of the dominant launch (accept + direction + trial: R x, u, D /
 * W x, u in place, 40 B per element) with next to no arithmetic, under the engine's pure-HBM streaming policy: median
 * and best HIP-event time of `reps` launches on n doubles per vector.  bench.py reports the engine's launch against this
 * measured ceiling beside the 8 TB/s pin peak. */
int cgo_bench_stream_mix(cgo_ctx *ctx, int64_t n, int32_t reps, double *median_us, double *best_us);
/* Placement search of a solver on a pure-HBM problem size: the time of that bare mix on the buffers as
 * first allocated, on the triple (x, u, D) the solver kept, and how many candidate triples were timed (0 = no search:
 * problem below the pure-HBM threshold, CGO_PLACE_TUNE=0, not enough free memory for the spare buffers, or an objective
 * with more than one parameter slot: the mix that is timed has the three streams x, u, D). */
int cgo_solver_placement_info(cgo_solver *s, double *as_allocated_us, double *chosen_us, int32_t *candidates);

#ifdef __cplusplus
}
#endif
#endif /* CGO_H */
