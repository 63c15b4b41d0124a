// Test double for the batched L-BFGS solves (GPU-less): the PRODUCT's device loop res_iterate_qn (csrc/cgo_resident_qn.hpp) and
// its scalar recursion (csrc/cgo_qn.hpp) over plain loops — one problem, the vectors in host memory, sums in index order.
// tests/test_batch_lbfgs_abi.py compiles this file itself and holds it to the oracle.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../conjugategradientoptim.jl_amd/csrc/cgo_resident_qn.hpp"

using namespace cgo;

namespace {

struct PlainQn {
    static constexpr int kNpts = 3;
    static constexpr bool kZeroCheck = true;
    int kind; int64_t n; const double *D;
    std::vector<double> x, u, S, Y, g, gt, xp;   // S, Y: [m+1][n]
    QnState q; QnCoef co;

    bool leader() const { return true; }
    long long clock() const { return 0; }

    double fg(const double *xv, double *gv) const {   // the objectives as the kernels state them (csrc/cgo_kernels.hip.hpp)
        double f = 0.0;
        if (kind == CGO_OBJ_QUAD_DIAG) {
            for (int64_t i = 0; i < n; ++i) { gv[i] = D[i] * xv[i]; f += 0.5 * (gv[i] * xv[i]); }
        } else if (kind == CGO_OBJ_ROSENBROCK_PAIRED) {
            for (int64_t i = 0; i + 1 < n; i += 2) {
                const double t1 = xv[i + 1] - xv[i] * xv[i], t2 = 1.0 - xv[i];
                f += 100.0 * (t1 * t1) + t2 * t2;
                gv[i] = -400.0 * (xv[i] * t1) - 2.0 * t2;
                gv[i + 1] = 200.0 * t1;
            }
        } else {   // Booth
            const double t1 = xv[0] + 2 * xv[1] - 7, t2 = 2 * xv[0] + xv[1] - 5;
            f += t1 * t1 + t2 * t2;
            gv[0] = 2 * t1 + 2 * t2 * 2;
            gv[1] = 2 * t1 * 2 + 2 * t2;
        }
        return f;
    }
    static double dot(const double *a, const double *b, int64_t n) { double s = 0.0; for (int64_t i = 0; i < n; ++i) s += a[i] * b[i]; return s; }

    void trial_sums(double a, TrialSums &o) {   // g holds ∇f(x)
        for (int64_t i = 0; i < n; ++i) xp[i] = x[i] + a * u[i];
        o.f = fg(xp.data(), gt.data());
        o.gtu = dot(gt.data(), u.data(), n); o.gtgt = dot(gt.data(), gt.data(), n); o.gtg = dot(gt.data(), g.data(), n);
        double yy = 0, uy = 0, ygt = 0;
        for (int64_t i = 0; i < n; ++i) { const double y = gt[i] - g[i]; yy += y * y; uy += u[i] * y; ygt += y * gt[i]; }
        o.yy = yy; o.uy = uy; o.ygt = ygt;
    }
    int trial(const double *a, int k, TrialSums *out) {
        fg(x.data(), g.data());
        for (int j = 0; j < 3; ++j) trial_sums(a[j], out[j]);
        (void)k;
        return 0;
    }
    bool trial_gradient_is_zero(double a) {
        for (int64_t i = 0; i < n; ++i) xp[i] = x[i] + a * u[i];
        fg(xp.data(), gt.data());
        for (int64_t i = 0; i < n; ++i) if (gt[i] != 0.0) return false;
        return true;
    }
    int push_update(double a) {
        double sums[QN_SUMS] = {};
        double *s = S.data() + (size_t)q.free_slot * n, *y = Y.data() + (size_t)q.free_slot * n;
        fg(x.data(), g.data());
        for (int64_t i = 0; i < n; ++i) { s[i] = a * u[i]; xp[i] = x[i] + s[i]; }
        fg(xp.data(), gt.data());
        for (int64_t i = 0; i < n; ++i) { y[i] = gt[i] - g[i]; x[i] = xp[i]; }
        sums[QS_SY] = dot(s, y, n); sums[QS_YY] = dot(y, y, n); sums[QS_SGN] = dot(s, gt.data(), n); sums[QS_YGN] = dot(y, gt.data(), n);
        for (int j = 0; j < q.count; ++j) {
            const double *sj = S.data() + (size_t)q.list[j] * n, *yj = Y.data() + (size_t)q.list[j] * n;
            double *t = sums + QS_PAIR0 + QP_PER_PAIR * j;
            t[QP_SJG] = dot(sj, gt.data(), n); t[QP_YJG] = dot(yj, gt.data(), n);
            t[QP_SJYN] = dot(sj, y, n); t[QP_YJSN] = dot(yj, s, n); t[QP_YJYN] = dot(yj, y, n);
        }
        qn_update(q, sums);
        qn_coefficients(q, co);
        return co.count;
    }
    int combine_trial(const double *a, int k, TrialSums *out, double &gu, double &uu) {
        fg(x.data(), g.data());
        for (int64_t i = 0; i < n; ++i) {
            double v = -co.gamma * g[i];
            for (int j = 0; j < co.count; ++j) v = v + co.cy[j] * Y[(size_t)q.list[j] * n + i];
            for (int j = 0; j < co.count; ++j) v = v + co.cs[j] * S[(size_t)q.list[j] * n + i];
            u[i] = v;
        }
        gu = dot(g.data(), u.data(), n); uu = dot(u.data(), u.data(), n);
        if (k > 0) for (int j = 0; j < 3; ++j) trial_sums(a[j], out[j]);
        return 0;
    }
};

}  // namespace

extern "C" {

// One problem from x0 in slices of `slice` iterations (≤ 0: 64).  handed: 1 when the device loop gave the problem back (nothing
// else of the outputs is then meaningful but iters_done).  Traces: [max_iters].
int simq_solve(int kind, int64_t n, const double *x0, const double *D, const cgo_cg_config *cfg, const cgo_ls_config *ls, int64_t slice,
               double *x_out, double *g_out, double *f_out, int64_t *iters_ran, int32_t *status, int64_t *total_evals,
               double *tr_f, double *tr_g, double *tr_a, int64_t *tr_e, int64_t *slices, int32_t *handed) {
    if (cfg->beta.kind != CGO_BETA_LBFGS || cfg->beta.lbfgs_m < 1 || cfg->beta.lbfgs_m > QN_MAX_M) return CGO_EINVAL;
    const int m = cfg->beta.lbfgs_m;
    PlainQn v{};
    v.kind = kind; v.n = n; v.D = D;
    v.x.assign(x0, x0 + n); v.u.assign(n, 0.0); v.g.assign(n, 0.0); v.gt.assign(n, 0.0); v.xp.assign(n, 0.0);
    v.S.assign((size_t)(m + 1) * n, 0.0); v.Y.assign((size_t)(m + 1) * n, 0.0);
    qn_init(v.q, m);
    qn_coefficients(v.q, v.co);
    ResConfig c{};
    c.ls = *ls; c.eps = cfg->eps; c.mu = cfg->beta.mu; c.beta_kind = cfg->beta.kind; c.npts = 3; c.max_iters = cfg->max_iters; c.log_on = 0;
    ResState s;
    std::memset(&s, 0, sizeof s);
    s.a_initial = NAN;
    // optim.jl:25-47, as the kernel's RES_FRESH branch has it
    s.f_x = v.fg(v.x.data(), v.g.data());
    const double f_x0 = s.f_x;
    s.gg = PlainQn::dot(v.g.data(), v.g.data(), n);
    bool zero = true;
    for (int64_t i = 0; i < n; ++i) { v.u[i] = -v.g[i]; zero = zero && v.g[i] == 0.0; }
    s.dphi0 = -s.gg; s.uu = s.gg; s.dir_neg = 1;
    *handed = 0; *slices = 0; *total_evals = 1;
    if (sumsq_in_range(s.gg)) s.norm = std::sqrt(s.gg);
    else if (s.gg == 0.0 && zero) s.norm = 0.0;
    else { *handed = 1; *iters_ran = 0; return CGO_OK; }
    std::vector<ResRecord> recs((size_t)(cfg->max_iters > 0 ? cfg->max_iters : 1) + 1);
    const int64_t budget = slice > 0 ? slice : 64;
    for (;;) {
        res_iterate_qn(c, s, v, budget, recs.data() + s.it);
        ++*slices;
        *total_evals += s.evals;
        if (s.reason == RES_STOP || s.reason == RES_HOST) break;
        if (!(s.reason == RES_BUDGET && s.done > 0)) return CGO_ESTATE;
    }
    for (int64_t i = 0; i < s.it; ++i) { tr_f[i] = recs[(size_t)i].f; tr_g[i] = recs[(size_t)i].norm; tr_a[i] = recs[(size_t)i].a; tr_e[i] = recs[(size_t)i].evals; }
    *iters_ran = s.it;
    if (s.reason == RES_HOST) { *handed = 1; return CGO_OK; }
    int64_t ran = 0;
    *status = stop_status(s.it, cfg->max_iters, s.f_x, s.norm, cfg->eps, f_x0, ran);
    *iters_ran = ran;
    *f_out = s.f_x;
    v.fg(v.x.data(), v.g.data());
    std::memcpy(x_out, v.x.data(), sizeof(double) * (size_t)n);
    std::memcpy(g_out, v.g.data(), sizeof(double) * (size_t)n);
    return CGO_OK;
}

// The ring on explicit vectors: candidate t is (s[t], y[t]), the gradient after it g[t] ([npush][n] each).  After every push:
// whether it was kept, the pair count, the slot list, γ and the direction coefficients (cy, cs: [npush][QN_MAX_M]); slot_of[t]:
// the physical slot candidate t was written to.
int simq_ring(int m, int64_t n, int npush, const double *s_all, const double *y_all, const double *g_all, int32_t *kept, int32_t *count,
              int32_t *list, double *gamma, double *cy, double *cs, int32_t *slot_of) {
    if (m < 1 || m > QN_MAX_M) return CGO_EINVAL;
    QnState q; QnCoef co;
    qn_init(q, m);
    std::vector<double> S((size_t)(m + 1) * n), Y((size_t)(m + 1) * n);
    for (int t = 0; t < npush; ++t) {
        const double *s = s_all + (size_t)t * n, *y = y_all + (size_t)t * n, *g = g_all + (size_t)t * n;
        slot_of[t] = q.free_slot;
        std::memcpy(S.data() + (size_t)q.free_slot * n, s, sizeof(double) * (size_t)n);   // (before s·y is known, as the push pass does)
        std::memcpy(Y.data() + (size_t)q.free_slot * n, y, sizeof(double) * (size_t)n);
        double sums[QN_SUMS] = {};
        sums[QS_SY] = PlainQn::dot(s, y, n); sums[QS_YY] = PlainQn::dot(y, y, n); sums[QS_SGN] = PlainQn::dot(s, g, n); sums[QS_YGN] = PlainQn::dot(y, g, n);
        for (int j = 0; j < q.count; ++j) {
            const double *sj = S.data() + (size_t)q.list[j] * n, *yj = Y.data() + (size_t)q.list[j] * n;
            double *p = sums + QS_PAIR0 + QP_PER_PAIR * j;
            p[QP_SJG] = PlainQn::dot(sj, g, n); p[QP_YJG] = PlainQn::dot(yj, g, n);
            p[QP_SJYN] = PlainQn::dot(sj, y, n); p[QP_YJSN] = PlainQn::dot(yj, s, n); p[QP_YJYN] = PlainQn::dot(yj, y, n);
        }
        kept[t] = qn_update(q, sums) ? 1 : 0;
        qn_coefficients(q, co);
        count[t] = q.count; gamma[t] = co.gamma;
        for (int j = 0; j < QN_MAX_M; ++j) { list[t * QN_MAX_M + j] = j < q.count ? q.list[j] : -1; cy[t * QN_MAX_M + j] = co.cy[j]; cs[t * QN_MAX_M + j] = co.cs[j]; }
    }
    return CGO_OK;
}

int simq_state_bytes(void) { return (int)sizeof(QnState); }
int simq_coef_bytes(void) { return (int)sizeof(QnCoef); }

// What lane 0 of k_batch_lbfgs does after a push pass, on the host: qn_update (which commits a kept pair) and qn_coefficients of
// cgo_qn.hpp on a state given as its 8-byte words and the 64 sums of the push row.  Out: the state and the coefficient block
// as words, whether the pair was kept.  (tests/test_batch_kernel_sums.py: the device's state, word for word.)
int simq_update(const unsigned long long *state_in, const double *sums, unsigned long long *state_out, unsigned long long *coef_out, int32_t *kept) {
    QnState q; QnCoef co;
    std::memcpy(&q, state_in, sizeof q);
    std::memset(&co, 0, sizeof co);
    if (q.m < 1 || q.m > QN_MAX_M || q.count < 0 || q.count > q.m || q.free_slot < 0 || q.free_slot > q.m) return CGO_EINVAL;
    for (int j = 0; j <= QN_SLOTS; ++j) if (q.list[j] < 0 || q.list[j] > q.m) return CGO_EINVAL;
    *kept = qn_update(q, sums) ? 1 : 0;
    qn_coefficients(q, co);
    std::memcpy(state_out, &q, sizeof q);
    std::memcpy(coef_out, &co, sizeof co);
    return CGO_OK;
}

}  // extern "C"
