// cgo_qn.hpp — the SCALAR side of L-BFGS in its Gram form, stated once over fixed-size arrays.
//
// The engine keeps the quasi-Newton state of a solve in std::vectors (Solver::iterate, qn_commit, qn_direction: cgo_engine.cpp)
// and runs the two-loop recursion of Nocedal & Wright Alg. 7.4 on stored inner products.  A batched L-BFGS solve
// (k_batch_lbfgs, cgo_kernels_batch_lbfgs.hip.hpp) runs the same statements on the device, one state per problem, where
// nothing can be allocated: here they are as CGO_HD functions over a QnState of compile-time size — the device loop
// (cgo_resident_qn.hpp) and the CPU tier's test double (tests/hostsim) both call these, Solver itself stays as it is.
//
// The ring has m + 1 physical slots: a candidate pair is written to the free slot BEFORE s·y > 0 is known, so a dropped
// candidate never clobbers a stored pair.  `list` names the slots of the stored pairs, newest → oldest.
#pragma once

#include "cgo_ctl.hpp"

namespace cgo {

constexpr int QN_MAX_M = 10;            // = cgo_batch_lbfgs_max_m()
constexpr int QN_SLOTS = QN_MAX_M + 1;  // physical slots of the largest ring

// The sums the push pass leaves (those of k_lbfgs_push_gram): four of the new pair, five per stored pair j (newest → oldest).
constexpr int QN_SUMS = 64;             // row width of the push pass (4 + 5·QN_MAX_M = 54, padded to a multiple of 8)
enum QnSum : int { QS_SY = 0, QS_YY, QS_SGN, QS_YGN, QS_PAIR0 };                    // s·y, y·y, s·g⁺, y·g⁺
enum QnPairSum : int { QP_SJG = 0, QP_YJG, QP_SJYN, QP_YJSN, QP_YJYN, QP_PER_PAIR };   // s_j·g⁺, y_j·g⁺, s_j·y, y_j·s, y_j·y
static_assert(QS_PAIR0 + QP_PER_PAIR * QN_MAX_M <= QN_SUMS, "the push row holds every sum");

struct QnState {
    int32_t m, count, free_slot, pad_;   // ring depth; stored pairs; the slot the next candidate is written to
    int32_t list[QN_SLOTS + 1];          // slots of the stored pairs, newest → oldest (entries ≥ count unused)
    double gamma;                        // s·y / y·y of the newest KEPT pair
    double rho[QN_SLOTS];                // 1 / s·y, by slot
    double sg[QN_SLOTS], yg[QN_SLOTS];   // s_j·g, y_j·g at the current g, by slot
    double SY[QN_SLOTS * QN_SLOTS];      // s_i·y_j at [i·(m+1) + j], by slot
    double YY[QN_SLOTS * QN_SLOTS];      // y_i·y_j
};
static_assert(sizeof(QnState) % 8 == 0, "the state is copied as 8-byte words");

// The coefficients of u = −γ·g + Σ cy_k·Y_{list[k]} + Σ cs_k·S_{list[k]}, and the recursion's scratch.
struct QnCoef {
    int32_t count, pad_;
    double gamma;
    double cy[QN_MAX_M], cs[QN_MAX_M];
    double a[QN_MAX_M], c[QN_MAX_M];     // α_k, c_k of the two loops (scratch: a run-time index, so not in registers)
};

CGO_HD inline void qn_init(QnState &q, int m) {
    q.m = m; q.count = 0; q.free_slot = 0; q.pad_ = 0;
    for (int j = 0; j <= QN_SLOTS; ++j) q.list[j] = 0;
    q.gamma = 1.0;
    for (int j = 0; j < QN_SLOTS; ++j) { q.rho[j] = 0.0; q.sg[j] = 0.0; q.yg[j] = 0.0; }
    for (int j = 0; j < QN_SLOTS * QN_SLOTS; ++j) { q.SY[j] = 0.0; q.YY[j] = 0.0; }
}

// Solver::qn_commit: the candidate in `slot` becomes the newest stored pair; the slot it evicts (or the lowest unused one)
// becomes the free slot of the following candidate.
CGO_HD inline void qn_commit(QnState &q, int slot) {
    const int m = q.m;
    for (int j = q.count; j > 0; --j) q.list[j] = q.list[j - 1];
    q.list[0] = slot;
    q.count++;
    if (q.count > m) {
        q.free_slot = q.list[q.count - 1];
        q.count--;
    } else {
        for (int p = 0; p <= m; ++p) {
            bool used = false;
            for (int j = 0; j < q.count; ++j) used = used || (q.list[j] == p);
            if (!used) { q.free_slot = p; break; }
        }
    }
}

// Solver::iterate lines 530–559 in their Gram form: g changed (g⁺ of the accepted step), so every stored pair's s_j·g, y_j·g
// are the new sums; the candidate's row and column of the Gram blocks, ρ and γ are taken only when s·y > 0, and then the
// slot is committed.  Returns whether the pair was kept.
CGO_HD inline bool qn_update(QnState &q, const double *sums) {
    const int slot = q.free_slot, c = q.count, P = q.m + 1;
    const double sy = sums[QS_SY], yy = sums[QS_YY];
    for (int j = 0; j < c; ++j) {
        const double *t = sums + QS_PAIR0 + QP_PER_PAIR * j;
        const int pj = q.list[j];
        q.sg[pj] = t[QP_SJG]; q.yg[pj] = t[QP_YJG];
        if (sy > 0.0) {
            q.SY[pj * P + slot] = t[QP_SJYN];   // s_j·y_new
            q.SY[slot * P + pj] = t[QP_YJSN];   // s_new·y_j
            q.YY[pj * P + slot] = t[QP_YJYN];
            q.YY[slot * P + pj] = t[QP_YJYN];
        }
    }
    if (!(sy > 0.0)) return false;   // dropped: the stored history is untouched
    q.SY[slot * P + slot] = sy; q.YY[slot * P + slot] = yy;
    q.sg[slot] = sums[QS_SGN]; q.yg[slot] = sums[QS_YGN];
    q.rho[slot] = 1.0 / sy;
    q.gamma = sy / yy;
    qn_commit(q, slot);
    return true;
}

// Solver::qn_direction: the two loops of Alg. 7.4 on scalars.  No stored pair: u = −g (γ = 1, no terms).
CGO_HD inline void qn_coefficients(const QnState &q, QnCoef &o) {
    const int c = q.count, P = q.m + 1;
    const int32_t *L = q.list;
    o.count = c; o.pad_ = 0;
    for (int k = 0; k < QN_MAX_M; ++k) { o.cy[k] = 0.0; o.cs[k] = 0.0; o.a[k] = 0.0; o.c[k] = 0.0; }
    if (c == 0) { o.gamma = 1.0; return; }
    const double gamma = q.gamma;
    o.gamma = gamma;
    for (int k = 0; k < c; ++k) {           // newest → oldest: α_k = ρ_k · s_k·q,  q = g − Σ_{j<k} α_j y_j
        double sq = q.sg[L[k]];
        for (int j = 0; j < k; ++j) sq -= o.a[j] * q.SY[L[k] * P + L[j]];
        o.a[k] = q.rho[L[k]] * sq;
    }
    for (int k = c - 1; k >= 0; --k) {      // oldest → newest: β_k = ρ_k · y_k·r,  r = γq + Σ_{j>k} c_j s_j
        double yq = q.yg[L[k]];
        for (int j = 0; j < c; ++j) yq -= o.a[j] * q.YY[L[k] * P + L[j]];
        double yr = gamma * yq;
        for (int j = c - 1; j > k; --j) yr += o.c[j] * q.SY[L[j] * P + L[k]];
        o.c[k] = o.a[k] - q.rho[L[k]] * yr;
    }
    for (int k = 0; k < c; ++k) { o.cy[k] = gamma * o.a[k]; o.cs[k] = -o.c[k]; }
}

}  // namespace cgo
