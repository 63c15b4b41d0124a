// cgo_path.hpp — predicted path: which steps a line search will ask for, known before the launch.
//
// Along a direction whose curvature c is known beforehand — exactly, for an objective with a constant Hessian — the line
// search's ϕ is the parabola ϕ(a) = f + a·dϕ₀ + ½a²·c.  The state machines of cgo_ctl.hpp are templated over an evaluator: run
// over that model they list the steps the real search will ask for, in order, and a launch then evaluates those instead of the
// whole tree of ls_trial_points_n.  A prediction only chooses WHICH points a launch evaluates; every decision is still taken on
// the sums the launch formed.  Plain scalar code, host and device clean like cgo_ctl.hpp (a header of its own: the text of
// cgo_ctl.hpp is part of every run-time compiled module, which has no use for this).
//
// The model, from the sums of the accepted point of iteration k (a* its step, gtu = g⁺·u_k, gtgt = g⁺·g⁺, ygt = y·g⁺), the
// direction sum dϕ₀_k = g·u_k of the launch that formed u_k, β of the update u_{k+1} = −g⁺ + β·u_k, and H constant:
//   c_k       = (gtu − dϕ₀_k) / a*                       curvature along u_k (H u_k = y / a*)
//   dϕ₀_{k+1} = −gtgt + β·gtu
//   c_{k+1}   = g⁺ᵀH g⁺ − 2β·ygt/a* + β²·c_k              g⁺ᵀH g⁺: the one sum a path launch adds (ObjCurv)
#pragma once

#include "cgo_ctl.hpp"

namespace cgo {

// evaluator over the model: records every distinct step asked for, up to 7, and answers from the parabola
struct PathModelEval {
    double f, d0, c;
    double a[CTL_MAXP];
    int n; bool over;
    CGO_HD int operator()(double step, double &phi, double &dphi, double, double, double, double) {
        bool seen = false;
        for (int j = 0; j < CTL_MAXP; ++j) if (j < n && a[j] == step) seen = true;
        if (!seen) {
            if (n >= CTL_MAXP) { over = true; return 1; }   // a longer search: its first seven
            for (int j = 0; j < CTL_MAXP; ++j) if (j == n) a[j] = step;   // (no run-time index into a local array: see ls_trial_points)
            ++n;
        }
        phi = f + step * d0 + 0.5 * (step * step) * c;
        dphi = d0 + step * c;
        return 0;
    }
};

// The steps the line search `ls` asks for, in order, on the model (f, dϕ₀, c), started from the previous accepted step
// a_initial → pts[0..k), k ≤ 7.  0 = not predicted: a non-finite input, c ≤ 0, dϕ₀ ≥ 0, Backtracking (whose accepted step is not
// its last trial), the Yuan–Wei–Lu conditions (they read u·u).
CGO_HD inline int ls_predicted_path(const cgo_ls_config &ls, double f, double dphi0, double c, double a_initial, double (&pts)[7]) {
    for (int j = 0; j < 7; ++j) pts[j] = 0.0;
    if (!(hd_isfinite(f) && hd_isfinite(dphi0) && hd_isfinite(c))) return 0;
    if (!(c > 0.0) || !(dphi0 < 0.0)) return 0;
    if (ls.kind != CGO_LS_STRONG_WOLFE_BISECTION && ls.kind != CGO_LS_WOLFE_BISECTION) return 0;
    if (ls.kind == CGO_LS_WOLFE_BISECTION && ls.cond_kind != CGO_COND_WOLFE) return 0;
    PathModelEval ev;
    ev.f = f; ev.d0 = dphi0; ev.c = c; ev.n = 0; ev.over = false;
    for (int j = 0; j < CTL_MAXP; ++j) ev.a[j] = 0.0;
    LSOut o = ls_out(0.0, 0.0, 0, CGO_INCOMPLETE);
    if (ls.kind == CGO_LS_STRONG_WOLFE_BISECTION) {
        (void)ls_strong_wolfe_t(ls, f, dphi0, a_initial, ev, o);
    } else {
        CtlNoBackend bk;   // (a bracket collapse needs vector work: the path ends there)
        double uu = 0.0;
        (void)ls_wolfe_bisection_t(ls, f, dphi0, uu, a_initial, ev, bk, o);
    }
    for (int j = 0; j < 7; ++j) pts[j] = ev.a[j];
    for (int j = 0; j < 7; ++j) if (j < ev.n && !(hd_isfinite(pts[j]) && pts[j] > 0.0)) return 0;   // a step no launch evaluates
    return ev.n;
}

}  // namespace cgo
