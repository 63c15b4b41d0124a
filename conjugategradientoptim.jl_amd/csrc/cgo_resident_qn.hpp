// cgo_resident_qn.hpp — res_iterate_qn: whole outer iterations of minimizeobjective with β = LBFGS(m), without the host.
//
// res_iterate (cgo_resident.hpp) with its β block replaced by the quasi-Newton update: the same resumable line-search
// machines, the same ResEval, stop test, records, RES_BUDGET / RES_STOP / RES_HOST and slice budget.  (A header of its own:
// cgo_resident.hpp is part of the text every run-time compiled module is built from, and that text does not change.)
//
// What V adds to the vector operations res_iterate asks for:
//   int  push_update(double a)   x ← x + a·u; the pair s = a·u, y = ∇f(x + a·u) − ∇f(x) into the ring's free slot; the sums of
//                                the push; then the scalar recursion (cgo_qn.hpp: qn_update, qn_coefficients) on the problem's
//                                QnState.  Returns the number of stored pairs, identical in every caller thread.
//   int  combine_trial(a, k, out, gu, uu)
//                                u = −γ·g + Σ cy_j·Y_j + Σ cs_j·S_j with the coefficients push_update left, g·u, u·u, and the
//                                first k trial points of the next line search — what accept_dir_trial leaves for CG.
// The hand-back conditions are res_iterate's, all decided BEFORE push_update touches x: a line-search outcome other than
// :success, a non-finite ϕ or norm, sumsq_in_range failing without the zero-gradient check settling it, WolfeBisection's
// bracket collapse.  The host then solves such a problem again from its own x0.
#pragma once

#include "cgo_qn.hpp"
#include "cgo_resident.hpp"

namespace cgo {

template <class V>
CGO_HD inline void res_iterate_qn(const ResConfig &c, ResState &s, V &v, int64_t budget, ResRecord *recs) {
    s.done = 0; s.log_len = 0; s.evals = 0; s.passes = 0; s.reason = RES_BUDGET;
    s.t_machine = 0; s.t_eval = 0; s.t_post = 0;
    const int npts = V::kNpts > 0 ? V::kNpts : c.npts;
    constexpr int NCP = V::kNpts > 0 ? V::kNpts : RES_MAXP;
    while (s.done < budget) {
        const int64_t n = s.it + 1;
        if (n > c.max_iters) { s.reason = RES_STOP; break; }                                          // optim.jl:162-169
        if (hd_isfinite(s.f_x) && hd_isfinite(s.norm) && s.norm < c.eps) { s.reason = RES_STOP; break; }   // optim.jl:53-80
        ResEval<V> ev{c, s, v, nullptr, 0, 0};
        LsMachine m{};
        m.state = 0; m.flag = 0; m.phi0 = s.f_x; m.d0 = s.dphi0; m.uu = s.uu; m.a_initial = s.a_initial;
        m.o = ls_out(0.0, 0.0, 0, CGO_INCOMPLETE);
        const bool strong = c.ls.kind == CGO_LS_STRONG_WOLFE_BISECTION;
        int rc = 3;
        {
            double phi = 0.0, dphi = 0.0;
            for (;;) {   // the line search asks, ONE place evaluates
                rc = strong ? ls_sw_machine(c.ls, m, phi, dphi) : ls_wb_machine(c.ls, m, phi, dphi);
                if (rc != 1) break;
                const int erc = ev(m.a, phi, dphi, m.h1, m.h2, m.h3, m.h4);
                if (erc) { rc = erc; break; }
            }
        }
        const LSOut o = m.o;
        if (rc == 9) { s.reason = RES_ERROR; break; }
        if (rc != 0 || o.status != CGO_SUCCESS || ev.evals == 0 || ev.overflow) { s.reason = RES_HOST; break; }   // optim.jl:93-104 → host
        const TrialSums t = ev.last;            // info.xp / df_xp: the LAST evaluated trial = the accepted one (both bisection searches)
        if (!sumsq_in_range(t.gtgt) && !res_trial_gradient_is_zero(v, t.gtgt, ev.last_a)) { s.reason = RES_HOST; break; }   // LinearAlgebra.norm rare path
        const double norm_xp = __builtin_sqrt(t.gtgt);                                                // optim.jl:107
        if (!hd_isfinite(o.phi) || !hd_isfinite(norm_xp)) { s.reason = RES_HOST; break; }              // optim.jl:108-121
        // optim.jl:136-141,152-159 (β of a quasi-Newton flavour: 0, as the engine records it)
        s.f_x = o.phi; s.norm = norm_xp; s.gg = t.gtgt; s.it = n; s.a_initial = o.a;
        s.evals += ev.evals;
        s.last_a = ev.last_a; s.last_beta = 0.0;
        if (v.leader()) { ResRecord &r = recs[s.done]; r.f = s.f_x; r.norm = s.norm; r.a = o.a; r.beta = 0.0; r.evals = o.evals; }
        s.done++;
        const bool will_stop = (n == c.max_iters) || (hd_isfinite(s.f_x) && hd_isfinite(s.norm) && s.norm < c.eps);
        // x ← xp, the candidate pair, the Gram blocks, ρ, γ, the slot (Solver::iterate 530–559) — also when the solve stops here:
        // x is the result
        const int stored = v.push_update(ev.last_a);
        s.passes++;
        s.ncache = 0;
        if (will_stop) continue;   // the loop ends at its next test; u is not part of the results
        const double a_next = ls_first_step(c.ls, s.a_initial);                                       // optim.jl:92
        double pts[RES_MAXP] = {0, 0, 0, 0, 0, 0, 0};
        int k = 0;
        if (hd_isfinite(a_next)) k = res_trial_points(c.ls, a_next, npts >= 7 ? 7 : (npts >= 5 ? 5 : (npts >= 3 ? 3 : 1)), pts);
        {   // pad: a pass evaluates a fixed number of points; the spare ones repeat the last real step (results ignored)
            double lastp = 0.0;
#pragma unroll
            for (int j = 0; j < NCP; ++j) { if (j < k) lastp = pts[j]; else pts[j] = lastp; }
        }
        TrialSums out[RES_MAXP] = {};
        double gu = 0.0, uu_new = 0.0;
        if (int rc2 = v.combine_trial(pts, k, out, gu, uu_new)) { (void)rc2; s.reason = RES_ERROR; break; }   // updatedir! + the first trials
        s.passes++;
        s.dphi0 = gu; s.uu = uu_new; s.dir_neg = (stored == 0) ? 1 : 0;
        s.ncache = k;
#pragma unroll
        for (int j = 0; j < NCP; ++j) { s.ca[j] = pts[j]; s.cs[j] = out[j]; }   // (entries ≥ k are never looked at)
    }
}

}  // namespace cgo
