// cgo_modes.hpp — what a launch of the gradient-free CG family (k_cg, k_cg_armed, k_chain: R_*, r_*) and of the stored-gradient
// family (k_fused: M_*, m_*) does, as a function of its mode: the mode bits, and which vectors a mode reads, writes and sums.
// Plain C++, constexpr only: the kernels (on their template argument), the backend's launches and byte accounting, the run-time
// compiled module and the CPU tests all ask HERE.  (The row layouts — widths, slots, RW, NS — stay with the kernels that fill the
// rows: cgo_kernels_cg.hip.hpp, cgo_kernels.hip.hpp.)
#pragma once

namespace cgo {
namespace dev {

enum RMode : int {
    R_ACCEPT = 1,  // x ← x + a_acc·u                       optim.jl:136,140
    R_DIR = 2,     // u ← −g + β·u ; Σ g·u, Σ u·u            cg_flavours.jl:10-12, nocedal.jl:56, wolfe.jl:240
    R_TRIAL = 4,   // NPTS × { xp = x + a_j·u ; g⁺ = ∇f(xp) ; all trial sums }   cg_utils.jl:4-23
    R_INIT = 8,    // u = −∇f(x) ; Σ f, Σ g·g                 optim.jl:25-26, cg_flavours.jl:29
    R_RESET = 16,  // u = −∇f(x) ; Σ g·u, Σ u·u               wolfe.jl:129
    R_UPG = 32,    // Σ (u + ∇f(x))²                          wolfe.jl:123
    R_GRAD = 64,   // gout = ∇f(x)                            (materialise for Results.gradient)
    R_GRADT = 128, // gout = ∇f(x + a_0·u)                    (rare: LinearAlgebra.norm scaled path on g⁺)
    R_PROJ = 256,  // solvesystem: x2 ← x2 + m·∇f(x + a_0·u) ; g⁺ = ∇f(x2) ; trial sums of g⁺ against ∇f(x), u
                   //                                          solve_system.jl:169-177,199-204,239-253  (m = P.beta)
    // Lazy direction: the direction is recoverable from the stored iterate one step later, so every second
    // accept + direction + trial launch leaves the OLD u in memory and the next launch forms the new one itself.
    R_ULAG = 1024, // on load, before anything else: u ← −∇f(x) + β_prev·u — memory holds (x_{k+1}, u_k), β_prev = β_k; no sums
                   // (those of this direction were formed by the launch that did not store it).  Alone: store that u.
    R_NOWU = 2048, // R_DIR without the store of u: registers, sums and trials use the new direction, memory keeps the old one
    // Replay: x may lag as well.  Memory holds (x_k, u_k) and the host the scalars (a*_k, β_k), (a*_{k+1}, β_{k+1}), …
    // of the steps accepted since; a launch rebuilds the current pair in registers from them.
    R_REPLAY = 4096, // on load, before anything else, for j < nrep: x ← x + ra[j]·u ; u ← −∇f(x) + rb[j]·u — the R_ACCEPT and R_DIR
                     // expressions; no sums (they belonged to the launches that first formed these directions).  Alone: store x and u.
    R_NOWX = 8192,   // R_ACCEPT without the store of x (always together with R_NOWU)
    // Lean sums: trial sums the solver's β flavour never reads (beta_unread_sums, cgo_ctl.hpp) are not formed —
    // compile-time only, no branch in the loop.  Row width and slot positions stay; a dropped slot leaves the tail as +0.0, the
    // others keep their accumulator chains bit for bit.  R_TRIAL block only.
    R_NOGTG = 16384,   // no Σ g⁺·g
    R_NOYY = 32768,    // no Σ y·y
    R_NOUY = 65536,    // no Σ u·y
    R_NOYGT = 131072   // no Σ y·g⁺
};
constexpr int R_EDGES = 512;   // stencil launches (cgo_kernels_chain.hip.hpp): publish the edge values of the CURRENT x, u only (after set_x0)
constexpr int R_LEAN = R_NOGTG | R_NOYY | R_NOUY | R_NOYGT;   // transparent to every decision taken on a mode but the row that runs

// ---- the facts about a mode, written for the rows of cgo_instances.def ----------------------------------------------------------
// (A combination no row has gets whatever these rules give: its launch fails with "mode not instantiated" before any byte count
// reaches the profile.)
constexpr int r_base(int mode) { return mode & ~R_LEAN; }   // lean sums drop arithmetic, not bytes
// streams u (R_EDGES only looks at the edge lanes' u: k_chain adds that itself)
constexpr bool r_reads_u(int mode) { return (mode & (R_ACCEPT | R_DIR | R_TRIAL | R_UPG | R_GRADT | R_PROJ | R_ULAG | R_REPLAY)) != 0; }
// stores x: an accept, unless told not to; the replay materialise pass.  Stores u: a new direction, unless told not to; both materialise passes
constexpr bool r_writes_x(int mode) { return ((mode & R_ACCEPT) != 0 && !(mode & R_NOWX)) || r_base(mode) == R_REPLAY; }
constexpr bool r_writes_u(int mode) { return (mode & R_INIT) != 0 || ((mode & (R_DIR | R_RESET)) != 0 && !(mode & R_NOWU)) || r_base(mode) == R_ULAG || r_base(mode) == R_REPLAY; }
constexpr bool r_writes_g(int mode) { return (mode & (R_GRAD | R_GRADT)) != 0; }
// leaves a row of sums (an accept-only launch ends the solve; the others store vectors for later readers)
constexpr bool r_has_sums(int mode) { const int m = r_base(mode); return m != R_ACCEPT && m != R_GRAD && m != R_GRADT && m != R_ULAG && m != R_REPLAY; }
constexpr bool r_big_only(int mode) { return (mode & (R_ULAG | R_NOWU | R_REPLAY | R_NOWX)) != 0; }   // pure-HBM (BIG) instantiations only: lag, replay, lean rows
constexpr bool r_read_only(int mode) { return mode == R_TRIAL || mode == R_UPG; }   // the read-only streaming threshold applies
constexpr bool r_evaluates(int mode) { return r_base(mode) != R_ACCEPT && r_base(mode) != R_EDGES; }   // ∇f, i.e. streams the parameter vectors
// n-long double vectors the launch streams, for an objective of p parameter vectors: x, u, parameters, x2 in and out, then the stores
constexpr int r_vectors(int mode, int p) {
    if (r_base(mode) == R_EDGES) return 0;
    return 1 + (r_reads_u(mode) ? 1 : 0) + (r_evaluates(mode) ? p : 0) + ((mode & R_PROJ) ? 2 : 0)
           + (r_writes_x(mode) ? 1 : 0) + (r_writes_u(mode) ? 1 : 0) + (r_writes_g(mode) ? 1 : 0);
}

// ---- the stored-gradient family (k_fused, cgo_kernels.hip.hpp; what each bit computes is told there) -----------------------------
enum Mode : int { M_ACCEPT = 1, M_DIR = 2, M_TRIAL = 4, M_BETA = 8, M_INIT = 16, M_RESET = 32, M_UPG = 64, M_BETAONLY = 128 };
// the facts about a mode, written for the CGO_FUSED_* rows of cgo_instances.def: what it loads …
constexpr bool m_reads_x(int mode) { return (mode & (M_ACCEPT | M_TRIAL | M_INIT)) != 0; }
constexpr bool m_reads_u(int mode) { return (mode & (M_ACCEPT | M_DIR | M_TRIAL | M_UPG | M_BETAONLY)) != 0; }
constexpr bool m_reads_g(int mode) { return (mode & (M_DIR | M_BETA | M_RESET | M_UPG | M_BETAONLY)) != 0; }
constexpr bool m_reads_gt(int mode) { return (mode & M_BETAONLY) != 0; }
// … ∇f: streams the parameter vectors and takes an objective-specific instantiation (the other modes run as ObjQuadDiag's) …
constexpr bool m_evaluates(int mode) { return (mode & (M_TRIAL | M_INIT)) != 0; }
constexpr bool m_writes_x(int mode) { return (mode & M_ACCEPT) != 0; }   // … what it stores …
constexpr bool m_writes_u(int mode) { return (mode & (M_DIR | M_RESET | M_INIT)) != 0; }
constexpr bool m_writes_gt(int mode) { return m_evaluates(mode); }
constexpr bool m_has_sums(int mode) { return mode != M_ACCEPT; }   // … a row of sums, unless the launch ends the solve …
constexpr bool m_read_only(int mode) { return mode == M_UPG || mode == M_BETAONLY; }   // … the read-only streaming threshold applies
constexpr int m_vectors(int mode, int p) {   // n-long double vectors the launch streams, for an objective of p parameter vectors
    return (m_reads_x(mode) ? 1 : 0) + (m_reads_u(mode) ? 1 : 0) + (m_reads_g(mode) ? 1 : 0) + (m_reads_gt(mode) ? 1 : 0)
           + (m_evaluates(mode) ? p : 0) + (m_writes_x(mode) ? 1 : 0) + (m_writes_u(mode) ? 1 : 0) + (m_writes_gt(mode) ? 1 : 0);
}
}  // namespace dev
}  // namespace cgo
