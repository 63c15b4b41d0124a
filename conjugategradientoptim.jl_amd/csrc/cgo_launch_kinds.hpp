// cgo_launch_kinds.hpp — which mode a launch of each kind (KK_*, cgo_engine.hpp) runs, per kernel family: the engine's entry points,
// kernel_symbol() and the probes' "is this a launch the engine issues" all read THESE tables.  Plain constexpr C++, as cgo_modes.hpp
// (the CPU tests read it through the host simulator).  What depends on the state of a solve — the lazy / replay / lean choice of
// accept_dir_trial_r and trial_r — is policy and stays with them; it is built from the modes named here.
#pragma once
#include "cgo_engine.hpp"
#include "cgo_modes.hpp"

namespace cgo {
// ---- k_cg / k_chain: default mode; trial points of the instantiation kernel_symbol() names — 1, npts_for(max_points()),
// npts_for(min(max_points(), 3)); the other modes a probe may ask for (0: none)
enum PointRule : int { PTS_ONE = 0, PTS_MAX, PTS_MAX3 };
struct RKind { int kk, mode; PointRule pts; int alt[2]; };
constexpr int R_ADT = dev::R_ACCEPT | dev::R_DIR | dev::R_TRIAL;
constexpr RKind R_KINDS[] = {
    {KK_INIT, dev::R_INIT, PTS_ONE, {dev::R_GRAD, 0}},   // (the stencil objective: R_EDGES too — probe_launch)
    {KK_TRIAL, dev::R_TRIAL, PTS_MAX3, {dev::R_ULAG | dev::R_TRIAL, dev::R_REPLAY | dev::R_TRIAL}},
    {KK_ACCEPT_DIR_TRIAL, R_ADT, PTS_MAX, {dev::R_ULAG | R_ADT, dev::R_REPLAY | R_ADT}},   // plain, launch B, launch S
    {KK_ACCEPT_TRIAL_NOSTORE, dev::R_REPLAY | R_ADT | dev::R_NOWU | dev::R_NOWX, PTS_MAX, {0, 0}},   // launch N
    {KK_MATERIALIZE_XU, dev::R_REPLAY, PTS_ONE, {0, 0}},
    {KK_ACCEPT_TRIAL_LAZY, R_ADT | dev::R_NOWU, PTS_MAX, {0, 0}},   // launch A
    {KK_MATERIALIZE_U, dev::R_ULAG, PTS_ONE, {0, 0}},
    {KK_ACCEPT_DIR, dev::R_ACCEPT | dev::R_DIR, PTS_ONE, {0, 0}},
    {KK_ACCEPT_ONLY, dev::R_ACCEPT, PTS_ONE, {0, 0}},
    {KK_RESET_DIR, dev::R_RESET, PTS_ONE, {0, 0}},
    {KK_UPG_NORM, dev::R_UPG, PTS_ONE, {0, 0}},
    {KK_DIR_TRIAL, dev::R_DIR | dev::R_TRIAL, PTS_MAX, {dev::R_DIR, 0}},
    {KK_SYS_PROJECT, dev::R_PROJ, PTS_ONE, {0, 0}}};
constexpr const RKind *r_kind(int kk) { for (const RKind &r : R_KINDS) if (r.kk == kk) return &r; return nullptr; }
constexpr int r_mode_of(int kk) { return r_kind(kk) ? r_kind(kk)->mode : -1; }
constexpr bool r_kind_allows(const RKind &r, int mode) { return mode == r.mode || (r.alt[0] && mode == r.alt[0]) || (r.alt[1] && mode == r.alt[1]); }

// ---- k_fused: default mode; the other mode a probe may ask for (0: none; KK_TRIAL: what runs where no β sums are needed); what a
// solver of the host-closure objective launches for this kind instead (the closure evaluates: the device sums, accepts and directs)
struct MKind { int kk, mode, alt, host; };
constexpr MKind M_KINDS[] = {
    {KK_INIT, dev::M_INIT, 0, dev::M_BETAONLY},
    {KK_TRIAL, dev::M_TRIAL | dev::M_BETA, dev::M_TRIAL, dev::M_BETAONLY},
    {KK_ACCEPT_DIR_TRIAL, dev::M_ACCEPT | dev::M_DIR | dev::M_TRIAL | dev::M_BETA, 0, dev::M_ACCEPT | dev::M_DIR},
    {KK_ACCEPT_DIR, dev::M_ACCEPT | dev::M_DIR, 0, dev::M_ACCEPT | dev::M_DIR},
    {KK_ACCEPT_ONLY, dev::M_ACCEPT, 0, dev::M_ACCEPT},
    {KK_RESET_DIR, dev::M_RESET, 0, dev::M_RESET},
    {KK_UPG_NORM, dev::M_UPG, 0, dev::M_UPG}};
constexpr const MKind *m_kind(int kk) { for (const MKind &r : M_KINDS) if (r.kk == kk) return &r; return nullptr; }
constexpr int m_mode_of(int kk) { return m_kind(kk) ? m_kind(kk)->mode : -1; }
}  // namespace cgo
