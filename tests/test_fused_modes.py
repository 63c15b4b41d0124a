"""CPU tier: what a launch of the stored-gradient family (k_fused) reads, writes and sums, as csrc/cgo_modes.hpp derives it from
the mode (m_*), and which mode a launch of each kind runs (csrc/cgo_launch_kinds.hpp) — the sibling of tests/test_launch_modes.py.
Both headers are compiled by the host compiler into the test double (sim_fused_mode, sim_launch_kinds).

The table of vector counts is a literal.  It was checked against the branch-per-mode bytes_for this header replaced, compiled
into a scratch program for the same inputs before it went: 10 rows × 5 objective kinds × 0 … 4 parameter vectors.  The two tables
of launch kinds are literals too, copied from the pairs of switches (kernel_symbol / probe_launch, kernel_symbol /
probe_launch_stored) they replaced."""
import ctypes as C
import os
import re

import _instances as I
from _cases import sim_lib
from test_launch_modes import _kinds

B = I.BITS
M_ACCEPT, M_DIR, M_TRIAL, M_BETA, M_INIT, M_RESET, M_UPG, M_BETAONLY = (B[k] for k in ("M_ACCEPT", "M_DIR", "M_TRIAL", "M_BETA", "M_INIT", "M_RESET", "M_UPG", "M_BETAONLY"))
ADTB = M_ACCEPT | M_DIR | M_TRIAL | M_BETA
# mode → (vectors besides the parameter vectors, does it stream the p parameter vectors); p = max(kind == QUAD_DIAG, n_params)
VECTORS = {M_INIT: (3, True), M_TRIAL | M_BETA: (4, True), M_TRIAL: (3, True), ADTB: (6, True), M_ACCEPT | M_DIR: (5, False),
           M_ACCEPT: (3, False), M_DIR: (3, False), M_RESET: (2, False), M_UPG: (2, False), M_BETAONLY: (3, False)}
NAMES = ("vectors", "reads_x", "reads_u", "reads_g", "reads_gt", "evaluates", "writes_x", "writes_u", "writes_gt", "has_sums", "read_only")


def _facts(mode, kind, n_params):
    out = (C.c_int * 11)()
    sim_lib().sim_fused_mode(mode, kind, n_params, out)
    return dict(zip(NAMES, [out[0]] + [bool(v) for v in out[1:]]))


def _rows():
    return [(fam, mode) for fam in ("FUSED_OBJ", "FUSED_FREE") for (mode,) in I.rows(fam)]


def test_every_row_is_in_the_table():
    assert [len(I.rows(f)) for f in ("FUSED_OBJ", "FUSED_FREE")] == [4, 6]
    assert {mode for _, mode in _rows()} == set(VECTORS) and len(_rows()) == len(VECTORS)


def test_vector_counts_are_the_table():
    for fam, mode in _rows():
        base, with_p = VECTORS[mode]
        for name, kind in _kinds().items():
            for n_params in range(5):
                p = max(1 if name == "CGO_OBJ_QUAD_DIAG" else 0, n_params)
                got = _facts(mode, kind, n_params)["vectors"]
                assert got == base + (p if with_p else 0) and got > 0, (fam, mode, name, n_params, got)


def test_sums_read_only_and_evaluates():
    for fam, mode in _rows():
        f = _facts(mode, 0, 0)
        assert f["has_sums"] == (mode != M_ACCEPT), (fam, mode)
        assert f["read_only"] == (mode in (M_UPG, M_BETAONLY)), (fam, mode)
        assert f["evaluates"] == (fam == "FUSED_OBJ") == VECTORS[mode][1], (fam, mode)
        assert f["read_only"] <= (not (f["writes_x"] or f["writes_u"] or f["writes_gt"])), (fam, mode)
    assert not _facts(M_UPG | M_BETAONLY, 0, 0)["read_only"]   # exact equality, not a mask


def test_loads_and_stores_of_every_row():
    """x u g g⁺ read / x u g⁺ written, as the comment block of csrc/cgo_kernels.hip.hpp describes each mode"""
    want = {M_INIT: ("x", "ug"), M_TRIAL | M_BETA: ("xug", "g"), M_TRIAL: ("xu", "g"), ADTB: ("xug", "xug"), M_ACCEPT | M_DIR: ("xug", "xu"),
            M_ACCEPT: ("xu", "x"), M_DIR: ("ug", "u"), M_RESET: ("g", "u"), M_UPG: ("ug", ""), M_BETAONLY: ("ugt", "")}
    for _, mode in _rows():
        f = _facts(mode, 0, 0)
        reads = "".join(c for c, k in (("x", "reads_x"), ("u", "reads_u"), ("g", "reads_g"), ("t", "reads_gt")) if f[k])
        writes = "".join(c for c, k in (("x", "writes_x"), ("u", "writes_u"), ("g", "writes_gt")) if f[k])   # (g: the g⁺ buffer)
        assert (reads, writes) == want[mode], (mode, reads, writes)


# ---- launch kind → mode -----------------------------------------------------------------------------------------------------
def _kk():
    src = open(os.path.join(I.CSRC, "cgo_engine.hpp")).read()
    body = re.search(r"enum KernelKind : int \{(.*?)\};", src, re.S).group(1)
    names = re.findall(r"^\s*(KK_[A-Z_]+)\b", body, re.M)
    assert names[0] == "KK_INIT" and names[-1] == "KK_COUNT"
    return {n: i for i, n in enumerate(names)}


def _table(fused):
    out = (C.c_int * (5 * 32))()
    n = sim_lib().sim_launch_kinds(fused, out, 32)
    return [tuple(out[5 * i:5 * i + 5]) for i in range(n)]


def test_k_cg_kinds_are_the_two_switches_they_replaced():
    K, R = _kk(), {k: v for k, v in B.items() if k.startswith("R_")}
    ADT = R["R_ACCEPT"] | R["R_DIR"] | R["R_TRIAL"]
    N = R["R_REPLAY"] | ADT | R["R_NOWU"] | R["R_NOWX"]
    ONE, MAX, MAX3 = 0, 1, 2
    want = [("KK_INIT", R["R_INIT"], ONE, R["R_GRAD"], 0), ("KK_TRIAL", R["R_TRIAL"], MAX3, R["R_ULAG"] | R["R_TRIAL"], R["R_REPLAY"] | R["R_TRIAL"]),
            ("KK_ACCEPT_DIR_TRIAL", ADT, MAX, R["R_ULAG"] | ADT, R["R_REPLAY"] | ADT), ("KK_ACCEPT_TRIAL_NOSTORE", N, MAX, 0, 0),
            ("KK_MATERIALIZE_XU", R["R_REPLAY"], ONE, 0, 0), ("KK_ACCEPT_TRIAL_LAZY", ADT | R["R_NOWU"], MAX, 0, 0),
            ("KK_MATERIALIZE_U", R["R_ULAG"], ONE, 0, 0), ("KK_ACCEPT_DIR", R["R_ACCEPT"] | R["R_DIR"], ONE, 0, 0),
            ("KK_ACCEPT_ONLY", R["R_ACCEPT"], ONE, 0, 0), ("KK_RESET_DIR", R["R_RESET"], ONE, 0, 0), ("KK_UPG_NORM", R["R_UPG"], ONE, 0, 0),
            ("KK_DIR_TRIAL", R["R_DIR"] | R["R_TRIAL"], MAX, R["R_DIR"], 0), ("KK_SYS_PROJECT", R["R_PROJ"], ONE, 0, 0)]
    assert _table(0) == [(K[k],) + tuple(rest) for k, *rest in want]
    # every mode a kind names, default or not, is a row of the k_cg family
    rows = {mode for fam in ("CG", "CG_LAG", "CG_REPLAY") for mode, _ in I.rows(fam)}
    assert {m for _, mode, _, a0, a1 in _table(0) for m in (mode, a0, a1) if m} <= rows


def test_k_fused_kinds_are_the_two_switches_they_replaced():
    K = _kk()
    want = [("KK_INIT", M_INIT, 0, M_BETAONLY), ("KK_TRIAL", M_TRIAL | M_BETA, M_TRIAL, M_BETAONLY), ("KK_ACCEPT_DIR_TRIAL", ADTB, 0, M_ACCEPT | M_DIR),
            ("KK_ACCEPT_DIR", M_ACCEPT | M_DIR, 0, M_ACCEPT | M_DIR), ("KK_ACCEPT_ONLY", M_ACCEPT, 0, M_ACCEPT), ("KK_RESET_DIR", M_RESET, 0, M_RESET),
            ("KK_UPG_NORM", M_UPG, 0, M_UPG)]
    assert _table(1) == [(K[k],) + tuple(rest) + (0,) for k, *rest in want]
    assert {m for _, mode, alt, host, _ in _table(1) for m in (mode, alt, host) if m} <= set(VECTORS)


# ---- stated once ------------------------------------------------------------------------------------------------------------
def test_the_facts_are_stated_once():
    """the objective-mode mask, the no-sums rule and the read-only pair: spelled out in cgo_modes.hpp and nowhere else in csrc/;
    bytes_for has no per-mode branch; one place formats a k_fused name; kernel_symbol and its L-BFGS half carry no byte formula"""
    texts = {f: open(os.path.join(I.CSRC, f)).read() for f in sorted(os.listdir(I.CSRC)) if f.endswith((".hpp", ".hip", ".def"))}
    pats = {"evaluates": r"M_TRIAL \| M_INIT|M_INIT \| M_TRIAL", "no sums": r"!= M_ACCEPT", "read only": r"M_UPG \|\| \w+ == M_BETAONLY|M_BETAONLY \|\| \w+ == M_UPG"}
    for what, pat in pats.items():
        assert [f for f, t in texts.items() if re.search(pat, t)] == ["cgo_modes.hpp"], what
    body = re.search(r"double bytes_for\(.*?\n\}", texts["cgo_hip_backend.hip"], re.S).group(0)
    assert "m_vectors(mode, p)" in body and "if" not in body and body.count("\n") <= 4, body
    assert sum(t.count("k_fused<%s") for t in texts.values()) == 1
    assert "struct Needs" not in texts["cgo_kernels.hip.hpp"] and "enum Mode" not in texts["cgo_kernels.hip.hpp"]
    for f, fn in (("cgo_backend_cg.hip", "kernel_symbol"), ("cgo_backend_lbfgs.hip", "lbfgs_symbol")):
        body = re.search(r"std::string HipBackend::%s\(.*?\n\}" % fn, texts[f], re.S).group(0)
        assert "8.0 * (double)n *" not in body and "bytes_r(" not in body and body.count("\n") <= 40, body
    # the pure-HBM question about the accept + direction + trial launch: asked in one member
    adt = r"bytes_r\(obj_->kind, (R_ADT|R_ACCEPT \| R_DIR \| R_TRIAL), .{0,60}?\) > big_bytes\("
    assert sum(len(re.findall(adt, t)) for t in texts.values()) == 1 and re.search(r"bool HipBackend::adt_is_big\(\) const \{ return " + adt, texts["cgo_backend_cg.hip"])
