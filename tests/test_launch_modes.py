"""CPU tier: what a launch of the gradient-free CG family reads, writes and sums, as csrc/cgo_modes.hpp derives it from the mode —
the one place the kernels (k_cg, k_cg_armed, k_chain), the backend's launch code and its byte accounting (bytes_r) ask.  The header
is compiled by the host compiler into the test double (sim_launch_mode, tests/hostsim/sim_backend.cpp), which also shows that it is
plain C++; every row of csrc/cgo_instances.def is walked for every built-in objective kind and the run-time compiled one, with 0 … 4
parameter vectors.

The table of vector counts below is a literal: it was printed by the branch-per-mode bytes_r this header replaced, for the same inputs,
before it went."""
import ctypes as C
import os
import re

import pytest

import _instances as I
from _cases import sim_lib

B = I.BITS
R_ACCEPT, R_DIR, R_TRIAL, R_INIT, R_RESET, R_UPG = (B[k] for k in ("R_ACCEPT", "R_DIR", "R_TRIAL", "R_INIT", "R_RESET", "R_UPG"))
R_GRAD, R_GRADT, R_PROJ, R_EDGES = (B[k] for k in ("R_GRAD", "R_GRADT", "R_PROJ", "R_EDGES"))
R_ULAG, R_NOWU, R_REPLAY, R_NOWX = (B[k] for k in ("R_ULAG", "R_NOWU", "R_REPLAY", "R_NOWX"))
R_LEAN = B["R_NOGTG"] | B["R_NOYY"] | B["R_NOUY"] | B["R_NOYGT"]
ADT = R_ACCEPT | R_DIR | R_TRIAL

# mode → (vectors besides the parameter vectors, does it stream the p parameter vectors); p = max(kind == QUAD_DIAG, n_params)
VECTORS = {
    R_INIT: (2, True), R_TRIAL: (2, True), ADT: (4, True), R_ACCEPT | R_DIR: (4, True), R_ACCEPT: (3, False), R_RESET: (2, True),
    R_UPG: (2, True), R_GRAD: (2, True), R_GRADT: (3, True), R_DIR: (3, True), R_DIR | R_TRIAL: (3, True), R_PROJ: (4, True),
    R_EDGES: (0, False),
    ADT | R_NOWU: (3, True), R_ULAG | ADT: (4, True), R_ULAG | R_TRIAL: (2, True), R_ULAG: (3, True),
    R_REPLAY | ADT | R_NOWU | R_NOWX: (2, True), R_REPLAY | ADT: (4, True), R_REPLAY | R_TRIAL: (2, True), R_REPLAY: (4, True),
}
NO_SUMS = {R_ACCEPT, R_GRAD, R_GRADT, R_ULAG, R_REPLAY}
FAMILIES = ("CG", "CG_LAG", "CG_REPLAY", "CG_LEAN", "CG_ARMED", "CHAIN")
BIG_ONLY = ("CG_LAG", "CG_REPLAY", "CG_LEAN")


def _kinds():
    """CGO_OBJ_* name → number (include/cgo.h) for the objectives with ahead-of-time kernels, the stencil one and the user's"""
    src = open(os.path.join(os.path.dirname(I.CSRC), "..", "include", "cgo.h")).read()
    num = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(CGO_OBJ_\w+) = (\d+)", src)}
    names = [k for k, _ in I.rows("OBJ")] + ["CGO_OBJ_ROSENBROCK_CHAINED", "CGO_OBJ_USER"]
    assert len(names) == 5 and num["CGO_OBJ_QUAD_DIAG"] == 0
    return {k: num[k] for k in names}


def _facts(mode, kind, n_params):
    out = (C.c_int * 7)()
    sim_lib().sim_launch_mode(mode, kind, n_params, out)
    return dict(zip(("vectors", "reads_u", "writes_x", "writes_u", "writes_g", "has_sums", "big_only"), [out[0]] + [bool(v) for v in out[1:]]))


def _rows():
    return [(fam, mode) for fam in FAMILIES for mode, _ in I.rows(fam)]


def test_every_family_is_walked_and_every_row_is_in_the_table():
    assert [len(I.rows(f)) for f in FAMILIES] == [12, 4, 4, 2, 1, 10]
    assert {mode & ~R_LEAN for _, mode in _rows()} == set(VECTORS)
    assert all(mode & R_LEAN and mode & R_TRIAL for mode, _ in I.rows("CG_LEAN"))


@pytest.mark.parametrize("fam", FAMILIES)
def test_vector_counts_are_the_table(fam):
    """(a) reads + writes, per objective kind and parameter count; lean bits change nothing; (e) no row but R_EDGES streams nothing"""
    kinds = _kinds()
    for mode, _ in I.rows(fam):
        base, with_p = VECTORS[mode & ~R_LEAN]
        for name, kind in kinds.items():
            for n_params in range(5):
                p = max(1 if name == "CGO_OBJ_QUAD_DIAG" else 0, n_params)
                want = base + (p if with_p else 0)
                got = _facts(mode, kind, n_params)["vectors"]
                assert got == want, (fam, mode, name, n_params, got, want)
                assert (got == 0) == (mode == R_EDGES), (fam, mode, name, n_params)
                for lean in (R_LEAN, B["R_NOGTG"] | B["R_NOYY"] | B["R_NOUY"]):
                    assert _facts(mode | lean, kind, n_params)["vectors"] == want, (fam, mode, lean)


def test_sums_are_left_by_every_row_but_the_five():
    """(b)"""
    for fam, mode in _rows():
        assert _facts(mode, 0, 0)["has_sums"] == (mode not in NO_SUMS), (fam, mode)
    assert NO_SUMS <= {mode for _, mode in _rows()}


def test_big_only_is_the_lag_replay_and_lean_rows():
    """(c)"""
    for fam, mode in _rows():
        if fam in BIG_ONLY:
            assert _facts(mode, 0, 0)["big_only"], (fam, mode)
    big_only = {mode for fam, mode in _rows() if fam in BIG_ONLY}
    for fam, mode in _rows():
        assert _facts(mode, 0, 0)["big_only"] == (mode in big_only), (fam, mode)


def test_lag_and_replay_rows_store_what_the_table_says_they_store():
    """(d) cgo_instances.def, in file order — lag: A (x only), B (both), a trial (nothing), the materialise pass (u);
    replay: N (nothing), S (both), a trial (nothing), the materialise pass (both); the lean rows: N and S again"""
    def stores(fam):
        return [(f["writes_x"], f["writes_u"]) for f in (_facts(mode, 0, 0) for mode, _ in I.rows(fam))]
    assert [m for m, _ in I.rows("CG_LAG")] == [ADT | R_NOWU, R_ULAG | ADT, R_ULAG | R_TRIAL, R_ULAG]
    assert stores("CG_LAG") == [(True, False), (True, True), (False, False), (False, True)]
    assert [m for m, _ in I.rows("CG_REPLAY")] == [R_REPLAY | ADT | R_NOWU | R_NOWX, R_REPLAY | ADT, R_REPLAY | R_TRIAL, R_REPLAY]
    assert stores("CG_REPLAY") == [(False, False), (True, True), (False, False), (True, True)]
    assert stores("CG_LEAN") == [(False, False), (True, True)]


def test_reads_and_gradient_stores_of_the_plain_rows():
    """the remaining booleans, for the rows whose comments in csrc/cgo_modes.hpp say it outright"""
    for mode in (R_INIT, R_RESET, R_GRAD, R_EDGES):          # u is overwritten or not looked at
        assert not _facts(mode, 0, 0)["reads_u"], mode
    for fam, mode in _rows():
        if mode not in (R_INIT, R_RESET, R_GRAD, R_EDGES):
            assert _facts(mode, 0, 0)["reads_u"], (fam, mode)
        assert _facts(mode, 0, 0)["writes_g"] == (mode in (R_GRAD, R_GRADT)), (fam, mode)
    for mode, wx, wu in ((R_INIT, False, True), (R_RESET, False, True), (R_ACCEPT, True, False), (R_ACCEPT | R_DIR, True, True),
                         (ADT, True, True), (R_DIR, False, True), (R_DIR | R_TRIAL, False, True), (R_TRIAL, False, False),
                         (R_UPG, False, False), (R_PROJ, False, False), (R_EDGES, False, False)):
        f = _facts(mode, 0, 0)
        assert (f["writes_x"], f["writes_u"]) == (wx, wu), mode


def test_the_facts_are_stated_once():
    """the u-reading mask, the no-sums list and the BIG-only mask: spelled out in cgo_modes.hpp and nowhere else in csrc/;
    bytes_r has no per-mode branch"""
    texts = {f: open(os.path.join(I.CSRC, f)).read() for f in sorted(os.listdir(I.CSRC)) if f.endswith((".hpp", ".hip", ".def"))}
    pats = {"reads u": r"R_ACCEPT \| R_DIR \| R_TRIAL \| R_UPG \| R_GRADT", "no sums": r"!= R_GRAD && \w+ != R_GRADT|== R_GRAD \|\| \w+ == R_GRADT",
            "BIG only": r"R_ULAG \| R_NOWU \| R_REPLAY \| R_NOWX"}
    for what, pat in pats.items():
        assert [f for f, t in texts.items() if re.search(pat, t)] == ["cgo_modes.hpp"], what
    body = re.search(r"double bytes_r\(.*?\n\}", texts["cgo_backend_cg.hip"], re.S).group(0)
    assert "r_vectors(mode, p)" in body and "if" not in body and body.count("\n") <= 4, body
