"""CPU tier of the two tables every batched solve is dispatched from: the tiers of a batch (batch_tier_of, cgo_backend_batch.hip) and
the programs of a run-time compiled objective's module (CGO_RTC_PROGRAM_ROWS / _KERNEL_ROWS / _EXTRA_ROWS, cgo_instances.def).
Text only: nothing here needs the library or a device."""
import glob
import os
import re

import _instances as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAMS = ["RTC_CREATE", "RTC_RESIDENT_PROBE", "RTC_BATCH", "RTC_BATCH_ROWS", "RTC_BATCH_PROBE", "RTC_BATCH_LBFGS", "RTC_BATCH_LBFGS_LDS"]


def _read(name):
    return open(os.path.join(I.CSRC, name), encoding="utf-8").read()


def tier_rows():
    """the rows of the tier table in tier order: (family, lookup, program, key prefix, PROBE program, PROBE key prefix, qn, LDS
    rows).  Each stands in the translation unit of its tier (tier_row_…); batch_tier_of (cgo_backend_batch.hip) orders them."""
    order = re.search(r"^const BatchTierRow &batch_tier_of\(BatchTier tier\) \{\n(.*?)^}", _read("cgo_backend_batch.hip"), re.M | re.S).group(1)
    cases = re.findall(r"(?:case BatchTier::(\w+)|default): return (tier_row_\w+)\(\);", order)
    assert [c[0] for c in cases] == ["LDS", "ROWS", "LBFGS", ""]
    units = "".join(_read(os.path.basename(p)) for p in sorted(glob.glob(os.path.join(I.CSRC, "cgo_backend_batch*.hip"))))
    rows = []
    for _tier, fn in cases:
        m = re.findall(r'^const BatchTierRow &%s\(\) \{\n    static const BatchTierRow row = \{"(\w+)", (\w+), (\w+), "([\w:]+)", (\w+), (?:"([\w:]+)"|nullptr), (true|false), (.+),$' % fn, units, re.M)
        assert len(m) == 1, fn
        f, a, p, k, pp, pk, qn, lds = m[0]
        rows.append((f, a, p, k, pp, pk or None, qn == "true", lds))
    return rows


def test_the_tier_numbers_are_the_headers():
    tiers = tier_rows()
    assert len(tiers) == 4
    enum = re.search(r"enum class BatchTier : int \{([^}]*)\}", _read("cgo_hip_backend.hpp")).group(1)
    assert [t.strip() for t in enum.split(",")] == ["LDS = 0", "ROWS = 1", "LBFGS = 2", "LBFGS_LDS = 3"]
    assert "constexpr int BATCH_TIERS = 4;" in _read("cgo_hip_backend.hpp")
    hdr = open(os.path.join(ROOT, "include", "cgo.h"), encoding="utf-8").read()
    documented = {int(n): fam for n, fam in re.findall(r"\btier (\d)  (k_\w+)", hdr)}
    assert documented == {i: t[0] for i, t in enumerate(tiers)}   # row i of the table is cgo_batch_probe_args.tier == i
    # the probe takes the batch's own row and refuses any other tier number
    probe = _read("cgo_backend_batch_probe.hip")
    assert "if (tier != (int)bat_tier_)" in probe and "t.family" in probe and "tier == " not in re.sub(r"//.*", "", probe)
    assert [t[6] for t in tiers] == [False, False, True, True]
    assert [t[7] for t in tiers] == ["[](int K, int) { return batch_vecs(K); }", "[](int, int) { return 0; }", "[](int, int) { return 0; }",
                                     "HipBackend::batch_lbfgs_lds_rows"]


def test_each_tier_names_kernels_its_program_holds():
    keyed = {(p, prefix): kernel for p, prefix, kernel, _macro, probe in I.rows("RTC_KERNEL") if not probe}
    twins = {(p, prefix): kernel for p, prefix, kernel, _macro, probe in I.rows("RTC_KERNEL") if probe}
    for family, lookup, prog, key, probe_prog, probe_key, _qn, _lds in tier_rows():
        assert keyed[(prog, key)] == family, family
        assert "%s<UserObjective, 3>" % family in I.rtc_program_kernels(prog)
        assert re.search(r"^static RowPick %s\(int obj_kind, int npts\) \{ return row_pick_for<\w+>\(obj_kind, npts\); \}$" % lookup,
                         "".join(_read(os.path.basename(p)) for p in glob.glob(os.path.join(I.CSRC, "cgo_backend_batch*.hip"))), re.M), lookup
        if family in ("k_batch", "k_batch_rows"):
            assert twins[(probe_prog, probe_key)] == family and probe_prog == "RTC_BATCH_PROBE"
        else:   # the user L-BFGS kernels have no PROBE twin: cgo_batch_probe refuses a model there
            assert (probe_prog, probe_key) == ("RTC_NONE", None), family
    assert sorted(twins.values()) == ["k_batch", "k_batch_rows", "k_resident"]
    # … in the C API's own words, where it was
    assert 'REQUIRE(p->tier < 2, "batch probe: the batched L-BFGS kernels of a run-time compiled objective have no PROBE twin (tiers 0 and 1)");' in _read("cgo_capi_batch.hip")


def test_every_further_program_is_compiled_in_one_place():
    assert list(I.rtc_programs()) == PROGRAMS
    enum = re.search(r"enum RtcProgram \{(.*?)\};", _read("cgo_rtc.hpp"), re.S).group(1)
    assert re.findall(r"^\s*(RTC_\w+)", enum, re.M) == ["RTC_NONE"] + PROGRAMS + ["RTC_PROGRAMS"]
    names = [v[0] for v in I.rtc_programs().values()]
    assert names == ["cgo_user_objective.hip", "cgo_user_objective_probe.hip", "cgo_user_objective_batch.hip", "cgo_user_objective_batch_rows.hip",
                     "cgo_user_objective_batch_probe.hip", "cgo_user_objective_batch_lbfgs.hip", "cgo_user_objective_batch_lbfgs_lds.hip"]
    for prog in PROGRAMS[1:]:
        assert I.rtc_program_kernels(prog), prog
    assert I.rtc_program_kernels("RTC_CREATE") == []   # (its kernels are the per-objective rows: rtc_create_wants)
    # rtc_build — what hands a program to hiprtc — is called by the creation of an objective and by rtc_compile_program alone
    code = {os.path.basename(p): re.sub(r"//.*", "", open(p, encoding="utf-8").read()) for p in glob.glob(os.path.join(I.CSRC, "*.hip"))}
    calls = {name: len(re.findall(r"(?<!int )\brtc_build\(", text)) for name, text in code.items()}
    assert {n: c for n, c in calls.items() if c} == {"cgo_rtc.hip": 1, "cgo_rtc_batch.hip": 1}
    body = I.rtc_compile_program_body()
    assert body.count("rtc_build(") == 1 and "std::lock_guard<std::mutex> lock(m.mu);" in body and "prog <= RTC_CREATE" in body
    assert "mods[RTC_CREATE]" in code["cgo_rtc.hip"] and "std::mutex mu;" in _read("cgo_rtc.hpp")
    assert I.every_program_module_is_unloaded()
    # the lookups take no lock
    lookups = _read("cgo_rtc_batch.hip").split("// ---- the lookups")[1]
    assert "lock" not in lookups and "mutex" not in lookups


def test_nothing_of_the_copies_survives():
    gone = ("rtc_compile_batch", "rtc_compile_batch_rows", "rtc_compile_batch_probe", "rtc_compile_batch_lbfgs", "rtc_compile_batch_lbfgs_lds",
            "rtc_compile_resident_probe", "batch_mod", "rows_mod", "probe_mod", "batch_probe_mod", "batch_lbfgs_mod", "batch_lbfgs_lds_mod",
            "bat_rows_", "bat_qn_lds_", "batch_lbfgs_launch", "batch_lbfgs_lds_launch", "batch_lbfgs_lds_on", "BatchProgram", "PROG_BATCH",
            "gen_rtc_lbfgs_sources", "gen_rtc_lbfgs_lds_sources", "cgo_rtc_batch_lbfgs", "cgo_rtc_batch_lbfgs_lds")
    for path in sorted(glob.glob(os.path.join(I.CSRC, "*"))):
        if os.path.isfile(path):
            text = open(path, encoding="utf-8").read()
            assert "_mod = nullptr" not in text, os.path.basename(path)
            for word in gone:   # (as whole identifiers)
                assert not re.search(r"(?<![A-Za-z0-9_])" + re.escape(word) + r"(?![A-Za-z0-9_])", text), (os.path.basename(path), word)
    assert not [p for p in os.listdir(I.CSRC) if re.match(r"gen_rtc_.*\.py$", p) and p != "gen_rtc_sources.py"]
    assert sorted(p for p in os.listdir(I.CSRC) if p.startswith("cgo_rtc")) == ["cgo_rtc.hip", "cgo_rtc.hpp", "cgo_rtc_batch.hip"]
    for once in ("#define CGO_STR2(x)", "#define ROW_NPTS(NPTS)", "std::string rtc_batch_lbfgs_defines() {"):
        assert sum(_read(os.path.basename(p)).count(once) for p in glob.glob(os.path.join(I.CSRC, "*.h*"))) == 1, once
