"""What the library can launch: the rows of csrc/cgo_instances.def, the one table the launch switches, the run-time compiled
module's name list and obj_tname() are expanded from.  One row per line, `FAMILY(field, field)`; nothing else is parsed."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "conjugategradientoptim.jl_amd", "csrc")
# the mode bits of the k_cg / k_chain family (R_*) and of k_fused (M_*): as csrc/cgo_modes.hpp declares them (`NAME = number`)
BITS = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b([RM]_[A-Z]+) = (\d+)\b", open(os.path.join(CSRC, "cgo_modes.hpp")).read())}
assert BITS["R_ACCEPT"] == 1 and BITS["R_EDGES"] == 512 and len([k for k in BITS if k.startswith("R_")]) == 18, BITS
assert {k: v for k, v in BITS.items() if k.startswith("M_")} == dict(M_ACCEPT=1, M_DIR=2, M_TRIAL=4, M_BETA=8, M_INIT=16, M_RESET=32, M_UPG=64,
                                                                     M_BETAONLY=128), BITS   # the run-time compiled module's names carry these numbers


def _value(field):
    """a count or mode bits or-ed together as a number, anything else (a name, a key) as written"""
    terms = [t.strip() for t in field.split("|")]
    return sum(BITS.get(t) or int(t) for t in terms) if all(t in BITS or t.isdigit() for t in terms) else field.strip().strip('"')


def rows(family):
    """the fields of every row of `family` (CG, CHAIN, FUSED_OBJ, …), in file order"""
    text = open(os.path.join(CSRC, "cgo_instances.def")).read()
    return [tuple(_value(f) for f in m.group(1).split(",")) for m in re.finditer(r"^ +%s\((.*)\)(?: \\)?$" % family, text, re.M)]


def mode_points(family):
    """(mode, points) for the odd point counts up to each row's largest"""
    return {(mode, p) for mode, top in rows(family) for p in range(1, top + 1, 2)}


def stray_uses():
    """Every line of csrc/*.hip that launches, or takes the address of, a kernel of the table's families anywhere but in a
    `#define ROW(` expander of the table.  Strings (reported symbols, hiprtc names) and comments do not count."""
    text = "\n".join(open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")))).replace("\\\n", " ")
    code = [re.sub(r'"(?:\\.|[^"\\])*"', '""', line).split("//")[0] for line in text.split("\n")]
    return [c.strip() for c in code if re.search(r"\bk_(cg|cg_armed|chain|fused|resident|resident_chain|batch|batch_rows|batch_lbfgs|batch_grad)<", c) and not c.startswith("#define ROW(")]


def rtc_programs():
    """the programs of a run-time compiled objective's module, in file order: {RtcProgram: (file name, wording, text layers)}"""
    return {r[0]: r[1:] for r in rows("RTC_PROGRAM")}


def rtc_program_kernels(prog):
    """the name expressions of a further program of the module, in order and without `cgo::dev::`: its rows of RTC_KERNEL (one
    per NPTS of the row macro they name, `, true` for a PROBE twin), then its rows of RTC_EXTRA"""
    out = []
    for p, _prefix, kernel, macro, probe in rows("RTC_KERNEL"):
        if p == prog:
            family = re.match(r"CGO_(\w+)_ROWS$", macro).group(1)
            out += ["%s<UserObjective, %d%s>" % (kernel, npts, ", true" if probe else "") for (npts,) in rows(family)]
    return out + ["%s<UserObjective>" % kernel for p, _key, kernel in rows("RTC_EXTRA") if p == prog]


def rtc_compile_program_body():
    """the code of rtc_compile_program (cgo_rtc_batch.hip), THE function that compiles every further program"""
    text = open(os.path.join(CSRC, "cgo_rtc_batch.hip")).read()
    return re.search(r"^int rtc_compile_program\(RtcModule &m, RtcProgram prog, std::string &log\) \{\n.*?^}", text, re.M | re.S).group(0)


def every_program_module_is_unloaded():
    """RtcModule holds one handle per program, and its destructor unloads every one of them"""
    return ("hipModule_t mods[RTC_PROGRAMS] = {};" in open(os.path.join(CSRC, "cgo_rtc.hpp")).read()
            and re.search(r"RtcModule::~RtcModule\(\) \{\s*for \(hipModule_t m : mods\)\s*if \(m\) \(void\)hipModuleUnload\(m\);\s*\}",
                          open(os.path.join(CSRC, "cgo_rtc.hip")).read()) is not None)
