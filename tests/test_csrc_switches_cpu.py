"""One kernel per source file: racformer_amd/csrc carries no build switches besides instrumentation and the reproducers of recorded
platform findings.  Every preprocessor conditional must either mention RAC_DIAGNOSTIC_BUILD -- it then exists only in
the builds of tools/build_variant.sh -- or test nothing but the allow-listed reproducer switches, and no `#ifndef NAME` /
`#define NAME value` pair offers a tuning value to the command line.  Source text only: nothing is compiled."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "racformer_amd", "csrc")

# reproducers of recorded platform findings, each with the DESIGN section that holds the finding
REPRODUCERS = {
    "RAC_GATHER_PACKED_FMA": "3.12",    # packed FP32 accumulation beside another stream's MFMA kernels: the evidence for -packed-fp32-ops
    "RAC_GATHER_LOADS_FIRST": "3.12",   # the same finding with every tap load issued before the first FMA
    "RAC_ABSMAX_MEMSET": "3.14",        # a memset node in the captured plan instead of the one-thread kernel
}

CONDITIONAL = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif)\b(.*)$")


def sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert files
    return files


def logical_lines(path):
    """(line number, text) with backslash continuations joined"""
    out, pending, start = [], "", 0
    for i, line in enumerate(open(path).read().split("\n"), 1):
        if not pending:
            start = i
        if line.endswith("\\"):
            pending += line[:-1] + " "
            continue
        out.append((start, pending + line))
        pending = ""
    return out


def conditionals():
    for path in sources():
        for no, line in logical_lines(path):
            m = CONDITIONAL.match(line)
            if m:
                cond = re.sub(r"//.*|/\*.*?\*/", "", m.group(2))
                yield f"{os.path.basename(path)}:{no}", line.strip(), set(re.findall(r"[A-Za-z_]\w*", cond)) - {"defined"}


def test_every_conditional_is_diagnostic_or_a_listed_reproducer():
    seen, bad = set(), []
    for where, line, names in conditionals():
        seen |= names
        if "RAC_DIAGNOSTIC_BUILD" not in names and not (names and names <= set(REPRODUCERS)):
            bad.append(f"{where}: {line}")
    assert not bad, "build switches in the product sources:\n" + "\n".join(bad)
    assert "RAC_DIAGNOSTIC_BUILD" in seen                      # (the scan does find conditionals)
    assert set(REPRODUCERS) <= seen, "allow-list entries nothing tests any more: " + ", ".join(sorted(set(REPRODUCERS) - seen))


def test_reproducers_are_recorded_in_design():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name, section in REPRODUCERS.items():
        start = design.index(f"\n### {section} ")
        end = design.index("\n### ", start + 1)
        assert name in design[start:end], f"{name} is not named in DESIGN {section}"


def test_no_overridable_default_values():
    bad = []
    for path in sources():
        lines = logical_lines(path)
        for (no, line), (_, nxt) in zip(lines, lines[1:]):
            m = re.match(r"^\s*#\s*ifndef\s+(\w+)", line)
            if m and m.group(1) not in REPRODUCERS and re.match(r"^\s*#\s*define\s+%s\b" % m.group(1), nxt):
                bad.append(f"{os.path.basename(path)}:{no}: {m.group(1)}")
    assert not bad, "#ifndef NAME / #define NAME pairs (make the value a plain #define):\n" + "\n".join(bad)
