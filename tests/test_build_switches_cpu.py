"""The build-time switches of csrc/ against DESIGN.md's "Build-time constants" table.

Every H2G_* macro that the sources test (#ifndef, #ifdef, #if, #elif, defined(...)) must have
a row in the table, and every row a macro: a new switch needs a DESIGN row, where a reviewer
sees it, and a deleted one takes its row along.  Include guards (a macro that the line after
its #ifndef defines to nothing) are left out.
"""
import glob
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "yet-another-halo2-fork_amd", "csrc")
NAME = r"H2G_[A-Z0-9_]+"


def macros_tested(text):
    lines = text.splitlines()
    found = set()
    for i, line in enumerate(lines):
        m = re.match(r"\s*#\s*(ifndef|ifdef|if|elif)\b(.*)", line)
        if not m:
            continue
        names = re.findall(NAME, m.group(2).split("//")[0])
        if m.group(1) == "ifndef" and names and i + 1 < len(lines):
            if re.fullmatch(r"\s*#\s*define\s+%s\s*" % re.escape(names[0]), lines[i + 1].split("//")[0]):
                continue  # include guard
        found.update(names)
    return found


def source_switches():
    found = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        with open(path, errors="replace") as f:
            found |= macros_tested(f.read())
    return found


def design_rows():
    with open(os.path.join(REPO, "DESIGN.md")) as f:
        text = f.read()
    m = re.search(r"^### Build-time constants\n(.*?)(?=^#{2,3} )", text, re.M | re.S)
    assert m, "DESIGN.md has no 'Build-time constants' section"
    rows = re.findall(r"^\| `(%s)` \|" % NAME, m.group(1), re.M)
    assert len(rows) == len(set(rows)), "a switch has two rows"
    return set(rows)


def test_parser_sees_every_form_and_skips_guards():
    text = "\n".join([
        "#ifndef H2G_GUARD_H", "#define H2G_GUARD_H", "#endif",
        "#ifndef H2G_A  // comment naming H2G_NOT_ME", "#define H2G_A 1", "#endif",
        "#ifdef H2G_B", "#endif",
        "#if H2G_C > 1 || defined(H2G_D)", "#elif defined H2G_E", "#endif",
        "  if (H2G_PLAIN_USE) {}",
    ])
    assert macros_tested(text) == {"H2G_A", "H2G_B", "H2G_C", "H2G_D", "H2G_E"}


def test_every_switch_has_a_design_row():
    src, doc = source_switches(), design_rows()
    assert src, "no switch found under csrc/ (moved sources?)"
    assert src == doc, f"only in csrc/: {sorted(src - doc)}; only in DESIGN.md: {sorted(doc - src)}"
