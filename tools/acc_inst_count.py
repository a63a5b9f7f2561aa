#!/usr/bin/env python3
"""Static instruction count of the MSM accumulation's hot loop (csrc/msm_acc.hip).

msm_acc_kernel is bound by instruction issue (DESIGN, "The accumulation's issue cost"), so
its cost is the number of vector ALU instructions one mixed addition executes, weighted by
their issue cycles.  This tool cross-compiles msm_acc.hip to gfx950 assembly with the
library's flags and prints, for the hot loop of msm_acc_kernel,
  * the VALU total (every instruction whose mnemonic starts with v_),
  * the v_mad_u64_u32 count and the other VALU instructions by mnemonic,
and for the kernel NumVgprs, ScratchSize and Occupancy as the compiler reports them.

The hot loop is the loop of the kernel (a label and the last backward branch to it) that
holds the most v_mad_u64_u32; of several with the same count, the widest.  Blocks the
compiler places behind the loop's backward branch (rare paths) are not counted; the whole
kernel's totals are printed beside the loop's so that a block that moved is seen.

    python tools/acc_inst_count.py [--json] [--csrc DIR] [--kernel NAME] [-DNAME=VALUE ...]

tests/test_acc_inst_count_cpu.py holds the counts against DESIGN's recorded values.
"""
import argparse
import collections
import json
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "yet-another-halo2-fork_amd"))
import build_lib as B  # noqa: E402

MAD = "v_mad_u64_u32"
_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")
_INST = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")
_META = re.compile(r"^;\s*(NumVgprs|ScratchSize|Occupancy):\s*(\d+)")


def assembly(csrc=None, defs=(), source="msm_acc.hip"):
    """gfx950 assembly of `source` with the library's flags (device side only)"""
    csrc = csrc or B.CSRC
    flags = [f for f in B.CFLAGS if f != "-fPIC"]
    if csrc != B.CSRC:
        flags = [csrc if f == B.CSRC else f for f in flags]
    cmd = [B.HIPCC] + flags + list(defs) + ["-x", "hip", "--cuda-device-only", "-S", os.path.join(csrc, source),
                                              "-o", "-"]
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernel_lines(asm, kernel):
    """the lines of `kernel`'s body and the metadata comments that follow it"""
    lines = asm.splitlines()
    start = None
    for i, ln in enumerate(lines):
        if start is None:
            if re.match(r"^_Z\w*%s\w*:" % re.escape(kernel), ln):
                start = i + 1
        elif ln.startswith(".Lfunc_end"):
            body = lines[start:i]
            meta = {}
            for m in lines[i:]:
                mm = _META.match(m)
                if mm and mm.group(1) not in meta:
                    meta[mm.group(1)] = int(mm.group(2))
                if len(meta) == 3:
                    break
            return body, meta
    raise SystemExit(f"kernel {kernel} not found in the assembly")


def _valu(lines):
    c = collections.Counter()
    for ln in lines:
        m = _INST.match(ln)
        if m and m.group(1).startswith("v_"):
            c[m.group(1)] += 1
    return c


def hot_loop(body):
    """(first line, last line) of the loop holding the most mads (ties: the widest)"""
    where = {}
    for i, ln in enumerate(body):
        m = _LABEL.match(ln)
        if m:
            where[m.group(1)] = i
    last_back = {}
    for i, ln in enumerate(body):
        m = _BRANCH.match(ln)
        if m and where.get(m.group(1), i) < i:
            last_back[m.group(1)] = i
    best = None
    for lab, end in last_back.items():
        a = where[lab]
        mads = sum(1 for ln in body[a:end + 1] if _INST.match(ln) and _INST.match(ln).group(1) == MAD)
        key = (mads, end - a)
        if best is None or key > best[0]:
            best = (key, a, end, lab)
    if best is None or best[0][0] == 0:
        raise SystemExit("no loop with a wide multiply found")
    return best[1], best[2], best[3]


def count(csrc=None, defs=(), kernel="msm_acc_kernel"):
    body, meta = kernel_lines(assembly(csrc, defs), kernel)
    a, b, lab = hot_loop(body)
    loop, whole = _valu(body[a:b + 1]), _valu(body)
    return {
        "kernel": kernel,
        "loop_label": lab,
        "valu": sum(loop.values()),
        "mad": loop[MAD],
        "other": sum(loop.values()) - loop[MAD],
        "by_mnemonic": dict(sorted(((k, v) for k, v in loop.items() if k != MAD), key=lambda kv: (-kv[1], kv[0]))),
        "kernel_valu": sum(whole.values()),
        "kernel_mad": whole[MAD],
        "NumVgprs": meta.get("NumVgprs"),
        "ScratchSize": meta.get("ScratchSize"),
        "Occupancy": meta.get("Occupancy"),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--json", action="store_true", help="one JSON object instead of the table")
    ap.add_argument("--csrc", help="another copy of the sources (a parent checkout's csrc)")
    ap.add_argument("--kernel", default="msm_acc_kernel")
    args, defs = ap.parse_known_args()
    r = count(args.csrc, defs, args.kernel)
    if args.json:
        print(json.dumps(r))
        return
    print(f"{r['kernel']}: hot loop {r['loop_label']}")
    print(f"  VALU {r['valu']}  {MAD} {r['mad']}  other {r['other']}"
          f"   (whole kernel: VALU {r['kernel_valu']}, {MAD} {r['kernel_mad']})")
    print(f"  NumVgprs {r['NumVgprs']}  ScratchSize {r['ScratchSize']}  Occupancy {r['Occupancy']}")
    for k, v in r["by_mnemonic"].items():
        print(f"  {v:5d}  {k}")


if __name__ == "__main__":
    main()
