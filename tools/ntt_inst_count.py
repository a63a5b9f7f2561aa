#!/usr/bin/env python3
"""Static instruction counts of the NTT kernels (csrc/ntt.hip).

The passes are bound by instruction issue (DESIGN, "NTT passes"), so what a pass executes
besides its multiplies is its cost.  This tool cross-compiles ntt.hip to gfx950 assembly with
the library's flags (tools/acc_inst_count.py's assembly()) and prints, for every instantiated
kernel, the whole kernel's VALU total and its count by mnemonic, the ds_bpermute_b32 and
s_nop counts, and NumVgprs, ScratchSize and Occupancy as the compiler reports them.  The
counts are static: a persistent kernel's loop body is counted once.  It also lists every lane
swap that reads a register written inside an asm statement fewer than two wait states before
(swap_hazards: the compiler pads that hazard only for instructions it emitted itself).

    python tools/ntt_inst_count.py [--json] [--csrc DIR] [--kernel SUBSTRING] [-DNAME=VALUE ...]

tests/test_ntt_inst_count_cpu.py holds the counts against DESIGN's recorded values.
"""
import argparse
import collections
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acc_inst_count as A  # noqa: E402

_KERNEL = re.compile(r"^(_Z\w+):\s*; @")
_NAME = re.compile(r"^_ZN3h2g\d+(\w+?_kernel)(?:I((?:L[ib]\d+E)+)E)?")


def _short(sym):
    """ntt_pass29p_kernel<6>, ntt_last29_kernel<false,true>, ... from the mangled name"""
    m = _NAME.match(sym)
    if not m:
        return sym
    args = [a[1:] if t == "i" else ("true" if a[1:] == "1" else "false")
            for t, a in ((x[1], x[1:-1]) for x in re.findall(r"L[ib]\d+E", m.group(2) or ""))]
    return m.group(1) + ("<%s>" % ",".join(args) if args else "")


_SWAP = re.compile(r"^\s+(v_permlane\d+_swap_b32\w*|v_mov_b32_dpp)\s+(.*)$")
_VREG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")


def _vregs(text):
    out = set()
    for m in _VREG.finditer(text):
        out |= {int(m.group(1))} if m.group(1) else set(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def swap_hazards(asm):
    """Lane swaps (v_permlane*_swap, DPP moves) that read a register an asm statement wrote
    fewer than two wait states earlier -> [(line number, swap, writer)].  The compiler pads
    this hazard for its own instructions only, so inside-asm writers are what can slip.
    The scan walks back through straight-line code and stops at a label: a writer across a
    branch target or a loop's back-edge is not seen.  Every swap of ntt.hip follows round A's
    products in one basic block; a swap placed first in a block needs another check."""
    lines = asm.splitlines()
    bad = []
    for i, ln in enumerate(lines):
        m = _SWAP.match(ln)
        if not m:
            continue
        regs, states, inside, j = _vregs(m.group(2)), 0, False, i - 1
        while j >= 0 and states < 2:
            t = lines[j].strip()
            j -= 1
            if t.startswith(";;#ASMEND"):
                inside = True
            elif t.startswith(";;#ASMSTART"):
                inside = False
            elif t.endswith(":"):
                break
            elif A._INST.match(" " + t):
                if inside and t.startswith("v_") and _vregs(t.split(",")[0]) & regs:
                    bad.append((i + 1, ln.strip(), t))
                states += 1 + (int(t.split()[1]) if t.startswith("s_nop") else 0)
    return bad


def count(csrc=None, defs=(), asm=None):
    """{kernel name: counts} for every kernel of ntt.hip"""
    asm = asm or A.assembly(csrc, defs, source="ntt.hip")
    lines = asm.splitlines()
    starts = [(i, m.group(1)) for i, ln in enumerate(lines) for m in [_KERNEL.match(ln)] if m]
    kernels = [(i, n) for i, n in starts if re.search(r"\.amdhsa_kernel %s$" % re.escape(n), asm, re.M)]
    res = {}
    for (i, sym), name in zip(kernels, [_short(n) for _, n in kernels]):
        end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        c, other = collections.Counter(), collections.Counter()
        for ln in lines[i + 1:end]:
            m = A._INST.match(ln)
            if m:
                (c if m.group(1).startswith("v_") else other)[m.group(1)] += 1
        meta = {}
        for ln in lines[end:]:
            mm = A._META.match(ln)
            if mm and mm.group(1) not in meta:
                meta[mm.group(1)] = int(mm.group(2))
            if len(meta) == 3:
                break
        res[name] = {
            "valu": sum(c.values()),
            "mad": c[A.MAD],
            "by_mnemonic": dict(sorted(c.items(), key=lambda kv: (-kv[1], kv[0]))),
            "ds_bpermute": other["ds_bpermute_b32"],
            "s_nop": other["s_nop"],
            "s_waitcnt": other["s_waitcnt"],
            "NumVgprs": meta.get("NumVgprs"),
            "ScratchSize": meta.get("ScratchSize"),
            "Occupancy": meta.get("Occupancy"),
        }
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--json", action="store_true", help="one JSON object instead of the table")
    ap.add_argument("--csrc", help="another copy of the sources (a parent checkout's csrc)")
    ap.add_argument("--kernel", default="", help="only kernels whose name contains this")
    args, defs = ap.parse_known_args()
    asm = A.assembly(args.csrc, defs, source="ntt.hip")
    res = {k: v for k, v in count(asm=asm).items() if args.kernel in k}
    hazards = swap_hazards(asm)
    if args.json:
        print(json.dumps({"kernels": res, "swap_hazards": hazards}))
        return
    for name, r in res.items():
        print(name)
        print(f"  VALU {r['valu']}  {A.MAD} {r['mad']}  ds_bpermute {r['ds_bpermute']}  s_nop {r['s_nop']}"
              f"  s_waitcnt {r['s_waitcnt']}")
        print(f"  NumVgprs {r['NumVgprs']}  ScratchSize {r['ScratchSize']}  Occupancy {r['Occupancy']}")
        top = [f"{v} {k}" for k, v in r["by_mnemonic"].items() if k != A.MAD][:8]
        print("  " + ", ".join(top))
    print(f"lane swaps within two wait states of an asm write of their operand: {len(hazards)}")
    for h in hazards:
        print("  line %d: %s  <-  %s" % h)


if __name__ == "__main__":
    main()
