#!/usr/bin/env python3
"""Generate csrc/f29_asm.inc: the F29 Montgomery products as single asm blocks.

A product written in C++ pays either a 64-bit join per column (the compiler starts every
column from 0 and adds the carry afterwards) or, with every multiply-add pinned by an empty
asm, one wait state per pin (DESIGN, "The accumulation's issue cost").  Written as ONE asm
statement the product is a plain chain -- the shifted carry is the first addend of the next
column's first v_mad_u64_u32 -- and pays the compiler's boundary pad once.

Each block computes exactly the integers of f29.h's mul29 / sqr29 / mul29x2: the same column
sums, the same m_k, the same output limbs.  Per column k < 9: the a.b multiply-adds, the
m_i M_(k-i) multiply-adds, m_k = (lo32(acc) * INV) & MASK, acc += m_k M_0, acc >>= 29; per
column 9 <= k < 17: the multiply-adds, r_(k-9) = lo32(acc) & MASK, acc >>= 29; r_8 = lo32(acc).

Registers.  m_k lives in output register r_k: m_(k-9) is last read in column k - 1 and r_(k-9)
is written in column k (m_8 gives way to r_8 after column 16), so the outputs are the only
temporaries and all are early-clobber.  The in-place blocks (_IP) instead write r_j over
limb j of one input, which is last read in column j + 8, and keep m_k in nine temporaries: no
more registers, and no copies where a loop-carried value is multiplied.
The 64-bit accumulator has to be readable as a pair (multiply-add, shift) and as its low
half alone (v_mul_lo_u32, v_and_b32, the closing move);
an asm operand prints only as the whole pair, so the accumulator is a fixed pair named in the
text and in the clobber list (ACC: the first product's, ACC2: the second's of a pair block).
M's limbs, INV and the mask are SGPR operands (VOP3 takes no 32-bit literal on gfx9; one
SGPR per instruction keeps within the constant-bus limit).

Only v_mad_u64_u32, v_mul_lo_u32, v_and_b32, v_lshrrev_b64 and v_mov_b32 appear, in the
register patterns the compiler emits for the C++ forms (accumulator pair as destination and
addend included), so no pair of them needs a wait state.

Order matters to one user.  A block's last write is its top limb (the closing move) and every
other output limb is written at least two instructions before the block ends.  ntt.hip relies
on exactly that: v_permlane*_swap must not read a register within two wait states of its
write, the compiler does not count states behind writes made inside an asm statement, and
WaveDif29::run therefore passes only the top limbs of the products that feed the swaps through
an `s_nop 1` statement.  A change to the instruction order here that moves another output
write into a block's last two instructions breaks that on the GPU without any error;
tools/ntt_inst_count.py's swap_hazards (held empty by tests/test_ntt_inst_count_cpu.py) is
the only check, so run it after any change to this file.

    python tools/f29_asm_gen.py            # rewrite csrc/f29_asm.inc
    python tools/f29_asm_gen.py --check    # exit 1 if the committed file differs
    python tools/f29_asm_gen.py --stdout

tests/test_f29_asm_cpu.py interprets every block over Python integers.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "yet-another-halo2-fork_amd", "csrc", "f29_asm.inc")

ACC = ("v2", "v3")   # accumulator pair of a block (of the first product of a pair block)
ACC2 = ("v4", "v5")  # accumulator pair of the second product of a pair block


def _pair(acc):
    return "v[%s:%s]" % (acc[0][1:], acc[1][1:])


def product(terms, acc=ACC, pre="", inplace=None):
    """Instruction list of REDC(sum of the products in `terms`).

    terms: list over k = 0..16 of lists of (x, y) operand names (without pre) whose
    products x * y make up column k.  pre prefixes every operand name but the constants.
    inplace: the input (e.g. "a") whose registers take the result -- its limb j is last read
    in column j + 8 and r_j is written in column j + 9 -- with m_k in temporaries m0..m8.
    """
    A, lo = _pair(acc), acc[0]
    op = lambda n: "%%[%s%s]" % (pre, n)
    m = lambda k: op(("m%d" if inplace else "r%d") % k)
    r = lambda j: op("%s%d" % (inplace or "r", j))
    out = []

    def mad(x, y):
        out.append("v_mad_u64_u32 %s, vcc, %s, %s, %s" % (A, x, y, A if out else "0"))

    for k in range(17):
        for x, y in terms[k]:
            mad(op(x), op(y))
        if k < 9:
            for i in range(k):
                mad(m(i), "%%[M%d]" % (k - i))
            out.append("v_mul_lo_u32 %s, %s, %%[INV]" % (m(k), lo))
            out.append("v_and_b32 %s, %%[MASK], %s" % (m(k), m(k)))
            mad(m(k), "%[M0]")
        else:
            for i in range(k - 8, 9):
                mad(m(i), "%%[M%d]" % (k - i))
            out.append("v_and_b32 %s, %%[MASK], %s" % (r(k - 9), lo))
        out.append("v_lshrrev_b64 %s, 29, %s" % (A, A))
    out.append("v_mov_b32 %s, %s" % (r(8), lo))
    return out


def mul_terms(a="a", b="b"):
    return [[("%s%d" % (a, i), "%s%d" % (b, k - i)) for i in range(max(0, k - 8), min(k, 8) + 1)] for k in range(17)]


def sqr_terms():
    """a^2 against the doubled limbs d_i = 2 a_i (inputs d0..d7): cross products once"""
    t = []
    for k in range(17):
        col = [("d%d" % i, "a%d" % (k - i)) for i in range(max(0, k - 8), 9) if 2 * i < k]
        if k % 2 == 0:
            col.append(("a%d" % (k // 2), "a%d" % (k // 2)))
        t.append(col)
    return t


def mul_x2_terms():
    ab, cd = mul_terms("a", "b"), mul_terms("c", "d")
    return [[p for pq in zip(ab[k], cd[k]) for p in pq] for k in range(17)]


def interleave(p, q):
    assert len(p) == len(q)
    return [x for pq in zip(p, q) for x in pq]


def blocks():
    return {
        "H2G_ASM_MUL29": product(mul_terms()),
        "H2G_ASM_SQR29": product(sqr_terms()),
        "H2G_ASM_MUL29X2": product(mul_x2_terms()),
        # a <- REDC(a b) and c <- REDC(a b + c d) in the registers of a / of c
        "H2G_ASM_MUL29_IP": product(mul_terms(), inplace="a"),
        "H2G_ASM_MUL29X2_IP": product(mul_x2_terms(), inplace="c"),
        # two independent products, their chains alternating instruction by instruction
        "H2G_ASM_MUL29_PAIR": interleave(product(mul_terms(), ACC), product(mul_terms(), ACC2, "x")),
    }


def render():
    o = ["// f29_asm.inc -- generated by tools/f29_asm_gen.py; do not edit (the generator's header",
         "// explains the blocks; tests/test_f29_asm_cpu.py interprets them).  One instruction per line.",
         "#define H2G_ASM_ACC_CLOBBER \"%s\", \"%s\"" % ACC,
         "#define H2G_ASM_ACC2_CLOBBER \"%s\", \"%s\"" % ACC2]
    for name, ins in blocks().items():
        o.append("#define %s \\" % name)
        for i, s in enumerate(ins):
            o.append('  "%s\\n\\t"%s' % (s, " \\" if i + 1 < len(ins) else ""))
    return "\n".join(o) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--stdout", action="store_true")
    args = ap.parse_args()
    text = render()
    if args.stdout:
        sys.stdout.write(text)
    elif args.check:
        with open(OUT) as f:
            sys.exit(0 if f.read() == text else 1)
    else:
        with open(OUT, "w") as f:
            f.write(text)
        for name, ins in blocks().items():
            print("%s: %d instructions" % (name, len(ins)))


if __name__ == "__main__":
    main()
