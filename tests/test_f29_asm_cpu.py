"""csrc/f29_asm.inc, the F29 products as single asm blocks, interpreted over Python integers.

The blocks (tools/f29_asm_gen.py) are the device side of mul29_acc, sqr29_acc, mul29x2_acc,
their in-place forms and mul29_pair.  They use five mnemonics, so a twenty-line interpreter
runs every line of them: at the worst-case operands of the bounds model (limbs at their
maxima, top limbs below 2^31, mul29x2's middle column near 2^64) and at 1000 random
operands.  Each block must give big-integer REDC (congruent, below x / R + M, limbs 0..7
normalised) and exactly the limbs of the C++ forms, which tests/native/f29_host.cpp runs on
the host; no 64-bit accumulator may wrap.  The committed file must be what the generator emits.
"""
import os
import random
import re
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "yet-another-halo2-fork_amd", "csrc")
sys.path.insert(0, os.path.join(REPO, "tools"))
import f29_asm_gen as G  # noqa: E402
import f29_bounds as F  # noqa: E402

RR = 1 << 261
MASK = (1 << 29) - 1
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
MNEMONICS = {"v_mad_u64_u32", "v_mul_lo_u32", "v_and_b32", "v_lshrrev_b64", "v_mov_b32"}


def limbs(v):
    return [(v >> (29 * i)) & MASK for i in range(8)] + [v >> 232]


def val(ls):
    return sum(int(x) << (29 * i) for i, x in enumerate(ls))


def consts(m):
    c = {"M%d" % i: x for i, x in enumerate(limbs(m))}
    c["INV"] = (-pow(m, -1, 1 << 29)) % (1 << 29)
    c["MASK"] = MASK
    return c


def blocks_of(text):
    """{macro name: [instruction, ...]} of the .inc file"""
    out, cur = {}, None
    for ln in text.splitlines():
        m = re.match(r"#define (H2G_ASM_\w+) \\$", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = re.match(r'\s*"(.*)\\n\\t"( \\)?$', ln)
        if m and cur is not None:
            cur.append(m.group(1))
            if not m.group(2):
                cur = None
    return out


def interpret(ins, regs):
    """run the block on regs (operand name or physical register -> 32-bit integer)"""
    def rd(t):
        if re.fullmatch(r"\d+", t):
            return int(t)
        m = re.fullmatch(r"v\[(\d+):(\d+)\]", t)
        if m:
            return regs["v" + m.group(1)] | regs["v" + m.group(2)] << 32
        return regs[t[2:-1] if t.startswith("%[") else t]

    def wr(t, v):
        m = re.fullmatch(r"v\[(\d+):(\d+)\]", t)
        if m:
            assert 0 <= v < 1 << 64, "a 64-bit accumulator wrapped"
            regs["v" + m.group(1)], regs["v" + m.group(2)] = v & 0xFFFFFFFF, v >> 32
        else:
            assert 0 <= v < 1 << 32
            regs[t[2:-1] if t.startswith("%[") else t] = v

    for line in ins:
        op, rest = line.split(None, 1)
        a = [x.strip() for x in rest.split(",")]
        assert op in MNEMONICS, op
        if op == "v_mad_u64_u32":
            assert a[1] == "vcc"
            wr(a[0], rd(a[2]) * rd(a[3]) + rd(a[4]))
        elif op == "v_mul_lo_u32":
            wr(a[0], rd(a[1]) * rd(a[2]) & 0xFFFFFFFF)
        elif op == "v_and_b32":
            wr(a[0], rd(a[1]) & rd(a[2]))
        elif op == "v_lshrrev_b64":
            wr(a[0], rd(a[2]) >> rd(a[1]))
        else:
            wr(a[0], rd(a[1]))
    return regs


def run_block(ins, m, out, **operands):
    regs = dict(consts(m))
    for name, ls in operands.items():
        regs.update({"%s%d" % (name, i): x for i, x in enumerate(ls)})
    interpret(ins, regs)
    return [regs["%s%d" % (out, i)] for i in range(9)]


def redc_ok(o, x, m):
    v = val(o)
    assert all(l < 1 << 29 for l in o[:8]), o
    assert (v - x * pow(RR, -1, m)) % m == 0
    assert v < x // RR + m + 1


@pytest.fixture(scope="module")
def blocks():
    with open(os.path.join(CSRC, "f29_asm.inc")) as f:
        return blocks_of(f.read())


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the C++ forms' limbs: tests/native/f29_host.cpp built for the host"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    exe = tmp_path_factory.mktemp("f29asm") / "f29_host"
    subprocess.run([HIPCC, "--offload-host-only", "-O2", "-std=c++17", "-I", CSRC,
                    os.path.join(REPO, "tests", "native", "f29_host.cpp"), "-o", str(exe)],
                   check=True, cwd=str(exe.parent))

    def go(cmds):
        text = "\n".join(op + " " + " ".join(str(x) for x in args) for op, args in cmds) + "\n"
        rows = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(rows) == len(cmds) and not any(r.startswith("ERR") for r in rows)
        return [[int(x) for x in r.split()] for r in rows]
    return go


def test_inc_is_what_the_generator_emits(blocks):
    with open(os.path.join(CSRC, "f29_asm.inc")) as f:
        assert f.read() == G.render()
    assert blocks == G.blocks()
    # the single product: 162 multiply-adds, 9 v_mul_lo_u32, 17 v_and_b32, 17 shifts, the move
    ops = [i.split()[0] for i in blocks["H2G_ASM_MUL29"]]
    assert {o: ops.count(o) for o in MNEMONICS} == {"v_mad_u64_u32": 162, "v_mul_lo_u32": 9, "v_and_b32": 17,
                                                    "v_lshrrev_b64": 17, "v_mov_b32": 1}
    for ins in blocks.values():
        assert {i.split()[0] for i in ins} <= MNEMONICS


def _mul_cases(m, rng):
    # mul29's column bound (limbs below 2^30, top limb below 2^31) against a normalised
    # operand: the output stays below 2^264, its top limb below 2^32 (mul29's contract)
    wide = [(1 << 30) - 1] * 8 + [(1 << 31) - 1]
    top = [MASK] * 9
    fixed = [(wide, top), (top, wide), (wide, limbs(m - 1)), (limbs(m - 1), wide), (top, top), ([2 * MASK] * 9, top),
             (limbs(0), wide), (limbs(1), limbs(1)), (limbs(m - 1), limbs(m - 1))]
    rnd = [([rng.getrandbits(30) for _ in range(8)] + [rng.getrandbits(31)],
            [rng.getrandbits(29) for _ in range(9)])[::rng.choice((1, -1))] for _ in range(1000)]
    return fixed + rnd


@pytest.mark.parametrize("fld", ["q", "r"])
def test_mul_blocks(blocks, host, fld):
    m = F.M if fld == "q" else F.MR
    cases = _mul_cases(m, random.Random(41))
    want = host([("mul" + fld, a + b) for a, b in cases])
    for (a, b), w in zip(cases, want):
        o = run_block(blocks["H2G_ASM_MUL29"], m, "r", a=a, b=b)
        redc_ok(o, val(a) * val(b), m)
        assert o == w
        assert run_block(blocks["H2G_ASM_MUL29_IP"], m, "a", a=a, b=b) == w
    # the pair block: two different products at once, each as the single block gives it
    for (a, b), (c, d), w0, w1 in zip(cases[::2], cases[1::2], want[::2], want[1::2]):
        regs = dict(consts(m))
        for name, ls in (("a", a), ("b", b), ("xa", c), ("xb", d)):
            regs.update({"%s%d" % (name, i): x for i, x in enumerate(ls)})
        interpret(blocks["H2G_ASM_MUL29_PAIR"], regs)
        assert [regs["r%d" % i] for i in range(9)] == w0
        assert [regs["xr%d" % i] for i in range(9)] == w1


@pytest.mark.parametrize("fld", ["q", "r"])
def test_sqr_block(blocks, host, fld):
    m = F.M if fld == "q" else F.MR
    rng = random.Random(42)
    cases = [[MASK] * 8 + [(1 << 30) - 1], [MASK] * 9, limbs(0), limbs(1), limbs(m - 1)]
    cases += [[rng.getrandbits(29) for _ in range(8)] + [rng.getrandbits(30)] for _ in range(1000)]
    want = host([("sqr" + fld, a) for a in cases])
    for a, w in zip(cases, want):
        o = run_block(blocks["H2G_ASM_SQR29"], m, "r", a=a, d=[2 * x for x in a[:8]])
        redc_ok(o, val(a) ** 2, m)
        assert o == w


@pytest.mark.parametrize("fld", ["q", "r"])
def test_mul_x2_blocks(blocks, host, fld):
    """a, c normalised, b, d limbs just below 1.5 * 2^30: the middle column sits at ~2^63.98"""
    m = F.M if fld == "q" else F.MR
    rng = random.Random(43)
    big = [3 * (1 << 29) - 1] * 9
    cases = [([MASK] * 9, big, [MASK] * 9, big)]
    for _ in range(1000):
        a = [rng.choice((MASK, rng.getrandbits(29))) for _ in range(9)]
        c = [rng.choice((MASK, rng.getrandbits(29))) for _ in range(9)]
        b = [rng.choice((3 * (1 << 29) - 1, rng.randrange(3 << 29))) for _ in range(9)]
        d = [rng.choice((3 * (1 << 29) - 1, rng.randrange(3 << 29))) for _ in range(9)]
        cases.append((a, b, c, d))
    want = host([("mulx2" + fld, a + b + c + d) for a, b, c, d in cases])
    for (a, b, c, d), w in zip(cases, want):
        o = run_block(blocks["H2G_ASM_MUL29X2"], m, "r", a=a, b=b, c=c, d=d)
        redc_ok(o, val(a) * val(b) + val(c) * val(d), m)
        assert o == w
        assert run_block(blocks["H2G_ASM_MUL29X2_IP"], m, "c", a=a, b=b, c=c, d=d) == w
