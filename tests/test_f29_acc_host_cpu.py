"""The accumulation's hot-loop forms of csrc/f29.h (xyzz29_madd_acc, subn29, the
carry-chained products) at the worst-case operands of the bounds model.

A host program (tests/native/f29_acc_host.cpp, the kernels' own header compiled for the host
side only) is built twice -- plainly, and with the address and undefined-behaviour
sanitisers -- and every test runs against both.  Results are checked with Python big
integers as in tests/test_f29_host_cpu.py, whose helpers this file uses: the mixed addition
against the affine group law of oracle/py/bn254_ref.py, normalised limbs, and the bound
tools/f29_bounds.py derives for the hot-loop form (the same class as xyzz29_madd's, so
the stored accumulators feed the same fixup).
"""
import os
import random
import subprocess

import pytest

import test_f29_host_cpu as H

B, F = H.B, H.F
MQ, RR, N29, MASK = H.MQ, H.RR, H.N29, H.MASK
limbs, val = H.limbs, H.val


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def run(request, tmp_path_factory):
    if not os.path.exists(H.HIPCC):
        pytest.skip("hipcc not found")
    exe = tmp_path_factory.mktemp("f29acc_" + request.param) / "f29_acc_host"
    flags = ["-O2"] if request.param == "plain" else [
        "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([H.HIPCC, "--offload-host-only", "-std=c++17", "-I", H.CSRC] + flags +
                   [os.path.join(H.REPO, "tests", "native", "f29_acc_host.cpp"), "-o", str(exe)],
                   check=True, cwd=str(exe.parent))

    def go(cmds):
        text = "\n".join(op + " " + " ".join(str(x) for x in args) for op, args in cmds) + "\n"
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        rows = r.stdout.splitlines()
        assert len(rows) == len(cmds)
        for row in rows:
            assert not row.startswith("ERR"), row
        return [[int(x) for x in row.split()] for row in rows]
    return go


@pytest.fixture(scope="module")
def model():
    return F.check()


def test_model_covers_the_hot_loop_form(model):
    """the fused subtractions' constants are the reviewed ones, and the hot-loop form's
    fixpoint is xyzz29_madd's: the accumulator class did not change"""
    assert F.source_fused_constants() == F.EXPECTED_FUSED
    assert model["madd_acc_fixpoint"] == model["madd_fixpoint"]
    assert max(model["madd_acc_fixpoint"]) < 2 ** 259.5
    assert model["madd_acc_intermediate"] < 2 ** 260
    # a fused K halved is rejected (K M must cover what is subtracted) at U2 - X and at
    # R^2 - PPP - 2Q; S2 - Y keeps a spare factor of 2 (a smaller K there lowers Y's own
    # fixpoint below it) -- it stays at xyzz29_madd's 64 so that the stored limbs are the same
    for i in (0, 2):
        ns = list(F.EXPECTED_FUSED["f29.h:xyzz29_madd_acc"])
        ns[i] = str(int(ns[i]) // 2)
        with pytest.raises(AssertionError):
            F.check(fused={"f29.h:xyzz29_madd_acc": ns})


def _one():
    return limbs(RR % MQ)


def _check_point(o, want, fix):
    st, pt = o[0], o[1:]
    assert st == 0
    assert H._affine(pt) == want
    assert all(l < N29 for k in range(4) for l in pt[9 * k:9 * k + 8])
    for v, bd in zip(H._coords(pt), fix):
        assert v < bd, (v.bit_length(), bd.bit_length())


def test_madd_acc_at_the_fixpoint_both_signs(run, model):
    """p's coordinates carry the largest multiple of M below the model's fixpoint; q and
    -q (a negative digit: y -> M - y before to29) are both added"""
    fix = model["madd_acc_fixpoint"]
    rng = random.Random(21)
    pts = H._points(32, 23)
    cases, want = [], []
    for i in range(0, 32, 2):
        p, q = pts[i], pts[i + 1]
        z = rng.randrange(1, MQ)
        P29 = H._xyzz(p, z, fix, rng, top=(i % 4 == 0))
        for qq in (q, B.g1_neg(q)):
            cases.append(P29 + H._q29(qq))
            want.append(B.g1_add(p, qq))
    got = run([("madda", c) for c in cases])
    for w, o in zip(want, got):
        _check_point(o, w, fix)


def test_madd_acc_special_cases_report_their_status(run, model):
    """p == -q -> 1 (the caller's identity flag), p == q -> 2 (the chunk is redone with the
    doubling form); the multiples of M that p carries do not hide either"""
    fix = model["madd_acc_fixpoint"]
    rng = random.Random(25)
    cases, want = [], []
    for p in H._points(6, 27):
        z = rng.randrange(1, MQ)
        for top in (True, False):
            P29 = H._xyzz(p, z, fix, rng, top=top)
            cases += [P29 + H._q29(B.g1_neg(p)), P29 + H._q29(p)]
            want += [1, 2]
    got = run([("madda", c) for c in cases])
    assert [o[0] for o in got] == want


def test_fresh_start_then_additions(run, model):
    """a run started from its first point, (x, y, 1, 1) with x, y in to29 form (< 32 M)"""
    fix = model["madd_acc_fixpoint"]
    pts = H._points(16, 29)
    cases, want = [], []
    for i in range(0, 16, 2):
        cases.append(H._q29(pts[i]) + _one() + _one() + H._q29(pts[i + 1]))
        want.append(B.g1_add(pts[i], pts[i + 1]))
    for w, o in zip(want, run([("madda", c) for c in cases])):
        _check_point(o, w, fix)


def test_chain_of_64_additions_stays_in_bounds(run, model):
    """the kernel's data flow: 64 mixed additions into one accumulator started afresh,
    alternating signs; bounds after every step, the sum against the affine group law, and
    the in-process chain gives the same limbs"""
    fix = model["madd_acc_fixpoint"]
    rng = random.Random(31)  # unrelated multiples of G: no partial sum meets the next point
    pts = [B.g1_mul(B.G1_GEN, rng.randrange(1, B.R)) for _ in range(65)]
    pts = [p if i % 3 else B.g1_neg(p) for i, p in enumerate(pts)]
    acc = H._q29(pts[0]) + _one() + _one()
    start, ref = list(acc), pts[0]
    for q in pts[1:]:
        o = run([("madda", acc + H._q29(q))])[0]
        ref = B.g1_add(ref, q)
        _check_point(o, ref, fix)
        acc = o[1:]
    whole = run([("chain", [64] + start + [l for q in pts[1:] for l in H._q29(q)])])[0]
    assert whole == [0] + acc


def test_chain_restarts_after_the_identity(run, model):
    """P, -P in the middle of a run: status 1, and the next point starts the run afresh"""
    pts = H._points(4, 33)
    a, b, c, d = pts
    start = H._q29(a) + _one() + _one()
    seq = [b, B.g1_neg(B.g1_add(a, b)), c, d]
    o = run([("chain", [4] + start + [l for q in seq for l in H._q29(q)])])[0]
    assert o[0] == 0 and H._affine(o[1:]) == B.g1_add(c, d)
    o3 = run([("chain", [2] + start + [l for q in seq[:2] for l in H._q29(q)])])[0]
    assert o3[0] == 1


def _subn_cases(K, b_limb_max, rng):
    """operands at subn29<K>'s conditions: b <= K M with limbs up to b_limb_max, a
    normalised with the largest top limb a + K M < 2^264 leaves"""
    km = K * MQ
    a_top = ((1 << 264) - km >> 232) - 2
    a_max = [MASK] * 8 + [a_top]
    low = [b_limb_max] * 8
    b_wide = low + [(km - val(low + [0])) >> 232]            # widest limbs, value just below K M
    assert val(b_wide) <= km
    cases = [(a_max, limbs(km)), (limbs(0), limbs(km)), (limbs(0), limbs(km - 1)), (a_max, limbs(0)),
             (limbs(0), limbs(0)), (a_max, b_wide), (limbs(0), b_wide), (limbs(1), limbs(km)),
             ([0] * 8 + [1], limbs(km))]
    for _ in range(40):
        a = [rng.getrandbits(29) for _ in range(8)] + [rng.randrange(a_top + 1)]
        b = [rng.randrange(b_limb_max + 1) for _ in range(8)]
        b.append(rng.randrange(((km - val(b + [0])) >> 232) + 1))
        cases.append((a, b))
    return cases


@pytest.mark.parametrize("K,b_limb_max", [(64, MASK), (32, 3 * MASK)])
def test_subn29_at_the_worst_operands_its_bound_admits(run, K, b_limb_max):
    """K = 64: U2 - X, S2 - Y (b normalised); K = 32: R^2 - (PPP + 2 Q), b a limb-wise sum of
    three normalised values.  The result is the integer a - b + K M in normalised limbs --
    the limbs norm29(sub29<K, OFF>(a, b)) gives"""
    cases = _subn_cases(K, b_limb_max, random.Random(K))
    got = run([(f"subn{K}", a + b) for a, b in cases])
    for (a, b), o in zip(cases, got):
        want = val(a) - val(b) + K * MQ
        assert want >= 0
        assert o == limbs(want), (a, b)


def test_chained_products_keep_the_product_contract(run):
    """mul29_acc / sqr29_acc / mul29x2_acc: REDC congruence, output bound and normalised limbs
    at the limb bounds (the operands of tests/test_f29_host_cpu.py)"""
    rng = random.Random(35)
    ops = H._operands(MQ, rng)
    pairs = [(a, b) for a in ops for b in ops[:8]]
    wide = [(1 << 30) - 1] * 8 + [(1 << 31) - 1]
    pairs += [(wide, limbs(MQ - 1)), (limbs(MQ - 1), wide)]
    for (a, b), o in zip(pairs, run([("mula", a + b) for a, b in pairs])):
        H.redc_ok(o, val(a) * val(b), MQ)
    sq = [a for a in ops if all(l < N29 for l in a[:8]) and a[8] < 1 << 30] + [[MASK] * 8 + [(1 << 30) - 1]]
    got_s = run([("sqra", a) for a in sq])
    got_m = run([("mula", a + a) for a in sq])
    for a, s, mm in zip(sq, got_s, got_m):
        H.redc_ok(s, val(a) ** 2, MQ)
        assert s == mm
    big = [3 * (1 << 29) - 1] * 9
    x2 = [([MASK] * 9, big, [MASK] * 9, big)]
    for _ in range(20):
        x2.append(tuple([rng.choice((hi, rng.randrange(hi + 1))) for _ in range(9)]
                        for hi in (MASK, 3 * (1 << 29) - 1, MASK, 3 * (1 << 29) - 1)))
    for (a, b, c, d), o in zip(x2, run([("mulx2a", a + b + c + d) for a, b, c, d in x2])):
        H.redc_ok(o, val(a) * val(b) + val(c) * val(d), MQ)
