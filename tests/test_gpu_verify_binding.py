"""h2g_verify_proof / h2g_verify_batch bind every proof slot, instance value, the instance
length, every key commitment, and the batch's random factors.

tests/test_gpu_verify.py compares the native verdict with the oracle's; both restate the same
verifier.rs, so a query, an h piece or an evaluation left out of both would pass there.  Here
no second verifier decides: a proof changed in one slot whose encoding is still valid must be
REJECTED -- OK means the slot is unbound, MALFORMED that the decoding differs from bn254_ref.
The slots come from tests/_proof_layout.py (the circuit alone, verifier.rs's order); the CPU
twin of this file, tests/test_verifier_binding_cpu.py, holds the oracle to the same sweep.
"""
import numpy as np
import pytest

import _gen_circuit as G
import _proof_layout as L
import bn254_ref as B
import h2g
import h2g_circuit as hc
import verifier as V

pytestmark = pytest.mark.gpu

OK, REJECTED, MALFORMED = h2g.VERIFY_OK, h2g.VERIFY_REJECTED, h2g.VERIFY_MALFORMED
S_INT = 0xC0FFEE
SCHEMES = ["shplonk", "gwc"]
COMBOS = [(m, t) for m in SCHEMES for t in ("blake2b", "keccak256")]
_PARAMS, _KEYS, _PROOFS = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _init():
    h2g.init()
    yield
    for kc in _KEYS.values():
        kc["vk"].close()
        kc["pk"].close()
    _KEYS.clear()
    _PROOFS.clear()
    for p in _PARAMS.values():
        p.close()
    _PARAMS.clear()


def _my(values):
    def build():
        made = [hc.my_circuit(6, input_value=v) for v in values]
        return made[0][0], [m[1] for m in made], [m[2] for m in made]
    return build


def _gen(case_id):
    def build():
        i = [G.case_id(c) for c in G.CASES].index(case_id)
        circ, wit, fill = G.generate(**G.CASES[i])
        return circ, [wit], [fill]
    return build


def _c3():
    circ, wit = hc.synthetic_c3(8, h2g.DeviceOps, seed=7)
    return circ, [wit], [None]


CASES = {
    "my_circuit": _my([42]),
    "two_my_circuits": _my([42, 1000]),            # two witnesses in one proof
    "s502-k7-d5-challenges": _gen("s502-k7-d5-challenges"),   # three phases
    "s405-k6-d17": _gen("s405-k6-d17"),            # sixteen h pieces: every power of x^n
    "c3_k8": _c3,
}


def key(name):
    """the case's circuit, witnesses, device key and verifying key (made once); the params
    come from a known secret, so oracle_verdict can decide the pairing equation with it"""
    if name not in _KEYS:
        circ, wits, fills = CASES[name]()
        assert circ.k <= 8
        if circ.k not in _PARAMS:
            _PARAMS[circ.k] = h2g.Params(circ.k, s=np.asarray(hc.fr_to_limbs(S_INT), dtype=np.uint64))
        pk = h2g.ProvingKey(_PARAMS[circ.k], circ)
        _KEYS[name] = dict(name=name, circ=circ, wits=wits, fills=fills, pk=pk, vk=h2g.VerifyingKey.from_pk(pk))
    return _KEYS[name]


def prove(kc, multiopen="shplonk", transcript="blake2b", wits=None):
    """-> (proof, its slots); the layout must account for every byte"""
    tag = (kc["name"], multiopen, transcript) if wits is None else None
    if tag not in _PROOFS:
        ws, fills, pk = wits or kc["wits"], kc["fills"], kc["pk"]
        if fills[0] is None:
            proof = pk.create_proof(ws[0], multiopen=multiopen, transcript=transcript)
        else:
            proof = pk.create_proof_multi(ws, fills=fills, multiopen=multiopen, transcript=transcript)
        layout = L.slots(kc["circ"], len(ws), multiopen)
        assert len(layout) * 32 == len(proof), (kc["name"], multiopen, L.counts(layout), len(proof))
        if tag is None:
            return proof, layout
        _PROOFS[tag] = (proof, layout)
    return _PROOFS[tag]


def columns(kc, wits=None):
    """per circuit, its instance columns as canonical ints"""
    return [[hc.mont_to_ints(col) for col in h2g.instance_columns(w, kc["circ"])] for w in (wits or kc["wits"])]


def oracle_verdict(kc, proof, cols, multiopen="shplonk"):
    if "vkc" not in kc:
        f, p = kc["pk"].vk_commitments()
        kc["vkc"] = ([V.affine_from_limbs(c) for c in f], [V.affine_from_limbs(c) for c in p])
    try:
        ok = V.verify(kc["circ"], None, bytes(proof), S_INT, vk=kc["vkc"], instances_multi=cols, multiopen=multiopen)
    except V.VerifyError:
        return MALFORMED
    return OK if ok else REJECTED


def named(v):
    return {OK: "OK", REJECTED: "REJECTED", MALFORMED: "MALFORMED"}.get(v, v)


# ----------------------------------------------------------------------------- 3a: one proof, every slot
@pytest.mark.parametrize("combo", COMBOS, ids=[f"{m}-{t}" for m, t in COMBOS])
def test_every_slot_is_bound(combo):
    """every point negated, every evaluation + 1: REJECTED exactly"""
    multiopen, transcript = combo
    kc = key("my_circuit")
    proof, layout = prove(kc, multiopen, transcript)
    cols = columns(kc)
    assert L.counts(layout) == ((15, 26, 2) if multiopen == "shplonk" else (15, 26, 3))
    assert kc["vk"].verify(proof, cols, multiopen, transcript) == OK
    wrong = []
    for i, (_, name) in enumerate(layout):
        got = kc["vk"].verify(L.mutate_by_kind(proof, layout, i), cols, multiopen, transcript)
        if got != REJECTED:
            wrong.append(f"slot {i} {name}: {named(got)}")
    assert not wrong, wrong


def test_encodings_and_neighbours():
    """SHPLONK / Blake2b: x + 1 is MALFORMED where bn254_ref cannot decode it and REJECTED where
    it can; v + r and x + p are MALFORMED; two neighbours of one kind swapped are REJECTED"""
    kc = key("my_circuit")
    proof, layout = prove(kc)
    cols = columns(kc)
    vk = kc["vk"]
    wrong, decoded, swapped = [], [], 0
    for i, (kind, name) in enumerate(layout):
        if kind == L.POINT:
            bad, decodes = L.next_x(proof, i)
            decoded.append(decodes)
            got, want = vk.verify(bad, cols), REJECTED if decodes else MALFORMED
            if got != want:
                wrong.append(f"next_x, slot {i} {name}: {named(got)}, want {named(want)}")
        got = vk.verify(L.alias(proof, i, kind), cols)
        if got != MALFORMED:
            wrong.append(f"alias, slot {i} {name}: {named(got)}")
        if L.can_swap(proof, layout, i):
            swapped += 1
            got = vk.verify(L.swap_with_next(proof, i), cols)
            if got != REJECTED:
                wrong.append(f"swap, slots {i} {name} and {i + 1} {layout[i + 1][1]}: {named(got)}")
    assert not wrong, wrong
    assert any(decoded) and not all(decoded)       # both ways are exercised
    # every pair inside the three runs of one kind, but for s_lookup / s_ltable and s_shuffle /
    # s_stable: MyCircuit's twin fixed columns, whose neighbouring evaluations are equal
    assert swapped == len(layout) - 3 - 2
    assert vk.verify(proof, cols) == OK


# ----------------------------------------------------------------------------- 3b: batches, nearly all bad
@pytest.mark.parametrize("multiopen", SCHEMES)
@pytest.mark.parametrize("name", ["two_my_circuits", "s502-k7-d5-challenges", "s405-k6-d17", "c3_k8"])
def test_batch_of_one_mutation_per_slot(name, multiopen):
    """one verify_batch call: a copy of the proof per slot, mutated there, and the untouched
    proof first, in the middle and last -- OK exactly at those three"""
    kc = key(name)
    proof, layout = prove(kc, multiopen)
    cols = columns(kc)
    muts = [L.mutate_by_kind(proof, layout, i) for i in range(len(layout))]
    half = len(muts) // 2
    proofs = [proof] + muts[:half] + [proof] + muts[half:] + [proof]
    slot_of = [None] + list(range(half)) + [None] + list(range(half, len(muts))) + [None]
    nb = len(proofs)
    verdicts, stats = kc["vk"].verify_batch(proofs, [cols] * nb, multiopen, rng_seed=bytes([5] * 32))
    wrong = []
    for pos, (got, slot) in enumerate(zip(verdicts, slot_of)):
        want = OK if slot is None else REJECTED
        if got != want:
            what = "the untouched proof" if slot is None else f"slot {slot} {layout[slot][1]}"
            wrong.append(f"position {pos}, {what}: {named(got)}")
    assert not wrong, wrong
    bad = nb - 3
    assert 1 < stats[0] <= 1 + 2 * bad * (nb - 1).bit_length()    # h2g.h: 1 + 2 f ceil(log2 B)
    npts = sum(1 for k, _ in layout if k == L.POINT)
    assert stats[2] == nb * npts                                   # every point of every copy, once


# ----------------------------------------------------------------------------- 3c: the random factors
class SameBytes:
    """an RNG whose every draw is the same: all r_i equal"""

    def fill_bytes(self, n):
        return (bytes(range(1, 65)) * ((n + 63) // 64))[:n]


def test_batch_factors_differ():
    """A = P with its last point pi + D, B = P with pi - D.  The challenge u is drawn before pi
    is read, so A leaves (s - u) D and B leaves -(s - u) D in the pairing equation, and under
    equal r_i the two cancel (the premise, shown first).  Under the r_i the batch verifier
    really draws they must not."""
    kc = key("my_circuit")
    P, layout = prove(kc)
    cols = columns(kc)
    vk = kc["vk"]
    last = len(layout) - 1
    assert layout[last] == (L.POINT, "shplonk.h2")
    pi = L.point_at(P, last)
    D = B.g1_mul(B.G1_GEN, 7)
    A_ = L.replace_point(P, last, B.g1_add(pi, D))
    B_ = L.replace_point(P, last, B.g1_add(pi, B.g1_neg(D)))
    assert vk.verify(A_, cols) == REJECTED
    assert vk.verify(B_, cols) == REJECTED
    verdicts, _ = vk.verify_batch([A_, B_], [cols] * 2, rng=SameBytes())
    assert verdicts == [OK, OK], "premise: the pair cancels under equal factors"
    for kw in (dict(rng_seed=bytes([1] * 32)), dict(rng_seed=bytes([2] * 32)), dict(rng_seed=bytes(range(32))), {}):
        verdicts, _ = vk.verify_batch([A_, B_], [cols] * 2, **kw)
        assert verdicts == [REJECTED, REJECTED], kw
        verdicts, _ = vk.verify_batch([A_, P, B_], [cols] * 3, **kw)
        assert verdicts == [REJECTED, OK, REJECTED], kw


# ----------------------------------------------------------------------------- 3d: instances
def test_every_instance_value_and_the_length_are_bound():
    kc = key("my_circuit")
    circ, vk = kc["circ"], kc["vk"]
    proof, _ = prove(kc)
    col = columns(kc)[0][0]
    assert len(col) == 6
    for j in range(len(col)):
        bad = list(col)
        bad[j] = (bad[j] + 1) % B.R
        assert vk.verify(proof, [[bad]]) == REJECTED, f"instance value {j}"
        if j == 0:
            assert oracle_verdict(kc, proof, [[bad]]) == REJECTED
    # zero padding leaves the instance polynomial alone: only the transcript binds the length
    assert vk.verify(proof, [[col + [0]]]) == REJECTED, "a 0 appended"
    assert vk.verify(proof, [[col[:-1]]]) == REJECTED, "the last value dropped"
    usable = circ.n - (circ.blinding_factors() + 1)
    long_col = col + [0] * (usable - len(col))
    wit = kc["wits"][0]
    proof_long, _ = prove(kc, wits=[hc.Witness(wit.advice, wit.instance, [usable])])
    assert proof_long != proof
    assert vk.verify(proof_long, [[long_col]]) == oracle_verdict(kc, proof_long, [[long_col]]) == OK
    assert vk.verify(proof_long, [[col]]) == oracle_verdict(kc, proof_long, [[col]]) == REJECTED
    assert vk.verify(proof, [[long_col]]) == REJECTED
    # one value more than the usable rows: Error::InstanceTooLarge
    too_long = long_col + [0]
    assert vk.verify(proof_long, [[too_long]]) == oracle_verdict(kc, proof_long, [[too_long]]) == MALFORMED
    assert vk.verify(proof, [[col]]) == OK


# ----------------------------------------------------------------------------- 3e: the key's commitments
def test_every_key_commitment_is_bound():
    """transcript_repr comes from the circuit, not from the key's points, so only the opening
    queries bind them: a key read back with one commitment negated rejects the valid proof"""
    kc = key("my_circuit")
    circ = kc["circ"]
    proof, _ = prove(kc)
    cols = columns(kc)
    data = kc["vk"].write(h2g.PROCESSED)
    nf, npm = circ.num_fixed, len(circ.perm_columns)
    assert len(data) == 6 + 32 * (nf + npm)
    queried = {c for c, _ in circ.queries()[1]}
    skipped = [f"fixed{c}" for c in range(nf) if c not in queried]   # no query: nothing can bind it
    assert skipped == []
    targets = [(f"fixed{c}", c) for c in range(nf) if c in queried] + [(f"sigma{i}", nf + i) for i in range(npm)]
    assert len(targets) == 11
    wrong = []
    for what, idx in targets:
        b = bytearray(data)
        b[6 + 32 * idx + 31] ^= 0x80
        vk2 = h2g.VerifyingKey.read(circ, bytes(b), kc["vk"].vp, h2g.PROCESSED)
        try:
            assert vk2.write(h2g.PROCESSED) == bytes(b)
            got = vk2.verify(proof, cols)
        finally:
            vk2.close()
        if got != REJECTED:
            wrong.append(f"{what}: {named(got)}")
    assert not wrong, wrong
    vk2 = h2g.VerifyingKey.read(circ, data, kc["vk"].vp, h2g.PROCESSED)
    assert vk2.verify(proof, cols) == OK
    vk2.close()
