"""h2g_verify_proof / h2g_verify_batch and the verifying-key handles against the oracle's
verifier (oracle/py/verifier.py).

Device proofs of the circuits the suite proves must verify OK across {shplonk, gwc} x
{blake2b, keccak256}, and on every case with k <= 8 the native verdict must equal the oracle's:
OK where it returns True, REJECTED where it returns False, MALFORMED where it raises
VerifyError.  The params come from a known secret (h2g_params_setup), so the oracle decides
DualMSM::check exactly as [s] left == right; the native side sees only Params.verifier()'s
three points and decides it by the pairing (pinned by tests/test_pairing_host_cpu.py).
"""
import numpy as np
import pytest

import _gen_circuit as G
import bn254_ref as B
import h2g
import h2g_circuit as hc
import verifier as V

pytestmark = pytest.mark.gpu

OK, REJECTED, MALFORMED = h2g.VERIFY_OK, h2g.VERIFY_REJECTED, h2g.VERIFY_MALFORMED
S_INT = 0xC0FFEE
COMBOS = [(m, t) for m in ("shplonk", "gwc") for t in ("blake2b", "keccak256")]
COMBO_IDS = [f"{m}-{t}" for m, t in COMBOS]
_PARAMS, _KEYS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _init():
    h2g.init()
    yield
    for key in _KEYS.values():
        key["vk"].close()
        key["pk"].close()
    _KEYS.clear()
    for p in _PARAMS.values():
        p.close()
    _PARAMS.clear()


def params(k):
    if k not in _PARAMS:
        _PARAMS[k] = h2g.Params(k, s=np.asarray(hc.fr_to_limbs(S_INT), dtype=np.uint64))
    return _PARAMS[k]


# ----------------------------------------------------------------------------- the cases
def _gen(case_id):
    def build():
        i = [G.case_id(c) for c in G.CASES].index(case_id)
        circ, wit, fill = G.generate(**G.CASES[i])
        return circ, [wit], [fill]
    return build


def _my(values):
    def build():
        made = [hc.my_circuit(6, input_value=v) for v in values]
        return made[0][0], [m[1] for m in made], [m[2] for m in made]
    return build


def _plain(fn, *args, **kw):
    def build():
        circ, wit = fn(*args, **kw)
        return circ, [wit], [None]
    return build


def _challenge():
    circ, wit, fill = hc.challenge_circuit(6, extended=True)
    return circ, [wit], [fill]


CASES = {
    "simple_k8": _plain(hc.simple_example, 8),
    "c3_k8": _plain(hc.synthetic_c3, 8, h2g.DeviceOps, seed=7),
    "two_circuits": _my([42, 1000]),             # instances, a lookup, a shuffle, two phases, two circuits
    "phased_challenges": _challenge,             # three phases, challenges inside gates and lookups
    "lookup_shuffle": _my([42]),
    "lookup_k8": _plain(hc.lookup_circuit, 8),
    "gen_s101": _gen("s101-k6-d3"),
    "gen_s206": _gen("s206-k7-d5"),
    "gen_s305": _gen("s305-k6-d8"),
    "gen_s405": _gen("s405-k6-d17"),
    "gen_s502": _gen("s502-k7-d5-challenges"),
    "gen_s603": _gen("s603-k7-d7"),
}


def key(name, build=None):
    """the case's circuit, witnesses, device key and verifying key (made once)"""
    if name not in _KEYS:
        circ, wits, fills = (build or CASES[name])()
        pk = h2g.ProvingKey(params(circ.k), circ)
        f, p = pk.vk_commitments()
        _KEYS[name] = dict(circ=circ, wits=wits, fills=fills, pk=pk, vk=h2g.VerifyingKey.from_pk(pk),
                           vkc=([V.affine_from_limbs(c) for c in f], [V.affine_from_limbs(c) for c in p]))
    return _KEYS[name]


def prove(kc, multiopen="shplonk", transcript="blake2b", seed=bytes([7] * 32), wits=None, fills=None):
    wits = wits or kc["wits"]
    fills = fills or kc["fills"]
    pk = kc["pk"]
    if len(wits) == 1 and fills[0] is None:
        return pk.create_proof(wits[0], seed=seed, multiopen=multiopen, transcript=transcript)
    if fills[0] is None:
        return pk.create_proof_multi(wits, seed=seed, multiopen=multiopen, transcript=transcript)
    return pk.create_proof_multi(wits, seed=seed, fills=fills, multiopen=multiopen, transcript=transcript)


def columns(kc, wits=None):
    return [h2g.instance_columns(w, kc["circ"]) for w in (wits or kc["wits"])]


def oracle_verdict(kc, proof, inst_cols, multiopen="shplonk", transcript="blake2b", vkc=None):
    ints = [[hc.mont_to_ints(col) for col in cols] for cols in inst_cols]
    try:
        ok = V.verify(kc["circ"], None, bytes(proof), S_INT, vk=vkc or kc["vkc"], instances_multi=ints,
                      multiopen=multiopen, transcript=transcript)
    except V.VerifyError:
        return MALFORMED
    return OK if ok else REJECTED


def n_evals(kc, nc=1):
    circ, pk = kc["circ"], kc["pk"]
    return (nc * pk.n_adv_q + pk.n_fix_q + 1 + len(circ.perm_columns) + nc * (3 * pk.nsets - 1 if pk.nsets else 0)
            + nc * 5 * len(circ.lookups) + nc * 2 * len(circ.shuffles))


# ----------------------------------------------------------------------------- valid proofs
@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("name", list(CASES))
def test_device_proofs_verify_and_match_the_oracle(name, combo):
    multiopen, transcript = combo
    kc = key(name)
    proof = prove(kc, multiopen, transcript)
    cols = columns(kc)
    assert kc["vk"].verify(proof, cols, multiopen, transcript) == OK
    assert oracle_verdict(kc, proof, cols, multiopen, transcript) == OK
    # the other scheme's / transcript's verifier refuses the same bytes
    other = "gwc" if multiopen == "shplonk" else "shplonk"
    assert kc["vk"].verify(proof, cols, other, transcript) in (REJECTED, MALFORMED)
    flip = "keccak256" if transcript == "blake2b" else "blake2b"
    assert kc["vk"].verify(proof, cols, multiopen, flip) == REJECTED


@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
def test_c3_k12_verifies(combo):
    multiopen, transcript = combo
    kc = key("c3_k12", _plain(hc.synthetic_c3, 12, h2g.DeviceOps, seed=7))
    proof = prove(kc, multiopen, transcript)
    assert kc["vk"].verify(proof, columns(kc), multiopen, transcript) == OK
    t = bytearray(proof)
    t[-40] ^= 1
    assert kc["vk"].verify(bytes(t), columns(kc), multiopen, transcript) in (REJECTED, MALFORMED)


# ----------------------------------------------------------------------------- rejections
@pytest.fixture(scope="module")
def base():
    """one circuit with instances, a lookup, a shuffle and two phases; one valid proof"""
    kc = key("lookup_shuffle")
    proof = prove(kc)
    return kc, proof, columns(kc)


def tampered(proof, pos, bit=0):
    t = bytearray(proof)
    t[pos] ^= 1 << bit
    return bytes(t)


@pytest.mark.parametrize("multiopen", ["shplonk", "gwc"])
def test_rejections_match_the_oracle(multiopen):
    kc = key("lookup_shuffle")
    cols = columns(kc)
    proof = prove(kc, multiopen)
    # the evaluations sit between the head points and the multi-open points; the number of
    # multi-open points is 2 (SHPLONK) or one per distinct opening point (GWC)
    shp = prove(kc, "shplonk")
    head_pts = len(shp) // 32 - n_evals(kc) - 2
    tail = len(proof) - 32 * (head_pts + n_evals(kc))
    ev0 = 32 * head_pts
    assert tail >= 64 and tail % 32 == 0
    cases = {
        "commitment bit 0": tampered(proof, 0, 0),
        "commitment bit 1": tampered(proof, 32 * 3 + 1, 1),
        "commitment bit 2": tampered(proof, 32 * 5 + 2, 2),
        "evaluation": tampered(proof, ev0 + 32 * 2, 0),
        "last evaluation": tampered(proof, ev0 + 32 * n_evals(kc) - 32, 3),
        "last witness point": tampered(proof, len(proof) - 32 + 4, 5),
    }
    seen = set()
    for what, bad in cases.items():
        got = kc["vk"].verify(bad, cols, multiopen)
        assert got == oracle_verdict(kc, bad, cols, multiopen), what
        assert got != OK, what
        seen.add(got)
    assert REJECTED in seen
    # a wrong instance value
    wrong = [[c.copy() for c in cols[0]]]
    wrong[0][0][0] = hc.fr_to_limbs((hc.fr_from_limbs(wrong[0][0][0]) + 1) % hc.R_MOD)
    assert kc["vk"].verify(proof, wrong, multiopen) == oracle_verdict(kc, proof, wrong, multiopen) == REJECTED
    assert kc["vk"].verify(proof, cols, multiopen) == OK


def test_proof_made_with_another_key():
    k1 = key("simple_k8")
    k2 = key("simple_k8_other", _plain(hc.simple_example, 8, blocks=10))   # other fixed values and copies
    assert k1["vk"].write() != k2["vk"].write()
    proof = prove(k2)
    cols = columns(k2)
    assert k2["vk"].verify(proof, cols) == OK
    got = k1["vk"].verify(proof, cols)
    assert got == oracle_verdict(k1, proof, cols) != OK


# ----------------------------------------------------------------------------- malformed inputs
def off_curve_x():
    x = 5
    while pow((x ** 3 + 3) % B.P, (B.P - 1) // 2, B.P) == 1:
        x += 1
    return x


def test_malformed_inputs_are_verdicts_not_errors(base):
    kc, proof, cols = base
    vk = kc["vk"]
    head_pts = len(proof) // 32 - n_evals(kc) - 2
    ev0 = 32 * head_pts
    r_bytes, p_bytes = B.R.to_bytes(32, "little"), B.P.to_bytes(32, "little")
    bad = {
        "truncated by 1": proof[:-1],
        "truncated by 32": proof[:-32],
        "one trailing byte": proof + b"\x00",
        "empty": b"",
        "an evaluation set to r": proof[:ev0 + 64] + r_bytes + proof[ev0 + 96:],
        "a point with x = p": proof[:64] + p_bytes + proof[96:],
        "x = p in the last point": proof[:-32] + p_bytes,
        "x off the curve": proof[:32] + off_curve_x().to_bytes(32, "little") + proof[64:],
        "the point at infinity": proof[:32] + bytes(32) + proof[64:],
    }
    for what, b in bad.items():
        assert len(b) != len(proof) or b != proof
        assert vk.verify(b, cols) == MALFORMED, what
    for what in ("an evaluation set to r", "a point with x = p", "x off the curve", "the point at infinity"):
        assert oracle_verdict(kc, bad[what], cols) == MALFORMED, what
    # too many instance values, an instance value >= r, a missing column
    n = kc["circ"].n
    long_col = [[np.zeros((n, 4), dtype=np.uint64)] + list(cols[0][1:])]
    assert vk.verify(proof, long_col) == MALFORMED
    assert oracle_verdict(kc, proof, long_col) == MALFORMED
    big = [[np.full((1, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)] + list(cols[0][1:])]
    assert vk.verify(proof, big) == MALFORMED
    # a malformed proof in a batch leaves its neighbours alone
    verdicts, stats = vk.verify_batch([proof, bad["x off the curve"], proof, bad["truncated by 1"]], [cols] * 4)
    assert verdicts == [OK, MALFORMED, OK, MALFORMED]
    assert stats[0] == 1
    assert vk.verify(proof, cols) == OK


# ----------------------------------------------------------------------------- key serialisation
@pytest.mark.parametrize("fmt", [h2g.PROCESSED, h2g.RAW_BYTES, h2g.RAW_BYTES_UNCHECKED])
def test_vk_write_read_round_trip(fmt):
    kc = key("lookup_k8")
    data = kc["vk"].write(fmt)
    assert kc["pk"].write(fmt)[: len(data)] == data
    circ = kc["circ"]
    assert len(data) == 6 + (32 if fmt == h2g.PROCESSED else 64) * (circ.num_fixed + len(circ.perm_columns))
    vk2 = h2g.VerifyingKey.read(circ, data, kc["vk"].vp, fmt)
    assert vk2.write(fmt) == data
    proof = prove(kc)
    assert vk2.verify(proof, columns(kc)) == OK
    vk2.close()
    for broken in (data[:-1], data + b"\x00", b"\x05" + data[1:]):
        with pytest.raises(h2g.H2GError):
            h2g.VerifyingKey.read(circ, broken, kc["vk"].vp, fmt)


def test_key_from_bytes_alone_verifies():
    """no params and no proving key alive: the verifier's 40 words, the key's bytes"""
    circ, wit = hc.simple_example(7)
    prm = h2g.Params(circ.k, s=np.asarray(hc.fr_to_limbs(S_INT + 5), dtype=np.uint64))
    pk = h2g.ProvingKey(prm, circ)
    proof = pk.create_proof(wit)
    vk = h2g.VerifyingKey.from_pk(pk)
    data = vk.write(h2g.PROCESSED)
    vp = prm.verifier()
    vk.close()
    pk.close()
    prm.close()
    vk2 = h2g.VerifyingKey.read(circ, data, vp, h2g.PROCESSED)
    cols = [h2g.instance_columns(wit, circ)]
    assert vk2.verify(proof, cols) == OK
    assert vk2.verify(tampered(proof, len(proof) - 100), cols) != OK
    vk2.close()


# ----------------------------------------------------------------------------- batches
B_ = 33


@pytest.fixture(scope="module")
def batch():
    """33 proofs of one key with distinct seeds and instances"""
    kc = key("lookup_shuffle")
    proofs, insts = [], []
    for i in range(B_):
        _, wit, fill = hc.my_circuit(6, input_value=42 + i)
        proofs.append(prove(kc, seed=bytes([i + 1] * 32), wits=[wit], fills=[fill]))
        insts.append([h2g.instance_columns(wit, kc["circ"])])
    assert len(set(proofs)) == B_
    head_pts = len(proofs[0]) // 32 - n_evals(kc) - 2
    return kc["vk"], proofs, insts, 32 * head_pts


def test_batch_all_valid_is_one_pairing_check(batch):
    vk, proofs, insts, _ = batch
    verdicts, stats = vk.verify_batch(proofs, insts, rng_seed=bytes(range(32)))
    assert verdicts == [OK] * B_
    assert stats[0] == 1
    assert stats[2] == B_ * (len(proofs[0]) // 32 - n_evals(key("lookup_shuffle")))   # every point, once
    assert stats[1] > 0


@pytest.mark.parametrize("pos", [0, 16, 32])
def test_batch_finds_the_one_invalid_proof(batch, pos):
    vk, proofs, insts, ev0 = batch
    bad = list(proofs)
    bad[pos] = tampered(proofs[pos], ev0 + 32)
    verdicts, stats = vk.verify_batch(bad, insts, rng_seed=bytes([9] * 32))
    assert verdicts == [REJECTED if i == pos else OK for i in range(B_)]
    assert 2 <= stats[0] <= 1 + 2 * 1 * 6


def test_batch_two_invalid_one_malformed(batch):
    vk, proofs, insts, ev0 = batch
    bad = list(proofs)
    bad[3] = tampered(proofs[3], ev0)
    bad[20] = proofs[20][:-32] + proofs[21][-32:]        # another proof's last opening point
    bad[27] = proofs[27][:-1]
    want = [OK] * B_
    want[3] = want[20] = REJECTED
    want[27] = MALFORMED
    seen = []
    for seed in (bytes([1] * 32), bytes([2] * 32)):      # other random factors, the same verdicts
        verdicts, stats = vk.verify_batch(bad, insts, rng_seed=seed)
        assert verdicts == want
        assert stats[0] <= 1 + 2 * 2 * 6
        seen.append(verdicts)
    assert seen[0] == seen[1]
    # a proof checked against another proof's instances
    swapped = list(insts)
    swapped[5], swapped[6] = insts[6], insts[5]
    verdicts, _ = vk.verify_batch(proofs, swapped, rng_seed=bytes([3] * 32))
    assert verdicts == [REJECTED if i in (5, 6) else OK for i in range(B_)]


def test_batch_with_the_system_rng(batch):
    vk, proofs, insts, ev0 = batch
    verdicts, stats = vk.verify_batch(proofs[:9], insts[:9])
    assert verdicts == [OK] * 9 and stats[0] == 1
    bad = [tampered(proofs[0], ev0)] + proofs[1:9]
    verdicts, _ = vk.verify_batch(bad, insts[:9])
    assert verdicts == [REJECTED] + [OK] * 8
    assert vk.verify_batch([], []) == ([], [0, 0, 0, 0])
    assert vk.verify_batch([bad[0]], [insts[0]])[0] == [REJECTED]


def test_batch_of_two_circuit_proofs():
    kc = key("two_circuits")
    proofs = [prove(kc, "gwc", "keccak256", seed=bytes([s] * 32)) for s in (1, 2, 3)]
    cols = columns(kc)
    verdicts, stats = kc["vk"].verify_batch(proofs, [cols] * 3, "gwc", "keccak256", rng_seed=bytes(32))
    assert verdicts == [OK] * 3 and stats[0] == 1
    verdicts, _ = kc["vk"].verify_batch(proofs, [cols, cols[::-1], cols], "gwc", "keccak256", rng_seed=bytes(32))
    assert verdicts == [OK, REJECTED, OK]
