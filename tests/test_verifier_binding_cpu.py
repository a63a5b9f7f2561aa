"""The oracle verifier (oracle/py/verifier.py) binds every element it reads.

The GPU tests compare h2g_verify_proof with this verifier, and both restate the same
verifier.rs; neither that comparison nor "valid proofs verify" shows that a query, an h piece or
an evaluation has not been left out of both.  This file needs no second verifier: a proof,
instance or key changed in one element, still validly encoded, must come back False -- not
True (the element is unbound) and not VerifyError (the decoding disagrees with bn254_ref).
The slots come from tests/_proof_layout.py, which reads the circuit alone.

MyCircuit (frontend_backend_split.rs:33-465) at k = 6: instances, a lookup, a shuffle, two
phases, four permutation columns; 43 slots under SHPLONK, 44 under GWC.
"""
import pytest

import _oracle as O
import _proof_layout as L
import bn254_ref as B
import h2g_circuit as hc
import verifier as V

SCHEMES = ["shplonk", "gwc"]
_MADE = {}


def setup_case():
    """circuit, witness source, SRS secret, key commitments and one oracle proof per scheme"""
    if not _MADE:
        circ, wit, fill = hc.my_circuit(6)
        s, g, gl = O.srs(circ.k)
        inst = [hc.mont_to_ints(wit.instance[0])[: int(wit.instance_lens[0])]]
        _MADE.update(circ=circ, wit=wit, fill=fill, s=s, g=g, gl=gl, inst=inst,
                     vk=O.vk_commitments(circ, wit, s, g, gl),
                     proofs={m: O.create_proof(circ, wit, g, gl, fill=fill, multiopen=m) for m in SCHEMES})
    return _MADE


def verify(proof, multiopen="shplonk", inst=None, vk=None):
    m = setup_case()
    return V.verify(m["circ"], inst or m["inst"], bytes(proof), m["s"], multiopen=multiopen, vk=vk or m["vk"])


def layout_of(multiopen):
    m = setup_case()
    layout = L.slots(m["circ"], 1, multiopen)
    assert len(layout) * 32 == len(m["proofs"][multiopen]), multiopen
    return layout


def test_layout_counts():
    assert L.counts(layout_of("shplonk")) == (15, 26, 2)
    assert L.counts(layout_of("gwc")) == (15, 26, 3)
    names = [n for _, n in layout_of("gwc")]
    assert len(set(names)) == len(names)
    for multiopen in SCHEMES:
        assert verify(setup_case()["proofs"][multiopen], multiopen) is True


@pytest.mark.parametrize("multiopen", SCHEMES)
def test_every_slot_is_bound(multiopen):
    """every point negated, every evaluation + 1: each is False"""
    proof = setup_case()["proofs"][multiopen]
    layout = layout_of(multiopen)
    wrong = []
    for i, (kind, name) in enumerate(layout):
        try:
            got = verify(L.mutate_by_kind(proof, layout, i), multiopen)
        except V.VerifyError as e:
            got = f"VerifyError({e})"
        if got is not False:
            wrong.append(f"slot {i} {name}: {got}")
    assert not wrong, wrong


@pytest.mark.parametrize("multiopen", SCHEMES)
def test_aliased_encodings_are_malformed(multiopen):
    """v + r and x + p at the first and last slot of each kind raise VerifyError"""
    proof = setup_case()["proofs"][multiopen]
    layout = layout_of(multiopen)
    for kind in (L.POINT, L.SCALAR):
        idx = [i for i, (k, _) in enumerate(layout) if k == kind]
        for i in (idx[0], idx[-1]):
            with pytest.raises(V.VerifyError):
                got = verify(L.alias(proof, i, kind), multiopen)
                pytest.fail(f"slot {i} {layout[i][1]}: aliased encoding gave {got}")


def test_every_key_commitment_is_bound():
    """transcript_repr is built from the circuit, so only the opening queries bind the key's
    points: each fixed and each permutation commitment negated is False"""
    m = setup_case()
    proof = m["proofs"]["shplonk"]
    fixed, sigma = m["vk"]
    assert len(fixed) == 7 and len(sigma) == 4
    fix_q = m["circ"].queries()[1]
    assert {c for c, _ in fix_q} == set(range(7))   # every fixed column is queried
    wrong = []
    for i in range(len(fixed)):
        vk = (fixed[:i] + [B.g1_neg(fixed[i])] + fixed[i + 1:], sigma)
        if verify(proof, vk=vk) is not False:
            wrong.append(f"fixed commitment {i}")
    for i in range(len(sigma)):
        vk = (fixed, sigma[:i] + [B.g1_neg(sigma[i])] + sigma[i + 1:])
        if verify(proof, vk=vk) is not False:
            wrong.append(f"permutation commitment {i}")
    assert not wrong, wrong


def test_every_instance_value_and_the_length_are_bound():
    m = setup_case()
    circ, proof = m["circ"], m["proofs"]["shplonk"]
    col = list(m["inst"][0])
    assert len(col) == 6
    for j in range(len(col)):
        bad = list(col)
        bad[j] = (bad[j] + 1) % B.R
        assert verify(proof, inst=[bad]) is False, f"instance value {j}"
    # the instance polynomial of a zero-padded column is the same: only the transcript binds the length
    assert verify(proof, inst=[col + [0]]) is False, "a 0 appended"
    assert verify(proof, inst=[col[:-1]]) is False, "the last value dropped"
    usable = circ.n - (circ.blinding_factors() + 1)
    assert usable == 58
    long_col = col + [0] * (usable - len(col))
    assert verify(proof, inst=[long_col]) is False, "padded to the usable rows"
    wit = m["wit"]
    wit_long = hc.Witness(wit.advice, wit.instance, [usable])
    proof_long = O.create_proof(circ, wit_long, m["g"], m["gl"], fill=m["fill"])
    assert proof_long != proof
    assert verify(proof_long, inst=[long_col]) is True
    assert verify(proof_long, inst=[col]) is False
    # one more than the usable rows: Error::InstanceTooLarge, for the prover and the verifier
    with pytest.raises(ValueError):
        O.create_proof(circ, hc.Witness(wit.advice, wit.instance, [usable + 1]), m["g"], m["gl"], fill=m["fill"])
    for p in (proof, proof_long):
        with pytest.raises(V.VerifyError, match="instance too large"):
            verify(p, inst=[long_col + [0]])


def test_shplonk_last_point_shifted_both_ways():
    """pi + D and pi - D (the pair the batch verifier's random factors must keep apart)"""
    proof = setup_case()["proofs"]["shplonk"]
    layout = layout_of("shplonk")
    last = len(layout) - 1
    assert layout[last] == (L.POINT, "shplonk.h2")
    pi = L.point_at(proof, last)
    D = B.g1_mul(B.G1_GEN, 7)
    assert verify(L.replace_point(proof, last, B.g1_add(pi, D))) is False
    assert verify(L.replace_point(proof, last, B.g1_add(pi, B.g1_neg(D)))) is False
