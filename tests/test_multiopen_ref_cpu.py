"""The multi-open restatement (tests/_multiopen_ref.py) against itself, before the device is
held to it: the reference's round trip (halo2_backend/src/poly/multiopen_test.rs:140-304,
k = 4) proved by the restated prover is accepted by the restated verifier, and rejected with
b's evaluation replaced by a's -- both schemes, both transcripts."""
import pytest

import _multiopen_ref as M

S_INT = 0xC0FFEE
K = 4
COMBOS = [(m, t) for m in ("shplonk", "gwc") for t in ("blake2b", "keccak256")]


@pytest.fixture(scope="module")
def proofs():
    return {c: M.round_trip_prove(c[0], c[1], K, S_INT) for c in COMBOS}


@pytest.mark.parametrize("scheme,kind", COMBOS, ids=[f"{m}-{t}" for m, t in COMBOS])
def test_round_trip(proofs, scheme, kind):
    proof = proofs[(scheme, kind)]
    # 3 commitments, 3 evaluations, then 2 points (SHPLONK) or one per distinct point (GWC: x, y)
    assert len(proof) == 32 * (3 + 3 + 2)
    T, cms, valid, invalid = M.round_trip_open(kind, proof)
    assert cms == [M.commit(p, S_INT) for p in M.round_trip_polys(K)]
    assert M.verify(scheme, T, S_INT, cms, valid, proof) is True
    T, cms, valid, invalid = M.round_trip_open(kind, proof)
    assert M.verify(scheme, T, S_INT, cms, invalid, proof) is False


def test_schemes_and_transcripts_differ(proofs):
    assert len(set(proofs.values())) == len(COMBOS)


def test_identity_commitment_is_refused():
    """one constant polynomial opened at one point: h(X) = 0 (SHPLONK), W(X) = 0 (GWC)"""
    for scheme in ("shplonk", "gwc"):
        T = M.writer("blake2b")
        with pytest.raises(M.V.VerifyError):
            M.prove(scheme, T, S_INT, [[5]], [(0, 77)])
        assert T.finalize() == b""
