"""The device prover and witness check on the generated circuits of tests/_gen_circuit.py
(pinned valid on the CPU by tests/test_generated_circuits_cpu.py): proof bytes against the C
restatement prover for satisfying and for unsatisfied witnesses, h2g_check_witness against the
plain-Python restatement, and two witnesses of one circuit in one proof.  The cases reach what
the hand-written circuits do not: gate trees of 30..120 nodes with NEG(NEG x), long chains,
Sethi-Ullman numbers >= 6, dozens of constants (0 and r - 1 among them), rotations up to
n - 1, degrees 3..17 (extended domains 2n..16n) with their permutation chunking, compound and
shared lookup tables, and challenges inside gate and lookup expressions."""
import numpy as np
import pytest

import _check_ref as CR
import _gen_circuit as G
import _oracle as O
import h2g
import h2g_circuit as hc

pytestmark = pytest.mark.gpu

_PARAMS = {}
IDS = [G.case_id(c) for c in G.CASES]


@pytest.fixture(scope="module", autouse=True)
def _init():
    h2g.init()
    yield
    for _, _, _, p in _PARAMS.values():
        p.close()
    _PARAMS.clear()


def _params(k):
    if k not in _PARAMS:
        s, g, gl = O.srs(k)
        _PARAMS[k] = (s, g, gl, h2g.Params(k, g, gl))
    return _PARAMS[k]


def device_check(pk, wit, ch, want):
    total, recs = pk.check_witness(wit, challenges=ch, cap=max(64, len(want) + 8))
    assert total == len(want)
    assert recs == sorted(want)


@pytest.mark.parametrize("i", range(len(G.CASES)), ids=IDS)
def test_generated_case(i):
    circ, wit, fill = G.generate(**G.CASES[i])
    _, g, gl, params = _params(circ.k)
    pk = h2g.ProvingKey(params, circ)
    kg = O.Keygen(circ, wit, g, gl)
    assert (pk.degree, pk.bf) == (circ.degree(), circ.blinding_factors())
    assert (pk.degree, pk.bf, pk.extended_k, pk.nsets) == (kg.degree, kg.bf, kg.extended_k, kg.nsets)
    assert pk.n_slots >= max(G.sethi_ullman(e) for e in G.roots(circ))

    # ---- proof bytes
    ch = []
    if fill is None:
        want = O.create_proof(circ, wit, g, gl, keygen=kg)
        assert pk.create_proof(wit) == want
        assert pk.create_proof(wit) == want
        full = wit
    else:
        want = O.create_proof(circ, wit, g, gl, keygen=kg, fill=fill, challenges_out=ch)
        got, got_ch = pk.create_proof_phased(fill, wit)
        assert got_ch == ch
        assert got == want
        full = fill.full(ch)
        assert pk.create_proof(full) == want
        assert pk.create_proof_phased(fill, wit) == (want, ch)
    seed2 = bytes(range(32))   # other blinding rows: other commitments, so other challenges
    if fill is None:
        assert pk.create_proof(wit, seed=seed2, vanishing_threads=3) == \
            O.create_proof(circ, wit, g, gl, keygen=kg, seed=seed2, vanishing_threads=3)
    else:
        ch2 = []
        want2 = O.create_proof(circ, wit, g, gl, keygen=kg, fill=fill, challenges_out=ch2, seed=seed2,
                               vanishing_threads=3)
        assert pk.create_proof_phased(fill, wit, seed=seed2, vanishing_threads=3) == (want2, ch2)
        assert ch2 != ch

    # ---- an unsatisfied witness: one solved cell off, so a gate's quotient is no polynomial;
    # both provers divide and truncate alike
    gen = circ.gen
    rng = np.random.default_rng(1000 + i)
    col = gen["out0"] + gen["last_phase"][int(rng.integers(len(gen["last_phase"])))]
    row = int(rng.integers(*gen["active"]))
    off = (hc.fr_from_limbs(full.advice[col, row]) + 1 + int(rng.integers(1 << 62))) % hc.R_MOD
    broken = CR.set_cell(full, col, row, off)
    assert pk.create_proof(broken) == O.create_proof(circ, broken, g, gl, keygen=kg)
    assert pk.create_proof(full) == O.create_proof(circ, full, g, gl, keygen=kg)   # and the key is as it was

    # ---- the witness check
    device_check(pk, full, ch, set())
    want_broken = CR.check(circ, broken, ch)
    assert (CR.GATE, col - gen["out0"], row) in want_broken
    device_check(pk, broken, ch, want_broken)
    seen = 0
    for t in range(3):
        c2, r2 = int(rng.integers(circ.num_advice)), int(rng.integers(gen["u"]))
        value = G.EDGE[int(rng.integers(len(G.EDGE)))] if t == 1 else int.from_bytes(rng.bytes(31), "little")
        bad = CR.set_cell(full, c2, r2, value)
        want_bad = CR.check(circ, bad, ch, seed=t)
        device_check(pk, bad, ch, want_bad)
        seen += len(want_bad)
    assert seen > 0, "no corruption was visible: the parity says nothing"
    kg.close()
    pk.close()


MULTI = [IDS.index(x) for x in ("s203-k7-d5", "s302-k7-d6", "s402-k6-d12")]


@pytest.mark.parametrize("i", MULTI, ids=[IDS[i] for i in MULTI])
def test_two_witnesses_in_one_proof(i):
    """create_proof over two circuits: the same constraint system, witnesses from two seeds"""
    circ, w0, fill = G.generate(**G.CASES[i])
    _, w1, _ = G.generate(**G.CASES[i], witness_seed=9000 + i)
    assert fill is None and not np.array_equal(w0.advice, w1.advice)
    _, g, gl, params = _params(circ.k)
    pk = h2g.ProvingKey(params, circ)
    want = O.create_proof(circ, w0, g, gl, wits=[w0, w1])
    assert pk.create_proof_multi([w0, w1]) == want
    assert pk.create_proof_multi([w0, w1]) == want
    assert pk.create_proof_multi([w1, w0]) == O.create_proof(circ, w0, g, gl, wits=[w1, w0])
    assert pk.create_proof(w1) == O.create_proof(circ, w1, g, gl)
    pk.close()


def test_identity_commitments_are_refused():
    """the device refuses what the oracle refuses (tests/test_generated_circuits_cpu.py), says
    why, and goes on proving: the params with a sibling circuit's key, the same key with
    another witness"""
    circ, wit = G.zero_table_lookup(6, zero=True)
    _, g, gl, params = _params(circ.k)
    pk = h2g.ProvingKey(params, circ)
    for _ in range(2):
        with pytest.raises(h2g.H2GError, match="points at infinity"):
            pk.create_proof(wit)
    pk.close()
    circ, wit = G.zero_table_lookup(6, zero=False)
    pk = h2g.ProvingKey(params, circ)
    assert pk.create_proof(wit) == O.create_proof(circ, wit, g, gl)
    pk.close()
    circ, zero = G.unblinded_boolean(6, zero=True)
    _, bits = G.unblinded_boolean(6, zero=False)
    pk = h2g.ProvingKey(params, circ)
    want = O.create_proof(circ, bits, g, gl)
    assert pk.create_proof(bits) == want
    with pytest.raises(h2g.H2GError, match="points at infinity"):
        pk.create_proof(zero)
    assert pk.create_proof(bits) == want
    assert pk.check_witness(zero) == (0, [])   # the witness is fine; only its proof cannot be written
    pk.close()
