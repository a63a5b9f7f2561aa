"""The device prover on generated circuits whose h(X) splits unevenly at a multi-pass size
(tests/_gen_circuit.py LARGE_CASES, pinned valid by tests/test_generated_circuits_cpu.py):
degrees 4, 6, 7, 8, 12 and 16 at k = 11 and 12, so extended_to_coeff runs on 2^13 .. 2^16
points, ends in the truncated last pass and hands 3, 5, 6, 7, 11 or 15 pieces to the
commitments.  The generated circuits of test_gpu_generated_circuits.py with such degrees sit at
k <= 7, where the one-block kernel does the whole transform.

Proof bytes against the C restatement prover for a satisfying and an unsatisfied witness (both
provers divide and truncate alike), h2g_check_witness against the plain-Python restatement, the
native verifier's verdict, and for two cases a key with cosets="streamed": h_gather and
subcoset_scatter then feed the same truncated transform."""
import numpy as np
import pytest

import _check_ref as CR
import _gen_circuit as G
import _ntt_shapes as S
import _oracle as O
import h2g
import h2g_circuit as hc

pytestmark = pytest.mark.gpu

_PARAMS = {}
IDS = [G.case_id(c) for c in G.LARGE_CASES]
SEED2 = bytes(range(32))
STREAMED = [i for i, c in enumerate(G.LARGE_CASES) if c["degree"] in (6, 7)]


@pytest.fixture(scope="module", autouse=True)
def _init():
    h2g.init()
    yield
    for _, _, _, p in _PARAMS.values():
        p.close()
    _PARAMS.clear()


def _params(k):
    """the oracle's SRS of k from its secret, so the params also carry the verifier's points"""
    if k not in _PARAMS:
        s, g, gl = O.srs(k)
        _PARAMS[k] = (s, g, gl, h2g.Params(k, s=np.asarray(hc.fr_to_limbs(s), dtype=np.uint64)))
    return _PARAMS[k]


def _require_truncated(circ, pk):
    """the key's extended_to_coeff takes the truncated last pass with its epilogue product"""
    pl = S.domain_plans(pk.degree, circ.k)["e2c"]
    assert pk.extended_k == S.extended_k(pk.degree, circ.k) > 10
    assert len(pl["split"]) >= 2 and (pl["trunc"], pl["one"]) == (True, False), pl


def device_check(pk, wit, want):
    total, recs = pk.check_witness(wit, challenges=[], cap=max(64, len(want) + 8))
    assert total == len(want)
    assert recs == sorted(want)


@pytest.mark.parametrize("i", range(len(G.LARGE_CASES)), ids=IDS)
def test_large_generated_case(i):
    circ, wit, fill = G.generate(**G.LARGE_CASES[i])
    assert fill is None
    _, g, gl, params = _params(circ.k)
    pk = h2g.ProvingKey(params, circ)
    kg = O.Keygen(circ, wit, g, gl)
    assert (pk.degree, pk.bf, pk.extended_k, pk.nsets) == (kg.degree, kg.bf, kg.extended_k, kg.nsets)
    _require_truncated(circ, pk)

    want = O.create_proof(circ, wit, g, gl, keygen=kg)
    assert pk.create_proof(wit) == want
    assert pk.create_proof(wit) == want
    assert pk.create_proof(wit, seed=SEED2, vanishing_threads=3) == \
        O.create_proof(circ, wit, g, gl, keygen=kg, seed=SEED2, vanishing_threads=3)

    vk = h2g.VerifyingKey.from_pk(pk)
    assert vk.verify(want, [h2g.instance_columns(wit, circ)]) == h2g.VERIFY_OK

    # an unsatisfied witness: one solved cell off, so a gate's quotient is no polynomial and
    # h(X) has coefficients in every piece; both provers divide and truncate alike
    gen = circ.gen
    rng = np.random.default_rng(7000 + i)
    col = gen["out0"] + gen["last_phase"][int(rng.integers(len(gen["last_phase"])))]
    row = int(rng.integers(*gen["active"]))
    off = (hc.fr_from_limbs(wit.advice[col, row]) + 1 + int(rng.integers(1 << 62))) % hc.R_MOD
    broken = CR.set_cell(wit, col, row, off)
    bad = O.create_proof(circ, broken, g, gl, keygen=kg)
    assert pk.create_proof(broken) == bad
    assert vk.verify(bad, [h2g.instance_columns(broken, circ)]) == h2g.VERIFY_REJECTED
    assert pk.create_proof(wit) == want   # and the key is as it was

    device_check(pk, wit, set())
    want_broken = CR.check(circ, broken, [])
    assert (CR.GATE, col - gen["out0"], row) in want_broken
    device_check(pk, broken, want_broken)

    if i in STREAMED:
        sk = h2g.ProvingKey(params, circ, cosets="streamed")
        assert sk.memory()["cosets"] == "streamed"
        assert (sk.degree, sk.extended_k) == (pk.degree, pk.extended_k)
        assert sk.create_proof(wit) == want
        assert sk.create_proof(wit, seed=SEED2, vanishing_threads=3) == \
            pk.create_proof(wit, seed=SEED2, vanishing_threads=3)
        assert sk.create_proof(broken) == bad
        sk.close()
    vk.close()
    kg.close()
    pk.close()
