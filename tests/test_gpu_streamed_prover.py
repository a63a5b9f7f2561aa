"""A key made with cosets="streamed" holds one n-point slot per column where a resident key
holds an extended coset, and gives the same bytes everywhere: proofs (against the C
restatement prover, and at k = 16 against a resident key), written keys in all three formats,
verifying-key commitments and witness-check records.  Its memory is measured from outside the
library's own accounting (free device bytes around keygen + proof + close).
"""
import re

import numpy as np
import pytest

import _check_ref as CR
import _gen_circuit as G
import _oracle as O
import bn254_ref as B
import h2g
import h2g_circuit as hc

pytestmark = pytest.mark.gpu

_PARAMS = {}
SEED2 = bytes(range(32))


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


def _case(seed):
    return next(c for c in G.CASES if c["seed"] == seed)


def _streamed(params, circ, **kw):
    pk = h2g.ProvingKey(params, circ, cosets="streamed", **kw)
    assert pk.memory()["cosets"] == "streamed"
    return pk


def _code(fn, *a, **kw):
    """the library's error code of a call that must fail"""
    with pytest.raises(h2g.H2GError) as e:
        fn(*a, **kw)
    return int(re.match(r"h2g error (\d+):", str(e.value)).group(1))


# ------------------------------------------------------------------ proofs against the oracle
# domains 2n (s105), 4n (s203, s206, s502), 8n (s308, s302, s505), 16n (s406); lookups with
# shared (s206) and advice-backed (s308) tables, shuffles, three phases (s502, s505)
GENERATED = [105, 203, 206, 302, 308, 406, 502, 505]


@pytest.mark.parametrize("seed", GENERATED, ids=[f"s{s}" for s in GENERATED])
def test_streamed_generated_case(seed):
    circ, wit, fill = G.generate(**_case(seed))
    _, g, gl, params = _params(circ.k)
    pk = _streamed(params, circ)
    kg = O.Keygen(circ, wit, g, gl)
    assert (pk.degree, pk.bf, pk.extended_k, pk.nsets) == (kg.degree, kg.bf, kg.extended_k, kg.nsets)
    if fill is None:
        want = O.create_proof(circ, wit, g, gl, keygen=kg)
        assert pk.create_proof(wit) == want
        assert pk.create_proof(wit) == want
        assert pk.create_proof(wit, seed=SEED2, vanishing_threads=3) == \
            O.create_proof(circ, wit, g, gl, keygen=kg, seed=SEED2, vanishing_threads=3)
    else:
        ch, ch2 = [], []
        want = O.create_proof(circ, wit, g, gl, keygen=kg, fill=fill, challenges_out=ch)
        assert pk.create_proof_phased(fill, wit) == (want, ch)
        assert pk.create_proof(fill.full(ch)) == want
        want2 = O.create_proof(circ, wit, g, gl, keygen=kg, fill=fill, challenges_out=ch2, seed=SEED2,
                               vanishing_threads=3)
        assert pk.create_proof_phased(fill, wit, seed=SEED2, vanishing_threads=3) == (want2, ch2)
        assert ch2 != ch
    kg.close()
    pk.close()


@pytest.mark.parametrize("multiopen", ["shplonk", "gwc"])
def test_streamed_keccak_style_keccak_transcript(multiopen):
    circ, wit = hc.keccak_style(9, words=16, seed=3)
    _, g, gl, params = _params(circ.k)
    pk = _streamed(params, circ)
    assert pk.create_proof(wit, multiopen=multiopen, transcript="keccak256") == \
        O.create_proof(circ, wit, g, gl, multiopen=multiopen, transcript="keccak256")
    assert pk.create_proof(wit, multiopen=multiopen) == O.create_proof(circ, wit, g, gl, multiopen=multiopen)
    pk.close()


def test_streamed_synthetic_c3():
    circ, wit = hc.synthetic_c3(12, O.OracleOps, seed=2)
    _, g, gl, params = _params(circ.k)
    pk = _streamed(params, circ)
    assert pk.create_proof(wit) == O.create_proof(circ, wit, g, gl)
    assert pk.create_proof(wit, seed=SEED2, vanishing_threads=3) == \
        O.create_proof(circ, wit, g, gl, seed=SEED2, vanishing_threads=3)
    pk.close()


@pytest.mark.parametrize("seed", [203, 402], ids=["s203", "s402"])
def test_streamed_two_witnesses_in_one_proof(seed):
    """the Horner chain in y continues across the circuits of a proof through every sub-coset"""
    case = _case(seed)
    circ, w0, fill = G.generate(**case)
    _, w1, _ = G.generate(**case, witness_seed=9000 + seed)
    assert fill is None and not np.array_equal(w0.advice, w1.advice)
    _, g, gl, params = _params(circ.k)
    pk = _streamed(params, circ)
    assert pk.create_proof_multi([w0, w1]) == O.create_proof(circ, w0, g, gl, wits=[w0, w1])
    assert pk.create_proof_multi([w1, w0]) == O.create_proof(circ, w0, g, gl, wits=[w1, w0])
    assert pk.create_proof(w1) == O.create_proof(circ, w1, g, gl)  # and back to one workspace's worth
    pk.close()


def test_streamed_unsatisfied_witness_and_witness_check():
    circ, wit, fill = G.generate(**_case(308))
    assert fill is None
    _, g, gl, params = _params(circ.k)
    pk = _streamed(params, circ)
    res = h2g.ProvingKey(params, circ)
    gen = circ.gen
    rng = np.random.default_rng(5)
    col = gen["out0"] + gen["last_phase"][int(rng.integers(len(gen["last_phase"])))]
    row = int(rng.integers(*gen["active"]))
    off = (hc.fr_from_limbs(wit.advice[col, row]) + 1 + int(rng.integers(1 << 62))) % hc.R_MOD
    broken = CR.set_cell(wit, col, row, off)
    want = O.create_proof(circ, broken, g, gl)
    assert pk.create_proof(broken) == want  # the quotient is no polynomial: both divide and truncate alike
    assert res.create_proof(broken) == want
    assert pk.create_proof(wit) == O.create_proof(circ, wit, g, gl)
    for w in (wit, broken):
        got = pk.check_witness(w, cap=256)
        assert got == res.check_witness(w, cap=256)
    assert pk.check_witness(wit) == (0, [])
    assert pk.check_witness(broken, cap=256)[0] > 0
    # the sort hints are what the key's last proof measured: the same proof last on both
    assert res.create_proof(wit) == pk.create_proof(wit)
    assert pk.lookup_sort_hints() == res.lookup_sort_hints()
    pk.close()
    res.close()


# ------------------------------------------------------------------ k = 16 against a resident key
def _same_as_resident(circ, wit, params):
    res = h2g.ProvingKey(params, circ)
    want = [res.create_proof(wit), res.create_proof(wit, seed=SEED2, vanishing_threads=3)]
    res.close()
    pk = _streamed(params, circ)
    got = [pk.create_proof(wit), pk.create_proof(wit, seed=SEED2, vanishing_threads=3)]
    pk.close()
    assert want[0] != want[1]
    assert got == want


def test_streamed_k16_synthetic_c3():
    circ, wit = hc.synthetic_c3(16, O.OracleOps, seed=2)
    _same_as_resident(circ, wit, _params(16)[3])


def test_streamed_k16_degree9_generated():
    """(most of this test's time is the witness generation on the CPU, ~9 s)"""
    circ, wit, fill = G.generate(seed=778, k=16, degree=9, gates=1, nodes=(30, 31), lookups=(1,), shuffle=True)
    assert fill is None and circ.degree() == 9
    _same_as_resident(circ, wit, _params(16)[3])


# ------------------------------------------------------------------ key bytes
@pytest.mark.parametrize("seed", [206, 505], ids=["s206", "s505"])
def test_streamed_key_bytes(seed):
    circ, wit, fill = G.generate(**_case(seed))
    _, g, gl, params = _params(circ.k)
    res = h2g.ProvingKey(params, circ)
    pk = _streamed(params, circ)

    def prove(key):
        return key.create_proof_phased(fill, wit)[0] if fill is not None else key.create_proof(wit)

    want = prove(res)
    assert prove(pk) == want
    files = {}
    for fmt in (h2g.RAW_BYTES, h2g.RAW_BYTES_UNCHECKED, h2g.PROCESSED):
        files[fmt] = res.write(fmt)
        assert pk.write(fmt) == files[fmt], fmt
        assert prove(pk) == want  # writing went through the h(X) buffer; the key is as it was
        back = _streamed(params, circ, data=files[fmt], fmt=fmt)
        assert prove(back) == want, fmt
        assert back.write(fmt) == files[fmt], fmt
        back.close()
    assert np.array_equal(pk.vk_commitments()[0], res.vk_commitments()[0])
    assert np.array_equal(pk.vk_commitments()[1], res.vk_commitments()[1])
    # a coset element that is no canonical field element is refused by both reads alike
    # (Processed: from_repr; RawBytes: the reduced-limbs check), the same file with r - 1 is not
    for fmt in (h2g.PROCESSED, h2g.RAW_BYTES):
        bad = bytearray(files[fmt])
        bad[-32:] = B.R.to_bytes(32, "little")  # the last permutation coset's last element
        codes = [_code(h2g.ProvingKey, params, circ, data=bytes(bad), fmt=fmt, cosets=c)
                 for c in ("resident", "streamed")]
        assert codes[0] == codes[1] == 1, (fmt, codes)  # H2G_ERR_ARG
        for trunc in (files[fmt][:-1], files[fmt] + b"\x00"):
            assert _code(h2g.ProvingKey, params, circ, data=trunc, fmt=fmt, cosets="streamed") == \
                _code(h2g.ProvingKey, params, circ, data=trunc, fmt=fmt)
    ok = bytearray(files[h2g.PROCESSED])
    ok[-32:] = (B.R - 1).to_bytes(32, "little")
    _streamed(params, circ, data=bytes(ok), fmt=h2g.PROCESSED).close()
    pk.close()
    res.close()


def test_streamed_verifying_key():
    circ, wit, _ = G.generate(**_case(206))
    # params with their G2 half (the verifier's), from a known s
    params = h2g.Params(circ.k, s=np.asarray(hc.fr_to_limbs(0x5eed0123456789abcdef), dtype=np.uint64))
    pk = _streamed(params, circ)
    vk = h2g.VerifyingKey.from_pk(pk)
    res = h2g.ProvingKey(params, circ)
    assert pk.create_proof(wit) == res.create_proof(wit)
    for a, b in zip(pk.vk_commitments(), res.vk_commitments()):
        assert np.array_equal(a, b)
    res.close()
    proof = pk.create_proof(wit)
    assert vk.verify(proof, [h2g.instance_columns(wit, circ)]) == h2g.VERIFY_OK
    flipped = bytearray(proof)
    flipped[-1] ^= 1
    assert vk.verify(bytes(flipped), [h2g.instance_columns(wit, circ)]) != h2g.VERIFY_OK
    vk.close()
    pk.close()
    params.close()


# ------------------------------------------------------------------ memory
def test_streamed_memory():
    """Free device bytes around keygen + first proof + close, per mode, at k = 12 with a
    degree-9 circuit (2^e = 8).  A resident key holds C extended cosets, C = F + P + A + I +
    nsets + 3 NL + NS (plus l_0, l_last, l_active), a streamed key C slots of n: the difference
    is at least C (ext - n) 32 bytes; half of it is required, the margin for allocator
    granularity.  The streamed key's extended arrays are h_ext, h_coeff and h_gather, 3 ext 32
    bytes: the SHPLONK workspace holds nothing in extended form (its buffers are n-point)."""
    circ, wit, fill = G.generate(seed=777, k=12, degree=9, lookups=(1,), shuffle=True)
    assert fill is None and circ.degree() == 9
    _, g, gl, params = _params(circ.k)
    n = 1 << circ.k

    def run(cosets):
        free0 = h2g.device_mem_info()[0]
        pk = h2g.ProvingKey(params, circ, cosets=cosets)
        proof = pk.create_proof(wit)
        mem = pk.memory()
        held = free0 - h2g.device_mem_info()[0]
        shape = (pk.extended_k, pk.nsets)
        pk.close()
        return proof, mem, held, free0, h2g.device_mem_info()[0], shape

    for c in ("resident", "streamed"):  # the device's own buffers (transform tables, work space) grow here
        run(c)
    p_res, m_res, held_res, start_res, end_res, (ek, nsets) = run("resident")
    p_str, m_str, held_str, start_str, end_str, _ = run("streamed")
    assert p_str == p_res
    ext = 1 << ek
    assert ext == 8 * n
    C = (circ.num_fixed + len(circ.perm_columns) + circ.num_advice + circ.num_instance + nsets
         + 3 * len(circ.lookups) + len(circ.shuffles))
    print(f"C = {C}, held resident {held_res}, streamed {held_str}, saved {held_res - held_str}, "
          f"C (ext - n) 32 = {C * (ext - n) * 32}; memory() resident {m_res}, streamed {m_str}")
    assert held_str <= held_res - C * (ext - n) * 32 // 2
    assert end_res == start_res and end_str == start_str
    assert m_str["ext_bytes"] <= 3 * ext * 32
    assert m_res["ext_bytes"] == (C + 3 + 2) * ext * 32  # the cosets, l_0 / l_last / l_active, h_ext and h_coeff
    assert m_str["bytes"] <= m_res["bytes"] - C * (ext - n) * 32
    assert m_res["cosets"] == "resident" and m_str["cosets"] == "streamed"


# ------------------------------------------------------------------ SPMD
def test_streamed_refused_under_spmd_transport():
    circ, wit, _ = G.generate(**_case(203))
    _, g, gl, params = _params(circ.k)
    pk = _streamed(params, circ)
    want = O.create_proof(circ, wit, g, gl)
    called = []

    def dummy(*a):
        called.append(a)
        raise RuntimeError("a streamed key must not reach the transport")

    h2g.set_spmd_transport(2, 0, allgather=dummy, bcast=dummy, allgather_host=dummy, exchange=dummy)
    try:
        with pytest.raises(h2g.H2GError, match="streamed"):
            pk.create_proof(wit)
        assert _code(pk.create_proof, wit) == 4  # H2G_ERR_STATE
    finally:
        h2g.set_spmd_transport(1)
    assert not called
    assert pk.create_proof(wit) == want
    pk.close()
