"""create_proof* with the prover's self-checks on (include/h2g.h; csrc/prover_selfcheck.cpp).

Valid witnesses: modes "verdict" and "arguments" return mode "off"'s bytes on every circuit
kind, multi-open scheme, transcript and key form, and report nothing.  Wrong witnesses: one
advice cell off in a usable row, which tests/_check_ref.py first confirms leaves a constraint
unsatisfied (and no lookup input outside its table: that stays H2G_ERR_ARG) -- mode "off"
returns bytes the verifier rejects, mode "verdict" refuses with H2G_ERR_UNSATISFIED, no bytes,
and records that name the fault; the key then proves a valid witness as a fresh key does."""
import ctypes

import numpy as np
import pytest

import _check_ref as CR
import _gen_circuit as G
import h2g
import h2g_circuit as hc

pytestmark = pytest.mark.gpu

OK, REJECTED = h2g.VERIFY_OK, h2g.VERIFY_REJECTED
S_INT = 0xC0FFEE
R = hc.R_MOD
SEEDS = list(range(8))
_PARAMS, _KEYS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _init():
    h2g.init()
    yield
    for kc in _KEYS.values():
        kc["vk"].close()
        kc["pk"].close()
    _KEYS.clear()
    for p in _PARAMS.values():
        p.close()
    _PARAMS.clear()


def params(k):
    if k not in _PARAMS:
        _PARAMS[k] = h2g.Params(k, s=np.asarray(hc.fr_to_limbs(S_INT), dtype=np.uint64))
    return _PARAMS[k]


# ----------------------------------------------------------------------------- the cases
def _plain(fn, *a):
    def build():
        circ, wit = fn(*a)
        return circ, [wit], [None]
    return build


def _phased(fn, *a):
    def build():
        circ, wit, fill = fn(*a)
        return circ, [wit], [fill]
    return build


def _gen(case_id):
    def build():
        i = [G.case_id(c) for c in G.CASES].index(case_id)
        circ, wit, fill = G.generate(**G.CASES[i])
        assert fill is None
        return circ, [wit], [None]
    return build


def _two():
    made = [hc.my_circuit(6, input_value=v) for v in (42, 1000)]
    return made[0][0], [m[1] for m in made], [m[2] for m in made]


CASES = {
    "simple_k8": _plain(hc.simple_example, 8),
    "mixed_k7": _plain(hc.mixed_circuit, 7),
    "lookup_k8": _plain(hc.lookup_circuit, 8),
    "challenge_k6": _phased(hc.challenge_circuit, 6),
    "my_circuit_k6": _phased(hc.my_circuit, 6),
    "gen_s203": _gen("s203-k7-d5"),
    "gen_s302": _gen("s302-k7-d6"),
    "gen_s402": _gen("s402-k6-d12"),
    "two_circuits": _two,
}
NAMES = list(CASES)


def key(name):
    if name not in _KEYS:
        circ, wits, fills = CASES[name]()
        pk = h2g.ProvingKey(params(circ.k), circ)
        _KEYS[name] = dict(circ=circ, wits=wits, fills=fills, pk=pk, vk=h2g.VerifyingKey.from_pk(pk))
    return _KEYS[name]


def prove(kc, mode="off", wits=None, fills=None, multiopen="shplonk", transcript="blake2b", pk=None,
          seed=bytes([7] * 32)):
    wits = wits or kc["wits"]
    fills = fills or kc["fills"]
    pk = pk or kc["pk"]
    pk.set_self_check(mode)
    try:
        if fills[0] is not None:
            return pk.create_proof_multi(wits, seed=seed, fills=fills, multiopen=multiopen, transcript=transcript)
        if len(wits) > 1:
            return pk.create_proof_multi(wits, seed=seed, multiopen=multiopen, transcript=transcript)
        return pk.create_proof(wits[0], seed=seed, multiopen=multiopen, transcript=transcript)
    finally:
        pk.set_self_check("off")


def columns(kc, wits=None):
    return [h2g.instance_columns(w, kc["circ"]) for w in (wits or kc["wits"])]


def last_challenges(circ):
    ch = np.zeros((max(circ.num_challenges, 1), 4), dtype=np.uint64)
    cnt = ctypes.c_int()
    h2g.check(h2g.lib().h2g_last_challenges(h2g.p64(ch), circ.num_challenges, ctypes.byref(cnt)))
    return hc.mont_to_ints(ch[: cnt.value])


def refused(kc, **kw):
    """mode "verdict" on a wrong witness -> the error"""
    with pytest.raises(h2g.UnsatisfiedError) as e:
        prove(kc, "verdict", **kw)
    assert e.value.code == h2g.ERR_UNSATISFIED and "self-check" in str(e.value)
    assert e.value.total >= 1 and e.value.failures == h2g.last_self_check()[1]
    assert e.value.failures == sorted(e.value.failures, key=lambda r: (r[3], r[0], r[1], r[2]))
    return e.value


# ----------------------------------------------------------------------------- valid witnesses
COMBOS = [("shplonk", "blake2b"), ("gwc", "blake2b"), ("shplonk", "keccak256"), ("gwc", "keccak256")]


@pytest.mark.parametrize("name", NAMES)
def test_valid_witness_same_bytes_in_every_mode(name):
    kc = key(name)
    for multiopen, transcript in COMBOS:
        base = prove(kc, "off", multiopen=multiopen, transcript=transcript)
        assert kc["vk"].verify(base, columns(kc), multiopen, transcript) == OK
        for mode in ("verdict", "arguments"):
            assert prove(kc, mode, multiopen=multiopen, transcript=transcript) == base, (mode, multiopen, transcript)
            assert h2g.last_self_check() == (0, [])


@pytest.mark.parametrize("name", ["mixed_k7", "my_circuit_k6"])
def test_valid_witness_streamed_key(name):
    kc = key(name)
    base = prove(kc, "off")
    pk = h2g.ProvingKey(params(kc["circ"].k), kc["circ"], cosets="streamed")
    for mode in ("off", "verdict", "arguments"):
        assert prove(kc, mode, pk=pk) == base
        assert h2g.last_self_check() == (0, [])
    pk.close()


def test_valid_witness_device_resident_and_assigned_entries():
    """the other two entry points: device-resident advice, and Assigned cells"""
    kc = key("mixed_k7")
    base = prove(kc, "off")
    d_adv = h2g.DevBuf.from_array(np.ascontiguousarray(kc["wits"][0].advice))
    for mode in ("verdict", "arguments"):
        kc["pk"].set_self_check(mode)
        assert kc["pk"].create_proof(kc["wits"][0], advice_dev_ptr=d_adv.ptr) == base
    kc["pk"].set_self_check("off")
    d_adv.close()
    wit = kc["wits"][0]

    def fill(phase, ch):
        cols = {c: wit.advice[c] for c in range(kc["circ"].num_advice) if kc["circ"].advice_phase[c] == phase}
        return cols, None, None

    for mode in ("off", "verdict", "arguments"):
        kc["pk"].set_self_check(mode)
        assert kc["pk"].create_proof_assigned([fill], [wit]) == base
    kc["pk"].set_self_check("off")


# ----------------------------------------------------------------------------- wrong witnesses
def corrupt_fill(fill, col, row, value):
    def f(phase, ch):
        out = dict(fill(phase, ch))
        if col in out:
            v = np.array(out[col], copy=True)
            v[row] = hc.fr_to_limbs(value)
            out[col] = v
        return out
    f.full = lambda ch: CR.set_cell(fill.full(ch), col, row, value)
    return f


def corruption(kc, seed, circuit=0):
    """one advice cell of a usable row set to another row's value of its column (which keeps
    lookup inputs inside their tables more often than a random value would) -> (wits, fills,
    full(challenges) -> the complete wrong witness of that circuit).  The draw is repeated until
    tests/_check_ref.py sees a failure and no lookup failure: no seed is skipped."""
    circ = kc["circ"]
    rng = np.random.default_rng([seed, circuit, len(circ.gates)])
    u = circ.usable_rows()
    base_fill = kc["fills"][circuit]
    for _ in range(200):
        col, row, other = int(rng.integers(circ.num_advice)), int(rng.integers(u)), int(rng.integers(u))
        ch0 = [3] * circ.num_challenges
        full0 = base_fill.full(ch0) if base_fill else kc["wits"][circuit]
        value = hc.fr_from_limbs(full0.advice[col, other])
        if value == hc.fr_from_limbs(full0.advice[col, row]):
            value = (value + 1 + int(rng.integers(1 << 30))) % R
        if base_fill:
            bad_fill = corrupt_fill(base_fill, col, row, value)
            full = bad_fill.full
        else:
            bad = CR.set_cell(kc["wits"][circuit], col, row, value)
            bad_fill, full = None, (lambda ch, bad=bad: bad)
        want = CR.check(circ, full(ch0), ch0)
        if not want or any(k == CR.LOOKUP for k, _, _ in want):
            continue
        wits, fills = list(kc["wits"]), list(kc["fills"])
        if bad_fill:
            fills[circuit] = bad_fill
        else:
            wits[circuit] = bad
        return wits, fills, full
    raise AssertionError("no visible corruption found")


def gate_records(recs):
    return sorted(r[:3] for r in recs if r[0] in (CR.GATE, CR.GATE_BLINDING))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", NAMES)
def test_wrong_cell_is_refused_and_located(name, seed):
    kc = key(name)
    circ, pk = kc["circ"], kc["pk"]
    circuit = len(kc["wits"]) - 1   # (two circuits: the second one is wrong)
    wits, fills, full = corruption(kc, seed, circuit)
    # mode off: bytes, which the verifier rejects
    proof = prove(kc, "off", wits=wits, fills=fills)
    assert len(proof) > 0 and h2g.last_self_check() == (0, [])
    assert kc["vk"].verify(proof, columns(kc, wits)) == REJECTED
    ch = last_challenges(circ)
    want = CR.check(circ, full(ch), ch)   # with the proof's own challenges
    assert want and not any(k == CR.LOOKUP for k, _, _ in want)
    # mode verdict: refused, and the same challenges again (the refusal comes after them)
    err = refused(kc, wits=wits, fills=fills)
    assert last_challenges(circ) == ch
    recs = err.failures
    assert all(r[3] == circuit for r in recs)
    assert all(r[0] in (CR.GATE, CR.GATE_BLINDING, CR.SHUFFLE, h2g.CHECK_PERMUTATION) for r in recs)
    # the gate records: h2g_check_witness's for the same witness and challenges, wherever they
    # do not depend on the blinding rows (two seeds of its own agree)
    a = pk.check_witness(full(ch), challenges=ch, copies=False, seed=bytes([1] * 32))[1]
    b = pk.check_witness(full(ch), challenges=ch, copies=False, seed=bytes([2] * 32))[1]
    if gate_records(a) == gate_records(b):
        assert gate_records(recs) == gate_records(a) == sorted(w for w in want if w[0] in (CR.GATE, CR.GATE_BLINDING))
    # the other arguments, one record each, exactly where the restatement finds one
    assert sorted(r[:3] for r in recs if r[0] == CR.SHUFFLE) == sorted(w for w in want if w[0] == CR.SHUFFLE)
    perm = [r for r in recs if r[0] == h2g.CHECK_PERMUTATION]
    assert perm == ([(h2g.CHECK_PERMUTATION, pk.nsets - 1, circ.usable_rows(), circuit)]
                    if any(w[0] == CR.COPY for w in want) else [])
    # mode arguments: refused alike -- the arguments were built right, the witness is wrong
    with pytest.raises(h2g.UnsatisfiedError) as e2:
        prove(kc, "arguments", wits=wits, fills=fills)
    assert e2.value.failures == recs
    # and the key proves the valid witness as before
    if seed == SEEDS[-1]:
        fresh = h2g.ProvingKey(params(circ.k), circ)
        assert prove(kc, "verdict") == prove(kc, "off", pk=fresh)
        fresh.close()


def test_refusal_writes_no_bytes():
    """the C entry itself: H2G_ERR_UNSATISFIED, *proof_len = 0, the buffer untouched"""
    kc = key("mixed_k7")
    circ, pk = kc["circ"], kc["pk"]
    wit = kc["wits"][0]
    bad = CR.set_cell(wit, 3, 9, hc.fr_from_limbs(wit.advice[3, 10]))   # tests/_check_ref.py's anchor
    assert CR.check(circ, bad) == {(CR.GATE, 0, 9), (CR.GATE, 3, 9)}
    adv = np.ascontiguousarray(bad.advice, dtype=np.uint64)
    ins = np.ascontiguousarray(bad.instance, dtype=np.uint64) if circ.num_instance else np.zeros(4, np.uint64)
    lens = np.ascontiguousarray(bad.instance_lens if circ.num_instance else np.zeros(1), dtype=np.uint32)
    buf = ctypes.create_string_buffer(b"\xAA" * 65536, 65536)
    ln = h2g.SZ(12345)
    pk.set_self_check("verdict")
    rc = h2g.lib().h2g_create_proof(pk.params.handle, pk.handle, h2g.VP(adv.ctypes.data), 0, h2g.p64(ins),
                                    lens.ctypes.data_as(ctypes.POINTER(h2g.U32)), bytes([7] * 32), 8, buf, 65536,
                                    ctypes.byref(ln))
    pk.set_self_check("off")
    assert rc == h2g.ERR_UNSATISFIED and ln.value == 0
    assert buf.raw == b"\xAA" * 65536
    assert b"self-check" in h2g.lib().h2g_last_error()
    total, recs = h2g.last_self_check(cap=1)   # total is exact past cap
    assert total == 2 and recs == [(CR.GATE, 0, 9, 0)]


def test_broken_copy_gives_one_permutation_record():
    """simple_example: a public input changed -- every gate holds, one copy does not"""
    kc = key("simple_k8")
    circ = kc["circ"]
    wit = kc["wits"][0]
    ins = wit.instance.copy()
    ins[0, 1] = hc.fr_to_limbs((hc.fr_from_limbs(ins[0, 1]) + 1) % R)
    bad = hc.Witness(wit.advice, ins, wit.instance_lens)
    want = CR.check(circ, bad)
    assert want and all(k == CR.COPY for k, _, _ in want)
    proof = prove(kc, "off", wits=[bad])
    assert kc["vk"].verify(proof, columns(kc, [bad])) == REJECTED
    err = refused(kc, wits=[bad])
    assert (err.total, err.failures) == (1, [(h2g.CHECK_PERMUTATION, kc["pk"].nsets - 1, circ.usable_rows(), 0)])
    assert prove(kc, "verdict") == prove(kc, "off")


def test_shuffle_with_one_changed_value():
    kc = key("lookup_k8")
    circ = kc["circ"]
    bad = CR.set_cell(kc["wits"][0], 3, 2, 1)
    want = CR.check(circ, bad)
    assert want == {(CR.SHUFFLE, 0, CR.NO_ROW)}
    assert kc["vk"].verify(prove(kc, "off", wits=[bad]), columns(kc, [bad])) == REJECTED
    err = refused(kc, wits=[bad])
    assert (err.total, err.failures) == (1, [(CR.SHUFFLE, 0, CR.NO_ROW, 0)])


def test_phase_one_cell_located_with_the_proofs_challenges():
    """challenge_circuit: z (phase 1) off at one row; the failing gate rows come from the
    challenges this very proof squeezed"""
    kc = key("challenge_k6")
    circ, fill = kc["circ"], kc["fills"][0]
    ch0 = [5, 6]
    z = fill.full(ch0).advice
    assert hc.fr_from_limbs(z[1, 10]) != 77
    bad_fill = corrupt_fill(fill, 1, 10, 77)
    err = refused(kc, fills=[bad_fill])
    ch = last_challenges(circ)
    assert len(ch) == 2 and ch != ch0
    want = CR.check(circ, bad_fill.full(ch), ch)
    assert want == {(CR.GATE, 0, 9), (CR.GATE, 0, 10)}
    assert [r[:3] for r in err.failures] == sorted(want)


# ----------------------------------------------------------------------------- mode "arguments"
def test_nonzero_unusable_rows():
    """an unblinded column (its rows [u, n) go into the commitment as handed in) that is not zero
    there: no gate is live in those rows, so modes "off" and "verdict" prove it and the proof
    verifies; mode "arguments" refuses it as the reference's sanity-checks do.  A blinded
    column's rows there are overwritten and not asked (challenge_circuit's `a` is random on all n
    rows, and proves in every mode above)."""
    circ, wit = G.unblinded_boolean(6, zero=False)
    n, u = circ.n, circ.usable_rows()
    assert circ.unblinded[0] and not circ.unblinded[1]
    pk = h2g.ProvingKey(params(circ.k), circ)
    vk = h2g.VerifyingKey.from_pk(pk)
    kc = dict(circ=circ, wits=[wit], fills=[None], pk=pk, vk=vk)
    base = prove(kc, "off")
    assert prove(kc, "arguments") == base
    adv = wit.advice.copy()
    adv[0, u] = hc.fr_to_limbs(5)
    adv[0, n - 1] = hc.fr_to_limbs(6)
    adv[1, u + 1] = hc.fr_to_limbs(7)      # the blinded column: not asked
    bad = hc.Witness(adv, wit.instance, wit.instance_lens)
    proof = prove(kc, "off", wits=[bad])
    assert proof != base and vk.verify(proof, columns(kc, [bad])) == OK
    assert prove(kc, "verdict", wits=[bad]) == proof
    with pytest.raises(h2g.UnsatisfiedError) as e:
        prove(kc, "arguments", wits=[bad])
    assert e.value.failures == [(h2g.CHECK_UNUSABLE_ROW, 0, u, 0), (h2g.CHECK_UNUSABLE_ROW, 0, n - 1, 0)]
    assert prove(kc, "arguments") == base
    vk.close()
    pk.close()


def test_missing_lookup_input_stays_an_argument_error():
    kc = key("lookup_k8")
    bad = CR.set_cell(kc["wits"][0], 0, 5, 300)
    assert any(k == CR.LOOKUP for k, _, _ in CR.check(kc["circ"], bad))
    for mode in ("off", "verdict", "arguments"):
        with pytest.raises(h2g.H2GError, match="h2g error 1.*not in the table") as e:
            prove(kc, mode, wits=[bad])
        assert not isinstance(e.value, h2g.UnsatisfiedError) and e.value.failures == []
        assert h2g.last_self_check() == (0, [])
    assert kc["vk"].verify(prove(kc, "verdict"), columns(kc)) == OK


# ----------------------------------------------------------------------------- transports
def test_refused_under_a_transport():
    kc = key("simple_k8")
    called = []

    def boom(*a):
        called.append(a)
        raise RuntimeError("a checked proof must not reach the transport")

    base = prove(kc, "off")
    h2g.set_spmd_transport(2, 0, allgather=boom, allgather_host=boom)
    try:
        for mode in ("verdict", "arguments"):
            with pytest.raises(h2g.H2GError, match="h2g error 4.*transport"):
                prove(kc, mode)
    finally:
        h2g.set_spmd_transport(1)
    h2g.set_shard_transport(2, launch=boom, collect=boom)
    try:
        with pytest.raises(h2g.H2GError, match="h2g error 4.*transport"):
            prove(kc, "verdict")
    finally:
        h2g.set_shard_transport(1)
    assert not called and not h2g.transport_errors()
    assert prove(kc, "verdict") == base


def test_mode_off_proves_under_a_working_transport():
    """two ranks over a working SPMD transport (tests/_selfcheck_spmd.py, one process per rank,
    sharing the GPU): with it installed modes "verdict" and "arguments" are H2G_ERR_STATE on every
    rank, mode "off" on the same key proves the single-device bytes through the collectives"""
    import json
    import os
    import socket
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(here, "_selfcheck_spmd.py")]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    line = [ln for ln in out.splitlines() if ln.startswith("SELFCHECK_SPMD ")]
    assert line, out[-4000:]
    ranks = json.loads(line[-1][len("SELFCHECK_SPMD "):])
    assert len(ranks) == 2
    for res in ranks:
        assert res["alone"] == {"verdict": True, "arguments": True}
        assert res["installed"] == {"verdict": [h2g.ERR_STATE, True], "arguments": [h2g.ERR_STATE, True], "off": True}
        assert res["gathers"] > 0      # mode off did go through the transport
        assert res["after"] is True

