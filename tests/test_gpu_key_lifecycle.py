"""A proving key owns its device resources: its workspace grows to the largest proof it has
made and keeps nothing it has outgrown, closing it gives everything back, and a failed keygen
or read leaves nothing behind.  All on hc.my_circuit(6) (k = 6, one lookup, one shuffle, two
advice phases); the proofs are the oracle's (oracle/c/prover.c) byte for byte, the memory
figures h2g.device_mem_info()'s free bytes, as in test_gpu_descriptors.py."""
import numpy as np
import pytest

import _check_ref as R
import _oracle as O
import h2g
import h2g_circuit as hc

pytestmark = pytest.mark.gpu

SCHEMES = ("shplonk", "gwc")
SEQUENCE = (1, 3, 1, 2, 3)  # circuits per proof: growth, then smaller proofs in the grown buffers


class _Env:
    """the circuit, two witnesses (input 42 and 1000), the params and the oracle's proofs"""

    def __init__(self):
        self.circ, w0, f0 = hc.my_circuit(6, input_value=42)
        _, w1, f1 = hc.my_circuit(6, input_value=1000)
        self.wits, self.fills = (w0, w1), (f0, f1)
        _, self.g, self.gl = O.srs(self.circ.k)
        self.params = h2g.Params(self.circ.k, self.g, self.gl)
        self._want = {}

    def inputs(self, nc, first):
        """nc circuits whose witnesses alternate, starting with witness `first`"""
        idx = [(first + i) % 2 for i in range(nc)]
        return [self.wits[i] for i in idx], [self.fills[i] for i in idx]

    def want(self, nc, first, scheme):
        key = (nc, first, scheme)
        if key not in self._want:
            wits, fills = self.inputs(nc, first)
            self._want[key] = O.create_proof(self.circ, wits[0], self.g, self.gl, wits=wits, fills=fills,
                                             multiopen=scheme)
        return self._want[key]

    def prove(self, pk, nc, first, scheme):
        wits, fills = self.inputs(nc, first)
        return pk.create_proof_multi(wits, fills=fills, multiopen=scheme)

    def run_sequence(self, pk, check=True):
        for step, nc in enumerate(SEQUENCE):
            for scheme in SCHEMES:
                got = self.prove(pk, nc, step % 2, scheme)
                if check:
                    assert got == self.want(nc, step % 2, scheme), (step, nc, scheme)


@pytest.fixture(scope="module")
def env():
    h2g.init()
    e = _Env()
    yield e
    e.params.close()


def _free_bytes():
    return h2g.device_mem_info()[0]


def _footprint(env, pk, measured):
    """One key's footprint: free memory before the key minus after its first proof, as
    measured -- but the runtime hands memory out in blocks that it keeps when they are freed,
    so in a process that has freed device memory before, a small key comes out of kept blocks
    and the measured figure is 0, a bound nothing can meet.  Then (and whenever it is the
    larger) the key's own arrays stand in, counted from the shape: the three l cosets and,
    per fixed and per permutation column, values, polynomial and extended coset.  That is
    less than what a key holds (no workspace), so the bound is never wider than the
    measured one would be in a fresh process."""
    n, ext = 1 << env.circ.k, 1 << pk.extended_k
    arrays = 32 * (3 * ext + (env.circ.num_fixed + len(env.circ.perm_columns)) * (2 * n + ext))
    assert arrays > 0
    return max(measured, arrays)


def test_growth_and_shrink_on_one_key(env):
    """1, 3, 1, 2, 3 circuits on one key: every buffer that grows with the circuit count is
    replaced once and then reused by smaller proofs -- an address kept across the growth, or
    a size taken for the buffer's, would change the bytes.  Then check_witness, whose own
    buffers grow after the proofs' have."""
    pk = h2g.ProvingKey(env.params, env.circ)
    env.run_sequence(pk)
    wit, fill = env.wits[0], env.fills[0]
    _, chs = pk.create_proof_phased(fill, wit)
    full = fill.full(chs)
    assert pk.check_witness(full, challenges=chs, cap=8) == (0, [])
    bad = R.set_cell(full, 0, 3, 12345)
    got_small = pk.check_witness(bad, challenges=chs, cap=1)    # the record buffer grows ...
    got = pk.check_witness(bad, challenges=chs, cap=64)         # ... and grows again
    fresh = h2g.ProvingKey(env.params, env.circ)
    want = fresh.check_witness(bad, challenges=chs, cap=64)
    fresh.close()
    assert want[0] > 0
    assert got == want
    assert got_small == (want[0], want[1][:1])
    # and the key still proves
    assert env.prove(pk, 2, 0, "shplonk") == env.want(2, 0, "shplonk")
    pk.close()


def test_growth_keeps_nothing(env):
    """A key that went through 1, 3, 1, 2, 3 circuits holds what a key that only ever made the
    3-circuit proof holds: no superseded buffer stays resident.  The bound is the smallest
    of the 3-circuit proof's lookup batch buffers (ProofRun::lookup_permuted: G groups of
    u = n - (bf + 1) rows; the row indices, 4 bytes each) -- a key that kept the 1-circuit
    sizes would hold several such buffers more."""
    warm = h2g.ProvingKey(env.params, env.circ)  # device-wide scratch (NTT, MSM) to its final size
    env.run_sequence(warm)
    warm.close()

    start = _free_bytes()
    grown = h2g.ProvingKey(env.params, env.circ)
    env.run_sequence(grown)
    first = _free_bytes()
    env.run_sequence(grown)  # nothing needs to grow now
    second = _free_bytes()
    print(f"free bytes: start {start}, after the sequence {first}, after it again {second}")
    assert second >= first
    held_grown = start - second
    grown.close()

    start = _free_bytes()
    fresh = h2g.ProvingKey(env.params, env.circ)
    for scheme in SCHEMES:
        assert env.prove(fresh, 3, 0, scheme) == env.want(3, 0, scheme)
    held_fresh = start - _free_bytes()
    bf = fresh.bf
    fresh.close()

    n = 1 << env.circ.k
    u = n - (bf + 1)
    groups = 2 * 3 * len(env.circ.lookups)  # input and table of every (circuit, lookup)
    bound = groups * u * 4
    print(f"held: grown key {held_grown}, fresh key {held_fresh}, bound {bound}")
    assert held_grown - held_fresh < bound


def test_create_prove_free_cycles(env):
    """keygen, a 2-circuit proof, close, 200 times: a member the destructor forgot would
    leak once per cycle"""
    def cycle():
        pk = h2g.ProvingKey(env.params, env.circ)
        proof = env.prove(pk, 2, 0, "shplonk")
        pk.close()
        return proof

    before = _free_bytes()
    pk = h2g.ProvingKey(env.params, env.circ)
    assert env.prove(pk, 2, 0, "shplonk") == env.want(2, 0, "shplonk")
    footprint = _footprint(env, pk, before - _free_bytes())
    pk.close()
    for _ in range(9):
        cycle()
    at10 = _free_bytes()
    for _ in range(190):
        last = cycle()
    at200 = _free_bytes()
    print(f"footprint {footprint}, free after cycle 10 {at10}, after cycle 200 {at200}")
    assert last == env.want(2, 0, "shplonk")
    assert at10 - at200 < footprint


@pytest.mark.parametrize("fmt", ["RAW_BYTES", "PROCESSED"])
def test_failed_reads_give_memory_back(env, fmt):
    """ProvingKey::read of a key with one field element at or above the modulus fails after
    the key's arrays are on the device: all of them are released"""
    fmt = getattr(h2g, fmt)
    before = _free_bytes()
    pk = h2g.ProvingKey(env.params, env.circ)
    assert env.prove(pk, 2, 0, "shplonk") == env.want(2, 0, "shplonk")
    footprint = _footprint(env, pk, before - _free_bytes())
    data = bytearray(pk.write(fmt))
    pk.close()
    data[-32:] = b"\xff" * 32  # the last element of the last sigma coset
    data = bytes(data)
    with pytest.raises(h2g.H2GError, match="not below the modulus"):
        h2g.ProvingKey(env.params, env.circ, data=data, fmt=fmt)
    start = _free_bytes()
    for _ in range(50):
        with pytest.raises(h2g.H2GError):
            h2g.ProvingKey(env.params, env.circ, data=data, fmt=fmt)
    end = _free_bytes()
    print(f"footprint {footprint}, free before the failed reads {start}, after {end}")
    assert start - end < footprint


def test_second_free_raises(env):
    """freed once: the handle is gone (ProvingKey.close() forgets the handle, so the second
    free goes to the library with the handle itself, as test_gpu_descriptors.py does)"""
    pk = h2g.ProvingKey(env.params, env.circ)
    handle = pk.handle
    pk.close()
    with pytest.raises(h2g.H2GError, match="unknown proving key"):
        h2g.check(h2g.lib().h2g_pk_free(handle))
