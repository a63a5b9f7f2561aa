"""h2g_create_proof_assigned: the proof made from a witness of Assigned cells (numerators plus
the Rational cells' denominators, evaluated on the device) is, byte for byte, the proof the
existing entries make from the evaluated witness -- which test_gpu_prover.py and
test_multi_circuit_oracle.py pin to the oracle.  The Assigned witnesses here are the circuits'
own witnesses with a random third of the usable cells rewritten as (value * d, d)."""
import numpy as np
import pytest

import _oracle as O
import h2g
import h2g_circuit as hc

pytestmark = pytest.mark.gpu

_PARAMS = {}


@pytest.fixture(scope="module", autouse=True)
def _init():
    h2g.init()
    yield
    for p in _PARAMS.values():
        p.close()
    _PARAMS.clear()


def _params(k):
    if k not in _PARAMS:
        _, g, gl = O.srs(k)
        _PARAMS[k] = h2g.Params(k, g, gl)
    return _PARAMS[k]


def _usable(circ):
    return circ.n - circ.blinding_factors() - 1


def assignify(fill, circ, seed, den_of=None, zero_cells=(), lists=None):
    """fill(phase, challenges) -> {column: values} as an Assigned source: a random third of the
    usable cells of every column it returns becomes (value * d, d), d random or den_of(challenges,
    column, rows) -> (len(rows), 4); zero_cells: (column, row, x) cells that become (x, 0).
    -> fill(phase, challenges) -> ({column: numerators}, index, den); every list handed out is
    also appended to `lists` as (phase, index)"""
    n, usable = circ.n, _usable(circ)

    def afill(phase, ch):
        rng = np.random.default_rng(seed * 100 + phase)
        cols, index, dens = {}, [], []
        for col, vals in sorted(fill(phase, ch).items()):
            vals = np.array(vals, dtype=np.uint64, copy=True)
            rows = np.flatnonzero(rng.integers(0, 3, size=min(len(vals), usable)) == 0)
            zeros = [(r, x) for c, r, x in zero_cells if c == col]
            rows = np.setdiff1d(rows, [r for r, _ in zeros])
            d = den_of(ch, col, rows) if den_of else O.random_fr(rng, len(rows) + 1)[: len(rows)]
            if len(rows):
                vals[rows] = O.binop("or_fr_mul", np.ascontiguousarray(vals[rows]), np.ascontiguousarray(d))
            for r, x in zeros:
                vals[r] = hc.fr_to_limbs(x)
                rows = np.append(rows, r)
                d = np.concatenate([d, np.zeros((1, 4), dtype=np.uint64)])
            order = np.argsort(rows, kind="stable")
            cols[col] = vals
            index.append(col * n + rows[order].astype(np.uint64))
            dens.append(d[order])
        index = np.concatenate(index).astype(np.uint64) if index else np.zeros(0, dtype=np.uint64)
        dens = np.concatenate(dens) if dens else np.zeros((0, 4), dtype=np.uint64)
        assert np.all(index[1:] > index[:-1])
        if lists is not None:
            lists.append((phase, index))
        return cols, index, dens

    return afill


def _whole(wit):
    """a complete single-phase witness as a fill"""
    return lambda phase, ch: {c: wit.advice[c] for c in range(wit.advice.shape[0])}


def test_simple_example_a_third_rational_and_a_zero_denominator():
    circ, wit = hc.simple_example(8)
    pk = h2g.ProvingKey(_params(8), circ)
    want = pk.create_proof(wit)
    assert want == pk.create_proof_multi([wit])
    # row 249 is usable and no gate or copy reads a1 there (the blocks end at row 247, s_mul is 0):
    # (x, 0) evaluates to the 0 the witness holds
    row = _usable(circ) - 1
    assert not wit.advice[1, row].any() and not circ.fixed_values[1][row].any()
    lists = []
    afill = assignify(_whole(wit), circ, seed=1, zero_cells=[(1, row, 123456789)], lists=lists)
    got = pk.create_proof_assigned([afill], [wit])
    assert got == want
    nden = len(lists[0][1])
    assert 2 * _usable(circ) // 3 - 60 < nden < 2 * _usable(circ) // 3 + 60  # a third of two columns
    assert 1 * circ.n + row in lists[0][1]
    # again on the grown scratch, and with the other seed and split
    assert pk.create_proof_assigned([afill], [wit]) == want
    assert (pk.create_proof_assigned([afill], [wit], seed=bytes(range(32)), vanishing_threads=3)
            == pk.create_proof(wit, seed=bytes(range(32)), vanishing_threads=3))
    pk.close()


def _challenge_dens(ch, col, rows):
    """denominators that depend on the challenges the callback was given"""
    base = (sum(ch) + 1) % hc.R_MOD
    return hc.ints_to_mont([(base * (col + 2) + int(r) + 1) % hc.R_MOD or 1 for r in rows])


@pytest.mark.parametrize("multiopen,transcript", [("shplonk", "blake2b"), ("gwc", "keccak256")])
def test_challenge_circuit_later_phases_from_the_challenges(multiopen, transcript):
    circ, wit, fill = hc.challenge_circuit(6, extended=True)
    pk = h2g.ProvingKey(_params(6), circ)
    want, chs = pk.create_proof_phased(fill, wit, multiopen=multiopen, transcript=transcript)
    assert chs[0] and chs[1]
    lists = []
    afill = assignify(fill, circ, seed=2, den_of=_challenge_dens, lists=lists)
    got = pk.create_proof_assigned([afill], [wit], multiopen=multiopen, transcript=transcript)
    assert got == want
    assert [p for p, _ in lists] == [0, 1, 2] and all(len(ix) for _, ix in lists)
    # phase 1's cells lie in its columns only (z and w), phase 2's in y
    n = circ.n
    assert set(np.unique(lists[1][1] // n)) <= {1, 2} and set(np.unique(lists[2][1] // n)) == {3}
    pk.close()


def test_entries_outside_the_phase_are_ignored():
    """a list that also names cells of other phases' columns (with denominators that would ruin
    them): the prover reads only the phase's columns, the proof is the same"""
    circ, wit, fill = hc.challenge_circuit(6, extended=True)
    pk = h2g.ProvingKey(_params(6), circ)
    want, _ = pk.create_proof_phased(fill, wit)
    inner = assignify(fill, circ, seed=3)

    def afill(phase, ch):
        cols, index, dens = inner(phase, ch)
        other = [c for c in range(circ.num_advice) if circ.advice_phase[c] != phase]
        extra = np.asarray([c * circ.n + r for c in other for r in (0, 5, 17)], dtype=np.uint64)
        index2 = np.concatenate([index, extra])
        dens2 = np.concatenate([dens, hc.ints_to_mont([7] * len(extra))])
        order = np.argsort(index2, kind="stable")
        return cols, index2[order], dens2[order]

    assert pk.create_proof_assigned([afill], [wit]) == want
    pk.close()


def test_two_circuits_with_different_lists_one_empty():
    circ, w0, f0 = hc.my_circuit(6, input_value=42)
    _, w1, f1 = hc.my_circuit(6, input_value=1000)
    pk = h2g.ProvingKey(_params(6), circ)
    want = pk.create_proof_multi([w0, w1], fills=[f0, f1])
    lists0 = []
    a0 = assignify(f0, circ, seed=4, lists=lists0)

    def a1(phase, ch):  # no divisions: count == 0 with NULL pointers
        return f1(phase, ch), None, None

    assert pk.create_proof_assigned([a0, a1], [w0, w1]) == want
    assert len(lists0) == 2 and all(len(ix) for _, ix in lists0)
    # the other way round, and both Rational with different lists
    want_r = pk.create_proof_multi([w1, w0], fills=[f1, f0])
    assert pk.create_proof_assigned([a1, a0], [w1, w0]) == want_r
    b1 = assignify(f1, circ, seed=5)
    assert pk.create_proof_assigned([a0, b1], [w0, w1]) == want
    pk.close()


def test_streamed_coset_key_gives_the_same_bytes():
    circ, w0, f0 = hc.my_circuit(6, input_value=42)
    resident = h2g.ProvingKey(_params(6), circ)
    want = resident.create_proof_multi([w0], fills=[f0])
    resident.close()
    pk = h2g.ProvingKey(_params(6), circ, cosets="streamed")
    assert pk.memory()["cosets"] == "streamed"
    assert pk.create_proof_assigned([assignify(f0, circ, seed=6)], [w0]) == want
    pk.close()


def test_bad_lists_fail_the_proof_and_the_key_proves_afterwards():
    circ, w0, f0 = hc.my_circuit(6, input_value=42)
    _, w1, f1 = hc.my_circuit(6, input_value=1000)
    pk = h2g.ProvingKey(_params(6), circ)
    good0, good1 = assignify(f0, circ, seed=7), assignify(f1, circ, seed=8)
    want = pk.create_proof_assigned([good0, good1], [w0, w1])
    assert want == pk.create_proof_multi([w0, w1], fills=[f0, f1])

    def broken(at_phase, how):
        def afill(phase, ch):
            cols, index, dens = good1(phase, ch)
            if phase == at_phase:
                index = index.copy()
                if how == "decreasing":
                    index[[3, 4]] = index[[4, 3]]
                elif how == "equal":
                    index[4] = index[3]
                else:
                    index[-1] = circ.num_advice * circ.n
            return cols, index, dens
        return afill

    for at_phase in (0, 1):
        for how, msg in (("decreasing", "strictly increasing"), ("equal", "strictly increasing"),
                         ("beyond", "num_advice")):
            with pytest.raises(h2g.H2GError, match=f"h2g error 1: .*{msg}.*circuit 1 phase {at_phase}"):
                pk.create_proof_assigned([good0, broken(at_phase, how)], [w0, w1])
            assert pk.create_proof_assigned([good0, good1], [w0, w1]) == want
    # the evaluated witness and a witness source are other entries' arguments
    inp = h2g.ProveInputs()
    inp.num_circuits = 1
    dummy = (h2g.VP * 1)()
    inp.advice = h2g.ctypes.cast(dummy, h2g.ctypes.POINTER(h2g.VP))
    src = h2g.AssignedSource(None, h2g.ASSIGNED_FILL(lambda *a: 1))
    ln = h2g.SZ()
    rc = h2g.lib().h2g_create_proof_assigned(pk.params.handle, pk.handle, h2g.ctypes.byref(inp), h2g.ctypes.byref(src),
                                             None, 0, h2g.ctypes.byref(ln))
    assert rc == 1 and b"must be NULL" in h2g.lib().h2g_last_error()
    pk.close()


def test_scratch_is_counted_and_given_back():
    """the key's scratch (num_advice x n numerators, the list) shows in h2g_pk_memory once an
    Assigned proof has run, is reused by the next, and goes with the key: 60 cycles of keygen,
    Assigned proof and close lose less than one key's arrays (the accounting of
    test_gpu_key_lifecycle.py: free device bytes, bounded by the key's own arrays counted from
    its shape)"""
    circ, w0, f0 = hc.my_circuit(6, input_value=42)
    params = _params(6)
    lists = []
    afill = assignify(f0, circ, seed=9, lists=lists)
    plain = h2g.ProvingKey(params, circ)
    want = plain.create_proof_multi([w0], fills=[f0])
    held_plain = plain.memory()["bytes"]
    plain.close()
    pk = h2g.ProvingKey(params, circ)
    assert pk.create_proof_assigned([afill], [w0]) == want
    held = pk.memory()["bytes"]
    longest = max(len(ix) for _, ix in lists)
    cells = circ.num_advice * circ.n * 32
    print(f"key bytes: witness source {held_plain}, Assigned source {held}, numerators {cells}, longest list {longest}")
    assert cells <= held - held_plain <= cells + longest * (8 + 32)
    assert pk.create_proof_assigned([afill], [w0]) == want
    assert pk.memory()["bytes"] == held  # nothing grows the second time
    ext = 1 << pk.extended_k
    footprint = 32 * (3 * ext + (circ.num_fixed + len(circ.perm_columns)) * (2 * circ.n + ext))
    handle = pk.handle
    pk.close()
    with pytest.raises(h2g.H2GError, match="unknown proving key"):
        h2g.check(h2g.lib().h2g_pk_memory(handle, (h2g.U64 * 4)()))

    def cycle():
        k = h2g.ProvingKey(params, circ)
        proof = k.create_proof_assigned([afill], [w0])
        k.close()
        return proof

    for _ in range(10):
        cycle()
    at10 = h2g.device_mem_info()[0]
    for _ in range(50):
        last = cycle()
    at60 = h2g.device_mem_info()[0]
    print(f"footprint {footprint}, free after cycle 10 {at10}, after cycle 60 {at60}")
    assert last == want
    assert at10 - at60 < footprint
