"""The device prover and witness check on circuits whose widths cross the prover's per-launch
capacities (tests/_wide_circuit.py; pinned valid on the CPU by tests/test_wide_circuits_cpu.py):
the host loops that split a stage's columns into launches of COPY_COLS_MAX, PREFIX_DIFF_MAX,
COMPRESS_BATCH_MAX, LOOKUP_KEYS_BATCH_MAX, PERM_MAXC, LIN_MAXT, NTT_MAX_BATCH,
POLY_INV_MAX_BATCH and MSM_MAX_BATCH columns, and the asynchronous MSMs' result ring, which a
stage with more than MSM_RING commitments outgrows.  The shapes are derived from
h2g.debug_limits(): one below, at, one above and past twice each capacity.

Every case: the device's proof bytes equal the oracle's, the native verifier accepts them, and
h2g_check_witness finds nothing.  All at k = 7."""
import numpy as np
import pytest

import _check_ref as CR
import _oracle as O
import _wide_circuit as W
import h2g
import h2g_circuit as hc

pytestmark = pytest.mark.gpu

LIM = h2g.debug_limits()
SHAPES = W.shapes(LIM)
COPY, RING, COMP = LIM["copy_cols"], LIM["msm_ring"], LIM["compress_batch"]
_STATE = {}


@pytest.fixture(scope="module", autouse=True)
def _init():
    h2g.init()
    yield
    if "params" in _STATE:
        _STATE["params"][3].close()
    _STATE.clear()


def _params():
    """the oracle's SRS from its secret, so the params also carry the verifier's points"""
    if "params" not in _STATE:
        s, g, gl = O.srs(W.K)
        _STATE["params"] = (s, g, gl, h2g.Params(W.K, s=np.asarray(hc.fr_to_limbs(s), dtype=np.uint64)))
    return _STATE["params"]


def check_shape(name, from_device=False, multiopen="shplonk", transcript="blake2b", cosets="resident"):
    """-> (circuit, witness, key, oracle proof); the caller closes the key"""
    circ, wit = W.wide_circuit(**SHAPES[name][0])
    _, g, gl, params = _params()
    pk = h2g.ProvingKey(params, circ, cosets=cosets)
    assert (pk.degree, pk.nsets) == (SHAPES[name][1]["d"], SHAPES[name][1]["nsets"])
    want = O.create_proof(circ, wit, g, gl, multiopen=multiopen, transcript=transcript)
    d_adv = h2g.DevBuf.from_array(wit.advice) if from_device else None
    try:
        got = pk.create_proof(wit, advice_dev_ptr=d_adv.ptr if d_adv else None, multiopen=multiopen,
                              transcript=transcript)
        assert got == want, name
        vk = h2g.VerifyingKey.from_pk(pk)
        assert vk.verify(got, [h2g.instance_columns(wit, circ)], multiopen=multiopen,
                         transcript=transcript) == h2g.VERIFY_OK
        vk.close()
        assert pk.check_witness(wit, advice_dev_ptr=d_adv.ptr if d_adv else None) == (0, [])
        # and again: the result ring and every workspace are as a first proof found them
        assert pk.create_proof(wit, advice_dev_ptr=d_adv.ptr if d_adv else None, multiopen=multiopen,
                               transcript=transcript) == want, name
    finally:
        if d_adv:
            d_adv.close()
    return circ, wit, pk, want


ADVICE = [COPY - 1, COPY, COPY + 1, 2 * COPY, 2 * COPY + 1]


@pytest.mark.parametrize("from_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("a", ADVICE)
def test_advice_columns_per_copy_launch(a, from_device):
    """15, 16, 17, 32, 33 advice columns from host memory and from a device pointer (copy_columns
    in launches of 16; check_witness sums its columns the same way)"""
    check_shape(f"advice-{a}", from_device)[2].close()


def test_check_witness_finds_a_cell_of_the_seventeenth_column():
    """the column that falls into the second copy launch: its one changed cell is reported, as
    the gate and the row the plain-Python restatement names, from host and device memory"""
    a = COPY + 1
    circ, wit, pk, _ = check_shape(f"advice-{a}")
    row = 77
    bad = CR.set_cell(wit, a - 1, row, 5)
    want = CR.check(circ, bad)
    assert want == {(CR.GATE, 1, row)}
    assert pk.check_witness(bad) == (1, sorted(want))
    d_adv = h2g.DevBuf.from_array(bad.advice)
    assert pk.check_witness(bad, advice_dev_ptr=d_adv.ptr) == (1, sorted(want))
    d_adv.close()
    assert pk.check_witness(wit) == (0, [])
    pk.close()


@pytest.mark.parametrize("a", [RING - 1, RING, RING + 1, 2 * RING + 1])
def test_one_phase_of_more_commitments_than_result_slots(a):
    """63 advice commitments leave a slot for the early vanishing commitment, 64 fill the ring
    without it, 65 and 129 outgrow it (and take two and three batched MSMs)"""
    check_shape(f"advice-{a}")[2].close()


def test_two_circuits_whose_advice_together_outgrows_the_ring():
    name = f"advice-{2 * COPY + 1}"
    circ, w0 = W.wide_circuit(**SHAPES[name][0])
    _, w1 = W.wide_circuit(**SHAPES[name][0], seed=1)
    assert 2 * circ.num_advice > RING >= circ.num_advice
    _, g, gl, params = _params()
    pk = h2g.ProvingKey(params, circ)
    want = O.create_proof(circ, w0, g, gl, wits=[w0, w1])
    for _ in range(2):
        assert pk.create_proof_multi([w0, w1]) == want
    vk = h2g.VerifyingKey.from_pk(pk)
    inst = [h2g.instance_columns(w0, circ), h2g.instance_columns(w1, circ)]
    assert vk.verify(want, inst) == h2g.VERIFY_OK
    vk.close()
    assert pk.create_proof(w1) == O.create_proof(circ, w1, g, gl)
    pk.close()


def test_two_phases_each_within_the_ring():
    """40 + 40 columns: the stage is what counts, not the proof"""
    h = (RING + COPY) // 2
    circ, _, pk, _ = check_shape(f"phases-{h}-{h}")
    assert circ.max_phase == 1 and circ.num_advice > RING
    pk.close()


@pytest.mark.parametrize("nl", [COMP // 2, COMP // 2 + 1, COMP, COMP + 1])
def test_lookups_with_distinct_tables(nl):
    """16, 17, 32, 33 lookups: 32, 34, 64, 66 compress and key items (batches of 32) and as many
    permuted columns committed in one stage (prefix differences in launches of 16; the last
    two fill and outgrow the ring)"""
    check_shape(f"lookups-{nl}")[2].close()


def test_lookups_sharing_one_table():
    """33 inputs and one table: 34 key items on the shared path"""
    check_shape(f"lookups-{COMP + 1}-shared")[2].close()


@pytest.mark.parametrize("name", [n for n in SHAPES if n.startswith("perm-")])
def test_permutation_sets_and_columns_per_launch(name):
    """degree 3: 63 and 64 sets of one column (the grand products' commitments against the
    ring); degree 11: 8, 9 columns in one set and 10 in 9 + 1; degree 19: one set of 17 (launches
    of 8 + 8 + 1)"""
    check_shape(name)[2].close()


@pytest.mark.parametrize("total", [LIM["poly_inv_batch"], LIM["poly_inv_batch"] + 1])
def test_grand_products_per_batched_inversion(total):
    """one permutation set, 14 or 15 lookups and a shuffle: 16 and 17 grand products"""
    check_shape(f"products-{total}")[2].close()


def test_gwc_at_the_widths_that_split():
    for name in (f"advice-{RING + 1}", f"lookups-{COMP // 2 + 1}"):
        check_shape(name, multiopen="gwc")[2].close()


def test_keccak_transcript_at_33_columns():
    check_shape(f"advice-{2 * COPY + 1}", transcript="keccak256")[2].close()


def test_streamed_key_at_17_columns_and_17_lookups():
    """a streamed-coset key transforms its columns sub-coset by sub-coset: the same launches
    split the same way, and the same bytes as the resident key's"""
    name = f"advice-{COPY + 1}-lookups-{COPY + 1}"
    _, wit, pk, want = check_shape(name)
    _, _, sk, want_s = check_shape(name, cosets="streamed")
    assert want_s == want and sk.memory()["cosets"] == "streamed"
    assert sk.create_proof(wit) == pk.create_proof(wit) == want
    assert sk.write() == pk.write()
    sk.close()
    pk.close()
