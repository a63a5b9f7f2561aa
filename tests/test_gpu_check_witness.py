"""h2g_check_witness on the device (include/h2g.h; csrc/check.hip) against the plain-Python
restatement tests/_check_ref.py (pinned by tests/test_check_witness_cpu.py): the anchors,
random single-cell corruptions, non-interference with create_proof, device-resident advice,
a key read back from bytes, record-buffer overflow with every lane failing, the grid-stride
path at k = 20, and the argument errors."""
import numpy as np
import pytest

import _check_ref as R
import h2g
import h2g_circuit as hc

pytestmark = pytest.mark.gpu

_params = {}


@pytest.fixture(scope="module", autouse=True)
def _init():
    h2g.init()
    yield
    for p in _params.values():
        p.close()
    _params.clear()


def params(k):
    if k not in _params:
        _params[k] = h2g.Params(k, s=np.asarray(hc.fr_to_limbs(0x5eed + k), dtype=np.uint64))
    return _params[k]


def device_check(pk, wit, ch, want, **kw):
    total, recs = pk.check_witness(wit, challenges=ch, cap=max(64, len(want) + 8), **kw)
    assert total == len(want)
    assert recs == sorted(want)   # the records, in (kind, index, row) order


@pytest.mark.parametrize("case", R.valid_cases(), ids=lambda c: c[0])
def test_anchor_valid(case):
    _, circ, wit, ch = case
    pk = h2g.ProvingKey(params(circ.k), circ)
    device_check(pk, wit, ch, set())
    assert pk.check_witness(wit, challenges=ch, cap=0) == (0, [])   # count only
    pk.close()


@pytest.mark.parametrize("case", R.corrupted_cases(), ids=lambda c: c[0])
def test_anchor_corrupted(case):
    _, circ, wit, ch, want = case
    pk = h2g.ProvingKey(params(circ.k), circ)
    device_check(pk, wit, ch, want)
    device_check(pk, wit, ch, want, seed=bytes(range(32)))   # another theta, other blinding rows
    assert pk.check_witness(wit, challenges=ch, cap=0) == (len(want), [])
    device_check(pk, wit, ch, {f for f in want if f[0] != R.COPY}, copies=False)
    pk.close()


@pytest.mark.parametrize("case", R.valid_cases(), ids=lambda c: c[0])
def test_restatement_parity(case):
    """random single-cell corruptions of the usable rows: device set == restatement set"""
    name, circ, wit, ch = case
    rng = np.random.default_rng(sum(name.encode()))
    pk = h2g.ProvingKey(params(circ.k), circ)
    u = circ.usable_rows()
    seen = 0
    for t in range(4):
        col, row = int(rng.integers(circ.num_advice)), int(rng.integers(u))
        value = int(rng.integers(0, 16)) if t % 2 else int.from_bytes(rng.bytes(31), "little")
        bad = R.set_cell(wit, col, row, value)
        want = R.check(circ, bad, ch, seed=t)
        device_check(pk, bad, ch, want)
        seen += len(want)
    assert seen > 0, "no corruption was visible: the parity says nothing"
    pk.close()


def test_check_does_not_disturb_proofs():
    """proof, check, proof: equal bytes (the check shares the workspace, the challenge slots
    and the lookup / shuffle scratch with create_proof)"""
    circ, wit = hc.mixed_circuit(7)
    pk = h2g.ProvingKey(params(circ.k), circ)
    before = pk.create_proof(wit)
    bad = R.set_cell(wit, 3, 9, 5)
    assert pk.check_witness(bad)[0] > 0
    assert pk.create_proof(wit) == before
    pk.close()
    circ, wit, fill = hc.my_circuit(6)
    pk = h2g.ProvingKey(params(circ.k), circ)
    before, chs = pk.create_proof_phased(fill, wit)
    device_check(pk, fill.full(chs), chs, set())   # the witness the proof was made from
    assert pk.check_witness(fill.full(R.CH_MY), challenges=[5])[0] == 6
    after, chs2 = pk.create_proof_phased(fill, wit)
    assert after == before and chs2 == chs
    pk.close()


def test_device_resident_advice():
    _, circ, wit, ch, want = R.corrupted_cases()[1]
    pk = h2g.ProvingKey(params(circ.k), circ)
    d_adv = h2g.DevBuf.from_array(np.ascontiguousarray(wit.advice))
    device_check(pk, wit, ch, want, advice_dev_ptr=d_adv.ptr)
    device_check(pk, wit, ch, want)
    d_adv.close()
    pk.close()


def test_key_read_from_bytes():
    for _, circ, wit, ch, want in R.corrupted_cases()[1:4]:
        pk = h2g.ProvingKey(params(circ.k), circ)
        data = pk.write()
        pk.close()
        pk2 = h2g.ProvingKey(params(circ.k), circ, data=data)
        device_check(pk2, wit, ch, want)
        pk2.close()


def test_overflow_and_every_lane_failing():
    """column c zeroed on the usable rows: the gate and the copy chain fail almost everywhere"""
    circ, wit = hc.synthetic_c3(10, h2g.DeviceOps)
    adv = wit.advice.copy()
    adv[2, : circ.usable_rows()] = 0
    bad = hc.Witness(adv, wit.instance, wit.instance_lens)
    want = R.check(circ, bad)
    assert len(want) > 1500
    pk = h2g.ProvingKey(params(circ.k), circ)
    total, recs = pk.check_witness(bad, cap=16)
    assert total == len(want)
    assert len(recs) == 16 and recs == sorted(recs) and len(set(recs)) == 16
    assert set(recs) <= want
    assert pk.check_witness(bad, cap=0) == (len(want), [])
    device_check(pk, bad, [], want)   # and with room for all of them
    pk.close()


def test_grid_stride_and_large_rows():
    """k = 20: the middle row is past one pass of a grid capped at 256 * 32 blocks of 64 rows.
    The expected set is structural (no restatement at this size): copy i ties c[i] to
    a[i + 1], and the list ends at u - 2."""
    k = 20
    circ, wit = hc.synthetic_c3(k, h2g.DeviceOps)
    u = circ.usable_rows()
    mid = 2**19 + 3
    adv = wit.advice.copy()
    for row in (0, mid, u - 1):
        adv[2, row] = hc.fr_to_limbs(12345)
    bad = hc.Witness(adv, wit.instance, wit.instance_lens)
    pk = h2g.ProvingKey(params(k), circ)
    device_check(pk, wit, [], set())
    device_check(pk, bad, [], {(1, 0, 0), (5, 0, 0), (1, 0, mid), (5, mid, mid), (1, 0, u - 1)})
    pk.close()


def test_argument_errors():
    circ, wit, fill = hc.my_circuit(6)
    pk = h2g.ProvingKey(params(circ.k), circ)
    full = fill.full(R.CH_MY)
    with pytest.raises(h2g.H2GError, match="h2g error 1"):
        pk.check_witness(full)   # the key has a challenge
    copies = circ.copies.copy()
    copies[1, 2] = circ.n   # a row >= n
    with pytest.raises(h2g.H2GError, match="h2g error 1"):
        pk.check_witness(full, challenges=R.CH_MY, copies=copies)
    copies = circ.copies.copy()
    copies[0, 4] = circ.num_advice   # a column out of range
    with pytest.raises(h2g.H2GError, match="h2g error 1"):
        pk.check_witness(full, challenges=R.CH_MY, copies=copies)
    d_adv = h2g.DevBuf(full.advice.nbytes + 16)
    with pytest.raises(h2g.H2GError, match="h2g error 1"):
        pk.check_witness(full, challenges=R.CH_MY, advice_dev_ptr=d_adv.ptr + 8)
    d_adv.close()
    with pytest.raises(h2g.H2GError, match="h2g error 5"):
        h2g.check(h2g.lib().h2g_check_witness(0xDEAD, None, None, 0, None))
    device_check(pk, full, R.CH_MY, set())   # the key is as it was
    pk.close()
