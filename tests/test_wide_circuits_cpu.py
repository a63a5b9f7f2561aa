"""The wide circuits of tests/_wide_circuit.py, pinned on the CPU: for every shape that
tests/test_gpu_wide_circuits.py proves on the device the oracle returns a proof,
oracle/py/verifier.py accepts it, the plain-Python MockProver restatement finds no failure, and
the circuit has the counts its case claims -- advice columns per phase, lookups, shuffles,
permutation columns, sets and degree -- so a changed helper cannot quietly move a case off its
capacity edge.  The shapes come from h2g.debug_limits(), host only."""
import numpy as np
import pytest

import _check_ref as CR
import _oracle as O
import _wide_circuit as W
import h2g
import verifier as V

LIM = h2g.debug_limits()
SHAPES = W.shapes(LIM)


def test_limits_seam_declared_bound_and_exported():
    for name in ("h2g_debug_limits", "h2g_debug_commit_batch_chunk", "h2g_debug_msm_batches_dev"):
        assert name in h2g.header_symbols() and name in h2g._SIGS and hasattr(h2g.lib(), name)
    assert list(LIM) == list(h2g.LIMITS) and len(LIM) == 10
    # the values the shapes' names were written for; a changed capacity moves the shapes with it
    assert LIM == dict(copy_cols=16, prefix_diff=16, compress_batch=32, lookup_keys_batch=32, perm_cols=8,
                       lin_terms=12, ntt_batch=8, poly_inv_batch=16, msm_batch=64, msm_ring=64)


def test_the_shapes_sit_on_the_capacities():
    names = set(SHAPES)
    c, r, b, p = LIM["copy_cols"], LIM["msm_ring"], LIM["compress_batch"], LIM["perm_cols"]
    want = {f"advice-{a}" for a in (c - 1, c, c + 1, 2 * c, 2 * c + 1, r - 1, r, r + 1, 2 * r + 1)}
    want |= {f"lookups-{n}" for n in (b // 2, b // 2 + 1, b, b + 1)} | {f"lookups-{b + 1}-shared"}
    want |= {f"perm-d3-{r - 1}", f"perm-d3-{r}", f"perm-d{p + 3}-{p}", f"perm-d{p + 3}-{p + 1}",
             f"perm-d{p + 3}-{p + 2}", f"perm-d{2 * p + 3}-{2 * p + 1}"}
    want |= {f"products-{LIM['poly_inv_batch']}", f"products-{LIM['poly_inv_batch'] + 1}"}
    want |= {f"phases-{(r + c) // 2}-{(r + c) // 2}", f"advice-{c + 1}-lookups-{c + 1}"}
    assert names == want


@pytest.mark.parametrize("name", list(SHAPES))
def test_shape_is_valid_and_as_claimed(name):
    kw, claim = SHAPES[name]
    circ, wit = W.wide_circuit(**kw)
    per_phase, nl, ns, p, nsets, d = W.counts(circ)
    assert dict(phase=per_phase, NL=nl, NS=ns, P=p, nsets=nsets, d=d) == claim
    assert circ.k == W.K and circ.num_advice == sum(per_phase)
    # every advice column is queried (so every one is opened), each at one rotation
    adv_q, _, _ = circ.queries()
    assert sorted(adv_q) == [(c, 0) for c in range(circ.num_advice)]
    tables = {tuple((e.op, e.a, e.b, e.c) for e in t) for _, t in circ.lookups}   # bare fixed queries
    if kw.get("shared_table"):
        assert len(tables) == 1
    else:
        assert len(tables) == nl
        tabs = [circ.fixed_values[1 + l].tobytes() for l in range(nl)]
        assert len(set(tabs)) == nl
    s, g, gl = O.srs(circ.k)
    proof = O.create_proof(circ, wit, g, gl)
    assert V.verify(circ, [], proof, s)
    assert CR.check(circ, wit) == set()
    again = W.wide_circuit(**kw)
    assert np.array_equal(again[1].advice, wit.advice) and np.array_equal(again[0].nodes, circ.nodes)
    other = W.wide_circuit(**kw, seed=1)   # the second circuit of a two-circuit proof
    assert np.array_equal(other[0].transcript_repr(), circ.transcript_repr())
    assert not np.array_equal(other[1].advice, wit.advice) and CR.check(circ, other[1]) == set()


def test_two_circuits_and_the_other_modes_verify():
    """the proofs the device file compares its bytes with, in the modes it uses them"""
    a = 2 * LIM["copy_cols"] + 1
    circ, w0 = W.wide_circuit(**SHAPES[f"advice-{a}"][0])
    _, w1 = W.wide_circuit(**SHAPES[f"advice-{a}"][0], seed=1)
    s, g, gl = O.srs(circ.k)
    proof = O.create_proof(circ, w0, g, gl, wits=[w0, w1])
    assert V.verify(circ, None, proof, s, instances_multi=[[], []])
    assert V.verify(circ, [], O.create_proof(circ, w0, g, gl, transcript="keccak256"), s, transcript="keccak256")
    for name in (f"advice-{LIM['msm_ring'] + 1}", f"lookups-{LIM['compress_batch'] // 2 + 1}"):
        circ, wit = W.wide_circuit(**SHAPES[name][0])
        assert V.verify(circ, [], O.create_proof(circ, wit, g, gl, multiopen="gwc"), s, multiopen="gwc")


def test_a_changed_cell_of_the_last_column_fails_its_gate_at_its_row():
    a = LIM["copy_cols"] + 1
    circ, wit = W.wide_circuit(**SHAPES[f"advice-{a}"][0])
    row = 77
    bad = CR.set_cell(wit, a - 1, row, 5)
    assert CR.check(circ, bad) == {(CR.GATE, 1, row)}
