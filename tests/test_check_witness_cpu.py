"""Pins tests/_check_ref.py -- the plain-Python restatement of h2g_check_witness's semantics
(MockProver::verify for a complete witness, halo2_frontend/src/dev.rs:742-1166, with the
blinding rows filled as the prover fills them) -- to known witnesses and their failure sets,
without the code under test: the GPU tests compare the device against this restatement."""
import pytest

import _check_ref as R


@pytest.mark.parametrize("case", R.valid_cases(), ids=lambda c: c[0])
def test_valid_witness_has_no_failures(case):
    _, circ, wit, ch = case
    assert R.check(circ, wit, ch) == set()


@pytest.mark.parametrize("case", R.corrupted_cases(), ids=lambda c: c[0])
def test_corrupted_witness_failure_set(case):
    _, circ, wit, ch, want = case
    assert R.check(circ, wit, ch) == want


def test_blinding_rows_do_not_depend_on_the_fill():
    """the selector live at row 57 reads the blinded a0[58], at row 60 it sits in a blinding
    row: the same two failures whatever values the blinding rows draw"""
    _, circ, wit, ch, want = R.corrupted_cases()[-1]
    assert R.check(circ, wit, ch, seed=1) == R.check(circ, wit, ch, seed=2) == want


def test_copies_can_be_skipped():
    _, circ, wit, ch, want = R.corrupted_cases()[1]
    assert R.check(circ, wit, ch, copies=False) == {f for f in want if f[0] != R.COPY}
