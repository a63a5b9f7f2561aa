"""batch_invert_assigned (halo2_frontend/src/circuit.rs:363-404) restated twice, for the tests of
h2g_assigned_to_fr and h2g_create_proof_assigned.

  convert      the oracle's batch_invert and binop("or_fr_mul") over the gathered denominators:
               fast, for the array checks
  convert_int  Python integers, num * pow(den, r - 2, r) % r with 0 for den == 0: for at most a
               few hundred cells, so that the pin does not rest on the oracle's inversion alone

Wire form (include/h2g.h): num (ncells, 4) numerators in Montgomery limbs, index the flat cell
indices of the Rational cells (strictly increasing), den (len(index), 4) their denominators.
Cells that are not listed keep their numerator."""
import numpy as np

import _oracle as O
import h2g_circuit as hc

R = hc.R_MOD
EDGE_DENS = (0, 1, R - 1, 2)
EDGE_NUMS = (0, R - 1)


def convert(num, index, den):
    num = np.ascontiguousarray(num, dtype=np.uint64).reshape(-1, 4)
    idx = np.asarray(index, dtype=np.int64).reshape(-1)
    out = num.copy()
    if len(idx) == 0:
        return out
    inv = O.batch_invert(np.ascontiguousarray(den, dtype=np.uint64).reshape(-1, 4))  # zeros stay zero
    out[idx] = O.binop("or_fr_mul", np.ascontiguousarray(num[idx]), inv)
    return out


def convert_int(num, index, den):
    """the same on canonical Python integers: lists in, list out"""
    out = [int(v) % R for v in num]
    for c, d in zip(index, den):
        d = int(d) % R
        out[int(c)] = out[int(c)] * pow(d, R - 2, R) % R if d else 0
    return out


def edge_case():
    """every edge denominator under every edge numerator and a random one, with unlisted cells
    between them: (num, index, den) as canonical integers"""
    rng = np.random.default_rng(77)
    nums = list(EDGE_NUMS) + [int.from_bytes(rng.bytes(32), "little") % R]
    num, index, den = [], [], []
    for d in EDGE_DENS:
        for x in nums:
            index.append(len(num))
            num.append(x)
            den.append(d)
            num.append((x + 5) % R)  # an unlisted neighbour
    return num, index, den


def random_case(rng, ncells, nden, ends=True):
    """random numerators, nden random Rational cells (cell 0 and the last cell among them when
    ends and nden allows) with random nonzero denominators -> (num, index uint64, den)"""
    num = O.random_fr(rng, ncells)
    if nden >= ncells:
        idx = np.arange(ncells, dtype=np.uint64)
    else:
        fixed = [0, ncells - 1][: min(nden, 2)] if ends else []
        rest = rng.choice(np.arange(1, ncells - 1), size=nden - len(fixed), replace=False) if nden > len(fixed) else []
        idx = np.sort(np.concatenate([np.asarray(fixed, dtype=np.int64), np.asarray(rest, dtype=np.int64)])).astype(np.uint64)
    den = O.random_fr(rng, max(len(idx), 1))[: len(idx)]
    return num, idx, den
