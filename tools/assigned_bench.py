"""Times the device evaluation of an Assigned witness (h2g_assigned_to_fr_dev, in place) against
the composition it replaces, and the prover entry built on it against the witness-source entry.

Conversion: the C3 shape at k = 22 (3 x 2^22 cells) and the keccak-style shape at k = 18 (32 x
2^18 cells), each with 1/16, 1/2 and all cells Rational (evenly spread).  `fused` is one
h2g_assigned_to_fr_dev call; `composed` is h2g_fr_batch_invert_dev over the contiguous
denominators followed by an h2g_fr_op_dev multiply over dense arrays of the same length -- the
composition WITHOUT the gather and scatter it would also need, so a lower bound of what it costs.
The two alternate, 2 warm-ups, then the median of 7 with min - max; host clock around a device
synchronise.

Proofs: create_proof_assigned against create_proof_phased fed the same witness already
evaluated, C3 k = 22 and keccak-style k = 18 with half the usable cells Rational, alternating,
2 warm-ups and the median of 7.  Both entries call back into Python for the witness and copy it
into the key's staging, so the difference is the upload to the scratch, the list's upload and
the conversion.  The CPU batch_invert_assigned this replaces is not measured here.
usage: python tools/assigned_bench.py [--out profiles/assigned/assigned_bench.json] [--small]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "yet-another-halo2-fork_amd")]

WARMUP, RUNS = 2, 7
FRACTIONS = ((1, 16), (1, 2), (1, 1))


def stats(v):
    return {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "assigned", "assigned_bench.json"))
    ap.add_argument("--small", action="store_true", help="k = 12 / 10 (a rehearsal of the tool, not a measurement)")
    a = ap.parse_args()
    import numpy as np

    import h2g
    import h2g_circuit as hc

    h2g.init()
    L = h2g.lib()

    def sync():
        h2g.check(L.h2g_synchronize())

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e3

    shapes = {"c3": (3, 12 if a.small else 22), "keccak": (32, 10 if a.small else 18)}
    out = {"tool": "tools/assigned_bench.py", "warmup": WARMUP, "runs": RUNS, "conversion": [], "proofs": []}
    rng = np.random.default_rng(7)
    for name, (cols, k) in shapes.items():
        ncells = cols << k
        cells = hc.random_mont(rng, ncells)
        d_num = h2g.DevBuf.from_array(cells)
        d_den = h2g.DevBuf.from_array(np.roll(cells, 12345, axis=0))
        d_dense = h2g.DevBuf(ncells * 32)
        for num_, den_ in FRACTIONS:
            idx = np.arange(0, ncells, den_ // num_, dtype=np.uint64)
            nden = len(idx)
            d_idx = h2g.DevBuf.from_array(idx)
            fused, composed = [], []
            for _ in range(WARMUP + RUNS):
                fused.append(timed(lambda: h2g.assigned_to_fr_dev(d_num.ptr, ncells, d_idx.ptr, d_den.ptr, nden,
                                                                  d_num.ptr)))

                def comp():
                    h2g.check(L.h2g_fr_batch_invert_dev(d_dense.ptr, nden, None))
                    h2g.check(L.h2g_fr_op_dev(h2g.OP_MUL, d_num.ptr, d_dense.ptr, None, d_num.ptr, nden, None))

                h2g.memcpy_dtod(d_dense.ptr, d_den.ptr, nden * 32)
                composed.append(timed(comp))
            row = {"shape": name, "k": k, "columns": cols, "cells": ncells, "rational": nden,
                   "per": h2g.debug_assigned_per(nden), "fused": stats(fused[WARMUP:]),
                   "composed_no_gather": stats(composed[WARMUP:])}
            print(json.dumps(row), flush=True)
            out["conversion"].append(row)
            d_idx.close()
        for b in (d_num, d_den, d_dense):
            b.close()

    for name, (cols, k) in shapes.items():
        circ, wit = hc.synthetic_c3(k, h2g.DeviceOps) if name == "c3" else hc.keccak_style(k)
        params = h2g.Params(k, s=np.asarray(hc.fr_to_limbs(0x1234567 + k), dtype=np.uint64))
        pk = h2g.ProvingKey(params, circ)
        n, u = circ.n, circ.usable_rows()
        rows = np.arange(0, u, 2)
        idx = np.concatenate([c * n + rows for c in range(circ.num_advice)]).astype(np.uint64)
        den = hc.random_mont(rng, len(idx))
        nums = np.ascontiguousarray(wit.advice).copy()
        flat = nums.reshape(-1, 4)
        flat[idx.astype(np.int64)] = h2g.fr_op(h2g.OP_MUL, np.ascontiguousarray(flat[idx.astype(np.int64)]), den)
        evaluated = {c: wit.advice[c] for c in range(circ.num_advice)}
        numer = {c: nums[c] for c in range(circ.num_advice)}
        t_asg, t_src, proofs = [], [], set()
        for _ in range(WARMUP + RUNS):
            t0 = time.perf_counter()
            p1 = pk.create_proof_assigned([lambda ph, ch: (numer, idx, den)], [wit])
            t1 = time.perf_counter()
            p2, _ = pk.create_proof_phased(lambda ph, ch: evaluated, wit)
            t2 = time.perf_counter()
            t_asg.append((t1 - t0) * 1e3)
            t_src.append((t2 - t1) * 1e3)
            proofs |= {p1, p2}
        row = {"circuit": circ.name, "k": k, "cells": circ.num_advice * n, "rational": len(idx),
               "same_proof_bytes": len(proofs) == 1, "create_proof_assigned": stats(t_asg[WARMUP:]),
               "create_proof_phased_evaluated": stats(t_src[WARMUP:])}
        print(json.dumps(row), flush=True)
        out["proofs"].append(row)
        pk.close()
        params.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    h2g.shutdown()


if __name__ == "__main__":
    main()
