"""Wall time of ProvingKey.check_witness (h2g_check_witness) on a valid witness, with
create_proof on the same key beside it as context: C3 at k = 22 and the keccak-style circuit
at k = 18 by default.  Warm-up first, the library synchronised before and after every timed
call, the median of the runs; one JSON line per circuit, and the box calibration line first.
usage: python tools/check_bench.py [--runs 7] [--warmup 2] [c3:22 keccak:18 ...]"""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "yet-another-halo2-fork_amd")]
import numpy as np  # noqa: E402

import h2g  # noqa: E402
import h2g_circuit as hc  # noqa: E402


def timed(fn, runs, warmup):
    """median / min wall ms of fn() over `runs` calls after `warmup`, synchronised around each"""
    L = h2g.lib()
    ms = []
    for it in range(warmup + runs):
        h2g.check(L.h2g_synchronize())
        t0 = time.perf_counter()
        fn()
        h2g.check(L.h2g_synchronize())
        if it >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 3), round(min(ms), 3)


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("cases", nargs="*", default=["c3:22", "keccak:18"], help="c3:K, keccak:K or c3xG:K (G gates)")
    a = ap.parse_args()
    runs, warmup = a.runs, a.warmup
    assert runs >= 5, "the median of at least 5 runs"
    cases = [c.split(":") for c in a.cases]
    h2g.init()
    print(json.dumps({"box_calibration": h2g.box_calibrate()}), flush=True)
    for kind, k in cases:
        k = int(k)
        circ, wit = hc.keccak_style(k) if kind == "keccak" else hc.synthetic_c3(k, h2g.DeviceOps)
        if kind.startswith("c3x"):  # C3 with its gate G times (scaled by constants): the gate kernel's A/B circuit
            gates = [hc.fixed(0) * (hc.const(j + 1) * (hc.advice(0) * hc.advice(1) - hc.advice(2)))
                     for j in range(int(kind[3:]))]
            circ = hc.Circuit(k, 3, 1, 0, gates, circ.perm_columns, circ.copies, circ.fixed_values,
                              name=f"synthetic-c3 k={k}, {len(gates)} gates")
        params = h2g.Params(k, s=np.asarray(hc.fr_to_limbs(0x1234567 + k), dtype=np.uint64))
        pk = h2g.ProvingKey(params, circ)
        d_adv = h2g.DevBuf.from_array(np.ascontiguousarray(wit.advice))
        total, _ = pk.check_witness(wit)
        assert total == 0, f"{circ.name}: the valid witness has {total} failures"
        out = {"circuit": circ.name, "k": k, "runs": runs, "copies": int(len(circ.copies)),
               "lookups": len(circ.lookups)}
        out["check_host_advice_ms"], out["check_host_advice_min_ms"] = timed(lambda: pk.check_witness(wit), runs, warmup)
        out["check_device_advice_ms"], out["check_device_advice_min_ms"] = timed(
            lambda: pk.check_witness(wit, advice_dev_ptr=d_adv.ptr), runs, warmup)
        out["check_device_advice_no_copies_ms"], _ = timed(
            lambda: pk.check_witness(wit, advice_dev_ptr=d_adv.ptr, copies=False), runs, warmup)
        out["create_proof_device_advice_ms"], out["create_proof_device_advice_min_ms"] = timed(
            lambda: pk.create_proof(wit, advice_dev_ptr=d_adv.ptr), runs, warmup)
        print(json.dumps(out), flush=True)
        d_adv.close()
        pk.close()
        params.close()
    h2g.shutdown()


if __name__ == "__main__":
    main()
