"""What the prover's self-checks cost (ProvingKey.set_self_check), beside the two things they
replace: create_proof on a valid witness in modes off / verdict / arguments, mode verdict on a
witness with one wrong gate cell (the cost of refusing), mode off followed by
VerifyingKey.verify, and check_witness followed by mode off.  C3 at k = 22 and the keccak-style
circuit at k = 18 by default, the advice resident on the device.  The arms alternate in one
process: one call of each per round, warm-up rounds first, the library synchronised before and
after every timed call, the median of the rounds; one JSON line per circuit, the box
calibration line first.
usage: python tools/selfcheck_bench.py [--runs 7] [--warmup 2] [c3:22 keccak:18 ...]"""
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


def alternate(arms, runs, warmup):
    """{name: (median, min) wall ms}: `warmup + runs` rounds, every arm once a round"""
    L = h2g.lib()
    ms = {name: [] for name in arms}
    for it in range(warmup + runs):
        for name, fn in arms.items():
            h2g.check(L.h2g_synchronize())
            t0 = time.perf_counter()
            fn()
            h2g.check(L.h2g_synchronize())
            if it >= warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: (round(statistics.median(v), 3), round(min(v), 3)) for name, v in ms.items()}


def wrong_gate_cell(kind, circ, wit):
    """the witness with one gate broken at a usable row and every lookup input still in its table
    (a missing lookup input is H2G_ERR_ARG in any mode, not a refusal).  C3: c off by one, which
    breaks a b - c (and the copy of c).  keccak-style: x_1 ^= 1 with y_0 and y_1, the two xors it
    enters, following it -- the lookups hold, the chain gate x_0[next] - y_0 does not."""
    adv = wit.advice.copy()
    row = circ.usable_rows() // 2
    row += row % 5 == 0   # (keccak-style: not one of its copy rows, every 5th)

    def bump(col, f):
        adv[col, row] = hc.fr_to_limbs(f(hc.fr_from_limbs(adv[col, row])) % hc.R_MOD)

    if kind == "keccak":
        W = circ.num_advice // 2
        for col in (1, W, W + 1):
            bump(col, lambda v: v ^ 1)
    else:
        bump(circ.num_advice - 1, lambda v: v + 1)
    return hc.Witness(adv, wit.instance, wit.instance_lens)


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("cases", nargs="*", default=["c3:22", "keccak:18"], help="c3:K or keccak:K")
    a = ap.parse_args()
    assert a.runs >= 5, "the median of at least 5 runs"
    h2g.init()
    print(json.dumps({"box_calibration": h2g.box_calibrate()}), flush=True)
    for kind, k in (c.split(":") for c in a.cases):
        k = int(k)
        circ, wit = hc.keccak_style(k) if kind == "keccak" else hc.synthetic_c3(k, h2g.DeviceOps)
        params = h2g.Params(k, s=np.asarray(hc.fr_to_limbs(0x1234567 + k), dtype=np.uint64))
        pk = h2g.ProvingKey(params, circ)
        vk = h2g.VerifyingKey.from_pk(pk)
        inst = [h2g.instance_columns(wit, circ)]
        d_adv = h2g.DevBuf.from_array(np.ascontiguousarray(wit.advice))
        bad = wrong_gate_cell(kind, circ, wit)
        d_bad = h2g.DevBuf.from_array(np.ascontiguousarray(bad.advice))

        def prove(mode, d=d_adv, w=wit):
            pk.set_self_check(mode)
            try:
                return pk.create_proof(w, advice_dev_ptr=d.ptr)
            finally:
                pk.set_self_check("off")

        def refuse():
            try:
                prove("verdict", d_bad, bad)
            except h2g.UnsatisfiedError as e:
                return e
            raise AssertionError("the wrong witness was not refused")

        base = prove("off")
        assert prove("verdict") == base and prove("arguments") == base, "a valid witness: mode off's bytes"
        assert vk.verify(base, inst) == h2g.VERIFY_OK
        assert vk.verify(prove("off", d_bad, bad), inst) == h2g.VERIFY_REJECTED
        err = refuse()
        assert pk.check_witness(wit, advice_dev_ptr=d_adv.ptr)[0] == 0

        def off_then_verify():
            assert vk.verify(prove("off"), inst) == h2g.VERIFY_OK

        def check_then_off():
            assert pk.check_witness(wit, advice_dev_ptr=d_adv.ptr)[0] == 0
            prove("off")

        res = alternate({"mode_off": lambda: prove("off"), "mode_verdict": lambda: prove("verdict"),
                         "mode_arguments": lambda: prove("arguments"), "mode_verdict_refusing": refuse,
                         "mode_off_then_verify": off_then_verify, "check_witness_then_mode_off": check_then_off},
                        a.runs, a.warmup)
        out = {"circuit": circ.name, "k": k, "runs": a.runs, "warmup": a.warmup, "lookups": len(circ.lookups),
               "refusal_records": err.total, "refusal_first": err.failures[:2]}
        for name, (med, mn) in res.items():
            out[name + "_ms"], out[name + "_min_ms"] = med, mn
        print(json.dumps(out), flush=True)
        d_adv.close()
        d_bad.close()
        vk.close()
        pk.close()
        params.close()
    h2g.shutdown()


if __name__ == "__main__":
    main()
