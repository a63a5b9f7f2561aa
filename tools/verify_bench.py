"""Wall time of VerifyingKey.verify / verify_batch (h2g_verify_proof / h2g_verify_batch): the
keccak-style circuit at the smallest k it supports (9) and C3 at k = 12 by default, a batch of
B distinct proofs all valid and with one invalid proof, B = 1 and --batch.  Per proof: the
host, decompression, MSM and pairing shares (h2g_verify_stages of the median run).  The
oracle's Python verify of one proof stands beside them as context only.  Warm-up first, the
median of the runs with min and max; one JSON line per circuit, the box calibration first.
usage: python tools/verify_bench.py [--batch 256] [--runs 7] [--warmup 2] [keccak:9 c3:12 ...]"""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "yet-another-halo2-fork_amd"), os.path.join(REPO, "oracle", "py")]
import numpy as np  # noqa: E402

import h2g  # noqa: E402
import h2g_circuit as hc  # noqa: E402

S_INT = 0x1234567


def timed(fn, runs, warmup):
    """(median, min, max) wall ms of fn() over `runs` calls after `warmup`, and the stage times
    of the median run; verify calls return with the device idle"""
    rows = []
    for it in range(warmup + runs):
        t0 = time.perf_counter()
        fn()
        ms = (time.perf_counter() - t0) * 1e3
        if it >= warmup:
            rows.append((ms, h2g.verify_stages()))
    rows.sort(key=lambda r: r[0])
    med = rows[len(rows) // 2]
    return {"ms": round(statistics.median(r[0] for r in rows), 3), "min_ms": round(rows[0][0], 3),
            "max_ms": round(rows[-1][0], 3),
            "stages_ms": dict(zip(("host", "decompress", "msm", "pairing"), (round(v, 3) for v in med[1])))}


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("cases", nargs="*", default=["keccak:9", "c3:12"], help="keccak:K or c3:K")
    a = ap.parse_args()
    assert a.runs >= 7, "the median of at least 7 runs"
    h2g.init()
    print(json.dumps({"box_calibration": h2g.box_calibrate()}), flush=True)
    for kind, k in (c.split(":") for c in a.cases):
        k = int(k)
        circ, wit = hc.keccak_style(k) if kind == "keccak" else hc.synthetic_c3(k, h2g.DeviceOps)
        params = h2g.Params(k, s=np.asarray(hc.fr_to_limbs(S_INT), dtype=np.uint64))
        pk = h2g.ProvingKey(params, circ)
        vk = h2g.VerifyingKey.from_pk(pk)
        B = a.batch
        proofs = [pk.create_proof(wit, seed=i.to_bytes(32, "little")) for i in range(1, B + 1)]
        cols = [h2g.instance_columns(wit, circ)]
        insts = [cols] * B
        bad = list(proofs)
        t = bytearray(bad[B // 3])
        t[-70] ^= 1                                     # inside h1 / the last evaluations: well formed or not, not valid
        bad[B // 3] = bytes(t)
        assert vk.verify(proofs[0], cols) == h2g.VERIFY_OK
        v_ok, st_ok = vk.verify_batch(proofs, insts)
        v_bad, st_bad = vk.verify_batch(bad, insts)
        assert v_ok == [h2g.VERIFY_OK] * B and st_ok[0] == 1
        assert [i for i, v in enumerate(v_bad) if v != h2g.VERIFY_OK] == [B // 3]
        out = {"circuit": circ.name, "k": k, "batch": B, "runs": a.runs, "proof_bytes": len(proofs[0]),
               "points_per_proof": st_ok[2] // B, "msm_terms_per_proof": st_ok[1] // B,
               "invalid_verdict": v_bad[B // 3], "invalid_pairing_checks": st_bad[0]}
        out["verify_one"] = timed(lambda: vk.verify(proofs[0], cols), a.runs, a.warmup)
        out["batch_all_valid"] = timed(lambda: vk.verify_batch(proofs, insts), a.runs, a.warmup)
        out["batch_one_invalid"] = timed(lambda: vk.verify_batch(bad, insts), a.runs, a.warmup)
        out["per_proof_ms_all_valid"] = round(out["batch_all_valid"]["ms"] / B, 4)
        out["one_invalid_costs_ms"] = round(out["batch_one_invalid"]["ms"] - out["batch_all_valid"]["ms"], 3)
        if not a.no_oracle and k <= 12:
            import verifier as V
            f, p = pk.vk_commitments()
            vkc = ([V.affine_from_limbs(c) for c in f], [V.affine_from_limbs(c) for c in p])
            g2, s_g2 = params.g2()
            t0 = time.perf_counter()
            ok = V.verify(circ, None, proofs[0], None, vk=vkc, instances_multi=[[hc.mont_to_ints(c) for c in cols[0]]],
                          g2=(V.g2_from_limbs(g2), V.g2_from_limbs(s_g2)))
            out["oracle_python_verify_one_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            assert ok
        print(json.dumps(out), flush=True)
        vk.close()
        pk.close()
        params.close()
    h2g.shutdown()


if __name__ == "__main__":
    main()
