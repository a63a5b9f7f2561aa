"""What a failing batch costs h2g_verify_batch under both isolation modes, and the device
pairing check alone.

B distinct proofs of the keccak-style circuit at k = 9 with f of them invalid at random
positions, f in {0, 1, 4, 16, 64}: wall time of verify_batch in mode 0 (bisection: a
combination launch and a host pairing per step) and mode 1 (the combined check, then one device
launch of per-proof checks), the two modes alternating in one process, the median of --runs
after --warmup each.  Then h2g_pairing_check_batch (validation, copies, launch) and its _dev
form (the launch and a synchronisation) alone for 1, 64, 256 and 1024 checks.  One JSON object,
printed and written to --out.
usage: python tools/pairing_bench.py [--batch 256] [--runs 7] [--warmup 2] [--out FILE]"""
import json
import os
import random
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "yet-another-halo2-fork_amd"), os.path.join(REPO, "oracle", "py")]
import numpy as np  # noqa: E402

import bn254_ref as B  # noqa: E402
import h2g  # noqa: E402
import h2g_circuit as hc  # noqa: E402

S_INT = 0x1234567
BAD_COUNTS = (0, 1, 4, 16, 64)
CHECK_COUNTS = (1, 64, 256, 1024)


def summary(ms):
    ms = sorted(ms)
    return {"ms": round(statistics.median(ms), 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3)}


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pairing", "pairing_bench.json"))
    a = ap.parse_args()
    h2g.init()
    out = {"box_calibration": h2g.box_calibrate(), "batch": a.batch, "runs": a.runs, "warmup": a.warmup}
    k = 9
    circ, wit = hc.keccak_style(k)
    params = h2g.Params(k, s=np.asarray(hc.fr_to_limbs(S_INT), dtype=np.uint64))
    vp = params.verifier()
    pk = h2g.ProvingKey(params, circ)
    vk = h2g.VerifyingKey.from_pk(pk)
    nb = a.batch
    proofs = [pk.create_proof(wit, seed=i.to_bytes(32, "little")) for i in range(1, nb + 1)]
    insts = [[h2g.instance_columns(wit, circ)]] * nb
    out["circuit"], out["k"] = circ.name, k
    rng = random.Random(2024)
    rows = []
    try:
        for f in [f for f in BAD_COUNTS if f <= nb]:
            bad_at = sorted(rng.sample(range(nb), f))
            ps = list(proofs)
            for i in bad_at:
                t = bytearray(ps[i])
                t[-70] ^= 1                    # inside the last evaluations: not valid
                ps[i] = bytes(t)
            ms, checks, stages, verdicts = {0: [], 1: []}, {}, {}, {}
            for it in range(a.warmup + a.runs):
                for mode in (0, 1):
                    h2g.verify_set_isolation(mode)
                    t0 = time.perf_counter()
                    v, st = vk.verify_batch(ps, insts)
                    el = (time.perf_counter() - t0) * 1e3
                    if it >= a.warmup:
                        ms[mode].append(el)
                    checks[mode], verdicts[mode] = st[0], v
                    stages[mode] = [round(x, 3) for x in h2g.verify_stages()]
            assert verdicts[0] == verdicts[1]
            assert [i for i, x in enumerate(verdicts[1]) if x != h2g.VERIFY_OK] == bad_at
            rows.append({"bad": f, "mode0": dict(summary(ms[0]), checks=checks[0], stages_ms=stages[0]),
                         "mode1": dict(summary(ms[1]), checks=checks[1], stages_ms=stages[1])})
    finally:
        h2g.verify_set_isolation(0)
    out["verify_batch"] = rows
    wins = [r["bad"] for r in rows if r["bad"] and r["mode1"]["ms"] < r["mode0"]["ms"]]
    out["mode1_wins_from_bad"] = min(wins) if wins else None

    # the check alone: valid and invalid pairs from the scalars
    pool = []
    for i in range(16):
        s_a = (0x9E3779B97F4A7C15 * (i + 1)) % B.R
        left = B.g1_mul(B.G1_GEN, s_a)
        right = B.g1_mul(B.G1_GEN, (s_a * S_INT + (i & 1)) % B.R)
        pool.append((B.g1_affine_mont_limbs(left) + B.g1_affine_mont_limbs(right), 1 - (i & 1)))
    alone = []
    for count in CHECK_COUNTS:
        lr = np.array([pool[i % 16][0] for i in range(count)], dtype=np.uint64).reshape(count, 2, 8)
        want = [pool[i % 16][1] for i in range(count)]
        d_lr, d_ok = h2g.DevBuf.from_array(lr), h2g.DevBuf(4 * count)
        host, dev = [], []
        for it in range(a.warmup + a.runs):
            t0 = time.perf_counter()
            ok = h2g.pairing_check_batch(vp, lr)
            t1 = time.perf_counter()
            h2g.pairing_check_batch(vp, d_lr.ptr, dev_count=count, d_ok=d_ok.ptr)
            h2g.check(h2g.lib().h2g_synchronize())
            t2 = time.perf_counter()
            assert list(ok) == want and list(d_ok.download(count, np.int32)) == want
            if it >= a.warmup:
                host.append((t1 - t0) * 1e3)
                dev.append((t2 - t1) * 1e3)
        alone.append({"count": count, "host_entry": summary(host), "dev_entry_and_sync": summary(dev)})
        d_lr.close()
        d_ok.close()
    out["pairing_check_batch"] = alone
    vk.close()
    pk.close()
    params.close()
    h2g.shutdown()
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
