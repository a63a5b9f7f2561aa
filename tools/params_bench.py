"""Times the params' downsizing: h2g_g1_to_lagrange_dev on resident points at k = 16, 20, 22 and
h2g_params_downsize 24 -> 22 (truncation, the group FFT and the new params' fixed-base
windows).  2 warm-ups, then the median of 7 with min - max; every case runs in a process of
its own under its own time limit.  Beside each result: h2g_params_setup at the same k, for
context only -- setup multiplies the one generator by n known scalars, a different job.
chains_per_s counts the (k/2 + 1) 2^k double-and-add chains of the transform, the figure to
hold against the segmented MSM's ~14 M chains/s.
usage: python tools/params_bench.py [--out profiles/params/params_bench.json]
       python tools/params_bench.py --one g1:20        (one case, one JSON line)"""
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "yet-another-halo2-fork_amd")]

CASES = [("g1:16", 120), ("g1:20", 180), ("g1:22", 420), ("downsize:24:22", 540)]  # (case, seconds allowed)
WARMUP, RUNS = 2, 7
S_INT = 0xBA5E5


def stats(v, prefix):
    return {prefix + "_ms_median": round(statistics.median(v), 3), prefix + "_ms_min": round(min(v), 3),
            prefix + "_ms_max": round(max(v), 3)}


def timed(fn, sync):
    out = []
    for it in range(WARMUP + RUNS):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if it >= WARMUP:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def one(case):
    import numpy as np

    import h2g
    import h2g_circuit as hc

    h2g.init()
    L = h2g.lib()
    s = np.asarray(hc.fr_to_limbs(S_INT), dtype=np.uint64)

    def sync():
        h2g.check(L.h2g_synchronize())

    kind, *ks = case.split(":")
    k = int(ks[-1])
    n = 1 << k
    out = {"case": case, "k": k, "warmup": WARMUP, "runs": RUNS}
    t0 = time.perf_counter()
    ref = h2g.Params(k, s=s)
    sync()
    out["params_setup_same_k_ms_once"] = round((time.perf_counter() - t0) * 1e3, 3)
    if kind == "g1":
        d_g, d_out = h2g.DevBuf(n * 64), h2g.DevBuf(n * 64)
        h2g.srs_setup_dev(s, n, d_g.ptr)
        ms = timed(lambda: h2g.g1_to_lagrange_dev(d_g.ptr, k, d_out.ptr), sync)
        out.update(stats(ms, "g1_to_lagrange_dev"))
        chains = (k / 2 + 1) * n
        out["chains"] = int(chains)
        out["chains_per_s"] = round(chains / (out["g1_to_lagrange_dev_ms_median"] * 1e-3))
        # the whole basis against setup's closed form, on the device's own copy
        got = d_out.download((n, 8))
        out["equals_setup_lagrange_basis"] = bool(np.array_equal(got, ref.export()[1]))
    else:
        big = h2g.Params(int(ks[0]), s=s)
        made = []

        def run():
            for p in made:
                p.close()
            made[:] = [big.downsize(k)]

        out["from_k"] = int(ks[0])
        out.update(stats(timed(run, sync), "params_downsize"))
        out["equals_setup_lagrange_basis"] = bool(np.array_equal(made[0].export()[1], ref.export()[1]))
    print(json.dumps(out), flush=True)
    assert out["equals_setup_lagrange_basis"], "the transform disagrees with h2g_params_setup"
    h2g.shutdown()


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "params", "params_bench.json"))
    a = ap.parse_args()
    if a.one:
        return one(a.one)
    results = []
    for case, limit in CASES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", case], capture_output=True,
                               text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            results.append({"case": case, "error": f"no result within {limit} s"})
            print(json.dumps(results[-1]), flush=True)
            break  # the device may still be busy with it: nothing more is started
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        results.append(json.loads(lines[-1]) if lines else {"case": case, "error": r.stderr[-400:]})
        print(json.dumps(results[-1]), flush=True)
        if r.returncode != 0:
            break
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/params_bench.py", "results": results}, f, indent=1)
        f.write("\n")
    return 0 if all("error" not in r for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
