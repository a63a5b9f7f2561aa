"""Times the standalone multi-open argument: h2g_multiopen_prove (SHPLONK and GWC) over 16
device-resident polynomials of 2^20 coefficients, each opened at 3 points (x, w x, w^-1 x) --
the evaluations, the argument's kernels and its commitments, the transcript on the host.  2
warm-ups, then the median of 7 with min - max.  Beside them, for context: the "shplonk h" +
"shplonk final" stages of a C3 k = 20 create_proof under h2g_prover_stage_sync(1) (the proof's
own 12 polynomials and 17 queries, its evaluations not included), the same code inside the prover.
There is no target: this is where the first number of this path on its own is written down.
usage: python tools/multiopen_bench.py [--out profiles/multiopen/multiopen_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "yet-another-halo2-fork_amd")]

K, NPOLY, WARMUP, RUNS = 20, 16, 2, 7
S_INT = 0xBA5E5


def stats(v):
    return {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multiopen", "multiopen_bench.json"))
    a = ap.parse_args()
    import numpy as np

    import h2g
    import h2g_circuit as hc

    h2g.init()
    L = h2g.lib()

    def sync():
        h2g.check(L.h2g_synchronize())

    n = 1 << K
    prm = h2g.Params(K, s=np.asarray(hc.fr_to_limbs(S_INT), dtype=np.uint64))
    rng = np.random.default_rng(20)
    base = rng.integers(0, 2**63, size=(n, 4), dtype=np.int64).astype(np.uint64)
    base[:, 3] &= np.uint64((1 << 60) - 1)  # limbs below r: valid (Montgomery) field elements
    bufs = [h2g.DevBuf.from_array(np.roll(base, 7919 * i, axis=0)) for i in range(NPOLY)]
    polys = [(b.ptr, n) for b in bufs]
    dom = h2g.Domain(3, K)  # only its omega is used
    x = np.asarray(hc.fr_to_limbs(0x1234567), dtype=np.uint64)
    xs = np.stack([x, x])
    pts = [x] + list(h2g.fr_op(h2g.OP_MUL, xs, np.ascontiguousarray(dom.consts[:2])))  # x, w x, w^-1 x
    dom.close()
    queries = [(i, p) for i in range(NPOLY) for p in pts]
    out = {"tool": "tools/multiopen_bench.py", "k": K, "polynomials": NPOLY, "points": len(pts),
           "queries": len(queries), "warmup": WARMUP, "runs": RUNS, "results": {}}
    for scheme in ("shplonk", "gwc"):
        ms, proofs = [], set()
        for it in range(WARMUP + RUNS):
            T = h2g.Transcript("blake2b")
            sync()
            t0 = time.perf_counter()
            prm.multiopen_prove(T, polys, queries, scheme)
            sync()
            if it >= WARMUP:
                ms.append((time.perf_counter() - t0) * 1e3)
            proofs.add(T.bytes())
            T.close()
        assert len(proofs) == 1
        out["results"][scheme] = dict(stats(ms), proof_bytes=len(next(iter(proofs))))
        print(json.dumps({scheme: out["results"][scheme]}), flush=True)
    for b in bufs:
        b.close()
    # the same code inside create_proof: C3 at k = 20, stage times at GPU completion
    circ, wit = hc.synthetic_c3(K, h2g.DeviceOps, seed=3)
    pk = h2g.ProvingKey(prm, circ)
    h2g.prover_stage_sync(True)
    tail = []
    for it in range(WARMUP + RUNS):
        pk.create_proof(wit)
        st = dict(h2g.prover_stages())
        if it >= WARMUP:
            tail.append(st["shplonk h"] + st["shplonk final"])
    h2g.prover_stage_sync(False)
    out["results"]["c3_k20_create_proof_shplonk_stages"] = stats(tail)
    print(json.dumps({"c3_k20_create_proof_shplonk_stages": out["results"]["c3_k20_create_proof_shplonk_stages"]}),
          flush=True)
    pk.close()
    prm.close()
    h2g.shutdown()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
