"""Measures what a streamed-coset key (h2g_key_options.cosets = H2G_COSETS_STREAMED) costs and saves.

Per circuit: create_proof with a resident and with a streamed key made from the same params,
both alive in one process on one box (2 warm-ups, then the median of 7 with min - max, the
two keys' proofs alternating), the proofs' equality, and both keys' h2g_pk_memory readings.
Circuits: C3 at k = 22, keccak-style at k = 18, and one wide generated circuit (k = 16,
degree 9, a lookup and a shuffle: 8 sub-cosets, 38 coset columns).

Per transform size (2^18 and 2^22, 8 columns, every sub-coset of a 4n extended domain in
turn): h2g_coeff_to_subcoset_dev -- the twist formed inside the NTT's first pass -- against
the composition it replaces (h2g_debug_coeff_to_subcoset_unfused_dev: a twist launch per
column, then the batched NTT), HIP-event times of 20 calls each, interleaved.

Every case runs in a process of its own under its own time limit.
usage: python tools/streamed_bench.py [--out profiles/streamed/streamed_bench.json]
       python tools/streamed_bench.py --one prove:c3:22      (one case, one JSON line)"""
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "yet-another-halo2-fork_amd"), os.path.join(REPO, "tests"),
                os.path.join(REPO, "oracle", "py")]

CASES = [("prove:c3:22", 420), ("prove:keccak:18", 300), ("prove:wide:16", 300),
         ("transform:18", 120), ("transform:22", 240)]  # (case, seconds allowed)
WARMUP, RUNS = 2, 7
S_INT = 0x1234567


def stats(v, prefix):
    return {prefix + "_ms_median": round(statistics.median(v), 3), prefix + "_ms_min": round(min(v), 3),
            prefix + "_ms_max": round(max(v), 3)}


def prove(kind, k):
    import numpy as np

    import h2g
    import h2g_circuit as hc

    h2g.init()
    if kind == "c3":
        circ, wit = hc.synthetic_c3(k, h2g.DeviceOps, seed=3)
    elif kind == "keccak":
        circ, wit = hc.keccak_style(k, words=16, seed=5)
    else:
        import _gen_circuit as G

        circ, wit, fill = G.generate(seed=778, k=k, degree=9, gates=1, nodes=(30, 31), lookups=(1,), shuffle=True)
        assert fill is None
    params = h2g.Params(k, s=np.asarray(hc.fr_to_limbs(S_INT), dtype=np.uint64))
    keys = {c: h2g.ProvingKey(params, circ, cosets=c) for c in ("resident", "streamed")}
    adv = h2g.DevBuf.from_array(np.ascontiguousarray(wit.advice))
    sync = lambda: h2g.check(h2g.lib().h2g_synchronize())
    ms = {c: [] for c in keys}
    proofs = {}
    for it in range(WARMUP + RUNS):
        for c, pk in keys.items():
            sync()
            t0 = time.perf_counter()
            p = pk.create_proof(wit=wit, advice_dev_ptr=adv.ptr)
            el = (time.perf_counter() - t0) * 1e3
            assert proofs.setdefault(c, p) == p
            if it >= WARMUP:
                ms[c].append(el)
    out = {"case": f"prove:{kind}:{k}", "k": k, "extended_k": keys["resident"].extended_k, "warmup": WARMUP,
           "runs": RUNS, "columns": {"fixed": circ.num_fixed, "perm": len(circ.perm_columns),
                                     "advice": circ.num_advice, "instance": circ.num_instance,
                                     "perm_sets": keys["resident"].nsets, "lookups": len(circ.lookups),
                                     "shuffles": len(circ.shuffles)}}
    for c in keys:
        out.update(stats(ms[c], c + "_proof"))
        out[c + "_memory"] = keys[c].memory()
    out["streamed_over_resident"] = round(out["streamed_proof_ms_median"] / out["resident_proof_ms_median"], 3)
    out["proofs_equal"] = proofs["resident"] == proofs["streamed"]
    out["proof_sha"] = hashlib.sha256(proofs["resident"]).hexdigest()[:16]
    # where the streamed proof's time goes: its stages beside the resident proof's
    for c, pk in keys.items():
        pk.create_proof(wit=wit, advice_dev_ptr=adv.ptr)
        try:
            out[c + "_stages_ms"] = h2g.prover_stages()
        except Exception as e:  # noqa: BLE001 -- the stage clock is optional diagnostics
            out[c + "_stages_ms"] = repr(e)
    print(json.dumps(out), flush=True)
    assert out["proofs_equal"], "the streamed key's proof differs from the resident key's"
    adv.close()
    for pk in keys.values():
        pk.close()
    params.close()
    h2g.shutdown()


def transform(k, cols=8, reps=20):
    import numpy as np

    import h2g

    h2g.init()
    L = h2g.lib()
    d = h2g.Domain(5, k)  # extended domain 4n
    E = 1 << (d.extended_k - d.k)
    n, nb = d.n, d.n * 32
    r = np.random.default_rng(k)
    a = r.integers(0, 2**63, size=(n, 4), dtype=np.int64).astype(np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)  # any integers below r: timing and equality only
    a = np.tile(a, (cols, 1))
    src, dst, dst2 = h2g.DevBuf.from_array(a), h2g.DevBuf(cols * nb), h2g.DevBuf(cols * nb)
    sp = (h2g.VP * cols)(*[src.ptr + i * nb for i in range(cols)])
    dp = (h2g.VP * cols)(*[dst.ptr + i * nb for i in range(cols)])
    dp2 = (h2g.VP * cols)(*[dst2.ptr + i * nb for i in range(cols)])
    fused = lambda t: h2g.check(L.h2g_coeff_to_subcoset_dev(d.h, sp, cols, t, dp, None))

    def unfused(t):
        h2g.check(L.h2g_debug_coeff_to_subcoset_unfused_dev(d.h, sp, cols, t, dp2, None))

    ev = []
    for _ in range(2):
        e = h2g.VP()
        h2g.check(L.h2g_event_create(ctypes.byref(e)))
        ev.append(e)
    same = True
    for t in range(E):
        fused(t)
        unfused(t)
        same = same and dst.download((cols * n, 4)).tobytes() == dst2.download((cols * n, 4)).tobytes()
    ms = {"fused": [], "twist_then_ntt": []}
    for rep in range(WARMUP + RUNS):
        for name, fn in (("fused", fused), ("twist_then_ntt", unfused)):
            h2g.check(L.h2g_synchronize())
            h2g.check(L.h2g_event_record(ev[0], None))
            for i in range(reps):
                fn(i % E)
            h2g.check(L.h2g_event_record(ev[1], None))
            h2g.check(L.h2g_synchronize())
            f = ctypes.c_float()
            h2g.check(L.h2g_event_elapsed_ms(ev[0], ev[1], ctypes.byref(f)))
            if rep >= WARMUP:
                ms[name].append(f.value / reps)
    out = {"case": f"transform:{k}", "k": k, "columns": cols, "sub_cosets": E, "calls_per_sample": reps,
           "warmup": WARMUP, "runs": RUNS, "results_equal": same}
    for name in ms:
        out.update(stats(ms[name], name))
    out["fused_over_twist_then_ntt"] = round(out["fused_ms_median"] / out["twist_then_ntt_ms_median"], 3)
    print(json.dumps(out), flush=True)
    assert same, "the fused transform disagrees with the twist + NTT composition"
    h2g.shutdown()


def one(case):
    kind, *rest = case.split(":")
    if kind == "prove":
        return prove(rest[0], int(rest[1]))
    return transform(int(rest[0]))


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--one")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "streamed", "streamed_bench.json"))
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
        json.dump({"tool": "tools/streamed_bench.py", "results": results}, f, indent=1)
        f.write("\n")
    return 0 if all("error" not in r for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
