"""h2g_msm_segmented_dev against the only way to do the same without it: one h2g_msm_dev call
per segment.  Default shape: 1024 segments x 128 random terms over 1024 * 100 + 40 bases (a
batch of 1024 keccak-style proofs' DualMSM sums).  The loop gets its bases gathered into
contiguous slices outside the timed window (h2g_msm_dev takes no index).  Both are timed in
this process, alternating, synchronised around each call, after a warm-up; the results are
compared.  One JSON line.
usage: python tools/msm_seg_bench.py [--segments 1024] [--terms 128] [--runs 7] [--warmup 2]"""
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


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=1024)
    ap.add_argument("--terms", type=int, default=128)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert a.runs >= 7, "the median of at least 7 runs"
    nseg, m = a.segments, a.terms
    nb, nnz = nseg * 100 + 40, nseg * m
    h2g.init()
    L = h2g.lib()
    rng = np.random.default_rng(2024)
    d_bases = h2g.DevBuf(nb * 64)
    h2g.srs_setup_dev(np.asarray(hc.fr_to_limbs(0xBA5E5), dtype=np.uint64), nb, d_bases.ptr)
    bases = d_bases.download((nb, 8))
    sc = rng.integers(0, 1 << 63, size=(nnz, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(nnz, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64(0x0FFFFFFFFFFFFFFF)          # < 2^252 < r: valid Montgomery limbs of a uniform-looking scalar
    ix = rng.integers(0, nb, size=nnz, dtype=np.uint32)
    off = (np.arange(nseg + 1, dtype=np.uint64) * m).astype(np.uint32)
    d_sc = h2g.DevBuf.from_array(sc)
    d_ix = h2g.DevBuf.from_array(ix)
    d_off = h2g.DevBuf.from_array(off)
    d_gather = h2g.DevBuf.from_array(np.ascontiguousarray(bases[ix]))   # the loop's contiguous bases
    d_out_a = h2g.DevBuf(nseg * 64)
    d_out_b = h2g.DevBuf(nseg * 64)

    def segmented():
        h2g.msm_segmented_dev(d_bases.ptr, nb, d_sc.ptr, d_ix.ptr, d_off.ptr, nseg, d_out_a.ptr)

    def loop():
        f = L.h2g_msm_dev
        for s in range(nseg):
            h2g.check(f(d_sc.ptr + 32 * m * s, d_gather.ptr + 64 * m * s, m, d_out_b.ptr + 64 * s, None))

    ms = {"segmented": [], "loop": []}
    for it in range(a.warmup + a.runs):
        for name, fn in (("segmented", segmented), ("loop", loop)):
            h2g.check(L.h2g_synchronize())
            t0 = time.perf_counter()
            fn()
            h2g.check(L.h2g_synchronize())
            if it >= a.warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    same = bool(np.array_equal(d_out_a.download((nseg, 8)), d_out_b.download((nseg, 8))))
    out = {"segments": nseg, "terms_per_segment": m, "bases": nb, "runs": a.runs, "results_equal": same}
    for name, v in ms.items():
        out[name + "_ms_median"] = round(statistics.median(v), 3)
        out[name + "_ms_min"] = round(min(v), 3)
        out[name + "_ms_max"] = round(max(v), 3)
    out["speedup_median"] = round(out["loop_ms_median"] / out["segmented_ms_median"], 2)
    out["wins_by_more_than_the_loop_spread"] = bool(
        out["loop_ms_min"] - out["segmented_ms_max"] > out["loop_ms_max"] - out["loop_ms_min"])
    print(json.dumps(out), flush=True)
    assert same, "the two ways disagree"
    h2g.shutdown()


if __name__ == "__main__":
    main()
