"""The self-checks under a working SPMD transport, on every rank of a two-rank proof: with the
transport installed, modes "verdict" and "arguments" are refused (H2G_ERR_STATE) before any
collective, and mode "off" -- on the same key, whose self-check was on a moment ago -- proves
the bytes the single-device prover gave.  Launched by tests/test_selfcheck_prover_gpu.py:
  python -m torch.distributed.run --nproc-per-node 2 ... tests/_selfcheck_spmd.py
(gloo: the ranks share one GPU, as in tests/_shard_prove.py)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(REPO, "yet-another-halo2-fork_amd"), HERE]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import h2g  # noqa: E402
import h2g_circuit as hc  # noqa: E402
import h2g_dist as D  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    h2g.init([0])
    circ, wit = hc.simple_example(6)
    params = h2g.Params(circ.k, s=np.asarray(hc.fr_to_limbs(0x5eed + circ.k), dtype=np.uint64))
    params.set_slab(*D.slab(1 << circ.k, world, rank))
    pk = h2g.ProvingKey(params, circ)
    want = pk.create_proof(wit)
    res = {"alone": {}, "installed": {}}
    for mode in ("verdict", "arguments"):
        pk.set_self_check(mode)
        res["alone"][mode] = pk.create_proof(wit) == want
    pk.set_self_check("off")
    g = D.SpmdGather(dist)
    g.install()
    try:
        for mode in ("verdict", "arguments"):
            pk.set_self_check(mode)
            try:
                pk.create_proof(wit)
                res["installed"][mode] = "proved"
            except h2g.H2GError as e:
                res["installed"][mode] = [e.code, "transport" in str(e)]
        pk.set_self_check("off")
        res["installed"]["off"] = pk.create_proof(wit) == want
        res["gathers"] = g.calls
    finally:
        D.SpmdGather.uninstall()
    pk.set_self_check("verdict")
    res["after"] = pk.create_proof(wit) == want
    mine = torch.frombuffer(bytearray(json.dumps(res, sort_keys=True).encode().ljust(512)), dtype=torch.uint8).clone()
    every = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(every, mine)
    if rank == 0:
        print("SELFCHECK_SPMD " + json.dumps([json.loads(bytes(t.numpy()).decode()) for t in every]), flush=True)
    pk.close()
    params.close()
    dist.barrier()


if __name__ == "__main__":
    main()
