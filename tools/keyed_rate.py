#!/usr/bin/env python3
"""What per-proof verifier keys cost (developer tool; DESIGN.md "Key tables").

The bench's C2 workload -- 4096 proofs of the real degree_bits-12 recursion circuit, resident in
HBM in the 64-proof tiled layout, two workspaces in flight -- timed in one process in three legs,
alternated so that clock drift hits them alike:
  (a) p2v_verifier_run                      (unkeyed kernels)
  (b) p2v_verifier_run_keyed, every id 0    (keyed kernels, one key)
  (c) p2v_verifier_run_keyed, 16 keys spread uniformly over the batch
The circuits of generator seeds 1..16 share their common data (asserted) and differ in their
key.  Every leg verifies valid proofs, all accepted (checked on the device after every launch):
(a) and (b) 64 distinct proofs of circuit 1, (c) 4 distinct proofs of each circuit, proof i of
the batch under key i % 16.  (A proof under a wrong key is not the same work: its query indices
no longer fit its Merkle paths, so the shared-node checks of k_merkle_cse flag followers that
k_merkle_fix re-runs.)  Each leg reports proofs/s, the shader clock
its pass held (clock probes at both ends) and proofs/s per GHz; the spread between the repeated
(a) legs is the yardstick for (b) and (c).  A closing serial pass gives each leg's per-kernel
times (p2v_verifier_last_timings).  Prints one JSON line.
"""
import argparse
import concurrent.futures as cf
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from support import generator, p2v_module  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--degree-bits", type=int, default=12)
    ap.add_argument("--keys", type=int, default=16)
    ap.add_argument("--per-key", type=int, default=4, help="distinct proofs per key")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3, help="times each leg is run (alternated)")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    p2v = p2v_module()
    p2v.check_build()
    g = generator()
    K, B = args.keys, args.batch
    gcs = [g.circuit(args.degree_bits, 4, 0, s, 28, 16, 0, 1) for s in range(1, K + 1)]
    assert all(c.common == gcs[0].common for c in gcs), "the seeds' circuits do not share their common data"
    assert len({c.vkey for c in gcs}) == K
    with cf.ThreadPoolExecutor(16) as ex:
        list(ex.map(lambda c: c.witness(1), gcs))
        texts = list(ex.map(lambda a: gcs[a[0]].proof(1, 1 + a[1]), [(k, j) for j in range(args.per_key) for k in range(K)]))
        texts0 = list(ex.map(lambda j: gcs[0].proof(1, 1 + j), range(len(texts))))   # as many, all of circuit 1
    base = p2v.VerifierCircuitData.from_json(gcs[0].common, gcs[0].vkey)
    vk = base.with_keys([c.vkey for c in gcs[1:]])
    assert vk.num_keys == K
    packed = vk.pack_many(texts)                      # text t: key t % K
    idx = np.arange(B) % len(texts)
    ids = (idx % K).astype(np.uint32)                 # uniform over the keys
    dev = torch.device("cuda", 0)
    d_mixed = torch.from_numpy(p2v.tile_proofs(np.ascontiguousarray(packed[idx])).view(np.int64)).to(dev)
    d_own = torch.from_numpy(p2v.tile_proofs(np.ascontiguousarray(vk.pack_many(texts0)[idx])).view(np.int64)).to(dev)
    d_rows = {"a": d_own, "b": d_own, "c": d_mixed}
    d_ids = {"a": None, "b": torch.zeros(B, dtype=torch.int32, device=dev), "c": torch.from_numpy(ids.view(np.int32)).to(dev)}
    d_ones = torch.ones(B, dtype=torch.int8, device=dev)
    d_want = {k: d_ones for k in "abc"}
    nv = 2
    bvs = [p2v.BatchVerifier(vk, 0, B) for _ in range(nv)]
    streams = [torch.cuda.current_stream(dev), torch.cuda.Stream(dev)]
    d_res = [torch.empty(B, dtype=torch.int8, device=dev) for _ in range(nv)]
    NPROBE = 256

    def launch(leg, j, sync):
        kid = d_ids[leg]
        bvs[j].run_device(d_rows[leg].data_ptr(), B, d_res[j].data_ptr(), stream=streams[j].cuda_stream, sync=sync, tiled=True,
                          key_ids=kid.data_ptr() if kid is not None else None)

    def timed(leg, steps):
        cnt = torch.zeros((nv, 2), dtype=torch.int64, device=dev)
        stamps = torch.zeros((2, NPROBE, 3), dtype=torch.int64, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(args.warmup):
            launch(leg, i % nv, False)
        streams[0].wait_stream(streams[1])
        e0.record(streams[0])
        streams[1].wait_stream(streams[0])
        p2v.clock_probe(stamps[0].data_ptr(), NPROBE, streams[0].cuda_stream)
        for i in range(steps):
            j = i % nv
            launch(leg, j, False)
            p2v.count_mismatches(d_res[j].data_ptr(), d_want[leg].data_ptr(), B, cnt[j].data_ptr(), streams[j].cuda_stream)
        streams[0].wait_stream(streams[1])
        p2v.clock_probe(stamps[1].data_ptr(), NPROBE, streams[0].cuda_stream)
        e1.record(streams[0])
        torch.cuda.synchronize(dev)
        c = cnt.cpu().numpy()
        assert int(c[:, 0].sum()) == 0 and int(c[:, 1].sum()) == steps, (leg, c.tolist())
        st = stamps.cpu().numpy().view(np.uint64)
        ghz = (p2v.clock_from_probes(st[0], st[1]) or {}).get("clock_ghz")
        rate = B * steps / (e0.elapsed_time(e1) * 1e-3)
        return {"proofs_per_s": round(rate, 1), "clock_ghz": ghz, "per_ghz": round(rate / ghz, 1) if ghz else None}

    legs = {k: [] for k in "abc"}
    for _ in range(args.repeats):
        for leg in "abc":
            legs[leg].append(timed(leg, args.steps))
    kernels = {}
    for leg in "abc":   # serial: per-kernel times of the last of a few synchronous runs
        for _ in range(3):
            launch(leg, 0, True)
        assert bool((d_res[0] == d_want[leg]).all())
        kernels[leg] = {k: round(v, 4) for k, v in bvs[0].last_timings().items()}
    med = {leg: float(np.median([r["per_ghz"] or 0 for r in legs[leg]])) for leg in legs}
    a = [r["per_ghz"] or 0 for r in legs["a"]]
    out = {"workload": f"{B} proofs, degree_bits {args.degree_bits}, tiled, device-resident, {nv} in flight, {K} keys",
           "steps": args.steps, "legs": legs, "median_per_ghz": {k: round(v, 1) for k, v in med.items()},
           "a_spread_per_ghz": round(max(a) - min(a), 1), "a_spread_rel": round((max(a) - min(a)) / med["a"], 5) if med["a"] else None,
           "b_over_a": round(med["b"] / med["a"], 5) if med["a"] else None, "c_over_a": round(med["c"] / med["a"], 5) if med["a"] else None,
           "serial_kernel_ms": kernels}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
