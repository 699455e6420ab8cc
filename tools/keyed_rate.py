#!/usr/bin/env python3
"""What per-proof verifier keys cost (developer tool; DESIGN.md "Key tables").

The bench's C2 workload -- 4096 proofs of the real degree_bits-12 recursion circuit, resident in
HBM in the 64-proof tiled layout, two workspaces in flight -- timed in one process in five legs,
alternated so that clock drift hits them alike (--legs picks a subset):
  (a) p2v_verifier_run                      (unkeyed kernels)
  (b) p2v_verifier_run_keyed, every id 0    (keyed kernels, one key)
  (c) p2v_verifier_run_keyed, 16 keys spread uniformly over the batch, the known-openings table
      on (one block of rows per key), warm
  (c0) as (c) with P2V_KNOWN_LEAVES=0       (no table: the keyed launch sequence before it)
  (c2) as (c) with P2V_KNOWN_LEAVES=2       (probe only: every opening misses, the cold regime)
  (c') as (c) on the SELF-NAMING family: the same shape with 71 public inputs, each proof ending
      them with its own circuit's verifier key (include/p2v.h "self-keyed circuits"); explicit ids
  (d)  the same batch on the self-keyed handle, no ids: k_key_resolve finds them on the device
(c') is (d)'s yardstick: its own spread over the repeats against the gap between their medians.
Each leg has a handle of its own and makes its two workspaces under its own environment (the
switches are read at p2v_verifier_create); a handle's table stays warm between its leg's passes.
The circuits of generator seeds 1..16 share their common data (asserted) and differ in their
key.  Every leg verifies valid proofs, all accepted (checked on the device after every launch):
(a) and (b) 64 distinct proofs of circuit 1, (c) 4 distinct proofs of each circuit, proof i of
the batch under key i % 16.  (A proof under a wrong key is not the same work: its query indices
no longer fit its Merkle paths, so the shared-node checks of k_merkle_cse flag followers that
k_merkle_fix re-runs.)  Each leg reports proofs/s, the shader clock
its pass held (clock probes at both ends) and proofs/s per GHz; the spread between the repeated
(a) legs is the yardstick for the others.  A closing serial pass gives each leg's per-kernel
times (p2v_verifier_last_timings), and a cold-start trace the table's hits, misses and inserted
rows per batch from a cold 16-key handle (--cold-steps).  The trace is of THIS workload, whose
--per-key distinct proofs per key open few distinct indices; traffic of all-distinct proofs warms
as derived in include/p2v.h.  Prints one JSON line.
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
    ap.add_argument("--cold-steps", type=int, default=6, help="batches of the cold-start trace")
    ap.add_argument("--legs", default="a,b,c,c0,c2,cs,d", help="legs to run, in order (cs: the docstring's c')")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    p2v = p2v_module()
    p2v.check_build()
    g = generator()
    K, B = args.keys, args.batch
    LEGS = args.legs.split(",")
    assert LEGS and set(LEGS) <= {"a", "b", "c", "c0", "c2", "cs", "d"}, LEGS
    plain = [leg for leg in LEGS if leg not in ("cs", "d")]   # the legs on the 4-public-input family
    idx = np.arange(B) % (K * args.per_key)           # proof i of a batch: text i % (K per_key), key i % K
    ids = (idx % K).astype(np.uint32)                 # uniform over the keys
    dev = torch.device("cuda", 0)
    leg_env = {"c0": {"P2V_KNOWN_LEAVES": "0"}, "c2": {"P2V_KNOWN_LEAVES": "2"}}
    d_zero, d_uniform = torch.zeros(B, dtype=torch.int32, device=dev), torch.from_numpy(ids.view(np.int32)).to(dev)
    d_ones = torch.ones(B, dtype=torch.int8, device=dev)
    d_want = {k: d_ones for k in LEGS}
    nv = 2
    d_rows, d_ids, handles = {}, {}, {}
    if plain:
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
        d_mixed = torch.from_numpy(p2v.tile_proofs(np.ascontiguousarray(packed[idx])).view(np.int64)).to(dev)
        d_own = torch.from_numpy(p2v.tile_proofs(np.ascontiguousarray(vk.pack_many(texts0)[idx])).view(np.int64)).to(dev)
        d_rows.update({"a": d_own, "b": d_own, "c": d_mixed, "c0": d_mixed, "c2": d_mixed})
        d_ids.update({"a": None, "b": d_zero, "c": d_uniform, "c0": d_uniform, "c2": d_uniform})
        handles.update({leg: base.with_keys([c.vkey for c in gcs[1:]]) for leg in plain})   # each with its own table
    if {"cs", "d"} & set(LEGS):   # the self-naming family: every proof's public inputs end with its circuit's key
        from selfkeys import NUM_PIS, proof_naming, tail_of
        scs = [g.circuit(args.degree_bits, NUM_PIS, 0, s, 28, 16, 0, 1) for s in range(1, K + 1)]
        assert all(c.common == scs[0].common for c in scs) and len({c.vkey for c in scs}) == K
        with cf.ThreadPoolExecutor(16) as ex:
            first = list(ex.map(lambda c: proof_naming(c, tail_of(c.vkey), 1, 1), scs))   # one witness per circuit
            rest = list(ex.map(lambda a: proof_naming(scs[a[0]], tail_of(scs[a[0]].vkey), 1, 1 + a[1]),
                               [(k, j) for j in range(1, args.per_key) for k in range(K)]))
        sbase = p2v.VerifierCircuitData.from_json(scs[0].common, scs[0].vkey)
        handles["cs"] = sbase.with_keys([c.vkey for c in scs[1:]])
        handles["d"] = sbase.with_keys([c.vkey for c in scs[1:]]).self_keyed()
        srows = np.ascontiguousarray(handles["cs"].pack_many(first + rest)[idx])   # text t: key t % K, as `packed`
        assert np.array_equal(p2v.BatchVerifier(handles["d"], 0, B).resolve_keys(srows, tiled=True), ids)
        d_self = torch.from_numpy(p2v.tile_proofs(srows).view(np.int64)).to(dev)
        d_rows.update({"cs": d_self, "d": d_self})
        d_ids.update({"cs": d_uniform, "d": None})
    bvs = []

    def workspaces(leg, count=nv):
        """The leg's workspaces, made under its environment; the earlier leg's are freed first."""
        bvs.clear()
        env = leg_env.get(leg, {})
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            bvs.extend(p2v.BatchVerifier(handles[leg], 0, B) for _ in range(count))
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    streams = [torch.cuda.current_stream(dev), torch.cuda.Stream(dev)]
    d_res = [torch.empty(B, dtype=torch.int8, device=dev) for _ in range(nv)]
    NPROBE = 256

    def launch(leg, j, sync):
        kid = d_ids[leg]
        bvs[j].run_device(d_rows[leg].data_ptr(), B, d_res[j].data_ptr(), stream=streams[j].cuda_stream, sync=sync, tiled=True,
                          key_ids=kid.data_ptr() if kid is not None else None)

    def timed(leg, steps):
        workspaces(leg)
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

    legs = {k: [] for k in LEGS}
    for _ in range(args.repeats):
        for leg in LEGS:
            legs[leg].append(timed(leg, args.steps))
    kernels = {}
    for leg in LEGS:   # serial: per-kernel times of the last of a few synchronous runs
        workspaces(leg, 1)
        for _ in range(3):
            launch(leg, 0, True)
        assert bool((d_res[0] == d_want[leg]).all())
        kernels[leg] = {k: round(v, 4) for k, v in bvs[0].last_timings().items()}
    known = {leg: handles[leg].known_stats() for leg in LEGS}
    # cold start: a fresh handle (a cold table of all keys), one batch at a time
    cold, cold_rows = [], []
    if plain:
        handles["cold"] = base.with_keys([c.vkey for c in gcs[1:]])
        d_rows["cold"], d_ids["cold"], d_want["cold"] = d_mixed, d_uniform, d_ones
        workspaces("cold", 1)
        prev = handles["cold"].known_stats()
        for _ in range(args.cold_steps):
            launch("cold", 0, True)
            cur = handles["cold"].known_stats()
            cold.append({k: cur[k] - prev[k] for k in cur})
            prev = cur
        cold_rows = [handles["cold"].known_rows(k) for k in range(K)]
    med = {leg: float(np.median([r["per_ghz"] or 0 for r in legs[leg]])) for leg in legs}
    out = {"workload": f"{B} proofs, degree_bits {args.degree_bits}, tiled, device-resident, {nv} in flight, {K} keys",
           "steps": args.steps, "legs": legs, "median_per_ghz": {k: round(v, 1) for k, v in med.items()},
           "serial_kernel_ms": kernels, "known_stats": known, "cold_trace": cold, "cold_rows_per_key": cold_rows}
    if med.get("a"):
        a = [r["per_ghz"] or 0 for r in legs["a"]]
        out.update({"a_spread_per_ghz": round(max(a) - min(a), 1), "a_spread_rel": round((max(a) - min(a)) / med["a"], 5),
                    "over_a": {leg: round(med[leg] / med["a"], 5) for leg in LEGS if leg != "a"}})
    if med.get("c") and med.get("c0"):
        out["c_over_c0"] = round(med["c"] / med["c0"], 5)
    if med.get("cs") and med.get("d"):   # (d) against its yardstick (c'): the gap of the medians beside (c')'s own spread
        cs = [r["per_ghz"] or 0 for r in legs["cs"]]
        out.update({"cs_spread_per_ghz": round(max(cs) - min(cs), 1), "d_minus_cs_per_ghz": round(med["d"] - med["cs"], 1),
                    "d_over_cs": round(med["d"] / med["cs"], 5), "d_within_cs_spread": bool(min(cs) <= med["d"] <= max(cs))})
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
