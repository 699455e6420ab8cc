#!/usr/bin/env python3
"""What interpreting gates as programs costs (developer tool).

The bench's C2 workload -- 4096 proofs of the real degree_bits-12 recursion circuit, resident in
HBM in the 64-proof tiled layout, two workspaces in flight -- timed in one process in two legs,
alternated so that clock drift hits them alike:
  (a) the circuit as it is: every gate through its hand-written kernel
  (b) the same proofs against the same circuit with every gate that tests/gate_programs.py
      restates renamed and registered as a gate program (k_vanish_prog_r2 interprets them)
Both legs verify the same valid proofs, all accepted (checked on the device after every launch).
Each leg reports proofs/s, the shader clock its pass held (clock probes at both ends) and
proofs/s per GHz; the spread between the repeated (a) legs is the yardstick for (b).  A closing
serial pass gives each leg's per-kernel times (p2v_verifier_last_timings: k_vanish is the slot
of all the vanishing classes together, k_merkle the main stream's).  Prints one JSON line.
"""
import argparse
import concurrent.futures as cf
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import gate_programs as gp  # noqa: E402
from support import generator, p2v_module  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--degree-bits", type=int, default=12)
    ap.add_argument("--distinct", type=int, default=64, help="distinct proofs in the batch")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3, help="times each leg is run (alternated)")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    p2v = p2v_module()
    p2v.check_build()
    B = args.batch
    gc = generator().circuit(args.degree_bits, 4, 0, 1, 28, 16, 0, 1)
    gc.witness(1)
    with cf.ThreadPoolExecutor(16) as ex:
        texts = list(ex.map(lambda j: gc.proof(1, 1 + j), range(args.distinct)))
    common, progs, idx = gp.rename(gc.common)
    vks = {"a": p2v.VerifierCircuitData.from_json(gc.common, gc.vkey),
           "b": p2v.VerifierCircuitData.from_json(common, gc.vkey, gates=progs)}
    assert vks["a"].num_program_gates == 0 and vks["b"].num_program_gates == len(idx)
    packed = vks["a"].pack_many(texts)
    dev = torch.device("cuda", 0)
    d_rows = torch.from_numpy(p2v.tile_proofs(np.ascontiguousarray(packed[np.arange(B) % len(texts)])).view(np.int64)).to(dev)
    d_want = torch.ones(B, dtype=torch.int8, device=dev)
    nv = 2
    bvs = {leg: [p2v.BatchVerifier(vks[leg], 0, B) for _ in range(nv)] for leg in "ab"}
    streams = [torch.cuda.current_stream(dev), torch.cuda.Stream(dev)]
    d_res = [torch.empty(B, dtype=torch.int8, device=dev) for _ in range(nv)]
    NPROBE = 256

    def launch(leg, j, sync):
        bvs[leg][j].run_device(d_rows.data_ptr(), B, d_res[j].data_ptr(), stream=streams[j].cuda_stream, sync=sync, tiled=True)

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
            p2v.count_mismatches(d_res[j].data_ptr(), d_want.data_ptr(), B, cnt[j].data_ptr(), streams[j].cuda_stream)
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

    legs = {k: [] for k in "ab"}
    for _ in range(args.repeats):
        for leg in "ab":
            legs[leg].append(timed(leg, args.steps))
    kernels = {}
    for leg in "ab":   # serial: per-kernel times of the last of a few synchronous runs
        for _ in range(3):
            launch(leg, 0, True)
        assert bool((d_res[0] == d_want).all())
        kernels[leg] = {k: round(v, 4) for k, v in bvs[leg][0].last_timings().items()}
    med = {leg: float(np.median([r["per_ghz"] or 0 for r in legs[leg]])) for leg in legs}
    a = [r["per_ghz"] or 0 for r in legs["a"]]
    out = {"workload": f"{B} proofs, degree_bits {args.degree_bits}, tiled, device-resident, {nv} in flight",
           "program_gates": len(idx), "program_instructions": {k: len(g.instrs) for k, g in progs.items()},
           "steps": args.steps, "legs": legs, "median_per_ghz": {k: round(v, 1) for k, v in med.items()},
           "a_spread_per_ghz": round(max(a) - min(a), 1), "a_spread_rel": round((max(a) - min(a)) / med["a"], 5) if med["a"] else None,
           "b_over_a": round(med["b"] / med["a"], 5) if med["a"] else None,
           "serial_kernel_ms": kernels}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
