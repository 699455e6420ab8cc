"""GPU tests (MI355X) of the known-openings table of the constants/sigmas tree (merkle.hip
k_merkle_known / k_merkle_known_miss, include/p2v.h p2v_circuit_known_stats).

The table is exact memoisation, so every status and trace word must equal the oracle's and those
of a verifier with the table off (P2V_KNOWN_LEAVES=0), cold, warm, and with one word changed
under a warm table; the counters say which openings took which way.  Each test makes its own
circuit handle, so its table starts cold.  The CPU model is tests/test_known_model.py."""
import json

import numpy as np
import pytest

from support import P, gen_circuit, mutate, oracle, p2v_module, trace_offsets

pytestmark = pytest.mark.gpu

ARGS = (6, 4, 0, 1, 28, 16, 0, 1)   # the smallest real circuit of the Merkle tests: LDE 2^9, cap 16, paths of 5
N = 128                             # two 64-proof tiles, above the latency mode
DISTINCT = 16


@pytest.fixture(scope="module")
def p2v():
    import torch   # before libp2v, as tests/test_gpu.py
    assert torch.cuda.is_available(), "torch sees no GPU"
    m = p2v_module()
    if m.device_count() == 0:
        pytest.fail("no GPU visible to libp2v")
    return m


_oracle_memo = {}


def _oracle(gc, proof):
    if proof not in _oracle_memo:
        _oracle_memo[proof] = oracle().verify_json(gc.common, gc.vkey, proof, trace=True)
    return _oracle_memo[proof]


@pytest.fixture(scope="module")
def work(p2v):
    """DISTINCT valid proofs of the circuit, their oracle results and their query indices."""
    gc = gen_circuit(*ARGS)
    proofs = [gc.proof(1 + i % 4, 11 + i) for i in range(DISTINCT)]
    vk = p2v.VerifierCircuitData.from_json(gc.common, gc.vkey)
    info = vk.info
    off = trace_offsets(info.num_challenges, info.num_fri_steps, info.num_query_rounds)["query_idx"]
    qidx = []
    for pr in proofs:
        st, tr = _oracle(gc, pr)
        assert st == 1
        qidx.append([int(x) for x in tr[off: off + info.num_query_rounds]])
    return {"gc": gc, "proofs": proofs, "qidx": qidx, "Q": info.num_query_rounds, "packed": vk.pack_many(proofs)}


def _fresh(p2v, gc):
    return p2v.VerifierCircuitData.from_json(gc.common, gc.vkey)


def _check_vs_oracle(gc, texts, res, tr):
    for i, t in enumerate(texts):
        st, otr = _oracle(gc, t)
        assert int(res[i]) == st, (i, int(res[i]), st)
        assert np.array_equal(tr[i], otr), (i, np.nonzero(tr[i] != otr)[0][:10])


def _off(p2v, gc, rows, monkeypatch, **kw):
    """The same rows on a verifier without the table (the launch sequence before it existed)."""
    monkeypatch.setenv("P2V_KNOWN_LEAVES", "0")
    vk = _fresh(p2v, gc)
    out = p2v.BatchVerifier(vk, 0, len(rows)).run(rows, trace=True, **kw)
    assert vk.known_stats() == {"hits": 0, "misses": 0, "inserted": 0}
    monkeypatch.delenv("P2V_KNOWN_LEAVES")
    return out


def _delta(a, b):
    return {k: b[k] - a[k] for k in a}


@pytest.mark.parametrize("n,tiled", [(N, False), (N, True), (640, True)])
def test_gpu_known_cold_then_warm(p2v, work, n, tiled, monkeypatch):
    """The same batch twice on a cold handle: both runs' statuses and traces equal the oracle's and
    the off build's; run 1 is all misses and inserts one row per distinct index opened, run 2 is
    all hits.  n = 640: the cold list (17 920 openings) is past the row form's four passes, so the
    miss kernel runs one lane per entry; n = 128: its row form."""
    gc, Q = work["gc"], work["Q"]
    sel = np.arange(n) % DISTINCT
    rows = np.ascontiguousarray(work["packed"][sel])
    texts = [work["proofs"][i] for i in sel]
    ref, rtr = _off(p2v, gc, rows, monkeypatch, tiled=tiled)
    vk = _fresh(p2v, gc)
    bv = p2v.BatchVerifier(vk, 0, n)
    distinct = len({i for k in set(sel.tolist()) for i in work["qidx"][k]})
    for run in range(2):
        res, tr = bv.run(rows, trace=True, tiled=tiled)
        _check_vs_oracle(gc, texts[:DISTINCT], res, tr)
        assert np.array_equal(res, ref) and np.array_equal(tr, rtr)
        s = vk.known_stats()
        print("run", run, s)
        if run == 0:
            assert s == {"hits": 0, "misses": n * Q, "inserted": distinct}
        else:
            assert s == {"hits": n * Q, "misses": n * Q, "inserted": distinct}


def _tree0(d, q):
    return d["proof"]["opening_proof"]["query_round_proofs"][q]["initial_trees_proof"]["evals_proofs"][0]


def test_gpu_known_warm_table_one_word_changed(p2v, work, monkeypatch):
    """After warming, one proof each with a tree-0 leaf word, the level-0 sibling or the top sibling
    changed, and one whose query carries another query's authentic leaf and path (right content,
    wrong index): each is rejected as the oracle rejects it, and the misses are exactly the
    mutated openings."""
    gc, Q = work["gc"], work["Q"]
    base = work["proofs"][0]
    qi = work["qidx"][0]
    depth = len(_tree0(json.loads(base), 0)[1]["siblings"])
    a = next(q for q in range(1, Q) if qi[q] != qi[0])

    def leaf_word(d):
        w = _tree0(d, 3)[0]
        w[len(w) - 1] = (w[len(w) - 1] + 1) % P

    def sib_at(q, l):
        def f(d):
            e = _tree0(d, q)[1]["siblings"][l]["elements"]
            e[2] = (e[2] + 1) % P
        return f

    def other_query(d):
        evs = d["proof"]["opening_proof"]["query_round_proofs"]
        evs[a]["initial_trees_proof"]["evals_proofs"][0] = json.loads(json.dumps(_tree0(d, 0)))

    muts = [mutate(base, leaf_word), mutate(base, sib_at(5, 0)), mutate(base, sib_at(7, depth - 1)), mutate(base, other_query)]
    sel = np.arange(N) % DISTINCT
    texts = [work["proofs"][i] for i in sel]
    vk = _fresh(p2v, gc)
    bv = p2v.BatchVerifier(vk, 0, N)
    warm = np.ascontiguousarray(work["packed"][sel])
    assert (bv.run(warm) == 1).all()
    s0 = vk.known_stats()
    rows = warm.copy()
    at = [9, 40, 77, 127]   # both tiles
    for k, m in zip(at, muts):
        rows[k] = vk.pack_many([m])[0]
        texts[k] = m
        assert _oracle(gc, m)[0] != 1
    res, tr = bv.run(rows, trace=True)
    _check_vs_oracle(gc, [texts[k] for k in at], res[at], tr[at])
    _check_vs_oracle(gc, texts[:8], res, tr)
    s1 = vk.known_stats()
    print(s0, s1)
    assert _delta(s0, s1) == {"hits": N * Q - len(muts), "misses": len(muts), "inserted": 0}
    ref, rtr = _off(p2v, gc, rows, monkeypatch)
    assert np.array_equal(res, ref) and np.array_equal(tr, rtr)


def test_gpu_known_nothing_false_is_remembered(p2v, work, monkeypatch):
    """A batch of random words on a cold table inserts no row; the honest batch afterwards is
    accepted, all misses, and only then are rows inserted."""
    gc, Q = work["gc"], work["Q"]
    vk = _fresh(p2v, gc)
    bv = p2v.BatchVerifier(vk, 0, N)
    W = work["packed"].shape[1]
    garbage = np.random.default_rng(9).integers(0, P, size=(N, W), dtype=np.uint64)
    res, tr = bv.run(garbage, trace=True)
    assert (res != 1).all()
    assert vk.known_stats() == {"hits": 0, "misses": N * Q, "inserted": 0}
    ref, rtr = _off(p2v, gc, garbage, monkeypatch)
    assert np.array_equal(res, ref) and np.array_equal(tr, rtr)
    sel = np.arange(N) % DISTINCT
    res = bv.run(np.ascontiguousarray(work["packed"][sel]))
    assert (res == 1).all()
    distinct = len({i for k in range(DISTINCT) for i in work["qidx"][k]})
    assert vk.known_stats() == {"hits": 0, "misses": 2 * N * Q, "inserted": distinct}


def test_gpu_known_two_workspaces_two_streams_share_a_cold_circuit(p2v, work, monkeypatch):
    """Two workspaces of one cold handle on two streams, run_device(sync=False) interleaved for three
    rounds: every run's statuses are the oracle's, its statuses and traces equal the off build's,
    and every opening was either a hit or a miss."""
    import torch
    gc, Q = work["gc"], work["Q"]
    dev = torch.device("cuda", 0)
    vk = _fresh(p2v, gc)
    bvs = [p2v.BatchVerifier(vk, 0, N) for _ in range(2)]
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    rows, expect, host_rows = [], [], []
    for j in range(2):   # two different batches over the same proofs, a corrupted leaf in each
        sel = (np.arange(N) * (j + 1) + j) % DISTINCT
        r = np.ascontiguousarray(work["packed"][sel])
        e = np.ones(N, dtype=np.int8)
        k = 17 + 64 * j
        bad = mutate(work["proofs"][sel[k]], lambda d: _tree0(d, 0)[0].__setitem__(0, (_tree0(d, 0)[0][0] + 1) % P))
        r[k] = vk.pack_many([bad])[0]
        e[k] = _oracle(gc, bad)[0]
        assert e[k] == -1
        rows.append(torch.from_numpy(r.view(np.int64)).to(dev))
        expect.append(e)
        host_rows.append(r)
    off = [_off(p2v, gc, r, monkeypatch) for r in host_rows]
    tw = vk.info.trace_words
    out = [[torch.empty(N, dtype=torch.int8, device=dev) for _ in range(3)] for _ in range(2)]
    trs = [[torch.empty((N, tw), dtype=torch.int64, device=dev) for _ in range(3)] for _ in range(2)]
    torch.cuda.synchronize(dev)
    for rnd in range(3):
        for j in range(2):
            bvs[j].run_device(rows[j].data_ptr(), N, out[j][rnd].data_ptr(), stream=streams[j].cuda_stream,
                              trace_ptr=trs[j][rnd].data_ptr(), sync=False)
    torch.cuda.synchronize(dev)
    for j in range(2):
        for rnd in range(3):
            assert np.array_equal(out[j][rnd].cpu().numpy(), expect[j]), (j, rnd)
            assert np.array_equal(out[j][rnd].cpu().numpy(), off[j][0]), (j, rnd)
            assert np.array_equal(trs[j][rnd].cpu().numpy().view(np.uint64), off[j][1]), (j, rnd)
    s = vk.known_stats()
    print(s)
    assert s["hits"] + s["misses"] == 6 * N * Q
    assert s["misses"] >= 6 and s["hits"] > 0   # the corrupted leaves always miss; later rounds find rows


@pytest.mark.parametrize("path", ["keyed", "small", "cse0", "budget"])
def test_gpu_known_off_paths_leave_the_counters_at_zero(p2v, work, path, monkeypatch):
    """Keyed runs, latency-mode runs (<= 64 proofs), P2V_MERKLE_CSE=0 and a table over its budget
    never touch the table; their statuses are the oracle's.  (budget: the 2^11-row table of the
    next circuit size, 1.8 MB against P2V_KNOWN_MAX_MB=1; this file's circuit would fit.)"""
    gc = work["gc"]
    n, kw = N, {}
    if path == "cse0":
        monkeypatch.setenv("P2V_MERKLE_CSE", "0")
    if path == "budget":
        monkeypatch.setenv("P2V_KNOWN_MAX_MB", "1")
        gc = gen_circuit(8, 4, 0, 1, 28, 16, 0, 1)
    if path == "small":
        n = 64
    if path == "keyed":
        kw["key_ids"] = np.zeros(n, dtype=np.uint32)
    proofs = work["proofs"] if gc is work["gc"] else [gc.proof(1, 3), gc.proof(2, 4)]
    vk = _fresh(p2v, gc)
    info = vk.info
    if path == "budget":
        assert (1 << info.lde_bits) * (info.leaf_widths[0] + 4 * (info.lde_bits - info.cap_height)) * 8 > 1 << 20
    texts = [proofs[i % len(proofs)] for i in range(n)]
    rows = np.ascontiguousarray(vk.pack_many(proofs)[np.arange(n) % len(proofs)])
    res, tr = p2v.BatchVerifier(vk, 0, n).run(rows, trace=True, **kw)
    _check_vs_oracle(gc, texts[:len(proofs)], res, tr)
    assert (res == 1).all()
    assert vk.known_stats() == {"hits": 0, "misses": 0, "inserted": 0}
    ref, rtr = _off(p2v, gc, rows, monkeypatch, **kw)   # the same path with P2V_KNOWN_LEAVES=0 beside it
    assert np.array_equal(res, ref) and np.array_equal(tr, rtr)


@pytest.mark.parametrize("env", [{"P2V_KNOWN_LEAVES": "2"}, {"P2V_SINGLE_STREAM": "1"},
                                 {"P2V_KNOWN_LEAVES": "2", "P2V_SINGLE_STREAM": "1"}])
def test_gpu_known_probe_only_and_single_stream(p2v, work, env, monkeypatch):
    """P2V_KNOWN_LEAVES=2 probes but never inserts, so three runs of one batch are all misses and
    the table stays empty; P2V_SINGLE_STREAM=1 runs the new kernels in line on the caller's stream,
    cold then warm.  A corrupted leaf and a corrupted top sibling ride along.  Statuses and traces
    equal the oracle's and the off build's in every run."""
    gc, Q = work["gc"], work["Q"]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    vk = _fresh(p2v, gc)
    bv = p2v.BatchVerifier(vk, 0, N)
    sel = np.arange(N) % DISTINCT
    texts = [work["proofs"][i] for i in sel]
    depth = len(_tree0(json.loads(texts[0]), 0)[1]["siblings"])

    def leaf(d):
        _tree0(d, 1)[0][0] = (_tree0(d, 1)[0][0] + 1) % P

    def top(d):
        e = _tree0(d, 2)[1]["siblings"][depth - 1]["elements"]
        e[0] = (e[0] + 1) % P
    texts[5], texts[100] = mutate(texts[5], leaf), mutate(texts[100], top)
    rows = np.ascontiguousarray(work["packed"][sel])   # the valid proofs; then the two corrupted ones
    for k in (5, 100):
        rows[k] = vk.pack_many([texts[k]])[0]
    probe_only = env.get("P2V_KNOWN_LEAVES") == "2"
    distinct = len({i for k in range(DISTINCT) for i in work["qidx"][k]})
    outs = []
    for run in range(3):
        res, tr = bv.run(rows, trace=True)
        outs.append((res, tr))
        _check_vs_oracle(gc, [texts[k] for k in (0, 5, 100)], res[[0, 5, 100]], tr[[0, 5, 100]])
        s = vk.known_stats()
        print(env, run, s)
        if probe_only:
            assert s == {"hits": 0, "misses": (run + 1) * N * Q, "inserted": 0}
        else:   # run 0 all misses; then everything but the two corrupted openings hits
            assert s == {"hits": run * (N * Q - 2), "misses": N * Q + 2 * run, "inserted": distinct}
    for k, v in env.items():
        monkeypatch.delenv(k)
    ref, rtr = _off(p2v, gc, rows, monkeypatch)
    for res, tr in outs:
        assert np.array_equal(res, ref) and np.array_equal(tr, rtr)
