"""GPU tests (MI355X) of the known-openings table under per-proof verifier keys (merkle.hip
"Keys", include/p2v.h p2v_circuit_known_key_rows).

The table of a handle with a key table has one block of rows per key, so a keyed run
(p2v_verifier_run_keyed) probes and fills row (key_ids[i], idx).  It stays exact memoisation: every
status and trace word equals the oracle's, per (key, proof) pair as tests/test_gpu_keys.py computes
them, and those of a fresh handle with the table off (P2V_KNOWN_LEAVES=0); the counters and the
per-key row counts say which openings took which way and under which key they were filed.  Each
test makes its own handle (with_keys), so its table starts cold.  Shapes: the family of
tests/test_keys.py (LDE 2^9, cap 16, paths of 5), 128-130 proofs (two or three 64-proof tiles,
above the latency mode), 640 for the lane form of the miss list.  The CPU model is
tests/test_known_keyed_model.py."""
import json

import numpy as np
import pytest

from support import P, oracle, p2v_module, trace_offsets
from test_gpu_keys import ERR_CIRCUIT, check, data, device_batch, run_device_ids

pytestmark = pytest.mark.gpu

N = 128
ZERO = {"hits": 0, "misses": 0, "inserted": 0}


@pytest.fixture(scope="module")
def p2v():
    import torch   # before libp2v, as tests/test_gpu.py
    assert torch.cuda.is_available(), "torch sees no GPU"
    m = p2v_module()
    if m.device_count() == 0:
        pytest.fail("no GPU visible to libp2v")
    return m


@pytest.fixture(scope="module")
def D(p2v):
    """The shared family data of tests/test_gpu_keys.py, with the query indices of every
    (key, proof) pair's oracle trace."""
    d = data(p2v)
    info = d.vk.info
    d.Q = info.num_query_rounds
    off = trace_offsets(info.num_challenges, info.num_fri_steps, d.Q)["query_idx"]
    d.qidx = d.tr[:, :, off: off + d.Q].astype(np.int64)   # [key][proof][Q]
    return d


def fresh(D, keys=None):
    """A new handle over the key table (default: all 5 keys): a cold table of its own."""
    return D.base.with_keys(D.keys[1:] if keys is None else keys)


def distinct(D, pairs):
    """Distinct (key, idx) rows that the openings of these (key, proof) pairs touch."""
    return len({(k, int(i)) for k, j in pairs for i in D.qidx[k, j]})


def off(p2v, D, rows, ids, monkeypatch, keys=None, **kw):
    """The same rows and ids on a fresh handle without the table (the launch sequence before it
    existed)."""
    monkeypatch.setenv("P2V_KNOWN_LEAVES", "0")
    vk = fresh(D, keys)
    out = p2v.BatchVerifier(vk, 0, len(rows)).run(rows, trace=True, key_ids=ids, **kw)
    assert vk.known_stats() == ZERO
    monkeypatch.delenv("P2V_KNOWN_LEAVES")
    return out


def delta(a, b):
    return {k: b[k] - a[k] for k in a}


def own_key_batch(D, n):
    """n valid proofs, proof i of circuit i % 3 under its own key."""
    ids = (np.arange(n) % 3).astype(np.uint32)
    return np.ascontiguousarray(D.packed[ids]), ids, D.st[ids, ids], D.tr[ids, ids]


@pytest.mark.parametrize("n,tiled", [(N, False), (N, True), (640, True)])
def test_gpu_known_keyed_cold_then_warm(p2v, D, n, tiled, monkeypatch):
    """Valid proofs each under its own key, twice on a cold handle: run 1 is all misses and inserts
    one row per distinct (key, index) opened, run 2 is all hits; the per-key row counts are the
    distinct indices of that key's proof.  n = 640: the cold list (17 920 openings) is past the row
    form's four passes, so the miss kernel runs one lane per entry; n = 128: its row form.  (On the
    parent commit a keyed run left every counter at zero.)"""
    rows, ids, want_st, want_tr = own_key_batch(D, n)
    assert (want_st == 1).all()
    ref, rtr = off(p2v, D, rows, ids, monkeypatch, tiled=tiled)
    vk = fresh(D)
    bv = p2v.BatchVerifier(vk, 0, n)
    d = distinct(D, [(k, k) for k in range(3)])
    for run in range(2):
        res, tr = bv.run(rows, trace=True, tiled=tiled, key_ids=ids)
        check(res, tr, want_st, want_tr)
        assert np.array_equal(res, ref) and np.array_equal(tr, rtr)
        s = vk.known_stats()
        print("run", run, s)
        assert s == {"hits": run * n * D.Q, "misses": n * D.Q, "inserted": d}
    per_key = [vk.known_rows(k) for k in range(5)]
    assert per_key == [distinct(D, [(k, k)]) for k in range(3)] + [0, 0] and sum(per_key) == d


@pytest.mark.parametrize("proof,own,other", [(0, 0, 4), (1, 1, 3)])
def test_gpu_known_keyed_key_isolation(p2v, D, proof, own, other, monkeypatch):
    """The soundness test.  Warm key `own` with its valid proof, then present the same rows under
    the hybrid key with the same digest and another cap: the transcript is the same, so the
    indices and every opened word are the same, and only the cap differs.  Every status is -1 as
    the oracle says, every opening misses, nothing is inserted and the other key's rows stay
    empty, on two consecutive runs; the own id afterwards is all hits."""
    assert D.st[own, proof] == 1 and D.st[other, proof] == -1
    assert np.array_equal(D.qidx[own, proof], D.qidx[other, proof])
    vk = fresh(D)
    bv = p2v.BatchVerifier(vk, 0, N)
    rows = np.ascontiguousarray(D.packed[[proof] * N])
    ids_own, ids_other = np.full(N, own, dtype=np.uint32), np.full(N, other, dtype=np.uint32)
    nq, d = N * D.Q, distinct(D, [(own, proof)])
    assert (bv.run(rows, key_ids=ids_own) == 1).all()
    s = vk.known_stats()
    assert s == {"hits": 0, "misses": nq, "inserted": d}
    ref, rtr = off(p2v, D, rows, ids_other, monkeypatch)
    for _ in range(2):
        res, tr = bv.run(rows, trace=True, key_ids=ids_other)
        check(res, tr, D.st[ids_other, proof], D.tr[ids_other, proof])
        assert (res == -1).all() and np.array_equal(res, ref) and np.array_equal(tr, rtr)
        s1 = vk.known_stats()
        assert delta(s, s1) == {"hits": 0, "misses": nq, "inserted": 0}
        assert vk.known_rows(other) == 0 and vk.known_rows(own) == d
        s = s1
    assert (bv.run(rows, key_ids=ids_own) == 1).all()
    assert delta(s, vk.known_stats()) == {"hits": nq, "misses": 0, "inserted": 0}


@pytest.mark.parametrize("first", ["unkeyed", "keyed"])
def test_gpu_known_keyed_id_zero_shares_the_unkeyed_rows(p2v, D, first):
    """Key 0's rows are the unkeyed runs' on a multi-key handle: warmed by one form, the other is
    all hits."""
    vk = fresh(D)
    bv = p2v.BatchVerifier(vk, 0, N)
    rows = np.ascontiguousarray(D.packed[[0] * N])
    zeros = np.zeros(N, dtype=np.uint32)
    nq, d = N * D.Q, distinct(D, [(0, 0)])
    order = [None, zeros] if first == "unkeyed" else [zeros, None]
    res, tr = bv.run(rows, trace=True, key_ids=order[0])
    check(res, tr, D.st[zeros, 0], D.tr[zeros, 0])
    assert vk.known_stats() == {"hits": 0, "misses": nq, "inserted": d}
    res, tr = bv.run(rows, trace=True, key_ids=order[1])
    check(res, tr, D.st[zeros, 0], D.tr[zeros, 0])
    assert vk.known_stats() == {"hits": nq, "misses": nq, "inserted": d}
    assert [vk.known_rows(k) for k in range(5)] == [d, 0, 0, 0, 0]


def test_gpu_known_keyed_equal_keys_keep_their_own_rows(p2v, D):
    """A table [k1, k1]: after id 0 is warm, id 1 misses once into its own rows, then hits."""
    vk = fresh(D, [D.keys[0]])
    assert vk.num_keys == 2
    bv = p2v.BatchVerifier(vk, 0, N)
    rows = np.ascontiguousarray(D.packed[[0] * N])
    nq, d = N * D.Q, distinct(D, [(0, 0)])
    want = []
    for k in (0, 1, 1):
        assert (bv.run(rows, key_ids=np.full(N, k, dtype=np.uint32)) == 1).all()
        want.append((vk.known_stats(), vk.known_rows(0), vk.known_rows(1)))
    assert want == [({"hits": 0, "misses": nq, "inserted": d}, d, 0),
                    ({"hits": 0, "misses": 2 * nq, "inserted": 2 * d}, d, d),
                    ({"hits": nq, "misses": 2 * nq, "inserted": 2 * d}, d, d)]


def test_gpu_known_keyed_mixed_matrix_under_a_warm_table(p2v, D, monkeypatch):
    """Every (key, proof) pair of the matrix (statuses 1 / 0 / -1 / -3, all 5 keys) under a table
    warmed with the valid proofs: host ids, device ids, tiled, and two lookahead batches back to
    back.  Statuses and traces equal the oracle's and the off build's, and every opening probed
    was a hit or a miss.  (A wrong-key proof's garbage indices can meet real rows at 2^9 rows, so
    `inserted` is asserted exactly only where every opening's truth is known.)"""
    import torch
    n = 130
    vk = fresh(D)
    bv = p2v.BatchVerifier(vk, 0, n)
    wrows, wids, wst, _ = own_key_batch(D, n)
    assert np.array_equal(bv.run(wrows, key_ids=wids), wst)
    s = vk.known_stats()
    assert s == {"hits": 0, "misses": n * D.Q, "inserted": distinct(D, [(k, k) for k in range(3)])}
    b1, b2 = D.batch(n, seed=41), D.batch(n, seed=42)
    offs = [off(p2v, D, b[0], b[1], monkeypatch) for b in (b1, b2)]
    runs = 0

    def same(res, tr, b, o):
        check(res, tr, b[2], b[3])
        assert np.array_equal(res, o[0]) and np.array_equal(tr, o[1])

    for tiled in (False, True):
        same(*bv.run(b1[0], trace=True, tiled=tiled, key_ids=b1[1]), b1, offs[0])
        d_res, d_tr, _keep = run_device_ids(p2v, bv, b1[0], b1[1], tiled=tiled)
        same(d_res.cpu().numpy(), d_tr.cpu().numpy().view(np.uint64), b1, offs[0])
        runs += 2
    st = torch.cuda.Stream()
    bufs = [device_batch(p2v, vk, b[0], b[1], tiled=(k == 1)) for k, b in enumerate((b1, b2))]
    outs = [run_device_ids(p2v, bv, b[0], b[1], tiled=(k == 1), lookahead=True, stream=st.cuda_stream, sync=False, bufs=bufs[k])
            for k, b in enumerate((b1, b2))]
    torch.cuda.synchronize()
    for o, b, f in zip(outs, (b1, b2), offs):
        same(o[0].cpu().numpy(), o[1].cpu().numpy().view(np.uint64), b, f)
    runs += 2
    s1 = vk.known_stats()
    print(s, s1)
    assert delta(s, s1)["hits"] + delta(s, s1)["misses"] == runs * n * D.Q
    assert delta(s, s1)["hits"] > 0 and delta(s, s1)["misses"] > 0


def _tree0(d, q):
    return d["proof"]["opening_proof"]["query_round_proofs"][q]["initial_trees_proof"]["evals_proofs"][0]


def _oracle_under(D, k, text):
    O = oracle()
    c, pr = O.circuit(D.common, D.keys[k]), O.proof(text)
    out = O.verify(c, pr, trace=True)
    O.L.or_proof_free(pr)
    O.L.or_circuit_free(c)
    return out


def test_gpu_known_keyed_one_word_changed_under_a_warm_table(p2v, D, monkeypatch):
    """After warming, proofs of keys 1 and 2 with one tree-0 leaf word, the level-0 sibling or the
    top sibling changed: rejected as the oracle rejects them under their key, and the misses are
    exactly the mutated openings."""
    n = 130
    vk = fresh(D)
    bv = p2v.BatchVerifier(vk, 0, n)
    rows, ids, want_st, want_tr = own_key_batch(D, n)
    want_st, want_tr = want_st.copy(), want_tr.copy()
    assert np.array_equal(bv.run(rows, key_ids=ids), want_st)
    s0 = vk.known_stats()
    depth = len(_tree0(json.loads(D.texts[1]), 0)[1]["siblings"])

    def leaf_word(q):
        def f(d):
            w = _tree0(d, q)[0]
            w[len(w) - 1] = (w[len(w) - 1] + 1) % P
        return f

    def sib_at(q, l):
        def f(d):
            e = _tree0(d, q)[1]["siblings"][l]["elements"]
            e[2] = (e[2] + 1) % P
        return f
    slots = [1, 2, 64, 65, 127, 128]   # i % 3 in {1, 2}: both tiles' edges and the partial tile
    muts = [leaf_word(3), leaf_word(11), sib_at(5, 0), sib_at(6, 0), sib_at(7, depth - 1), sib_at(27, depth - 1)]
    for slot, m in zip(slots, muts):
        k = int(ids[slot])
        assert k in (1, 2)
        d = json.loads(D.texts[k])
        m(d)
        text = json.dumps(d, separators=(",", ":")).encode()
        want_st[slot], want_tr[slot] = _oracle_under(D, k, text)
        assert want_st[slot] == -1
        rows[slot] = vk.pack_many([text])[0]
    assert {int(ids[s]) for s in slots} == {1, 2}
    res, tr = bv.run(rows, trace=True, key_ids=ids)
    check(res, tr, want_st, want_tr)
    s1 = vk.known_stats()
    print(s0, s1)
    assert delta(s0, s1) == {"hits": n * D.Q - len(muts), "misses": len(muts), "inserted": 0}
    ref, rtr = off(p2v, D, rows, ids, monkeypatch)
    assert np.array_equal(res, ref) and np.array_equal(tr, rtr)


def test_gpu_known_keyed_nothing_false_is_remembered(p2v, D, monkeypatch):
    """A batch of random words with random valid ids on a cold handle inserts no row under any
    key."""
    vk = fresh(D)
    bv = p2v.BatchVerifier(vk, 0, N)
    rng = np.random.default_rng(9)
    garbage = rng.integers(0, P, size=(N, D.packed.shape[1]), dtype=np.uint64)
    ids = rng.integers(0, 5, size=N).astype(np.uint32)
    assert set(ids.tolist()) == set(range(5))
    res, tr = bv.run(garbage, trace=True, key_ids=ids)
    assert (res != 1).all()
    assert vk.known_stats() == {"hits": 0, "misses": N * D.Q, "inserted": 0}
    assert [vk.known_rows(k) for k in range(5)] == [0] * 5
    ref, rtr = off(p2v, D, garbage, ids, monkeypatch)
    assert np.array_equal(res, ref) and np.array_equal(tr, rtr)


def test_gpu_known_keyed_out_of_range_ids(p2v, D):
    """Ids num_keys and 2^32 - 1 mixed into a 70-proof batch, host and device ids: P2V_ERR_CIRCUIT
    for those (their trace rows unspecified), the oracle's status for the rest; a following honest
    batch is correct.  (The table learns from such a proof only what is true of the last key, to
    which its id is clamped.)"""
    n = 70
    vk = fresh(D)
    nk = vk.num_keys
    bv = p2v.BatchVerifier(vk, 0, n)
    ids = np.array(([0, 1, nk, 2 ** 32 - 1, 2] * (n // 5 + 1))[:n], dtype=np.uint32)
    pj = np.arange(n) % 3
    rows = np.ascontiguousarray(D.packed[pj])
    bad = ids >= nk
    safe = np.where(bad, 0, ids)
    want_st = np.where(bad, ERR_CIRCUIT, D.st[safe, pj]).astype(np.int8)
    want_tr = D.tr[safe, pj]
    skip = set(np.flatnonzero(bad).tolist())
    res, tr = bv.run(rows, trace=True, key_ids=ids)
    check(res, tr, want_st, want_tr, skip=skip)
    d_res, d_tr, _keep = run_device_ids(p2v, bv, rows, ids)
    check(d_res.cpu().numpy(), d_tr.cpu().numpy().view(np.uint64), want_st, want_tr, skip=skip)
    s = vk.known_stats()
    assert s["hits"] + s["misses"] == 2 * n * D.Q
    hrows, hids, hst, htr = own_key_batch(D, n)
    res, tr = bv.run(hrows, trace=True, key_ids=hids)
    check(res, tr, hst, htr)
    assert (res == 1).all()


def test_gpu_known_keyed_two_workspaces_two_streams_share_a_cold_handle(p2v, D, monkeypatch):
    """Two workspaces of one cold multi-key handle on two streams, sync=False, interleaved for three
    rounds: every run's statuses and traces equal the oracle's and the off build's, and every
    opening was a hit or a miss."""
    import torch
    n = 130
    dev = torch.device("cuda", 0)
    vk = fresh(D)
    bvs = [p2v.BatchVerifier(vk, 0, n) for _ in range(2)]
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    batches = [D.batch(n, seed=81), D.batch(n, seed=82)]
    offs = [off(p2v, D, b[0], b[1], monkeypatch) for b in batches]
    bufs = [[device_batch(p2v, vk, b[0], b[1]) for _ in range(3)] for b in batches]
    outs = [[None] * 3 for _ in range(2)]
    for rnd in range(3):
        for j, b in enumerate(batches):
            outs[j][rnd] = run_device_ids(p2v, bvs[j], b[0], b[1], stream=streams[j].cuda_stream, sync=False, bufs=bufs[j][rnd])
    torch.cuda.synchronize(dev)
    for j, b in enumerate(batches):
        for rnd in range(3):
            res, tr = outs[j][rnd][0].cpu().numpy(), outs[j][rnd][1].cpu().numpy().view(np.uint64)
            check(res, tr, b[2], b[3])
            assert np.array_equal(res, offs[j][0]) and np.array_equal(tr, offs[j][1]), (j, rnd)
    s = vk.known_stats()
    print(s)
    assert s["hits"] + s["misses"] == 6 * n * D.Q
    assert s["hits"] > 0 and s["inserted"] > 0


@pytest.mark.parametrize("path", ["keyed_budget", "small", "cse0"])
def test_gpu_known_keyed_off_paths_leave_the_counters_at_zero(p2v, D, path, monkeypatch):
    """P2V_KNOWN_KEYED_MAX_MB=0 (the one-key table: a keyed run leaves zeros, an unkeyed run on the
    same handle still counts), a keyed latency-mode run (64 proofs) and a keyed run with
    P2V_MERKLE_CSE=0 never touch the table; their statuses are the oracle's."""
    n = 64 if path == "small" else N
    if path == "cse0":
        monkeypatch.setenv("P2V_MERKLE_CSE", "0")
    if path == "keyed_budget":
        monkeypatch.setenv("P2V_KNOWN_KEYED_MAX_MB", "0")
    vk = fresh(D)
    bv = p2v.BatchVerifier(vk, 0, n)
    rows, ids, want_st, want_tr = own_key_batch(D, n)
    res, tr = bv.run(rows, trace=True, key_ids=ids)
    check(res, tr, want_st, want_tr)
    assert vk.known_stats() == ZERO and [vk.known_rows(k) for k in range(5)] == [0] * 5
    if path == "keyed_budget":
        zeros = np.zeros(n, dtype=np.uint32)
        urows = np.ascontiguousarray(D.packed[[0] * n])
        res, tr = bv.run(urows, trace=True)
        check(res, tr, D.st[zeros, 0], D.tr[zeros, 0])
        d = distinct(D, [(0, 0)])
        assert vk.known_stats() == {"hits": 0, "misses": n * D.Q, "inserted": d}
        assert (bv.run(urows, key_ids=zeros) == 1).all()   # id 0, but keyed: not the table's
        assert vk.known_stats() == {"hits": 0, "misses": n * D.Q, "inserted": d}
        assert [vk.known_rows(k) for k in range(5)] == [d, 0, 0, 0, 0]


@pytest.mark.parametrize("covered", [False, True])
def test_gpu_known_keyed_budget_threshold(p2v, covered, monkeypatch):
    """A real threshold: the 2^11-row table of the next circuit size with lookups (about 1.8 MB per
    key), 3 keys.  A P2V_KNOWN_KEYED_MAX_MB between one key's and three keys' bytes gives the
    one-key behaviour (keyed runs leave zeros, unkeyed runs count); one MB more covers all three
    and a keyed run's second pass is all hits."""
    D8 = data(p2v, 8, 1, 1)
    info = D8.vk.info
    Q = info.num_query_rounds
    one = (1 << info.lde_bits) * ((info.leaf_widths[0] + 4 * (info.lde_bits - info.cap_height)) * 8 + 4)
    lo = (3 * one - 1) >> 20
    assert one <= lo << 20 < 3 * one <= (lo + 1) << 20 and one > 1 << 20
    monkeypatch.setenv("P2V_KNOWN_KEYED_MAX_MB", str(lo + 1 if covered else lo))
    vk = D8.base.with_keys(D8.keys[1:3])
    assert vk.num_keys == 3
    n = N
    bv = p2v.BatchVerifier(vk, 0, n)
    ids = (np.arange(n) % 3).astype(np.uint32)
    rows = np.ascontiguousarray(D8.packed[ids])
    for run in range(2):
        res, tr = bv.run(rows, trace=True, key_ids=ids)
        check(res, tr, D8.st[ids, ids], D8.tr[ids, ids])
        s = vk.known_stats()
        if covered:
            assert (s["hits"], s["misses"]) == (run * n * Q, n * Q) and s["inserted"] > 0
        else:
            assert s == ZERO
    assert sum(vk.known_rows(k) for k in range(3)) == vk.known_stats()["inserted"]
    if not covered:
        zeros = np.zeros(n, dtype=np.uint32)
        res, tr = bv.run(np.ascontiguousarray(D8.packed[zeros]), trace=True)
        check(res, tr, D8.st[zeros, 0], D8.tr[zeros, 0])
        s = vk.known_stats()
        assert (s["hits"], s["misses"]) == (0, n * Q) and s["inserted"] == vk.known_rows(0) > 0


@pytest.mark.parametrize("env", [{"P2V_KNOWN_LEAVES": "2"}, {"P2V_SINGLE_STREAM": "1"},
                                 {"P2V_KNOWN_LEAVES": "2", "P2V_SINGLE_STREAM": "1"}])
def test_gpu_known_keyed_probe_only_and_single_stream(p2v, D, env, monkeypatch):
    """P2V_KNOWN_LEAVES=2 probes but never inserts, so three keyed runs of one batch are all misses
    and every key's rows stay empty; P2V_SINGLE_STREAM=1 runs the table's kernels in line on the
    caller's stream, cold then warm.  The whole (key, proof) matrix rides along."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n = 130
    vk = fresh(D)
    bv = p2v.BatchVerifier(vk, 0, n)
    rows, ids, want_st, want_tr = D.batch(n, seed=10)
    probe_only = env.get("P2V_KNOWN_LEAVES") == "2"
    outs, stats = [], []
    for run in range(3):
        res, tr = bv.run(rows, trace=True, key_ids=ids)
        check(res, tr, want_st, want_tr)
        outs.append((res, tr))
        stats.append(vk.known_stats())
        print(env, run, stats[-1])
        assert stats[-1]["hits"] + stats[-1]["misses"] == (run + 1) * n * D.Q
    if probe_only:
        assert stats[-1] == {"hits": 0, "misses": 3 * n * D.Q, "inserted": 0}
        assert [vk.known_rows(k) for k in range(5)] == [0] * 5
    else:   # rows are inserted by the cold run alone: the same batch again opens nothing new
        assert stats[0]["hits"] == 0 and stats[0]["inserted"] > 0
        assert stats[1]["inserted"] == stats[2]["inserted"] == stats[0]["inserted"]
        assert delta(stats[1], stats[2])["hits"] == delta(stats[0], stats[1])["hits"] > 0
        assert sum(vk.known_rows(k) for k in range(5)) == stats[0]["inserted"]
    for k in env:
        monkeypatch.delenv(k)
    ref, rtr = off(p2v, D, rows, ids, monkeypatch)
    for res, tr in outs:
        assert np.array_equal(res, ref) and np.array_equal(tr, rtr)


def test_gpu_known_keyed_pooled_path(p2v, D):
    """p2v_verify_batch_keyed with 300 proofs, twice: equal to the workspace path, and the handle's
    counters move (the chunks of at least 256 proofs take the table)."""
    vk = fresh(D)
    rows, ids, want_st, _tr = D.batch(300, seed=300)
    got = p2v.verify_batch(vk, rows, key_ids=ids)
    assert np.array_equal(got, want_st)
    s0 = vk.known_stats()
    assert s0["hits"] + s0["misses"] >= 256 * D.Q and s0["inserted"] > 0
    assert np.array_equal(p2v.verify_batch(vk, rows, key_ids=ids), want_st)
    s1 = vk.known_stats()
    assert delta(s0, s1)["hits"] > 0 and delta(s0, s1)["inserted"] == 0
    ws = p2v.BatchVerifier(fresh(D), 0, 300).run(rows, key_ids=ids)
    assert np.array_equal(ws, got)


@pytest.mark.parametrize("table", ["off", "on"])
def test_gpu_known_keyed_flagged_followers(p2v, D, table, monkeypatch):
    """The scenario of tests/test_gpu_keys.py test_gpu_keyed_flagged_followers_row_form: 130 valid
    proofs each under its own key, eight with one follower's top-level sibling bumped (tree 0 in
    four, tree 2 in four).  off (P2V_KNOWN_LEAVES=0): tree 0 goes through plan / chains /
    k_merkle_fix, whose cap comparison reads the lane's key -- the path the default now routes
    around.  on: a cold table, so the same openings come through k_merkle_known_miss's row form
    (3 640 entries, below its switch to the lane form) and the key read once per entry."""
    n = 130
    rows, ids, want_st, want_tr = own_key_batch(D, n)
    rows, want_st, want_tr = rows.copy(), want_st.copy(), want_tr.copy()
    slots = [0, 7, 20, 63, 64, 65, 100, 129]
    for i, slot in enumerate(slots):
        k, tree = int(ids[slot]), (0 if i < 4 else 2)
        qidx = [int(x) for x in D.qidx[k, k]]
        d = json.loads(D.texts[k])
        qr = d["proof"]["opening_proof"]["query_round_proofs"]
        lvl = len(qr[0]["initial_trees_proof"]["evals_proofs"][tree][1]["siblings"]) - 1
        fol = [q for q in range(1, len(qidx)) if any(qidx[h] >> lvl == qidx[q] >> lvl for h in range(q))]
        e = qr[fol[i % len(fol)]]["initial_trees_proof"]["evals_proofs"][tree][1]["siblings"][lvl]["elements"]
        e[i % 4] = (e[i % 4] + 1) % P
        text = json.dumps(d, separators=(",", ":")).encode()
        want_st[slot], want_tr[slot] = _oracle_under(D, k, text)
        rows[slot] = D.vk.pack_many([text])[0]
    assert (want_st[slots] == -1).all() and (np.delete(want_st, slots) == 1).all()
    if table == "off":
        monkeypatch.setenv("P2V_KNOWN_LEAVES", "0")
    vk = fresh(D)
    res, tr = p2v.BatchVerifier(vk, 0, n).run(rows, trace=True, key_ids=ids)
    check(res, tr, want_st, want_tr)
    if table == "off":
        assert vk.known_stats() == ZERO
    else:   # every tree-0 opening but the bumped ones is True, and filed under its proof's key
        assert vk.known_stats() == {"hits": 0, "misses": n * D.Q, "inserted": distinct(D, [(k, k) for k in range(3)])}
        assert [vk.known_rows(k) for k in range(5)] == [distinct(D, [(k, k)]) for k in range(3)] + [0, 0]
