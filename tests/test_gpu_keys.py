"""Keyed verification on the GPU (MI355X): one launch, proof i against key key_ids[i] of the
circuit's key table (p2v_verifier_run_keyed / p2v_verify_batch_keyed), held bit for bit against
the oracle run once per (key, proof) pair.  Integer arithmetic: no tolerance anywhere."""
import os

import numpy as np
import pytest

from support import oracle, p2v_module
from test_keys import family, key_table

pytestmark = pytest.mark.gpu

ERR_CIRCUIT = -6


@pytest.fixture(scope="module")
def p2v():
    import torch   # before libp2v, as tests/test_gpu.py
    assert torch.cuda.is_available(), "torch sees no GPU"
    m = p2v_module()
    if m.device_count() == 0:
        pytest.fail("no GPU visible to libp2v")
    return m


class Data:
    """One circuit family: the key table [k1, k2, k3, hybrid(cap1, dig2), hybrid(cap2, dig1)], the
    proofs (the three valid ones, then one generator-corrupted proof of circuit 1 per reject class
    the generator has a flag for), and the oracle's status and trace of every (key, proof) pair."""

    def __init__(self, p2v, nb, mode, lk):
        O = oracle()
        gcs = family(nb, mode, lk)
        self.gcs = gcs
        self.common = gcs[0].common
        self.keys = key_table(gcs)
        self.texts = [g.proof(1, 1) for g in gcs] + [gcs[0].proof(1, 10 + f, flags=f) for f in (1, 2, 4)]
        self.base = p2v.VerifierCircuitData.from_json(self.common, self.keys[0])
        self.vk = self.base.with_keys(self.keys[1:])
        assert self.vk.num_keys == len(self.keys)
        self.packed = self.vk.pack_many(self.texts)
        nk, npr = len(self.keys), len(self.texts)
        self.st = np.zeros((nk, npr), dtype=np.int8)
        self.tr = np.zeros((nk, npr, self.vk.info.trace_words), dtype=np.uint64)
        for k, key in enumerate(self.keys):
            c = O.circuit(self.common, key)
            for j, t in enumerate(self.texts):
                pr = O.proof(t)
                self.st[k, j], self.tr[k, j] = O.verify(c, pr, trace=True)
                O.L.or_proof_free(pr)
            O.L.or_circuit_free(c)
        # the shape the assertions below rely on
        assert [int(self.st[k, k]) for k in range(3)] == [1, 1, 1]
        assert all(self.st[a, b] == 0 for a in range(3) for b in range(3) if a != b)
        assert (self.st[3, 0], self.st[3, 1], self.st[4, 0], self.st[4, 1]) == (0, -1, -1, 0)
        self.corrupt = sorted({int(self.st[0, j]) for j in range(3, npr)})   # the reject classes under their own key
        assert -3 in self.corrupt and 0 in self.corrupt

    def batch(self, n, seed):
        """n (key, proof) pairs in a seeded shuffle: every pair of the matrix in turn, so each of
        the 5 keys, the statuses 1 / 0 / -1 among the valid proofs and every corrupted proof's
        class under its own key are present (asserted) from n = 3 * 5 on; below that the pairs
        that carry them come first."""
        nk, npr = self.st.shape
        lead = [(0, 0), (3, 1), (1, 0), (2, 2), (4, 1), (0, 3), (0, 4), (0, 5)]
        rest = [(k, j) for k in range(nk) for j in range(npr) if (k, j) not in lead]
        rng = np.random.default_rng(seed)
        rest = [rest[i] for i in rng.permutation(len(rest))]
        pairs = (lead + rest) * (n // (nk * npr) + 1)
        pairs = [pairs[i] for i in rng.permutation(n)] if n >= len(lead) else pairs[:n]
        ids = np.array([k for k, _ in pairs], dtype=np.uint32)
        pj = np.array([j for _, j in pairs])
        want_st, want_tr = self.st[ids, pj], self.tr[ids, pj]
        if n >= len(lead):
            assert set(ids.tolist()) == set(range(nk))
            valid = want_st[pj < 3]
            assert {1, 0, -1} <= set(valid.tolist())
            assert set(self.corrupt) <= set(want_st[(pj >= 3) & (ids == 0)].tolist())
        else:
            assert {1, -1} <= set(want_st.tolist()) and len(set(ids.tolist())) == n
        return np.ascontiguousarray(self.packed[pj]), ids, want_st, want_tr


_data = {}


def data(p2v, nb=6, mode=1, lk=0) -> Data:
    if (nb, mode, lk) not in _data:
        _data[(nb, mode, lk)] = Data(p2v, nb, mode, lk)
    return _data[(nb, mode, lk)]


def device_batch(p2v, vk, rows, ids, tiled=False):
    """The batch, its ids and result buffers in device memory, complete (synchronised)."""
    import torch
    n = rows.shape[0]
    d_in = torch.from_numpy((p2v.tile_proofs(rows) if tiled else rows).view(np.int64)).cuda()
    d_ids = torch.from_numpy(ids.view(np.int32).copy()).cuda()
    d_res = torch.full((n,), 7, dtype=torch.int8, device="cuda")
    d_tr = torch.zeros((n, vk.info.trace_words), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return d_in, d_ids, d_res, d_tr


def run_device_ids(p2v, bv, rows, ids, tiled=False, lookahead=False, stream=0, sync=True, bufs=None):
    """A device-resident batch with device ids (P2V_FLAG_INPUT_DEVICE): statuses and traces."""
    d_in, d_ids, d_res, d_tr = bufs or device_batch(p2v, bv.circuit, rows, ids, tiled)
    bv.run_device(d_in.data_ptr(), rows.shape[0], d_res.data_ptr(), stream=stream, trace_ptr=d_tr.data_ptr(), sync=sync,
                  tiled=tiled, lookahead=lookahead, key_ids=d_ids.data_ptr())
    return d_res, d_tr, (d_in, d_ids)


def check(res, tr, want_st, want_tr, skip=()):
    assert np.array_equal(res, want_st), (res.tolist(), want_st.tolist())
    keep = np.array([i not in skip for i in range(len(res))])
    assert np.array_equal(tr[keep], want_tr[keep])


# 3, 64: latency mode (k_merkle_row); 65, 130: the throughput kernels, a partial last tile, two and three waves
@pytest.mark.parametrize("device_ids", [False, True])
@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("n", [3, 64, 65, 130])
def test_gpu_keyed_batch_matches_oracle_matrix(p2v, n, tiled, device_ids):
    D = data(p2v)
    rows, ids, want_st, want_tr = D.batch(n, seed=n)
    bv = p2v.BatchVerifier(D.vk, 0, n)
    if device_ids:
        d_res, d_tr, _keep = run_device_ids(p2v, bv, rows, ids, tiled=tiled)
        res, tr = d_res.cpu().numpy(), d_tr.cpu().numpy().view(np.uint64)
    else:
        res, tr = bv.run(rows, trace=True, tiled=tiled, key_ids=ids)
    check(res, tr, want_st, want_tr)


def test_gpu_keyed_lookup_circuit(p2v):
    """The further case: mode 1 with lookups at degree_bits 8."""
    D = data(p2v, 8, 1, 1)
    rows, ids, want_st, want_tr = D.batch(65, seed=8)
    res, tr = p2v.BatchVerifier(D.vk, 0, 65).run(rows, trace=True, key_ids=ids)
    check(res, tr, want_st, want_tr)


def _with_env(name, value, fn):
    """The switches are read at verifier creation (as tests/test_gpu.py sets them)."""
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


# P2V_TRANSCRIPT modes 1..3 by their names, and the plain one-path-per-lane k_merkle
@pytest.mark.parametrize("name,value", [("P2V_TRANSCRIPT", "row"), ("P2V_TRANSCRIPT", "quad"), ("P2V_TRANSCRIPT", "lane"),
                                        ("P2V_MERKLE_CSE", "0")])
def test_gpu_keyed_forced_variants(p2v, name, value):
    D = data(p2v)
    rows, ids, want_st, want_tr = D.batch(130, seed=130)

    def go():
        bv = p2v.BatchVerifier(D.vk, 0, 130)
        host = bv.run(rows, trace=True, tiled=True, key_ids=ids)
        d_res, d_tr, _keep = run_device_ids(p2v, bv, rows, ids)
        return host, (d_res.cpu().numpy(), d_tr.cpu().numpy().view(np.uint64))
    for res, tr in _with_env(name, value, go):
        check(res, tr, want_st, want_tr)


def test_gpu_keyed_flagged_followers_row_form(p2v):
    """Flagged followers of a keyed run through the short-list row form of k_merkle_fix
    (csrc/merkle.hip): tree 0's cap entry is then read from each lane's own key.  130 valid proofs,
    each under its own key (above the latency mode; a keyed run keeps no known openings, so tree 0
    goes through plan / chains / fix); eight of them carry one follower's top-level sibling bumped,
    which only check (C) sees (as tests/test_gpu.py test_gpu_merkle_fix_list_full_batch_of_garbage),
    in tree 0 (four proofs) and tree 2 (four).  Eight list entries are far below the switch to the
    lane form.  Statuses and traces equal the oracle's, with shared-node paths and without."""
    import json
    from support import P, trace_offsets
    O = oracle()
    D = data(p2v)
    info = D.vk.info
    off = trace_offsets(info.num_challenges, info.num_fri_steps, info.num_query_rounds)["query_idx"]
    n = 130
    ids = np.array([i % 3 for i in range(n)], dtype=np.uint32)
    rows = np.ascontiguousarray(D.packed[ids])   # proof k is the valid proof of circuit k
    want_st, want_tr = D.st[ids, ids].copy(), D.tr[ids, ids].copy()
    assert (want_st == 1).all()
    slots = [0, 7, 20, 63, 64, 65, 100, 129]   # both sides of a tile edge, the last (partial) tile
    for i, slot in enumerate(slots):
        k, tree = int(ids[slot]), (0 if i < 4 else 2)
        qidx = [int(x) for x in D.tr[k, k][off: off + info.num_query_rounds]]
        d = json.loads(D.texts[k])
        qr = d["proof"]["opening_proof"]["query_round_proofs"]
        lvl = len(qr[0]["initial_trees_proof"]["evals_proofs"][tree][1]["siblings"]) - 1
        # followers whose node at the top level is a lower query's too: they meet their owner below it
        fol = [q for q in range(1, len(qidx)) if any(qidx[h] >> lvl == qidx[q] >> lvl for h in range(q))]
        e = qr[fol[i % len(fol)]]["initial_trees_proof"]["evals_proofs"][tree][1]["siblings"][lvl]["elements"]
        e[i % 4] = (e[i % 4] + 1) % P
        text = json.dumps(d, separators=(",", ":")).encode()
        c, pr = O.circuit(D.common, D.keys[k]), O.proof(text)
        want_st[slot], want_tr[slot] = O.verify(c, pr, trace=True)
        O.L.or_proof_free(pr)
        O.L.or_circuit_free(c)
        rows[slot] = D.vk.pack_many([text])[0]
    assert (want_st[slots] == -1).all() and (np.delete(want_st, slots) == 1).all()
    for cse in ("1", "0"):
        res, tr = _with_env("P2V_MERKLE_CSE", cse, lambda: p2v.BatchVerifier(D.vk, 0, n).run(rows, trace=True, key_ids=ids))
        check(res, tr, want_st, want_tr)


@pytest.mark.parametrize("form", [None, "lane"])
def test_gpu_keyed_lookahead_two_batches(p2v, form):
    """P2V_FLAG_LOOKAHEAD (k_transcript* on the transcript stream): two batches back to back on one
    workspace without a host sync in between, with different id arrays."""
    import torch
    D = data(p2v)
    b1, b2 = D.batch(130, seed=1), D.batch(130, seed=2)
    assert not np.array_equal(b1[1], b2[1])

    def go():
        bv = p2v.BatchVerifier(D.vk, 0, 130)
        st = torch.cuda.Stream()
        bufs = [device_batch(p2v, D.vk, b[0], b[1], tiled=(k == 1)) for k, b in enumerate((b1, b2))]
        outs = [run_device_ids(p2v, bv, b[0], b[1], tiled=(k == 1), lookahead=True, stream=st.cuda_stream, sync=False, bufs=bufs[k])
                for k, b in enumerate((b1, b2))]
        torch.cuda.synchronize()
        return [(o[0].cpu().numpy(), o[1].cpu().numpy().view(np.uint64)) for o in outs]
    got = _with_env("P2V_TRANSCRIPT", form, go) if form else go()
    for (res, tr), b in zip(got, (b1, b2)):
        check(res, tr, b[2], b[3])


def test_gpu_keyed_equals_unkeyed_path(p2v):
    D = data(p2v)
    n = 130
    rows, _ids, _st, _tr = D.batch(n, seed=5)
    on_base = p2v.BatchVerifier(D.base, 0, n).run(rows, trace=True)
    bv = p2v.BatchVerifier(D.vk, 0, n)
    none = bv.run(rows, trace=True, key_ids=None)
    zero = bv.run(rows, trace=True, key_ids=np.zeros(n, dtype=np.uint32))
    for got in (none, zero):
        assert np.array_equal(got[0], on_base[0]) and np.array_equal(got[1], on_base[1])
    assert {1, 0, -3} <= set(on_base[0].tolist())
    for j, key in enumerate(D.keys):   # all ids j == an unkeyed run on the circuit built from vkey j
        alone = p2v.VerifierCircuitData.from_json(D.common, key)
        want = p2v.BatchVerifier(alone, 0, n).run(rows, trace=True)
        got = bv.run(rows, trace=True, key_ids=np.full(n, j, dtype=np.uint32))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), j


@pytest.mark.parametrize("n", [5, 70])
def test_gpu_keyed_out_of_range_ids(p2v, n):
    """An id >= num_keys: P2V_ERR_CIRCUIT for that proof (its trace row unspecified), the others
    as the oracle says; host and device ids alike.  n = 70: the throughput kernels."""
    D = data(p2v)
    nk = D.vk.num_keys
    ids = np.array(([0, 1, nk, 2 ** 32 - 1, 2] * (n // 5 + 1))[:n], dtype=np.uint32)
    pj = np.arange(n) % 3
    rows = np.ascontiguousarray(D.packed[pj])
    bad = ids >= nk
    safe = np.where(bad, 0, ids)
    want_st = np.where(bad, ERR_CIRCUIT, D.st[safe, pj]).astype(np.int8)
    want_tr = D.tr[safe, pj]
    assert bad[2] and bad[3] and not bad[[0, 1, 4]].any()
    bv = p2v.BatchVerifier(D.vk, 0, n)
    res, tr = bv.run(rows, trace=True, key_ids=ids)
    check(res, tr, want_st, want_tr, skip=set(np.flatnonzero(bad).tolist()))
    d_res, d_tr, _keep = run_device_ids(p2v, bv, rows, ids)
    check(d_res.cpu().numpy(), d_tr.cpu().numpy().view(np.uint64), want_st, want_tr, skip=set(np.flatnonzero(bad).tolist()))


def test_gpu_keyed_raw_words_reduce_mod_p(p2v):
    """Key words >= p given to with_keys are the same key as their residues."""
    from support import P
    D = data(p2v)
    k = D.base.vkey_words(D.keys[1])
    a, b, c = k.copy(), k.copy(), k.copy()
    a[0], a[-1] = 5, 9                      # a cap word and a digest word
    b[0], b[-1] = 5 + P, 9 + P
    c[0], c[-1] = 6, 10
    vk = D.base.with_keys([a, b, c])
    rows = np.ascontiguousarray(D.packed[[1, 1, 1]])
    res, tr = p2v.BatchVerifier(vk, 0, 3).run(rows, trace=True, key_ids=np.array([1, 2, 3], dtype=np.uint32))
    assert np.array_equal(tr[0], tr[1]) and res[0] == res[1]
    assert not np.array_equal(tr[0], tr[2])


def test_gpu_keyed_pooled_path(p2v):
    """p2v_verify_batch_keyed: 300 proofs are more than one chunk at the 256-proof chunk floor (the
    id slices travel with the chunks); equal to the workspace path, and again from the pool."""
    D = data(p2v)
    rows, ids, want_st, _tr = D.batch(300, seed=300)
    ws = p2v.BatchVerifier(D.vk, 0, 300).run(rows, key_ids=ids)
    assert np.array_equal(ws, want_st)
    for _ in range(2):
        assert np.array_equal(p2v.verify_batch(D.vk, rows, key_ids=ids), ws)
    small = p2v.verify_batch(D.vk, rows[:40], key_ids=ids[:40])   # one latency-mode launch, host ids
    assert np.array_equal(small, ws[:40])
    unkeyed = p2v.verify_batch(D.vk, rows)                        # key_ids=None: p2v_verify_batch
    assert np.array_equal(unkeyed, p2v.verify_batch(D.base, rows))
    assert not np.array_equal(unkeyed, ws)
