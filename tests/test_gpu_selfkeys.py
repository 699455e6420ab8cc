"""Self-keyed circuits on the GPU (MI355X): a run without key ids on a self-keyed handle resolves
each proof's key on the device from the tail of its public inputs (keys.hip k_key_resolve) and
verifies the proof against it.  Expected ids: the numpy restatement of selfkeys.py; statuses and
traces: the oracle under the expected key.  Integer arithmetic: no tolerance anywhere.  Trace rows
are skipped only for proofs whose expected id is KEY_NONE (their status is ERR_CIRCUIT)."""
import numpy as np
import pytest

from selfkeys import ERR_CIRCUIT, KEY_NONE, data, key_of, synthetic_keys
from support import p2v_module, proof_bytes
from test_keys import family

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def p2v():
    import torch   # before libp2v, as tests/test_gpu.py
    assert torch.cuda.is_available(), "torch sees no GPU"
    m = p2v_module()
    if m.device_count() == 0:
        pytest.fail("no GPU visible to libp2v")
    return m


class Handles:
    def __init__(self, p2v):
        D = data()
        self.base = p2v.VerifierCircuitData.from_json(D.common, D.keys[0])
        self.plain = self.base.with_keys(D.keys[1:])      # the five-key table, unmarked
        self.vk = self.plain.self_keyed()
        assert self.vk.is_self_keyed and self.vk.num_keys == 5 and not self.plain.is_self_keyed
        self.packed = self.vk.pack_many(D.texts)


_handles = []


def handles(p2v) -> Handles:
    if not _handles:
        _handles.append(Handles(p2v))
    return _handles[0]


def check(res, tr, pj):
    """Statuses and traces of batch pj against the oracle under the expected keys."""
    D = data()
    assert np.array_equal(res, D.st[pj]), (res.tolist(), D.st[pj].tolist())
    keep = D.ids[pj] != KEY_NONE
    assert np.array_equal(tr[keep], D.tr[pj][keep])


def device_run(p2v, bv, rows, tiled=False, lookahead=False, stream=0, sync=True, key_ids=None):
    """A device-resident batch, no ids unless given: the tensors of the statuses and traces."""
    import torch
    n = rows.shape[0]
    d_in = torch.from_numpy((p2v.tile_proofs(rows) if tiled else rows).view(np.int64)).cuda()
    d_res = torch.full((n,), 7, dtype=torch.int8, device="cuda")
    d_tr = torch.zeros((n, bv.circuit.info.trace_words), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    bv.run_device(d_in.data_ptr(), n, d_res.data_ptr(), stream=stream, trace_ptr=d_tr.data_ptr(), sync=sync, tiled=tiled,
                  lookahead=lookahead, key_ids=key_ids)
    return d_res, d_tr, d_in


# 3, 64: latency mode; 65: a partial second tile; 130: three waves, a partial last tile
@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("n", [3, 64, 65, 130])
def test_gpu_self_keyed_batch_matrix(p2v, n, tiled, on_device):
    D, H = data(), handles(p2v)
    pj = D.batch(n, seed=n)
    rows = np.ascontiguousarray(H.packed[pj])
    bv = p2v.BatchVerifier(H.vk, 0, n)
    if on_device:
        d_res, d_tr, _keep = device_run(p2v, bv, rows, tiled=tiled)
        res, tr = d_res.cpu().numpy(), d_tr.cpu().numpy().view(np.uint64)
    else:
        res, tr = bv.run(rows, trace=True, tiled=tiled)
    check(res, tr, pj)
    ids = bv.resolve_keys(rows, tiled=tiled)
    assert ids.dtype == np.uint32 and np.array_equal(ids, D.ids[pj]), (ids.tolist(), D.ids[pj].tolist())
    # the same run with the expected ids given: bit-identical, the no-key rows' traces aside
    res2, tr2 = bv.run(rows, trace=True, tiled=tiled, key_ids=D.ids[pj])
    keep = D.ids[pj] != KEY_NONE
    assert np.array_equal(res, res2) and np.array_equal(tr[keep], tr2[keep])


def test_gpu_resolve_keys_device_ids_and_unmarked_handle(p2v):
    """p2v_verifier_resolve_keys with ids in device memory (P2V_FLAG_RESULT_DEVICE), and on an
    unmarked handle: the resolution does not depend on the mark."""
    import ctypes
    import torch
    D, H = data(), handles(p2v)
    n = 130
    pj = D.batch(n, seed=9)
    rows = np.ascontiguousarray(H.packed[pj])
    bv = p2v.BatchVerifier(H.plain, 0, n)
    assert np.array_equal(bv.resolve_keys(rows), D.ids[pj])
    d_in = torch.from_numpy(p2v.tile_proofs(rows).view(np.int64)).cuda()
    d_ids = torch.full((n + 3,), 5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    flags = p2v.FLAG_INPUT_DEVICE | p2v.FLAG_RESULT_DEVICE | p2v.FLAG_INPUT_TILED | p2v.FLAG_NO_SYNC
    rc = p2v.lib().p2v_verifier_resolve_keys(bv._h, ctypes.c_void_p(d_in.data_ptr()), n, ctypes.c_void_p(d_ids.data_ptr()), None, flags)
    assert rc == p2v.E_OK
    torch.cuda.synchronize()
    got = d_ids.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:n], D.ids[pj]) and (got[n:] == 5).all()   # nothing written past n


def test_gpu_self_keyed_probing_4099_keys(p2v):
    """The fixture's five keys, then 4 094 synthetic ones in digest-sharing groups with a duplicate
    of k2 among them: long probe sequences on the device.  k2's proofs get id 1, not the
    duplicate's index, and the statuses are those of the five-key handle."""
    D, H = data(), handles(p2v)
    syn = synthetic_keys(4094, 50, seed=21)
    syn[1000] = key_of(D.keys[1])
    big = H.vk.with_keys(syn)
    assert big.is_self_keyed and big.num_keys == 4099
    n = 130
    pj = D.batch(n, seed=130)
    rows = np.ascontiguousarray(H.packed[pj])
    bv = p2v.BatchVerifier(big, 0, n)
    ids = bv.resolve_keys(rows)
    assert np.array_equal(ids, D.ids[pj]), (ids.tolist(), D.ids[pj].tolist())
    assert big.find_key(syn[1000]) == 1 and big.find_key(syn[4093]) == 5 + 4093
    # proofs naming synthetic keys deep in the table, the last one included
    far = [5, 5 + 49, 5 + 999, 5 + 1001, 5 + 4093]
    frows = np.ascontiguousarray(H.packed[[0] * len(far)])
    npis = big.info.num_public_inputs
    for r, k in zip(frows, far):
        key = syn[k - 5]
        r[npis - 68: npis] = np.concatenate([key[-4:], key[:-4]])   # public inputs lead the packed words
    assert np.array_equal(bv.resolve_keys(frows), np.array(far, dtype=np.uint32))
    res, tr = bv.run(rows, trace=True)
    check(res, tr, pj)


def test_gpu_self_keyed_ingest_paths(p2v):
    """Every ingest path reaches the resolver: binary and JSON proofs packed on the device, the
    pooled host pipeline in chunks, the sharded form, and the Python batch entry."""
    D, H = data(), handles(p2v)
    n = 70
    pj = D.batch(n, seed=70)
    want = D.st[pj]
    texts = [D.texts[j] for j in pj]
    rows = np.ascontiguousarray(H.packed[pj])
    bv = p2v.BatchVerifier(H.vk, 0, n)
    assert np.array_equal(bv.run(rows), want)
    res, codes = bv.run_bytes([proof_bytes(t, pi_prefix=bool(i % 2)) for i, t in enumerate(texts)])
    assert (codes == 0).all() and bv.last_bytes_device == n and np.array_equal(res, want)
    res, codes = bv.run_json(texts)
    assert (codes == 0).all() and bv.last_json_device > 0 and np.array_equal(res, want)
    res, codes, ndev = p2v.verify_batch_bytes(H.vk, [proof_bytes(t) for t in texts], 0, 32)   # three chunks
    assert (codes == 0).all() and ndev == n and np.array_equal(res, want)
    assert np.array_equal(p2v.verify_batch_devices(H.vk, rows, [0, 0], chunk=32), want)        # two shards in chunks
    assert np.array_equal(p2v.verify_batch(H.vk, rows), want)                                 # one chunk
    got = p2v.verify_proof_batch(H.vk, texts)
    assert [1 if g is True else 0 if g is False else g.status for g in got] == want.tolist()
    # the pooled path in more than one chunk at the 256-proof chunk floor
    pj3 = D.batch(300, seed=300)
    assert np.array_equal(p2v.verify_batch(H.vk, np.ascontiguousarray(H.packed[pj3])), D.st[pj3])


def test_gpu_self_keyed_lookahead_two_batches(p2v):
    """P2V_FLAG_LOOKAHEAD: two device-resident batches with different id patterns back to back on
    one workspace without a host sync in between; each run's ids are in the buffer of its parity."""
    import torch
    D, H = data(), handles(p2v)
    b1, b2 = D.batch(65, seed=1), D.batch(65, seed=2)
    assert not np.array_equal(D.ids[b1], D.ids[b2])
    bv = p2v.BatchVerifier(H.vk, 0, 65)
    st = torch.cuda.Stream()
    outs = [device_run(p2v, bv, np.ascontiguousarray(H.packed[b]), tiled=(k == 1), lookahead=True, stream=st.cuda_stream, sync=False)
            for k, b in enumerate((b1, b2))]
    torch.cuda.synchronize()
    for (d_res, d_tr, _keep), b in zip(outs, (b1, b2)):
        check(d_res.cpu().numpy(), d_tr.cpu().numpy().view(np.uint64), b)


def test_gpu_self_keyed_override_one_key_and_short_variant(p2v):
    D, H = data(), handles(p2v)
    n = 70
    pj = D.batch(n, seed=5)
    rows = np.ascontiguousarray(H.packed[pj])
    # explicit ids override the resolution: all ids 0 is the oracle's column for k1
    res, tr = p2v.BatchVerifier(H.vk, 0, n).run(rows, trace=True, key_ids=np.zeros(n, dtype=np.uint32))
    assert np.array_equal(res, D.st_k1[pj]) and np.array_equal(tr, D.tr_k1[pj])
    assert not np.array_equal(D.st_k1[pj], D.st[pj])
    # K = 1: the cyclic check -- every proof must name key 0
    one = H.base.self_keyed()
    assert one.num_keys == 1
    res, tr = p2v.BatchVerifier(one, 0, n).run(rows, trace=True)
    named0 = D.ids[pj] == 0
    assert np.array_equal(res, np.where(named0, D.st[pj], ERR_CIRCUIT))
    assert np.array_equal(tr[named0], D.tr[pj][named0])
    i0, i1 = int(np.flatnonzero(pj == 0)[0]), int(np.flatnonzero(pj == 1)[0])
    assert res[i0] == 1 and res[i1] == ERR_CIRCUIT     # circuit 1's self-naming proof, circuit 2's
    res3, _ = p2v.BatchVerifier(one, 0, 3).run(rows[[i0, i1, i0]], trace=True)   # the latency mode
    assert res3.tolist() == [1, ERR_CIRCUIT, 1]
    # a shape variant with 4 public inputs: shorter than a key, every proof names none
    g4 = family(6, 1, 0)
    sv = H.vk.shape_variant(4, H.vk.info.final_poly_len)
    assert sv.is_self_keyed and sv.info.num_public_inputs == 4
    rows4 = sv.pack_many([g.proof(1, 1) for g in g4] * 24)
    bv4 = p2v.BatchVerifier(sv, 0, len(rows4))
    assert (bv4.run(rows4) == ERR_CIRCUIT).all() and (bv4.run(rows4[:3]) == ERR_CIRCUIT).all()
    assert (bv4.resolve_keys(rows4) == KEY_NONE).all()


def test_gpu_self_keyed_known_openings(p2v):
    """A self-keyed run is a keyed run: on a handle whose known-openings table covers every key it
    fills and probes the per-key rows."""
    D, H = data(), handles(p2v)
    vk = H.base.with_keys(D.keys[1:]).self_keyed()   # a fresh handle: its table starts empty
    n = 130
    pj = D.batch(n, seed=6)
    rows = np.ascontiguousarray(H.packed[pj])
    bv = p2v.BatchVerifier(vk, 0, n)
    first = bv.run(rows, trace=True)
    for k in (0, 1, 2):
        assert vk.known_rows(k) > 0, k
    s1 = vk.known_stats()
    second = bv.run(rows, trace=True)
    s2 = vk.known_stats()
    assert s2["hits"] > s1["hits"]
    check(first[0], first[1], pj)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])


def test_gpu_unmarked_handle_verifies_against_key_0(p2v):
    D, H = data(), handles(p2v)
    n = 70
    pj = D.batch(n, seed=7)
    rows = np.ascontiguousarray(H.packed[pj])
    res, tr = p2v.BatchVerifier(H.plain, 0, n).run(rows, trace=True)
    assert np.array_equal(res, D.st_k1[pj]) and np.array_equal(tr, D.tr_k1[pj])
    d_res, d_tr, _keep = device_run(p2v, p2v.BatchVerifier(H.plain, 0, n), rows, tiled=True)
    assert np.array_equal(d_res.cpu().numpy(), D.st_k1[pj])
    assert np.array_equal(p2v.verify_batch(H.plain, rows), D.st_k1[pj])
