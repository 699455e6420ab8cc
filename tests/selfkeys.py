"""Self-keyed circuits (include/p2v.h "self-keyed circuits"): the test data of test_selfkeys.py
(host) and test_gpu_selfkeys.py (MI355X).  A family of generator circuits whose proofs end their
public inputs with a VerifierOnlyCircuitData, the restatement of which key such a tail names --
written from the public-input layout, with numpy on the JSON texts, not through the library --
and the oracle's verdict for every proof under the key it names."""
import ctypes
import json

import numpy as np

from support import P, gen_circuit, generator, oracle
from test_keys import SEEDS, key_table

KEY_NONE = 0xFFFFFFFF
ERR_CIRCUIT = -6
CAP_LEN = 16                      # the generator's cap_height is 4
TAIL = 4 + 4 * CAP_LEN            # circuit_digest, then the cap
NUM_PIS = TAIL + 3                # three free leading inputs: the tail is a proper suffix


def family71(seeds=SEEDS):
    """test_keys.family (degree_bits 6, mode 1, 28 queries) with 71 public inputs."""
    gcs = [gen_circuit(6, NUM_PIS, 0, s, 28, 16, 0, 1) for s in seeds]
    assert all(g.common == gcs[0].common for g in gcs), "seeds give different common data"
    assert len({g.vkey for g in gcs}) == len(gcs), "seeds give equal verifier keys"
    return gcs


def _elements(vkey: bytes):
    d = json.loads(vkey)
    cap = [int(x) for h in d["constants_sigmas_cap"] for x in h["elements"]]
    dig = [int(x) for x in d["circuit_digest"]["elements"]]
    assert len(cap) == 4 * CAP_LEN and len(dig) == 4
    return cap, dig


def tail_of(vkey: bytes) -> np.ndarray:
    """The public-input tail that names this key: circuit_digest first, then the cap."""
    cap, dig = _elements(vkey)
    return np.array(dig + cap, dtype=np.uint64)


def key_of(vkey: bytes) -> np.ndarray:
    """The key encoding: the cap first, then circuit_digest."""
    cap, dig = _elements(vkey)
    return np.array(cap + dig, dtype=np.uint64)


def tail_to_key(tail: np.ndarray) -> np.ndarray:
    return np.concatenate([tail[4:], tail[:4]])


def public_inputs(proof: bytes) -> np.ndarray:
    return np.array([int(x) % P for x in json.loads(proof)["public_inputs"]], dtype=np.uint64)


def lookup(table: np.ndarray, key: np.ndarray) -> int:
    """The lowest index of `key` among the rows of `table` ([K, words], canonical), or -1."""
    hit = np.flatnonzero((table == key[None, :]).all(axis=1))
    return int(hit[0]) if hit.size else -1


def expected_ids(texts, table: np.ndarray) -> np.ndarray:
    """Per proof JSON the index of the key (rows of `table`, key encoding) its public inputs end
    with, KEY_NONE where they name none or are shorter than a key."""
    ids = np.full(len(texts), KEY_NONE, dtype=np.uint32)
    for i, t in enumerate(texts):
        pis = public_inputs(t)
        if pis.size >= table.shape[1]:
            k = lookup(table, tail_to_key(pis[pis.size - table.shape[1]:]))
            if k >= 0:
                ids[i] = k
    return ids


def synthetic_keys(n: int, group: int, seed: int, words: int = TAIL) -> np.ndarray:
    """n distinct canonical keys in groups of `group` that share their four digest words."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, P, size=(n, words), dtype=np.uint64)
    for g in range(0, n, group):
        keys[g:g + group, -4:] = keys[g, -4:]
    assert len({k.tobytes() for k in keys}) == n
    return keys


# ----------------------------------------------------------------------------- generator
def _gen_lib():
    L = generator().L
    L.p2v_gen_witness_new_pis.restype = ctypes.c_void_p
    L.p2v_gen_witness_new_pis.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int]
    return L


def proof_naming(gc, tail, wseed=1, pseed=1, flags=0) -> bytes:
    """A proof of generator circuit gc whose last len(tail) public inputs are `tail`
    (p2v_gen_witness_new_pis; an empty tail: p2v_gen_witness_new's witness)."""
    L = _gen_lib()
    t = np.ascontiguousarray(tail, dtype=np.uint64)
    cache = gc.__dict__.setdefault("_wit_pis", {})
    wkey = (wseed, t.tobytes())
    if wkey not in cache:
        w = L.p2v_gen_witness_new_pis(gc.h, wseed, t.ctypes.data if t.size else None, t.size)
        if not w:
            raise RuntimeError(L.p2v_gen_last_error().decode())
        cache[wkey] = w
    ptr = L.p2v_gen_proof_json_flags(gc.h, cache[wkey], pseed, flags)
    if not ptr:
        raise RuntimeError(L.p2v_gen_last_error().decode())
    s = ctypes.string_at(ptr)
    L.p2v_gen_free_str(ptr)
    return s


# ----------------------------------------------------------------------------- fixture
class Data:
    """The key table [k1, k2, k3, hybrid(cap1, dig2), hybrid(cap2, dig1)] over the 71-input family
    and the proofs:
      0-2   the valid proof of each circuit, naming its own key
      3     circuit 1's naming k2 (valid under k1; id 1, under which the oracle rejects it)
      4     circuit 1's naming hybrid(cap1, dig2) (id 3)
      5     circuit 1's with a random tail (no key)
      6     circuit 1's whose tail differs from k1's in the last cap word only (no key)
      7-9   circuit 1's generator-corrupted proofs (flags 1, 2, 4) naming k1
      10    circuit 1's naming hybrid(cap2, dig1) (id 4: the right digest over a wrong cap, -1)
    with the expected ids (expected_ids above) and the oracle's status and trace of each proof
    under the key it names (no key: ERR_CIRCUIT, the trace row unspecified) and under k1."""

    def __init__(self):
        O = oracle()
        self.gcs = gcs = family71()
        self.common = gcs[0].common
        self.keys = key_table(gcs)
        self.table = np.stack([key_of(k) for k in self.keys])
        tails = [tail_of(k) for k in self.keys]
        rnd = np.random.default_rng(7).integers(0, P, size=TAIL, dtype=np.uint64)
        near = tails[0].copy()
        near[-1] = (int(near[-1]) + 1) % P
        g1 = gcs[0]
        self.texts = ([proof_naming(g, tails[i]) for i, g in enumerate(gcs)]
                      + [proof_naming(g1, tails[1]), proof_naming(g1, tails[3]), proof_naming(g1, rnd), proof_naming(g1, near)]
                      + [proof_naming(g1, tails[0], pseed=10 + f, flags=f) for f in (1, 2, 4)]
                      + [proof_naming(g1, tails[4])])
        self.ids = expected_ids(self.texts, self.table)
        assert self.ids.tolist() == [0, 1, 2, 1, 3, KEY_NONE, KEY_NONE, 0, 0, 0, 4]
        npr = len(self.texts)
        circ = [O.circuit(self.common, k) for k in self.keys]
        tw = O.L.or_trace_words(circ[0])
        self.st = np.full(npr, ERR_CIRCUIT, dtype=np.int8)      # under the named key
        self.tr = np.zeros((npr, tw), dtype=np.uint64)
        self.st_k1 = np.zeros(npr, dtype=np.int8)               # every proof under k1 (an unmarked handle, ids all 0)
        self.tr_k1 = np.zeros((npr, tw), dtype=np.uint64)
        for j, t in enumerate(self.texts):
            pr = O.proof(t)
            if self.ids[j] != KEY_NONE:
                self.st[j], self.tr[j] = O.verify(circ[int(self.ids[j])], pr, trace=True)
            self.st_k1[j], self.tr_k1[j] = O.verify(circ[0], pr, trace=True)
            O.L.or_proof_free(pr)
        for c in circ:
            O.L.or_circuit_free(c)

    def batch(self, n, seed):
        """n proof indices: the proofs in turn (a lead order that puts ids 0, 1, 4 and statuses
        1, 0, -1 first), shuffled from n = 15 on.  Every batch of n >= 15 holds each of the five
        ids, the statuses 1, 0, -1, -3 and -6, and at most n / 4 proofs that name no key."""
        lead = [0, 3, 10, 1, 2, 4, 7, 5, 8, 9, 6]
        pj = np.array((lead * (n // len(lead) + 1))[:n])
        if n >= 15:
            pj = pj[np.random.default_rng(seed).permutation(n)]
            assert set(range(5)) <= set(self.ids[pj].tolist())
            assert {1, 0, -1, -3, ERR_CIRCUIT} <= set(self.st[pj].tolist())
            assert 0 < int((self.ids[pj] == KEY_NONE).sum()) <= n // 4
        return pj


_data = []


def data() -> Data:
    if not _data:
        _data.append(Data())
    return _data[0]
