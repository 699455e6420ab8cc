"""Self-keyed circuits, host side (no GPU): the key lookup (p2v_circuit_find_key, whose hash and
probing the device resolver shares), the public-input tail in the key encoding, the self-keyed
mark and what keeps it, and the generator entry that lets a valid proof name a key."""
import ctypes

import numpy as np
import pytest

from selfkeys import (KEY_NONE, NUM_PIS, TAIL, data, expected_ids, family71, key_of, lookup, proof_naming, public_inputs,
                      synthetic_keys, tail_of, tail_to_key)
from support import P, oracle, p2v_module
from test_keys import family, key_table


@pytest.fixture(scope="module")
def p2v():
    return p2v_module()


@pytest.fixture(scope="module")
def base(p2v):
    g = family71()[0]
    return p2v.VerifierCircuitData.from_json(g.common, g.vkey)


def test_find_key_fixture_table_and_duplicates(p2v, base):
    keys = key_table(family71())
    table = np.stack([key_of(k) for k in keys])
    assert base.key_words == TAIL and base.info.num_public_inputs == NUM_PIS
    assert base.find_key(table[0]) == 0 and base.find_key(table[1]) == -1   # a one-key handle
    vk = base.with_keys(keys[1:])
    for k, row in enumerate(table):
        assert vk.find_key(row) == lookup(table, row) == k
        assert np.array_equal(row, vk.vkey_words(keys[k]))                   # the restated encoding is the library's
    off = table[2].copy()
    off[0] = (int(off[0]) + 1) % P
    assert vk.find_key(off) == lookup(table, off) == -1
    # a duplicated key: the lowest index; a key appended after its duplicate keeps its own
    dup = np.stack([table[1], table[3], table[0], table[1], table[2]])
    full = np.concatenate([table[:1], dup])
    vd = base.with_keys(dup)
    for row in full:
        assert vd.find_key(row) == lookup(full, row)
    assert vd.find_key(table[1]) == 1 and vd.find_key(table[0]) == 0 and vd.find_key(table[2]) == 5
    assert p2v.lib().p2v_circuit_find_key(vk.handle, None) == p2v.E_ARG
    assert p2v.lib().p2v_circuit_find_key(None, table[0].ctypes.data) == p2v.E_ARG
    with pytest.raises(p2v.P2VError):
        vk.find_key(table[0][:-1])


def test_find_key_words_plus_p_are_the_same_key(base):
    """Words >= p in the query and in the table (with_keys reduces them) name their residues."""
    small = np.random.default_rng(3).integers(0, 1 << 31, size=(3, TAIL), dtype=np.uint64)
    vk = base.with_keys([small[0], small[1] + np.uint64(P)])
    assert vk.find_key(small[0] + np.uint64(P)) == 1 and vk.find_key(small[0]) == 1
    assert vk.find_key(small[1]) == 2 and vk.find_key(small[1] + np.uint64(P)) == 2
    mixed = small[1].copy()
    mixed[::2] += np.uint64(P)
    assert vk.find_key(mixed) == 2
    assert vk.find_key(small[2]) == -1 and vk.find_key(small[2] + np.uint64(P)) == -1


def test_find_key_5000_keys_sharing_digests(base):
    """Groups of 50 keys share their four digest words (as hybrid keys do): every key is found at
    its own index, and a key with any one word changed is absent."""
    keys = synthetic_keys(5000, 50, seed=11)
    vk = base.with_keys(keys)
    assert vk.num_keys == 5001
    for k, row in enumerate(keys):
        assert vk.find_key(row) == k + 1, k
    rng = np.random.default_rng(12)
    present = {r.tobytes() for r in keys}
    for _ in range(200):
        row = keys[rng.integers(0, len(keys))].copy()
        w = int(rng.integers(0, TAIL))
        row[w] = (int(row[w]) + 1 + int(rng.integers(0, 1000))) % P
        assert row.tobytes() not in present
        assert vk.find_key(row) == -1


def test_key_from_public_inputs(p2v, base):
    D = data()
    for t, want in zip(D.texts, D.ids):
        pis = public_inputs(t)
        assert pis.size == NUM_PIS
        key = base.key_from_public_inputs(pis)
        assert np.array_equal(key, tail_to_key(pis[-TAIL:]))
        got = base.with_keys(D.keys[1:]).find_key(key)
        assert got == (-1 if want == KEY_NONE else int(want))
    pis = public_inputs(D.texts[1])
    assert np.array_equal(base.key_from_public_inputs(pis), key_of(D.keys[1]))          # digest-first tail, cap-first key
    assert np.array_equal(base.key_from_public_inputs(pis[3:]), key_of(D.keys[1]))      # exactly a key long
    assert np.array_equal(base.key_from_public_inputs(np.concatenate([pis, pis])), key_of(D.keys[1]))
    for short in (pis[4:], pis[:0]):                                                    # 67 inputs, none
        with pytest.raises(p2v.P2VError) as e:
            base.key_from_public_inputs(short)
        assert e.value.code == p2v.E_SHAPE
    out = np.zeros(TAIL, dtype=np.uint64)
    assert p2v.lib().p2v_key_from_public_inputs(base.handle, pis.ctypes.data, pis.size, None) == p2v.E_ARG
    assert p2v.lib().p2v_key_from_public_inputs(None, pis.ctypes.data, pis.size, out.ctypes.data) == p2v.E_ARG


def test_self_keyed_mark(p2v, base):
    keys = key_table(family71())
    assert not base.is_self_keyed
    sk = base.self_keyed()
    assert sk is not base and sk.is_self_keyed and not base.is_self_keyed
    assert sk.num_keys == 1 and sk.info == base.info
    kt = base.with_keys(keys[1:])
    assert not kt.is_self_keyed and kt.self_keyed().num_keys == 5                       # marking keeps the table
    skt = sk.with_keys(keys[1:])
    assert skt.is_self_keyed and skt.num_keys == 5                                      # with_keys keeps the mark
    for npis in (NUM_PIS + 2, TAIL, TAIL - 1, 4):                                       # shape variants too, short ones included
        sv = skt.shape_variant(npis, base.info.final_poly_len)
        assert sv.is_self_keyed and sv.num_keys == 5 and sv.info.num_public_inputs == npis
        assert not kt.shape_variant(npis, base.info.final_poly_len).is_self_keyed
    ext = p2v.VerifierCircuitData.from_json(family71()[0].common, keys[0], ext=p2v.EXT_HASH_OR_NOOP)
    assert ext.self_keyed().info.ext == p2v.EXT_HASH_OR_NOOP
    g4 = family(6, 1, 0)[0]                                                             # 4 public inputs
    vk4 = p2v.VerifierCircuitData.from_json(g4.common, g4.vkey)
    with pytest.raises(p2v.P2VError) as e:
        vk4.self_keyed()
    assert e.value.code == p2v.E_CIRCUIT
    assert not vk4.is_self_keyed
    h = ctypes.c_void_p()
    assert p2v.lib().p2v_circuit_self_keyed(None, ctypes.byref(h)) == p2v.E_ARG
    assert p2v.lib().p2v_circuit_is_self_keyed(None) == p2v.E_ARG
    assert p2v.KEY_NONE == KEY_NONE


def test_generator_tail_entry():
    O = oracle()
    gcs = family71()
    assert proof_naming(gcs[0], np.zeros(0, np.uint64)) == gcs[0].proof(1, 1)           # ntail = 0: the same bytes
    D = data()
    table = np.stack([key_of(k) for k in D.keys])
    for i, g in enumerate(gcs):                                                         # valid proofs that name their own key
        assert np.array_equal(public_inputs(D.texts[i])[-TAIL:], tail_of(g.vkey))
        assert O.verify_json(g.common, g.vkey, D.texts[i]) == 1
    assert expected_ids(D.texts[:3], table).tolist() == [0, 1, 2]
    assert O.verify_json(D.common, D.keys[0], D.texts[3]) == 1                          # circuit 1's naming k2: valid under k1,
    assert O.verify_json(D.common, D.keys[1], D.texts[3]) == 0                          # rejected under the key it names
    # the leading inputs and everything else the witness draws are those of the untouched witness
    assert np.array_equal(public_inputs(D.texts[0])[:3], public_inputs(gcs[0].proof(1, 1))[:3])
    g0 = family(6, 0, 0)[0]                                                             # mode 0 is not a real circuit
    with pytest.raises(RuntimeError):
        proof_naming(g0, np.zeros(4, np.uint64))
