"""Key tables (include/p2v.h "key tables"): many VerifierOnlyCircuitData over one
CommonCircuitData.  Host side only (no GPU): the key encoding, the derived circuits, and the
test data the GPU suite (test_gpu_keys.py) relies on -- generator circuits that differ in their
verifier key alone, and the oracle's verdict for every (key, proof) pair."""
import ctypes
import json

import numpy as np
import pytest

from support import P, gen_circuit, oracle, p2v_module

SEEDS = (1, 2, 3)
# (degree_bits, mode, lookups) of the circuit families whose seeds share their common data
FAMILIES = [(6, 0, 0), (6, 1, 0), (6, 2, 0), (8, 1, 1)]


def family(degree_bits=6, mode=1, lookups=0, seeds=SEEDS):
    """The generator's circuits of these seeds; asserts what every keyed test relies on: their
    CommonCircuitData texts are byte-identical and their verifier keys pairwise distinct."""
    gcs = [gen_circuit(degree_bits, 4, lookups, s, 28, 16, 0, mode) for s in seeds]
    assert all(g.common == gcs[0].common for g in gcs), "seeds give different common data"
    assert len({g.vkey for g in gcs}) == len(gcs), "seeds give equal verifier keys"
    return gcs


def hybrid_vkey(cap_of: bytes, digest_of: bytes) -> bytes:
    """A VerifierOnlyCircuitData with one key's constants_sigmas_cap and another's circuit_digest."""
    a, b = json.loads(cap_of), json.loads(digest_of)
    return json.dumps({"constants_sigmas_cap": a["constants_sigmas_cap"], "circuit_digest": b["circuit_digest"]},
                      separators=(",", ":")).encode()


def key_table(gcs):
    """[k1, k2, k3, hybrid(cap1, dig2), hybrid(cap2, dig1)] as vkey JSON texts."""
    return [g.vkey for g in gcs] + [hybrid_vkey(gcs[0].vkey, gcs[1].vkey), hybrid_vkey(gcs[1].vkey, gcs[0].vkey)]


@pytest.fixture(scope="module")
def p2v():
    return p2v_module()


@pytest.mark.parametrize("nb,mode,lk", FAMILIES)
def test_seeds_share_common_data_and_differ_in_key(nb, mode, lk):
    gcs = family(nb, mode, lk)
    caps = [json.dumps(json.loads(g.vkey)["constants_sigmas_cap"]) for g in gcs]
    digs = [json.dumps(json.loads(g.vkey)["circuit_digest"]) for g in gcs]
    assert len(set(caps)) == len(gcs) and len(set(digs)) == len(gcs)   # both halves of the key differ


def test_oracle_verdict_matrix_and_hybrid_keys():
    """Proof b under key a: accepted on the diagonal; elsewhere the wrong digest changes every
    challenge, so the Plonk identity fails first (REJECT).  The hybrid keys isolate the two places
    a key enters: a right digest with a wrong cap fails the constants/sigmas Merkle proof (-1)."""
    O = oracle()
    gcs = family(6, 1, 0)
    proofs = [g.proof(1, 1) for g in gcs]
    for a, ga in enumerate(gcs):
        for b, pr in enumerate(proofs):
            assert O.verify_json(ga.common, ga.vkey, pr) == (1 if a == b else 0), (a, b)
    keys = key_table(gcs)
    assert O.verify_json(gcs[0].common, keys[3], proofs[0]) == 0    # cap 1 + digest 2
    assert O.verify_json(gcs[0].common, keys[3], proofs[1]) == -1
    assert O.verify_json(gcs[0].common, keys[4], proofs[0]) == -1   # cap 2 + digest 1
    assert O.verify_json(gcs[0].common, keys[4], proofs[1]) == 0


@pytest.mark.parametrize("nb,mode,lk", [(6, 1, 0), (8, 1, 1)])
def test_vkey_words_are_the_tail_of_circuit_words(p2v, nb, mode, lk):
    gcs = family(nb, mode, lk)
    vk = p2v.VerifierCircuitData.from_json(gcs[0].common, gcs[0].vkey)
    assert vk.key_words == 4 * (1 << vk.info.cap_height) + 4
    for g in gcs:
        w = vk.vkey_words(g.vkey)
        assert w.dtype == np.uint64 and w.size == vk.key_words
        assert np.array_equal(w, p2v.circuit_words(g.common, g.vkey)[-vk.key_words:])


def _vkey_rc(p2v, vk, text: bytes):
    out = np.zeros(vk.key_words + 8, dtype=np.uint64)
    return p2v.lib().p2v_vkey_from_json(vk.handle, text, len(text), out.ctypes.data), out


def test_vkey_from_json_errors(p2v):
    gc = family(6, 1, 0)[0]
    vk = p2v.VerifierCircuitData.from_json(gc.common, gc.vkey)
    d = json.loads(gc.vkey)
    for cap in (d["constants_sigmas_cap"][:-1], d["constants_sigmas_cap"] + d["constants_sigmas_cap"][:1], []):
        bad = json.dumps({"constants_sigmas_cap": cap, "circuit_digest": d["circuit_digest"]}).encode()
        rc, _ = _vkey_rc(p2v, vk, bad)
        assert rc == p2v.E_CIRCUIT
        msg = p2v.lib().p2v_last_error_message().decode()
        assert msg == "validateMerkleCapLength: constants_sigmas_cap has wrong size"
        with pytest.raises(p2v.P2VError) as e:   # the constructors' check and message
            p2v.VerifierCircuitData.from_json(gc.common, bad)
        assert e.value.code == p2v.E_CIRCUIT and e.value.message == msg
    for cut in (1, len(gc.vkey) // 2, len(gc.vkey) - 1):
        assert _vkey_rc(p2v, vk, gc.vkey[:cut])[0] == p2v.E_PARSE
    assert _vkey_rc(p2v, vk, b'{"constants_sigmas_cap":[]}')[0] == p2v.E_PARSE          # no circuit_digest
    three = json.dumps({"constants_sigmas_cap": d["constants_sigmas_cap"],
                        "circuit_digest": {"elements": d["circuit_digest"]["elements"][:3]}}).encode()
    assert _vkey_rc(p2v, vk, three)[0] == p2v.E_PARSE
    assert p2v.lib().p2v_vkey_from_json(vk.handle, gc.vkey, len(gc.vkey), None) == p2v.E_ARG


def test_vkey_values_reduce_mod_p_as_the_constructor_does(p2v):
    """Elements >= p and negative ones: the key encoding holds what the circuit constructor reads
    (aeson's Integer through Goldilocks.hs:98-102).  (Raw words >= p given to with_keys: on the
    GPU, test_gpu_keys.py.)"""
    gc = family(6, 1, 0)[0]
    vk = p2v.VerifierCircuitData.from_json(gc.common, gc.vkey)
    d = json.loads(gc.vkey)
    canon = vk.vkey_words(gc.vkey)
    assert (canon < np.uint64(P)).all()
    shifts = [P, -P, 2 * P, -3 * P]   # each element moved by a multiple of p: above p, above 2^64, negative
    k = 0
    for dg in d["constants_sigmas_cap"] + [d["circuit_digest"]]:
        for i in range(4):
            s = shifts[k % 4]
            dg["elements"][i] = int(dg["elements"][i]) + s
            k += 1
    wild = json.dumps(d).encode()
    assert np.array_equal(vk.vkey_words(wild), canon)
    via_ctor = p2v.VerifierCircuitData.from_words(p2v.circuit_words(gc.common, wild))
    # the constructor reads the same values: its word encoding of the shifted key ends in them
    assert np.array_equal(p2v.circuit_words(gc.common, wild)[-vk.key_words:], canon)
    assert via_ctor.info == vk.info


def test_with_keys_counts_limits_and_info(p2v):
    gcs = family(6, 1, 0)
    vk = p2v.VerifierCircuitData.from_json(gcs[0].common, gcs[0].vkey)
    assert vk.num_keys == 1
    keys = key_table(gcs)
    kt = vk.with_keys(keys[1:])
    assert kt.num_keys == 1 + len(keys) - 1 and vk.num_keys == 1   # base untouched
    assert kt.info == vk.info
    again = kt.with_keys([vk.vkey_words(keys[0])])                  # word arrays; deriving twice appends
    assert again.num_keys == kt.num_keys + 1 and again.info == vk.info
    assert vk.with_keys(np.stack([vk.vkey_words(k) for k in keys])).num_keys == 1 + len(keys)   # one [K, words] array
    assert vk.with_keys([]).num_keys == 1
    sv = kt.shape_variant(vk.info.num_public_inputs + 3, vk.info.final_poly_len)
    assert sv is not kt and sv.num_keys == kt.num_keys
    assert sv.info.num_public_inputs == vk.info.num_public_inputs + 3
    ext = p2v.VerifierCircuitData.from_json(gcs[0].common, gcs[0].vkey, ext=p2v.EXT_HASH_OR_NOOP)
    assert ext.with_keys(keys[1:2]).info.ext == p2v.EXT_HASH_OR_NOOP
    # P2V_MAX_KEYS = 65536 keys in total
    zeros = np.zeros((65535, vk.key_words), dtype=np.uint64)
    full = vk.with_keys(zeros)
    assert full.num_keys == 65536
    for base, extra in ((full, zeros[:1]), (vk, np.zeros((65536, vk.key_words), dtype=np.uint64)), (kt, zeros)):
        with pytest.raises(p2v.P2VError) as e:
            base.with_keys(extra)
        assert e.value.code == p2v.E_ARG
    with pytest.raises(p2v.P2VError) as e:   # a key of another circuit's cap length
        vk.with_keys([np.zeros(vk.key_words - 4, dtype=np.uint64)])
    assert e.value.code == p2v.E_ARG
    h = ctypes.c_void_p()
    assert p2v.lib().p2v_circuit_with_keys(vk.handle, None, 1, ctypes.byref(h)) == p2v.E_ARG
    assert p2v.lib().p2v_circuit_num_keys(None) == p2v.E_ARG
