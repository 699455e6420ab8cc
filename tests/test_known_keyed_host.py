"""Host side of the per-key view of the known-openings table (include/p2v.h
p2v_circuit_known_key_rows, p2v.py VerifierCircuitData.known_rows): the entry point exists, a
handle that no verifier was created on has no table (0 rows for every key), and a key past the
handle's table is an argument error.  No GPU: a handle without a table is answered before any
device call.  The kernels are held to the oracle in tests/test_gpu_known_keyed.py."""
import ctypes

import pytest

from support import p2v_module
from test_keys import family, key_table


@pytest.fixture(scope="module")
def p2v():
    return p2v_module()


def test_known_key_rows_entry_point_and_arguments(p2v):
    L = p2v.lib()
    assert hasattr(L, "p2v_circuit_known_key_rows")
    gcs = family(6, 1, 0)
    keys = key_table(gcs)
    base = p2v.VerifierCircuitData.from_json(gcs[0].common, keys[0])
    vk = base.with_keys(keys[1:])
    assert (base.num_keys, vk.num_keys) == (1, 5)
    assert base.known_rows(0) == 0
    assert [vk.known_rows(k) for k in range(5)] == [0] * 5
    assert vk.known_stats() == {"hits": 0, "misses": 0, "inserted": 0}
    for h, bad in ((base, 1), (vk, 5), (vk, 2 ** 32 - 1)):
        with pytest.raises(p2v.P2VError) as e:
            h.known_rows(bad)
        assert e.value.code == p2v.E_ARG
    out = ctypes.c_uint64(7)   # the C entry point: the count is zeroed on every path, null arguments are refused
    assert L.p2v_circuit_known_key_rows(vk.handle, 0, 5, ctypes.byref(out)) == p2v.E_ARG and out.value == 0
    assert L.p2v_circuit_known_key_rows(vk.handle, 0, 4, ctypes.byref(out)) == p2v.E_OK and out.value == 0
    assert L.p2v_circuit_known_key_rows(None, 0, 0, ctypes.byref(out)) == p2v.E_ARG
    assert L.p2v_circuit_known_key_rows(vk.handle, 0, 0, None) == p2v.E_ARG
