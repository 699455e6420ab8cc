"""GPU tests (MI355X) of gate parameters other than the generator's one set per gate kind
(csrc/vanish.h eval_gate, gate_coset, gate_random_access; the host plan of csrc/api_workspace.cpp: each
item's first alpha exponent, the coset part counts, the heaviest-first order), and of gate
programs fed with edge values.

A generated circuit's gate strings are replaced by the entries of shapes.PARAMS (each fits 135
wires and 2 constants).  The generator's proofs keep their shape, Merkle paths, transcript and FRI
rounds against the swapped circuit; only the identity fails, so the whole trace stays comparable
with the oracle's, whose gate programs tests/test_shapes_cpu.py pins against the literal for every
entry.  Reached, by the parameters: the RandomAccess `switch (nbits)` arms 0, 1, 2, 3 and its
default form (bits 5 and 6; the generator's 4 is the remaining arm); BaseSum with one limb and the
bases 0, 1, 2, 3, 4, 16; coset gates of 1, 2, 3, 7, 11 and 15 parts, with degree >= 2^bits,
without intermediates, and with a weight list that ends in the second or the first part.
Statuses and full traces equal the oracle's with ==."""
import json

import numpy as np
import pytest

import shapes as SH
from support import p2v_module, randomize_openings
from test_gpu_challenges import Case, kernels

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def p2v():
    import torch   # before libp2v, as tests/test_gpu.py
    assert torch.cuda.is_available(), "torch sees no GPU"
    m = p2v_module()
    if m.device_count() == 0:
        pytest.fail("no GPU visible to libp2v")
    return m


_base = {}


def base(p2v, r) -> Case:
    """The mode-1 circuit of 2^6 rows at r rounds with a valid proof and two copies with uniform
    `constants` openings (every gate filter then an arbitrary value)."""
    if r not in _base:
        gc = SH.circuit(6, r=r)
        a, b = gc.proof(1, 1), gc.proof(2, 2)
        _base[r] = Case(p2v, gc, texts=[a, randomize_openings(a, 7, keys=("constants",)), randomize_openings(b, 8, keys=("constants",))])
    return _base[r]


def _swapped_vs_oracle(p2v, r, repl, ns):
    B = base(p2v, r)
    D = Case(p2v, B.gc, texts=B.texts, common=SH.swap(B.gc.common, repl))
    assert D.vk.info == B.vk.info
    for unit in (True, False):
        st, tr = D.want(unit)
        _, tr0 = B.want(unit)
        assert st.tolist() == [0, 0, 0]
        live = slice(None) if unit else slice(1, None)   # a filter that is arbitrary or 1: the swapped gate's terms are in C_i
        assert (D.combined(tr)[live] != 0).all()
        assert (D.combined(tr)[live] != B.combined(tr0)[live]).all(), "the swapped gate is not live"
        for n in ns:
            D.check(p2v, n, unit_filters=unit)
    return D


@pytest.mark.parametrize("kind,p", SH.ENTRIES, ids=lambda x: str(x).replace(" ", ""))
@pytest.mark.parametrize("r", [2, 3])
def test_gpu_gate_parameters_one_gate_at_a_time(p2v, r, kind, p):
    """One gate string replaced by a table entry, at r = 2 and r = 3 (the _r2 and _rn kernels):
    the trace of three proofs equals the oracle's with the circuit's filters and with every filter
    1, and the oracle's C_i is non-zero and not the unswapped circuit's."""
    _swapped_vs_oracle(p2v, r, {kind: p}, ns=(3,))


@pytest.mark.parametrize("r", [2, 3])
def test_gpu_gate_parameters_every_kind_at_once(p2v, r):
    """Every kind replaced in one circuit (other first alpha exponents for every item after the
    first, another heaviest-first order): n = 3 (the latency path) and n = 70 (the batch path)."""
    D = _swapped_vs_oracle(p2v, r, SH.ALL_AT_ONCE, ns=(3, 70))
    print("r =", r, "kernels:", kernels(D.vk, D.gates))


# ----------------------------------------------------------------------------- edge-valued wires
N_EDGE = 24


def _edge_proofs(gc, with_constants):
    from test_gpu_field import _pool
    pool = _pool()
    text = gc.proof(1, 1)
    o = json.loads(text)["proof"]["openings"]
    wires = SH.edge_rows(pool, len(o["wires"]), N_EDGE, 5)
    consts = SH.edge_rows(pool, len(o["constants"]), N_EDGE, 6)
    return [SH.with_openings(text, wires=w, **({"constants": k} if with_constants else {})) for w, k in zip(wires, consts)]


@pytest.mark.parametrize("with_constants", [False, True], ids=["wires", "wires_and_constants"])
@pytest.mark.parametrize("swapped", [False, True], ids=["standard", "all_replaced"])
@pytest.mark.parametrize("r", [2, 3])
def test_gpu_gate_programs_on_edge_valued_openings(p2v, r, swapped, with_constants):
    """The `wires` openings (and the `constants`) of a proof replaced by values of the field
    tests' edge pool: whole rows of 0, 1, p - 1, 2^32 - 1, 2^32, 2^32 + 1, rows of 2^k, 2^k +- 1 and
    p - 2^k, and those among uniform values, which uniform field elements never put into a gate
    program.  With every filter 1, on the generator's circuit and on the one with every kind
    replaced: the trace equals the oracle's on the latency path (n = 24) and the batch path (70)."""
    gc = SH.circuit(6, r=r)
    D = Case(p2v, gc, texts=_edge_proofs(gc, with_constants), common=SH.swap(gc.common, SH.ALL_AT_ONCE) if swapped else None)
    st, tr = D.want(True)
    comb = D.combined(tr)
    assert len({tuple(c) for c in comb.tolist()}) == N_EDGE   # every proof has a C_i of its own
    assert (comb[6:] != 0).all()
    D.check(p2v, N_EDGE, unit_filters=True)
    D.check(p2v, 70, unit_filters=True)
