"""Every form of the device permutation at steered inner-round and output edge states
(poseidon_steer.py: the input is found by running the chosen state backwards), against the oracle's
permutation (Hash/Poseidon.hs:42-46), word for word.  The forms: the throughput permutation's
template instances as production runs them (p2v_selftest op 23, and ops 1 and 2), the latency forms
(ops 9 and 10) and the leaf sponge (op 24, Hash/Sponge.hs:26-31).  Steered states share their waves
with random ones, so a wave-uniform fix-up branch runs with lanes that need it and lanes that do
not, and every launch has at least 130 items: it crosses a wave edge into a part-filled wave.
What the campaigns reach, by the exact model, is asserted in test_poseidon_steer.py and again in
the fixture here."""
import numpy as np
import pytest

import poseidon_steer as ps
from support import oracle, p2v_module, sbox_edge_values

pytestmark = pytest.mark.gpu

P = ps.P
FORMS = {0: "permute_dev<true, true>", 1: "permute_dev<true, false>", 2: "permute_dev<false, true>"}


@pytest.fixture(scope="module")
def p2v():
    # torch first, then libp2v: the order test_gpu.py, bench.py and smoke() use
    import torch
    assert torch.cuda.is_available(), "torch sees no GPU"
    m = p2v_module()
    if m.device_count() == 0:
        pytest.fail("no GPU visible to libp2v")
    return m


@pytest.fixture(scope="module")
def C():
    c = ps.campaigns()
    ps.check_conditions(c)
    return c


def _mixed(inputs, seed, zh=False):
    """The steered inputs shuffled among random states (a third as many, and at least up to 130
    items): (the u64 array, the oracle's outputs)."""
    rng = np.random.default_rng(seed)
    n_rnd = max(len(inputs) // 3, 130 - len(inputs), 8)
    st = [list(s) for s in inputs] + [[int(x) for x in r] for r in rng.integers(0, 1 << 64, size=(n_rnd, 12), dtype=np.uint64)]
    st = [st[i] for i in rng.permutation(len(st))]
    assert len(st) >= 130
    O = oracle()
    exp = [O.permute([x % P for x in s[:8]] + [0] * 4 if zh else [x % P for x in s]) for s in st]
    return np.array(st, dtype=np.uint64), np.array(exp, dtype=np.uint64)


def _masked(exp, gm):
    m = exp.copy()
    for g in range(3):
        if not (gm >> g) & 1:
            m[:, 4 * g:4 * g + 4] = 0
    return m


def _check(p2v, what, op, a, exp, b=None):
    out = p2v.device_selftest(op, a, None if b is None else np.array(b, dtype=np.uint64))
    assert out.shape == exp.shape, (what, out.shape)
    bad = np.nonzero((out != exp).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), [([hex(int(x)) for x in a[i]], [hex(int(x)) for x in out[i]],
                                            [hex(int(x)) for x in exp[i]]) for i in bad[:2]])


def _check_variants(p2v, a, exp, forms, zh, gms=(7,)):
    for form in forms:
        for gm in gms:
            _check(p2v, (FORMS[form], "zh", zh, "gm", gm), 23, a, _masked(exp, gm), [form, zh, gm])


def test_gpu_sbox_edges_in_every_round(p2v, C):
    """A: in each round 0..29, 32 states whose S-box inputs of that round (12 in a full round, word 0
    in a partial one) are the S-box edge values; the -2^64 fix-up of the S-box multiply runs in
    every round.  Ops 1, 9 and 10 and the other two template instances."""
    a, exp = _mixed([s["inp"] for s in C["A"]], 1)
    for op in (1, 9, 10):
        _check(p2v, op, op, a, exp)
    _check_variants(p2v, a, exp, (1, 2), 0)


def test_gpu_zh_forms(p2v, C):
    """B: words 8..11 entering as 0.  Round-0 edge inputs on words 0..7, 8 steered S-box inputs of
    round 1, and the states that aim the carry of the peeled round 0 (D), through the compression
    op and both zh instances at every gm the leaf sponge passes."""
    a, exp = _mixed([s["inp"] for s in C["B"]] + [s["inp"] for s in C["D"] if s["zh"]], 2, zh=True)
    _check(p2v, 2, 2, a, _masked(exp, 1))
    _check_variants(p2v, a, exp, (0, 1), 1, (1, 4, 6, 7))


def test_gpu_output_edges(p2v, C):
    """C: outputs steered to 0, 1, 2^32 - 2, 2^32 - 1, 2^32, p - 2, p - 1 in every word position.
    Words inside gm are the canonical value, words outside it 0, for every gm of every instance."""
    a, exp = _mixed([s["inp"] for s in C["C"]], 3)
    for op in (1, 9, 10):
        _check(p2v, op, op, a, exp)
    _check_variants(p2v, a, exp, (0, 1, 2), 0, range(1, 8))


def test_gpu_mds_carry_in_inner_rounds(p2v, C):
    """D: the carry fix-up of mds_group in full rounds 1, 2, (3,) 26..29: >= 32 rows that take it and
    >= 32 that stop just below the threshold per round, in the waves of every instance."""
    a, exp = _mixed([s["inp"] for s in C["D"] if not s["zh"]], 4)
    _check_variants(p2v, a, exp, (0, 1, 2), 0)
    _check(p2v, 1, 1, a, exp)


def test_gpu_merged_block_branch_rows(p2v, C):
    """E: chain rows 1 and 2 of every block of 4 merged partial rounds of both schedules, and the
    group rows of pblock<2>: the state entering each block makes the row's carry run in some lanes
    and narrowly not in others."""
    a, exp = _mixed([s["inp"] for s in C["E"]], 5)
    _check_variants(p2v, a, exp, (0, 1, 2), 0)
    _check(p2v, 1, 1, a, exp)


def _sponge(O, words, noop):
    """the leaf sponge, overwrite mode, no padding (Hash/Sponge.hs:26-31); hash_or_noop when asked"""
    if noop and len(words) <= 4:
        return list(words) + [0] * (4 - len(words))
    st = [0] * 12
    for i in range(0, len(words), 8):
        blk = words[i:i + 8]
        st[:len(blk)] = [w % P for w in blk]
        st = O.permute(st)
    return st[:4]


def test_gpu_leaf_sponge(p2v):
    """F: leaf_sponge (its one-block-ahead prefetch, and the zh and gm it derives from the length) at
    every length 0..33 and the standard circuit's leaf widths, 140 leaves each of edge and random
    words; on the sponge path words >= p too, read mod p.  len <= 5 with and without hash_or_noop."""
    O = oracle()
    rng = np.random.default_rng(6)
    edges = ps.OUT_EDGES + sbox_edge_values()[::7]
    wide = [P, P + 1, (1 << 64) - 1, (1 << 64) - (1 << 32)]
    for n_words in list(range(34)) + [w for w in ps.STANDARD_LEAF_WIDTHS if w > 33]:
        for noop in ((0, 1) if n_words <= 5 else (0,)):
            pool = edges if noop and n_words <= 4 else edges + wide
            a = rng.integers(0, P if noop and n_words <= 4 else 1 << 64, size=(140, n_words), dtype=np.uint64)
            pick = rng.integers(0, 3, size=a.shape) == 0
            a[pick] = np.array(pool, dtype=np.uint64)[rng.integers(0, len(pool), size=int(pick.sum()))]
            exp = np.array([_sponge(O, [int(x) for x in row], noop) for row in a], dtype=np.uint64).reshape(140, 4)
            if n_words == 0:
                assert not exp.any()
            _check(p2v, ("leaf_sponge", n_words, noop), 24, a, exp, [n_words, noop])
