"""CPU model of the known-openings table with a key dimension (merkle.hip "Keys"), restated in
Python over the stand-in hash of tests/test_known_model.py.

A key fixes the cap, so the table has one block of rows per key: the row of (key k, index idx) is
k << bits | idx, and the miss kernel takes the cap it compares against and the row it writes from
one read of the opening's id, clamped to nkeys - 1.  Over random sequences of honest, mutated and
wrong-key openings (an honest opening of one key presented under another id, ids past the table
among them) the memoised status equals the plain one under the clamped key's cap, and no (key,
idx) row ever holds an opening that is False under that key's cap.  The GPU suite holds the kernels
themselves to the oracle (tests/test_gpu_known_keyed.py)."""
import random

import pytest

from test_known_model import honest_tree, mutated, plain_ok


class KeyedKnown:
    """The table and the two kernels.  mode 1: probe and insert; mode 2: probe only."""

    def __init__(self, bits, nkeys, mode=1):
        self.bits, self.nkeys, self.mode = bits, nkeys, mode
        self.rows = [None] * (nkeys << bits)   # row k << bits | idx: the remembered words, valid once set
        self.hits = self.misses = self.inserted = self.plain_calls = 0

    def key(self, kid):   # known_key(): the id clamped as lane_key() clamps it
        return min(kid, self.nkeys - 1)

    def row(self, k, idx):   # known_row()
        return k << self.bits | idx

    def probe(self, leaf, sibs, idx, kid):   # k_merkle_known: loads and compares only
        row = self.rows[self.row(self.key(kid), idx)]
        return row is not None and row == (tuple(leaf), tuple(sibs))

    def miss(self, leaf, sibs, idx, kid, depth, caps):   # k_merkle_known_miss
        self.plain_calls += 1
        k = self.key(kid)   # read once: the cap compared against and the row written are this key's
        ok = plain_ok(leaf, sibs, idx, depth, caps[k])
        r = self.row(k, idx)
        if ok and self.mode == 1 and self.rows[r] is None:   # rows are written once, never rewritten
            self.rows[r] = (tuple(leaf), tuple(sibs))
            self.inserted += 1
        return ok

    def batch(self, openings, depth, caps):
        """One run: every opening probed against the table as it stood before the run's miss
        kernel, then the misses computed (and inserted)."""
        hit = [self.probe(*o) for o in openings]
        out = []
        for o, h in zip(openings, hit):
            if h:
                self.hits += 1
                out.append(True)
            else:
                self.misses += 1
                out.append(self.miss(*o, depth, caps))
        return out

    def check_rows(self, depth, caps):
        """Nothing False is remembered, and only under its own key and index."""
        for r, row in enumerate(self.rows):
            if row is not None:
                k, idx = r >> self.bits, r & ((1 << self.bits) - 1)
                assert plain_ok(list(row[0]), list(row[1]), idx, depth, caps[k]), (k, idx)


def keyed_trees(rnd, bits, cap_height, width, nkeys):
    """One honest tree per key (so one cap per key); the last key repeats key 0's tree: equal caps
    under two ids still fill two blocks of rows."""
    trees = [honest_tree(rnd, bits, cap_height, width) for _ in range(nkeys - 1)]
    trees.append(trees[0])
    return [t[0] for t in trees], [t[1] for t in trees], trees[0][2]


def random_opening(rnd, openers, bits, depth, nkeys):
    k = rnd.randrange(nkeys)
    u = rnd.random()
    if u < 0.25:
        o = mutated(rnd, openers[k], bits, depth)
    else:
        o = openers[k](rnd.randrange(1 << bits))
    kid = k
    if 0.25 <= u < 0.5:   # wrong key: another id, ids past the table among them (clamped to the last key)
        kid = rnd.choice([j for j in range(nkeys) if j != k] + [nkeys, nkeys + 3, 2 ** 32 - 1])
    elif k == nkeys - 1 and rnd.random() < 0.5:
        kid = rnd.choice([nkeys, 2 ** 32 - 1])   # an out-of-range id is a statement about the last key
    return (*o, kid)


@pytest.mark.parametrize("bits,cap_height,width,nkeys", [(6, 2, 5, 3), (7, 4, 9, 5), (5, 0, 3, 2), (4, 4, 2, 4)])
@pytest.mark.parametrize("mode", [1, 2])
def test_keyed_model_memoised_status_is_the_plain_status(bits, cap_height, width, nkeys, mode):
    rnd = random.Random(bits * 31 + cap_height * 7 + mode + 100 * nkeys)
    openers, caps, depth = keyed_trees(rnd, bits, cap_height, width, nkeys)
    K = KeyedKnown(bits, nkeys, mode)
    total = wrong_key_true = 0
    for _ in range(60):
        ops = [random_opening(rnd, openers, bits, depth, nkeys) for _ in range(rnd.randrange(1, 40))]
        ref = [plain_ok(leaf, sibs, idx, depth, caps[min(kid, nkeys - 1)]) for leaf, sibs, idx, kid in ops]
        assert K.batch(ops, depth, caps) == ref
        total += len(ops)
        K.check_rows(depth, caps)
    assert K.hits + K.misses == total and K.plain_calls == K.misses
    if mode == 2:
        assert K.hits == 0 and K.inserted == 0
    else:
        assert K.inserted == sum(r is not None for r in K.rows) and K.hits > 0
        filled = {r >> bits for r, row in enumerate(K.rows) if row is not None}
        assert filled == set(range(nkeys))   # every key's block, the twin of key 0 in its own


def test_keyed_model_an_opening_warm_under_one_key_misses_under_another():
    """The soundness case of the GPU suite: warm key 0, present the same words under key 1 (another
    cap): rejected, a miss every time, nothing inserted; under key 2 (key 0's cap again) one miss
    into its own rows, then a hit."""
    rnd = random.Random(3)
    bits, nkeys = 6, 3
    openers, caps, depth = keyed_trees(rnd, bits, 2, 7, nkeys)
    assert caps[0] != caps[1] and caps[0] == caps[2]
    K = KeyedKnown(bits, nkeys)
    idx = [rnd.randrange(1 << bits) for _ in range(100)]
    warm = [(*openers[0](i), 0) for i in idx]
    assert all(K.batch(warm, depth, caps))
    d = len(set(idx))
    assert (K.hits, K.misses, K.inserted) == (0, 100, d)
    for rep in range(2):
        assert not any(K.batch([(*openers[0](i), 1) for i in idx], depth, caps))
        assert (K.hits, K.misses, K.inserted) == (0, 100 * (rep + 2), d)
    assert all(K.batch(warm, depth, caps))
    assert (K.hits, K.misses, K.inserted) == (100, 300, d)
    twin = [(*openers[0](i), 2) for i in idx]
    assert all(K.batch(twin, depth, caps)) and (K.hits, K.misses, K.inserted) == (100, 400, 2 * d)
    assert all(K.batch(twin, depth, caps)) and (K.hits, K.misses, K.inserted) == (200, 400, 2 * d)
    K.check_rows(depth, caps)


def test_keyed_fill_rate_arithmetic():
    """K keys used uniformly: a 4 096-proof batch draws 28 * 4096 / K indices per key over 2^15
    rows, so with K = 16 a row is still empty after m batches with probability e^(-0.219 m):
    99 % of the rows after 21 batches, 99.9 % after 32 (include/p2v.h)."""
    per_key = 28 * 4096 / 16
    rate = per_key / 2 ** 15
    assert abs(rate - 0.219) < 0.001
    empty = lambda m: (1 - 2.0 ** -15) ** (per_key * m)   # noqa: E731
    assert 0.9898 < 1 - empty(21) < 0.9900 and 1 - empty(20) < 0.9875   # 98.99 %: the table's "99 %"
    assert empty(31) > 0.001 > empty(32)
