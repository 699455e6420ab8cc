"""CPU model of the known-openings table (merkle.hip k_merkle_known / k_merkle_known_miss),
restated in Python over a stand-in hash.

The table remembers the complete input (leaf words, sibling words) of tree-0 openings that the
plain computation found True against the circuit's cap, direct-mapped by leaf index; an opening is
accepted from the table only when every word equals the remembered row.  That is memoisation of a
pure function, so it needs nothing from the hash: over random sequences of honest and mutated
openings the memoised status equals the plain one (Hash/Merkle.hs:27-42), whatever the table
holds, and the table never holds an opening whose plain status is False.  The GPU suite holds the
kernels themselves to the oracle (tests/test_gpu_known.py)."""
import random

import pytest

MASK = (1 << 64) - 1


def h2(a, b):   # stand-in compression: any deterministic function of the ordered pair
    x = (a * 0x9E3779B97F4A7C15 + b * 0xC2B2AE3D27D4EB4F + 0x165667B19E3779F9) & MASK
    x ^= x >> 29
    return (x * 0xBF58476D1CE4E5B9) & MASK


def sponge(words):   # stand-in leaf hash: any deterministic function of the word list
    acc = 0x27D4EB2F165667C5
    for w in words:
        acc = h2(acc, w)
    return acc


def plain_ok(leaf, sibs, idx, depth, cap):
    """The reference computation of one opening: leaf sponge, path, cap entry."""
    cur = sponge(leaf)
    for l in range(depth):
        cur = h2(sibs[l], cur) if idx & 1 else h2(cur, sibs[l])
        idx >>= 1
    return cap.get(idx) == cur


class Known:
    """The table and the two kernels.  mode 1: probe and insert; mode 2: probe only."""

    def __init__(self, bits, mode=1):
        self.rows = [None] * (1 << bits)   # row idx: the remembered words, valid once set
        self.mode = mode
        self.hits = self.misses = self.inserted = 0
        self.plain_calls = 0

    def probe(self, leaf, sibs, idx):   # k_merkle_known: loads and compares only
        row = self.rows[idx]
        return row is not None and row == (tuple(leaf), tuple(sibs))

    def miss(self, leaf, sibs, idx, depth, cap):   # k_merkle_known_miss
        self.plain_calls += 1
        ok = plain_ok(leaf, sibs, idx, depth, cap)
        if ok and self.mode == 1 and self.rows[idx] is None:   # rows are written once, never rewritten
            self.rows[idx] = (tuple(leaf), tuple(sibs))
            self.inserted += 1
        return ok

    def batch(self, openings, depth, cap):
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
                out.append(self.miss(*o, depth, cap))
        return out


def honest_tree(rnd, bits, cap_height, width):
    depth = bits - cap_height
    leaves = [[rnd.getrandbits(64) for _ in range(width)] for _ in range(1 << bits)]
    levels = [[sponge(w) for w in leaves]]
    for l in range(depth):
        prev = levels[-1]
        levels.append([h2(prev[2 * i], prev[2 * i + 1]) for i in range(len(prev) // 2)])
    cap = dict(enumerate(levels[depth]))

    def opening(idx):
        return list(leaves[idx]), [levels[l][(idx >> l) ^ 1] for l in range(depth)], idx
    return opening, cap, depth


def mutated(rnd, opening, bits, depth):
    """An opening that differs from the honest one of some index in one place."""
    idx = rnd.randrange(1 << bits)
    leaf, sibs, idx = opening(idx)
    kind = rnd.randrange(4)
    if kind == 0:
        leaf[rnd.randrange(len(leaf))] ^= 1 << rnd.randrange(64)
    elif kind == 1 and depth:
        sibs[0] = (sibs[0] + 1) & MASK
    elif kind == 2 and depth:
        sibs[depth - 1] = (sibs[depth - 1] + 1) & MASK
    else:   # another index's authentic leaf and path: the content is right, the index is wrong
        idx = (idx + 1 + rnd.randrange((1 << bits) - 1)) % (1 << bits)
    return leaf, sibs, idx


@pytest.mark.parametrize("bits,cap_height,width", [(6, 2, 5), (7, 4, 9), (5, 0, 3), (4, 4, 2)])
@pytest.mark.parametrize("mode", [1, 2])
def test_known_model_memoised_status_is_the_plain_status(bits, cap_height, width, mode):
    rnd = random.Random(bits * 31 + cap_height * 7 + mode)
    opening, cap, depth = honest_tree(rnd, bits, cap_height, width)
    K = Known(bits, mode)
    total = 0
    for _ in range(60):
        ops = [mutated(rnd, opening, bits, depth) if rnd.random() < 0.3 else opening(rnd.randrange(1 << bits))
               for _ in range(rnd.randrange(1, 40))]
        ref = [plain_ok(*o, depth, cap) for o in ops]
        assert K.batch(ops, depth, cap) == ref
        total += len(ops)
        for idx, row in enumerate(K.rows):   # nothing false is remembered, and only under its own index
            if row is not None:
                assert plain_ok(list(row[0]), list(row[1]), idx, depth, cap)
    assert K.hits + K.misses == total
    assert K.plain_calls == K.misses
    if mode == 2:
        assert K.hits == 0 and K.inserted == 0
    else:
        assert K.inserted == sum(r is not None for r in K.rows) and K.hits > 0


def test_known_model_cold_then_warm_and_one_word_changed():
    rnd = random.Random(11)
    bits, cap_height, width = 6, 2, 7
    opening, cap, depth = honest_tree(rnd, bits, cap_height, width)
    idx = [rnd.randrange(1 << bits) for _ in range(200)]
    ops = [opening(i) for i in idx]
    K = Known(bits)
    assert all(K.batch(ops, depth, cap))
    assert (K.hits, K.misses, K.inserted) == (0, len(ops), len(set(idx)))
    assert all(K.batch(ops, depth, cap))
    assert (K.hits, K.misses, K.inserted) == (len(ops), len(ops), len(set(idx)))
    leaf, sibs, i = opening(idx[0])
    for bad in ((leaf[:-1] + [leaf[-1] ^ 1], sibs, i), (leaf, [sibs[0] ^ 1] + sibs[1:], i), (leaf, sibs[:-1] + [sibs[-1] ^ 1], i),
                (leaf, sibs, idx[0] ^ 1)):
        before = K.misses
        assert K.batch([bad], depth, cap) == [False]
        assert K.misses == before + 1 and K.inserted == len(set(idx))


def test_known_model_garbage_inserts_nothing():
    rnd = random.Random(5)
    bits, cap_height, width = 6, 2, 7
    opening, cap, depth = honest_tree(rnd, bits, cap_height, width)
    K = Known(bits)
    junk = [([rnd.getrandbits(64) for _ in range(width)], [rnd.getrandbits(64) for _ in range(depth)], rnd.randrange(1 << bits))
            for _ in range(300)]
    assert not any(K.batch(junk, depth, cap))
    assert (K.hits, K.inserted) == (0, 0) and all(r is None for r in K.rows)


def test_known_fill_rate_arithmetic():
    """Uniform indices: a 4 096-proof batch opens 28 * 4096 of the 2^15 rows' indices, so a row is
    still empty with probability (1 - 2^-15)^(114 688 k) after k batches."""
    draws = 28 * 4096
    empty1 = (1 - 2.0 ** -15) ** draws
    assert 0.96 < 1 - empty1 < 0.98
    assert 1 - empty1 ** 2 > 0.999
