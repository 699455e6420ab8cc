"""GPU tests (MI355X) of the device field arithmetic and the FRI query code, each production
function on its own (p2v_selftest ops 12-20, include/p2v.h): gl::add / sub / neg / mul_small /
emul / esqr, inv_chain / einv / einv2, pow_root, epow_u, reduce_powers and the folding forms of
every arity, against exact Python integers mod p on inputs built to take the rare branches that
the field elements of whole proofs (effectively random) never reach.  Every output word is
compared with ==; every reach condition is computed from the inputs and asserted."""
import random

import numpy as np
import pytest

from support import P, gen_circuit, p2v_module
from test_transcript_literal import (ROOTS, eadd, einv, emul, epow, escale, fold_coset, fold_coset_lagrange,
                                     reduce_with_powers, rev_bits)

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def p2v():
    # torch first, then libp2v: the order test_gpu.py, bench.py and smoke() use
    import torch
    assert torch.cuda.is_available(), "torch sees no GPU"
    m = p2v_module()
    if m.device_count() == 0:
        pytest.fail("no GPU visible to libp2v")
    return m


def _pool():
    """The edge pool V: canonical values only (the contract of add / sub / neg / emul / inversions)."""
    vals = {0, 1, 2, 3, P - 2, P - 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1}
    for k in range(64):
        vals |= {v for v in (1 << k, (1 << k) - 1, (1 << k) + 1, P - (1 << k)) if 0 <= v < P}
    rng = random.Random(317)
    rnd = set()
    while len(rnd) < 64:
        v = rng.randrange(P)
        if v not in vals:
            rnd.add(v)
    return sorted(vals) + sorted(rnd)


V = _pool()
PAIRS = [(u, v) for u in V for v in V]


def _run(p2v, op, items, b=None):
    a = np.array(items, dtype=np.uint64).reshape(len(items), -1)
    assert len(items) % 64 != 0, "item counts are chosen off the wave size: the last wave has idle lanes"
    out = p2v.device_selftest(op, a, None if b is None else np.array(b, dtype=np.uint64))
    return [tuple(int(x) for x in row) for row in out.tolist()]


def _same(what, items, out, exp):
    assert len(out) == len(exp) == len(items)
    bad = [i for i in range(len(exp)) if tuple(out[i]) != tuple(exp[i])]
    hx = lambda t: [hex(int(x)) for x in t]   # noqa: E731
    assert not bad, (what, len(bad), [(i, hx(items[i][:8]), hx(out[i]), hx(exp[i])) for i in bad[:4]])


def _odd(items):
    """The items, with the first repeated where their count is a multiple of 64."""
    return items + items[:1] if len(items) % 64 == 0 else items


def test_pool_is_the_stated_one():
    assert len(V) == 317 and len(set(V)) == 317 and all(0 <= v < P for v in V)
    assert len(PAIRS) == 100489


def test_gpu_field_plain_ops_all_edge_pairs(p2v):
    """gl::add, sub, neg, mul_small(., 7), mul_small(., low 32 bits of b) on every ordered pair of
    the pool, and mul_small by the constants 1, 7, 2^32 - 1 on every pool value."""
    items = _odd(PAIRS + [(v, c) for v in V for c in (1, 7, (1 << 32) - 1)])
    exp = [((x + y) % P, (x - y) % P, (-x) % P, 7 * x % P, x * (y & 0xFFFFFFFF) % P) for x, y in items]
    _same("F ops", items, _run(p2v, 12, items), exp)


def test_gpu_emul_edge_placements(p2v):
    """gl::emul on the device (mul128 and reduce128_nc's device branches, the 7 bd carry word, the
    third-word fold): every pool pair in six placements over the two components, the 4096 corner
    quadruples, and esqr on every pool pair.  Asserted reach: the borrow branch of reduce128_nc
    (low 64 bits of a product below its top 32 bits) and the third word of the cross sum."""
    rng = random.Random(1301)
    r = lambda: rng.randrange(P)   # noqa: E731
    place = [[(u, 0, v, 0) for u, v in PAIRS], [(0, u, 0, v) for u, v in PAIRS], [(u, 0, 0, v) for u, v in PAIRS],
             [(u, r(), v, r()) for u, v in PAIRS], [(r(), u, r(), v) for u, v in PAIRS], [(u, u, v, v) for u, v in PAIRS]]
    borrow = sum(1 for u, v in PAIRS if ((u * v) & M64) < ((u * v) >> 96))
    assert borrow >= 100, borrow

    def third_word(xa, xb, ya, yb):   # rbh = h2 + h3 + carry(l2 + l3) wraps
        p2, p3 = xa * yb, xb * ya
        return (p2 >> 64) + (p3 >> 64) + (((p2 & M64) + (p3 & M64)) >> 64) > M64
    wraps = sum(1 for it in place[5] if third_word(*it))
    assert wraps >= 1000, wraps
    corners = [0, 1, P - 1, P - 2, (1 << 32) - 1, 1 << 32, 1 << 63, P - (1 << 32)]
    quad = [(a, b, c, d) for a in corners for b in corners for c in corners for d in corners]
    for k, items in enumerate(place + [quad, [(u, v, u, v) for u, v in PAIRS]]):
        items = _odd(items)
        exp = [emul((a, b), (c, d)) for a, b, c, d in items]
        _same(f"emul set {k}", items, _run(p2v, 13, items), exp)


def _ext_specials(rng):
    """F^2 values of every class the inversions distinguish, three of each: the zero and
    non-zero ones interleave, so that a wave's lanes take both sides of einv2's fallback."""
    r = lambda: rng.randrange(1, P)   # noqa: E731
    out = []
    for _ in range(3):
        out += [(0, 0), (1, 0), (0, 1), (P - 1, P - 1), (r(), 0), (0, r()), (r(), r())]
    return out


def test_gpu_inversions_zero_fallback(p2v):
    """inv_chain (x^(p-2) by the addition chain, 0 -> 0), einv and einv2 with its zero fallback,
    against pow(norm, p - 2, p) (the reference's invExt) and against x x^-1 = 1.  einv2's items
    with u = 0, v = 0 and both share their waves with non-zero items (asserted)."""
    rng = random.Random(72)
    xs = _odd([(v,) for v in V] + [(rng.randrange(P),) for _ in range(4096)] + [(0,)])
    out = _run(p2v, 14, xs)
    _same("inv_chain", xs, out, [(pow(x, P - 2, P),) for x, in xs])
    assert all(x * o % P == 1 for (x,), (o,) in zip(xs, out) if x)
    assert out[0] == (0,) and xs[0] == (0,)

    sp = _ext_specials(rng)
    us = _odd(sp + [(a, b) for a in V[::9] for b in (0, 1, P - 1, V[5])])
    out = _run(p2v, 15, us)
    _same("einv", us, out, [einv(u) for u in us])
    assert all(emul(u, o) == (1, 0) for u, o in zip(us, out) if u != (0, 0))
    assert out[0] == (0, 0)

    items = _odd([u + v for u in sp for v in sp])
    kinds = [(it[:2] == (0, 0), it[2:] == (0, 0)) for it in items]
    assert {(True, False), (False, True), (True, True), (False, False)} <= set(kinds)
    waves = [kinds[i:i + 64] for i in range(0, len(kinds), 64)]
    assert all(any(a or b for a, b in w) and any(not (a or b) for a, b in w) for w in waves), "every wave diverges"
    out = _run(p2v, 16, items)
    _same("einv2", items, out, [einv(it[:2]) + einv(it[2:]) for it in items])
    for it, o in zip(items, out):
        for x, ix in ((it[:2], o[:2]), (it[2:], o[2:])):
            assert emul(x, ix) == ((1, 0) if x != (0, 0) else (0, 0)), it


def test_gpu_pow_root_and_epow(p2v):
    """pow_root(c, k, e) for every k = 0..32 with exponents that differ per lane (0, 1, 2^k - 1,
    2^(k-1), random below 2^k: the exponents the query code passes), against pow(ROOTS[k], e, p);
    epow_u on edge and random F^2 values at the small and the largest uniform exponents."""
    rng = random.Random(33)
    for k in range(33):
        es = {0, 1 % (1 << k), (1 << k) - 1, (1 << k) >> 1} | {rng.randrange(1 << k) for _ in range(90)}
        items = [(e,) for e in sorted(es)]
        items = (items * (70 // len(items) + 1))[:77] if len(items) < 64 else _odd(items)
        rng.shuffle(items)
        _same(f"pow_root k={k}", items, _run(p2v, 17, items, [k]), [(pow(ROOTS[k], e, P),) for e, in items])
    sh = V[:]
    rng.shuffle(sh)
    xs = _odd(list(zip(V, sh)) + [(v, 0) for v in V[::5]] + [(0, v) for v in V[::5]]
              + [(rng.randrange(P), rng.randrange(P)) for _ in range(64)])
    for e in (0, 1, 2, 3, 7, 8, 255, 256, (1 << 32) - 1):
        _same(f"epow_u e={e}", xs, _run(p2v, 18, xs, [e]), [epow(x, e) for x in xs])


def _alphas(rng):
    return [(0, 0), (1, 0), (0, 1), (P - 1, 0), (0, P - 1), (P - 1, P - 1)] + [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]


def _segment_tables(p2v):
    """(name, lengths[5], ns): five-segment tables whose boundaries fall inside 8-word chunks,
    with zero-length segments, for every N mod 8, N < 8, N = 8 and three chunks and more; the
    two-segment second-batch shape, also with its first segment empty; and the first / second
    batch of real circuits (without and with lookups), from their widths as k_fri derives them."""
    import json
    tabs = [("N=0", [0, 0, 0, 0, 0], 5)]
    for N in list(range(1, 18)) + [23, 24, 25, 29, 31, 32, 40, 43]:
        a, b = N // 3, N // 2
        tabs.append((f"N={N} no-lookup shape", [a, 1 if N - a - b > 0 else 0, b, N - a - b - (1 if N - a - b > 0 else 0), 0], 5))
        tabs.append((f"N={N} empty middle", [N - N // 4, 0, 0, N // 4, 0], 5))
    tabs += [("second batch", [2, 9, 0, 0, 0], 2), ("second batch rr=0", [0, 11, 0, 0, 0], 2), ("one segment", [13, 0, 0, 0, 0], 1)]
    for lk in (0, 5):
        gc = gen_circuit(6, 4, lk, 1, 28, 16, 0, 1)
        w = p2v.VerifierCircuitData.from_json(gc.common, gc.vkey).info.oracle_widths
        c = json.loads(gc.common)
        r, qdf = c["config"]["num_challenges"], c["quotient_degree_factor"]
        npp_all = r * -(-c["config"]["num_routed_wires"] // qdf)
        tabs.append((f"real s0 lk={lk}", [w[0], w[1], npp_all, w[3], w[2] - npp_all], 5))
        tabs.append((f"real s1 lk={lk}", [min(r, npp_all), w[2] - npp_all, 0, 0, 0], 2))
        assert (w[2] - npp_all > 0) == (lk != 0)
    return tabs


def test_gpu_reduce_powers_segments_and_accumulators(p2v):
    """reduce_powers (chunks of 8 with 128 + 3-bit unreduced accumulators, the N mod 8 head,
    seg_addr over up to five segments) against the literal reduce_with_powers on the concatenated
    segments.  The segments lie apart and out of order in the item, separated by words that
    must not be read.  Asserted reach: a chunk whose exact unreduced sum is >= 3 2^128 and one
    whose sum is < 2^128 (Acc3::top both ways)."""
    rng = random.Random(1002)
    alphas = _alphas(rng)
    top_max, top_min, seen_mod = 0, 9, set()
    for name, lens, ns in _segment_tables(p2v):
        N = sum(lens[:ns])
        seen_mod.add(N % 8)
        # place the segments: order 3, 0, 4, 1, 2 in the item, one guard word between them
        offs, w = [0] * 5, 2
        for s in (3, 0, 4, 1, 2):
            offs[s] = w
            w += lens[s] + 1
        stride = w
        pats = [lambda k: 0, lambda k: P - 1, lambda k: (1 << 32) - 1, lambda k: (P - 1) * (k & 1),
                lambda k: (P - 1) * (1 - (k & 1)), lambda k: rng.randrange(P), lambda k: rng.randrange(P)]
        items, exp = [], []
        for pat in pats:
            for al in alphas:
                ys = [pat(k) for k in range(N)]
                it = [rng.randrange(P) for _ in range(stride)]   # guard words: random
                it[0], it[1] = al
                k = 0
                for s in range(ns):
                    it[offs[s]:offs[s] + lens[s]] = ys[k:k + lens[s]]
                    k += lens[s]
                items.append(tuple(it))
                exp.append(reduce_with_powers(al, [(y, 0) for y in ys]))
                ap = [(1, 0)]
                for _ in range(8):
                    ap.append(emul(ap[-1], al))
                for j in range(0, N - N % 8, 8):
                    for comp in (0, 1):
                        tot = (ys[j] if comp == 0 else 0) + sum(ys[j + t] * ap[t][comp] for t in range(1, 8))
                        top_max, top_min = max(top_max, tot >> 128), min(top_min, tot >> 128)
        items = _odd(items)
        exp = exp + exp[:len(items) - len(exp)]
        _same("reduce_powers " + name, items, _run(p2v, 19, items, [stride, ns] + offs + lens), exp)
    assert seen_mod == set(range(8))
    assert top_max >= 3 and top_min == 0, (top_max, top_min)


def _poly_eval(coeffs, x):
    acc = (0, 0)
    for c in reversed(coeffs):
        acc = eadd(emul(acc, x), c)
    return acc


@pytest.mark.parametrize("ab", range(1, 9))
def test_gpu_fold_every_arity(p2v, ab):
    """One folding step at arity 2^ab through k_fri's own dispatch (fold_regs for 1..3,
    fold16_halves for 4, fold_generic for 5..8) with the production twiddles and 1 / 2^ab:
    constant evaluations fold to the constant, evaluations of a polynomial of degree < 2^ab to
    its value at beta, and all p - 1, b = 0, b = 1 (beta on the coset) and random items to
    foldCosetWith's value: the literal fold_coset up to arity 16, its Lagrange form (pinned to
    fold_coset by test_fold_coset_lagrange_is_fold_coset) above.  The device gets b = beta / ofs
    and the values in received order, v[k] = xs[rev k]."""
    rng = random.Random(900 + ab)
    n = 1 << ab
    re = lambda: (rng.randrange(P), rng.randrange(P))   # noqa: E731
    few = ab >= 7
    cases = []   # (b, ofs, xs, known value or None)
    for c in [(0, 0), (1, 0), (P - 1, P - 1), re()][:2 if few else 4]:
        cases.append((re(), rng.randrange(1, P), [c] * n, c))
    for deg in ([n - 1, 1] if few else [n - 1, n - 1, n // 2, 1, 0]):
        coeffs = [re() for _ in range(deg + 1)]
        ofs, b = rng.randrange(1, P), re()
        xs = [_poly_eval(coeffs, (ofs * pow(ROOTS[ab], j, P) % P, 0)) for j in range(n)]
        cases.append((b, ofs, xs, _poly_eval(coeffs, escale(ofs, b))))
    for b in [re(), (0, 0), (1, 0)]:
        cases.append((b, rng.randrange(1, P), [(P - 1, P - 1)] * n, None))
    for b in [(0, 0), (1, 0), (P - 1, 0), (0, 1)]:
        cases.append((b, rng.randrange(1, P), [re() for _ in range(n)], None))
    for _ in range(9 if few else 50):
        cases.append((re(), rng.randrange(1, P), [re() for _ in range(n)], None))
    assert len(cases) % 64 != 0 and (not few or len(cases) <= 36)
    ref = fold_coset if ab <= 4 else fold_coset_lagrange
    items, exp = [], []
    for b, ofs, xs, known in cases:
        want = ref(escale(ofs, b), ab, ofs, xs)
        assert known is None or want == known
        v = [xs[rev_bits(ab, k)] for k in range(n)]
        items.append(tuple(b) + tuple(w for e in v for w in e))
        exp.append(want)
    _same(f"fold ab={ab}", items, _run(p2v, 20, items, [ab]), exp)
