"""The steering helper (poseidon_steer.py) in exact integers, with no device: the round-by-round
permutation and its inverse (Hash/Poseidon.hs:42-101), that every steered state of the campaigns
meets its target in its round, the restated branch predicates against independent arithmetic, and
that the campaigns tests/test_gpu_poseidon_steer.py runs reach every rare branch of
csrc/poseidon.h, and narrowly miss it, as often as they must: the coverage is proved here."""
import random

import poseidon_fold3_model as f3
import poseidon_steer as ps
from support import add_nc, oracle, preimage_round0, sbox_edge_values

P, M, RC = ps.P, ps.M, ps.RC
M32 = ps.M32
RC0 = RC[:12]


def test_round_trip_kat_and_oracle():
    O = oracle()
    assert ps.permute(list(range(12))) == ps.pm.KAT
    assert ps.permute_inv(ps.pm.KAT) == list(range(12))
    rng = random.Random(1)
    assert all(sum(ps.M[i][k] * ps.MINV[k][j] for k in range(12)) % P == (i == j) for i in range(12) for j in range(12))
    for v in (0, 1, P - 1, 2**32 - 1, 2**32 + 1, 2**48, rng.randrange(P)):
        assert ps.sbox_inv(ps.sbox(v)) == v == ps.sbox(ps.sbox_inv(v))
    for _ in range(8):
        s = [rng.randrange(P) for _ in range(12)]
        o = ps.permute(s)
        assert o == ps.pm.perm_plain(s) == O.permute(s)
        assert ps.permute_inv(o) == s
        r = rng.randrange(30)
        assert ps.round_inv(ps.round_fwd(s, r), r) == s


def test_steering_round_trips_at_random_rounds():
    """states steered at rounds 0..29 to edge and random words round-trip exactly, and steered
    outputs are the oracle's"""
    O = oracle()
    rng = random.Random(2)
    edges = [0, 1, P - 1, 2**32 - 1, 2**32 + 1, 2**48]
    for r in list(range(30)) + [rng.randrange(30) for _ in range(10)]:
        x = [rng.choice(edges) if rng.randrange(2) else rng.randrange(P) for _ in range(12)]
        inp = ps.steer(r, x)
        assert ps.sbox_inputs(inp, r) == x
        if r == 0:
            assert [w % P for w in ps.steer_zh_round0(x[:8])[:8]] == inp[:8]
    o = [0, 1, 2**32 - 2, 2**32 - 1, 2**32, P - 1, P - 2, 0, 1, 2**32 - 1, 2**32, P - 1]
    assert O.permute(ps.steer_out(o)) == o == ps.permute(ps.steer_out(o))


def test_branch_predicates_against_plain_arithmetic():
    """mul_dev is a multiply mod p into [0, 2^64) whose neg is the stated predicate; sbox_dev is
    x^7; row_carry is poseidon_fold3_model.row's reduction with the same carry"""
    rng = random.Random(3)
    ev = sbox_edge_values()
    for _ in range(4000):
        a = rng.choice(ev) if rng.randrange(2) else rng.randrange(2**64)
        b = rng.choice(ev) if rng.randrange(2) else rng.randrange(2**64)
        r, neg = ps.mul_dev(a, b)
        assert 0 <= r < 2**64 and r % P == a * b % P
        t = (a * b & ps.M64) + ((a * b >> 64) & M32) * M32
        assert neg == (t < 2**64 and t < (a * b >> 96))
    assert ps.mul_dev(2**48, 2**48) == (P - 1, True)             # 2^96 = -1: lo = h0 = 0, product >> 96 = 1
    assert ps.sbox_neg(2**48) >= {1} and ps.sbox_neg(2**24) >= {2}
    for v in ev:
        for w in ([v] if v >= M32 else [v, v + P]):
            assert ps.sbox_dev(w)[0] % P == pow(v, 7, P)
    for _ in range(500):
        vals = [rng.randrange(2**64) for _ in range(12)]
        k = rng.randrange(P)
        i = rng.randrange(12)
        r, c, lo = ps.row_carry(M[i], vals, k)
        rr, cc, _ = f3.row(M[i], vals, k & M32, k >> 32, False)
        assert (r, c) == (rr, cc) and r % P == (sum(m * v for m, v in zip(M[i], vals)) + k) % P
    # the carry is what the fix-up branch tests: it needs ah_lo above 2^32 - 2^11
    y = ps.aim_mds(rng, ps.mds_consts(1))
    assert all(lo > 2**32 - 2**11 for _, c, lo in ps.mds_rows(y, ps.mds_consts(1)) if c)


def test_every_steered_target_is_hit():
    O = oracle()
    C = ps.campaigns()
    for s in C["A"]:
        x = ps.sbox_inputs(s["inp"], s["round"])
        assert x == s["x"], s["round"]
        if s["round"] == 0:   # the device's own first addition: the 64-bit value itself wherever one exists
            assert s["inp"] == [preimage_round0(v, i, RC0) % P for i, v in enumerate(x)]
            assert all(add_nc(w, c) == (v if v >= M32 else v + P) for w, c, v in zip(s["inp"], RC0, x))
    for s in C["B"]:
        assert s["inp"][8:] == [0] * 4
        x = ps.sbox_inputs(s["inp"], s["round"])
        assert [x[i] for i in s["idx"]] == s["x"]
        if s["round"] == 0:
            assert all(add_nc(w, c) in (v, v + P) and (v < M32 or add_nc(w, c) == v) for w, c, v in zip(s["inp"], RC0, s["x"]))
    for s in C["C"]:
        assert O.permute([w % P for w in s["inp"]]) == s["o"]
    for s in C["D"]:
        assert all(ps.unique(v) for v in s["y"])
        x = ps.sbox_inputs(s["inp"], s["round"])
        assert [ps.sbox(v) for v in x[:len(s["y"])]] == s["y"]
        if s["zh"]:
            assert s["inp"][8:] == [0] * 4 and [add_nc(w, c) % P for w, c in zip(s["inp"], RC0)][:8] == x[:8]
    for s in C["E"]:
        assert all(ps.unique(v) for v in s["sp"])
        x = ps.sbox_inputs(s["inp"], s["round"])
        assert [ps.sbox(x[0])] + x[1:] == s["sp"]


def test_standard_leaf_widths_are_the_circuits():
    from support import gen_circuit, p2v_module
    gc = gen_circuit(12, 4, 0)
    info = p2v_module().VerifierCircuitData.from_json(gc.common, gc.vkey).info
    steps = tuple(2 << a for a in info.step_arity_bits[:info.num_fri_steps])
    assert set(info.leaf_widths + steps) == set(ps.STANDARD_LEAF_WIDTHS)


def test_campaigns_reach_their_branches():
    """the conditions of the device test, by the model alone"""
    C = ps.campaigns()
    ps.check_conditions(C)
    # the final canon subtracts in every output group: words that the device holds as value + p
    sub = [0, 0, 0]
    for s in C["C"]:
        w = ps.final_words(s["inp"])
        if w is not None:
            assert [v % P for v in w] == s["o"]
            for k, v in enumerate(w):
                sub[k // 4] += v >= P
    assert min(sub) >= 8, sub
    # an aimed miss is a miss: no state of E aimed below the threshold carries in its aimed row
    for s in C["E"]:
        R = ps.block_rows(s["sp"], s["round"], s["D"])
        row = R[s["row"]] if isinstance(s["row"], str) else R["out"][s["row"]]
        assert row[1] == s["hit"], s
