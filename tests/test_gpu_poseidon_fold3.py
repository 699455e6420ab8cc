"""The throughput permutation's leading merged unit on the device (p2v_selftest op 22: full round
3's MDS folded into partial rounds 4-5, csrc/poseidon.h `dv::pblock<3, true>`) against the
exact-integer model of poseidon_fold3_model.py, and the whole device permutation (ops 1 and 2)
against the oracle's (Hash/Poseidon.hs:42-46)."""
import numpy as np
import pytest

import poseidon_fold3_model as f3
from support import oracle, p2v_module

pytestmark = pytest.mark.gpu

P, M, RC = f3.P, f3.M, f3.RC
M32 = f3.M32
D1 = 2   # poseidon.h PF_LEAD


@pytest.fixture(scope="module")
def p2v():
    # torch first, then libp2v: the order test_gpu.py, bench.py and smoke() use
    import torch
    assert torch.cuda.is_available(), "torch sees no GPU"
    m = p2v_module()
    if m.device_count() == 0:
        pytest.fail("no GPU visible to libp2v")
    return m


def _aim_y1_row(u, target):
    """word 0's high half such that the y1 row's high accumulator ends in `target` (mod 2^32)"""
    rest = (RC[48] >> 32) + sum(M[0][j] * (u[j] >> 32) for j in range(1, 12))
    u[0] = ((((target - rest) & M32) * pow(M[0][0], -1, 1 << 32)) & M32) << 32 | (u[0] & M32)


def _aim_chain1(u, T, target):
    """Moves d between the high halves of words 6 and 7, whose entries in MDS row 0 are equal:
    the y1 row's accumulators, and so y1, stay what they were, and chain row 1's high accumulator
    moves by (G'_1[0][6] - G'_1[0][7]) d.  Returns False when `target` has the wrong parity."""
    assert M[0][6] == M[0][7]
    u[6] &= M32
    u[7] |= M32 << 32
    c = f3.level_coefs(T, 1, 0)
    y1 = f3.pm.sbox(f3.row(M[0], u, RC[48] & M32, RC[48] >> 32, False)[0])
    ah = (T[3][1][0] >> 32) + sum(cj * (v >> 32) for cj, v in zip(c, list(u) + [y1]))
    g = c[6] - c[7]
    k = g & -g                                                   # the power of two in g
    need = (target - ah) & M32
    if need % k:
        return False
    d = ((need // k) * pow(g // k, -1, (1 << 32) // k)) % ((1 << 32) // k)
    u[6] |= d << 32
    u[7] -= d << 32
    return True


def _crafted(rng, T, n):
    """u whose y1 row or chain row 1 (the two rare-carry branch reductions of the unit) has its
    high accumulator's low word at 2^32 - 1 / 2^32 - 2 (the fix-up runs) or far below the
    threshold (it does not), mixed so that lanes of one wave differ."""
    out = []
    while len(out) < n:
        u = [int(x) for x in rng.integers(0, 1 << 64, 12, dtype=np.uint64)]
        kind = len(out) % 4
        if kind == 0:
            _aim_y1_row(u, M32)
        elif kind == 1:
            _aim_y1_row(u, (1 << 32) - (1 << 12))                # row sums < 2^9: t >> 32 < 2^12 is below it
        elif not (_aim_chain1(u, T, M32 if kind == 2 else (1 << 32) - (1 << 20)) or
                  _aim_chain1(u, T, M32 - 1 if kind == 2 else (1 << 32) - (1 << 20) - 1)):
            continue
        out.append(u)
    return out


def test_gpu_leading_unit_vs_exact_model(p2v):
    """4 096 states through op 22: random u, the edge u (0, 1, p - 1, 2^64 - 1, single words at
    2^64 - 1, lazy representatives) and crafted u that take the carry fix-up of the y1 row and of
    chain row 1 in some lanes of a wave and not in others; the output rows' branch-free fix-up
    runs in hundreds of random rows.  Compared mod p with the model (the device's S-box outputs
    are lazy representatives of the model's)."""
    rng = np.random.default_rng(22)
    T = f3.lead_tables(D1)
    states = f3.edge_states()
    crafted = _crafted(rng, T, 512)
    states += crafted
    states += [[int(x) for x in r] for r in rng.integers(0, 1 << 64, size=(4096 - len(states), 12), dtype=np.uint64)]
    assert len(states) == 4096
    order = rng.permutation(4096)                                # crafted and random lanes share waves
    states = [states[i] for i in order]
    out = p2v.device_selftest(22, np.array(states, dtype=np.uint64))
    fired = {"y1": 0, "chain1": 0, "out": 0}
    for u, o in zip(states, out):
        info = {}
        exp = [x % P for x in f3.lead(u, D1, T, info=info)]
        assert [int(x) for x in o] == exp, [hex(x) for x in u]
        for name in info["carry"]:
            fired[name[:3] if name.startswith("out") else name] += 1
    # the branch forms really ran on both sides: 128 crafted hits and 128 near misses each
    assert 120 <= fired["y1"] <= 136 and 120 <= fired["chain1"] <= 136, fired
    assert fired["out"] > 50, fired


def test_gpu_permutation_forms_vs_oracle(p2v):
    """ops 1 and 2 (the generic and the compression form of permute_dev) on 2^15 random states
    and the KAT against the oracle's permutation"""
    from support import KAT_IN, KAT_OUT
    O = oracle()
    rng = np.random.default_rng(23)
    a = np.concatenate([np.array([KAT_IN], dtype=np.uint64), rng.integers(0, 1 << 64, size=(1 << 15, 12), dtype=np.uint64)])
    full = p2v.device_selftest(1, a)
    comp = p2v.device_selftest(2, a)
    assert [int(x) for x in full[0]] == KAT_OUT
    for i, st in enumerate(a.tolist()):
        assert full[i].tolist() == O.permute([x % P for x in st]), i
        assert comp[i][:4].tolist() == O.permute([x % P for x in st[:8]] + [0] * 4)[:4], i
