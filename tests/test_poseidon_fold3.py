"""Full round 3's MDS folded into the first merged partial-round unit of the throughput
permutation (csrc/poseidon.h `PFTab`, `make_pf`, `dv::pblock<3, true>`; model and formulas in
poseidon_fold3_model.py).  In exact integer arithmetic:
  * the algebra: the new schedule, leading unit + ordinary blocks, equals rounds 3..25 of the plain
    permutation (Hash/Poseidon.hs:48-60) from random and edge S-box outputs u, lazy
    representatives included, and the whole restated permutation equals the KAT
    (Hash/Poseidon.hs:27-35); the device's row reductions are modelled bit for bit;
  * the bounds: with every 32-bit half at 2^32 - 1 every accumulator of every row stays below
    2^64 and each reduction's precondition holds; the maxima are those of today's blocks of
    depth 3 and 4;
  * the tables the device reads (dumped on the host by tools/pf_dump.cpp) equal the model's.
"""
import json
import math
import os
import random
import shutil
import subprocess

import pytest

import poseidon_fold3_model as f3

pm = f3.pm
P, M, RC = f3.P, f3.M, f3.RC
TOP = 2**64 - 1


@pytest.mark.parametrize("D1", [2, 3])
def test_restated_permutation_matches_kat_and_plain(D1):
    rng = random.Random(30 + D1)
    assert f3.perm_fold3(list(range(12)), D1, rng) == pm.KAT
    for _ in range(12):
        s = [rng.randrange(P) for _ in range(12)]
        assert f3.perm_fold3(s, D1, rng) == pm.perm_plain(s)


@pytest.mark.parametrize("D1", [2, 3])
def test_new_schedule_equals_rounds_3_to_25(D1):
    rng = random.Random(40 + D1)
    states = f3.edge_states()
    states += [[rng.randrange(2**64) for _ in range(12)] for _ in range(24)]
    states += [[pm.lift(rng.randrange(2**33), rng) for _ in range(12)] for _ in range(8)]   # x and x + p
    for u in states:
        assert f3.linear_section(u, D1, rng) == f3.linear_section_plain(u), u


@pytest.mark.parametrize("D1,levels,coef,rowsum", [(2, 2, 20.38, 23.85), (3, 3, 28.24, 31.72)])
def test_leading_unit_rows_cannot_overflow(D1, levels, coef, rowsum):
    """worst case: every input half 2^32 - 1 (u and every y at 2^64 - 1) and every constant half
    2^32 - 1; row() asserts the accumulators and each reduction's precondition"""
    T = f3.lead_tables(D1)
    assert levels == D1                                           # M3 + D1 partial rounds: D1 levels
    acc = f3.row(M[0], [TOP] * 12, f3.M32, f3.M32, False)[2]      # the y1 row
    assert acc < 2**44
    big_c = big_s = 0
    for k in range(1, D1 + 1):
        for i in (range(12) if k == D1 else [0]):
            c = f3.level_coefs(T, k, i)
            f3.row(c, [TOP] * len(c), f3.M32, f3.M32, wide=(D1 == 3 and k == D1))
            big_c, big_s = max(big_c, max(c)), max(big_s, sum(c))
    assert round(math.log2(big_c), 2) == coef and round(math.log2(big_s), 2) == rowsum
    # the same maxima as today's block of depth D1 + 1, every y column included
    G, H = pm.levels(D1 + 1)
    D = D1 + 1
    assert big_c == max(max(max(r) for r in G[D]), max(max(H[D][m]) for m in H[D]))
    assert big_s == max(sum(G[D][i]) + sum(H[D][m][i] for m in H[D]) for i in range(12))
    # chain level 1 (and the y1 row) use the rare-carry branch form dv::reduce_rows: t < 2^49
    assert sum(f3.level_coefs(T, 1, 0)) < 2**17
    if D1 == 2:   # output rows through dv::reduce_t: row sums < 2^24
        assert big_s < 2**24


def test_cpp_tables_match_model(tmp_path):
    """tools/pf_dump.cpp prints make_pf's tables.  The leading unit's PBlock: d[0] = rc[4][0] (the y1
    row); chain level k = 1..D1-1 at cf[k-1] (G'_k row 0, then the y1 column G_k[0][0] and
    H_k[m][0], m < k, from [12]; the newest y takes its MDS entry inline) with d'_k[0] at d[k];
    output row i at cf[2+i] (G'_D1 row i, G_D1[i][0], H_D1[m][i] for m < D1) with d'_D1[i] at
    d[4+i].  The ordinary blocks are laid out as test_poseidon_merge.py states, from round 4 + D1."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    root = os.path.join(os.path.dirname(__file__), "..")
    exe = str(tmp_path / "pf_dump")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-o", exe, os.path.join(root, "tools", "pf_dump.cpp")],
                          stderr=subprocess.DEVNULL)
    dump = json.loads(subprocess.check_output([exe]))
    D1 = dump["lead_rounds"]
    assert D1 in f3.SCHEDULES and len(dump["blocks"]) == len(f3.SCHEDULES[D1])
    T = f3.lead_tables(D1)
    Gp, Y1, H, dp = T
    cf, dd = dump["lead"]["cf"], dump["lead"]["d"]
    assert dd[0] == RC[48]
    for k in range(1, D1):
        ycols = ([Y1[k][0]] + [H[k][m][0] for m in range(2, k)]) if k > 1 else []   # level 1: y1 is the newest, inline
        assert cf[k - 1][:12] == Gp[k][0] and cf[k - 1][12:12 + len(ycols)] == ycols, k
        assert dd[k] == dp[k][0], k
    for i in range(12):
        ycols = [Y1[D1][i]] + [H[D1][m][i] for m in range(2, D1)]
        assert cf[2 + i][:12] == Gp[D1][i] and cf[2 + i][12:12 + len(ycols)] == ycols, i
        assert H[D1][D1][i] == M[i][0]                            # the newest y's inline entry
        assert dd[4 + i] == dp[D1][i], i
    r = 4 + D1
    for D, blk in zip(f3.SCHEDULES[D1], dump["blocks"]):
        G, Hb = pm.levels(D)
        d = pm.dconsts(r, D)
        cf, dd = blk["cf"], blk["d"]
        for k in range(1, D):
            assert dd[k - 1] == d[k][0], (r, k)
        for k in range(2, D):
            assert cf[k - 2][:12] == G[k][0]
            assert cf[k - 2][12:12 + k - 2] == [Hb[k][m][0] for m in range(2, k)]
        for i in range(12):
            assert cf[2 + i][:12] == G[D][i], (r, i)
            assert cf[2 + i][12:12 + D - 2] == [Hb[D][m][i] for m in range(2, D)]
            assert dd[4 + i] == d[D][i]
        r += D
    assert r == 26
