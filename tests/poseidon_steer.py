"""Steering the Poseidon permutation (Hash/Poseidon.hs:42-101) to chosen inner-round and output
states, in exact integers.

The permutation is a bijection and every round inverts: the S-box x -> x^7 with the exponent
7^-1 mod (p - 1), the MDS layer with its inverse matrix over F_p.  So the S-box inputs of any round,
and the output state, can be chosen and the input found by running backwards; the device code
(csrc/poseidon.h `permute_dev`) then meets the chosen values in that round, where random inputs
never put them.  P, M and RC are test_poseidon_merge's.

Representatives.  The device keeps lazy 64-bit values; what its rare branches do depends on the
64-bit value, not on the field element.  A canonical x >= 2^32 - 1 has exactly one 64-bit
representative (x + p >= 2^64), so the device holds x itself wherever the field element is x.  Every
word whose high half a crafted state relies on is therefore asserted to be >= 2^32 - 1 (`unique`),
and smaller S-box edge inputs are counted under either representative (`sbox_neg`).

Besides the steering this restates, each with its source lines, what decides the rare branches:
the `neg` predicate of the S-box multiply (`mul_dev`) and the carry of the branch-form row
reductions (`row_carry`).  `campaigns()` builds the steered states of tests/test_poseidon_steer.py
(which proves their coverage from these models alone) and tests/test_gpu_poseidon_steer.py (which
runs them on the device), once.
"""
import random
from functools import lru_cache

import test_poseidon_merge as pm
from support import preimage_round0, sbox_edge_values

P, M, RC = pm.P, pm.M, pm.RC
M32 = 2**32 - 1
M64 = 2**64 - 1
SINV = pow(7, -1, P - 1)
OUT_EDGES = [0, 1, 2**32 - 2, 2**32 - 1, 2**32, P - 2, P - 1]
# the leaves the standard circuit (2^12 rows, arity-16 FRI steps) sponges: its four initial trees' and
# a step tree's of 16 F^2 values (test_poseidon_steer.py holds them against the circuit's own)
STANDARD_LEAF_WIDTHS = (85, 135, 20, 16, 32)


def is_full(r):
    return r < 4 or r >= 26


def rc(r):
    return RC[12 * r:12 * r + 12]


def sbox(x):
    return pow(x, 7, P)


def sbox_inv(y):
    return pow(y, SINV, P)


def solve_mod_p(A, b):
    """x with A x = b over F_p (A square), or None when A is singular."""
    n = len(A)
    A = [list(row) + [v] for row, v in zip(A, b)]
    for c in range(n):
        piv = next((r for r in range(c, n) if A[r][c] % P), None)
        if piv is None:
            return None
        A[c], A[piv] = A[piv], A[c]
        inv = pow(A[c][c], -1, P)
        A[c] = [x * inv % P for x in A[c]]
        for r in range(n):
            if r != c and A[r][c]:
                f = A[r][c]
                A[r] = [(x - f * y) % P for x, y in zip(A[r], A[c])]
    return [A[r][n] for r in range(n)]


def _mat_inv(A):
    n = len(A)
    cols = [solve_mod_p(A, [int(i == k) for i in range(n)]) for k in range(n)]
    return [[cols[j][i] for j in range(n)] for i in range(n)]


MINV = _mat_inv(M)


def mat_vec(A, s):
    return [sum(a * x for a, x in zip(row, s)) % P for row in A]


def round_fwd(s, r):
    s = [(x + c) % P for x, c in zip(s, rc(r))]
    if is_full(r):
        s = [sbox(x) for x in s]
    else:
        s[0] = sbox(s[0])
    return mat_vec(M, s)


def round_inv(s, r):
    s = mat_vec(MINV, s)
    if is_full(r):
        s = [sbox_inv(x) for x in s]
    else:
        s[0] = sbox_inv(s[0])
    return [(x - c) % P for x, c in zip(s, rc(r))]


def permute(s):
    s = [x % P for x in s]
    for r in range(30):
        s = round_fwd(s, r)
    return s


def permute_inv(o):
    s = [x % P for x in o]
    for r in range(29, -1, -1):
        s = round_inv(s, r)
    return s


def sbox_inputs(s, r):
    """The 12 words of round r after its constants: its S-box inputs (word 0 alone in a partial
    round; words 1..11 pass on unchanged)."""
    s = [x % P for x in s]
    for k in range(r):
        s = round_fwd(s, k)
    return [(x + c) % P for x, c in zip(s, rc(r))]


def steer(r, x):
    """The canonical input whose round-r words after the constants are x: all 12 S-box inputs of a
    full round, the S-box input (word 0) and the 11 free words of a partial one.  For r = 0 it is
    support.preimage_round0 word by word: the device's add_nc then gives x itself when
    x >= 2^32 - 1, x + p otherwise."""
    s = [(v - c) % P for v, c in zip(x, rc(r))]
    for k in range(r - 1, -1, -1):
        s = round_inv(s, k)
    return s


def steer_out(o):
    """The input whose output is o."""
    return permute_inv(o)


ZH = [sbox(c) for c in RC[8:12]]   # poseidon.h make_zh: round 0's S-box outputs of words 8..11 entering as 0


def steer_zh_round0(x8):
    """Words 8..11 enter as 0: the input whose round-0 S-box inputs of words 0..7 are x8 (the 64-bit
    value itself wherever one exists: support.preimage_round0)."""
    return [preimage_round0(v, i, RC[:12]) for i, v in enumerate(x8)] + [0] * 4


def steer_zh_round1(idx, vals):
    """Words 8..11 enter as 0: the input whose round-1 S-box inputs of the 8 words idx are vals.
    Round 0's S-box outputs of words 8..11 are the constants ZH, so those of words 0..7 solve an
    8 x 8 system over F_p; None when it is singular.  Deeper rounds have no such freedom."""
    assert len(idx) == len(vals) == 8
    rhs = [(v - RC[12 + i] - sum(M[i][j] * ZH[j - 8] for j in range(8, 12))) % P for i, v in zip(idx, vals)]
    y = solve_mod_p([[M[i][j] for j in range(8)] for i in idx], rhs)
    return None if y is None else steer_zh_round0([sbox_inv(v) for v in y])


def steer_zh(r, idx, vals):
    """steer under the constraint that words 8..11 enter as 0: round 0 (idx = words 0..7) or 1"""
    assert r in (0, 1), "deeper rounds cannot be steered with words 8..11 fixed: the zh=0 call of the same instance reaches them"
    if r == 0:
        assert list(idx) == list(range(8))
        return steer_zh_round0(vals)
    return steer_zh_round1(idx, vals)


def unique(x):
    """x (canonical) has one 64-bit representative: the device holds x itself"""
    return M32 <= x < P


# ---------------------------------------------------------------- what decides the rare branches
def mul_dev(a, b):
    """gl::mul_nc_dev_v<2> / <3> on 64-bit a, b (csrc/gl.h:117-135): (the 64-bit result, neg).
    product = lo + h0 2^64 + (h1 + cm) 2^96 (gl.h:117-122); t = lo + h0 (2^32 - 1) with carry ct
    (gl.h:128); the subtraction of h1 with borrow-in cm borrows (bw2) iff t mod 2^64 < product >> 96
    (gl.h:129-130); neg = bw2 & ~ct (gl.h:131), i.e. t < 2^64 and t < product >> 96; pos = ct & ~bw2
    adds 2^32 - 1 (gl.h:132), neg adds 2^64 - 2^32 + 1 mod 2^64 (gl.h:134, mul_fix_neg gl.h:157)."""
    prod = a * b
    lo, h0, hi = prod & M64, (prod >> 64) & M32, prod >> 96
    t = lo + h0 * M32
    ct, tm = t > M64, t & M64
    bw = tm < hi
    u = (tm - hi) & M64
    neg = bw and not ct
    assert neg == (t < 2**64 and t < hi)
    if ct and not bw:
        r = u + M32
        assert r <= M64                  # gl.h:132: the MAD's carry c4 is dropped
    elif neg:
        r = (u + P) & M64
    else:
        r = u
    return r, neg


def sbox_dev(v):
    """dv::sbox_n on the 64-bit value v (poseidon.h:374-403): (the 64-bit result, the neg flags of
    the products x^2 (stage 1), x^3 and x^4 (stage 2), x^7 (stage 3))."""
    x2, n2 = mul_dev(v, v)
    x3, n3 = mul_dev(v, x2)
    x4, n4 = mul_dev(x2, x2)
    x7, n7 = mul_dev(x3, x4)
    return x7, (n2, n3 or n4, n7)


def sbox_neg(x):
    """Stages (1..3) of the S-box whose -2^64 fix-up runs for the S-box input x (canonical) under
    every 64-bit representative the device may hold: x alone when x >= 2^32 - 1, else x and x + p."""
    reps = [x] if x >= M32 else [x, x + P]
    sets = [{k + 1 for k, f in enumerate(sbox_dev(v)[1]) if f} for v in reps]
    return set.intersection(*sets)


def row_carry(coefs, vals, k):
    """One branch-form row: dv::row_unfixed / reduce_rows / prow2_unfixed (poseidon.h:304-313,
    327-337, 501-508) over the 64-bit values vals with the constant k's halves starting the two
    accumulators.  t = al + ah_hi (2^32 - 1) (no carry), rh = (t >> 32) + ah_lo with the carry c that
    the fix-up branch tests.  Returns (the 64-bit result, c, ah_lo).  As pm.row and
    poseidon_fold3_model.row model it; this one also returns what a near miss is measured by."""
    al, ah = k & M32, k >> 32
    for c, v in zip(coefs, vals):
        assert 0 <= c < 2**32 and 0 <= v < 2**64
        al += c * (v & M32)
        ah += c * (v >> 32)
    assert al < 2**64 and ah < 2**64
    t = al + (ah >> 32) * M32
    assert t < 2**64
    rh = (t >> 32) + (ah & M32)
    carried = rh > M32
    r = ((rh & M32) << 32) | (t & M32)
    if carried:
        r += M32
    assert r < 2**64
    return r, carried, ah & M32


def mds_consts(r):
    """the constants whose halves start round_pp(r)'s rows: round r + 1's, none after round 29
    (poseidon.h:429-430, RcSplit poseidon.h:116)"""
    return rc(r + 1) if r < 29 else [0] * 12


ZRC = [(RC[12 + i] + sum(M[i][j] * ZH[j - 8] for j in range(8, 12))) % P for i in range(12)]   # poseidon.h make_zrc


def mds_rows(y, k, nw=12):
    """mds_group<.., nw> on the S-box outputs y (64-bit): per row (result, carried, ah_lo)"""
    return [row_carry(M[i][:nw], y[:nw], k[i]) for i in range(12)]


NEAR_MDS = 2**32 - 2**12     # a row sum < 2^9 keeps t >> 32 < 2^11: ah_lo from here on, no carry = a near miss
AIM_MISS_MDS = 2**32 - 2**11
NEAR_BLOCK = 2**32 - 2**21   # chain row 2 and the pblock<2> rows: row sums < 2^17, t >> 32 < 2^18
AIM_MISS_BLOCK = 2**32 - 2**20


def _solve_mod_2_32(A):
    """Gauss-Jordan on the augmented m x (m + 1) system mod 2^32 with odd pivots; None without one."""
    m = len(A)
    for col in range(m):
        piv = next((r for r in range(col, m) if A[r][col] & 1), None)
        if piv is None:
            return None
        A[col], A[piv] = A[piv], A[col]
        inv = pow(A[col][col], -1, 1 << 32)
        A[col] = [(x * inv) & M32 for x in A[col]]
        for r in range(m):
            if r != col and A[r][col]:
                f = A[r][col]
                A[r] = [(x - f * y) & M32 for x, y in zip(A[r], A[col])]
    return [A[r][m] for r in range(m)]


def _rand_unique(rng):
    return rng.randrange(1 << 32, (1 << 64) - (1 << 32))   # high half in [1, 2^32 - 2]: unique and < p


def aim_mds(rng, k, nw=12):
    """S-box outputs y (nw words, each with one representative) of which 1-3 rows of M y + k have
    their high accumulator's low word aimed at 2^32 - 1 (the fix-up runs) or 2^32 - 2^11 (just below
    the threshold), by solving for as many words' high halves mod 2^32 as tests/test_gpu.py
    `_mds_fixup_cases` does for one isolated layer."""
    while True:
        rows = sorted(rng.sample(range(12), rng.randrange(1, 4)))
        cols = sorted(rng.sample(range(nw), len(rows)))
        y = [_rand_unique(rng) for _ in range(nw)]
        target = [M32 if rng.randrange(2) else AIM_MISS_MDS for _ in rows]
        A = [[M[i][j] for j in cols] + [(t - (k[i] >> 32) - sum(M[i][j] * (y[j] >> 32) for j in range(nw) if j not in cols)) & M32]
             for t, i in zip(target, rows)]
        h = _solve_mod_2_32(A)
        if h is None or not all(1 <= v < M32 for v in h):
            continue
        for v, j in zip(h, cols):
            y[j] = (v << 32) | (y[j] & M32)
        assert all(unique(v) for v in y)
        return y


def count_rows(rows, near):
    """(carries, near misses) among (result, carried, ah_lo) rows"""
    return sum(c for _, c, _ in rows), sum((not c) and lo >= near for _, c, lo in rows)


# blocks of merged partial rounds: (entry round, depth) by form (poseidon.h make_pf / make_pm; form 0's
# leading unit, rounds 3..5, is op 22's)
BLOCKS = {0: [(6 + 4 * b, 4) for b in range(5)], 1: [(4 + 4 * b, 4) for b in range(5)] + [(24, 2)]}


def block_rows(sp, r, D):
    """The branch-form rows of dv::pblock<D> (poseidon.h:530-553) entered at round r with s' = sp (y1,
    the block's first S-box output, in word 0): {'chain1': row, 'chain2': row} for D = 4,
    {'chain1': row, 'out': [12 rows]} for D = 2; rows as row_carry's.  Tables as pm.levels /
    pm.dconsts state them (tests/test_poseidon_merge.py checks them against the C++ ones)."""
    G, H = pm.levels(D)
    d = pm.dconsts(r, D)
    z1 = row_carry(M[0], sp, d[1][0])
    y2 = sbox(z1[0] % P)
    if not unique(y2):
        return None
    if D == 2:
        return {"chain1": z1, "out": [row_carry(G[2][i] + [M[i][0]], sp + [y2], d[2][i]) for i in range(12)]}
    return {"chain1": z1, "chain2": row_carry(G[2][0] + [H[2][2][0]], sp + [y2], d[2][0])}


def aim_block(rng, r, D, row, hit):
    """s' entering the block at round r whose row ('chain1', 'chain2', or an output row number of a
    depth-2 block) has its high accumulator's low word at 2^32 - 1 (hit) or below the threshold.
    chain1: word 0's high half is solved (M[0][0] is odd).  The others: a difference d moves between
    the high halves of words 6 and 7, whose MDS row-0 entries are equal, so chain row 1 and y2 stay
    and the aimed row's accumulator moves by (c_6 - c_7) d (tests/test_gpu_poseidon_fold3.py
    `_aim_chain1`); a target of the wrong parity is lowered by one."""
    G, _ = pm.levels(D)
    d = pm.dconsts(r, D)
    while True:
        sp = [_rand_unique(rng) for _ in range(12)]
        if row == "chain1":
            target = M32 if hit else AIM_MISS_MDS
            rest = (d[1][0] >> 32) + sum(M[0][j] * (sp[j] >> 32) for j in range(1, 12))
            h0 = (((target - rest) & M32) * pow(M[0][0], -1, 1 << 32)) & M32
            if not 1 <= h0 < M32:
                continue
            sp[0] = (h0 << 32) | (sp[0] & M32)
        else:
            assert M[0][6] == M[0][7]
            sp[6] &= M32
            sp[7] |= M32 << 32
            y2 = sbox(row_carry(M[0], sp, d[1][0])[0] % P)
            if row == "chain2":
                c, k = G[2][0] + [M[0][0]], d[2][0]
            else:
                c, k = G[2][row] + [M[row][0]], d[2][row]
            ah = (k >> 32) + sum(cj * (v >> 32) for cj, v in zip(c, sp + [y2]))
            g = c[6] - c[7]
            if g == 0:
                return None
            p2 = g & -g
            target = M32 if hit else AIM_MISS_BLOCK
            need = (target - ah) & M32
            if need % p2:
                need -= 1
            if need % p2:
                continue
            dd = ((need // p2) * pow(g // p2, -1, (1 << 32) // p2)) % ((1 << 32) // p2)
            if not 1 <= dd < M32:
                continue
            sp[6] |= dd << 32
            sp[7] -= dd << 32
        if all(unique(v) for v in sp) and block_rows(sp, r, D) is not None:
            return sp


def block_entry(sp):
    """the round's words after its constants for s' = sp: word 0 back through the S-box"""
    return [sbox_inv(sp[0])] + sp[1:]


def final_words(inp):
    """The 64-bit words the throughput form holds before gl::canon (poseidon.h:650-661): round 29's
    mds_group rows on its S-box outputs, or None where one of those has two representatives."""
    y = [sbox(x) for x in sbox_inputs(inp, 29)]
    if not all(unique(v) for v in y):
        return None
    return [r for r, _, _ in mds_rows(y, [0] * 12)]


# ---------------------------------------------------------------- the campaigns
A_PER_ROUND = 32
DE_PER_BRANCH = 36      # hits and as many aimed misses per branch (the condition is >= 32 of each)
D_PER_ROUND = 56
D_ROUNDS = [1, 2, 3, 26, 27, 28, 29]   # round 3 has an MDS layer of its own in form 1 alone


def _campaign_a(rng):
    """S-box edge inputs in every round: A_PER_ROUND states per round, all 12 S-box inputs of a full
    round and word 0 of a partial one from support.sbox_edge_values().  Every full round gets every
    edge value; the partial rounds share them round-robin behind three values per round that take
    the fix-up in stage 1, 2 and 3."""
    ev = sbox_edge_values()
    by_stage = {k: [v for v in ev if k in sbox_neg(v)] for k in (1, 2, 3)}
    out, nxt = [], 0
    for r in range(30):
        if is_full(r):
            pool = ev + [rng.choice(ev) for _ in range(12 * A_PER_ROUND - len(ev))]
            assert len(pool) == 12 * A_PER_ROUND
            rng.shuffle(pool)
            xs = [pool[12 * i:12 * i + 12] for i in range(A_PER_ROUND)]
        else:
            heads = [by_stage[k][r % len(by_stage[k])] for k in (1, 2, 3)]
            rest = [ev[(nxt + i) % len(ev)] for i in range(A_PER_ROUND - 3)]
            nxt += A_PER_ROUND - 3
            xs = [[v] + [rng.randrange(P) for _ in range(11)] for v in heads + rest]
        out += [{"round": r, "x": x, "inp": steer(r, x)} for x in xs]
    return out


def _campaign_b(rng):
    """zh forms: round-0 edge inputs on words 0..7, and 8 steered S-box inputs of round 1"""
    ev = sbox_edge_values()
    pool = ev + [rng.choice(ev) for _ in range(-len(ev) % 8)]
    rng.shuffle(pool)
    out = [{"round": 0, "idx": list(range(8)), "x": pool[k:k + 8], "inp": steer_zh(0, range(8), pool[k:k + 8])}
           for k in range(0, len(pool), 8)]
    pool = ev + [rng.choice(ev) for _ in range(-len(ev) % 8)]
    rng.shuffle(pool)
    for k in range(0, len(pool), 8):
        while True:
            idx = sorted(rng.sample(range(12), 8))
            inp = steer_zh(1, idx, pool[k:k + 8])
            if inp is not None:
                break
        out.append({"round": 1, "idx": idx, "x": pool[k:k + 8], "inp": inp})
    return out


def _campaign_c(rng):
    """Outputs at the canonical edges: every edge value in every word position among other edge
    values (7 rotations), alone among random words (84 states), and small values (whose 64-bit word
    before canon may be the value + p) in whole groups."""
    n = len(OUT_EDGES)
    outs = [[OUT_EDGES[(k + t) % n] for k in range(12)] for t in range(n)]
    for k in range(12):
        for v in OUT_EDGES:
            o = [rng.randrange(P) for _ in range(12)]
            o[k] = v
            outs.append(o)
    for _ in range(48):
        outs.append([rng.choice([0, 1, 2, 2**32 - 2, rng.randrange(2**32 - 1)]) if rng.randrange(3) else rng.randrange(P)
                     for _ in range(12)])
    return [{"o": o, "inp": steer_out(o)} for o in outs]


def _campaign_d(rng):
    """The MDS carry in the inner full rounds, and in the peeled round 0 of the zh forms (c_zrc)."""
    out = []
    for r in D_ROUNDS:
        for _ in range(D_PER_ROUND):
            y = aim_mds(rng, mds_consts(r))
            out.append({"round": r, "zh": False, "y": y, "inp": steer(r, [sbox_inv(v) for v in y])})
    for _ in range(D_PER_ROUND):
        y = aim_mds(rng, ZRC, 8)
        out.append({"round": 0, "zh": True, "y": y, "inp": steer_zh_round0([sbox_inv(v) for v in y])})
    return out


def _campaign_e(rng):
    """The branch-form rows of the merged blocks: chain rows 1 and 2 of every depth-4 block of both
    forms, chain row 1 and the 12 group rows of form 1's depth-2 block."""
    out = []
    for form in (0, 1):
        for r, D in BLOCKS[form]:
            rows = ["chain1", "chain2"] if D == 4 else ["chain1"] + list(range(12))
            for row in rows:
                per = DE_PER_BRANCH if isinstance(row, str) else 3
                for hit in (True, False):
                    for _ in range(per):
                        sp = aim_block(rng, r, D, row, hit)
                        if sp is None:
                            continue
                        out.append({"form": form, "round": r, "D": D, "row": row, "hit": hit, "sp": sp,
                                    "inp": steer(r, block_entry(sp))})
    return out


@lru_cache(maxsize=1)
def campaigns():
    rng = random.Random(2324)
    return {"A": _campaign_a(rng), "B": _campaign_b(rng), "C": _campaign_c(rng), "D": _campaign_d(rng), "E": _campaign_e(rng)}


def coverage_a(states):
    """per round: how many of the steered S-box inputs take the -2^64 fix-up in stage 1, 2, 3, under
    whichever representative the device holds"""
    cov = {r: [0, 0, 0] for r in range(30)}
    for s in states:
        for x in (s["x"] if is_full(s["round"]) else s["x"][:1]):
            for k in sbox_neg(x):
                cov[s["round"]][k - 1] += 1
    return cov


def coverage_d(states):
    """(round, zh) -> (carries, near misses) of the aimed layer, by row_carry"""
    cov = {}
    for s in states:
        rows = mds_rows(s["y"], ZRC, 8) if s["zh"] else mds_rows(s["y"], mds_consts(s["round"]))
        h, m = count_rows(rows, NEAR_MDS)
        key = (s["round"], s["zh"])
        cov[key] = (cov.get(key, (0, 0))[0] + h, cov.get(key, (0, 0))[1] + m)
    return cov


def coverage_e(states):
    """(form, entry round, 'chain1' | 'chain2' | 'out') -> (carries, near misses) of that row, by
    block_rows; a depth-2 block's 12 output rows count together, being one branch per group"""
    cov = {}
    for s in states:
        R = block_rows(s["sp"], s["round"], s["D"])
        name = s["row"] if isinstance(s["row"], str) else "out"
        rows = R["out"] if name == "out" else [R[name]]
        h, m = count_rows(rows, NEAR_MDS if name == "chain1" else NEAR_BLOCK)
        key = (s["form"], s["round"], name)
        cov[key] = (cov.get(key, (0, 0))[0] + h, cov.get(key, (0, 0))[1] + m)
    return cov


def check_conditions(C):
    """The coverage the campaigns owe, from the models above alone (no device): asserted by the CPU
    test and again beside the device compare."""
    ev = sbox_edge_values()
    # A: the -2^64 fix-up in every round, in stage 2 too (x^3, x^4: two of the four products); every
    # edge value in a full round >= 1 and in a partial round
    cov = coverage_a(C["A"])
    assert all(sum(cov[r]) > 0 and cov[r][1] > 0 for r in range(30)), cov
    in_full = {x for s in C["A"] if is_full(s["round"]) and s["round"] >= 1 for x in s["x"]}
    in_part = {s["x"][0] for s in C["A"] if not is_full(s["round"])}
    assert set(ev) <= in_full and set(ev) <= in_part
    assert all(sum(s["round"] == r for s in C["A"]) == A_PER_ROUND for r in range(30))
    # C: every edge value in every word position
    assert all(any(s["o"][k] == v for s in C["C"]) for k in range(12) for v in OUT_EDGES)
    # D: >= 32 carries and >= 32 near misses per aimed layer (the states serve forms 0 and 1 alike;
    # round 3 counts for form 1)
    cov = coverage_d(C["D"])
    assert sorted(cov) == sorted([(r, False) for r in D_ROUNDS] + [(0, True)])
    assert all(h >= 32 and m >= 32 for h, m in cov.values()), cov
    # E: the same per branch-form row of every block of each form
    cov = coverage_e(C["E"])
    want = [(f, r, row) for f in (0, 1) for r, D in BLOCKS[f] for row in (("chain1", "chain2") if D == 4 else ("chain1", "out"))]
    assert sorted(cov) == sorted(want)
    assert all(h >= 32 and m >= 32 for h, m in cov.values()), cov
    assert sum(len(v) for v in C.values()) <= 4000
