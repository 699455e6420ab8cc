"""Exact-integer model of the throughput permutation's leading merged unit (csrc/poseidon.h
`PFTab`, `dv::pblock<3, true>`): full round 3's MDS folded into the first partial rounds.

After round 3's S-boxes (outputs u, Hash/Poseidon.hs:48-52) words 1..11 of M u + rc[4] are used
only linearly until the next materialisation.  With s'_0 = y1 = sbox((M u)_0 + rc[4][0]) and
s'_j = (M u + rc[4])_j (j >= 1), level k of the unit is

    G'_k u + G_k[:,0] y1 + sum_{m=2..k} H_k[:,m] y_m + d'_k,
    G'_k = G_k[:,1:] M[1:,:],   d'_k = G_k[:,1:] rc[4][1:] + d_k (mod p),

with G_k, H_k, d_k those of a block of partial rounds starting at round 4 (test_poseidon_merge.py
`levels`, `dconsts`).  Row 0 of level k < D1 is the S-box input of the unit's round k + 1; level D1
is the state entering round 4 + D1.  Shared by tests/test_poseidon_fold3.py (CPU) and
tests/test_gpu_poseidon_fold3.py.
"""
import test_poseidon_merge as pm

P, M, RC = pm.P, pm.M, pm.RC
M32 = 2**32 - 1
SCHEDULES = {2: [4, 4, 4, 4, 4], 3: [4, 4, 4, 4, 3]}   # D1 -> the ordinary blocks after the leading unit; poseidon.h PF_LEAD = 2


def lead_tables(D1):
    """G'[k], the y1 column Y1[k], H[k][m] (m = 2..k) and d'[k] for k = 1..D1."""
    G, H = pm.levels(D1)
    d = pm.dconsts(4, D1)
    rc4 = RC[48:60]
    Gp = {k: [[sum(G[k][i][l] * M[l][j] for l in range(1, 12)) for j in range(12)] for i in range(12)] for k in range(1, D1 + 1)}
    Y1 = {k: [G[k][i][0] for i in range(12)] for k in range(1, D1 + 1)}
    dp = {k: [(sum(G[k][i][l] * rc4[l] for l in range(1, 12)) + d[k][i]) % P for i in range(12)] for k in range(1, D1 + 1)}
    return Gp, Y1, H, dp


def level_coefs(T, k, i):
    """row i of level k over (u_0..u_11, y1, y_2..y_k)"""
    Gp, Y1, H, _ = T
    return Gp[k][i] + [Y1[k][i]] + [H[k][m][i] for m in range(2, k + 1)]


def row(coefs, vals, dl, dh, wide):
    """One device row: the two accumulators over the 32-bit halves start at the constant's halves
    (dl, dh); then dv::reduce_rows / reduce_t (wide=False: t = al + ah_hi (2^32 - 1), + ah_lo 2^32
    with one wrap fix-up) or dv::reduce_w (wide=True).  Every stated precondition is asserted.
    Returns (value in [0, 2^64), whether the wrap fix-up ran, the larger accumulator)."""
    al, ah = dl, dh
    for c, v in zip(coefs, vals):
        assert 0 <= c < 2**32 and 0 <= v < 2**64
        al += c * (v & M32)
        ah += c * (v >> 32)
    assert al < 2**64 and ah < 2**64                 # the v_mad_u64_u32 chains cannot overflow
    if not wide:
        t = al + (ah >> 32) * M32
        assert t < 2**64                             # madm1_co: no carry
        r = t + ((ah & M32) << 32)
    else:
        lo = al + ((ah & M32) << 32)
        hi = (ah >> 32) + (lo >> 64)
        assert hi < 2**32                            # addc0 stays a 32-bit word
        r = (lo % 2**64) + hi * M32
    carried = r >= 2**64
    if carried:
        r = r - 2**64 + M32
    assert r < 2**64                                 # one wrap fix-up is enough
    return r, carried, max(al, ah)


def lead(u, D1, T=None, rng=None, info=None):
    """The leading unit on the S-box outputs u of round 3 (any values < 2^64) -> the 12 words
    entering round 4 + D1, in [0, 2^64).  rng: S-box outputs get random lazy representatives.
    info (a dict): 'carry' gets the list of rows whose wrap fix-up ran ('y1', 'chain<k>', 'out<i>')."""
    T = T or lead_tables(D1)
    dp = T[3]
    carry = []
    lift = (lambda x: pm.lift(x, rng)) if rng else (lambda x: x)
    z, c, _ = row(M[0], u, RC[48] & M32, RC[48] >> 32, False)
    if c:
        carry.append("y1")
    ys = [lift(pm.sbox(z))]                          # y1, y2, ...
    for k in range(1, D1):
        z, c, _ = row(level_coefs(T, k, 0), list(u) + ys, dp[k][0] & M32, dp[k][0] >> 32, False)
        if c:
            carry.append("chain%d" % k)
        ys.append(lift(pm.sbox(z)))
    out = []
    for i in range(12):
        z, c, _ = row(level_coefs(T, D1, i), list(u) + ys, dp[D1][i] & M32, dp[D1][i] >> 32, D1 == 3)
        if c:
            carry.append("out%d" % i)
        out.append(z)
    if info is not None:
        info["carry"] = carry
    return out


def linear_section(u, D1, rng):
    """rounds 3 (after its S-boxes) .. 25 by the new schedule: u -> the state entering round 26"""
    s = lead(u, D1, rng=rng)
    r = 4 + D1
    for D in SCHEDULES[D1]:
        s = pm.block([pm.lift(x % P, rng) for x in s], r, D, rng)
        r += D
    assert r == 26
    return [x % P for x in s]


def linear_section_plain(u):
    s = [(sum(M[i][j] * u[j] for j in range(12)) + RC[48 + i]) % P for i in range(12)]
    for r in range(4, 26):
        s[0] = pm.sbox(s[0])
        s = [(sum(M[i][j] * s[j] for j in range(12)) + RC[12 * (r + 1) + i]) % P for i in range(12)]
    return s


def perm_fold3(s, D1, rng):
    """the whole permutation as permute_dev runs it: rounds 0..2, round 3's S-boxes, the linear
    section, rounds 26..29"""
    s = [(s[i] + RC[i]) % P for i in range(12)]
    for r in range(3):
        s = [pm.sbox(x) for x in s]
        s = [(sum(M[i][j] * s[j] for j in range(12)) + RC[12 * (r + 1) + i]) % P for i in range(12)]
    u = [pm.lift(pm.sbox(x), rng) for x in s]
    s = linear_section(u, D1, rng)
    for r in range(26, 30):
        s = [pm.sbox(x) for x in s]
        s = [(sum(M[i][j] * s[j] for j in range(12)) + (RC[12 * (r + 1) + i] if r < 29 else 0)) % P for i in range(12)]
    return s


def edge_states():
    """u at the edges: all words 0, 1, p - 1, 2^64 - 1; single words at 2^64 - 1 over zeros and
    over p - 1; lazy representatives x + p of small x"""
    top = 2**64 - 1
    st = [[v] * 12 for v in (0, 1, P - 1, top, P, P + 1, 2**32 - 1, 2**32, top - 2**32)]
    for j in range(12):
        for base in (0, P - 1):
            s = [base] * 12
            s[j] = top
            st.append(s)
    return st
