"""A second, independent restatement of the Fiat-Shamir transcript, the FRI query rounds and
the Plonk identity's permutation part, checked against the oracle.

The oracle (oracle/oracle.c) and the GPU kernels share one author's reading of the reference.
This file is a literal Python transliteration of the transcript, written clause by clause
from the Haskell and sharing no code with either. The only shared piece is the Poseidon
permutation, taken from the oracle and pinned by the reference's KAT (Hash/Poseidon.hs:27-35).
It re-derives every challenge of the golden fixtures straight from their JSON and requires the
oracle's trace words to match:

- public-input hash
- betas, gammas, alphas
- lookup deltas
- zeta
- FRI alpha and betas
- PoW response
- query indices

The FRI part (below) restates combineInitial, the coset folding by the reference's own
interpolation, and the final polynomial, and checks every query's values.

test_gpu pins the GPU trace to the oracle word for word, so this check covers the device
transcript and FRI values as well. Pure Python loops, small cases only; CPU suite."""
import gzip
import json
import os

import pytest

from support import GOLDEN, P, oracle

RATE = 8


def F(x):
    """JSON numbers are Integers reduced mod p (Algebra/Goldilocks.hs:101-102)."""
    return int(x) % P


def permutation(state):
    return oracle().permute(list(state))


# ---- Hash/Sponge.hs:26-31: overwrite mode, no padding, [] -> zero digest
def sponge(xs):
    state = [0] * 12
    while xs:
        this, xs = xs[:8], xs[8:]
        state = permutation(this + state[len(this):])
    return state[:4]


# ---- Challenge/Pure.hs:27-107.  A mode is ("A", old, inp) or ("S", old, out).
def overwrite(new, old):
    return new + old[len(new):]


def duplex(inp, old):
    return permutation(overwrite(inp, old))


def extract(state):
    return list(reversed(state[:RATE]))


def fresh_squeezing(new):
    return ("S", new, extract(new))


def absorb_felt(x, mode):
    if mode[0] == "S":
        return absorb_felt(x, ("A", mode[1], []))
    _, old, inp = mode
    if len(inp) < RATE:
        return ("A", old, inp + [x])
    return absorb_felt(x, ("A", duplex(inp, old), []))


def squeeze_felt(mode):
    kind, old, lst = mode
    if kind == "S":
        if not lst:
            return squeeze_felt(fresh_squeezing(permutation(old)))
        return lst[0], ("S", old, lst[1:])
    if not lst:
        return squeeze_felt(fresh_squeezing(permutation(old)))
    return squeeze_felt(fresh_squeezing(duplex(lst, old)))


class Duplex:
    def __init__(self):
        self.mode = ("A", [0] * 12, [])           # zeroState, no domain separator

    def absorb(self, xs):                         # instance Absorb [a]: left to right
        for x in xs:
            self.mode = absorb_felt(x, self.mode)

    def squeeze(self):
        x, self.mode = squeeze_felt(self.mode)
        return x

    def squeeze_n(self, n):
        return [self.squeeze() for _ in range(n)]

    def squeeze_ext(self):                        # instance Squeeze GoldilocksExt: (re, im)
        return [self.squeeze(), self.squeeze()]


def cap(c):
    """instance Absorb MerkleCap / Digest: the digests' elements in order."""
    return [F(x) for d in c for x in d["elements"]]


def ext_list(xs):
    """instance Absorb FExt: [re, im]."""
    return [F(v) for e in xs for v in e]


def proof_challenges(common, vkey, pwpi):
    """Challenge/Verifier.hs:58-103 followed by Challenge/FRI.hs:65-104."""
    cfg = common["config"]
    r = cfg["num_challenges"]
    has_lookup = common["num_lookup_polys"] > 0
    proof = pwpi["proof"]
    pi_hash = sponge([F(x) for x in pwpi["public_inputs"]])
    d = Duplex()
    d.absorb([F(x) for x in vkey["circuit_digest"]["elements"]])
    d.absorb(pi_hash)
    d.absorb(cap(proof["wires_cap"]))
    betas = d.squeeze_n(r)
    gammas = d.squeeze_n(r)
    deltas = []
    if has_lookup:
        deltas = betas + gammas + d.squeeze_n(2 * r)   # mkLookupDeltaList: chunks of 4
    d.absorb(cap(proof["plonk_zs_partial_products_cap"]))
    alphas = d.squeeze_n(r)
    d.absorb(cap(proof["quotient_polys_cap"]))
    zeta = d.squeeze_ext()
    # friChallenges, Challenge/FRI.hs:65-104; toFriOpenings order :46-61
    o = proof["openings"]
    batch_this = sum((o[k] for k in ("constants", "plonk_sigmas", "wires", "plonk_zs", "partial_products",
                                      "quotient_polys", "lookup_zs")), [])
    batch_next = o["plonk_zs_next"] + o["lookup_zs_next"]
    d.absorb(ext_list(batch_this))
    d.absorb(ext_list(batch_next))
    fri_alpha = d.squeeze_ext()
    fp = proof["opening_proof"]
    fri_betas = []
    for c in fp["commit_phase_merkle_caps"]:
        d.absorb(cap(c))
        fri_betas += d.squeeze_ext()
    d.absorb(ext_list(fp["final_poly"]["coeffs"]))
    d.absorb([F(fp["pow_witness"])])
    pow_response = d.squeeze()
    lde_size = 1 << (common["fri_params"]["degree_bits"] + cfg["fri_config"]["rate_bits"])
    qidx = [x % lde_size for x in d.squeeze_n(cfg["fri_config"]["num_query_rounds"])]
    return {"pi_hash": pi_hash, "betas": betas, "gammas": gammas, "alphas": alphas, "deltas": deltas,
            "zeta": zeta, "fri_alpha": fri_alpha, "fri_betas": fri_betas, "pow_response": [pow_response],
            "qidx": qidx}


def _fixtures():
    with open(os.path.join(GOLDEN, "expected.json")) as f:
        cases = json.load(f)["cases"]

    def rd(name):
        with gzip.open(os.path.join(GOLDEN, name), "rb") as f:
            return f.read()
    return cases, rd


def test_sponge_of_nothing_is_zero_digest():
    assert sponge([]) == [0, 0, 0, 0]            # Hash/Sponge.hs:28, #PI = 0 -> pi_hash = 0^4


@pytest.mark.parametrize("idx", range(len(_fixtures()[0])))
def test_literal_transcript_matches_oracle_trace(idx):
    cases, rd = _fixtures()
    case = cases[idx]
    common_b, vkey_b = rd(case["circuit"] + "_common.json.gz"), rd(case["circuit"] + "_vkey.json.gz")
    proof_b = rd(case["name"] + "_proof.json.gz")
    common, vkey, pwpi = json.loads(common_b), json.loads(vkey_b), json.loads(proof_b)
    ch = proof_challenges(common, vkey, pwpi)
    _, tr = oracle().verify_json(common_b, vkey_b, proof_b, trace=True)
    tr = [int(x) for x in tr]
    r = common["config"]["num_challenges"]
    S = len(pwpi["proof"]["opening_proof"]["commit_phase_merkle_caps"])
    Q = common["config"]["fri_config"]["num_query_rounds"]
    # trace layout: include/p2v.h (off_pi_hash .. off_query_idx)
    k = 0
    got = {}
    for name, n in (("pi_hash", 4), ("betas", r), ("gammas", r), ("alphas", r), ("deltas", 4 * r), ("zeta", 2),
                    ("fri_alpha", 2), ("fri_betas", 2 * S), ("pow_response", 1), ("qidx", Q)):
        got[name] = tr[k:k + n]
        k += n
    if not ch["deltas"]:
        ch["deltas"] = [0] * (4 * r)                # zero when the circuit has no lookups
    for name in got:
        assert got[name] == ch[name], (case["name"], name)


# ---------------------------------------------------------------------------------------------
# FRI query rounds, the same way: a literal restatement of Plonk/FRI.hs:128-327 (combineInitial,
# prepareCoset, foldCosetWith by the reference's own O(arity^2) interpolation with
# pow_ x (-k), foldingStep, the final polynomial), checked against the oracle's per-query
# trace words (combineInitial value, value after the last fold, final-polynomial value).
# The oracle folds by a 16-point iDFT instead, so the two share no folding code.

def fmul(a, b):
    return a * b % P


def finv(a):                                       # inv x = x^(p-2): inv 0 = 0 (Goldilocks.hs:155-156)
    return pow(a, P - 2, P)


def fpow(x, e):                                    # pow with negative exponents (Goldilocks.hs:166-169)
    return pow(finv(x), -e, P) if e < 0 else pow(x, e, P)


def emul(x, y):                                    # F[X]/(X^2 - 7) (GoldilocksExt.hs:54-100)
    return ((x[0] * y[0] + 7 * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def eadd(x, y):
    return ((x[0] + y[0]) % P, (x[1] + y[1]) % P)


def esub(x, y):
    return ((x[0] - y[0]) % P, (x[1] - y[1]) % P)


def escale(s, x):
    return (s * x[0] % P, s * x[1] % P)


def einv(x):
    n = (x[0] * x[0] - 7 * x[1] * x[1]) % P
    ni = finv(n)
    return (x[0] * ni % P, (-x[1]) * ni % P)


def epow(x, e):
    r, b = (1, 0), x
    while e:
        if e & 1:
            r = emul(r, b)
        b = emul(b, b)
        e >>= 1
    return r


def reduce_with_powers(alpha, xs):                 # sum alpha^i x_i (Goldilocks.hs:180-183)
    acc = (0, 0)
    for x in reversed(xs):
        acc = eadd(x, emul(alpha, acc))
    return acc


def roots_of_unity():                              # Goldilocks.hs:69-71: [h^(2^(32-k)) | k <- 0..32]
    h, out = 0x64fdd1a46201e246, []
    x = h
    while x != 1:
        out.append(x)
        x = x * x % P
    out.append(1)
    return list(reversed(out))


ROOTS = roots_of_unity()
MUL_GEN = 0xc65c18b67785d900


def rev_bits(n, i):                                # FFT.hs:20-25
    return int(format(i, f"0{n}b")[::-1], 2) if n else 0


def fold_coset(beta, arity_bits, offset, xs):      # foldCosetWith, Plonk/FRI.hs:262-279
    arity = 1 << arity_bits
    omega = ROOTS[arity_bits]
    ys = []
    for k in range(arity):
        acc = (0, 0)
        for j in range(arity):
            x_omega_j = fmul(offset, fpow(omega, j))
            acc = eadd(acc, escale(fpow(x_omega_j, -k), xs[j]))
        ys.append(acc)
    tot, bk = (0, 0), (1, 0)
    for y in ys:
        tot = eadd(tot, emul(bk, y))
        bk = emul(bk, beta)
    return escale(finv(arity), tot)


def fri_query_values(common, pwpi, ch):
    """Per query: (combineInitial, value after the last folding step, final polynomial at x)."""
    cfg = common["config"]
    r = cfg["num_challenges"]
    qdf = common["quotient_degree_factor"]
    npp = -(-cfg["num_routed_wires"] // qdf)
    logn = common["fri_params"]["degree_bits"]
    logn_lde = logn + cfg["fri_config"]["rate_bits"]
    proof = pwpi["proof"]
    o = proof["openings"]
    ext = lambda xs: [(F(a), F(b)) for a, b in xs]
    alpha = tuple(ch["fri_alpha"])
    zeta = tuple(ch["zeta"])
    y0 = reduce_with_powers(alpha, ext(sum((o[k] for k in ("constants", "plonk_sigmas", "wires", "plonk_zs",
                                                          "partial_products", "quotient_polys", "lookup_zs")), [])))
    y1 = reduce_with_powers(alpha, ext(o["plonk_zs_next"] + o["lookup_zs_next"]))
    strat = cfg["fri_config"]["reduction_strategy"]
    arities = []
    if "ConstantArityBits" in strat:               # expandReductionStrategy :341-352
        a, fbits = strat["ConstantArityBits"]
        lg = logn
        while lg > fbits:
            arities.append(a)
            lg -= a
    else:
        arities = list(strat["Fixed"])
    betas = [tuple(ch["fri_betas"][2 * i:2 * i + 2]) for i in range(len(arities))]
    fp = proof["opening_proof"]
    final_coeffs = ext(fp["final_poly"]["coeffs"])
    out = []
    for q, qr in enumerate(fp["query_round_proofs"]):
        idx = ch["qidx"][q]
        leaves = [[F(x) for x in lp[0]] for lp in qr["initial_trees_proof"]["evals_proofs"]]
        consts, wires, pp_lookup, quot = leaves
        pp, lookup = pp_lookup[:r * npp], pp_lookup[r * npp:]
        first = consts + wires + pp + quot + lookup              # combineInitial :170-185
        second = pp[:r] + lookup
        g0 = reduce_with_powers(alpha, [(x, 0) for x in first])
        g1 = reduce_with_powers(alpha, [(x, 0) for x in second])
        omega, eta = ROOTS[logn], ROOTS[logn_lde]
        point_x = (fmul(MUL_GEN, fpow(eta, rev_bits(logn_lde, idx))), 0)
        loc1 = escale(omega, zeta)
        one = emul(esub(g0, y0), einv(esub(point_x, zeta)))
        two = emul(esub(g1, y1), einv(esub(point_x, loc1)))
        cur = eadd(emul(epow(alpha, len(second)), one), two)
        initial = cur
        shift, size, qi = MUL_GEN, logn_lde, idx                 # foldingStep :291-323
        for s, a in enumerate(arities):
            evals = ext(qr["steps"][s]["evals"])
            start = rev_bits(size, (qi >> a) << a)               # prepareCoset :245-256
            offset = fmul(shift, fpow(ROOTS[size], start))
            xs = [evals[rev_bits(a, i)] for i in range(1 << a)]  # reverseIndexBitsList
            cur = fold_coset(betas[s], a, offset, xs)
            shift = fpow(shift, 1 << a)
            size, qi = size - a, qi >> a
        x_final = fmul(shift, fpow(ROOTS[size], rev_bits(size, qi)))   # folding_query_loc :288-291
        val, xp = (0, 0), 1
        for c in final_coeffs:                                   # evalPolynomialAt :325-327
            val = eadd(val, escale(xp, c))
            xp = fmul(xp, x_final)
        out.append((initial, cur, val))
    return out


@pytest.mark.parametrize("idx", range(len(_fixtures()[0])))
def test_literal_fri_query_values_match_oracle_trace(idx):
    cases, rd = _fixtures()
    case = cases[idx]
    if case["status"] < 0:
        pytest.skip("the reference raises before the folded values exist (Merkle / evaluation error)")
    common_b, vkey_b = rd(case["circuit"] + "_common.json.gz"), rd(case["circuit"] + "_vkey.json.gz")
    proof_b = rd(case["name"] + "_proof.json.gz")
    common, vkey, pwpi = json.loads(common_b), json.loads(vkey_b), json.loads(proof_b)
    ch = proof_challenges(common, vkey, pwpi)
    vals = fri_query_values(common, pwpi, ch)
    _, tr = oracle().verify_json(common_b, vkey_b, proof_b, trace=True)
    tr = [int(x) for x in tr]
    r = common["config"]["num_challenges"]
    S = len(pwpi["proof"]["opening_proof"]["commit_phase_merkle_caps"])
    Q = common["config"]["fri_config"]["num_query_rounds"]
    o_qin = 4 + 3 * r + 4 * r + 4 + 2 * S + 1 + Q + 4 * r       # include/p2v.h trace layout
    o_qfold, o_qfin = o_qin + 2 * Q, o_qin + 4 * Q
    for q, (ini, fold, fin) in enumerate(vals):
        assert tuple(tr[o_qin + 2 * q:o_qin + 2 * q + 2]) == ini, (case["name"], q, "combineInitial")
        assert tuple(tr[o_qfold + 2 * q:o_qfold + 2 * q + 2]) == fold, (case["name"], q, "folded")
        assert tuple(tr[o_qfin + 2 * q:o_qfin + 2 * q + 2]) == fin, (case["name"], q, "final poly")


def test_fold16_in_halves_is_the_same_interpolant():
    """k_fri folds an arity-16 coset in two halves (fri.h fold16_halves):
    with v the coset values in received order (vals[rev k] = v[k]), E / O the 8-point transforms
    of v[0..7] / v[8..15] and w = omega_16, sum_k c_k b^k = (1 + b^8) E(b) + (1 - b^8) O(w^-1 b),
    where c_k = sum_j vals_j w^(-jk).  Exact integers, against that direct sum."""
    import random
    rng = random.Random(16)
    winv = finv(ROOTS[4])

    def dft_horner(vals, root_inv, b):             # sum_k (sum_j vals_j root_inv^(jk)) b^k
        n = len(vals)
        tot, bk = (0, 0), (1, 0)
        for k in range(n):
            ck = (0, 0)
            for j in range(n):
                ck = eadd(ck, escale(pow(root_inv, j * k, P), vals[j]))
            tot = eadd(tot, emul(bk, ck))
            bk = emul(bk, b)
        return tot

    one = (1, 0)
    for _ in range(12):
        v = [(rng.randrange(P), rng.randrange(P)) for _ in range(16)]
        b = (rng.randrange(P), rng.randrange(P))
        vals = [None] * 16
        for k in range(16):
            vals[rev_bits(4, k)] = v[k]
        direct = dft_horner(vals, winv, b)
        half = lambda u: [u[rev_bits(3, m)] for m in range(8)]   # vals8[rev3 j] = u[j]
        lo = dft_horner(half(v[:8]), winv * winv % P, b)
        hi = dft_horner(half(v[8:]), winv * winv % P, escale(winv, b))
        b8 = epow(b, 8)
        assert eadd(emul(eadd(one, b8), lo), emul(esub(one, b8), hi)) == direct


def fold_coset_lagrange(beta, arity_bits, offset, xs):
    """foldCosetWith's value by Lagrange's formula instead of fold_coset's coefficient sums (which
    take arity^2 modular powers: too slow from arity 128 on).  The interpolant of xs_j at the coset
    points x_j = offset omega^j, at beta: with Z(X) = X^n - offset^n and Z'(x_j) = n x_j^(n-1) =
    n offset^n / x_j, P(beta) = Z(beta) / (n offset^n) * sum_j xs_j x_j / (beta - x_j); where beta
    is a coset point itself the value is that point's xs_j."""
    n = 1 << arity_bits
    omega = ROOTS[arity_bits]
    pts, x = [], offset % P
    for _ in range(n):
        pts.append(x)
        x = x * omega % P
    if beta[1] == 0 and beta[0] in pts:
        return xs[pts.index(beta[0])]
    tot = (0, 0)
    for xj, v in zip(pts, xs):
        tot = eadd(tot, emul(escale(xj, v), einv(esub(beta, (xj, 0)))))
    z = esub(epow(beta, n), (pow(offset, n, P), 0))
    return escale(finv(n * pow(offset, n, P) % P), emul(z, tot))


def test_fold_coset_lagrange_is_fold_coset():
    """The Lagrange form the GPU fold tests use as their reference at arity bits >= 5 equals the
    literal fold_coset for arity bits 1..5: random values, beta in F^2, in the base field, 0, and
    on a coset point (exact integers)."""
    import random
    rng = random.Random(55)
    for ab in range(1, 6):
        n = 1 << ab
        for t in range(6):
            ofs = rng.randrange(1, P)
            xs = [(rng.randrange(P), rng.randrange(P)) for _ in range(n)]
            beta = [(rng.randrange(P), rng.randrange(P)), (rng.randrange(P), 0), (0, 0),
                    (ofs * pow(ROOTS[ab], rng.randrange(n), P) % P, 0), (ofs, 0), (0, rng.randrange(P))][t]
            assert fold_coset_lagrange(beta, ab, ofs, xs) == fold_coset(beta, ab, ofs, xs), (ab, t)


def test_literal_transcript_and_fri_std_n12_two_folding_steps():
    """The standard recursion shape (degree_bits 12: two arity-16 folds, a 16-coefficient final
    polynomial), freshly generated: challenges and every per-query FRI value, literal vs oracle."""
    from support import gen_circuit
    gc = gen_circuit(12, 4, 0)
    pj = gc.proof(1, 1)
    common, vkey, pwpi = json.loads(gc.common), json.loads(gc.vkey), json.loads(pj)
    ch = proof_challenges(common, vkey, pwpi)
    st, tr = oracle().verify_json(gc.common, gc.vkey, pj, trace=True)
    assert st == 1
    tr = [int(x) for x in tr]
    r, Q = common["config"]["num_challenges"], common["config"]["fri_config"]["num_query_rounds"]
    S = len(pwpi["proof"]["opening_proof"]["commit_phase_merkle_caps"])
    assert S == 2
    o_qidx = 4 + 3 * r + 4 * r + 4 + 2 * S + 1
    assert tr[o_qidx:o_qidx + Q] == ch["qidx"]
    assert tr[4 + 3 * r + 4 * r:4 + 3 * r + 4 * r + 2] == ch["zeta"]
    o_qin = o_qidx + Q + 4 * r
    for q, (ini, fold, fin) in enumerate(fri_query_values(common, pwpi, ch)):
        assert tuple(tr[o_qin + 2 * q:o_qin + 2 * q + 2]) == ini
        assert tuple(tr[o_qin + 2 * Q + 2 * q:o_qin + 2 * Q + 2 * q + 2]) == fold
        assert tuple(tr[o_qin + 4 * Q + 2 * q:o_qin + 4 * Q + 2 * q + 2]) == fin
        assert fold == fin                          # round_ok for a valid proof
    combined, quot = plonk_values(common, pwpi, ch)
    o_comb = o_qidx + Q
    assert [tuple(tr[o_comb + 2 * i:o_comb + 2 * i + 2]) for i in range(r)] == combined
    assert [tuple(tr[o_comb + 2 * r + 2 * i:o_comb + 2 * r + 2 * i + 2]) for i in range(r)] == quot


# ---------------------------------------------------------------------------------------------
# The Plonk identity's permutation part, the same way: Plonk/Vanishing.hs:48-111 (zs1 and the
# partial-product chunks, combined with powers of each alpha) and Plonk/Verifier.hs:35-51 (the
# quotient chunks reduced in powers of zeta^n), for the circuits without lookups.  The
# generator's gate filters are exactly 0 at zeta, so the gate terms add 0 and the
# combined value is the permutation part alone; test_gpu covers the gate programs themselves
# with every filter set to 1.

def eval_lagrange0(nn, zeta):                       # Algebra/Poly.hs:14-17
    if zeta == (1, 0):
        return (1, 0)
    return emul(esub(epow(zeta, nn), (1, 0)), einv(escale(nn % P, esub(zeta, (1, 0)))))


def eprod(xs):
    acc = (1, 0)
    for x in xs:
        acc = emul(acc, x)
    return acc


def chunks(k, xs):                                  # Misc/Aux.hs:110-113
    return [xs[i:i + k] for i in range(0, len(xs), k)]


def plonk_values(common, pwpi, ch):
    """(combined C_i per challenge round, sum_k zeta^(nk) q_{i,k} per round)."""
    cfg = common["config"]
    r, qdf = cfg["num_challenges"], common["quotient_degree_factor"]
    nn = 1 << common["fri_params"]["degree_bits"]
    o = pwpi["proof"]["openings"]
    ext = lambda xs: [(F(a), F(b)) for a, b in xs]
    zeta = tuple(ch["zeta"])
    zs, zs_next = ext(o["plonk_zs"]), ext(o["plonk_zs_next"])
    wires, sigmas, pps = ext(o["wires"]), ext(o["plonk_sigmas"]), ext(o["partial_products"])
    k_is = [F(k) for k in common["k_is"]]
    zs1 = [emul(eval_lagrange0(nn, zeta), esub(z, (1, 0))) for z in zs]
    pp_checks = []
    for i, pp_chunk in enumerate(chunks(common["num_partial_products"], pps)[:r]):
        beta, gamma = ch["betas"][i], ch["gammas"][i]
        numers = chunks(qdf, [eadd(eadd(w, escale(fmul(beta, k), zeta)), (gamma, 0)) for k, w in zip(k_is, wires)])
        denoms = chunks(qdf, [eadd(eadd(w, escale(beta, s)), (gamma, 0)) for s, w in zip(sigmas, wires)])
        current = [zs[i]] + pp_chunk + [zs_next[i]]
        prs = list(zip(current, current[1:]))     # Misc/Aux.hs:76-79
        for (prev, nxt), nu, de in zip(prs, numers, denoms):
            pp_checks.append(esub(emul(prev, eprod(nu)), emul(nxt, eprod(de))))
    terms = zs1 + pp_checks                       # ++ lookup_checks (none) ++ gates (all 0 here)
    combined = []
    for a in ch["alphas"]:                        # combineWithPowersOfAlpha, Vanishing.hs:54-56
        acc = (0, 0)
        for x in reversed(terms):
            acc = eadd(x, escale(a, acc))
        combined.append(acc)
    zeta_n = epow(zeta, nn)
    quot = []
    for chunk in chunks(qdf, ext(o["quotient_polys"])):   # Verifier.hs:43-49
        acc = (0, 0)
        for x in reversed(chunk):
            acc = eadd(x, emul(zeta_n, acc))
        quot.append(acc)
    return combined, quot


@pytest.mark.parametrize("idx", range(len(_fixtures()[0])))
def test_literal_plonk_identity_values_match_oracle_trace(idx):
    cases, rd = _fixtures()
    case = cases[idx]
    common_b, vkey_b = rd(case["circuit"] + "_common.json.gz"), rd(case["circuit"] + "_vkey.json.gz")
    common = json.loads(common_b)
    if common["num_lookup_polys"] > 0 or case["circuit"].endswith(("_m1", "_m2")):
        pytest.skip("live gate / lookup terms: the full restatement is tests/test_vanishing_literal.py")
    proof_b = rd(case["name"] + "_proof.json.gz")
    vkey, pwpi = json.loads(vkey_b), json.loads(proof_b)
    ch = proof_challenges(common, vkey, pwpi)
    combined, quot = plonk_values(common, pwpi, ch)
    _, tr = oracle().verify_json(common_b, vkey_b, proof_b, trace=True)
    tr = [int(x) for x in tr]
    r = common["config"]["num_challenges"]
    S = len(pwpi["proof"]["opening_proof"]["commit_phase_merkle_caps"])
    Q = common["config"]["fri_config"]["num_query_rounds"]
    o_comb = 4 + 3 * r + 4 * r + 4 + 2 * S + 1 + Q     # include/p2v.h trace layout
    o_quot = o_comb + 2 * r
    for i in range(r):
        assert tuple(tr[o_comb + 2 * i:o_comb + 2 * i + 2]) == combined[i], (case["name"], i, "C_i")
        assert tuple(tr[o_quot + 2 * i:o_quot + 2 * i + 2]) == quot[i], (case["name"], i, "quotient")
    nn = 1 << common["fri_params"]["degree_bits"]
    eqs_ok = all(emul(q, esub(epow(tuple(ch["zeta"]), nn), (1, 0))) == c for q, c in zip(quot, combined))
    assert eqs_ok == bool(tr[o_quot + 2 * r + 6 * Q] & 1), case["name"]
