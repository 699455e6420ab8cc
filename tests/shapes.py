"""Circuit shapes beyond the generator's defaults, for tests/test_shapes_cpu.py,
tests/test_gpu_challenges.py and tests/test_gpu_gate_params.py: circuits with 1, 3 and 4
challenge rounds (Generator.circuit's num_challenges), and generated circuits whose gate strings
are replaced by other parameters of the same gate kind.

A swapped circuit keeps its shape (135 wires, 2 constants, the selector groups, the constants
oracle), so the generator's proofs of the unswapped circuit keep their Merkle paths, transcript
and FRI rounds against it; only the gate terms of C_i(zeta) change, the identity fails (status
0) and the whole trace stays comparable with the oracle's."""
from __future__ import annotations

import json
import random

from support import P, gen_circuit, mutate, randomize_openings

PHANTOM = "_phantom: PhantomData<plonky2_field::goldilocks_field::GoldilocksField>"
NUM_WIRES, NUM_CONSTS = 135, 2
ROUNDS = (1, 3, 4)   # the challenge rounds besides the generator's default 2


def circuit(nb=6, mode=1, lk=0, ng=0, r=2, ext=0, arities=(), seed=1):
    """gen_circuit with r challenge rounds; r = 2 is the default call, with its cache key."""
    args = (nb, 4, lk, seed, 28, 16, ng, mode, ext, tuple(arities))
    return gen_circuit(*args) if r == 2 else gen_circuit(*args, num_challenges=r)


def proof_pool(gc):
    """Two valid proofs, one proof with each of the generator's flags 1 (first FRI layer), 2 (last
    FRI layer) and 4 (quotient opening), and two proofs with every opening but the wires uniform."""
    valid = [gc.proof(1, 1), gc.proof(2, 2)]
    flagged = [gc.proof(1, 3, flags=1), gc.proof(2, 4, flags=2), gc.proof(1, 5, flags=4)]
    return valid + flagged + [randomize_openings(valid[0], 41), randomize_openings(valid[1], 42)]


N_VALID = 2   # proof_pool()[:N_VALID] are the valid proofs


# ----------------------------------------------------------------------------- gate strings
def roots_of_unity():   # the 2^k-th roots the reference's enumerateSubgroup uses
    x, out = 0x64fdd1a46201e246, []
    while x != 1:
        out.append(x)
        x = x * x % P
    return list(reversed(out + [1]))


def barycentric_weights(bits):
    """1 / prod_{j != i} (x_i - x_j) over the subgroup of order 2^bits, in Python integers."""
    g = roots_of_unity()[bits]
    pts = [pow(g, i, P) for i in range(1 << bits)]
    out = []
    for i, x in enumerate(pts):
        prod = 1
        for j, y in enumerate(pts):
            if j != i:
                prod = prod * (x - y) % P
        out.append(pow(prod, P - 2, P))
    return out


def coset_string(bits, degree, nweights=None):
    w = barycentric_weights(bits)[:nweights]
    return ("CosetInterpolationGate { subgroup_bits: %d, degree: %d, barycentric_weights: [%s], %s }<D=2>"
            % (bits, degree, ", ".join(str(x) for x in w), PHANTOM))


def gate_string(kind, p):
    if kind == "Arithmetic":
        return "ArithmeticGate { num_ops: %d }" % p
    if kind == "ArithmeticExtension":
        return "ArithmeticExtensionGate { num_ops: %d }" % p
    if kind == "MulExtension":
        return "MulExtensionGate { num_ops: %d }" % p
    if kind == "Constant":
        return "ConstantGate { num_consts: %d }" % p
    if kind == "Exponentiation":
        return "ExponentiationGate { num_power_bits: %d }" % p
    if kind == "Reducing":
        return "ReducingGate { num_coeffs: %d }" % p
    if kind == "ReducingExtension":
        return "ReducingExtensionGate { num_coeffs: %d }" % p
    if kind == "BaseSum":
        return "BaseSumGate { num_limbs: %d } + Base: %d" % p
    if kind == "RandomAccess":
        return "RandomAccessGate { bits: %d, num_copies: %d, num_extra_constants: %d, %s }<D=2>" % (p + (PHANTOM,))
    if kind == "CosetInterpolation":
        return coset_string(*p)
    raise ValueError(kind)


# Every entry fits 135 wires and 2 constants (csrc/circuit.cpp gate_footprint).  What each reaches
# in csrc/vanish.h, from the parameters alone:
# - RandomAccess bits 0, 1, 2, 3: those arms of `switch (nbits)`; 5 and 6: its `default` multilinear form
#   (the generator's 4 is the remaining arm);
# - BaseSum limbs 1: the `else h = V.w(1)` branch; bases 0 (empty product), 1, 3, 4, 16;
# - Coset (bits, degree) -> parts = (2^bits - 2) div (degree - 1) + 1: (1,2) 1, (2,2) 3, (2,3) 2, (3,2) 7,
#   (3,9) 1 with degree > npts, (4,2) 15, (4,15) 2, (4,16) 1, (5,4) 11, (5,6) 7, (6,64) 1 with nint = 0;
#   (4,6) with 10 or 3 of its 16 weights: the `k >= nweights` break in the second / first part.
PARAMS = {
    "Arithmetic": [1, 33],
    "ArithmeticExtension": [1, 16],
    "MulExtension": [1, 22],
    "Constant": [1],
    "Exponentiation": [1, 2],
    "Reducing": [1, 2],
    "ReducingExtension": [1, 2],
    "BaseSum": [(1, 2), (2, 2), (10, 3), (31, 4), (16, 16), (5, 1), (5, 0)],
    "RandomAccess": [(0, 20, 2), (1, 10, 0), (2, 8, 2), (3, 6, 1), (5, 3, 2), (5, 1, 0), (6, 1, 2)],
    "CosetInterpolation": [(1, 2), (2, 2), (2, 3), (3, 2), (3, 9), (4, 2), (4, 15), (4, 16), (5, 4), (5, 6), (6, 64),
                           (4, 6, 10), (4, 6, 3)],
}
ENTRIES = [(kind, p) for kind, ps in PARAMS.items() for p in ps]
# one circuit with every kind replaced at once: the largest footprints, the RandomAccess default
# form, a base-4 BaseSum and a single-part coset gate
ALL_AT_ONCE = {"Arithmetic": 33, "ArithmeticExtension": 16, "MulExtension": 22, "Constant": 1, "Exponentiation": 2,
               "Reducing": 2, "ReducingExtension": 1, "BaseSum": (31, 4), "RandomAccess": (5, 3, 2),
               "CosetInterpolation": (6, 64)}


def coset_parts(bits, degree, nweights=None):
    """The chunks the reference evaluates (Gate/Custom/CosetInterp.hs:56-60): the initials, zipped
    with the zip3 of the chunked domain, values and weights (the first chunk `degree` long, the
    others degree - 1)."""
    npts = 1 << bits
    nw = npts if nweights is None else nweights

    def nchunks(n):
        return 1 + -(-(n - min(degree, n)) // (degree - 1))
    return min((npts - 2) // (degree - 1) + 1, nchunks(npts), nchunks(nw))


def gate_index(gates, kind):
    """The index of the circuit's gate of this kind (its Debug string starts with kind + 'Gate ')."""
    hits = [i for i, s in enumerate(gates) if s.startswith(kind + "Gate ")]
    assert len(hits) == 1, (kind, hits)
    return hits[0]


def swap(common: bytes, repl: dict) -> bytes:
    """The common data with the gate of each kind in `repl` replaced by gate_string(kind, repl[kind])."""
    c = json.loads(common)
    for kind, p in repl.items():
        c["gates"][gate_index(c["gates"], kind)] = gate_string(kind, p)
    return json.dumps(c, separators=(",", ":")).encode()


# ----------------------------------------------------------------------------- edge-valued openings
def edge_rows(pool, width, n, seed):
    """n rows of `width` F^2 openings from the edge pool: a whole row of one edge value each for
    0, 1, p - 1, 2^32 - 1, 2^32, 2^32 + 1 (rows 0..5), then rows of edge values only, then edge
    values among uniform ones."""
    rng = random.Random(seed)
    whole = [0, 1, P - 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1]
    assert all(v in pool for v in whole)
    rows = []
    for i in range(n):
        if i < len(whole):
            rows.append([[whole[i], whole[i]] for _ in range(width)])
        elif i % 2 == 0:
            rows.append([[rng.choice(pool), rng.choice(pool)] for _ in range(width)])
        else:
            rows.append([[rng.choice(pool) if rng.random() < 0.5 else rng.randrange(P) for _ in range(2)] for _ in range(width)])
    return rows


def with_openings(proof: bytes, **cols) -> bytes:
    """The proof with the opening vectors `cols` (key -> [[re, im]]) put in place of its own."""
    def f(d):
        o = d["proof"]["openings"]
        for k, v in cols.items():
            assert len(v) == len(o[k]), (k, len(v), len(o[k]))
            o[k] = v
    return mutate(proof, f)
