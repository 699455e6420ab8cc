"""The reference's own gates restated as gate programs (p2v.GateProgram, include/p2v.h "gate
programs"), for the tests of user-registered gates: a generated circuit's gate strings are
renamed to strings the library does not know, and these programs take the built-in kernels' place.

Written from the reference's constraint programs, Gate/Constraints.hs:40-128 and
Gate/Custom/{Poseidon,RandomAccess,Reducing}.hs, one function per gate, in their own terms
(wire / cnst / hash, wireExt, commitExt, let_); the Poseidon constants are those of
Hash/Constants.hs as csrc/poseidon_constants.h holds them.  tests/test_gate_programs.py pins
every one against the oracle's or_eval_gate, independently of the GPU."""
from __future__ import annotations

import os
import re
from functools import lru_cache

from support import PKG, p2v_module

PREFIX = "X"   # renamed gate string = PREFIX + original: no built-in pattern matches it


class Ext:
    """Ext (Expr v): a simulated F^2-over-F^2 element (Gate/Vars.hs:56-57, GoldilocksExt.hs:54-61)."""

    def __init__(self, u, v):
        self.u, self.v = u, v

    def __add__(self, o):
        return Ext(self.u + o.u, self.v + o.v)

    def __sub__(self, o):
        return Ext(self.u - o.u, self.v - o.v)

    def __mul__(self, o):   # X^2 = 7 as the literal LitE 7
        return Ext(self.u * o.u + 7 * (self.v * o.v), self.u * o.v + self.v * o.u)

    def __iter__(self):
        return iter((self.u, self.v))


@lru_cache(maxsize=1)
def poseidon_tables() -> dict:
    """Hash/Constants.hs, from the generated header (tools/gen_constants.py)."""
    text = open(os.path.join(PKG, "csrc", "poseidon_constants.h")).read()
    out = {}
    for name in ("MDS_CIRC", "MDS_DIAG", "FAST_PARTIAL_FIRST_ROUND_CONSTANT", "FAST_PARTIAL_ROUND_CONSTANTS",
                 "FAST_PARTIAL_ROUND_VS", "FAST_PARTIAL_ROUND_W_HATS", "FAST_PARTIAL_ROUND_INITIAL_MATRIX", "ALL_ROUND_CONSTANTS"):
        m = re.search(r"#define P2V_" + name + r"_INIT\b(.*?)(?=#define|#endif)", text, re.S)
        out[name] = [int(v, 0) for v in re.findall(r"0x[0-9a-fA-F]+|\b\d+\b", m.group(1))]
    assert len(out["MDS_CIRC"]) == 12 and len(out["ALL_ROUND_CONSTANTS"]) == 360 and len(out["FAST_PARTIAL_ROUND_VS"]) == 242
    assert len(out["FAST_PARTIAL_ROUND_INITIAL_MATRIX"]) == 121 and len(out["FAST_PARTIAL_ROUND_CONSTANTS"]) == 22
    return out


def mds_coeff(i, j):   # mdsMatrixCoeff, Hash/Constants.hs:24-25
    t = poseidon_tables()
    return t["MDS_CIRC"][(j - i) % 12] + (t["MDS_DIAG"][i] if i == j else 0)


# ----------------------------------------------------------------------------- the gates
def arithmetic(g, num_ops, wrong=False):   # Constraints.hs:45-46
    for i in range(num_ops):
        j = 4 * i
        lhs = g.wire(j + 3) - g.const(0) * g.wire(j) * g.wire(j + 1)
        t = g.const(1) * g.wire(j + 2)
        g.commit(lhs + t if wrong and i == 0 else lhs - t)   # wrong: one SUB turned into ADD


def wire_ext(g, i):
    return Ext(g.wire(i), g.wire(i + 1))


def from_base(g, x):
    return Ext(x, g.lit(0))


def arithmetic_ext(g, num_ops):   # :49-54
    for i in range(num_ops):
        j = 8 * i
        c0, c1 = from_base(g, g.const(0)), from_base(g, g.const(1))
        g.commit_ext(wire_ext(g, j + 6) - c0 * wire_ext(g, j) * wire_ext(g, j + 2) - c1 * wire_ext(g, j + 4))


def base_sum(g, num_limbs, base):   # :57-62
    def limb(i):
        return g.wire(i + 1)

    def go(k):
        return limb(k) + base * go(k + 1) if k < num_limbs - 1 else limb(k)
    g.commit(go(0) - g.wire(0))
    for i in range(num_limbs):
        pr = g.lit(1)
        for k in range(base):
            pr = pr * (limb(i) - k)
        g.commit(pr)


def constant(g, num_consts):   # :68-69
    for i in range(num_consts):
        g.commit(g.const(i) - g.wire(i))


def exponentiation(g, n):   # :114-128
    base, out = g.wire(0), g.wire(n + 1)

    def tmp(i):
        return g.wire(n + 2 + i)

    def cur_bit(i):
        return g.wire((n - 1 - i) + 1)
    for i in range(n):
        prev = g.lit(1) if i == 0 else tmp(i - 1) * tmp(i - 1)
        comp = prev * (cur_bit(i) * base + (1 - cur_bit(i)))
        g.commit(comp - tmp(i))
    g.commit(out - tmp(n - 1))


def mul_ext(g, num_ops):   # :80-83
    for i in range(num_ops):
        j = 6 * i
        g.commit_ext(wire_ext(g, j + 4) - from_base(g, g.const(0)) * wire_ext(g, j) * wire_ext(g, j + 2))


def public_input(g):   # :88-89
    for i in range(4):
        g.commit(g.wire(i) - g.pi_hash(i))


def scale_ext(c, e):
    return Ext(c * e.u, c * e.v)


def poseidon_mds(g):   # Custom/Poseidon.hs:49-59
    for i in range(12):
        acc = None
        for j in range(12):
            t = scale_ext(g.lit(mds_coeff(i, j)), wire_ext(g, 2 * j))
            acc = t if acc is None else acc + t
        g.commit_ext(wire_ext(g, 2 * (i + 12)) - acc)


def random_access(g, num_bits, copies, extra):   # Custom/RandomAccess.hs:47-88
    veclen = 1 << num_bits
    width = 2 + veclen
    bits_start = width * copies + extra

    def bits(k, j):
        return g.wire(bits_start + k * num_bits + j)
    for k in range(copies):
        for j in range(num_bits):
            g.commit(bits(k, j) * (bits(k, j) - 1))
        rec = g.lit(0)
        for j in reversed(range(num_bits)):   # foldr (\b acc -> 2*acc + b) 0
            rec = 2 * rec + bits(k, j)
        g.commit(rec - g.wire(k * width))
        vals = [g.wire(k * width + 2 + i) for i in range(veclen)]
        for j in range(num_bits):   # lookup_eq
            b = bits(k, j)
            vals = [x + b * (y - x) for x, y in zip(vals[0::2], vals[1::2])]
        assert len(vals) == 1
        g.commit(vals[0] - g.wire(k * width + 1))
    for j in range(extra):
        g.commit(g.const(j) - g.wire(copies * width + j))


def reducing(g, n, ext=False):   # Custom/Reducing.hs:28-60
    output, alpha, initial = wire_ext(g, 0), wire_ext(g, 2), wire_ext(g, 4)
    start = 6 + (2 * n if ext else n)

    def coeff(i):
        return wire_ext(g, 6 + 2 * i) if ext else from_base(g, g.wire(6 + i))

    def accum(i):
        return wire_ext(g, start + 2 * i) if i < n - 1 else output
    for i in range(n):
        prev = initial if i == 0 else accum(i - 1)
        g.commit_ext(prev * alpha + coeff(i) - accum(i))


def poseidon(g):   # Custom/Poseidon.hs:63-150
    T = poseidon_tables()
    rc = T["ALL_ROUND_CONSTANTS"]

    def sbox(x):
        x2 = x * x
        x3 = x * x2
        x4 = x2 * x2
        return x3 * x4

    def mds(state):   # row by row: a row's sum is complete before the next row starts
        out = []
        for i in range(12):
            acc = None
            for j, x in enumerate(state):
                t = mds_coeff(i, j) * x
                acc = t if acc is None else acc + t
            out.append(acc)
        return out

    def plus_rc(r, state):
        return [x + rc[12 * r + i] for i, x in enumerate(state)]

    def inp(i):
        return g.wire(i)

    def delta(i):
        return g.wire(25 + i)
    swap = g.wire(24)
    g.commit(swap * (swap - 1))
    for i in range(4):
        g.commit(swap * (inp(i + 4) - inp(i)) - delta(i))
    state = [inp(i) + delta(i) for i in range(4)] + [inp(i) - delta(i - 4) for i in range(4, 8)] + [inp(i) for i in range(8, 12)]
    for r in range(4):   # initial full rounds
        s2 = plus_rc(r, state)
        if r != 0:
            sb = [g.wire(29 + 12 * (r - 1) + i) for i in range(12)]
            for i in range(12):
                g.commit(s2[i] - sb[i])
            s2 = sb
        state = mds([sbox(x) for x in s2])
    # partial rounds
    state = [x + c for x, c in zip(state, T["FAST_PARTIAL_FIRST_ROUND_CONSTANT"])]
    init = T["FAST_PARTIAL_ROUND_INITIAL_MATRIX"]   # partialMdsMatrixCoeff i j = matrix ! (j, i)
    rest = state[1:]
    new = []
    for i in range(11):
        acc = None
        for j, x in enumerate(rest):
            t = init[11 * j + i] * x
            acc = t if acc is None else acc + t
        new.append(acc)
    state = [state[0]] + new
    for r in range(22):
        sb = g.wire(29 + 36 + r)
        g.commit(state[0] - sb)
        y = sbox(sb)
        z = y + T["FAST_PARTIAL_ROUND_CONSTANTS"][r] if r < 21 else y
        st2 = [z] + state[1:]
        cs = [mds_coeff(0, 0)] + T["FAST_PARTIAL_ROUND_W_HATS"][11 * r: 11 * r + 11]
        d = None
        for e, c in zip(st2, cs):   # dotProd
            t = e * c
            d = t if d is None else d + t
        vs = T["FAST_PARTIAL_ROUND_VS"][11 * r: 11 * r + 11]
        state = [d] + [x + z * t for x, t in zip(st2[1:], vs)]
    for r in range(4):   # final full rounds
        s2 = plus_rc(r + 26, state)
        sb = [g.wire(29 + 36 + 22 + 12 * r + i) for i in range(12)]
        for i in range(12):
            g.commit(s2[i] - sb[i])
        state = mds([sbox(x) for x in sb])
    for i in range(12):
        g.commit(state[i] - g.wire(i + 12))


# ----------------------------------------------------------------------------- by gate string
RESTATED = {0: "Arithmetic", 1: "ArithmeticExtension", 2: "BaseSum", 4: "Constant", 5: "Exponentiation", 8: "MulExtension",
            10: "PublicInput", 11: "Poseidon", 12: "PoseidonMds", 13: "RandomAccess", 14: "Reducing", 15: "ReducingExtension"}


def restate(gate: str, wrong: bool = False):
    """The program of one of the reference's gate strings, or None for a gate that is not restated
    (Noop / Lookup / LookupTable have no constraints, CosetInterpolation is left to its kernel)."""
    p2v = p2v_module()
    w = p2v._gate_words(gate)
    tag, f = w[0], w[1:]
    if tag not in RESTATED:
        return None
    g = p2v.GateProgram()
    if tag == 0:
        arithmetic(g, f[0], wrong)
    elif tag == 1:
        arithmetic_ext(g, f[0])
    elif tag == 2:
        base_sum(g, f[0], f[1])
    elif tag == 4:
        constant(g, f[0])
    elif tag == 5:
        exponentiation(g, f[0])
    elif tag == 8:
        mul_ext(g, f[0])
    elif tag == 10:
        public_input(g)
    elif tag == 11:
        assert f[0] == 12
        poseidon(g)
    elif tag == 12:
        assert f[0] == 12
        poseidon_mds(g)
    elif tag == 13:
        random_access(g, f[0], f[1], f[2])
    elif tag == 14:
        reducing(g, f[0])
    elif tag == 15:
        reducing(g, f[0], ext=True)
    return g


def rename(common: bytes, only=None, wrong=()):
    """(common JSON with the restated gates renamed, {renamed string: program}, their gate indices).
    only: rename just these gate indices; wrong: gate indices that get the wrong Arithmetic."""
    import json
    c = json.loads(common)
    progs, idx = {}, []
    for i, s in enumerate(c["gates"]):
        if only is not None and i not in only:
            continue
        g = restate(s, wrong=i in wrong)
        if g is None:
            continue
        c["gates"][i] = PREFIX + s
        progs[PREFIX + s] = g
        idx.append(i)
    return json.dumps(c, separators=(",", ":")).encode(), progs, idx
