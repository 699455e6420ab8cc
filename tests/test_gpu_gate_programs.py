"""GPU tests (MI355X) of user-registered gate programs (include/p2v.h "gate programs",
csrc/vanish_prog.hip).  The generator knows only the reference's gates, so a generated circuit's
gate strings are renamed to strings the library does not know and the programs of
tests/gate_programs.py (pinned against the oracle by tests/test_gate_programs.py) are registered
for them: the oracle verifies the original JSON, p2v the renamed JSON with programs, and statuses
and full traces must be equal word for word, for every proof of every batch."""
import json

import numpy as np
import pytest

import gate_programs as gp
from support import P, gen_circuit, oracle, p2v_module, trace_offsets

pytestmark = pytest.mark.gpu

MODE1 = (6, 4, 0, 1, 28, 16, 0, 1)
MODE2 = (6, 4, 0, 1, 28, 16, 0, 2)
LOOKUP = (6, 4, 4, 1, 28, 16, 0, 1)   # the real circuit with one lookup table (40 entries: it fits 64 rows)


@pytest.fixture(scope="module")
def p2v():
    import torch   # before libp2v, as tests/test_gpu.py
    assert torch.cuda.is_available(), "torch sees no GPU"
    m = p2v_module()
    if m.device_count() == 0:
        pytest.fail("no GPU visible to libp2v")
    return m


_oracle_memo = {}


def _oracle(gc, proof, unit_filters=False):
    key = (gc.common, gc.vkey, proof, unit_filters)
    if key not in _oracle_memo:
        _oracle_memo[key] = oracle().verify_json(gc.common, gc.vkey, proof, trace=True, unit_filters=unit_filters)
    return _oracle_memo[key]


_pool_memo = {}


def _pool(gc):
    """Two valid proofs and the generator's three reject classes: corrupted quotient opening,
    first FRI layer, last FRI layer."""
    if gc not in _pool_memo:
        _pool_memo[gc] = [gc.proof(1, 1), gc.proof(2, 2), gc.proof(1, 3, flags=4), gc.proof(1, 4, flags=1), gc.proof(2, 5, flags=2)]
    return _pool_memo[gc]


def _offsets(vk):
    i = vk.info
    return trace_offsets(i.num_challenges, i.num_fri_steps, i.num_query_rounds), i.num_challenges


def _combined(vk, tr):
    o, r = _offsets(vk)
    return tr[..., o["combined"]: o["combined"] + 2 * r]


# ----------------------------------------------------------------------------- 1: the interpreter on edge values
def _f2_eval(instrs, wires, consts, pih):
    """A program over exact Python integers: [(re, im)] of its commits."""
    v, out = [], []
    for ins in instrs:
        op = ins[0]
        if op == 0:
            v.append(wires[ins[1]])
        elif op == 1:
            v.append(consts[ins[1]])
        elif op == 2:
            v.append((pih[ins[1]], 0))
        elif op == 3:
            v.append((ins[1] % P, 0))
        elif op == 4:
            (a, b), (c, d) = v[ins[1]], v[ins[2]]
            v.append(((a + c) % P, (b + d) % P))
        elif op == 5:
            (a, b), (c, d) = v[ins[1]], v[ins[2]]
            v.append(((a - c) % P, (b - d) % P))
        elif op == 6:
            (a, b), (c, d) = v[ins[1]], v[ins[2]]
            v.append(((a * c + 7 * b * d) % P, (a * d + b * c) % P))
        elif op == 7:
            a, b = v[ins[1]]
            v.append((7 * b % P, a))
        else:
            out.append(v[ins[1]])
    return out


EDGE = [0, 1, P - 1, (1 << 32) - 1, P - (1 << 32), 1 << 48]


def _every_opcode(p2v):
    """A small program through every opcode and operand kind: slots read as both operands, leaf
    operands of every kind on both sides, a slot reused after its value died, products of edge
    values (emul's rare reduction paths), IMG of a leaf and of a slot, commits of both."""
    g = p2v.GateProgram()
    w = [g.wire(i) for i in range(6)]
    k0, k1 = g.const(0), g.const(1)
    h = [g.pi_hash(i) for i in range(4)]
    a = w[0] * w[1]
    b = w[2] * w[2]
    g.commit(a)
    g.commit(a * b - (w[3] + k0) * (k1 - h[0]))
    c = (a + b).img()
    g.commit(c)
    g.commit(w[4].img() * c + g.lit(P - 1) * h[1])
    g.commit(w[5])
    g.commit((g.lit((1 << 64) - 1) - w[0]) * (h[2] + h[3]) * (w[1] - w[1]))
    d = w[0] * w[0]
    for i in range(1, 6):
        d = d * w[i] + d
    g.commit(d - k0.img())
    g.commit(g.lit(1 << 48) * w[3] * (1 << 48))
    return g, 6, 2


def _poseidon(p2v):
    return gp.restate("PoseidonGate(PhantomData<plonky2_field::goldilocks_field::GoldilocksField>)<WIDTH=12>"), 135, 2


@pytest.mark.parametrize("which", ["every_opcode", "poseidon"])
def test_gpu_gate_program_interpreter_edge_values(p2v, which):
    """p2v_selftest op 21: the device interpreter on 256 rows built from 0, 1, p - 1, 2^32 - 1,
    p - 2^32, 2^48 and random values; every output word equals exact integer arithmetic."""
    g, nw, nk = (_every_opcode if which == "every_opcode" else _poseidon)(p2v)
    n, W = 256, 2 * (nw + nk) + 4
    rng = np.random.default_rng(21)
    items = rng.integers(0, P, (n, W), dtype=np.uint64)
    edge = np.array(EDGE, dtype=np.uint64)
    for i in range(n):
        if i < len(EDGE):
            items[i, :] = edge[i]                                   # one edge value everywhere
        elif i < 64:
            items[i, :] = edge[rng.integers(0, len(EDGE), W)]       # edge values only
        elif i < 192:
            m = rng.random(W) < 0.5                                 # edge values among random ones
            items[i, m] = edge[rng.integers(0, len(EDGE), int(m.sum()))]
    out = p2v.device_selftest(21, items, np.concatenate([np.array([nw, nk], dtype=np.uint64), g.words()]))
    assert out.shape == (n, 2 * g.num_commits)
    bad = []
    for i in range(n):
        row = [int(x) for x in items[i]]
        wires = [(row[2 * j], row[2 * j + 1]) for j in range(nw)]
        consts = [(row[2 * (nw + j)], row[2 * (nw + j) + 1]) for j in range(nk)]
        want = [x for pr in _f2_eval(g.instrs, wires, consts, row[2 * (nw + nk):]) for x in pr]
        got = [int(x) for x in out[i]]
        if got != want:
            bad.append((i, [j for j in range(len(want)) if got[j] != want[j]][:4]))
    assert not bad, bad[:8]
    # the host evaluator states the same semantics
    w0 = items[7]
    assert np.array_equal(g.evaluate(w0[: 2 * nw], w0[2 * nw: 2 * (nw + nk)], w0[2 * (nw + nk):]).reshape(-1), out[7])


# ----------------------------------------------------------------------------- 2: whole proofs
class Renamed:
    """A generated circuit, its renamed twin with every restated gate as a program, the proof
    pool with the oracle's results on the original JSON."""

    def __init__(self, p2v, args, only=None, wrong=()):
        self.gc = gen_circuit(*args)
        self.common, self.progs, self.idx = gp.rename(self.gc.common, only=only, wrong=wrong)
        self.orig = p2v.VerifierCircuitData.from_json(self.gc.common, self.gc.vkey)
        self.vk = p2v.VerifierCircuitData.from_json(self.common, self.gc.vkey, gates=self.progs)
        assert self.vk.num_program_gates == len(self.idx) > 0
        self.texts = _pool(self.gc)
        self.packed = self.vk.pack_many(self.texts)
        assert np.array_equal(self.packed, self.orig.pack_many(self.texts))


_renamed = {}


def _get(p2v, args):
    if args not in _renamed:
        _renamed[args] = Renamed(p2v, args)
    return _renamed[args]


@pytest.mark.parametrize("args", [MODE1, MODE2])
@pytest.mark.parametrize("n,tiled", [(128, False), (128, True), (3, False), (3, True)])
def test_gpu_gate_programs_whole_proofs(p2v, args, n, tiled):
    """Every restated gate of the circuit as a program: n = 128 (two tiles, the batch path) and
    n = 3 (the latency path), proof-major and tiled, valid proofs and the generator's three reject
    classes.  Statuses and full traces equal the oracle's on the original JSON and the same batch
    through the built-in kernels; every C_i(zeta) of the oracle is non-zero, so a program that was
    skipped could not pass."""
    D = _get(p2v, args)
    sel = (np.arange(n) + (0 if n > 3 else 1)) % len(D.texts)   # n = 3: a valid proof and two reject classes
    rows = np.ascontiguousarray(D.packed[sel])
    want = [_oracle(D.gc, D.texts[j]) for j in sel]
    for st, otr in want:
        assert (_combined(D.orig, otr) != 0).all(), "a combined constraint value is zero"
    assert {int(st) for st, _ in want} >= {1, 0}
    res, tr = p2v.BatchVerifier(D.vk, 0, n).run(rows, trace=True, tiled=tiled)
    ref, rtr = p2v.BatchVerifier(D.orig, 0, n).run(rows, trace=True, tiled=tiled)
    for i, (st, otr) in enumerate(want):
        assert int(res[i]) == int(st), (i, int(res[i]), int(st))
        assert np.array_equal(tr[i], otr), (i, np.nonzero(tr[i] != otr)[0][:10])
    assert np.array_equal(res, ref) and np.array_equal(tr, rtr)


# ----------------------------------------------------------------------------- 3: one gate at a time
def _gate_cases():
    out = []
    for args in (MODE1, MODE2):
        gates = json.loads(gen_circuit(*args).common)["gates"]
        out += [(args, i) for i, s in enumerate(gates) if gp.restate(s) is not None]
    return out


def test_gpu_gate_programs_one_gate_at_a_time_unit_filters(p2v):
    """Each restated gate in turn as the circuit's only program gate, every filter := 1
    (unit_filters): the trace, `combined` in it, equals the oracle's unit_filters trace of the
    original circuit, so a wrong program cannot hide behind a filter that is 0 at zeta."""
    cases = _gate_cases()
    assert len(cases) == 15
    for args, gi in cases:
        gc = gen_circuit(*args)
        common, progs, idx = gp.rename(gc.common, only={gi})
        assert idx == [gi]
        vk = p2v.VerifierCircuitData.from_json(common, gc.vkey, gates=progs)
        assert vk.num_program_gates == 1
        texts = _pool(gc)[:3]
        res, tr = p2v.BatchVerifier(vk, 0, len(texts)).run(vk.pack_many(texts), trace=True, unit_filters=True)
        for i, t in enumerate(texts):
            st, otr = _oracle(gc, t, unit_filters=True)
            assert (_combined(vk, otr) != 0).all()
            assert np.array_equal(_combined(vk, tr[i]), _combined(vk, otr)), (args, gi, i)
            assert int(res[i]) == int(st) and np.array_equal(tr[i], otr), (args, gi, i, np.nonzero(tr[i] != otr)[0][:10])


# ----------------------------------------------------------------------------- 4: a wrong program
def test_gpu_gate_programs_wrong_program_is_noticed(p2v):
    """The Arithmetic restatement with one SUB turned into ADD: valid proofs are rejected
    (status 0), `combined` differs from the oracle's, and every other trace word (transcript, FRI,
    quotient) still agrees."""
    gc = gen_circuit(*MODE1)
    gates = json.loads(gc.common)["gates"]
    ai = next(i for i, s in enumerate(gates) if s.startswith("ArithmeticGate"))
    common, progs, idx = gp.rename(gc.common, wrong={ai})
    vk = p2v.VerifierCircuitData.from_json(common, gc.vkey, gates=progs)
    o, r = _offsets(vk)
    texts = [gc.proof(1, 1), gc.proof(2, 2), gc.proof(1, 7)]
    res, tr = p2v.BatchVerifier(vk, 0, len(texts)).run(vk.pack_many(texts), trace=True)
    keep = np.ones(vk.info.trace_words, dtype=bool)
    keep[o["combined"]: o["combined"] + 2 * r] = False
    keep[o["flags"]] = False
    for i, t in enumerate(texts):
        st, otr = _oracle(gc, t)
        assert st == 1 and int(res[i]) == 0, (i, st, int(res[i]))
        assert not np.array_equal(_combined(vk, tr[i]), _combined(vk, otr))
        assert np.array_equal(tr[i][keep], otr[keep]), (i, np.nonzero((tr[i] != otr) & keep)[0][:10])
        assert int(tr[i][o["flags"]]) & 1 == 0 and int(otr[o["flags"]]) & 1 == 1   # eqs_ok


# ----------------------------------------------------------------------------- 5: keys and lookups
def test_gpu_gate_programs_keyed_batch(p2v):
    """Two verifier keys over the renamed common data (with_keys keeps the programs): proof i
    against key ids[i] equals the oracle's result for that key on the original JSON."""
    g1, g2 = gen_circuit(*MODE1), gen_circuit(6, 4, 0, 2, 28, 16, 0, 1)
    assert g1.common == g2.common and g1.vkey != g2.vkey
    common, progs, idx = gp.rename(g1.common)
    vk = p2v.VerifierCircuitData.from_json(common, g1.vkey, gates=progs).with_keys([g2.vkey])
    assert vk.num_keys == 2 and vk.num_program_gates == len(idx)
    texts = [g1.proof(1, 1), g2.proof(1, 1), g1.proof(1, 3, flags=4), g2.proof(2, 2)]
    n = 128
    sel = np.arange(n) % len(texts)
    ids = ((np.arange(n) // len(texts)) % 2).astype(np.uint32)
    rows = np.ascontiguousarray(vk.pack_many(texts)[sel])
    O = oracle()
    want = {(k, j): O.verify_json(g1.common, (g1, g2)[k].vkey, texts[j], trace=True) for k in range(2) for j in range(len(texts))}
    assert {int(st) for st, _ in want.values()} >= {1, 0}
    for lat in (False, True):   # the batch path and the latency path
        m = 3 if lat else n
        res, tr = p2v.BatchVerifier(vk, 0, m).run(rows[:m] if not lat else rows[4:7], trace=True, key_ids=ids[:m] if not lat else ids[4:7])
        for i in range(m):
            q = i if not lat else 4 + i
            st, otr = want[(int(ids[q]), int(sel[q]))]
            assert int(res[i]) == int(st) and np.array_equal(tr[i], otr), (lat, i)


def test_gpu_gate_programs_with_a_lookup_table(p2v):
    """The real circuit with one lookup table, its non-lookup gates as programs (the Lookup /
    LookupTable gates have no constraints and stay built-in): equal to the oracle, valid proofs
    and a rejected one, on both paths."""
    D = _get(p2v, LOOKUP)
    assert D.vk.info.has_lookups
    for n in (128, 3):
        sel = np.arange(n) % len(D.texts)
        res, tr = p2v.BatchVerifier(D.vk, 0, n).run(np.ascontiguousarray(D.packed[sel]), trace=True)
        for i, j in enumerate(sel):
            st, otr = _oracle(D.gc, D.texts[j])
            assert int(res[i]) == int(st) and np.array_equal(tr[i], otr), (n, i, np.nonzero(tr[i] != otr)[0][:10])
        assert {int(x) for x in res} >= {1, 0}
