"""CPU tests of user-registered gate programs (include/p2v.h "gate programs"): the tests' own
restatements of the reference's gates against the oracle, the encoding's validation, circuit
creation with and without programs, and a model of the slot allocation of the lowering
(csrc/circuit.cpp lower_gate_program).  The GPU side is tests/test_gpu_gate_programs.py."""
import json
import random

import numpy as np
import pytest

import gate_programs as gp
from support import P, gen_circuit, oracle, p2v_module

MODE1 = (6, 4, 0, 1, 28, 16, 0, 1)
MODE2 = (6, 4, 0, 1, 28, 16, 0, 2)


@pytest.fixture(scope="module")
def p2v():
    return p2v_module()


def _oracle_gate(gate, wires, consts, pih):
    out = np.zeros((512, 2), np.uint64)
    n = oracle().L.or_eval_gate(gate.encode(), wires.ctypes.data, len(wires), consts.ctypes.data, len(consts), pih.ctypes.data,
                                out.ctypes.data, 512)
    assert 0 <= n <= 512, n
    return out[:n]


@pytest.mark.parametrize("args", [MODE1, MODE2])
def test_restatements_equal_the_oracle(p2v, args):
    """Every restated gate string of the circuit, on 8 random F^2 rows and the generator's
    satisfying row: GateProgram.evaluate == or_eval_gate on the original string, word for word,
    with the same number of constraints."""
    gc = gen_circuit(*args)
    c = json.loads(gc.common)
    nw, nk = c["config"]["num_wires"], c["config"]["num_constants"]
    rng = np.random.default_rng(11)
    seen = 0
    for gi, s in enumerate(c["gates"]):
        g = gp.restate(s)
        if g is None:
            continue
        seen += 1
        rows = [(rng.integers(0, P, (nw, 2), dtype=np.uint64), rng.integers(0, P, (nk, 2), dtype=np.uint64),
                 rng.integers(0, P, 4, dtype=np.uint64)) for _ in range(8)]
        w, k, h, n = gc.gate_row(gi, 3, nw, nk)
        w2, k2 = np.zeros((nw, 2), np.uint64), np.zeros((nk, 2), np.uint64)
        w2[:, 0], k2[:, 0] = w, k
        rows.append((w2, k2, h))
        for wires, consts, pih in rows:
            want = _oracle_gate(s, wires, consts, pih)
            got = g.evaluate(wires, consts, pih)
            assert got.shape == want.shape == (g.num_commits, 2), (s, got.shape, want.shape)
            assert np.array_equal(got, want), (s, np.nonzero(got != want)[0][:4])
        assert not g.evaluate(*rows[-1]).any(), s   # the satisfying row satisfies the restatement
    assert seen >= 3   # mode 2, the small gate set, has three restated gates
    print(args, "restated gates:", seen)


def test_restatements_cover_the_listed_gates(p2v):
    kinds = set()
    for args in (MODE1, MODE2):
        for s in json.loads(gen_circuit(*args).common)["gates"]:
            if gp.restate(s) is not None:
                kinds.add(p2v._gate_words(s)[0])
    assert kinds == set(gp.RESTATED), sorted(set(gp.RESTATED) - kinds)


# ----------------------------------------------------------------------------- encoding and validation
MAGIC = 0x5032564700000001


def _words(*instrs, magic=MAGIC, count=None):
    w = [magic, len(instrs) if count is None else count]
    for i in instrs:
        w.extend(i)
    return np.array(w, dtype=np.uint64)


def _renamed(p2v):
    gc = gen_circuit(*MODE1)
    common, progs, idx = gp.rename(gc.common)
    return gc, common, progs, idx


def _create_with(p2v, gc, common, progs, name, words):
    progs = dict(progs)
    progs[name] = words
    return p2v.VerifierCircuitData.from_json(common, gc.vkey, gates=progs)


def test_encoding_errors(p2v):
    """Each error class of the format, by a minimal program."""
    gc, common, progs, idx = _renamed(p2v)
    c = json.loads(common)
    nw, nk = c["config"]["num_wires"], c["config"]["num_constants"]
    arith = next(s for s in c["gates"] if s.startswith(gp.PREFIX + "ArithmeticGate"))
    z2, z4 = np.zeros((nw, 2), np.uint64), np.zeros(4, np.uint64)

    def code(words, where="create"):
        with pytest.raises(p2v.P2VError) as e:
            if where == "create":
                _create_with(p2v, gc, common, progs, arith, words)
            else:
                p2v.gate_program_eval(words, z2, np.zeros((nk, 2), np.uint64), z4)
        return e.value.code

    ok = _words((0, 0), (0, 1), (4, 0, 1), (8, 2))
    assert p2v.gate_program_eval(ok, z2, np.zeros((nk, 2), np.uint64), z4).shape == (1, 2)
    for where in ("create", "eval"):
        assert code(_words((0, 0), (4, 0, 1), (8, 1)), where) == p2v.E_PARSE          # forward operand
        assert code(_words((0, 0), (4, 0, 0), (8, 2)), where) == p2v.E_PARSE          # COMMIT of a value not yet defined
        assert code(_words((0, 0), (9, 0)), where) == p2v.E_PARSE                     # bad opcode
        assert code(ok[:-1], where) == p2v.E_PARSE                                    # truncated
        assert code(_words((0, 0), count=2), where) == p2v.E_PARSE                    # fewer instructions than stated
        assert code(np.append(ok, np.uint64(0)), where) == p2v.E_PARSE                # trailing words
        assert code(_words((0, 0), magic=MAGIC + 1), where) == p2v.E_PARSE            # bad magic / version
        assert code(_words((0, nw), (8, 0)), where) == p2v.E_CIRCUIT                  # wire index
        assert code(_words((1, nk), (8, 0)), where) == p2v.E_CIRCUIT                  # constant index
        assert code(_words((2, 4), (8, 0)), where) == p2v.E_CIRCUIT                   # public-inputs-hash index
    # the last index of each is fine
    _create_with(p2v, gc, common, progs, arith, _words((0, nw - 1), (1, nk - 1), (2, 3), (8, 0), (8, 1), (8, 2)))


def test_registration_errors(p2v):
    gc, common, progs, idx = _renamed(p2v)
    c = json.loads(common)
    some = next(iter(progs))
    w = progs[some].words()
    L = p2v.lib()
    import ctypes
    cj, vj = bytes(common), bytes(gc.vkey)

    def create(pairs):
        arr = (p2v._GateProgramC * len(pairs))()
        keep = [(n.encode(), np.ascontiguousarray(x)) for n, x in pairs]
        for i, (n, x) in enumerate(keep):
            arr[i] = p2v._GateProgramC(n, len(n), x.ctypes.data, x.size)
        h = ctypes.c_void_p()
        rc = L.p2v_circuit_from_json_gates(cj, len(cj), vj, len(vj), 0, arr, len(pairs), ctypes.byref(h))
        if rc == 0:
            L.p2v_circuit_free(h)
        return rc
    allp = [(n, g.words()) for n, g in progs.items()]
    assert create(allp) == p2v.E_OK
    assert create(allp + [(some, w)]) == p2v.E_ARG                                    # the same string twice
    assert create(allp + [("ArithmeticGate { num_ops: 20 }", w)]) == p2v.E_ARG        # a built-in gate's string
    assert create(allp + [("NoopGate", w)]) == p2v.E_ARG
    assert create(allp + [("NobodyUsesThisGate", w)]) == p2v.E_OK                     # unused: ignored
    # unused and beyond the limits: still ignored; unused and malformed: the encoding error
    big = _words(*([(3, 1)] + [(4, 0, 0)] * p2v.GATE_PROGRAM_MAX_INSTRS))
    assert create(allp + [("NobodyUsesThisGate", big)]) == p2v.E_OK
    assert create(allp + [("NobodyUsesThisGate", w[:-1])]) == p2v.E_PARSE
    assert c["gates"].count(some) >= 1


def _chain(live):
    """A program with exactly `live` results alive at once: live sums of wire 0, then all read."""
    ins = [(0, 0)] + [(4, 0, 0)] * live
    acc = 1
    for v in range(2, live + 1):
        ins.append((4, acc, v))
        acc = live + v - 1
    ins.append((8, acc))
    return _words(*ins)


def test_limits(p2v):
    """One value over the live limit and one instruction over the instruction limit are
    P2V_E_CIRCUIT at creation; the limits themselves are accepted."""
    gc, common, progs, idx = _renamed(p2v)
    arith = next(s for s in progs if s.startswith(gp.PREFIX + "ArithmeticGate"))
    LIVE, INS = p2v.GATE_PROGRAM_MAX_LIVE, p2v.GATE_PROGRAM_MAX_INSTRS
    assert _lower(_decode(_chain(LIVE)))[1] == LIVE and _lower(_decode(_chain(LIVE + 1)))[1] == LIVE + 1
    _create_with(p2v, gc, common, progs, arith, _chain(LIVE))
    with pytest.raises(p2v.P2VError) as e:
        _create_with(p2v, gc, common, progs, arith, _chain(LIVE + 1))
    assert e.value.code == p2v.E_CIRCUIT and "alive" in e.value.message
    full = [(0, 0)] + [(4, 0, 0)] * (INS - 2) + [(8, 1)]
    _create_with(p2v, gc, common, progs, arith, _words(*full))
    with pytest.raises(p2v.P2VError) as e:
        _create_with(p2v, gc, common, progs, arith, _words(*(full + [(8, 1)])))
    assert e.value.code == p2v.E_CIRCUIT and "instructions" in e.value.message


# ----------------------------------------------------------------------------- circuit creation
def test_circuit_creation_with_programs(p2v):
    """The renamed circuit is refused without programs (today's behaviour) and accepted with them;
    everything derived from the circuit is the original's; the programs survive with_keys and
    shape_variant; the word encoding matches the UnknownGate's name."""
    gc, common, progs, idx = _renamed(p2v)
    orig = p2v.VerifierCircuitData.from_json(gc.common, gc.vkey)
    assert orig.num_program_gates == 0
    with pytest.raises(p2v.P2VError) as e:
        p2v.VerifierCircuitData.from_json(common, gc.vkey)
    assert e.value.code == p2v.E_CIRCUIT and "gateConstraints: unknown gate" in e.value.message
    with pytest.raises(p2v.P2VError) as e:
        p2v.VerifierCircuitData.from_json(common, gc.vkey, gates={})
    assert e.value.code == p2v.E_CIRCUIT
    some = next(iter(progs))
    with pytest.raises(p2v.P2VError) as e:   # one program missing
        p2v.VerifierCircuitData.from_json(common, gc.vkey, gates={k: v for k, v in progs.items() if k != some})
    assert e.value.code == p2v.E_CIRCUIT and some in e.value.message
    vk = p2v.VerifierCircuitData.from_json(common, gc.vkey, gates=progs)
    assert vk.num_program_gates == len(idx) >= 8
    assert vk.info == orig.info
    proof = gc.proof(1, 1)
    assert np.array_equal(vk.pack(proof), orig.pack(proof))
    assert np.array_equal(vk.pack_words(p2v.proof_words(proof)), orig.pack(proof))
    assert np.array_equal(vk.pack_many([proof, gc.proof(2, 2)]), orig.pack_many([proof, gc.proof(2, 2)]))
    keyed = vk.with_keys([gc.vkey])
    assert keyed.num_program_gates == len(idx) and keyed.num_keys == 2
    var = vk.shape_variant(vk.info.num_public_inputs + 1, vk.info.final_poly_len)
    assert var.num_program_gates == len(idx) and var.info.num_public_inputs == vk.info.num_public_inputs + 1
    # the word encoding: tag 16 with the renamed string as its name
    words = p2v.circuit_words(common, gc.vkey)
    with pytest.raises(p2v.P2VError) as e:
        p2v.VerifierCircuitData.from_words(words)
    assert e.value.code == p2v.E_CIRCUIT
    vw = p2v.VerifierCircuitData.from_words(words, gates=progs)
    assert vw.num_program_gates == len(idx) and vw.info == orig.info
    # the default call is the old one
    assert p2v.VerifierCircuitData.from_json(gc.common, gc.vkey, gates=None).info == orig.info
    assert p2v.VerifierCircuitData.from_json(gc.common, gc.vkey, gates=progs).num_program_gates == 0


# ----------------------------------------------------------------------------- lowering model
def _decode(words):
    """[(op, a, b)] of an encoding (well-formed here)."""
    w = [int(x) for x in words]
    out, i = [], 2
    for _ in range(w[1]):
        op = w[i]
        n = 2 if op in (4, 5, 6) else 1
        out.append((op, w[i + 1], w[i + 2] if n == 2 else None))
        i += 1 + n
    return out


def _lower(instrs):
    """The slot allocation of lower_gate_program restated: leaf values take no slot; a result is
    alive from its instruction to its last use; operands are read before the result is written, so
    a value's slot is free for the instruction that reads it last; the lowest free slot is taken.
    Returns ([(instruction, slot read or written...)], slots used, maximum alive at once)."""
    defs = [k for k, (op, a, b) in enumerate(instrs) if op != 8]
    leaf = [instrs[k][0] <= 3 for k in defs]
    last = list(defs)
    for k, (op, a, b) in enumerate(instrs):
        if op >= 4:
            last[a] = k
            if b is not None:
                last[b] = k
    slot, used, events, val, nslots, max_live = {}, set(), [], 0, 0, 0
    alive = set()
    for k, (op, a, b) in enumerate(instrs):
        if op <= 3:
            val += 1
            continue
        reads = [x for x in (a, b) if x is not None and not leaf[x]]
        for x in reads:
            events.append(("read", k, x, slot[x]))
        for x in reads:
            if last[x] == k:
                used.discard(slot[x])
                alive.discard(x)
        if op != 8:
            s = 0
            while s in used:
                s += 1
            used.add(s)
            alive.add(val)
            slot[val] = s
            events.append(("write", k, val, s))
            nslots = max(nslots, s + 1)
            max_live = max(max_live, len(alive))
            if last[val] == k:
                used.discard(s)
                alive.discard(val)
            val += 1
    return events, nslots, max_live


def _encode(instrs):
    return _words(*[tuple(x for x in ins if x is not None) for ins in instrs])


def _check_lowering(instrs):
    events, nslots, max_live = _lower(instrs)
    # the library's own lowering (csrc/circuit.cpp lower_gate_program) assigns as many slots
    info = p2v_module().gate_program_info(_encode(instrs))
    assert info["slots"] == nslots, (info, nslots)
    assert info["instructions"] == len(instrs) and info["commits"] == sum(op == 8 for op, _, _ in instrs)
    owner = {}
    for kind, k, v, s in events:
        if kind == "write":
            owner[s] = v
        else:
            assert owner[s] == v, ("slot read after reuse", k, v, s, owner[s])
    assert nslots == max_live, (nslots, max_live)
    return nslots


def _random_program(rng, n):
    instrs, nv = [(0, 0, None), (3, 5, None)], 2
    for _ in range(n):
        op = rng.choice([0, 1, 3, 4, 4, 5, 6, 6, 7, 8])
        if op <= 3:
            instrs.append((op, rng.randrange(4), None))
        elif op in (7, 8):
            instrs.append((op, rng.randrange(max(0, nv - 12), nv), None))
        else:
            instrs.append((op, rng.randrange(max(0, nv - 12), nv), rng.randrange(nv)))
        nv += op != 8
    return instrs


def test_lowering_model(p2v):
    """No slot is read after it was given to another value, and the slots used are exactly the
    maximum number of results alive at once: on the PoseidonGate program and on random programs.
    The library's lowering reports the same slot count for every one of them
    (p2v_gate_program_info), and the limit lies where the count says (test_limits)."""
    g = gp.restate("PoseidonGate(PhantomData<plonky2_field::goldilocks_field::GoldilocksField>)<WIDTH=12>")
    n = _check_lowering(_decode(g.words()))
    print("PoseidonGate program:", len(g.instrs), "instructions,", g.num_commits, "constraints,", n, "slots")
    assert g.num_commits == 123 and len(g.instrs) <= p2v.GATE_PROGRAM_MAX_INSTRS and n <= p2v.GATE_PROGRAM_MAX_LIVE
    rng = random.Random(7)
    for t in range(200):
        _check_lowering(_random_program(rng, rng.randrange(1, 120)))
