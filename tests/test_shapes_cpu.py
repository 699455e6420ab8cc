"""CPU tests that pin the references of tests/test_gpu_challenges.py and
tests/test_gpu_gate_params.py before the device is compared with them: circuits with 1, 3 and 4
challenge rounds, and gate parameters other than the generator's (tests/shapes.py).

The oracle's statuses and trace words are held against the three literal restatements: the
transcript and the FRI rounds (test_transcript_literal.py), C_i(zeta) and the quotient identity
(vanishing_literal.py) and verifyProof end to end (verifier_literal.py).  Exact integers
throughout: every comparison is ==."""
import json
import random

import numpy as np
import pytest

import gate_programs as gp
import shapes as SH
import vanishing_literal as VL
import verifier_literal as VLIT
from support import P, oracle, p2v_module, randomize_openings, trace_offsets
from test_gate_programs import _oracle_gate
from test_transcript_literal import fri_query_values, proof_challenges, sponge
from test_vanishing_literal import _check


def _pairs(tr, off, n):
    return [(int(tr[off + 2 * i]), int(tr[off + 2 * i + 1])) for i in range(n)]


def _offsets(common, pwpi):
    r = common["config"]["num_challenges"]
    S = len(pwpi["proof"]["opening_proof"]["commit_phase_merkle_caps"])
    Q = common["config"]["fri_config"]["num_query_rounds"]
    return r, S, Q, trace_offsets(r, S, Q)


# ----------------------------------------------------------------------------- challenge rounds
CONFIGS = {"real": dict(mode=1, lk=0), "real_lookup": dict(mode=1, lk=4), "degenerate_lookup": dict(mode=0, lk=1)}


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("nb", [6, 7])
@pytest.mark.parametrize("r", SH.ROUNDS)
def test_challenge_rounds_oracle_equals_the_literals(r, nb, cfg):
    """r = 1, 3, 4 at degree bits 6 and 7 (an odd degree), a real circuit without and with a lookup
    table and the degenerate circuit with two tables: on two valid proofs, one proof per generator
    flag and two proofs with uniform openings, the oracle's challenges, lookup deltas, query
    indices, per-query FRI values, C_i, quotient values and identity verdict equal the literals',
    and its status is the literal verifyProof's: 1 for the valid proofs, -3 or 0 for the rest."""
    gc = SH.circuit(nb, r=r, **CONFIGS[cfg])
    common, vkey = json.loads(gc.common), json.loads(gc.vkey)
    assert common["config"]["num_challenges"] == r
    seen = []
    for i, text in enumerate(SH.proof_pool(gc)):
        pwpi = json.loads(text)
        st, tr = oracle().verify_json(gc.common, gc.vkey, text, trace=True)
        seen.append(st)
        r_, S, Q, off = _offsets(common, pwpi)
        ch = proof_challenges(common, vkey, pwpi)
        words = [int(x) for x in tr]
        want = dict(ch, deltas=ch["deltas"] or [0] * (4 * r))
        k = 0
        for name, n in (("pi_hash", 4), ("betas", r), ("gammas", r), ("alphas", r), ("deltas", 4 * r), ("zeta", 2),
                        ("fri_alpha", 2), ("fri_betas", 2 * S), ("pow_response", 1), ("qidx", Q)):
            assert words[k:k + n] == want[name], (i, name)
            k += n
        assert k == off["combined"]
        assert bool(common["luts"]) == any(want["deltas"])
        comb, parts, eqs_ok = _check(common, vkey, pwpi, tr)
        if st >= 0:   # below 0 the reference raises before the folded values exist
            for q, (ini, fold, fin) in enumerate(fri_query_values(common, pwpi, ch)):
                assert _pairs(tr, off["q_initial"], Q)[q] == ini, (i, q)
                assert _pairs(tr, off["q_folded"], Q)[q] == fold, (i, q)
                assert _pairs(tr, off["q_final"], Q)[q] == fin, (i, q)
        assert VLIT.verify_proof(common, vkey, pwpi) == st, i
        if i < SH.N_VALID:
            assert st == 1 and eqs_ok
            if CONFIGS[cfg]["mode"] == 1:   # a real circuit: every term of every round is live
                assert all(x != (0, 0) for x in comb)
                assert all(x != (0, 0) for k in ("zs1", "pp", "lookup", "gates") for x in parts[k])
                assert len(parts["zs1"]) == r and len(parts["pp"]) == r * (common["num_partial_products"] + 1)
        else:
            assert st in (-3, 0), (i, st)
    assert seen[:2] == [1, 1] and set(seen[2:]) == {-3, 0}


def test_generator_refuses_other_round_counts():
    from support import generator
    for r in (0, 5, -1):
        with pytest.raises(RuntimeError) as e:
            generator().circuit(6, 4, 0, 1, 28, 16, 0, 1, num_challenges=r)
        assert "num_challenges" in str(e.value)


@pytest.mark.parametrize("r", SH.ROUNDS)
def test_generator_conventions_do_not_depend_on_the_round_count(r):
    """The generator's remaining switches at r = 1, 3, 4 give what they give at r = 2: flag 8
    accepts; MinSize arities, hiding salts, hash_or_noop leaves, ext 16 and a Fixed strategy each
    accept their valid proof and reject flags 1, 2 and 4 as -3, 0, 0 (the oracle, under the same
    conventions)."""
    O = oracle()
    g = SH.circuit(6, r=r)
    g2 = SH.circuit(6)
    assert O.verify_json(g.common, g.vkey, g.proof(1, 2, flags=8)) == O.verify_json(g2.common, g2.vkey, g2.proof(1, 2, flags=8)) == 1
    for ext, arities in ((1, (2, 2)), (2, ()), (4, (1, 1, 1)), (16, ()), (0, (3, 1))):
        g = SH.circuit(6, r=r, ext=ext, arities=arities)
        assert json.loads(g.common)["config"]["num_challenges"] == r
        got = [O.verify_json(g.common, g.vkey, g.proof(1, 2, flags=f), ext=ext) for f in (0, 1, 2, 4)]
        assert got == [1, -3, 0, 0], (ext, arities, got)


# ----------------------------------------------------------------------------- gate parameters
def _edge_pool():
    from test_gpu_field import _pool
    return _pool()


def _rows(seed, n=12):
    """(wires, constants, pi hash) rows: whole rows of one edge value, rows of edge values only,
    edge values among uniform ones, uniform rows."""
    pool = _edge_pool()
    rng = random.Random(seed)
    out = []
    for w in SH.edge_rows(pool, SH.NUM_WIRES, n - 2, seed):
        k = [[rng.choice(pool), rng.choice(pool)] for _ in range(SH.NUM_CONSTS)]
        h = [rng.choice(pool) for _ in range(4)]
        if len(out) < 6:   # the whole row is one value: constants and the public-input hash too
            k, h = [[w[0][0]] * 2] * SH.NUM_CONSTS, [w[0][0]] * 4
        out.append((w, k, h))
    for _ in range(2):
        out.append(([[rng.randrange(P), rng.randrange(P)] for _ in range(SH.NUM_WIRES)],
                    [[rng.randrange(P), rng.randrange(P)] for _ in range(SH.NUM_CONSTS)], [rng.randrange(P) for _ in range(4)]))
    return out


@pytest.mark.parametrize("kind,p", SH.ENTRIES, ids=lambda x: str(x).replace(" ", ""))
def test_gate_parameters_oracle_equals_the_literal(kind, p):
    """Every entry of the parameter table on edge-valued and uniform rows: or_eval_gate equals
    vanishing_literal.gate_constraints word for word, with as many constraints, and so does the
    gate's restatement as a gate program where tests/gate_programs.py has one.  No entry is
    dropped: the literal accepts every one, and so must the oracle."""
    s = SH.gate_string(kind, p)
    g = VL.parse_gate(s)
    prog = gp.restate(s)
    assert (prog is None) == (kind == "CosetInterpolation")
    for i, (w, k, h) in enumerate(_rows(1 + SH.ENTRIES.index((kind, p)))):
        wa, ka, ha = np.array(w, dtype=np.uint64), np.array(k, dtype=np.uint64), np.array(h, dtype=np.uint64)
        got = _oracle_gate(s, wa, ka, ha)
        want = VL.gate_constraints(g, VL.Vars([tuple(x) for x in k], [tuple(x) for x in w], h))
        assert [tuple(int(x) for x in row) for row in got] == want, (s[:60], i)
        if prog is not None:
            assert np.array_equal(prog.evaluate(wa, ka, ha), got), (s[:60], i)
    if kind == "CosetInterpolation":   # the reference's chunk count: zip3 of the chunked domain, values and weights
        assert len(want) == 2 + 4 * (SH.coset_parts(*p) - 1) + 2
        assert SH.coset_parts(*p) == {(4, 6, 10): 2, (4, 6, 3): 1}.get(p, ((1 << p[0]) - 2) // (p[1] - 1) + 1)


def unit_filter_combined(common, pwpi, ch):
    """C_i with every gate filter 1 (the parity mode of the oracle and the library), from the
    literal's unfiltered gate constraints.  Circuits without lookups only."""
    assert not common["luts"]
    _, parts = VL.all_plonk_constraints(common, pwpi, ch, sponge)
    gates = []
    for cons in parts["unfiltered"]:
        gates = VL.long_zip_add(gates, cons)
    terms = parts["zs1"] + parts["pp"] + gates
    return [VL.combine_with_powers_of_alpha(a, terms) for a in ch["alphas"]]


SWAPS = [({kind: p}, "%s%s" % (kind, str(p).replace(" ", ""))) for kind, p in SH.ENTRIES] + [(SH.ALL_AT_ONCE, "all")]


# r = 3 for the circuit with every kind replaced: the gate programs do not depend on r, the
# alpha-combination does
SWAP_CASES = [(s[0], 2, s[1]) for s in SWAPS] + [(SH.ALL_AT_ONCE, 3, "all-r3")]


@pytest.mark.parametrize("repl,r", [c[:2] for c in SWAP_CASES], ids=[c[2] for c in SWAP_CASES])
def test_swapped_circuit_combined_equals_the_literal(repl, r):
    """The mode-1 circuit with one gate string replaced by a table entry, and with every kind
    replaced at once (that one at r = 3 too): on a valid proof of the unswapped circuit and on one with
    uniform `constants` openings, the oracle's C_i equals the literal's, with the circuit's
    filters and with unit filters; every word is non-zero and differs from the unswapped
    circuit's, so the swapped gate is live.  The proof keeps its transcript and FRI rounds: only
    the identity fails."""
    gc = SH.circuit(6, r=r)
    common_b = SH.swap(gc.common, repl)
    common, vkey = json.loads(common_b), json.loads(gc.vkey)
    base = gc.proof(1, 1)
    for text in (base, randomize_openings(base, 7, keys=("constants",))):
        pwpi = json.loads(text)
        ch = proof_challenges(common, vkey, pwpi)
        _, _, _, off = _offsets(common, pwpi)
        st, tr = oracle().verify_json(common_b, gc.vkey, text, trace=True)
        _, tr0 = oracle().verify_json(gc.common, gc.vkey, text, trace=True)
        if text is not base:   # every filter is an arbitrary value: the swapped gate's term is in C_i
            assert st == 0
            comb, _, eqs_ok = _check(common, vkey, pwpi, tr)
            assert not eqs_ok and all(a != 0 and b != 0 for a, b in comb)
            assert all(x != y for x, y in zip(_pairs(tr, off["combined"], r), _pairs(tr0, off["combined"], r)))
        stu, tru = oracle().verify_json(common_b, gc.vkey, text, trace=True, unit_filters=True)
        _, tru0 = oracle().verify_json(gc.common, gc.vkey, text, trace=True, unit_filters=True)
        got = _pairs(tru, off["combined"], r)
        assert stu == 0 and got == unit_filter_combined(common, pwpi, ch)
        assert all(a != 0 and b != 0 for a, b in got)
        assert all(x != y for x, y in zip(got, _pairs(tru0, off["combined"], r)))
        keep = np.ones(len(tr), dtype=bool)   # everything but C_i and the verdict is the unswapped circuit's
        keep[off["combined"]: off["combined"] + 2 * r] = False
        keep[off["flags"]] = False
        assert np.array_equal(tru[keep], tru0[keep])


def test_unit_filter_literal_on_the_unswapped_circuit():
    """unit_filter_combined itself, where nothing is swapped: the oracle's unit-filter C_i of the
    generator's own circuit (the reference of test_gpu's unit-filter tests)."""
    for r in (2, 3):
        gc = SH.circuit(6, r=r)
        text = gc.proof(1, 1)
        common, pwpi = json.loads(gc.common), json.loads(text)
        _, _, _, off = _offsets(common, pwpi)
        _, tru = oracle().verify_json(gc.common, gc.vkey, text, trace=True, unit_filters=True)
        assert _pairs(tru, off["combined"], r) == unit_filter_combined(common, pwpi, proof_challenges(common, json.loads(gc.vkey), pwpi))


# ----------------------------------------------------------------------------- the refusal
def test_coset_gate_beyond_the_wires_is_refused():
    """CosetInterpolationGate{bits 6, degree 63} has one intermediate pair: its shifted_loc is
    wires 137-138 of 135 and the reference's wire lookup raises; degree 64 has none, reads up to
    wire 134 and loads."""
    p2v = p2v_module()
    gc = SH.circuit(6)
    with pytest.raises(p2v.P2VError) as e:
        p2v.VerifierCircuitData.from_json(SH.swap(gc.common, {"CosetInterpolation": (6, 63)}), gc.vkey)
    assert e.value.code == p2v.E_CIRCUIT and "(Array.!)" in e.value.message and "wire" in e.value.message
    vk = p2v.VerifierCircuitData.from_json(SH.swap(gc.common, {"CosetInterpolation": (6, 64)}), gc.vkey)
    assert vk.info == p2v.VerifierCircuitData.from_json(gc.common, gc.vkey).info


def test_every_table_entry_loads():
    """Each entry, and all kinds at once, is a circuit the library accepts at r = 2 and r = 3."""
    p2v = p2v_module()
    for r in (2, 3):
        gc = SH.circuit(6, r=r)
        for repl, _ in SWAPS:
            vk = p2v.VerifierCircuitData.from_json(SH.swap(gc.common, repl), gc.vkey)
            assert vk.info.num_challenges == r
