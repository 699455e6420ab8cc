"""GPU tests (MI355X) of circuits with 1, 3 and 4 challenge rounds (config.num_challenges; the
generator's default and every other GPU test: 2).  r != 2 takes the generic forms of the five
vanishing kernels (k_vanish_rn, k_vanish_poseidon_rn, k_vanish_coset_rn, k_vanish_lookup_rn,
k_vanish_prog_rn) and changes every r-dependent size: the challenge counts of the transcript
kernels, the leaf widths of k_leaf and k_fri, the stride of the vanishing parts, the trace layout
of k_status and the word offsets of the device packers.

The references are pinned by tests/test_shapes_cpu.py.  Statuses and full traces equal the
oracle's with ==; every test asserts the status classes it reached."""
import json

import numpy as np
import pytest

import shapes as SH
from support import P, oracle, p2v_module, proof_bytes, trace_offsets

pytestmark = pytest.mark.gpu

CONFIGS = {"real": dict(mode=1, lk=0), "real_lookup": dict(mode=1, lk=4), "degenerate_lookup": dict(mode=0, lk=2, ng=3)}


@pytest.fixture(scope="module")
def p2v():
    import torch   # before libp2v, as tests/test_gpu.py
    assert torch.cuda.is_available(), "torch sees no GPU"
    m = p2v_module()
    if m.device_count() == 0:
        pytest.fail("no GPU visible to libp2v")
    return m


def kernels(vk, gates):
    """The vanishing kernels a run of this circuit launches (csrc/api_run.cpp), from r and the classes
    its gates fall into."""
    sfx = "_r2" if vk.info.num_challenges == 2 else "_rn"
    out = ["k_vanish" + sfx]
    if any(s.startswith("PoseidonGate") for s in gates):
        out.append("k_vanish_poseidon" + sfx)
    if any(s.startswith("CosetInterpolationGate") for s in gates):
        out.append("k_vanish_coset" + sfx)
    if vk.info.has_lookups:
        out.append("k_vanish_lookup" + sfx)
    if vk.num_program_gates:
        out.append("k_vanish_prog" + sfx)
    return out


class Case:
    """A circuit, its proof pool (shapes.proof_pool) packed once, and the oracle's status and
    trace of every pool proof, computed once per filter mode and never changed."""

    def __init__(self, p2v, gc, ext=0, texts=None, common=None):
        self.gc, self.ext = gc, ext
        self.common = gc.common if common is None else common   # the circuit verified: gc's, or gc's with gates swapped
        self.vk = p2v.VerifierCircuitData.from_json(self.common, gc.vkey, ext)
        self.texts = SH.proof_pool(gc) if texts is None else texts
        self.packed = self.vk.pack_many(self.texts)
        i = self.vk.info
        self.r = i.num_challenges
        self.off = trace_offsets(i.num_challenges, i.num_fri_steps, i.num_query_rounds)
        self.gates = json.loads(self.common)["gates"]
        self._want = {}

    def want(self, unit_filters=False):
        if unit_filters not in self._want:
            O = oracle()
            c = O.circuit(self.common, self.gc.vkey, self.ext)
            res = []
            for t in self.texts:
                pr = O.proof(t)
                res.append(O.verify(c, pr, trace=True, unit_filters=unit_filters))
                O.L.or_proof_free(pr)
            O.L.or_circuit_free(c)
            self._want[unit_filters] = np.array([st for st, _ in res]), np.array([tr for _, tr in res])
        return self._want[unit_filters]

    def combined(self, tr):
        return tr[..., self.off["combined"]: self.off["combined"] + 2 * self.r]

    def check(self, p2v, n, tiled=False, unit_filters=False, sel=None):
        """n pool proofs in turn through one run: statuses and traces equal the oracle's."""
        sel = np.arange(n) % len(self.texts) if sel is None else sel
        st, tr = self.want(unit_filters)
        res, got = p2v.BatchVerifier(self.vk, 0, n).run(np.ascontiguousarray(self.packed[sel]), trace=True, tiled=tiled,
                                                       unit_filters=unit_filters)
        assert np.array_equal(res, st[sel]), (res.tolist(), st[sel].tolist())
        bad = np.nonzero((got != tr[sel]).any(axis=1))[0]
        assert len(bad) == 0, (bad[:8], np.nonzero(got[bad[0]] != tr[sel][bad[0]])[0][:10])
        return st[sel], tr[sel]


_cases = {}


def case(p2v, r, cfg="real", nb=6, **kw) -> Case:
    key = (r, cfg, nb, tuple(sorted(kw.items())))
    if key not in _cases:
        _cases[key] = Case(p2v, SH.circuit(nb, r=r, **CONFIGS[cfg], **kw), ext=kw.get("ext", 0))
    return _cases[key]


# ----------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("n,tiled", [(5, False), (5, True), (70, False), (70, True)])
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("r", SH.ROUNDS)
def test_gpu_challenge_rounds_vs_oracle(p2v, r, cfg, n, tiled):
    """r = 1, 3, 4: a real circuit, a real circuit with one lookup table and the degenerate circuit
    with two tables in three selector groups; n = 5 (the latency path, k_merkle_row) and n = 70 (the
    batch path: one full tile and a ragged one), proof-major and tiled; valid proofs, the
    generator's three reject classes and proofs with uniform openings.  Then the same batch with
    every filter 1: each C_i is non-zero and the oracle's."""
    D = case(p2v, r, cfg)
    assert D.vk.info.num_challenges == r and D.vk.info.has_lookups == (cfg != "real")
    print("r =", r, cfg, "n =", n, "kernels:", kernels(D.vk, D.gates))
    st, tr = D.check(p2v, n, tiled)
    assert {1, -3, 0} <= set(st.tolist()), st.tolist()
    if cfg != "degenerate_lookup":   # a real circuit: C_i is live on every proof
        assert (D.combined(tr) != 0).all()
    _, tru = D.check(p2v, n, tiled, unit_filters=True)
    assert (D.combined(tru) != 0).all()
    assert (D.combined(tru) != D.combined(tr)).all()   # the mode is live
    if cfg != "real":
        nl = len(json.loads(D.gc.common)["luts"])
        assert (tru[:, D.off["lut_re"]: D.off["lut_re"] + r * nl] != 0).all()


@pytest.mark.parametrize("form", ["row", "quad", "lane"])
@pytest.mark.parametrize("cfg", ["real", "real_lookup"])
@pytest.mark.parametrize("r", [3, 4])
def test_gpu_challenge_rounds_transcript_forms(p2v, r, cfg, form, monkeypatch):
    """Each transcript layout forced in turn (P2V_TRANSCRIPT): 3r or 3r + 2r squeezed challenges
    around the caps; at r = 4 the betas and gammas are exactly one rate block."""
    monkeypatch.setenv("P2V_TRANSCRIPT", form)
    D = case(p2v, r, cfg)
    st, _ = D.check(p2v, len(D.texts))
    assert {1, -3, 0} <= set(st.tolist())


# ----------------------------------------------------------------------------- Merkle paths
def _merkle_cases(D):
    """A valid proof, then copies with one word changed: a sibling and a leaf word in each of the
    four initial trees (leaf widths: constants and sigmas, 135, r (1 + npp + nlp), r qdf) and a sibling in the step tree."""
    base = D.texts[0]
    out = [base]
    Q = D.vk.info.num_query_rounds

    def change(f):
        d = json.loads(base)
        f(d["proof"]["opening_proof"]["query_round_proofs"])
        out.append(json.dumps(d, separators=(",", ":")).encode())

    for t in range(4):
        def sib(qr, t=t):
            s = qr[(5 * t + 1) % Q]["initial_trees_proof"]["evals_proofs"][t][1]["siblings"]
            e = s[t % len(s)]["elements"]
            e[t] = (e[t] + 1) % P

        def leaf(qr, t=t):
            ev = qr[(3 * t + 2) % Q]["initial_trees_proof"]["evals_proofs"][t][0]
            ev[-1] = (ev[-1] + 1) % P   # the last word: its place depends on r in trees 2 and 3
        change(sib)
        change(leaf)

    def step(qr):
        s = qr[11 % Q]["steps"][0]["merkle_proof"]["siblings"]
        assert s, "the step tree has no level below its cap"
        s[-1]["elements"][2] = (s[-1]["elements"][2] + 1) % P
    change(step)
    return out


@pytest.mark.parametrize("cfg", ["real", "real_lookup"])
def test_gpu_challenge_rounds_merkle_paths(p2v, cfg, monkeypatch):
    """r = 3 on the batch path (P2V_LAT_MAX=0): one sibling or leaf word changed in each initial
    tree and in the step tree.  The shared-node kernels (P2V_MERKLE_CSE=1) and the plain one
    (P2V_MERKLE_CSE=0) both give the oracle's words, -1 and -2 among them."""
    base = case(p2v, 3, cfg)
    D = Case(p2v, base.gc, texts=_merkle_cases(base))
    assert D.vk.info.leaf_widths[2] == 3 * (1 + 9 + (7 if cfg == "real_lookup" else 0)) and D.vk.info.leaf_widths[3] == 3 * 8
    monkeypatch.setenv("P2V_LAT_MAX", "0")
    seen = []
    for cse in ("1", "0"):
        monkeypatch.setenv("P2V_MERKLE_CSE", cse)
        st, _ = D.check(p2v, len(D.texts))
        seen.append(st.tolist())
    assert seen[0] == seen[1] == [1] + [-1] * 8 + [-2]


# ----------------------------------------------------------------------------- keys and ingest
def test_gpu_challenge_rounds_keyed_batch(p2v):
    """r = 3, two verifier keys over one common data: proof i against key ids[i] equals the oracle
    run with that key, on the batch path (n = 70) and the latency path (n = 3)."""
    g1, g2 = SH.circuit(6, r=3), SH.circuit(6, r=3, seed=2)
    assert g1.common == g2.common and g1.vkey != g2.vkey
    vk = p2v.VerifierCircuitData.from_json(g1.common, g1.vkey).with_keys([g2.vkey])
    assert vk.num_keys == 2 and vk.info.num_challenges == 3
    texts = [g1.proof(1, 1), g2.proof(1, 1), g1.proof(1, 3, flags=4), g2.proof(2, 2), g2.proof(1, 4, flags=1)]
    O = oracle()
    want = {(k, j): O.verify_json(g1.common, (g1, g2)[k].vkey, t, trace=True) for k in range(2) for j, t in enumerate(texts)}
    assert {int(st) for st, _ in want.values()} >= {1, 0, -3}
    packed = vk.pack_many(texts)
    for n in (70, 3):
        sel = np.arange(n) % len(texts) if n > 3 else np.array([0, 3, 4])
        ids = ((np.arange(n) // len(texts)) % 2 if n > 3 else np.array([0, 1, 1])).astype(np.uint32)   # n = 70: every (key, proof) pair
        res, tr = p2v.BatchVerifier(vk, 0, n).run(np.ascontiguousarray(packed[sel]), trace=True, key_ids=ids)
        for i in range(n):
            st, otr = want[(int(ids[i]), int(sel[i]))]
            assert int(res[i]) == int(st) and np.array_equal(tr[i], otr), (n, i)
        assert {int(x) for x in res} >= ({1, 0, -3} if n > 3 else {1, -3})


def test_gpu_challenge_rounds_bytes_ingest(p2v):
    """k_bytes_pack at r = 3 with a lookup table (leaf widths 51 and 24, 21 lookup openings twice):
    the assertions of test_gpu.test_gpu_bytes_ingest_matches_host_reader on this circuit."""
    from test_gpu import test_gpu_bytes_ingest_matches_host_reader as body
    gc = SH.circuit(6, lk=4, r=3)
    body(p2v, (6, 4, 4, 1, 28, 16, 0, 1, 0, (), 3), 0)
    # and the packed words against the JSON path's, proof by proof
    vk = p2v.VerifierCircuitData.from_json(gc.common, gc.vkey)
    texts = SH.proof_pool(gc)
    words, codes = p2v.BatchVerifier(vk, 0, len(texts)).pack_bytes([proof_bytes(t, pi_prefix=bool(i % 2)) for i, t in enumerate(texts)])
    assert not codes.any() and np.array_equal(words, vk.pack_many(texts))


def test_gpu_challenge_rounds_json_ingest(p2v):
    """k_json_pack at r = 3 with a lookup table: texts in the template's format take the device
    packer, a re-indented and a truncated text the host reader; decode codes, packed words and
    statuses equal the host packer's (p2v_pack_proofs_json) followed by a plain run."""
    D = case(p2v, 3, "real_lookup")
    texts = list(D.texts) + [json.dumps(json.loads(D.texts[1]), indent=1).encode(), D.texts[0][:-9], b"[]"] + list(D.texts[:2])
    codes_h = np.empty(len(texts), np.int32)
    packed = D.vk.pack_many(texts, codes=codes_h)
    ok = codes_h == 0
    assert ok.sum() == len(texts) - 2
    want = np.where(ok, 0, np.where(codes_h == -3, -5, -7)).astype(np.int8)
    bv = p2v.BatchVerifier(D.vk, 0, len(texts))
    want[ok] = bv.run(np.ascontiguousarray(packed[ok]))
    res, codes = bv.run_json(texts)
    assert list(codes) == list(codes_h) and list(res) == list(want)
    assert bv.last_json_device >= 5 + 2   # at least the generator's own texts
    st, _ = D.want()
    assert list(res[: len(D.texts)]) == st.tolist() and {1, -3, 0} <= set(st.tolist())
    words, codes2 = bv.pack_json(texts)
    assert list(codes2) == list(codes_h)
    assert np.array_equal(words[ok], packed[ok]) and not words[~ok].any()


# ----------------------------------------------------------------------------- gate programs
@pytest.mark.parametrize("n", [128, 3])
@pytest.mark.parametrize("r", [3, 1])
def test_gpu_challenge_rounds_gate_programs(p2v, r, n):
    """The restated gates of the real circuit as registered programs (test_gpu_gate_programs'
    Renamed) at r = 3 and r = 1: k_vanish_prog_rn on the batch path (n = 128) and the latency path
    (n = 3).  Equal to the oracle on the original JSON and to the built-in kernels."""
    import test_gpu_gate_programs as TP
    D = TP._get(p2v, (6, 4, 0, 1, 28, 16, 0, 1, 0, (), r))
    assert D.vk.info.num_challenges == r
    print("r =", r, "n =", n, "kernels:", kernels(D.vk, json.loads(D.common)["gates"]))
    sel = (np.arange(n) + (0 if n > 3 else 1)) % len(D.texts)
    rows = np.ascontiguousarray(D.packed[sel])
    want = [TP._oracle(D.gc, D.texts[j]) for j in sel]
    assert {int(st) for st, _ in want} >= {1, 0}
    for st, otr in want:
        assert (TP._combined(D.orig, otr) != 0).all()
    res, tr = p2v.BatchVerifier(D.vk, 0, n).run(rows, trace=True)
    ref, rtr = p2v.BatchVerifier(D.orig, 0, n).run(rows, trace=True)
    for i, (st, otr) in enumerate(want):
        assert int(res[i]) == int(st) and np.array_equal(tr[i], otr), (i, np.nonzero(tr[i] != otr)[0][:10])
    assert np.array_equal(res, ref) and np.array_equal(tr, rtr)
    # every filter 1: a program that was skipped could not pass
    resu, tru = p2v.BatchVerifier(D.vk, 0, n).run(rows, trace=True, unit_filters=True)
    for i, j in enumerate(sel):
        st, otr = TP._oracle(D.gc, D.texts[j], unit_filters=True)
        assert int(resu[i]) == int(st) and np.array_equal(tru[i], otr), (i, np.nonzero(tru[i] != otr)[0][:10])


# ----------------------------------------------------------------------------- other step trees
@pytest.mark.parametrize("n", [5, 70])
def test_gpu_challenge_rounds_ext_arities(p2v, n):
    """r = 3 at degree bits 7 with steps of arity 8 and 4 under MinSize, hiding salts and
    hash_or_noop leaves (ext 7): two step trees of other widths, salted leaves of 3 (1 + npp) + 4
    and 3 qdf + 4 words."""
    D = case(p2v, 3, "real", nb=7, ext=7, arities=(3, 2))
    assert D.vk.info.step_arity_bits == (3, 2) and D.vk.info.num_challenges == 3
    st, tr = D.check(p2v, n)
    assert {1, -3, 0} <= set(st.tolist()) and (D.combined(tr) != 0).all()
