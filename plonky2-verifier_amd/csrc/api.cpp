// api.cpp — the C-ABI of libp2v (include/p2v.h): the drop-in boundary for
// verifyProof :: VerifierCircuitData -> ProofWithPublicInputs -> Bool
// (reference src/Plonk/Verifier.hs:56-65), batched, on MI355X.  This unit: the circuit handle's
// entry points; the workspace, the batch run, the host pipeline, the ingest and the self-tests are
// api_workspace.cpp, api_run.cpp, api_pipe.cpp, api_ingest.cpp and api_selftest.cpp.
#include <cstring>
#include <thread>
#include "api_internal.hpp"
#include "gl.h"

thread_local std::string g_err;

p2v_circuit::~p2v_circuit() {
  for (HostPipe* p : pool) pipe_free(p);
  for (auto& k : known) { (void)hipSetDevice(k->device); k.reset(); }
}

// Keys in ascending index order, a key equal to an earlier one skipped: the lowest index wins.
const std::vector<uint32_t>& p2v_circuit::key_lookup() const {
  std::call_once(key_tab_once, [&] {
    const size_t nk = c.num_keys();
    const int kw = c.key_words();
    size_t size = 2;
    while (size < 2 * nk) size <<= 1;
    key_tab.assign(size, 0);
    const uint32_t mask = (uint32_t)size - 1;
    for (size_t k = 0; k < nk; k++) {
      uint64_t h = 0;
      for (int i = 0; i < kw; i++) h = p2v_key_hash(h, c.key_word(k, i));
      uint32_t slot = (uint32_t)h & mask;
      for (; key_tab[slot]; slot = (slot + 1) & mask) {
        const size_t e = key_tab[slot] - 1;
        int i = 0;
        while (i < kw && c.key_word(e, i) == c.key_word(k, i)) i++;
        if (i == kw) break;
      }
      if (!key_tab[slot]) key_tab[slot] = (uint32_t)k + 1;
    }
  });
  return key_tab;
}

extern "C" {

const char* p2v_last_error_message(void) { return g_err.c_str(); }
const char* p2v_kernel_names(void) { return kKernelNames; }

int p2v_circuit_from_json(const char* common_json, size_t common_len, const char* vkey_json, size_t vkey_len, p2v_circuit** out) {
  return p2v_circuit_from_json_ex(common_json, common_len, vkey_json, vkey_len, 0, out);
}

int p2v_circuit_from_json_ex(const char* common_json, size_t common_len, const char* vkey_json, size_t vkey_len, uint32_t ext,
                             p2v_circuit** out) {
  return p2v_circuit_from_json_gates(common_json, common_len, vkey_json, vkey_len, ext, nullptr, 0, out);
}

// the caller's gate programs, decoded (P2V_E_PARSE) after the checks that need no circuit:
// P2V_E_ARG for a string registered twice or one that is a built-in gate's
static int named_programs(const p2v_gate_program* progs, size_t nprogs, std::vector<NamedGateProgram>& out) {
  if (nprogs && !progs) return fail(P2V_E_ARG, "null argument");
  for (size_t i = 0; i < nprogs; i++) {
    if (!progs[i].gate || (!progs[i].words && progs[i].nwords)) return fail(P2V_E_ARG, "null argument");
    std::string name(progs[i].gate, progs[i].gate_len);
    for (const auto& np : out) if (np.gate == name) return fail(P2V_E_ARG, "gate program registered twice: " + name);
    if (parse_gate_string(name).kind != G_UNKNOWN) return fail(P2V_E_ARG, "a gate program cannot override a built-in gate: " + name);
    out.push_back(NamedGateProgram{std::move(name), GateProgram{}});
  }
  return guarded(P2V_E_PARSE, [&] {
    for (size_t i = 0; i < nprogs; i++) out[i].prog = decode_gate_program(progs[i].words, progs[i].nwords);
  });
}

int p2v_circuit_from_json_gates(const char* common_json, size_t common_len, const char* vkey_json, size_t vkey_len, uint32_t ext,
                                const p2v_gate_program* progs, size_t nprogs, p2v_circuit** out) {
  if (!common_json || !vkey_json || !out) return fail(P2V_E_ARG, "null argument");
  if (ext & ~P2V_EXT_PLONKY2) return fail(P2V_E_ARG, "unknown P2V_EXT_* flag");
  std::vector<NamedGateProgram> np;
  RCK(named_programs(progs, nprogs, np));
  return guarded(P2V_E_PARSE, [&] {
    JVal cj = parse_json(common_json, common_len);
    JVal vj = parse_json(vkey_json, vkey_len);
    auto pc = std::make_unique<p2v_circuit>();
    pc->c = parse_circuit(cj, vj, ext, np);
    *out = pc.release();
  });
}

int p2v_circuit_num_program_gates(const p2v_circuit* pc) {
  if (!pc) return fail(P2V_E_ARG, "null argument");
  int k = 0;
  for (int g = 0; g < pc->c.n_gate_eval; g++) k += pc->c.gates[g].kind == G_PROGRAM;
  return k;
}

int p2v_gate_program_info(const uint64_t* words, size_t nwords, int64_t info[4]) {
  if (!words || !info) return fail(P2V_E_ARG, "null argument");
  return guarded(P2V_E_PARSE, [&] {
    const GateProgram g = decode_gate_program(words, nwords);
    info[0] = (int64_t)g.size(); info[1] = g.num_commits; info[2] = (int64_t)g.def.size();
    info[3] = lower_gate_program(g, nullptr);
  });
}

int p2v_gate_program_eval(const uint64_t* words, size_t nwords, const uint64_t* wires, int nwires, const uint64_t* consts, int nconsts,
                          const uint64_t pih[4], uint64_t* out, int maxout) {
  if (!words || nwires < 0 || nconsts < 0 || maxout < 0 || (nwires && !wires) || (nconsts && !consts) || (maxout && !out))
    return fail(P2V_E_ARG, "null argument");
  int n = 0;
  const int rc = guarded(P2V_E_PARSE, [&] {
    const GateProgram g = decode_gate_program(words, nwords);
    if (g.max_wire >= nwires) throw CircuitError("(Array.!): gate program reads a wire beyond the row");
    if (g.max_const >= nconsts) throw CircuitError("(Array.!): gate program reads a constant beyond the row");
    if (g.max_pih >= 4) throw CircuitError("(!!): gate program reads a public-inputs-hash word beyond 4");
    if (g.max_pih >= 0 && !pih) throw CircuitError("gate program reads the public-inputs hash, none given");
    n = g.num_commits;
    if (n <= maxout) eval_gate_program(g, wires, consts, pih, out);
  });
  if (rc != P2V_OK) return rc;
  if (n > maxout) return fail(P2V_E_ARG, "p2v_gate_program_eval: more constraints than maxout");
  return n;
}

int p2v_circuit_from_words(const uint64_t* words, size_t n, p2v_circuit** out) {
  return p2v_circuit_from_words_ex(words, n, 0, out);
}

int p2v_circuit_from_words_ex(const uint64_t* words, size_t n, uint32_t ext, p2v_circuit** out) {
  return p2v_circuit_from_words_gates(words, n, ext, nullptr, 0, out);
}

int p2v_circuit_from_words_gates(const uint64_t* words, size_t n, uint32_t ext, const p2v_gate_program* progs, size_t nprogs,
                                 p2v_circuit** out) {
  if (!words || !out) return fail(P2V_E_ARG, "null argument");
  if (ext & ~P2V_EXT_PLONKY2) return fail(P2V_E_ARG, "unknown P2V_EXT_* flag");
  std::vector<NamedGateProgram> np;
  RCK(named_programs(progs, nprogs, np));
  return guarded(P2V_E_PARSE, [&] {
    auto pc = std::make_unique<p2v_circuit>();
    pc->c = parse_circuit_words(words, n, ext, np);
    *out = pc.release();
  });
}

int p2v_pack_proof_words(const p2v_circuit* pc, const uint64_t* words, size_t n, uint64_t* dst) {
  if (!pc || !words || !dst) return fail(P2V_E_ARG, "null argument");
  return guarded(P2V_E_PARSE, [&] { pack_proof_words(pc->c, words, n, dst); });
}

int p2v_pack_proof_bytes(const p2v_circuit* pc, const uint8_t* bytes, size_t n, uint64_t* dst) {
  if (!pc || !bytes || !dst) return fail(P2V_E_ARG, "null argument");
  return guarded(P2V_E_PARSE, [&] { pack_proof_bytes(pc->c, bytes, n, dst); });
}

void p2v_circuit_free(p2v_circuit* c) { delete c; }

int p2v_circuit_get_info(const p2v_circuit* pc, p2v_circuit_info* info) {
  if (!pc || !info) return fail(P2V_E_ARG, "null argument");
  const Circuit& c = pc->c;
  memset(info, 0, sizeof *info);
  info->degree_bits = c.degree_bits; info->lde_bits = c.lde_bits; info->cap_height = c.cap_height;
  info->num_challenges = c.r; info->num_query_rounds = c.num_queries; info->num_fri_steps = (int)c.arities.size();
  info->final_poly_len = c.final_len; info->num_public_inputs = c.num_pis;
  info->num_openings_this = (int)c.L.n_this; info->num_openings_next = (int)c.L.n_next;
  info->has_lookups = c.lut_in.empty() ? 0 : 1; info->num_gates = (int)c.gates.size();
  info->proof_words = c.L.words; info->trace_words = c.trace_words;
  for (int t = 0; t < 4; t++) { info->oracle_widths[t] = c.oracle_width[t]; info->leaf_widths[t] = c.leaf_width[t]; }
  info->ext = c.ext;
  for (size_t s = 0; s < c.arities.size() && s < 8; s++) info->step_arity_bits[s] = c.arities[s];
  return P2V_OK;
}

int p2v_pack_proof_json(const p2v_circuit* pc, const char* proof_json, size_t len, uint64_t* dst) {
  if (!pc || !proof_json || !dst) return fail(P2V_E_ARG, "null argument");
  return guarded(P2V_E_PARSE, [&] {
    JVal pj = parse_json(proof_json, len);
    pack_proof(pc->c, pj, dst);
  });
}

int p2v_proof_shape_json(const char* proof_json, size_t len, int* num_public_inputs, int* final_poly_len) {
  if (!proof_json || !num_public_inputs || !final_poly_len) return fail(P2V_E_ARG, "null argument");
  try {
    proof_shape_json(parse_json(proof_json, len), *num_public_inputs, *final_poly_len);
    return P2V_OK;
  } catch (const std::exception& e) { return fail(P2V_E_PARSE, e.what()); }
}

int p2v_proof_shape_words(const uint64_t* words, size_t n, int* num_public_inputs, int* final_poly_len) {
  if (!words || !num_public_inputs || !final_poly_len) return fail(P2V_E_ARG, "null argument");
  try {
    proof_shape_words(words, n, *num_public_inputs, *final_poly_len);
    return P2V_OK;
  } catch (const std::exception& e) { return fail(P2V_E_PARSE, e.what()); }
}

int p2v_circuit_shape_variant(const p2v_circuit* pc, int num_public_inputs, int final_poly_len, p2v_circuit** out) {
  if (!pc || !out) return fail(P2V_E_ARG, "null argument");
  *out = nullptr;
  try {   // its own mapping: a CircuitError here is the proof's shape past this build's limits
    auto v = std::make_unique<p2v_circuit>();
    v->c = circuit_shape_variant(pc->c, num_public_inputs, final_poly_len);
    *out = v.release();
    return P2V_OK;
  } catch (const std::exception& e) { return fail(P2V_E_SHAPE, e.what()); }
}

int p2v_vkey_from_json(const p2v_circuit* pc, const char* vkey_json, size_t len, uint64_t* dst) {
  if (!pc || !vkey_json || !dst) return fail(P2V_E_ARG, "null argument");
  return guarded(P2V_E_PARSE, [&] { vkey_words(pc->c, parse_json(vkey_json, len), dst); });
}

int p2v_circuit_with_keys(const p2v_circuit* base, const uint64_t* key_words, size_t nkeys, p2v_circuit** out) {
  if (!base || !out || (nkeys && !key_words)) return fail(P2V_E_ARG, "null argument");
  *out = nullptr;
  const Circuit& B = base->c;
  if (nkeys > (size_t)P2V_MAX_KEYS || B.num_keys() + nkeys > (size_t)P2V_MAX_KEYS)
    return fail(P2V_E_ARG, "p2v_circuit_with_keys: more than P2V_MAX_KEYS keys");
  return guarded(P2V_E_ARG, [&] {
    auto v = std::make_unique<p2v_circuit>();
    v->c = B;
    const size_t nw = nkeys * (size_t)B.key_words();
    v->c.extra_keys.reserve(B.extra_keys.size() + nw);
    for (size_t i = 0; i < nw; i++) v->c.extra_keys.push_back(key_words[i] % gl::P);
    *out = v.release();
  });
}

int p2v_circuit_num_keys(const p2v_circuit* pc) {
  if (!pc) return fail(P2V_E_ARG, "null argument");
  return (int)pc->c.num_keys();
}

int p2v_circuit_find_key(const p2v_circuit* pc, const uint64_t* key_words) {
  if (!pc || !key_words) return fail(P2V_E_ARG, "null argument");
  const Circuit& C = pc->c;
  const int kw = C.key_words();
  const std::vector<uint32_t>& tab = pc->key_lookup();
  const uint32_t mask = (uint32_t)tab.size() - 1;
  uint64_t h = 0;
  for (int i = 0; i < kw; i++) h = p2v_key_hash(h, key_words[i] % gl::P);
  uint32_t slot = (uint32_t)h & mask;
  for (size_t probes = 0; probes < tab.size() && tab[slot]; probes++, slot = (slot + 1) & mask) {
    const size_t k = tab[slot] - 1;
    int i = 0;
    while (i < kw && C.key_word(k, i) == key_words[i] % gl::P) i++;
    if (i == kw) return (int)k;
  }
  return -1;
}

int p2v_key_from_public_inputs(const p2v_circuit* pc, const uint64_t* pis, size_t npis, uint64_t* key_words) {
  if (!pc || (!pis && npis) || !key_words) return fail(P2V_E_ARG, "null argument");
  const int kw = pc->c.key_words(), cap_len = pc->c.cap_len;
  if (npis < (size_t)kw) return fail(P2V_E_SHAPE, "public inputs shorter than a verifier key (4 + 4 * cap_len words)");
  const uint64_t* tail = pis + (npis - (size_t)kw);
  for (int i = 0; i < kw; i++) key_words[i] = tail[p2v_key_tail_word(i, cap_len)];
  return P2V_OK;
}

int p2v_circuit_self_keyed(const p2v_circuit* base, p2v_circuit** out) {
  if (!base || !out) return fail(P2V_E_ARG, "null argument");
  *out = nullptr;
  if (base->c.num_pis < base->c.key_words())
    return fail(P2V_E_CIRCUIT, "p2v_circuit_self_keyed: the circuit's public inputs are shorter than a verifier key");
  return guarded(P2V_E_ARG, [&] {
    auto v = std::make_unique<p2v_circuit>();
    v->c = base->c;
    v->c.self_keyed = true;
    *out = v.release();
  });
}

int p2v_circuit_is_self_keyed(const p2v_circuit* pc) {
  if (!pc) return fail(P2V_E_ARG, "null argument");
  return pc->c.self_keyed ? 1 : 0;
}

int p2v_pack_proofs_json(const p2v_circuit* pc, const char* const* jsons, const size_t* lens, size_t n, uint64_t* dst,
                         int32_t* codes, int threads) {
  if (!pc || (n && (!jsons || !lens || !dst || !codes))) return fail(P2V_E_ARG, "null argument");
  if (n == 0) return 0;
  const Circuit& C = pc->c;
  const int64_t W = C.L.words;
  auto dom_pack = [&](size_t i, std::string* msg) -> int32_t {
    try {
      JVal pj = parse_json(jsons[i], lens[i]);
      pack_proof(C, pj, dst + (size_t)W * i);
      return P2V_OK;
    } catch (const ShapeError& e) { if (msg) *msg = e.what(); return P2V_E_SHAPE; }
    catch (const std::exception& e) { if (msg) *msg = e.what(); return P2V_E_PARSE; }
  };
  // template from the first proof that packs
  ProofTemplate T;
  bool have_t = false;
  size_t first = 0;
  std::vector<std::string> msgs(n);
  for (; first < n && !have_t; first++) {
    try { have_t = T.build(C, jsons[first], lens[first], dst + (size_t)W * first); codes[first] = P2V_OK; }
    catch (...) { codes[first] = dom_pack(first, &msgs[first]); }
  }
  auto work = [&](size_t a, size_t b) {
    for (size_t i = a; i < b; i++) {
      if (have_t && T.pack(jsons[i], lens[i], dst + (size_t)W * i)) { codes[i] = P2V_OK; continue; }
      codes[i] = dom_pack(i, &msgs[i]);
    }
  };
  const size_t rest = n - first;
  int nt = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
  if (nt < 1) nt = 1;
  if ((size_t)nt > rest) nt = (int)(rest ? rest : 1);
  if (nt <= 1) work(first, n);
  else {
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; t++) pool.emplace_back(work, first + rest * t / nt, first + rest * (t + 1) / nt);
    for (auto& th : pool) th.join();
  }
  int nfail = 0;
  for (size_t i = 0; i < n; i++)
    if (codes[i] != P2V_OK) { if (!nfail) g_err = "proof " + std::to_string(i) + ": " + msgs[i]; nfail++; }
  return nfail;
}

int p2v_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int p2v_circuit_known_stats(const p2v_circuit* c, int device, uint64_t out[3]) {
  if (!c || !out) return fail(P2V_E_ARG, "null argument");
  out[0] = out[1] = out[2] = 0;
  const KnownTable* k = nullptr;
  {
    std::lock_guard<std::mutex> lk(c->known_mu);
    for (auto& t : c->known) if (t->device == device) k = t.get();
  }
  if (!k) return P2V_OK;
  HCK(hipSetDevice(device));
  HCK(hipDeviceSynchronize());
  HCK(hipMemcpy(out, k->stat.p, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return P2V_OK;
}

int p2v_circuit_known_key_rows(const p2v_circuit* c, int device, uint32_t key, uint64_t* valid_rows) {
  if (!c || !valid_rows) return fail(P2V_E_ARG, "null argument");
  *valid_rows = 0;
  if (key >= c->c.num_keys()) return fail(P2V_E_ARG, "key id past the circuit's key table");
  const KnownTable* k = nullptr;
  {
    std::lock_guard<std::mutex> lk(c->known_mu);
    for (auto& t : c->known) if (t->device == device) k = t.get();
  }
  if (!k || key >= (uint32_t)k->kkeys) return P2V_OK;
  HCK(hipSetDevice(device));
  HCK(hipDeviceSynchronize());
  const size_t nrows = (size_t)1 << c->c.lde_bits;
  std::vector<uint32_t> flags(nrows);
  HCK(hipMemcpy(flags.data(), (const uint32_t*)k->valid.p + key * nrows, nrows * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (uint32_t f : flags) *valid_rows += f == P2V_KNOWN_VALID;
  return P2V_OK;
}

}  // extern "C"
