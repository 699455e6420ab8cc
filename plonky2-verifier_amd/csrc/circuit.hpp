// circuit.hpp — host side of the drop-in boundary: decode VerifierCircuitData
// (reference src/Types.hs:47-240, Gate strings src/Gate/Parser.hs:27-242), validate it
// once (circuit-level `error`s of the reference surface here), derive the fixed packed
// proof layout, and pack ProofWithPublicInputs JSON (Types.hs:245-279) into it.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "json.hpp"

namespace p2v {

enum GateKind : int32_t {   // Gate/Base.hs:27-45
  G_ARITH = 0, G_ARITH_EXT, G_BASESUM, G_COSET, G_CONST, G_EXP, G_LOOKUP, G_LOOKUPTABLE,
  G_MULEXT, G_NOOP, G_PI, G_POSEIDON, G_POSEIDON_MDS, G_RANDACC, G_REDUCING, G_REDUCING_EXT, G_UNKNOWN,
  G_PROGRAM   // an UnknownGate whose constraints are a caller's program (include/p2v.h "gate programs")
};

// A gate program (include/p2v.h, version-1 encoding), decoded and checked for form: SSA,
// straight-line, every operand an earlier value.  Instruction i is op[i] with operands a[i], b[i]
// (value numbers; for the leaf ops a[i] is the index / the literal reduced mod p).
enum GateOp : uint8_t { GP_WIRE = 0, GP_CONST, GP_PIHASH, GP_LIT, GP_ADD, GP_SUB, GP_MUL, GP_IMG, GP_COMMIT, GP_NUM_OPS };
struct GateProgram {
  std::vector<uint8_t> op;
  std::vector<uint64_t> a, b;
  std::vector<int32_t> def;        // value number -> the instruction that defines it
  int num_commits = 0;
  int64_t max_wire = -1, max_const = -1, max_pih = -1;
  size_t size() const { return op.size(); }
  bool empty() const { return op.empty(); }
};
// throws ParseError (bad magic, truncation, trailing words, unknown opcode, operand not an earlier value)
GateProgram decode_gate_program(const uint64_t* words, size_t n);
// the number of words of the encoding that starts at `words` (walks at most max_words; ParseError)
size_t gate_program_extent(const uint64_t* words, size_t max_words);
// F^2 rows in, constraints (re, im) out; the caller has checked the indices against the rows
void eval_gate_program(const GateProgram& g, const uint64_t* wires, const uint64_t* consts, const uint64_t* pih, uint64_t* out);
// What the device interpreter reads (vanish_prog.hip): [count, then 3 words per instruction
// {op | slot << 8 | kind_a << 16 | kind_b << 24, a, b}].  The leaf values are operand kinds of
// their own; every other value gets an LDS slot by liveness (alive from its instruction to its
// last use): straight-line SSA lifetimes are intervals, so taking the lowest free slot in
// program order uses exactly as many slots as values are alive at once.  Returns that number.
enum { GPK_SLOT = 0, GPK_WIRE, GPK_CONST, GPK_PIHASH, GPK_LIT };
int lower_gate_program(const GateProgram& g, std::vector<uint64_t>* out);
struct NamedGateProgram { std::string gate; GateProgram prog; };

struct GateDesc {
  int32_t kind = G_UNKNOWN;
  int64_t p0 = 0, p1 = 0, p2 = 0;
  std::vector<uint64_t> weights;   // CosetInterpolationGate barycentric weights
  std::string text;
  std::string name;                // UnknownGate: the gate string as given (what a gate program is matched by)
  GateProgram prog;                // G_PROGRAM
};

// Fixed per-circuit packed proof layout (u64 words).  Order:
//   pis | wires_cap | zs_pp_cap | quotient_cap | openings(batch_this ++ batch_next)
//   | commit caps | final poly | pow witness | Q x [4 leaves | 4 paths | steps x (evals | path)]
struct Layout {
  int64_t pis = 0, wcap = 0, zcap = 0, qcap = 0;
  int64_t open = 0;                         // start of the F^2 openings (2 words each)
  int64_t o_const = 0, o_sig = 0, o_wires = 0, o_zs = 0, o_pp = 0, o_quot = 0, o_lzs = 0;   // batch_this
  int64_t o_zs_next = 0, o_lzs_next = 0;    // batch_next
  int64_t n_this = 0, n_next = 0;           // F^2 counts
  int64_t ccaps = 0, final_poly = 0, pow = 0;
  int64_t q0 = 0, qstride = 0;
  int64_t leaf[4] = {0, 0, 0, 0}, path[4] = {0, 0, 0, 0};   // offsets inside one query
  std::vector<int64_t> step_evals, step_path;                 // offsets inside one query
  int64_t words = 0;
};

struct Circuit {
  // CircuitConfig (Types.hs:73-84)
  int num_wires = 0, num_routed = 0, num_gate_consts = 0, r = 0, max_qdf = 0;
  // FriConfig / FriParams (Types.hs:116-174)
  int rate_bits = 0, cap_height = 0, pow_bits = 0, num_queries = 0, degree_bits = 0, lde_bits = 0;
  std::vector<int> arities;                 // expandReductionStrategy, Plonk/FRI.hs:337-354
  bool hiding = false;                      // fri_params.hiding (Types.hs:153)
  std::vector<int> params_arities;          // fri_params.reduction_arity_bits (Types.hs:155)
  uint32_t ext = 0;                         // P2V_EXT_* (include/p2v.h): opt-in plonky2 conventions
  // CommonCircuitData (Types.hs:47-61)
  std::vector<GateDesc> gates;
  std::vector<int> sel_idx;
  std::vector<int> grp_start, grp_end;
  int qdf = 0, num_gate_constraints = 0, num_constants = 0, num_pis = 0;
  std::vector<uint64_t> k_is;
  int npp = 0, nlp = 0, nls = 0;
  std::vector<std::vector<uint64_t>> lut_in, lut_out;
  // VerifierOnlyCircuitData (Types.hs:236-240)
  std::vector<uint64_t> cs_cap;             // 4 words per digest
  uint64_t digest[4] = {0, 0, 0, 0};
  // further verifier keys of the same common data (p2v_circuit_with_keys): key k >= 1 at
  // extra_keys[(k - 1) * key_words()], in the key encoding [cap digests | circuit_digest]; key 0
  // is cs_cap / digest above
  std::vector<uint64_t> extra_keys;
  int key_words() const { return 4 * cap_len + 4; }
  size_t num_keys() const { return 1 + extra_keys.size() / (size_t)key_words(); }
  // word i of key k in the key encoding
  uint64_t key_word(size_t k, int i) const {
    if (k) return extra_keys[(k - 1) * (size_t)key_words() + i];
    return i < 4 * cap_len ? cs_cap[i] : digest[i - 4 * cap_len];
  }
  // self-keyed handle (p2v_circuit_self_keyed): runs without ids resolve each proof's key from the
  // tail of its public inputs (include/p2v.h "self-keyed circuits"); kept by the derived handles
  bool self_keyed = false;
  int final_len_override = -1;              // shape variant (circuit_shape_variant): final_poly length
  // derived
  int cap_len = 0, final_len = 0;
  int oracle_width[4] = {0, 0, 0, 0};       // data columns per initial oracle (Plonk/FRI.hs:56-65)
  int leaf_width[4] = {0, 0, 0, 0};         // packed leaf words: + SALT_SIZE salts under P2V_EXT_HIDING
  bool noop_leaves = false;                 // P2V_EXT_HASH_OR_NOOP: leaves of <= 4 words are their digest
  int depth0 = 0;                           // initial Merkle path length
  std::vector<int> step_depth;
  int n_gate_eval = 0;                      // gates actually evaluated: min(#selector_indices, #gates)
  int64_t alpha_base_gates = 0;             // #terms before the gate terms (Vanishing.hs:67-72)
  int64_t n_pp_terms_per_round = 0, n_lookup_terms_per_round = 0;
  Layout L;
  int64_t trace_words = 0;
};

// progs: gate programs by gate string; an UnknownGate with one becomes a G_PROGRAM gate
Circuit parse_circuit(const JVal& common, const JVal& vkey, uint32_t ext = 0,
                      const std::vector<NamedGateProgram>& progs = {});   // throws ParseError / CircuitError
// the same from the word-encoded Types.hs values (include/p2v.h, "Word-encoded values")
Circuit parse_circuit_words(const uint64_t* words, size_t n, uint32_t ext = 0,
                            const std::vector<NamedGateProgram>& progs = {});   // throws ParseError / CircuitError
void pack_proof_words(const Circuit& c, const uint64_t* words, size_t n, uint64_t* dst);   // ParseError / ShapeError
// a VerifierOnlyCircuitData JSON in the key encoding (c.key_words() words: the cap digests, then
// circuit_digest); ParseError, or CircuitError when the cap is not of the circuit's length
void vkey_words(const Circuit& c, const JVal& vkey, uint64_t* dst);
// plonky2's binary ProofWithPublicInputs serialization (circuit.cpp); ParseError / ShapeError
void pack_proof_bytes(const Circuit& c, const uint8_t* bytes, size_t n, uint64_t* dst);
// The same format as a fixed map for the device packer (json_pack.hip k_bytes_pack): runs of u64
// words (source byte offset, packed word, count) in file order, the sibling-count bytes and their
// expected values, and the byte length before the public inputs.
struct BytesMap {
  std::vector<int64_t> run_src, run_dst, run_len;
  std::vector<int64_t> chk_off;
  std::vector<uint8_t> chk_val;
  int64_t fixed = 0;
};
BytesMap bytes_map(const Circuit& c);
// throws ParseError / ShapeError; rec (optional, [words]) receives each packed word's number ordinal
void pack_proof(const Circuit& c, const JVal& proof, uint64_t* dst, int32_t* rec = nullptr);

// template-guided fast path of pack_proof (circuit.cpp); pack() == false: use pack_proof
struct ProofTemplate {
  std::string text;
  std::vector<std::pair<size_t, size_t>> spans;   // number tokens of the template text
  std::vector<int64_t> dst_of;                    // number ordinal -> packed word (-1: unused)
  bool build(const Circuit& c, const char* s, size_t n, uint64_t* dst);   // throws like pack_proof
  bool pack(const char* s, size_t n, uint64_t* dst) const;
  // the device form of the template (json_pack.hip): the skeleton (every byte outside the
  // number tokens, concatenated) and the packed word of each token.  False when a byte-level
  // scan for runs of [0-9-] would not find exactly the template's number tokens (e.g. digits
  // inside a key): the device path is then unusable for this template.
  bool device_form(std::vector<uint8_t>& skel, std::vector<int32_t>& tok_dst) const;
};
GateDesc parse_gate_string(const std::string& s);              // Gate/Parser.hs:107-130

// Shape variants.  The reference reads public_inputs and final_poly.coeffs at whatever length a
// proof carries (Hash/Sponge.hs:26-31, Plonk/FRI.hs:325-327, Challenge/FRI.hs:83); the packed
// layout is fixed per circuit, so a proof with other lengths is verified against a variant of the
// circuit whose layout has them.  Throws CircuitError past this build's limits.
Circuit circuit_shape_variant(const Circuit& base, int num_pis, int final_len);
// the two lengths as a proof carries them (JSON / word-encoded); ParseError if they cannot be read
void proof_shape_json(const JVal& proof, int& num_pis, int& final_len);
void proof_shape_words(const uint64_t* words, size_t n, int& num_pis, int& final_len);

}  // namespace p2v
