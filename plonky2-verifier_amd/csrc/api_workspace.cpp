// api_workspace.cpp — the tables a workspace derives from a circuit, and the workspace
// (p2v_verifier) itself: creation, chaining, release.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "api_internal.hpp"
#include "gl.h"
#include "poseidon_constants.h"

std::mutex g_chain_mu;   // p2v_verifier_chain links (chain_prev / chain_next of every verifier)

// ---- what p2v_verifier_create derives from the circuit, one function per table ----

// the scalar and layout fields of DevCircuit, the unit orders, root powers and step shifts
void fill_scalars(const Circuit& C, DevCircuit& d) {
  d.r = C.r; d.Q = C.num_queries; d.S = (int)C.arities.size(); d.T = 4 + d.S;
  d.num_pis = C.num_pis; d.cap_len = C.cap_len; d.degree_bits = C.degree_bits; d.lde_bits = C.lde_bits; d.pow_bits = C.pow_bits;
  d.num_wires = C.num_wires; d.num_routed = C.num_routed; d.num_constants = C.num_constants; d.ngc = C.num_gate_consts;
  d.ngroups = (int)C.grp_start.size(); d.nls = C.nls; d.nlp = C.nlp; d.npp = C.npp; d.qdf = C.qdf; d.nluts = (int)C.lut_in.size();
  d.depth0 = C.depth0; d.final_len = C.final_len;
  for (int t = 0; t < 4; t++) { d.width[t] = C.oracle_width[t]; d.lwidth[t] = C.leaf_width[t]; }
  d.noop_leaves = C.noop_leaves ? 1 : 0;
  d.n_gates = C.n_gate_eval; d.n_pp_terms = (int)C.n_pp_terms_per_round; d.n_lookup_terms = (int)C.n_lookup_terms_per_round;
  d.alpha_base_gates = C.alpha_base_gates;
  d.prog_pih = -1;
  const Layout& L = C.L;
  d.pis = L.pis; d.wcap = L.wcap; d.zcap = L.zcap; d.qcap = L.qcap; d.o_const = L.o_const; d.o_sig = L.o_sig; d.o_wires = L.o_wires;
  d.o_zs = L.o_zs; d.o_pp = L.o_pp; d.o_quot = L.o_quot; d.o_lzs = L.o_lzs; d.o_zs_next = L.o_zs_next; d.o_lzs_next = L.o_lzs_next;
  d.n_this = L.n_this; d.n_next = L.n_next; d.ccaps = L.ccaps; d.final_poly = L.final_poly; d.pow = L.pow; d.q0 = L.q0; d.qstride = L.qstride;
  for (int t = 0; t < 4; t++) { d.leaf[t] = L.leaf[t]; d.path[t] = L.path[t]; }
  {   // unit orders: most expensive tree first (stable), see DevCircuit::leaf_order
    std::vector<std::pair<int64_t, int>> lc, mc;
    for (int t = 0; t < d.T; t++) {
      const int64_t len = t < 4 ? C.leaf_width[t] : (2ll << C.arities[t - 4]);
      lc.push_back({-(len + 7) / 8, t});
      mc.push_back({-(int64_t)(t < 4 ? C.depth0 : C.step_depth[t - 4]), t});
    }
    std::stable_sort(lc.begin(), lc.end()); std::stable_sort(mc.begin(), mc.end());
    for (int k = 0; k < d.T; k++) { d.leaf_order[k] = (int8_t)lc[k].second; d.merkle_order[k] = (int8_t)mc[k].second; }
  }
  for (int s = 0; s < d.S; s++) { d.step_evals[s] = L.step_evals[s]; d.step_path[s] = L.step_path[s]; d.arity[s] = C.arities[s]; d.step_depth[s] = C.step_depth[s]; }
  d.words = L.words;
  for (int i = 0; i < 4; i++) d.digest[i] = C.digest[i];
  { uint64_t x = gl::TWO_ADIC_GEN; for (int m = 0; m <= 32; m++) { d.root_pow2[m] = x; x = gl::mul(x, x); } }
  {
    uint64_t shift = gl::MULT_GEN; int logn = C.lde_bits;
    for (int s = 0; s <= d.S; s++) {
      d.step_shift[s] = shift; d.step_shift_inv[s] = gl::inv(shift);
      if (s < d.S) { d.step_logn[s] = logn; d.inv_arity[s] = gl::inv(1ULL << C.arities[s]); shift = gl::pow(shift, 1ULL << C.arities[s]); logn -= C.arities[s]; }
    }
  }
}

std::vector<uint64_t> fri_twiddles(const Circuit& C) {
  const int S = (int)C.arities.size();
  std::vector<uint64_t> tw(256 * (size_t)(S ? S : 1), 0);
  for (int s = 0; s < S; s++) {
    int ab = C.arities[s];
    uint64_t om_inv = gl::inv(gl::subgroup_gen(ab)), x = 1;
    for (int j = 0; j < (1 << ab) && j < 256; j++) { tw[256 * s + j] = x; x = gl::mul(x, om_inv); }
  }
  return tw;
}

namespace {
// PoseidonGate part 3 (vanish_poseidon.hip): the state entering the fast partial rounds is
// A'(M sb + rc) (Gate/Custom/Poseidon.hs:92-104: mdsLayer, + fastPartialFirstConstant,
// mdsInitPartial with A' = diag(1, A), A[i][j] = INITIAL_MATRIX[j][i]); as one affine map of the
// S-box outputs sb: W = A'M (12 x 12) and k = A' rc, mod p.  Returns [W row-major | k].
std::vector<uint64_t> poseidon_part3_table() {
  static const uint64_t init[121] = P2V_FAST_PARTIAL_ROUND_INITIAL_MATRIX_INIT;
  static const uint64_t rc[12] = P2V_FAST_PARTIAL_FIRST_ROUND_CONSTANT_INIT;
  static const uint32_t circ[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
  auto M = [&](int i, int j) -> uint64_t { return circ[((j - i) % 12 + 12) % 12] + (i == 0 && j == 0 ? 8 : 0); };
  auto Ap = [&](int i, int l) -> uint64_t {   // A'[i][l]
    if (i == 0 || l == 0) return (i == l) ? 1 : 0;
    return init[11 * (l - 1) + (i - 1)];
  };
  std::vector<uint64_t> t(156, 0);
  for (int i = 0; i < 12; i++) {
    for (int j = 0; j < 12; j++) {
      uint64_t acc = 0;
      for (int l = 0; l < 12; l++) acc = gl::add(acc, gl::mul(Ap(i, l), M(l, j)));
      t[12 * i + j] = acc;
    }
    uint64_t acc = 0;
    for (int l = 0; l < 12; l++) acc = gl::add(acc, gl::mul(Ap(i, l), rc[l] % gl::P));
    t[144 + i] = acc;
  }
  return t;
}

// the gate and lookup tables
struct CircuitTables {
  std::vector<int32_t> gkind, ggrp, gwoff, gs, ge; std::vector<int64_t> gpar; std::vector<uint64_t> wts;
  std::vector<uint64_t> lin, lout; std::vector<int64_t> loff, llen;
  std::vector<uint32_t> rin, rout; std::vector<int64_t> roff; std::vector<int32_t> rch, pbase{0};
  std::vector<uint64_t> gprog; std::vector<int64_t> gpoff;   // the lowered gate programs (circuit.hpp lower_gate_program)
};
CircuitTables circuit_tables(const Circuit& C) {
  CircuitTables t;
  for (int g = 0; g < C.n_gate_eval; g++) {
    const GateDesc& gd = C.gates[g];
    t.gkind.push_back(gd.kind); t.ggrp.push_back(C.sel_idx[g]);
    t.gpar.push_back(gd.p0); t.gpar.push_back(gd.p1); t.gpar.push_back(gd.p2);
    t.gwoff.push_back((int32_t)t.wts.size()); t.wts.insert(t.wts.end(), gd.weights.begin(), gd.weights.end());
    t.gpoff.push_back(gd.kind == G_PROGRAM ? (int64_t)t.gprog.size() : -1);
    if (gd.kind == G_PROGRAM) {
      std::vector<uint64_t> low;
      lower_gate_program(gd.prog, &low);
      t.gprog.insert(t.gprog.end(), low.begin(), low.end());
    }
  }
  t.gwoff.push_back((int32_t)t.wts.size());
  t.gs.assign(C.grp_start.begin(), C.grp_start.end()); t.ge.assign(C.grp_end.begin(), C.grp_end.end());
  for (size_t k = 0; k < C.lut_in.size(); k++) {
    t.loff.push_back((int64_t)t.lin.size()); t.llen.push_back((int64_t)C.lut_in[k].size());
    t.lin.insert(t.lin.end(), C.lut_in[k].begin(), C.lut_in[k].end()); t.lout.insert(t.lout.end(), C.lut_out[k].begin(), C.lut_out[k].end());
  }
  // evalFinalRE (Lookups.hs:103-109): cur = sum_i delta^(N-1-i) (inp_i + B out_i) over the table
  // padded to N = ceil(len / slots) * slots entries with its FIRST entry.  Stored reversed
  // (index t = N-1-i is the power of delta) and zero-filled to a multiple of P2V_LUT_CHUNK, so
  // the device evaluates it as sum_c delta^(16c) sum_j delta^j e'_(16c+j) (baby/giant steps).
  const int64_t slots = C.num_routed / 3;
  for (size_t k = 0; k < C.lut_in.size(); k++) {
    const auto& li = C.lut_in[k]; const auto& lo = C.lut_out[k];
    const int64_t len = (int64_t)li.size();
    const int64_t N = slots > 0 ? (len + slots - 1) / slots * slots : 0;
    bool small = len > 0;
    for (int64_t i = 0; i < len && small; i++) small = li[i] < (1u << 24) && lo[i] < (1u << 24);
    const int64_t nch = small ? (N + P2V_LUT_CHUNK - 1) / P2V_LUT_CHUNK : 0;
    t.roff.push_back((int64_t)t.rin.size()); t.rch.push_back((int32_t)nch);
    t.pbase.push_back(t.pbase.back() + (int32_t)((nch + P2V_LUT_PIECE - 1) / P2V_LUT_PIECE));
    for (int64_t j = 0; j < nch * P2V_LUT_CHUNK; j++) {
      const int64_t i = N - 1 - j, ii = i < len ? i : 0;
      t.rin.push_back(j < N ? (uint32_t)li[ii] : 0u);
      t.rout.push_back(j < N ? (uint32_t)lo[ii] : 0u);
    }
  }
  return t;
}

// transcript op program: proofChallenges (Challenge/Verifier.hs:58-103) + friChallenges (Challenge/FRI.hs:65-104);
// d holds its scalars (fill_scalars) and receives ntops
std::vector<int32_t> transcript_ops(const Circuit& C, DevCircuit& d) {
  const Layout& L = C.L;
  std::vector<int32_t> ops;
  auto op = [&](int t, int64_t a_, int64_t n_) { ops.push_back(t); ops.push_back((int32_t)a_); ops.push_back((int32_t)n_); };
  const int r = d.r, C4 = 4 * C.cap_len;
  op(TOP_ABSORB_DIGEST, 0, 4);   // stays op 0: the keyed transcripts take it before the op loop (kernels.hip)
  op(TOP_ABSORB_PIH, 0, 4);
  op(TOP_ABSORB_SOA, L.wcap, C4);
  op(TOP_SQUEEZE, CH_BETA(d), r);
  op(TOP_SQUEEZE, CH_GAMMA(d), r);
  if (C.nlp > 0) { op(TOP_COPY, CH_DELTA(d), 2 * r); op(TOP_SQUEEZE, CH_DELTA(d) + 2 * r, 2 * r); }
  else op(TOP_ZERO, CH_DELTA(d), 4 * r);
  op(TOP_ABSORB_SOA, L.zcap, C4);
  op(TOP_SQUEEZE, CH_ALPHA(d), r);
  op(TOP_ABSORB_SOA, L.qcap, C4);
  op(TOP_SQUEEZE, CH_ZETA(d), 2);
  op(TOP_ABSORB_SOA, L.o_const, 2 * (L.n_this + L.n_next));
  op(TOP_SQUEEZE, CH_FRI_ALPHA(d), 2);
  for (int s = 0; s < d.S; s++) { op(TOP_ABSORB_SOA, L.ccaps + (int64_t)s * C4, C4); op(TOP_SQUEEZE, CH_FRI_BETA(d) + 2 * s, 2); }
  op(TOP_ABSORB_SOA, L.final_poly, 2 * C.final_len);
  op(TOP_ABSORB_SOA, L.pow, 1);
  op(TOP_SQUEEZE, CH_POW(d), 1);
  op(TOP_SQUEEZE_IDX, CH_QIDX(d), d.Q);
  d.ntops = (int)(ops.size() / 3);
  return ops;
}

// vanishing work items, heaviest first so their waves are dispatched first; d receives the
// class bounds vcls and n_vitems
std::vector<int32_t> vanish_items(const Circuit& C, DevCircuit& d) {
  std::vector<int32_t> vit;
  auto item = [&](int t, int a_, int b_, int64_t first) { vit.push_back(t); vit.push_back(a_); vit.push_back(b_); vit.push_back((int32_t)first); };
  auto kind = [&](int g) { return C.gates[g].kind; };
  d.vcls[0] = 0;
  for (int g = 0; g < C.n_gate_eval; g++)
    if (kind(g) == G_POSEIDON) for (int k = 0; k < P2V_POSEIDON_PARTS; k++) item(VI_GATE, g, k, p2v_poseidon_part_first_term(k));
  d.vcls[1] = (int)(vit.size() / 4);
  for (int g = 0; g < C.n_gate_eval; g++)   // one item per interpolation chunk (dev.h p2v_coset_parts)
    if (kind(g) == G_COSET) {
      const GateDesc& gd = C.gates[g];
      const int64_t parts = p2v_coset_parts((int)gd.p0, gd.p1, (int32_t)gd.weights.size());
      for (int64_t k = 0; k < parts; k++) item(VI_GATE, g, (int)k, p2v_coset_part_first_term(k));
    }
  d.vcls[2] = (int)(vit.size() / 4);
  for (int g = 0; g < C.n_gate_eval; g++) if (kind(g) != G_POSEIDON && kind(g) != G_COSET && kind(g) != G_PROGRAM) item(VI_GATE, g, 0, 0);
  for (int j = 0; j < d.r; j++) item(VI_PP, j, 0, d.r + (int64_t)j * d.n_pp_terms);
  item(VI_ZS1, 0, 0, 0);
  d.vcls[3] = (int)(vit.size() / 4);
  if (d.nluts > 0)
    for (int j = 0; j < d.r; j++) item(VI_LOOKUP, j, 0, d.r + (int64_t)d.r * d.n_pp_terms + (int64_t)j * d.n_lookup_terms);
  d.vcls[4] = (int)(vit.size() / 4);
  {   // the program gates (vanish_prog.hip), one item each, the longest program first
    std::vector<int> pg;
    for (int g = 0; g < C.n_gate_eval; g++) if (kind(g) == G_PROGRAM) pg.push_back(g);
    std::stable_sort(pg.begin(), pg.end(), [&](int x, int y) { return C.gates[x].prog.size() > C.gates[y].prog.size(); });
    for (int g : pg) item(VI_GATE, g, 0, 0);
  }
  d.n_vitems = (int)(vit.size() / 4);
  d.vcls[5] = d.n_vitems;
  return vit;
}
}  // namespace

// the staging buffer for batches given in host memory (run from host, JSON / binary ingest)
hipError_t input_buf(p2v_verifier* v) {
  return v->in.p ? hipSuccess : v->in.alloc(v->in_bytes);
}

extern "C" {

void p2v_verifier_free(p2v_verifier* v) {
  if (!v) return;
  {   // unlink: no workspace keeps a pointer to this one, and its own link goes away
    std::lock_guard<std::mutex> lk(g_chain_mu);
    for (p2v_verifier* n : v->chain_next) n->chain_prev = nullptr;
    if (v->chain_prev) {
      auto& nx = v->chain_prev->chain_next;
      nx.erase(std::remove(nx.begin(), nx.end(), v), nx.end());
    }
  }
  (void)hipSetDevice(v->device);
  delete v;
}

int p2v_verifier_chain(p2v_verifier* v, p2v_verifier* prev) {
  if (!v) return fail(P2V_E_ARG, "null verifier");
  if (prev && prev->device != v->device) return fail(P2V_E_ARG, "p2v_verifier_chain: verifiers on different devices");
  std::lock_guard<std::mutex> lk(g_chain_mu);
  if (v->chain_prev) {
    auto& nx = v->chain_prev->chain_next;
    nx.erase(std::remove(nx.begin(), nx.end(), v), nx.end());
  }
  v->chain_prev = prev;
  if (prev) prev->chain_next.push_back(v);
  return P2V_OK;
}

int p2v_verifier_create(const p2v_circuit* pc, int device, size_t max_batch, p2v_verifier** out) {
  if (!pc || !out || max_batch == 0) return fail(P2V_E_ARG, "null argument / zero batch");
  // not a silent fall to auto: a measurement would report the default under the pair form's name
  if (const char* tm = getenv("P2V_TRANSCRIPT"); tm && !strcmp(tm, "pair"))
    return fail(P2V_E_ARG, "P2V_TRANSCRIPT=pair: the pair transcript form was retired (DESIGN.md §5.7)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(P2V_E_NODEVICE, "no HIP device available: libp2v verifies on MI355X only (no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(P2V_E_ARG, "bad device index");
  HCK(hipSetDevice(device));
  const Circuit& C = pc->c;
  VerifierPtr v(new p2v_verifier());   // every early return below frees what was made so far
  v->circ = pc; v->device = device; v->max_batch = max_batch;
  v->Bmax = (max_batch + 63) / 64 * 64;
  if (const char* ss = getenv("P2V_SINGLE_STREAM")) v->single_stream = ss[0] == '1';
  if (const char* ds = getenv("P2V_DEBUG_SYNC")) v->debug_sync = ds[0] == '1';
  if (const char* lm = getenv("P2V_LANE_MIN")) v->lane_min_batch = atoi(lm) > 0 ? atoi(lm) : v->lane_min_batch;
  if (const char* qm = getenv("P2V_QUAD_MIN")) v->quad_min_batch = atoi(qm) > 0 ? atoi(qm) : v->quad_min_batch;
  if (const char* mc = getenv("P2V_MERKLE_CSE")) v->merkle_cse = mc[0] != '0';
  if (const char* kl = getenv("P2V_KNOWN_LEAVES")) v->known_mode = kl[0] == '0' ? 0 : kl[0] == '2' ? 2 : 1;
  if (const char* lx = getenv("P2V_LAT_MAX")) v->lat_max_batch = atoi(lx) >= 0 ? atoi(lx) : v->lat_max_batch;
  if (const char* tm = getenv("P2V_TRANSCRIPT")) v->transcript_mode = !strcmp(tm, "row") ? 1 : !strcmp(tm, "quad") ? 2 : !strcmp(tm, "lane") ? 3 : 0;
  DevCircuit& d = v->dc;
  memset(&d, 0, sizeof d);
  fill_scalars(C, d);
  const CircuitTables t = circuit_tables(C);
  d.n_lut_pieces = t.pbase.back();
#define ACK(x) HCK_AS("device allocation", x)
  {   // the key table [nkeys][4 cap_len + 4]; key 0 leads it, so its cap is the unkeyed runs' cs_cap
    std::vector<uint64_t> keys(C.cs_cap);
    keys.insert(keys.end(), C.digest, C.digest + 4);
    keys.insert(keys.end(), C.extra_keys.begin(), C.extra_keys.end());
    keys.insert(keys.end(), 8, 0);   // padding the keyed transcripts may read and drop (dev.h)
    ACK(upload(v->t_cs, keys, d.keys));
    d.cs_cap = d.keys;
    d.nkeys = (int32_t)C.num_keys();
    const std::vector<uint32_t>& tab = pc->key_lookup();   // the lookup over them (keys.hip k_key_resolve)
    ACK(upload(v->t_ktab, tab, d.key_tab));
    d.key_tab_mask = (uint32_t)tab.size() - 1;
  }
  ACK(v->kid.alloc(v->Bmax * sizeof(uint32_t)));
  for (DevBuf& b : v->kres) ACK(b.alloc(v->Bmax * sizeof(uint32_t)));
  ACK(upload(v->t_kis, C.k_is, d.k_is));
  ACK(upload(v->t_gkind, t.gkind, d.gate_kind)); ACK(upload(v->t_gpar, t.gpar, d.gate_par)); ACK(upload(v->t_ggrp, t.ggrp, d.gate_grp));
  ACK(upload(v->t_gwoff, t.gwoff, d.gate_woff)); ACK(upload(v->t_w, t.wts, d.weights)); ACK(upload(v->t_gs, t.gs, d.grp_start)); ACK(upload(v->t_ge, t.ge, d.grp_end));
  ACK(upload(v->t_lin, t.lin, d.lut_in)); ACK(upload(v->t_lout, t.lout, d.lut_out)); ACK(upload(v->t_loff, t.loff, d.lut_off)); ACK(upload(v->t_llen, t.llen, d.lut_len));
  ACK(upload(v->t_tw, fri_twiddles(C), d.twiddles)); ACK(upload(v->t_ops, transcript_ops(C, d), d.tops)); ACK(upload(v->t_vit, vanish_items(C, d), d.vitems));
  ACK(upload(v->t_rin, t.rin, d.lut_rin)); ACK(upload(v->t_rout, t.rout, d.lut_rout)); ACK(upload(v->t_roff, t.roff, d.lut_roff));
  ACK(upload(v->t_rch, t.rch, d.lut_rchunks)); ACK(upload(v->t_pbase, t.pbase, d.lut_pbase));
  ACK(upload(v->t_pw, poseidon_part3_table(), d.pos_w));
  ACK(upload(v->t_gprog, t.gprog, d.gprog)); ACK(upload(v->t_gpoff, t.gpoff, d.gate_poff));
  const size_t B = v->Bmax;
  const size_t chw = (size_t)(4 + 7 * d.r + 4 + 2 * d.S + 1 + d.Q + 4);
  v->in_bytes = (size_t)C.L.words * v->Bmax * 8;   // whole 64-proof tiles (P2V_FLAG_INPUT_TILED); allocated on first use
  ACK(v->chal.alloc(chw * B * 8));
  ACK(v->chal2.alloc(chw * B * 8));
  ACK(v->leafdig.alloc((size_t)d.Q * d.T * 4 * B * 8));
  ACK(v->mk.alloc((size_t)d.Q * d.T * B));
  ACK(v->fbits.alloc((size_t)d.Q * B * 4));
  ACK(v->qvals.alloc((size_t)d.Q * 6 * B * 8));
  ACK(v->van.alloc((size_t)(1 + 4 * d.r) * B * 8));
  ACK(v->vparts.alloc((size_t)d.n_vitems * 2 * d.r * B * 8));
  ACK(v->lutre.alloc((size_t)d.r * (d.nluts ? d.nluts : 1) * B * 8));
  ACK(v->lutpart.alloc((size_t)d.r * (d.n_lut_pieces ? d.n_lut_pieces : 1) * B * 8));
  ACK(v->res.alloc(B));
  ACK(v->h_res.grow(B));
  ACK(v->trace.alloc((size_t)C.trace_words * B * 8));
  // shared-node Merkle paths: on unless P2V_MERKLE_CSE=0 or the shape exceeds the plan's fields
  d.mcse = v->merkle_cse && d.Q <= P2V_CSE_MAX_Q && d.depth0 <= P2V_CSE_MAX_DEPTH && B <= (size_t)P2V_CSE_MAX_B && d.T < 32;
  if (d.mcse) {
    const size_t ncls = 1 + (size_t)d.S, nb = 1 + (size_t)d.depth0;
    d.mcap = (int64_t)d.T * d.Q * (int64_t)B;
    ACK(v->m_plan.alloc(ncls * d.Q * B * 4));
    ACK(v->m_fol.alloc(ncls * d.Q * B * 8));
    ACK(v->m_chain.alloc(nb * (size_t)d.mcap * 4));
    const size_t cnt_bytes = (nb + 1) * 64;   // bucket counters and the fix-list length, 64 B apart
    ACK(v->m_count.alloc(cnt_bytes));
    ACK(hipMemset(v->m_count.p, 0, cnt_bytes));   // then zeroed by each run's k_merkle_resolve
    ACK(v->m_fix.alloc((size_t)d.mcap * 4));
    ACK(v->m_badq.alloc((size_t)d.T * d.Q * B));
    ACK(v->m_node.alloc((size_t)d.T * d.Q * 4 * B * 8));
    d.mplan = (uint32_t*)v->m_plan.p; d.mfol = (uint64_t*)v->m_fol.p; d.mchain = (uint32_t*)v->m_chain.p;
    d.mcount = (int32_t*)v->m_count.p; d.mfixn = d.mcount + nb * 16; d.mfix = (uint32_t*)v->m_fix.p;
    d.mbadq = (uint8_t*)v->m_badq.p; d.mnode = (uint64_t*)v->m_node.p;
  }
  // known openings of tree 0: with the shared-node paths only, and when the table fits its budget
  // (P2V_KNOWN_MAX_MB, default 128: a policy value, one key's rows).  A leaf that is its own digest
  // is not hashed.  A handle with a key table gets every key's rows when they fit
  // P2V_KNOWN_KEYED_MAX_MB together (default 1024, a policy value too), else key 0's alone: a table
  // of some keys would send every opening of the others through the miss list, which costs more
  // than no table.  Decided by the handle's first workspace on the device.
  d.nleaf = d.T;
  d.kwords = d.lwidth[0] + 4 * d.depth0;
  if (v->known_mode && d.mcse && !(d.noop_leaves && d.lwidth[0] <= 4)) {
    size_t budget_mb = 128, keyed_mb = 1024;
    if (const char* mb = getenv("P2V_KNOWN_MAX_MB")) budget_mb = atoll(mb) > 0 ? (size_t)atoll(mb) : 0;
    if (const char* mb = getenv("P2V_KNOWN_KEYED_MAX_MB")) keyed_mb = atoll(mb) > 0 ? (size_t)atoll(mb) : 0;
    const size_t bytes = ((size_t)1 << d.lde_bits) * ((size_t)d.kwords * 8 + 4);   // one key's
    if (bytes <= budget_mb << 20) {
      std::lock_guard<std::mutex> lk(pc->known_mu);
      for (auto& k : pc->known) if (k->device == device) v->known = k.get();
      if (!v->known) {
        auto k = std::make_unique<KnownTable>();
        k->device = device;
        k->kkeys = d.nkeys > 1 && bytes * (size_t)d.nkeys <= keyed_mb << 20 ? d.nkeys : 1;
        const size_t nrows = (size_t)k->kkeys << d.lde_bits;
        ACK(k->rows.alloc(nrows * d.kwords * 8)); ACK(k->valid.alloc(nrows * 4)); ACK(k->stat.alloc(64));
        ACK(hipMemset(k->rows.p, 0, nrows * d.kwords * 8)); ACK(hipMemset(k->valid.p, 0, nrows * 4)); ACK(hipMemset(k->stat.p, 0, 64));
        ACK(hipStreamSynchronize(nullptr));   // the first run's stream does not wait for the null stream
        v->known = k.get();
        pc->known.push_back(std::move(k));
      }
    }
    if (v->known) {
      ACK(v->k_miss.alloc((size_t)d.Q * B * 4));
      ACK(v->k_missn.alloc(64));
      ACK(hipMemset(v->k_missn.p, 0, 64));   // then zeroed by each run's k_status
      ACK(hipStreamSynchronize(nullptr));
      d.krows = (uint64_t*)v->known->rows.p; d.kvalid = (uint32_t*)v->known->valid.p; d.kstat = (unsigned long long*)v->known->stat.p;
      d.kmiss = (uint32_t*)v->k_miss.p; d.kmissn = (int32_t*)v->k_missn.p;
    }
  }
  for (Event& x : v->ev) ACK(x.create_timed());
  v->timed = true;
  ACK(v->dep_p1.create()); ACK(v->dep_side.create()); ACK(v->p1_done.create());
  // the side stream carries few, long-latency waves (vanishing items, FRI queries), at the default
  // priority (a high-priority queue changed nothing: DESIGN.md "Retired run-time switches")
  ACK(v->side.create());
  // (the latency-mode and lookahead streams are created on first use: every stream a process
  // creates may take one of its few hardware queues, GPU_MAX_HW_QUEUES = 4, and two workspaces'
  // main and side streams must not share one)
  ACK(v->dep_v3.create());
  for (int k = 0; k < 2; k++) { ACK(v->tr_done[k].create()); ACK(v->chal_free[k].create()); }
  ACK(v->dep_fri.create());
#undef ACK
  d.chal = (uint64_t*)v->chal.p; d.leafdig = (uint64_t*)v->leafdig.p; d.mk_ok = (uint8_t*)v->mk.p;
  d.fri_bits = (uint32_t*)v->fbits.p; d.qvals = (uint64_t*)v->qvals.p; d.van = (uint64_t*)v->van.p; d.vparts = (uint64_t*)v->vparts.p; d.lutre = (uint64_t*)v->lutre.p; d.lutpart = (uint64_t*)v->lutpart.p;
  *out = v.release();
  return P2V_OK;
}

}  // extern "C"
