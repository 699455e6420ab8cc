// api.cpp — the C-ABI of libp2v (include/p2v.h): the drop-in boundary for
// verifyProof :: VerifierCircuitData -> ProofWithPublicInputs -> Bool
// (reference src/Plonk/Verifier.hs:56-65), batched, on MI355X.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>
#include "../../include/p2v.h"
#include "circuit.hpp"
#include "dev.h"
#include "gl.h"
#include "poseidon_constants.h"

extern "C" __global__ void k_phase1(DevCircuit, int, int);
extern "C" __global__ void k_phase1_lane(DevCircuit, int, int);
extern "C" __global__ void k_transcript(DevCircuit, int);
extern "C" __global__ void k_transcript_lane(DevCircuit, int);
extern "C" __global__ void k_phase1_keyed(DevCircuit, int, int);
extern "C" __global__ void k_phase1_lane_keyed(DevCircuit, int, int);
extern "C" __global__ void k_transcript_keyed(DevCircuit, int);
extern "C" __global__ void k_transcript_lane_keyed(DevCircuit, int);
extern "C" __global__ void k_leaf(DevCircuit);
extern "C" __global__ void k_merkle(DevCircuit);
extern "C" __global__ void k_merkle_row(DevCircuit);
extern "C" __global__ void k_merkle_plan(DevCircuit);
extern "C" __global__ void k_merkle_cse(DevCircuit);
extern "C" __global__ void k_merkle_fix(DevCircuit);
extern "C" __global__ void k_merkle_resolve(DevCircuit);
extern "C" __global__ void k_merkle_known(DevCircuit);
extern "C" __global__ void k_merkle_known_miss(DevCircuit);
extern "C" __global__ void k_fri(DevCircuit);
extern "C" __global__ void k_vanish_r2(DevCircuit);
extern "C" __global__ void k_vanish_rn(DevCircuit);
extern "C" __global__ void k_vanish_poseidon_r2(DevCircuit);
extern "C" __global__ void k_vanish_poseidon_rn(DevCircuit);
extern "C" __global__ void k_vanish_coset_r2(DevCircuit);
extern "C" __global__ void k_vanish_coset_rn(DevCircuit);
extern "C" __global__ void k_vanish_lookup_r2(DevCircuit);
extern "C" __global__ void k_vanish_lookup_rn(DevCircuit);
extern "C" __global__ void k_vanish_prog_r2(DevCircuit);
extern "C" __global__ void k_vanish_prog_rn(DevCircuit);
extern "C" __global__ void k_selftest_prog(DevCircuit, uint64_t*, int);
extern "C" __global__ void k_lut(DevCircuit);
extern "C" __global__ void k_vanish_final(DevCircuit);
extern "C" __global__ void k_status(DevCircuit, int8_t*, uint64_t*, int64_t);
extern "C" __global__ void k_selftest(int, const uint64_t*, const uint64_t*, uint64_t*, int64_t);
extern "C" __global__ void k_selftest_forms(int, const uint64_t*, uint64_t*, int64_t);
extern "C" __global__ void k_selftest_field(int, DevCircuit, const uint64_t*, uint64_t*);
extern "C" __global__ void k_count_mismatches(const int8_t*, const int8_t*, int64_t, unsigned long long*);
extern "C" __global__ void k_clock_probe(unsigned long long*);
extern "C" __global__ void k_json_pack(const uint8_t*, const uint64_t*, int, const uint8_t*, int64_t, const int32_t*, int64_t, uint64_t*, int64_t, int8_t*);
extern "C" __global__ void k_bytes_pack(const uint8_t*, const uint64_t*, int, const int64_t*, const int64_t*, const int64_t*, int,
                                        const int64_t*, const uint8_t*, int, int64_t, int64_t, int64_t, uint64_t*, int64_t, int8_t*);

using namespace p2v;

namespace {
thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

// fn() with the host readers' exceptions as return codes; any other std::exception is `other`
template <class F>
int guarded(int other, F fn) {
  try { fn(); return P2V_OK; }
  catch (const ShapeError& e) { return fail(P2V_E_SHAPE, e.what()); }
  catch (const ParseError& e) { return fail(P2V_E_PARSE, e.what()); }
  catch (const CircuitError& e) { return fail(P2V_E_CIRCUIT, e.what()); }
  catch (const std::exception& e) { return fail(other, e.what()); }
}

// per-kernel timing slots; k_fri and k_vanish run on the side stream, concurrently with k_merkle
// (k_leaf + k_transcript: the two halves of k_phase1 as the lookahead path launches them).
// Slot 0 is the retired transposing build's; it keeps its name and place (callers index by this
// list) and is never recorded.
const char* kKernelNames = "k_transpose,k_phase1,k_merkle,k_fri,k_vanish,k_status,k_vanish_final,k_lut,k_leaf,k_transcript,k_merkle_known";
enum Slot { SLOT_TRANSPOSE, SLOT_PHASE1, SLOT_MERKLE, SLOT_FRI, SLOT_VANISH, SLOT_STATUS, SLOT_VANISH_FINAL, SLOT_LUT, SLOT_LEAF,
            SLOT_TRANSCRIPT, SLOT_KNOWN, kNumKernels };   // the order of kKernelNames

// Device resources are owned by type: each owner is move-only and releases what it holds in its
// destructor, on the device that is current then (p2v_verifier_free and pipe_free set it).
// Device or pinned host memory with its size:
template <class T, hipError_t (*Alloc)(void**, size_t), hipError_t (*Free)(void*)>
struct Mem {
  T* p = nullptr;
  size_t bytes = 0;
  Mem() = default;
  Mem(Mem&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  Mem& operator=(Mem&& o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
  ~Mem() { free_(); }
  hipError_t alloc(size_t n) {
    free_();
    const hipError_t e = Alloc((void**)&p, n ? n : 16);
    if (e == hipSuccess) bytes = n; else p = nullptr;
    return e;
  }
  hipError_t grow(size_t n) { return n <= bytes ? hipSuccess : alloc(n); }   // never shrinks
  void free_() { if (p) (void)Free(p); p = nullptr; bytes = 0; }
};
hipError_t pinned_alloc(void** p, size_t n) { return hipHostMalloc(p, n); }
using DevBuf = Mem<void, hipMalloc, hipFree>;
using PinnedBuf = Mem<int8_t, pinned_alloc, hipHostFree>;

// a stream or an event: empty until created, usable wherever the plain handle is
template <class H, hipError_t (*Destroy)(H)>
struct Owned {
  H h = nullptr;
  Owned() = default;
  Owned(Owned&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
  Owned& operator=(Owned&& o) noexcept { std::swap(h, o.h); return *this; }
  ~Owned() { if (h) (void)Destroy(h); }
  operator H() const { return h; }
};
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
  hipError_t create() { return hipStreamCreateWithFlags(&h, hipStreamNonBlocking); }
};
struct Event : Owned<hipEvent_t, hipEventDestroy> {
  hipError_t create() { return hipEventCreateWithFlags(&h, hipEventDisableTiming); }
  hipError_t create_timed() { return hipEventCreate(&h); }
};
}  // namespace

struct HostPipe;
// The circuit's known openings of tree 0 on one device (merkle.hip k_merkle_known): the rows, their
// flags and the three counters.  Shared by every workspace of the circuit on that device; it warms
// across runs and never affects a result, only time.  kkeys: the keys it covers, one block of
// 2^lde_bits rows each (dev.h krows): every key of the handle's table, or key 0 alone (a one-key
// handle, or all keys' rows over P2V_KNOWN_KEYED_MAX_MB), never a subset.  Keyed runs use it only
// when it covers every key.
struct KnownTable {
  int device = -1;
  int kkeys = 1;
  DevBuf rows, valid, stat;
};
// The circuit handle also owns the verifiers the one-shot entry points (p2v_verify_batch,
// p2v_verify_batch_devices) run on, kept across calls (a drop-in verifyProof
// call must not re-create workspaces, streams and events).  Read-only for the circuit itself.
struct p2v_circuit {
  Circuit c;
  mutable std::mutex pool_mu;
  mutable std::vector<HostPipe*> pool;   // idle and busy pipes of every device
  mutable std::mutex known_mu;
  mutable std::vector<std::unique_ptr<KnownTable>> known;   // one per device, made by the first workspace that wants it
  ~p2v_circuit();
};

namespace {
// a table on the device, and the DevCircuit field that points to it
template <class T>
hipError_t upload(DevBuf& b, const std::vector<T>& h, const T*& field) {
  hipError_t e = b.alloc(h.size() * sizeof(T));
  if (e != hipSuccess) return e;
  field = (const T*)b.p;
  if (!h.empty()) e = hipMemcpy(b.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
  return e;
}

std::mutex g_chain_mu;   // p2v_verifier_chain links (chain_prev / chain_next of every verifier)

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

}  // namespace


struct p2v_verifier {
  const p2v_circuit* circ = nullptr;
  int device = 0;
  size_t max_batch = 0, Bmax = 0;
  DevCircuit dc{};
  size_t in_bytes = 0;              // the host-input staging buffer `in`, allocated by the first run that needs it
                                    // (device-resident batches never do: a 131 072-proof workspace saves 16.6 GB)
  std::atomic<bool> p1_recorded{false};   // read by the workspaces chained to this one, from their host threads
  p2v_verifier* chain_prev = nullptr;     // chain links: guarded by g_chain_mu
  std::vector<p2v_verifier*> chain_next;  // workspaces whose chain_prev is this one (cleared when this one is freed)
  unsigned la_seq = 0;
  float last_ms[kNumKernels] = {0};
  bool timed = false;               // all of ev[] exist: p2v_verifier_run records them
  int transcript_mode = 0;          // 0 auto, 1 row, 2 quad, 3 lane (env P2V_TRANSCRIPT)
  int quad_min_batch = 4096;        // auto: quad form from this batch size on (env P2V_QUAD_MIN); round 5: with the
                                    // latency row form (lposeidon.h) the row transcript wins up to 2048 proofs
                                    // (2048: 2.40 against 2.98 ms serial, 1.084 against 1.077 M proofs/s at two in
                                    // flight; 4096: the same serial, 1.13 against 1.225 M; profiles/r05h_*)
  int lane_min_batch = 16384;       // auto: lane form from this batch size on (env P2V_LANE_MIN)
  bool merkle_cse = true;           // shared Merkle nodes hashed once (env P2V_MERKLE_CSE=0: one full path per lane)
  bool cse_dirty = false;           // a run enqueued k_merkle_plan but not k_merkle_resolve
  int known_mode = 1;               // known openings of tree 0 (env P2V_KNOWN_LEAVES: 0 off, 1 probe and insert,
                                    // 2 probe only: every opening misses, the cold cost, measurement)
  const KnownTable* known = nullptr;   // the circuit's table on this device (null: none, over P2V_KNOWN_MAX_MB or off)
  bool known_dirty = false;         // a run enqueued k_merkle_known but not k_status
  int lat_max_batch = 64;           // latency mode (row-form Merkle paths, k_fri on its own stream) up to this
                                    // batch size (env P2V_LAT_MAX, measurement)
  bool single_stream = false;       // env P2V_SINGLE_STREAM=1: no side stream (measurement)
  bool debug_sync = false;          // env P2V_DEBUG_SYNC=1: name each launch on stderr and synchronise after it (fault isolation)
  // JSON ingest on the device (p2v_verifier_run_json): the current template and its device form
  ProofTemplate tmpl;
  bool have_tmpl = false;
  int64_t skel_len = 0, ntok = 0;
  // binary-proof ingest (p2v_verifier_run_bytes): the circuit's byte map on the device, made once
  bool have_bmap = false;
  int nruns = 0, nchk = 0;
  int64_t bfixed = 0;

  // What the workspace owns on the device.  Members are destroyed in reverse order: the buffers
  // first (hipFree waits for the device, so nothing is queued any more), then the streams, the
  // events and the pinned memory.
  // pinned host staging for the small device->host results (statuses, JSON ok flags): a copy
  // to pageable memory would stage through the runtime and stall the other streams' work
  PinnedBuf h_res;
  Event ev[2 * kNumKernels];        // start/end per kernel
  Event dep_p1, dep_side, dep_fri, dep_v3;
  Event p1_done;                    // recorded on the caller's stream after phase 1 (p2v_verifier_chain)
  // transcript lookahead (P2V_FLAG_LOOKAHEAD): its own stream, two challenge buffers used by
  // alternate runs; tr_done[s]: the transcript into buffer s is complete, chal_free[s]: the run
  // that read buffer s has completed (k_status)
  Event tr_done[2], chal_free[2];
  Stream side;
  Stream side2;                     // small batches: k_fri beside the vanishing kernels (latency mode)
  Stream ts;                        // the lookahead transcript's
  Stream side3;                     // latency mode: the coset / misc vanishing kernels beside the Poseidon parts
  DevBuf kid;                       // staging for key ids given in host memory (p2v_verifier_run_keyed): Bmax u32
  DevBuf in, chal, chal2, leafdig, mk, fbits, qvals, van, vparts, lutre, lutpart, res, trace;
  DevBuf m_plan, m_fol, m_chain, m_count, m_fix, m_badq, m_node;   // shared-node Merkle paths (dev.h mcse)
  DevBuf k_miss, k_missn;           // known openings: this workspace's miss list and its length
  DevBuf t_cs, t_kis, t_gkind, t_gpar, t_ggrp, t_gwoff, t_w, t_gs, t_ge, t_lin, t_lout, t_loff, t_llen, t_tw, t_ops, t_vit, t_rin, t_rout, t_roff, t_rch, t_pbase, t_pw, t_gprog, t_gpoff;
  DevBuf j_blob, j_offs, j_skel, j_tok, j_ok;          // JSON / binary ingest, grown on demand
  DevBuf b_rsrc, b_rdst, b_rlen, b_coff, b_cval;       // the byte map
};
struct VerifierFree { void operator()(p2v_verifier* v) const { p2v_verifier_free(v); } };
using VerifierPtr = std::unique_ptr<p2v_verifier, VerifierFree>;

// One device's pipeline for batches in host memory (p2v_verify_batch / _devices): a verifier, a
// compute stream and a copy stream, and a ring of kRing device chunk buffers, so chunk i+1's H2D
// copy (copy stream) overlaps chunk i's verification (compute stream) and up to kRing chunks are in
// flight.  Owned by the circuit's pool, reused across calls.
struct HostPipe {
  static constexpr int kRing = 3;
  int device = -1;
  size_t cap = 0;                 // the verifier's max_batch = the largest chunk
  bool have_ring = false;
  std::vector<uint64_t> hoffs[kRing];
  bool busy = false;
  // owned, destroyed in reverse order: the buffers, the events, the pinned memory, the streams
  // and last the verifier (through p2v_verifier_free)
  VerifierPtr v;
  Stream st, cs;
  PinnedBuf h_res, h_ok;          // pinned staging for dres and dok
  Event copied[kRing], freed[kRing];
  DevBuf ring[kRing];
  DevBuf kring[kRing];            // the chunks' key ids (p2v_verify_batch_keyed): cap u32 each
  DevBuf dres;                    // device statuses of the whole call (grown on demand)
  // binary-proof ingest (p2v_verify_batch_bytes): per ring slot the chunk's bytes and offsets on
  // the device, the offsets' host copy (hoffs, rewritten once the slot's previous copy is done),
  // and the device packer's ok flags of the whole call
  DevBuf bbytes[kRing], boffs[kRing], dok;
};

namespace {
void pipe_free(HostPipe* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->st) (void)hipStreamSynchronize(p->st);
  if (p->cs) (void)hipStreamSynchronize(p->cs);
  delete p;
}
constexpr int kPoolIdleMax = 4;   // idle pipes kept per (circuit, device)

#define HCK_AS(what, x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { return fail(P2V_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e_)); } } while (0)
#define HCK(x) HCK_AS(#x, x)
#define RCK(x) do { const int rc_ = (x); if (rc_ != P2V_OK) return rc_; } while (0)   // a P2V_* code passed on

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

p2v_circuit::~p2v_circuit() {
  for (HostPipe* p : pool) pipe_free(p);
  for (auto& k : known) { (void)hipSetDevice(k->device); k.reset(); }
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

// the staging buffer for batches given in host memory (run from host, JSON / binary ingest)
static hipError_t input_buf(p2v_verifier* v) {
  return v->in.p ? hipSuccess : v->in.alloc(v->in_bytes);
}

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
  }
  ACK(v->kid.alloc(v->Bmax * sizeof(uint32_t)));
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

size_t p2v_tiled_words(size_t n, size_t proof_words) { return (n + 63) / 64 * 64 * proof_words; }

void p2v_tile_proofs(const uint64_t* pm, size_t n, size_t W, uint64_t* tiled) {
  if (!pm || !tiled) return;
  const size_t tiles = (n + 63) / 64;
  for (size_t t = 0; t < tiles; t++) {
    uint64_t* dst = tiled + t * W * 64;
    for (size_t w = 0; w < W; w++)
      for (size_t l = 0; l < 64; l++) {
        const size_t i = t * 64 + l;
        dst[w * 64 + l] = i < n ? pm[i * W + w] : 0;
      }
  }
}

// the transcript form's kernel (tl lanes per proof; 1: lane, else row / quad): with the
// leaf hashing in its launch, and on its own (the lookahead path).  A keyed run (d.key_id set)
// takes the kernels whose digest absorb reads the lane's key; the unkeyed kernels are untouched.
static void launch_phase1(const DevCircuit& d, int tl, int nt_blocks, int leaf_blocks, hipStream_t s) {
  auto* k = d.key_id ? (tl == 1 ? k_phase1_lane_keyed : k_phase1_keyed) : (tl == 1 ? k_phase1_lane : k_phase1);
  k<<<nt_blocks + leaf_blocks, 256, 0, s>>>(d, nt_blocks, tl);
}
static void launch_transcript(const DevCircuit& d, int tl, int nt_blocks, hipStream_t s) {
  auto* k = d.key_id ? (tl == 1 ? k_transcript_lane_keyed : k_transcript_keyed) : (tl == 1 ? k_transcript_lane : k_transcript);
  k<<<nt_blocks, 256, 0, s>>>(d, tl);
}
// one class of vanishing items, [first, last) of d.vitems: one wave per item and 64-proof tile
static void launch_vanish(void (*k)(DevCircuit), int first, int last, int NPB, hipStream_t s, const DevCircuit& d) {
  k<<<(last - first) * NPB, 64, 0, s>>>(d);
}

int p2v_verifier_run(p2v_verifier* v, const uint64_t* proofs, size_t n, int8_t* results, uint64_t* trace, void* stream_, uint32_t flags) {
  return p2v_verifier_run_keyed(v, proofs, nullptr, n, results, trace, stream_, flags);
}

// key_ids == nullptr: every proof against key 0, the kernels' unkeyed path (d.key_id stays null)
int p2v_verifier_run_keyed(p2v_verifier* v, const uint64_t* proofs, const uint32_t* key_ids, size_t n, int8_t* results,
                           uint64_t* trace, void* stream_, uint32_t flags) {
  if (!v || (!proofs && n) || !results) return fail(P2V_E_ARG, "null argument");
  if (n > v->max_batch) return fail(P2V_E_ARG, "batch larger than max_batch");
  if (n == 0) return P2V_OK;
  HCK(hipSetDevice(v->device));
  hipStream_t st = (hipStream_t)stream_;
  const Circuit& C = v->circ->c;
  DevCircuit d = v->dc;
  d.n = (int)n;
  d.unit_filters = (flags & P2V_FLAG_UNIT_FILTERS) ? 1 : 0;
  d.tiled = (flags & P2V_FLAG_INPUT_TILED) ? 1 : 0;
  d.wstride = d.tiled ? 64 : 1;
  d.B = (int)((n + 63) / 64 * 64);
  const int64_t words = C.L.words;
  const uint64_t* src = proofs;
  if (!(flags & P2V_FLAG_INPUT_DEVICE)) {
    const size_t in_words = d.tiled ? p2v_tiled_words(n, (size_t)words) : (size_t)words * n;
    HCK(input_buf(v));
    HCK(hipMemcpyAsync(v->in.p, proofs, in_words * 8, hipMemcpyHostToDevice, st));
    src = (const uint64_t*)v->in.p;
  }
  d.key_id = key_ids;
  if (key_ids && !(flags & P2V_FLAG_INPUT_DEVICE)) {
    HCK(hipMemcpyAsync(v->kid.p, key_ids, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    d.key_id = (const uint32_t*)v->kid.p;
  }
  int8_t* dres = (flags & P2V_FLAG_RESULT_DEVICE) ? results : (int8_t*)v->res.p;
  uint64_t* dtrace = nullptr;
  if (trace) dtrace = (flags & P2V_FLAG_RESULT_DEVICE) ? trace : (uint64_t*)v->trace.p;
  const int NPB = d.B / 64;
  const bool tm = v->timed;
  hipStream_t sd = v->single_stream ? st : (hipStream_t)v->side;
  uint32_t timed_mask = 0;   // slots recorded in this run (only those are read back)
#define T0(k, s_) do { if (tm) { HCK(hipEventRecord(v->ev[2 * (k)], s_)); timed_mask |= 1u << (k); } } while (0)
#define T1(k, s_) do { if (tm) HCK(hipEventRecord(v->ev[2 * (k) + 1], s_)); } while (0)
  // fault isolation (P2V_DEBUG_SYNC=1): each launch is named before it runs and waited for
#define DBG(name, s_) do { if (v->debug_sync) { fprintf(stderr, "p2v: launched %s\n", name); fflush(stderr); \
    HCK(hipStreamSynchronize(s_)); HCK(hipGetLastError()); fprintf(stderr, "p2v: finished %s\n", name); fflush(stderr); } } while (0)
  d.soa = src;   // kernels read the caller's batch in place (devcommon.h ld())
  // phase 1: transcript waves + leaf-hash waves in one launch (the leaf sponges do not
  // depend on the challenges, so they fill the GPU while the serial transcripts run)
  // transcript form: the row form (16 lanes/proof) has the lowest latency, the quad form
  // (4 lanes/proof) a lower total cost; batches from 4096 proofs hide the quad latency behind
  // their leaf hashing.  P2V_TRANSCRIPT=row|quad|lane overrides (measurement).
  // From lane_min_batch on, the lane form (one lane per proof, about half of the quad's issue
  // cycles per proof: 85.9 M against 169.4 M VALU instructions per 4096 proofs, DESIGN.md §7.0,
  // with a ~5.7 ms chain): the batch's leaf hashing in the same launch outlasts the chain, so it
  // costs no latency (C5's 131 072-proof launches +2.9 %, C3's 16 384 +1 %)
  int tl = d.B >= v->lane_min_batch ? 1 : d.B >= v->quad_min_batch ? 4 : 16;
  if (v->transcript_mode == 1) tl = 16;
  else if (v->transcript_mode == 2) tl = 4;
  else if (v->transcript_mode == 3) tl = 1;
  const int nt_blocks = (tl * d.B + 255) / 256;
  // Known openings of tree 0 (merkle.hip k_merkle_known): runs above the latency mode with the
  // shared-node paths.  Tree 0 then leaves the leaf units and the plan / chains / resolve; its
  // statuses come from the probe and the miss kernel at the head of the side stream.  A keyed run
  // takes the table only on a handle with more than one key whose table covers them all (the
  // kernels index it by the id clamped to nkeys - 1); a keyed run on a one-key handle keeps the
  // launch sequence it had.
  const bool lat = d.n <= v->lat_max_batch;
  const bool key_rows = !key_ids || (d.nkeys > 1 && v->known && v->known->kkeys == d.nkeys);
  if (v->known && key_rows && !lat && d.mcse) {
    d.kmode = v->known_mode; d.kskip = 1;
    int k = 0;
    for (int j = 0; j < d.T; j++) if (v->dc.leaf_order[j] != 0) d.leaf_order[k++] = v->dc.leaf_order[j];
    d.nleaf = k;
  }
  const int leaf_units = d.Q * d.nleaf * NPB;
  // staggered workspaces (p2v_verifier_chain): phase 1 after the linked workspace's latest one
  bool chained = false;   // read under the lock: chain links may change from other host threads
  {
    std::lock_guard<std::mutex> lk(g_chain_mu);   // the linked workspace cannot be freed meanwhile
    chained = v->chain_prev != nullptr;
    if (v->chain_prev && v->chain_prev->p1_recorded.load(std::memory_order_acquire))
      HCK(hipStreamWaitEvent(st, v->chain_prev->p1_done, 0));
  }
  // transcript lookahead: the transcript on v->ts into the challenge buffer of this run's parity,
  // after the run that last read that buffer; the leaf hashing on st; k_merkle after both
  const bool la = (flags & P2V_FLAG_LOOKAHEAD) && (flags & P2V_FLAG_INPUT_DEVICE) && sd != st && !chained;
  int la_slot = 0;
  if (la) {
    if (!v->ts) HCK(v->ts.create());
    la_slot = (int)(v->la_seq++ & 1u);
    d.chal = (uint64_t*)(la_slot ? v->chal2.p : v->chal.p);
    HCK(hipStreamWaitEvent(v->ts, v->chal_free[la_slot], 0));
    T0(SLOT_TRANSCRIPT, v->ts);
    launch_transcript(d, tl, nt_blocks, v->ts);
    DBG("k_transcript", v->ts);
    T1(SLOT_TRANSCRIPT, v->ts);
    HCK(hipEventRecord(v->tr_done[la_slot], v->ts));
    T0(SLOT_LEAF, st);
    k_leaf<<<(leaf_units + 3) / 4, 256, 0, st>>>(d);
    DBG("k_leaf", st);
    T1(SLOT_LEAF, st);
    HCK(hipStreamWaitEvent(st, v->tr_done[la_slot], 0));   // k_merkle reads the query indices
    HCK(hipEventRecord(v->dep_p1, st));                     // the side kernels read the challenges
    HCK(hipStreamWaitEvent(sd, v->dep_p1, 0));
  } else {
    T0(SLOT_PHASE1, st);
    launch_phase1(d, tl, nt_blocks, (leaf_units + 3) / 4, st);
    DBG("k_phase1", st);
    T1(SLOT_PHASE1, st);
    if (sd != st) {
      HCK(hipEventRecord(v->dep_p1, st));
      HCK(hipStreamWaitEvent(sd, v->dep_p1, 0));
    }
  }
  HCK(hipEventRecord(v->p1_done, st));   // k_merkle's inputs are complete on st here in both forms
  v->p1_recorded.store(true, std::memory_order_release);
  // latency mode (at most 64 proofs): the Merkle paths in the row form (k_merkle_row: 16 lanes per
  // path, 4x shorter chains, 16x the lanes), one-wave work-groups for k_fri, and k_fri on a stream
  // of its own beside the vanishing kernels instead of after them.  Measured:
  // one proof 2.19 -> 1.98 ms, 64 proofs 2.18 -> 2.10 ms; at 128 proofs the row form's lanes cost more than its latency saves
  const int mk_wg = lat ? 64 : 256;
  const bool fri2 = lat && sd != st;
  if (fri2 && !v->side2) HCK(v->side2.create());
  if (fri2) {
    HCK(hipStreamWaitEvent(v->side2, v->p1_done, 0));
    T0(SLOT_FRI, v->side2);
    k_fri<<<(d.Q * NPB * 64 + mk_wg - 1) / mk_wg, mk_wg, 0, v->side2>>>(d);
    DBG("k_fri", v->side2);
    T1(SLOT_FRI, v->side2);
    HCK(hipEventRecord(v->dep_fri, v->side2));
  }
  // phase 2: Merkle paths on the main stream; FRI queries and the vanishing kernel (few,
  // long-latency waves) on the side stream, concurrently
  if (d.kmode) {   // tree 0 from the table, first on the side stream (P2V_SINGLE_STREAM: in line); on the main stream
                   // before k_merkle_plan it measured 2.4 % slower pipelined
    // k_status zeroes the miss counter for the next run; a run that stopped in between leaves it to be zeroed here
    if (v->known_dirty) HCK(hipMemsetAsync(v->k_missn.p, 0, 64, sd));
    v->known_dirty = true;
    T0(SLOT_KNOWN, sd);
    k_merkle_known<<<(unsigned)(((int64_t)d.Q * d.n * 16 + 255) / 256), 256, 0, sd>>>(d);
    DBG("k_merkle_known", sd);
    // grid-stride over the miss list, as k_merkle_fix; at least one lane per opening of a full list
    const unsigned miss_blocks = (unsigned)std::max<int64_t>(P2V_KNOWN_MISS_BLOCKS, ((int64_t)d.Q * d.n + 255) / 256);
    k_merkle_known_miss<<<miss_blocks, 256, 0, sd>>>(d);
    DBG("k_merkle_known_miss", sd);
    T1(SLOT_KNOWN, sd);
  }
  T0(SLOT_LUT, sd);
  if (d.n_lut_pieces > 0) k_lut<<<(d.r * d.n_lut_pieces * NPB + 3) / 4, 256, 0, sd>>>(d);
  DBG("k_lut", sd);
  T1(SLOT_LUT, sd);
  // the vanishing items in one kernel per class (register allocation per class), timed together
  T0(SLOT_VANISH, sd);
  // (one wave per work-group; the _r2 forms hold exactly the standard 2 challenge rounds)
  const bool r2 = d.r == 2;
  // latency mode: the coset and misc items on a stream of their own, beside the Poseidon parts
  // (each class is a handful of waves whose chain is the batch's tail)
  hipStream_t sv = sd;
  if (fri2) {
    if (!v->side3) HCK(v->side3.create());
    HCK(hipStreamWaitEvent(v->side3, v->p1_done, 0));
    sv = v->side3;
  }
  if (d.vcls[1] > d.vcls[0]) launch_vanish(r2 ? k_vanish_poseidon_r2 : k_vanish_poseidon_rn, d.vcls[0], d.vcls[1], NPB, sd, d);
  DBG("k_vanish_poseidon", sd);
  if (d.vcls[2] > d.vcls[1]) launch_vanish(r2 ? k_vanish_coset_r2 : k_vanish_coset_rn, d.vcls[1], d.vcls[2], NPB, sv, d);
  DBG("k_vanish_coset", sv);
  launch_vanish(r2 ? k_vanish_r2 : k_vanish_rn, d.vcls[2], d.vcls[3], NPB, sv, d);   // never empty: the Z(1) item
  DBG("k_vanish", sv);
  if (sv != sd) {
    HCK(hipEventRecord(v->dep_v3, sv));
    HCK(hipStreamWaitEvent(sd, v->dep_v3, 0));   // k_vanish_final sums every item
  }
  if (d.vcls[4] > d.vcls[3]) launch_vanish(r2 ? k_vanish_lookup_r2 : k_vanish_lookup_rn, d.vcls[3], d.vcls[4], NPB, sd, d);
  DBG("k_vanish_lookup", sd);
  // the program gates (vanish_prog.hip): after the other classes on the side stream, so a circuit
  // without them runs the launch sequence it always did
  if (d.vcls[5] > d.vcls[4]) launch_vanish(r2 ? k_vanish_prog_r2 : k_vanish_prog_rn, d.vcls[4], d.vcls[5], NPB, sd, d);
  DBG("k_vanish_prog", sd);
  T1(SLOT_VANISH, sd);
  T0(SLOT_VANISH_FINAL, sd);
  k_vanish_final<<<(d.B + 255) / 256, 256, 0, sd>>>(d);
  DBG("k_vanish_final", sd);
  T1(SLOT_VANISH_FINAL, sd);
  if (!fri2) {   // after the vanishing kernels (before them: pipelined -1.5 %, DESIGN.md "Retired run-time switches")
    T0(SLOT_FRI, sd);
    k_fri<<<(d.Q * NPB * 64 + 255) / 256, 256, 0, sd>>>(d);
    DBG("k_fri", sd);
    T1(SLOT_FRI, sd);
  }
  if (sd != st) HCK(hipEventRecord(v->dep_side, sd));
  T0(SLOT_MERKLE, st);
  const int merkle_units = d.Q * d.T * NPB;
  if (lat) k_merkle_row<<<(unsigned)(((int64_t)d.Q * d.T * d.n * 16 + 255) / 256), 256, 0, st>>>(d);
  else if (d.mcse) {
    // shared nodes once: plan + bucketed chains + followers' statuses (merkle.hip); the chain
    // grid covers every bucket's last partial wave
    const int ncls = 1 + d.S;
    // k_merkle_resolve zeroes the bucket counters for the next run; a run that stopped between
    // the plan and the resolve (an error return) leaves them to be zeroed here
    if (v->cse_dirty) HCK(hipMemsetAsync(v->m_count.p, 0, (size_t)(d.depth0 + 2) * 64, st));
    v->cse_dirty = true;
    k_merkle_plan<<<(ncls * d.Q * NPB + P2V_PLAN_WAVES - 1) / P2V_PLAN_WAVES, 64 * P2V_PLAN_WAVES, 0, st>>>(d);
    DBG("k_merkle_plan", st);
    const int64_t cse_waves = ((int64_t)(d.T - d.kskip) * d.Q * d.n + 63) / 64 + d.depth0 + 1;
    k_merkle_cse<<<(unsigned)((cse_waves + 31) / 32 * 8), 256, 0, st>>>(d);   // a multiple of 8 blocks (cse_wave: XCD ranges)
    DBG("k_merkle_cse", st);
    // grid-stride over the (usually empty) list: the latency form for up to 16 entries per block,
    // the lane form beyond (one wave per SIMD: a list of every follower, a garbage batch, costs about one
    // more batch); a larger grid waited ~0.5 ms per launch for free slots beside the other batch (r06e)
    k_merkle_fix<<<P2V_FIX_BLOCKS, 256, 0, st>>>(d);
    DBG("k_merkle_fix", st);
    k_merkle_resolve<<<(d.Q * (d.T - d.kskip) * NPB + 3) / 4, 256, 0, st>>>(d);
    DBG("k_merkle_resolve", st);
    v->cse_dirty = false;
  } else k_merkle<<<(merkle_units + 3) / 4, 256, 0, st>>>(d);
  DBG("k_merkle", st);
  T1(SLOT_MERKLE, st);
  if (sd != st) HCK(hipStreamWaitEvent(st, v->dep_side, 0));
  if (fri2) HCK(hipStreamWaitEvent(st, v->dep_fri, 0));
  T0(SLOT_STATUS, st);
  k_status<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(d, dres, dtrace, C.trace_words);
  DBG("k_status", st);
  T1(SLOT_STATUS, st);
  v->known_dirty = false;
  // the challenge buffer's last reader is done (a run without the flag used buffer 0: a later
  // lookahead transcript into buffer 0 must wait for it as well)
  if (la) HCK(hipEventRecord(v->chal_free[la_slot], st));
  else if (sd != st) HCK(hipEventRecord(v->chal_free[0], st));
#undef T0
#undef T1
#undef DBG
  HCK(hipGetLastError());
  if (!(flags & P2V_FLAG_RESULT_DEVICE)) {
    HCK(hipMemcpyAsync(v->h_res.p, dres, n, hipMemcpyDeviceToHost, st));
    if (trace) HCK(hipMemcpyAsync(trace, dtrace, (size_t)C.trace_words * n * 8, hipMemcpyDeviceToHost, st));
  }
  if (!(flags & P2V_FLAG_NO_SYNC) || !(flags & P2V_FLAG_RESULT_DEVICE)) {
    HCK(hipStreamSynchronize(st));
    if (!(flags & P2V_FLAG_RESULT_DEVICE)) memcpy(results, v->h_res.p, n);
    if (tm) {
      for (int k = 0; k < kNumKernels; k++) {
        float ms = 0;
        if ((timed_mask >> k) & 1u) { if (hipEventElapsedTime(&ms, v->ev[2 * k], v->ev[2 * k + 1]) == hipSuccess) v->last_ms[k] = ms; }
        else v->last_ms[k] = 0;   // not launched in this build / run
      }
      (void)hipGetLastError();   // a failed timing query must not surface as the next call's error
    }
  }
  return P2V_OK;
}

// a pipe of circuit c on `device` whose verifier holds `cap` proofs: an idle one of the pool (the
// smallest that fits), else a new one
static int pipe_acquire(const p2v_circuit* c, int device, size_t cap, HostPipe** out) {
  *out = nullptr;
  {
    std::lock_guard<std::mutex> lk(c->pool_mu);
    HostPipe* best = nullptr;
    for (HostPipe* p : c->pool)
      if (!p->busy && p->device == device && p->cap >= cap && (!best || p->cap < best->cap)) best = p;
    if (best) { best->busy = true; *out = best; return P2V_OK; }
  }
  auto* p = new HostPipe();
  p->device = device; p->cap = cap;
  int rc = P2V_OK;
  if (hipSetDevice(device) != hipSuccess || p->st.create() != hipSuccess || p->cs.create() != hipSuccess)
    rc = fail(P2V_E_DEVICE, "stream creation on device " + std::to_string(device));
  p2v_verifier* v = nullptr;
  if (rc == P2V_OK) rc = p2v_verifier_create(c, device, cap, &v);
  p->v.reset(v);
  if (rc != P2V_OK) { pipe_free(p); return rc; }
  p->busy = true;
  std::lock_guard<std::mutex> lk(c->pool_mu);
  c->pool.push_back(p);
  *out = p;
  return P2V_OK;
}

static void pipe_release(const p2v_circuit* c, HostPipe* p, bool broken) {
  HostPipe* drop = nullptr;
  {
    std::lock_guard<std::mutex> lk(c->pool_mu);
    p->busy = false;
    int idle = 0;
    for (HostPipe* q : c->pool) idle += (!q->busy && q->device == p->device) ? 1 : 0;
    if (broken || idle > kPoolIdleMax) {   // a pipe whose run failed is not reused
      c->pool.erase(std::remove(c->pool.begin(), c->pool.end(), p), c->pool.end());
      drop = p;
    }
  }
  pipe_free(drop);
}

// what a chunked call of n proofs of W words needs on pipe p: the ring (made once), the device
// statuses and their pinned copy, and for the binary path (want_ok) the same for the ok flags
static int pipe_prepare(HostPipe* p, size_t n, size_t W, bool want_ok) {
  if (!p->have_ring) {
    for (int k = 0; k < HostPipe::kRing; k++) {
      HCK(p->ring[k].alloc(p->cap * W * 8));
      HCK(p->kring[k].alloc(p->cap * sizeof(uint32_t)));
      if (!p->copied[k]) HCK(p->copied[k].create());
      if (!p->freed[k]) HCK(p->freed[k].create());
    }
    p->have_ring = true;
  }
  HCK(p->dres.grow(n));
  if (want_ok) HCK(p->dok.grow(n));
  HCK(p->h_res.grow(n));
  if (want_ok) HCK(p->h_ok.grow(n));
  return P2V_OK;
}

// the verifier capacity for m proofs in chunks of ch: one chunk in 64-proof granules (powers of
// two), else the chunk
static size_t pipe_cap(size_t m, size_t ch) {
  size_t cap = 64;
  while (cap < std::min(m, ch)) cap <<= 1;
  if (m > ch) cap = ch;
  return cap;
}

// verify m proofs (proof-major rows in host memory) on pipe p: one run for a single chunk (the
// latency path: H2D, kernels, D2H on the pipe's stream); otherwise chunks of <= p->cap proofs
// through the ring, copies on the copy stream, verification on the compute stream, statuses
// accumulated on the device and copied back once.  key_ids (host memory, or null: key 0): proof
// i's key, each chunk's slice copied with the chunk.
static int pipe_run(HostPipe* p, const uint64_t* src, const uint32_t* key_ids, size_t m, int8_t* results, size_t W, size_t chunk) {
  HCK(hipSetDevice(p->device));
  if (m <= chunk) return p2v_verifier_run_keyed(p->v.get(), src, key_ids, m, results, nullptr, p->st, 0);
  RCK(pipe_prepare(p, m, W, false));
  const size_t nch = (m + chunk - 1) / chunk;
  for (size_t i = 0; i < nch; i++) {
    const int b = (int)(i % HostPipe::kRing);
    const size_t off = i * chunk, len = std::min(chunk, m - off);
    if (i >= (size_t)HostPipe::kRing) HCK(hipStreamWaitEvent(p->cs, p->freed[b], 0));   // its last reader is done
    HCK(hipMemcpyAsync(p->ring[b].p, src + off * W, len * W * 8, hipMemcpyHostToDevice, p->cs));
    if (key_ids) HCK(hipMemcpyAsync(p->kring[b].p, key_ids + off, len * sizeof(uint32_t), hipMemcpyHostToDevice, p->cs));
    HCK(hipEventRecord(p->copied[b], p->cs));
    HCK(hipStreamWaitEvent(p->st, p->copied[b], 0));
    RCK(p2v_verifier_run_keyed(p->v.get(), (const uint64_t*)p->ring[b].p, key_ids ? (const uint32_t*)p->kring[b].p : nullptr, len,
                               (int8_t*)p->dres.p + off, nullptr, p->st, P2V_FLAG_INPUT_DEVICE | P2V_FLAG_RESULT_DEVICE | P2V_FLAG_NO_SYNC));
    HCK(hipEventRecord(p->freed[b], p->st));
  }
  HCK(hipMemcpyAsync(p->h_res.p, p->dres.p, m, hipMemcpyDeviceToHost, p->st));
  HCK(hipStreamSynchronize(p->st));
  memcpy(results, p->h_res.p, m);
  return P2V_OK;
}

// the chunk size of a shard of m proofs: the given one, or (0) about an eighth of the shard in
// multiples of 256 between 256 and 16384, so a batch of a few thousand proofs still has several
// chunks in flight and a large one keeps its launches large
static size_t auto_chunk(size_t m, size_t chunk) {
  if (chunk) return chunk;
  const size_t c = (m / 8 + 255) / 256 * 256;
  return std::min<size_t>(16384, std::max<size_t>(256, c));
}

// p2v_verify_batch_devices and p2v_verify_batch_keyed: shards over `devices`, proof i against key
// key_ids[i] (null: key 0)
static int verify_batch_sharded(const p2v_circuit* c, const uint64_t* proofs, const uint32_t* key_ids, size_t n, int8_t* results,
                                const int* devices, int ndevices, size_t chunk) {
  if (!c || !devices || ndevices <= 0 || (n && (!proofs || !results))) return fail(P2V_E_ARG, "null argument / no devices");
  if (n == 0) return P2V_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(P2V_E_NODEVICE, "no HIP device available: libp2v verifies on MI355X only (no CPU fallback)");
  for (int i = 0; i < ndevices; i++)
    if (devices[i] < 0 || devices[i] >= ndev) return fail(P2V_E_ARG, "bad device index " + std::to_string(devices[i]));
  const size_t W = (size_t)c->c.L.words;
  const int shards = (int)std::min<size_t>((size_t)ndevices, n);
  std::vector<int> rcs(shards, P2V_OK);
  std::vector<std::string> msgs(shards);
  auto work = [&](int s) {
    const size_t base = n / shards, extra = n % shards;   // p2v.shard_bounds
    const size_t a = s * base + std::min<size_t>(s, extra), b = a + base + ((size_t)s < extra ? 1 : 0);
    const size_t m = b - a;
    const size_t ch = m <= 64 ? m : auto_chunk(m, chunk);
    HostPipe* p = nullptr;
    int rc = pipe_acquire(c, devices[s], pipe_cap(m, ch), &p);
    if (rc == P2V_OK) {
      rc = pipe_run(p, proofs + a * W, key_ids ? key_ids + a : nullptr, m, results + a, W, ch);
      pipe_release(c, p, rc != P2V_OK);
    }
    if (rc != P2V_OK) msgs[s] = g_err;   // g_err is thread-local: carry the message back
    rcs[s] = rc;
  };
  if (shards == 1) work(0);   // the calling thread (a drop-in verifyProof call starts no thread)
  else {
    std::vector<std::thread> pool;
    for (int s = 0; s < shards; s++) pool.emplace_back(work, s);
    for (auto& t : pool) t.join();
  }
  for (int s = 0; s < shards; s++)
    if (rcs[s] != P2V_OK)
      return fail(rcs[s], "shard " + std::to_string(s) + " (device " + std::to_string(devices[s]) + "): " + msgs[s]);
  return P2V_OK;
}

int p2v_verify_batch_devices(const p2v_circuit* c, const uint64_t* proofs, size_t n, int8_t* results,
                             const int* devices, int ndevices, size_t chunk) {
  return verify_batch_sharded(c, proofs, nullptr, n, results, devices, ndevices, chunk);
}

int p2v_verify_batch_keyed(const p2v_circuit* c, const uint64_t* proofs, const uint32_t* key_ids, size_t n, int8_t* results, int device) {
  if (!c || (n && (!proofs || !results))) return fail(P2V_E_ARG, "null argument");
  return verify_batch_sharded(c, proofs, key_ids, n, results, &device, 1, 0);
}

// ---- ingest: JSON texts or plonky2 binary proofs -> packed rows of v->in ----

// A batch's texts or bytes and its offsets (rebased to the batch's first byte) on the device, in
// j_blob / j_offs, with room for the packer's ok flags in j_ok.  rel is the offsets' host copy:
// the caller keeps it until the stream is synchronised.
static int stage_batch(p2v_verifier* v, const void* blob, const uint64_t* offsets, size_t n, std::vector<uint64_t>& rel, hipStream_t st) {
  const uint64_t base = offsets[0], bytes = offsets[n] - base;
  HCK(v->j_blob.grow(bytes + 64));   // + vector / unaligned-load slack
  HCK(v->j_offs.grow((n + 1) * 8));
  HCK(v->j_ok.grow(n));
  rel.resize(n + 1);
  for (size_t i = 0; i <= n; i++) rel[i] = offsets[i] - base;
  HCK(hipMemcpyAsync(v->j_blob.p, (const uint8_t*)blob + base, bytes, hipMemcpyHostToDevice, st));
  HCK(hipMemcpyAsync(v->j_offs.p, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
  return P2V_OK;
}

// the device packer's ok flags of the staged batch, read back through the pinned buffer
static int read_ok_flags(p2v_verifier* v, size_t n, std::vector<int8_t>& okf, hipStream_t st) {
  HCK(hipGetLastError());
  HCK(hipMemcpyAsync(v->h_res.p, v->j_ok.p, n, hipMemcpyDeviceToHost, st));
  HCK(hipStreamSynchronize(st));
  okf.assign(v->h_res.p, v->h_res.p + n);
  return P2V_OK;
}

// The proofs the device packer did not take (other formatting, exotic numbers, errors): the host
// reader, one row at a time.  pack_row(i, row) packs proof i or throws as p2v_pack_proof_json /
// _bytes do; codes[i] is that call's code.  n_device receives the count of device-packed proofs.
static int host_fallback(p2v_verifier* v, size_t n, const std::vector<int8_t>& okf, int32_t* codes, size_t* n_device,
                         hipStream_t st, const std::function<void(size_t, uint64_t*)>& pack_row) {
  const size_t W = (size_t)v->circ->c.L.words;
  std::vector<uint64_t> row(W);
  if (n_device) for (size_t i = 0; i < n; i++) *n_device += okf[i] ? 1 : 0;
  for (size_t i = 0; i < n; i++) {
    codes[i] = P2V_OK;
    if (okf[i]) continue;
    try {
      pack_row(i, row.data());
      HCK(hipMemcpyAsync((uint64_t*)v->in.p + i * W, row.data(), W * 8, hipMemcpyHostToDevice, st));
      HCK(hipStreamSynchronize(st));   // row is reused
    } catch (const ShapeError&) { codes[i] = P2V_E_SHAPE; }
    catch (...) { codes[i] = P2V_E_PARSE; }
  }
  return P2V_OK;
}

// h on the device in b, grown to bytes + slack
static hipError_t put(DevBuf& b, const void* h, size_t bytes, size_t slack) {
  hipError_t e = b.grow(bytes + slack);
  if (e == hipSuccess && bytes) e = hipMemcpy(b.p, h, bytes, hipMemcpyHostToDevice);
  return e;
}

// JSON texts: the device packer against the template, the host reader for the rest
static int pack_json_into(p2v_verifier* v, const char* blob, const uint64_t* offsets, size_t n,
                          int32_t* codes, size_t* n_device, void* stream_) {
  if (n_device) *n_device = 0;
  if (!v || (n && (!blob || !offsets || !codes))) return fail(P2V_E_ARG, "null argument");
  if (n > v->max_batch) return fail(P2V_E_ARG, "batch larger than max_batch");
  if (n == 0) return P2V_OK;
  HCK(hipSetDevice(v->device));
  HCK(input_buf(v));
  hipStream_t st = (hipStream_t)stream_;
  const Circuit& C = v->circ->c;
  const int64_t W = C.L.words;
  auto text = [&](size_t i) { return blob + offsets[i]; };
  auto tlen = [&](size_t i) { return (size_t)(offsets[i + 1] - offsets[i]); };
  std::vector<uint64_t> row((size_t)W);
  // template: keep the current one while it packs the batch's first proof, else rebuild it
  // from the first proof the full reader accepts
  bool fresh = false;
  if (!(v->have_tmpl && v->tmpl.pack(text(0), tlen(0), row.data()))) {
    v->have_tmpl = false;
    for (size_t i = 0; i < n && !v->have_tmpl && i < 64; i++) {
      try { v->have_tmpl = v->tmpl.build(C, text(i), tlen(i), row.data()); } catch (...) { v->have_tmpl = false; }
    }
    fresh = v->have_tmpl;
  }
  std::vector<uint8_t> skel; std::vector<int32_t> tok;
  const bool dev_ok = v->have_tmpl && (!fresh || v->tmpl.device_form(skel, tok));
  if (fresh && dev_ok) {
    HCK(put(v->j_skel, skel.data(), skel.size(), 64));   // + vector-load slack
    HCK(put(v->j_tok, tok.data(), tok.size() * sizeof(int32_t), 64));
    v->skel_len = (int64_t)skel.size(); v->ntok = (int64_t)tok.size();
  } else if (fresh || !v->have_tmpl) {
    // a new template without a device form (or none at all): drop the previous template's
    // device form, so no later batch pairs it with this host template
    v->skel_len = 0; v->ntok = 0;
  }
  std::vector<int8_t> okf(n, 0);
  std::vector<uint64_t> rel;
  if (dev_ok && v->ntok > 0) {
    RCK(stage_batch(v, blob, offsets, n, rel, st));
    k_json_pack<<<(unsigned)n, 256, 0, st>>>((const uint8_t*)v->j_blob.p, (const uint64_t*)v->j_offs.p, (int)n, (const uint8_t*)v->j_skel.p,
                                             v->skel_len, (const int32_t*)v->j_tok.p, v->ntok, (uint64_t*)v->in.p, W, (int8_t*)v->j_ok.p);
    RCK(read_ok_flags(v, n, okf, st));
  }
  return host_fallback(v, n, okf, codes, n_device, st, [&](size_t i, uint64_t* dst) {
    JVal pj = parse_json(text(i), tlen(i));
    pack_proof(C, pj, dst);
  });
}

// the circuit's byte map (circuit.cpp bytes_map) on the verifier's device, made once
static int ensure_bytes_map(p2v_verifier* v) {
  if (v->have_bmap) return P2V_OK;
  const BytesMap m = bytes_map(v->circ->c);
  HCK(put(v->b_rsrc, m.run_src.data(), m.run_src.size() * 8, 16));   // (a retry after a failure reuses what is there)
  HCK(put(v->b_rdst, m.run_dst.data(), m.run_dst.size() * 8, 16));
  HCK(put(v->b_rlen, m.run_len.data(), m.run_len.size() * 8, 16));
  HCK(put(v->b_coff, m.chk_off.data(), m.chk_off.size() * 8, 16));
  HCK(put(v->b_cval, m.chk_val.data(), m.chk_val.size(), 16));
  v->nruns = (int)m.run_len.size(); v->nchk = (int)m.chk_off.size(); v->bfixed = m.fixed;
  v->have_bmap = true;
  return P2V_OK;
}

// k_bytes_pack against v's byte map: n proofs of src (offsets offs) into rows, ok flags into ok
static void launch_bytes_pack(const p2v_verifier* v, const DevBuf& src, const DevBuf& offs, size_t n, void* rows, int8_t* ok, hipStream_t st) {
  const Circuit& C = v->circ->c;
  k_bytes_pack<<<(unsigned)n, 256, 0, st>>>((const uint8_t*)src.p, (const uint64_t*)offs.p, (int)n, (const int64_t*)v->b_rsrc.p,
                                            (const int64_t*)v->b_rdst.p, (const int64_t*)v->b_rlen.p, v->nruns, (const int64_t*)v->b_coff.p,
                                            (const uint8_t*)v->b_cval.p, v->nchk, v->bfixed, (int64_t)C.num_pis, C.L.pis,
                                            (uint64_t*)rows, C.L.words, ok);
}

// plonky2 binary proofs: k_bytes_pack against the circuit's byte map, the host reader for any
// proof that fails a check
static int pack_bytes_into(p2v_verifier* v, const uint8_t* blob, const uint64_t* offsets, size_t n,
                           int32_t* codes, size_t* n_device, void* stream_) {
  if (n_device) *n_device = 0;
  if (!v || (n && (!blob || !offsets || !codes))) return fail(P2V_E_ARG, "null argument");
  if (n > v->max_batch) return fail(P2V_E_ARG, "batch larger than max_batch");
  if (n == 0) return P2V_OK;
  HCK(hipSetDevice(v->device));
  HCK(input_buf(v));
  hipStream_t st = (hipStream_t)stream_;
  RCK(ensure_bytes_map(v));
  std::vector<int8_t> okf;
  std::vector<uint64_t> rel;
  RCK(stage_batch(v, blob, offsets, n, rel, st));
  launch_bytes_pack(v, v->j_blob, v->j_offs, n, v->in.p, (int8_t*)v->j_ok.p, st);
  RCK(read_ok_flags(v, n, okf, st));
  return host_fallback(v, n, okf, codes, n_device, st, [&](size_t i, uint64_t* dst) {
    pack_proof_bytes(v->circ->c, blob + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), dst);
  });
}

// plonky2 binary proofs in host memory, verified through the circuit's pooled pipe: per chunk the
// bytes are copied on the copy stream, packed on the device (k_bytes_pack into a ring slot) and
// verified on the compute stream, up to kRing chunks in flight.  Proofs the device packer flags
// are packed by the host reader afterwards and verified in one more run (or get the reader's
// code), so results and codes equal p2v_verifier_run_bytes'.
int p2v_verify_batch_bytes(const p2v_circuit* c, const uint8_t* blob, const uint64_t* offsets, size_t n,
                           int8_t* results, int32_t* codes, size_t* n_device, int device, size_t chunk) {
  if (n_device) *n_device = 0;
  if (!c || (n && (!blob || !offsets || !results || !codes))) return fail(P2V_E_ARG, "null argument");
  if (n == 0) return P2V_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(P2V_E_NODEVICE, "no HIP device available: libp2v verifies on MI355X only (no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(P2V_E_ARG, "bad device index");
  const Circuit& C = c->c;
  const size_t W = (size_t)C.L.words;
  const size_t ch = auto_chunk(n, chunk);
  HostPipe* p = nullptr;
  int rc = pipe_acquire(c, device, pipe_cap(n, ch), &p);
  if (rc != P2V_OK) return rc;
  auto body = [&]() -> int {
    HCK(hipSetDevice(device));
    p2v_verifier* v = p->v.get();
    RCK(ensure_bytes_map(v));
    RCK(pipe_prepare(p, n, W, true));
    const size_t nch = (n + ch - 1) / ch;
    for (size_t i = 0; i < nch; i++) {
      const int b = (int)(i % HostPipe::kRing);
      const size_t off = i * ch, len = std::min(ch, n - off);
      const uint64_t base = offsets[off], bytes = offsets[off + len] - base;
      if (i >= (size_t)HostPipe::kRing) {
        HCK(hipEventSynchronize(p->copied[b]));              // the slot's host offsets are no longer read
        HCK(hipStreamWaitEvent(p->cs, p->freed[b], 0));      // its device buffers' last reader is done
      }
      HCK(p->bbytes[b].grow(bytes + 64));   // + unaligned-load slack
      HCK(p->boffs[b].grow((p->cap + 1) * 8));   // for the largest chunk (len <= cap): made once
      auto& ho = p->hoffs[b];
      ho.resize(len + 1);
      for (size_t k = 0; k <= len; k++) ho[k] = offsets[off + k] - base;
      HCK(hipMemcpyAsync(p->bbytes[b].p, blob + base, bytes, hipMemcpyHostToDevice, p->cs));
      HCK(hipMemcpyAsync(p->boffs[b].p, ho.data(), (len + 1) * 8, hipMemcpyHostToDevice, p->cs));
      HCK(hipEventRecord(p->copied[b], p->cs));
      HCK(hipStreamWaitEvent(p->st, p->copied[b], 0));
      launch_bytes_pack(v, p->bbytes[b], p->boffs[b], len, p->ring[b].p, (int8_t*)p->dok.p + off, p->st);
      HCK(hipGetLastError());
      RCK(p2v_verifier_run(v, (const uint64_t*)p->ring[b].p, len, (int8_t*)p->dres.p + off, nullptr, p->st,
                           P2V_FLAG_INPUT_DEVICE | P2V_FLAG_RESULT_DEVICE | P2V_FLAG_NO_SYNC));
      HCK(hipEventRecord(p->freed[b], p->st));
    }
    HCK(hipMemcpyAsync(p->h_res.p, p->dres.p, n, hipMemcpyDeviceToHost, p->st));
    HCK(hipMemcpyAsync(p->h_ok.p, p->dok.p, n, hipMemcpyDeviceToHost, p->st));
    HCK(hipStreamSynchronize(p->st));
    memcpy(results, p->h_res.p, n);
    // the proofs the device packer did not take: the host reader, then one more run for those it packs
    std::vector<size_t> redo;
    std::vector<uint64_t> rows;
    for (size_t i = 0; i < n; i++) {
      codes[i] = P2V_OK;
      if (p->h_ok.p[i]) { if (n_device) (*n_device)++; continue; }
      rows.resize((redo.size() + 1) * W);
      try {
        pack_proof_bytes(C, blob + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), rows.data() + redo.size() * W);
        redo.push_back(i);
      } catch (const ShapeError&) { codes[i] = P2V_E_SHAPE; results[i] = P2V_ERR_SHAPE; }
      catch (...) { codes[i] = P2V_E_PARSE; results[i] = P2V_ERR_PARSE; }
    }
    if (!redo.empty()) {
      std::vector<int8_t> rr(redo.size());
      RCK(pipe_run(p, rows.data(), nullptr, redo.size(), rr.data(), W, p->cap));
      for (size_t k = 0; k < redo.size(); k++) results[redo[k]] = rr[k];
    }
    return P2V_OK;
  };
  rc = body();
  pipe_release(c, p, rc != P2V_OK);
  return rc;
}

// the packed rows of v->in back to the host (words, if wanted), zeroed where a proof did not pack
static int finish_pack(p2v_verifier* v, int rc, size_t n, const int32_t* codes, uint64_t* words, void* stream_) {
  if (rc != P2V_OK || n == 0 || !words) return rc;
  hipStream_t st = (hipStream_t)stream_;
  const size_t W = (size_t)v->circ->c.L.words;
  HCK(hipMemcpyAsync(words, v->in.p, n * W * 8, hipMemcpyDeviceToHost, st));
  HCK(hipStreamSynchronize(st));
  for (size_t i = 0; i < n; i++)
    if (codes[i] != P2V_OK) memset(words + i * W, 0, W * 8);
  return P2V_OK;
}

// the packed rows of v->in verified; a proof that did not pack gets its reader's status
static int run_packed(p2v_verifier* v, int rc, size_t n, int8_t* results, const int32_t* codes, void* stream_) {
  if (rc != P2V_OK || n == 0) return rc;
  RCK(p2v_verifier_run(v, (const uint64_t*)v->in.p, n, results, nullptr, stream_, P2V_FLAG_INPUT_DEVICE));
  for (size_t i = 0; i < n; i++)
    if (codes[i] != P2V_OK) results[i] = codes[i] == P2V_E_SHAPE ? P2V_ERR_SHAPE : P2V_ERR_PARSE;
  return P2V_OK;
}

int p2v_verifier_pack_bytes(p2v_verifier* v, const uint8_t* blob, const uint64_t* offsets, size_t n,
                            int32_t* codes, size_t* n_device, uint64_t* words, void* stream_) {
  return finish_pack(v, pack_bytes_into(v, blob, offsets, n, codes, n_device, stream_), n, codes, words, stream_);
}

int p2v_verifier_run_bytes(p2v_verifier* v, const uint8_t* blob, const uint64_t* offsets, size_t n,
                           int8_t* results, int32_t* codes, size_t* n_device, void* stream_) {
  if (n && !results) return fail(P2V_E_ARG, "null argument");
  return run_packed(v, pack_bytes_into(v, blob, offsets, n, codes, n_device, stream_), n, results, codes, stream_);
}

int p2v_verifier_pack_json(p2v_verifier* v, const char* blob, const uint64_t* offsets, size_t n,
                           int32_t* codes, size_t* n_device, uint64_t* words, void* stream_) {
  return finish_pack(v, pack_json_into(v, blob, offsets, n, codes, n_device, stream_), n, codes, words, stream_);
}

int p2v_verifier_run_json(p2v_verifier* v, const char* blob, const uint64_t* offsets, size_t n,
                          int8_t* results, int32_t* codes, size_t* n_device, void* stream_) {
  if (n && !results) return fail(P2V_E_ARG, "null argument");
  return run_packed(v, pack_json_into(v, blob, offsets, n, codes, n_device, stream_), n, results, codes, stream_);
}

// p2v_selftest ops 12-20: the field and FRI query code on items read as a proof batch is, through
// a DevCircuit that holds the item array and the tables fill_scalars / fri_twiddles make for a
// circuit with FRI arity bits 1..8 (step s = ab - 1).  b words, item words in and out per op;
// the shared words are checked here, so the kernel reads nothing outside an item.
static int selftest_field(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  static const size_t kB[9] = {0, 0, 0, 0, 0, 1, 1, 12, 1}, kIn[9] = {2, 4, 1, 2, 4, 1, 2, 0, 0}, kOut[9] = {5, 2, 1, 2, 4, 1, 2, 2, 2};
  const size_t bw = kB[op - 12], wo = kOut[op - 12];
  size_t w = kIn[op - 12];
  if (bw && !b) return fail(P2V_E_ARG, "bad op / null argument");
  if (op == 17 && b[0] > 32) return fail(P2V_E_ARG, "pow_root: k > 32");
  if (op == 18 && b[0] > 0xFFFFFFFFull) return fail(P2V_E_ARG, "epow_u: e >= 2^32");
  if (op == 19) {
    w = (size_t)b[0];
    bool ok = b[0] >= 2 && b[0] <= (1u << 20) && b[1] <= 5;
    for (int k = 0; k < 5 && ok; k++) ok = b[2 + k] <= b[0] && b[7 + k] <= b[0] - b[2 + k];
    if (!ok) return fail(P2V_E_ARG, "reduce_powers: segment table outside the item");
  }
  if (op == 20) {
    if (b[0] < 1 || b[0] > 8) return fail(P2V_E_ARG, "fold: arity bits outside 1..8");
    w = 2 + (2u << b[0]);
  }
  if (n > (size_t)INT32_MAX - 64) return fail(P2V_E_ARG, "too many items");
  if (n == 0) return P2V_OK;
  Circuit C;
  C.arities = {1, 2, 3, 4, 5, 6, 7, 8};
  C.step_depth.assign(8, 0); C.L.step_evals.assign(8, 0); C.L.step_path.assign(8, 0);
  DevCircuit d{};
  fill_scalars(C, d);
  DevBuf da, db, dout, dtw;
#define SCK(x) HCK_AS("p2v_selftest", x)
  SCK(da.alloc(n * w * 8)); SCK(db.alloc(bw * 8)); SCK(dout.alloc(n * wo * 8));
  SCK(upload(dtw, fri_twiddles(C), d.twiddles));
  SCK(hipMemcpy(da.p, a, n * w * 8, hipMemcpyHostToDevice));
  if (bw) SCK(hipMemcpy(db.p, b, bw * 8, hipMemcpyHostToDevice));
  d.soa = (const uint64_t*)da.p; d.words = (int64_t)w; d.wstride = 1; d.tiled = 0;
  d.n = (int32_t)n; d.B = (int32_t)((n + 63) / 64 * 64);
  hipLaunchKernelGGL(k_selftest_field, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, d, (const uint64_t*)db.p, (uint64_t*)dout.p);
  SCK(hipGetLastError());
  SCK(hipMemcpy(out, dout.p, n * wo * 8, hipMemcpyDeviceToHost));
#undef SCK
  return P2V_OK;
}

// p2v_selftest op 21: the gate-program interpreter (vanish_prog.hip) on items laid out as a proof's
// openings are: b = nwires, nconsts, the program.  The program is checked here as at circuit
// creation, so the kernel reads nothing outside an item and writes no slot past the file; like the
// other ops' shared words, a b that does not pass is P2V_E_ARG, decided before any device call.
static int selftest_prog(int device, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  if (!b) return fail(P2V_E_ARG, "bad op / null argument");
  if (b[0] > (1u << 20) || b[1] > (1u << 20)) return fail(P2V_E_ARG, "gate program rows beyond this build's limits");
  if (n > (size_t)INT32_MAX - 64) return fail(P2V_E_ARG, "too many items");
  const int64_t nw = (int64_t)b[0], nc = (int64_t)b[1];
  GateProgram g;
  std::vector<uint64_t> low;
  try {
    // the encoding's own instruction count bounds the walk: at most 3 words per instruction
    if (b[2] != P2V_WORDS_GATE_MAGIC) throw ParseError("gate program: bad magic / version");
    if (b[3] > (uint64_t)P2V_GATE_PROGRAM_MAX_INSTRS) throw CircuitError("gate program beyond this build's limits (instructions)");
    g = decode_gate_program(b + 2, gate_program_extent(b + 2, 2 + 3 * (size_t)b[3]));
    if (g.max_wire >= nw || g.max_const >= nc) throw CircuitError("(Array.!): gate program reads beyond the row");
    if (g.max_pih >= 4) throw CircuitError("(!!): gate program reads a public-inputs-hash word beyond 4");
    if (lower_gate_program(g, &low) > P2V_GATE_PROGRAM_MAX_LIVE) throw CircuitError("gate program beyond this build's limits (values alive at once)");
  } catch (const std::exception& e) { return fail(P2V_E_ARG, std::string("selftest op 21: ") + e.what()); }
  const int ndev = p2v_device_count();
  if (ndev == 0) return fail(P2V_E_NODEVICE, "no HIP device");
  if (device < 0 || device >= ndev) return fail(P2V_E_ARG, "bad device index");
  if (n == 0 || g.num_commits == 0) return P2V_OK;
  HCK(hipSetDevice(device));
  const size_t w = (size_t)(2 * (nw + nc) + 4), wo = 2 * (size_t)g.num_commits;
  DevCircuit d{};
  d.prog_pih = 2 * (nw + nc);
  d.o_wires = 0; d.o_const = 2 * nw;   // ngroups = nls = 0: Vars::k(i) is constant i
  d.words = (int64_t)w; d.wstride = 1; d.tiled = 0;
  d.n = (int32_t)n; d.B = (int32_t)((n + 63) / 64 * 64);
  DevBuf da, dout, dprog;
#define SCK(x) HCK_AS("p2v_selftest", x)
  SCK(da.alloc(n * w * 8)); SCK(dout.alloc(n * wo * 8));
  SCK(upload(dprog, low, d.gprog));
  SCK(hipMemcpy(da.p, a, n * w * 8, hipMemcpyHostToDevice));
  d.soa = (const uint64_t*)da.p;
  hipLaunchKernelGGL(k_selftest_prog, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, d, (uint64_t*)dout.p, g.num_commits);
  SCK(hipGetLastError());
  SCK(hipMemcpy(out, dout.p, n * wo * 8, hipMemcpyDeviceToHost));
#undef SCK
  return P2V_OK;
}

int p2v_selftest(int device, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  const bool needs_b = op == 0 || op == 3 || op == 4 || op == 6;
  // op 11 was the retired pair form's permutation; the ops keep their numbers
  if (op < 0 || op > 21 || op == 11 || (n && (!a || !out || (needs_b && !b)))) return fail(P2V_E_ARG, "bad op / null argument");
  if (op == 21) return selftest_prog(device, a, b, out, n);
  const int ndev = p2v_device_count();
  if (ndev == 0) return fail(P2V_E_NODEVICE, "no HIP device");
  if (device < 0 || device >= ndev) return fail(P2V_E_ARG, "bad device index");
  if (op < 12 && n == 0) return P2V_OK;
  HCK(hipSetDevice(device));
  if (op >= 12) return selftest_field(op, a, b, out, n);
  // words per item of a / b and of out
  const bool scalar = op == 0 || op == 3 || op == 5 || op == 6 || op == 7 || op == 8;
  const size_t w = scalar ? 1 : 12, wo = op == 6 ? 2 : w;
  const size_t bw = op == 4 ? 24 : scalar && needs_b ? n : 2;
  DevBuf da, db, dout;
#define SCK(x) HCK_AS("p2v_selftest", x)
  SCK(da.alloc(n * w * 8)); SCK(db.alloc(bw * 8)); SCK(dout.alloc(n * wo * 8));
  SCK(hipMemcpy(da.p, a, n * w * 8, hipMemcpyHostToDevice));
  if (needs_b) SCK(hipMemcpy(db.p, b, bw * 8, hipMemcpyHostToDevice));
  if (op >= 9) {
    const int lanes = op == 9 ? 16 : 4;
    hipLaunchKernelGGL(k_selftest_forms, dim3((unsigned)((n * lanes + 255) / 256)), dim3(256), 0, 0, op, (const uint64_t*)da.p,
                       (uint64_t*)dout.p, (int64_t)n);
  } else {
    const size_t lanes = op == 8 ? 2 : 1;   // op 8: a lane pair per item
    hipLaunchKernelGGL(k_selftest, dim3((unsigned)((n * lanes + 255) / 256)), dim3(256), 0, 0, op, (const uint64_t*)da.p,
                       (const uint64_t*)db.p, (uint64_t*)dout.p, (int64_t)n);
  }
  SCK(hipGetLastError());
  SCK(hipMemcpy(out, dout.p, n * wo * 8, hipMemcpyDeviceToHost));
#undef SCK
  return P2V_OK;
}

int p2v_count_mismatches(const int8_t* results, const int8_t* expect, size_t n, uint64_t* counters, void* stream) {
  if (!counters || (n && (!results || !expect))) return fail(P2V_E_ARG, "null argument");
  const unsigned blocks = n ? (unsigned)((n + 255) / 256) : 1;
  hipLaunchKernelGGL(k_count_mismatches, dim3(blocks), dim3(256), 0, (hipStream_t)stream, results, expect, (int64_t)n,
                     (unsigned long long*)counters);
  HCK(hipGetLastError());
  return P2V_OK;
}

int p2v_clock_probe(uint64_t* stamps, int nblocks, void* stream) {
  if (!stamps || nblocks <= 0) return fail(P2V_E_ARG, "null argument / no blocks");
  hipLaunchKernelGGL(k_clock_probe, dim3((unsigned)nblocks), dim3(64), 0, (hipStream_t)stream, (unsigned long long*)stamps);
  HCK(hipGetLastError());
  return P2V_OK;
}

int p2v_verifier_last_timings(const p2v_verifier* v, float* out, int max) {
  if (!v || !out) return 0;
  int k = 0;
  for (; k < kNumKernels && k < max; k++) out[k] = v->last_ms[k];
  return k;
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

int p2v_verify_batch(const p2v_circuit* c, const uint64_t* proofs, size_t n, int8_t* results, int device) {
  return p2v_verify_batch_keyed(c, proofs, nullptr, n, results, device);
}

}  // extern "C"
