// api_internal.hpp — what more than one host unit of the C-ABI (api*.cpp) needs: the error
// plumbing, the resource owners, the three handle structs and the few helpers that cross units.
// Everything between the visibility pragmas had internal linkage while the C-ABI was one
// translation unit; hidden visibility keeps it out of libp2v.so's exports.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>
#include "../../include/p2v.h"
#include "circuit.hpp"
#include "dev.h"

using namespace p2v;

#pragma GCC visibility push(hidden)
extern thread_local std::string g_err;   // defined in api.cpp
inline int fail(int code, const std::string& msg) { g_err = msg; return code; }

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
inline const char* kKernelNames = "k_transpose,k_phase1,k_merkle,k_fri,k_vanish,k_status,k_vanish_final,k_lut,k_leaf,k_transcript,k_merkle_known";
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
inline hipError_t pinned_alloc(void** p, size_t n) { return hipHostMalloc(p, n); }
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

// a table on the device, and the DevCircuit field that points to it
template <class T>
hipError_t upload(DevBuf& b, const std::vector<T>& h, const T*& field) {
  hipError_t e = b.alloc(h.size() * sizeof(T));
  if (e != hipSuccess) return e;
  field = (const T*)b.p;
  if (!h.empty()) e = hipMemcpy(b.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
  return e;
}

extern std::mutex g_chain_mu;   // p2v_verifier_chain links (chain_prev / chain_next of every verifier)  (api_workspace.cpp)
#pragma GCC visibility pop

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
  // the key lookup table (dev.h DevCircuit::key_tab), built by the first call that needs it
  // (p2v_circuit_find_key, p2v_verifier_create); the key table never changes after construction
  mutable std::once_flag key_tab_once;
  mutable std::vector<uint32_t> key_tab;
  const std::vector<uint32_t>& key_lookup() const;   // api.cpp
  ~p2v_circuit();
};

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
  DevBuf kres[2];                   // the ids k_key_resolve writes (self-keyed runs), Bmax u32 each: [la_slot], as the
                                    // challenge buffers, so two lookahead runs in flight keep their own
  DevBuf t_ktab;                    // DevCircuit::key_tab
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

#define HCK_AS(what, x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { return fail(P2V_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e_)); } } while (0)
#define HCK(x) HCK_AS(#x, x)
#define RCK(x) do { const int rc_ = (x); if (rc_ != P2V_OK) return rc_; } while (0)   // a P2V_* code passed on

#pragma GCC visibility push(hidden)
// api_workspace.cpp
void fill_scalars(const Circuit& C, DevCircuit& d);
std::vector<uint64_t> fri_twiddles(const Circuit& C);
hipError_t input_buf(p2v_verifier* v);
// api_pipe.cpp
void pipe_free(HostPipe* p);
int pipe_acquire(const p2v_circuit* c, int device, size_t cap, HostPipe** out);
void pipe_release(const p2v_circuit* c, HostPipe* p, bool broken);
int pipe_prepare(HostPipe* p, size_t n, size_t W, bool want_ok);
size_t pipe_cap(size_t m, size_t ch);
int pipe_run(HostPipe* p, const uint64_t* src, const uint32_t* key_ids, size_t m, int8_t* results, size_t W, size_t chunk);
size_t auto_chunk(size_t m, size_t chunk);
#pragma GCC visibility pop
