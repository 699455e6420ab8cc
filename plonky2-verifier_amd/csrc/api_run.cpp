// api_run.cpp — one batch on a workspace: the launch sequence of p2v_verifier_run_keyed, its
// timings, and the 64-proof tiling helpers.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include "api_internal.hpp"
#include "kernels.h"

extern "C" {

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

// key_ids == nullptr: every proof against key 0, the kernels' unkeyed path (d.key_id stays null);
// on a self-keyed handle instead the ids k_key_resolve reads from the proofs (keys.hip), and the
// run is a keyed run from there on
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
  const bool resolve = !key_ids && C.self_keyed;   // d.key_id: the id buffer of this run's parity, set where it is launched
  const bool has_ids = key_ids || resolve;
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
  const bool key_rows = !has_ids || (d.nkeys > 1 && v->known && v->known->kkeys == d.nkeys);
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
    if (resolve) {   // ahead of the transcript, its first reader; the run that last read this id buffer is the
                     // one that last read the challenge buffer (k_leaf on st reads no key)
      d.key_id = (const uint32_t*)v->kres[la_slot].p;
      k_key_resolve<<<d.B / 256 + (d.B % 256 != 0), 256, 0, v->ts>>>(d, (uint32_t*)v->kres[la_slot].p);
      DBG("k_key_resolve", v->ts);
    }
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
    if (resolve) {
      d.key_id = (const uint32_t*)v->kres[0].p;
      k_key_resolve<<<d.B / 256 + (d.B % 256 != 0), 256, 0, st>>>(d, (uint32_t*)v->kres[0].p);
      DBG("k_key_resolve", st);
    }
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

// the resolution of a self-keyed run alone, on any handle
int p2v_verifier_resolve_keys(p2v_verifier* v, const uint64_t* proofs, size_t n, uint32_t* key_ids, void* stream_, uint32_t flags) {
  if (!v || (!proofs && n) || (!key_ids && n)) return fail(P2V_E_ARG, "null argument");
  if (n > v->max_batch) return fail(P2V_E_ARG, "batch larger than max_batch");
  if (n == 0) return P2V_OK;
  HCK(hipSetDevice(v->device));
  hipStream_t st = (hipStream_t)stream_;
  DevCircuit d = v->dc;
  d.n = (int)n;
  d.tiled = (flags & P2V_FLAG_INPUT_TILED) ? 1 : 0;
  d.wstride = d.tiled ? 64 : 1;
  d.B = (int)((n + 63) / 64 * 64);
  d.soa = proofs;
  if (!(flags & P2V_FLAG_INPUT_DEVICE)) {
    const size_t words = (size_t)v->circ->c.L.words;
    HCK(input_buf(v));
    HCK(hipMemcpyAsync(v->in.p, proofs, (d.tiled ? p2v_tiled_words(n, words) : words * n) * 8, hipMemcpyHostToDevice, st));
    d.soa = (const uint64_t*)v->in.p;
  }
  const bool to_device = flags & P2V_FLAG_RESULT_DEVICE;
  // host ids stage through `kid`, as host-given ids do: only stream-ordered runs touch it, never a
  // lookahead run's resolver on v->ts (which writes kres[la_slot])
  uint32_t* dids = to_device ? key_ids : (uint32_t*)v->kid.p;
  k_key_resolve<<<d.B / 256 + (d.B % 256 != 0), 256, 0, st>>>(d, dids);
  if (v->debug_sync) {
    fprintf(stderr, "p2v: launched k_key_resolve\n"); fflush(stderr);
    HCK(hipStreamSynchronize(st)); HCK(hipGetLastError());
    fprintf(stderr, "p2v: finished k_key_resolve\n"); fflush(stderr);
  }
  HCK(hipGetLastError());
  if (!to_device) HCK(hipMemcpyAsync(key_ids, dids, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (!(flags & P2V_FLAG_NO_SYNC) || !to_device) HCK(hipStreamSynchronize(st));
  return P2V_OK;
}

int p2v_verifier_last_timings(const p2v_verifier* v, float* out, int max) {
  if (!v || !out) return 0;
  int k = 0;
  for (; k < kNumKernels && k < max; k++) out[k] = v->last_ms[k];
  return k;
}

}  // extern "C"
