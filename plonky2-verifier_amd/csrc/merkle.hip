// merkle.hip — the Merkle path kernels of the batch verifier (Hash/Merkle.hs:27-42).  Each step of
// a path (tree_path, the climb, the cap entry) is defined once per form: the lane form (one lane per
// path, the throughput permutation) and the row form (16 lanes per path, lposeidon.h).
//   k_merkle      path compression for the 4 initial trees and every FRI step tree, one lane per
//                 (proof, query, tree)
//   k_merkle_plan, k_merkle_cse, k_merkle_fix, k_merkle_resolve   the same, shared nodes hashed once
//   k_merkle_known, k_merkle_known_miss   tree 0 (the circuit's own) against the table of openings
//                 already found True; only the openings not in it are hashed
//   k_merkle_row  latency mode: every path in the row form
#include "leafhash.h"
#include "kernels.h"

using namespace p2d;

// ------------------------------------------------------------------------ packed words
// Entry word of the chain buckets (mchain), the fix list (mfix) and the miss list (kmiss, t = 0):
//   t << 27 | q << 22 | p    5-bit tree, 5-bit query (P2V_CSE_MAX_Q), 22-bit proof (P2V_CSE_MAX_B)
__device__ __forceinline__ uint32_t entry_pack(int t, int q, int p) { return (uint32_t)t << 27 | (uint32_t)q << 22 | (uint32_t)p; }
__device__ __forceinline__ void entry_unpack(uint32_t id, int& t, int& q, int& p) {
  t = (int)(id >> 27); q = (int)((id >> 22) & 31); p = (int)(id & 0x3FFFFFu);
}
// Plan word (mplan) of query q in a tree class: e | owner << 4 | same_leaf << 9 | root << 10
//   e: the levels q owns (4 bits, P2V_CSE_MAX_DEPTH), owner: the query it meets at level e,
//   same_leaf: that query opens the same leaf, root: the lowest query under q's cap entry
__device__ __forceinline__ uint32_t plan_pack(int e, int owner, bool same_leaf, int root) {
  return (uint32_t)e | (uint32_t)owner << 4 | (uint32_t)same_leaf << 9 | (uint32_t)root << 10;
}
__device__ __forceinline__ int plan_e(uint32_t pw) { return (int)(pw & 15); }
__device__ __forceinline__ int plan_owner(uint32_t pw) { return (int)((pw >> 4) & 31); }
__device__ __forceinline__ bool plan_same_leaf(uint32_t pw) { return (pw >> 9) & 1; }
__device__ __forceinline__ int plan_root(uint32_t pw) { return (int)((pw >> 10) & 31); }
// the status byte of (tree t, query q, proof p): mk_ok is [Q][T][B]
__device__ __forceinline__ uint8_t& mk_at(const DevCircuit& c, int t, int q, int p) { return c.mk_ok[(int64_t)(q * c.T + t) * c.B + p]; }

// ------------------------------------------------------------------------ Merkle paths
#ifndef P2V_MERKLE_WAVES
#define P2V_MERKLE_WAVES 6   // amdgpu_waves_per_eu on k_merkle: 77-79 VGPRs, 6 waves/SIMD, no scratch (serial +4.7 %, pipelined unchanged; 0 = compiler default, 5 waves)
#endif
#if P2V_MERKLE_WAVES > 0
#define P2V_MERKLE_ATTR __attribute__((amdgpu_waves_per_eu(P2V_MERKLE_WAVES)))
#else
#define P2V_MERKLE_ATTR
#endif
// Tree t of query q (lane proof p): path length, word offset of its siblings in the proof, and the
// query's leaf index in that tree (FRI step trees: the index shifted by the earlier arities)
__device__ __forceinline__ void tree_path(const DevCircuit& c, int t, int q, int p, int& depth, int64_t& poff, uint32_t& idx) {
  const int64_t base = c.q0 + (int64_t)q * c.qstride;
  idx = (uint32_t)chal(c, CH_QIDX(c) + q, p);
  if (t < 4) { depth = c.depth0; poff = base + c.path[t]; }
  else {
    const int s = t - 4;
    int sh = 0;
    for (int j = 0; j <= s; j++) sh += c.arity[j];
    idx >>= sh; depth = c.step_depth[s]; poff = base + c.step_path[s];
  }
}
__device__ __forceinline__ void load_leafdig(const DevCircuit& c, int t, int q, int p, uint64_t (&cur)[4]) {
  const uint64_t* src = c.leafdig + ((int64_t)(q * c.T + t) * 4) * c.B + p;
#pragma unroll
  for (int i = 0; i < 4; i++) cur[i] = src[(int64_t)i * c.B];
}
// Word i of entry ci of tree t's cap: tree 0's is the circuit's (a keyed run, wave-uniform: the
// lane's key), the others' are in the proof
__device__ __forceinline__ uint64_t cap_root(const DevCircuit& c, int t, uint32_t ci, int i, int p) {
  if (t == 0) return c.key_id ? lane_key(c, p)[ci * 4 + i] : c.cs_cap[ci * 4 + i];
  if (t == 1) return ld(c, c.wcap + ci * 4 + i, p);
  if (t == 2) return ld(c, c.zcap + ci * 4 + i, p);
  if (t == 3) return ld(c, c.qcap + ci * 4 + i, p);
  return ld(c, c.ccaps + (int64_t)(t - 4) * 4 * c.cap_len + ci * 4 + i, p);
}

// ---- lane form: one lane per path
// One level of a path (Hash/Merkle.hs:27-42): even index compress(cur, sib), odd compress(sib, cur)
// LEAD: permute_dev's (poseidon.h; false in k_merkle alone)
template <bool LEAD = true>
__device__ __forceinline__ void merkle_level(uint64_t (&cur)[4], const uint64_t (&sib)[4], bool odd) {
  uint64_t st[12];
#pragma unroll
  for (int i = 0; i < 4; i++) { st[i] = odd ? sib[i] : cur[i]; st[4 + i] = odd ? cur[i] : sib[i]; st[8 + i] = 0; }
  p2::permute_dev<true, LEAD>(st, true, 1);   // compress: words 8..11 enter as 0, only 0..3 are read
#pragma unroll
  for (int i = 0; i < 4; i++) cur[i] = st[i];
}
// Levels [l0, l1) from node cur at index idx (both left at level l1), the siblings at poff.
// node(l) runs between a level's sibling load and its compression (merkle_chain's check (B)).
struct NoNode { __device__ __forceinline__ void operator()(int) const {} };
template <class F = NoNode, bool LEAD = true>
__device__ __forceinline__ void lane_climb(const DevCircuit& c, int64_t poff, int l0, int l1, int p, uint64_t (&cur)[4], uint32_t& idx, F node = F{}) {
  for (int l = l0; l < l1; l++) {
    uint64_t sib[4];
    // one level's 32 B of siblings per load (proof-major: the line re-fetches this leaves hit
    // the Infinity Cache; tiled: whole 512-B rows per wave)
#pragma unroll
    for (int i = 0; i < 4; i++) sib[i] = ld(c, poff + 4 * l + i, p);
    node(l);
    merkle_level<LEAD>(cur, sib, idx & 1u);
    idx >>= 1;
  }
}
// cap_roots !! (idx >> depth) == the path's root
__device__ __forceinline__ bool cap_ok(const DevCircuit& c, int t, uint32_t idx, const uint64_t (&cur)[4], int p) {
  bool ok = idx < (uint32_t)c.cap_len;
  const uint32_t ci = ok ? idx : 0;
#pragma unroll
  for (int i = 0; i < 4; i++) ok = ok && (cap_root(c, t, ci, i, p) == cur[i]);
  return ok;
}

// ---- row form (lposeidon.h): 16 lanes per path, lanes 0..3 hold the node, lanes 4..7 the other
// half of the compression's input
// Levels [l0, depth) from node cur at index idx: the node at the top, idx left at that level
__device__ __forceinline__ uint64_t row_climb(const DevCircuit& c, int64_t poff, int l0, int depth, int p, const lp::Row& LR, const lp::TLdsL& TL,
                                              uint64_t cur, uint32_t& idx) {
  const int L = LR.L;
  for (int l = l0; l < depth; l++) {   // even index: compress(cur, sib), odd: compress(sib, cur)
    const uint64_t sib = L < 8 ? ld(c, poff + 4 * l + (L & 3), p) : 0;
    const uint64_t c0 = rp::get_word(cur, 0), c1 = rp::get_word(cur, 1), c2 = rp::get_word(cur, 2), c3 = rp::get_word(cur, 3);
    const uint64_t cb = L == 4 ? c0 : L == 5 ? c1 : L == 6 ? c2 : c3;
    const bool odd = idx & 1u;
    const uint64_t x = L < 4 ? (odd ? sib : cur) : L < 8 ? (odd ? cb : sib) : 0;
    cur = lp::permute(x, LR, TL);   // lanes 0..3: the compression's output
    idx >>= 1;
  }
  return cur;
}
// cap_ok for a row: the same in every lane of the row
__device__ __forceinline__ bool row_cap_ok(const DevCircuit& c, int t, uint32_t idx, uint64_t cur, int p, int L) {
  const bool ok = idx < (uint32_t)c.cap_len;
  const uint32_t ci = ok ? idx : 0;
  uint64_t root = 0;
  if (L < 4) root = cap_root(c, t, ci, L, p);
  const uint64_t eq = (L >= 4 || root == cur) ? 1 : 0;
  return ok && (rp::get_word(eq, 0) & rp::get_word(eq, 1) & rp::get_word(eq, 2) & rp::get_word(eq, 3));
}

// The whole path of (tree t, query q, proof p) against its cap entry
__device__ __forceinline__ bool path_ok(const DevCircuit& c, int t, int q, int p) {
  int depth; int64_t poff; uint32_t idx;
  tree_path(c, t, q, p, depth, poff, idx);
  uint64_t cur[4];
  load_leafdig(c, t, q, p, cur);
  lane_climb<NoNode, false>(c, poff, 0, depth, p, cur, idx);
  return cap_ok(c, t, idx, cur, p);
}
__device__ __forceinline__ void merkle_unit(const DevCircuit& c) {
  const int lane = threadIdx.x & 63;
  const int unit = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int NPB = c.B >> 6;
  if (unit >= c.Q * c.T * NPB) return;
  const int pb = unit % NPB, qt = unit / NPB;   // (position, query)-major: deepest paths first
  const int q = qt % c.Q, t = c.merkle_order[qt / c.Q];
  const int p = pb * 64 + lane;
  mk_at(c, t, q, p) = path_ok(c, t, q, p) ? 1 : 0;
}
extern "C" __global__ void __launch_bounds__(256) P2V_MERKLE_ATTR k_merkle(DevCircuit c) { merkle_unit(c); }

// ------------------------------------------------------------------------ Merkle paths, shared nodes once
// The Q queries of a proof open paths in the same trees, and two queries whose leaf indices agree
// above bit l hash the same parent at level l and everything above it: with 28 queries and cap 16
// a third of the top-level compressions repeat (13.4 % of all compressions of the standard proof).
// Each parent is hashed once, by its OWNER, the lowest query under it.  Query q owns the levels
// 0 .. e_q - 1 (a prefix: ownership only shrinks going up), so its work is one chain of e_q
// compressions; at level e_q < depth it meets its owner o (a lower query) and stops.
// Exact, whatever the proof holds.  q's reference path equals o's above level e_q when both
// compress the same pair there and read the same siblings above it, so for every follower q
//   (A) o's sibling at level e_q is q's node (same leaf, e_q = 0: the leaf digests are equal),
//   (B) q's sibling at level e_q is o's node (checked by o's chain, which knows its follower there),
//   (C) q's and o's siblings above level e_q are equal (same leaf: from level 0 on),
// and then q's status is o's.  A follower that fails a check is flagged and re-run from its own
// node at level e_q (k_merkle_fix), unless its root (the lowest query under its cap entry, whose
// chain is a whole path) failed: then k_status stops at that lower query whatever q's status is
// (Plonk/FRI.hs:105-117, queries in order).  Statuses and codes are the plain k_merkle's bit for
// bit; honest proofs fail no check.
//   k_merkle_plan     one lane per (tree class, query, proof): e, owner, followers, root; appends
//                     the chains to buckets by length, one global atomic per (work-group, bucket)
//                     (the 4 initial trees share the leaf index, each FRI step tree shifts it)
//   k_merkle_cse      one lane per chain, longest bucket first: waves of equal-length chains
//   k_merkle_fix      the flagged followers (a compact list; none for honest proofs)
//   k_merkle_resolve  one lane per (tree, query, proof): a follower takes the status of its
//                     first flagged or root ancestor
#define P2V_CSE_CSTRIDE 16   // counters 64 B apart: atomics on one line serialise
__device__ __forceinline__ void class_shape(const DevCircuit& c, int cls, int& sh, int& depth) {
  sh = 0; depth = c.depth0;
  if (cls > 0) { for (int j = 0; j < cls; j++) sh += c.arity[j]; depth = c.step_depth[cls - 1]; }
}
__device__ __forceinline__ int tree_class(int t) { return t < 4 ? 0 : t - 3; }
// the plan word of (tree t, query q, proof p): one per tree class
__device__ __forceinline__ int64_t plan_at(const DevCircuit& c, int t, int q, int p) { return ((int64_t)tree_class(t) * c.Q + q) * c.B + p; }
extern "C" __global__ void __launch_bounds__(64 * P2V_PLAN_WAVES) k_merkle_plan(DevCircuit c) {
  __shared__ int hist[P2V_CSE_MAX_DEPTH + 1], gbase[P2V_CSE_MAX_DEPTH + 1];
  const int lane = threadIdx.x & 63;
  const int unit = blockIdx.x * P2V_PLAN_WAVES + (threadIdx.x >> 6);
  const int NPB = c.B >> 6, ncls = 1 + c.S;
  const int nb = c.depth0 + 1;
  if (threadIdx.x < (unsigned)nb) hist[threadIdx.x] = 0;
  __syncthreads();
  const bool unit_live = unit < ncls * c.Q * NPB;   // wave-uniform
  const int pb = unit % NPB, cq = unit / NPB;
  const int q = cq % c.Q, cls = unit_live ? cq / c.Q : 0;
  const int p = pb * 64 + lane;
  const bool live = unit_live && p < c.n;
  int sh, depth;
  class_shape(c, cls, sh, depth);
  // class 0: the initial trees, without tree 0 in a run with known openings (kskip = 1: its
  // statuses are k_merkle_known's and k_merkle_known_miss's alone)
  const int ntr = cls == 0 ? 4 - c.kskip : 1, t0 = cls == 0 ? c.kskip : 3 + cls;
  int e = 0, loc = 0, cnt = 0;
  if (live) {
    const uint64_t* qi = c.chal + (int64_t)CH_QIDX(c) * c.B + p;
    const uint32_t me = (uint32_t)qi[(int64_t)q * c.B] >> sh;
    // b = bit length of (index xor other's index): the two paths first share a parent at level b - 1
    int minb = 64, owner = q, root = q;
    bool have_root = false;
    uint64_t fol = ~0ULL;
    for (int k0 = 0; k0 < c.Q; k0 += 4) {
      uint32_t ik[4];
#pragma unroll
      for (int u = 0; u < 4; u++) ik[u] = k0 + u < c.Q ? (uint32_t)qi[(int64_t)(k0 + u) * c.B] >> sh : me;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int k = k0 + u;
        if (k >= c.Q) break;
        const uint32_t x = me ^ ik[u];
        const int b = x ? 32 - __clz(x) : 0;
        if (!have_root && b <= depth) { root = k; have_root = true; }   // lowest query under the cap entry
        if (k < q) {
          if (b < minb) { minb = b; owner = k; }   // the lowest query sharing q's lowest shared parent
        } else if (k > q && b >= 1 && b <= depth) {
          // the lowest query in the sibling subtree at level b - 1 meets q there (if q owns that level)
          const int sl = 5 * (b - 1);
          if (((fol >> sl) & 31) == 31) fol ^= (uint64_t)(31 ^ k) << sl;
        }
      }
    }
    e = minb - 1 >= depth ? depth : (minb >= 1 ? minb - 1 : 0);
    if (e < depth) fol |= ~0ULL << (5 * e);   // levels q does not own: their owner checks the follower
    const int64_t pi = ((int64_t)cls * c.Q + q) * c.B + p;
    c.mplan[pi] = plan_pack(e, owner, minb == 0, root);
    c.mfol[pi] = fol;
    for (int tt = 0; tt < ntr; tt++) {
      c.mbadq[((int64_t)(t0 + tt) * c.Q + q) * c.B + p] = 0;
      mk_at(c, t0 + tt, q, p) = 0;   // written again by its chain, k_merkle_fix or k_merkle_resolve
    }
  }
  // the wave's lanes of one length: one run of that bucket, tree-major; a work-group's runs are
  // packed in LDS, then one global atomic per (work-group, bucket) places them
  uint64_t todo = __ballot(live);
  while (todo) {
    const int lead = __ffsll((unsigned long long)todo) - 1;
    const int eb = __shfl(e, lead);
    const uint64_t grp = __ballot(live && e == eb);
    const int n = __popcll(grp);
    int off = 0;
    if (lane == lead) off = atomicAdd(&hist[eb], n * ntr);
    off = __shfl(off, lead);
    if (live && e == eb) { loc = off + __popcll(grp & ((1ULL << lane) - 1)); cnt = n; }
    todo &= ~grp;
  }
  __syncthreads();
  if (threadIdx.x < (unsigned)nb) {
    const int h = hist[threadIdx.x];
    gbase[threadIdx.x] = h ? atomicAdd(&c.mcount[threadIdx.x * P2V_CSE_CSTRIDE], h) : 0;
  }
  __syncthreads();
  if (live) {
    uint32_t* dst = c.mchain + (int64_t)e * c.mcap;
    const int64_t base = (int64_t)gbase[e] + loc;
    for (int tt = 0; tt < ntr; tt++) {
      const int64_t pos = base + (int64_t)tt * cnt;
      if (pos < c.mcap) dst[pos] = entry_pack(t0 + tt, q, p);   // (always: T Q B slots)
    }
  }
}
// Set the re-run flag of (t, q, p); true for the one caller that set it first.  A follower can fail
// two checks, its owner's (B) and its own (A)/(C), so the flag is one bit set by an atomic OR on the
// flag byte's 32-bit word (the flag array is [T][Q][B], B a multiple of 64: the word is in bounds).
__device__ __forceinline__ bool cse_flag_once(const DevCircuit& c, int t, int q, int p) {
  const size_t at = ((size_t)t * c.Q + q) * c.B + p;
  uint32_t* w = (uint32_t*)(c.mbadq + (at & ~(size_t)3));
  const uint32_t bit = 1u << (8 * (at & 3));
  return !(atomicOr(w, bit) & bit);
}
// a follower to re-run from its own node (k_merkle_fix): flag + one list entry.  Each (t, q, p) is
// listed at most once, so the list (capacity T Q B) cannot overflow; the guard below is therefore
// unreachable, and fails safe: an entry that could not be listed is rejected, never left to a stale
// status (k_merkle_plan also clears every status byte of the run)
__device__ __forceinline__ void cse_flag(const DevCircuit& c, int t, int q, int p) {
  if (!cse_flag_once(c, t, q, p)) return;
  const int at = atomicAdd(c.mfixn, 1);
  if (at < c.mcap) c.mfix[at] = entry_pack(t, q, p);
  else mk_at(c, t, q, p) = 0;
}
// Which chains a wave of k_merkle_cse runs: bucket b (the chain length) and wave w of that bucket,
// bucket-major, longest first.  The 64 lanes of a wave are then runs of a few proofs from many
// 64-proof tiles, and the other proofs of every 128-B line they read sit in other buckets, read long
// after the line has left the XCD's L2: 6.6x the algorithmic bytes (profiles/r05z_pmc_traffic.json,
// VERDICT r5 item 1; the tile-merged order that addressed it measured slower: DESIGN.md "Retired
// build options").
__device__ __forceinline__ bool cse_wave(const DevCircuit& c, int& b, int64_t& w) {
  const int nbk = c.depth0 + 1;
  uint64_t nw[P2V_CSE_MAX_DEPTH + 1];
  uint64_t total = 0;
#pragma unroll
  for (int k = 0; k <= P2V_CSE_MAX_DEPTH; k++) {
    nw[k] = k < nbk ? ((uint64_t)min((int64_t)c.mcount[k * P2V_CSE_CSTRIDE], c.mcap) + 63) >> 6 : 0;
    total += nw[k];
  }
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  int64_t g = (int64_t)blockIdx.x * 4 + wv;
#pragma unroll
  for (int k = P2V_CSE_MAX_DEPTH; k >= 0; k--) {   // longest chains first
    if (g >= 0 && g < (int64_t)nw[k]) { b = k; w = g; }
    g -= (int64_t)nw[k];
  }
  return g < 0;
}
__device__ __forceinline__ void merkle_chain(const DevCircuit& c) {
  const int lane = threadIdx.x & 63;
  int b = -1;
  int64_t w = 0;
  if (!cse_wave(c, b, w)) return;
  const int64_t cnt = min((int64_t)c.mcount[b * P2V_CSE_CSTRIDE], c.mcap);
  const int64_t slot = w * 64 + lane;
  if (slot >= cnt) return;
  int t, q, p;
  entry_unpack(c.mchain[(int64_t)b * c.mcap + slot], t, q, p);
  const int64_t pi = plan_at(c, t, q, p);
  const uint32_t pw = c.mplan[pi];
  const uint64_t fol = c.mfol[pi];
  const int e = b;   // == plan_e(pw): the bucket is the chain length (wave-uniform)
  int depth; int64_t poff; uint32_t idx;
  tree_path(c, t, q, p, depth, poff, idx);
  uint64_t cur[4];
  load_leafdig(c, t, q, p, cur);
  lane_climb(c, poff, 0, e, p, cur, idx, [&](int l) __attribute__((always_inline)) {   // (a call would put the captures in scratch)
    const int f = (int)((fol >> (5 * l)) & 31);
    if (f != 31) {   // (B): the follower meeting this path here holds this node as its sibling
      const int64_t fo = poff + (int64_t)(f - q) * c.qstride + 4 * l;
      bool bad = false;
#pragma unroll
      for (int i = 0; i < 4; i++) bad |= ld(c, fo + i, p) != cur[i];
      if (bad) cse_flag(c, t, f, p);
    }
  });
  if (e == depth) {
    mk_at(c, t, q, p) = cap_ok(c, t, idx, cur, p) ? 1 : 0;
    return;
  }
  uint64_t* nd = c.mnode + ((int64_t)(t * c.Q + q) * 4) * c.B + p;   // k_merkle_fix resumes here
#pragma unroll
  for (int i = 0; i < 4; i++) nd[(int64_t)i * c.B] = cur[i];
  const int owner = plan_owner(pw);
  const int64_t oo = poff + (int64_t)(owner - q) * c.qstride;   // the owner's siblings in this tree
  bool bad = false;
  int l0 = e + 1;
  if (plan_same_leaf(pw)) {   // equal digests, and (C) from level 0
    uint64_t od[4];
    load_leafdig(c, t, owner, p, od);
#pragma unroll
    for (int i = 0; i < 4; i++) bad |= od[i] != cur[i];
    l0 = 0;
  } else {   // (A)
#pragma unroll
    for (int i = 0; i < 4; i++) bad |= ld(c, oo + 4 * e + i, p) != cur[i];
  }
  for (int l = l0; l < depth; l++)   // (C)
#pragma unroll
    for (int i = 0; i < 4; i++) bad |= ld(c, poff + 4 * l + i, p) != ld(c, oo + 4 * l + i, p);
  if (bad) cse_flag(c, t, q, p);
}
#ifndef P2V_CSE_WAVES
#define P2V_CSE_WAVES 5   // amdgpu_waves_per_eu on k_merkle_cse: 90 VGPRs, no spills; 6 (80 VGPRs, 40 B of spills
                          // outside the chain loop) measured 0.7-1.4 % slower pipelined (profiles/r05v_cse_waves.txt)
#endif
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(P2V_CSE_WAVES))) k_merkle_cse(DevCircuit c) { merkle_chain(c); }

// The frame of the two list kernels (k_merkle_fix, k_merkle_known_miss): n entries, read once, on
// the batch's critical path.  A short list (the usual one; none at all for honest proofs) runs in
// the row form of the permutation (lposeidon.h: 16 lanes per path, ~8.5 us per dependent
// compression against ~20 us for one lane), grid-stride over the list rows.  A list of more than
// LIST::LONG entries per block takes the lane form, one lane per entry: it then costs about one
// k_merkle, not list/rows passes of the latency form.  LIST: the threshold and the two forms of one
// entry, lane(c, k) and row(c, k, LR, TL).
template <class LIST>
__device__ __forceinline__ void list_entries(const DevCircuit& c, int64_t n) {
  __shared__ TLdsAny T;
  if (n > (int64_t)gridDim.x * LIST::LONG) {   // grid-uniform
    const int64_t lanes = (int64_t)gridDim.x * 256;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += lanes) LIST::lane(c, k);
    return;
  }
  if ((int64_t)blockIdx.x * 16 >= n) return;   // block-uniform: no entry for this block's rows (honest batches: all)
  tlds_fill_form(T, 16);
  __builtin_amdgcn_s_setprio(3);
  lp::Row LR;
  lp::init(LR, T.l, threadIdx.x);
  const int64_t rows = (int64_t)gridDim.x * 16;
  for (int64_t k = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4; k < n; k += rows) LIST::row(c, k, LR, T.l);   // row-uniform
}
// The flagged followers, each from its own node at its meeting level to its cap entry.  A long
// list: adversarial batches of garbage proofs flag about half of all paths.
struct FixList {
static constexpr int LONG = 16;   // more entries than latency rows
// entry k: its path from its meeting level e on; false when a lower query fails first (status 0)
static __device__ __forceinline__ bool entry(const DevCircuit& c, int64_t k, int& t, int& q, int& p, int& e, int& depth, int64_t& poff, uint32_t& idx) {
  entry_unpack(c.mfix[k], t, q, p);
  const uint32_t pw = c.mplan[plan_at(c, t, q, p)];
  if (!mk_at(c, t, plan_root(pw), p)) return false;
  e = plan_e(pw);
  tree_path(c, t, q, p, depth, poff, idx);
  idx >>= e;
  return true;
}
static __device__ __forceinline__ void lane(const DevCircuit& c, int64_t k) {
  int t, q, p, e, depth; int64_t poff; uint32_t idx;
  if (!entry(c, k, t, q, p, e, depth, poff, idx)) { mk_at(c, t, q, p) = 0; return; }
  uint64_t cur[4];
  const uint64_t* nd = c.mnode + ((int64_t)(t * c.Q + q) * 4) * c.B + p;
#pragma unroll
  for (int i = 0; i < 4; i++) cur[i] = nd[(int64_t)i * c.B];
  lane_climb(c, poff, e, depth, p, cur, idx);
  mk_at(c, t, q, p) = cap_ok(c, t, idx, cur, p) ? 1 : 0;
}
static __device__ __forceinline__ void row(const DevCircuit& c, int64_t k, const lp::Row& LR, const lp::TLdsL& TL) {
  const int L = LR.L;
  int t, q, p, e, depth; int64_t poff; uint32_t idx;
  if (!entry(c, k, t, q, p, e, depth, poff, idx)) {
    if (L == 0) mk_at(c, t, q, p) = 0;
    return;
  }
  uint64_t cur = L < 4 ? c.mnode[((int64_t)(t * c.Q + q) * 4 + L) * c.B + p] : 0;
  cur = row_climb(c, poff, e, depth, p, LR, TL, cur, idx);
  const bool ok = row_cap_ok(c, t, idx, cur, p, L);
  if (L == 0) mk_at(c, t, q, p) = ok ? 1 : 0;
}
};
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) k_merkle_fix(DevCircuit c) {
  list_entries<FixList>(c, min((int64_t)*c.mfixn, c.mcap));
}
extern "C" __global__ void __launch_bounds__(256) k_merkle_resolve(DevCircuit c) {
  if (blockIdx.x == 0 && threadIdx.x <= (unsigned)c.depth0) c.mcount[threadIdx.x * P2V_CSE_CSTRIDE] = 0;   // the next run's
  if (blockIdx.x == 0 && threadIdx.x == 0) *c.mfixn = 0;
  const int lane = threadIdx.x & 63;
  const int unit = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int NPB = c.B >> 6;
  if (unit >= c.Q * (c.T - c.kskip) * NPB) return;
  const int pb = unit % NPB, qt = unit / NPB;
  const int q = qt % c.Q, t = qt / c.Q + c.kskip;   // (known openings: trees 1 .. T - 1)
  const int p = pb * 64 + lane;
  if (p >= c.n) return;
  const int cls = tree_class(t);
  int sh, depth;
  class_shape(c, cls, sh, depth);
  const uint32_t* plan = c.mplan + (int64_t)cls * c.Q * c.B + p;
  const uint8_t* badq = c.mbadq + (int64_t)t * c.Q * c.B + p;
  uint32_t pw = plan[(int64_t)q * c.B];
  if (plan_e(pw) == depth || badq[(int64_t)q * c.B]) return;   // a root or a re-run follower: written
  // the first ancestor whose status is its own: a root chain or a re-run follower
  int a = plan_owner(pw);
  for (int hop = 0; hop < c.Q; hop++) {
    pw = plan[(int64_t)a * c.B];
    if (plan_e(pw) == depth || badq[(int64_t)a * c.B]) break;
    a = plan_owner(pw);
  }
  uint8_t* mk = c.mk_ok + (int64_t)t * c.B + p;   // not mk_at: two of its addresses cost this kernel's register count
  const int64_t qs = (int64_t)c.T * c.B;
  mk[q * qs] = mk[a * qs];
}

// ------------------------------------------------------------------------ known openings of tree 0
// Tree 0 (constants/sigmas) belongs to the circuit, not to the proof: its cap is in the verifier
// key (Plonk/FRI.hs:105-117), so the leaf and the sibling path opened at index idx are the same
// words in every honest proof of the circuit.  The Merkle check is a pure function of (cap, idx,
// leaf words, sibling words) and the cap is fixed per circuit, so an input that evaluated to True
// once is True for ever: the circuit keeps, per device, a table direct-mapped by idx of inputs that
// the full computation below found True, and an opening whose kwords words equal row idx word for
// word is accepted without hashing.  Exact memoisation: nothing is assumed of the hash, and an
// opening that differs from the row in one word (or meets an empty row) takes the reference
// computation.  Runs above the latency mode with shared-node paths only (api_run.cpp).
// Keys.  A key fixes the cap, so the argument holds per key: the table of a handle with a key table
// has one block of 2^lde_bits rows per key, row (k, idx) at (int64)k << lde_bits | idx, key 0's block
// first (an unkeyed run and a keyed opening with id 0 share it).  The id is clamped to nkeys - 1 as
// lane_key() clamps it: what an out-of-range id teaches the table is a true statement about the
// last key (k_status still answers P2V_ERR_CIRCUIT for that proof).  The miss kernel reads an
// entry's id ONCE and takes both the cap entry it compares against and the row it claims and
// writes from that one value, so an opening proved under key A cannot land in key B's rows even
// if the id array changed under the run.  c.key_id is a kernel argument: the test is wave-uniform,
// and an unkeyed run takes the scalar cs_cap operands and row idx it always did.
//   k_merkle_known       16 lanes per (query, proof): flag, then the row against the proof's
//                        words; loads and compares only.  Hit: mk_ok = 1.  Miss: listed
//   k_merkle_known_miss  the listed openings in full (leaf sponge, path, cap entry); a True one is
//                        inserted (kmode 1)
// Ordering.  A row goes EMPTY -> BUSY -> VALID once and is never written again: the lane group
// whose compare-and-swap took it from EMPTY writes the words, fences at device scope, and stores
// VALID with release at agent scope; a reader loads the flag with acquire at agent scope before it
// reads a word.  So a reader that sees VALID sees the final words, and every other view (EMPTY,
// BUSY, a flag that some lanes of the group see later than others) is a miss: a stale or torn view
// can only cost the computation, never accept an opening.  Runs of other workspaces on other
// streams read and fill the same table concurrently under the same rule.
// The key of lane p's proof: its id clamped as lane_key() clamps it, 0 in an unkeyed run.  One load
// that the compiler may not repeat (see "Keys" above).
__device__ __forceinline__ uint32_t known_key(const DevCircuit& c, int p) {
  if (!c.key_id) return 0;
  return min(__hip_atomic_load(c.key_id + min(p, c.n - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), (uint32_t)(c.nkeys - 1));
}
__device__ __forceinline__ int64_t known_row(const DevCircuit& c, uint32_t k, uint32_t idx) { return (int64_t)k << c.lde_bits | idx; }
// cap_root / cap_ok / row_cap_ok of tree 0 under key k (from known_key), not under whatever the id
// array holds by now
__device__ __forceinline__ uint64_t key_cap_root(const DevCircuit& c, uint32_t k, uint32_t ci, int i) {
  return c.key_id ? c.keys[(int64_t)k * (4 * c.cap_len + 4) + ci * 4 + i] : c.cs_cap[ci * 4 + i];
}
__device__ __forceinline__ bool key_cap_ok(const DevCircuit& c, uint32_t k, uint32_t idx, const uint64_t (&cur)[4]) {
  bool ok = idx < (uint32_t)c.cap_len;
  const uint32_t ci = ok ? idx : 0;
#pragma unroll
  for (int i = 0; i < 4; i++) ok = ok && (key_cap_root(c, k, ci, i) == cur[i]);
  return ok;
}
__device__ __forceinline__ bool key_row_cap_ok(const DevCircuit& c, uint32_t k, uint32_t idx, uint64_t cur, int L) {
  const bool ok = idx < (uint32_t)c.cap_len;
  const uint32_t ci = ok ? idx : 0;
  uint64_t root = 0;
  if (L < 4) root = key_cap_root(c, k, ci, L);
  const uint64_t eq = (L >= 4 || root == cur) ? 1 : 0;
  return ok && (rp::get_word(eq, 0) & rp::get_word(eq, 1) & rp::get_word(eq, 2) & rp::get_word(eq, 3));
}
extern "C" __global__ void __launch_bounds__(256) k_merkle_known(DevCircuit c) {
  const int lane = threadIdx.x & 63, L = threadIdx.x & 15;
  const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;   // the opening: proofs fastest
  const bool live = g < (int64_t)c.Q * c.n;
  const int64_t gg = live ? g : 0;
  const int p = (int)(gg % c.n), q = (int)(gg / c.n);
  const uint32_t idx = (uint32_t)chal(c, CH_QIDX(c) + q, p);   // < 2^lde_bits: masked by the transcript
  const int64_t r = known_row(c, known_key(c, p), idx);   // the row of (the lane's key, idx)
  const int64_t base = c.q0 + (int64_t)q * c.qstride;
  const int lw = c.lwidth[0];
  bool bad = !live;
  if (live) {
    bad = __hip_atomic_load(c.kvalid + r, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != P2V_KNOWN_VALID;
    if (!bad) {
      const uint64_t* row = c.krows + r * c.kwords;   // lane L: words L, L + 16, ...: 128-B reads of the row
#pragma unroll 3
      for (int j = L; j < c.kwords; j += 16)
        bad |= row[j] != ld(c, j < lw ? base + c.leaf[0] + j : base + c.path[0] + (j - lw), p);
    }
  }
  const bool miss = live && ((__ballot(bad) >> (lane & 48)) & 0xFFFFu) != 0;   // any lane of the group
  // the wave's misses are adjacent in the list (a dense list stays in proof order): one atomic per wave
  const uint64_t mm = __ballot(miss && L == 0);
  bool listed = false;
  if (mm) {
    int at = 0;
    if (lane == 0) at = atomicAdd(c.kmissn, __popcll(mm));
    at = __shfl(at, 0);
    const int64_t pos = (int64_t)at + __popcll(mm & ((1ULL << lane) - 1));
    listed = pos < (int64_t)c.Q * c.B;   // (always: one entry per opening of the run)
    if (miss && L == 0 && listed) c.kmiss[pos] = entry_pack(0, q, p);
  }
  // a miss is k_merkle_known_miss's to decide; one that could not be listed is rejected
  if (live && L == 0 && (!miss || !listed)) mk_at(c, 0, q, p) = miss ? 0 : 1;
}
// row r (known_row of the key the opening was proved under) of a True opening: by the one group
// (or lane, nl = 1) that takes it from EMPTY
__device__ __forceinline__ void known_insert(const DevCircuit& c, int64_t r, int q, int p, int L, int nl, bool mine) {
  const int64_t base = c.q0 + (int64_t)q * c.qstride;
  const int lw = c.lwidth[0];
  if (mine) {
    uint64_t* row = c.krows + r * c.kwords;
    for (int j = L; j < c.kwords; j += nl) row[j] = ld(c, j < lw ? base + c.leaf[0] + j : base + c.path[0] + (j - lw), p);
  }
  // each lane's words are complete at device scope after its own fence; the group's lanes then
  // report through a ballot, and lane 0 stores the flag only on every lane's report, so the flag
  // store depends on all the group's fences, not on the wave's lanes running in step (see
  // "Ordering" above)
  __threadfence();
  const int lane = threadIdx.x & 63;
  const uint64_t grp = nl == 1 ? 1ULL << lane : 0xFFFFULL << (lane & 48);
  const uint64_t done = __ballot(mine);
  if (mine && L == 0 && (done & grp) == grp) {
    __hip_atomic_store(c.kvalid + r, P2V_KNOWN_VALID, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    atomicAdd(c.kstat + 2, 1ULL);
  }
}
struct MissList {
static constexpr int LONG = 64;   // more than 4 passes of the latency rows
// one listed opening in the lane form: the reference computation as k_phase1's leaf unit and
// k_merkle's path run it
static __device__ __forceinline__ void lane(const DevCircuit& c, int64_t k) {
  int t, q, p;
  entry_unpack(c.kmiss[k], t, q, p);   // t == 0
  const int64_t base = c.q0 + (int64_t)q * c.qstride;
  const uint32_t idx0 = (uint32_t)chal(c, CH_QIDX(c) + q, p);
  const uint32_t kk = known_key(c, p);   // read once: the cap below and the row are this key's
  uint64_t st[12];
  leaf_sponge(c, base + c.leaf[0], c.lwidth[0], p, st);
  uint64_t cur[4] = {st[0], st[1], st[2], st[3]};
  uint32_t idx = idx0;
  lane_climb(c, base + c.path[0], 0, c.depth0, p, cur, idx);
  const bool ok = key_cap_ok(c, kk, idx, cur);
  mk_at(c, 0, q, p) = ok ? 1 : 0;
  const int64_t r = known_row(c, kk, idx0);
  const bool mine = ok && c.kmode == 1 && atomicCAS(c.kvalid + r, P2V_KNOWN_EMPTY, P2V_KNOWN_BUSY) == P2V_KNOWN_EMPTY;
  known_insert(c, r, q, p, 0, 1, mine);
}
static __device__ __forceinline__ void row(const DevCircuit& c, int64_t k, const lp::Row& LR, const lp::TLdsL& TL) {
  const int L = LR.L;
  const int lw = c.lwidth[0];
  int t, q, p;
  entry_unpack(c.kmiss[k], t, q, p);   // t == 0
  const int64_t base = c.q0 + (int64_t)q * c.qstride;
  const uint32_t idx0 = (uint32_t)chal(c, CH_QIDX(c) + q, p);
  // read once, and lane 0's value in all 16 lanes: the cap below and the row are this key's
  const uint32_t kk = c.key_id ? (uint32_t)rp::get_word((uint64_t)known_key(c, p), 0) : 0u;
  // the leaf sponge (Hash/Sponge.hs:26-31; overwrite mode, no padding): lane L < 8 takes word
  // i + L of each block, the other state words stay
  uint64_t x = 0;
  for (int i = 0; i < lw; i += 8) {
    if (L < 8 && i + L < lw) x = ld(c, base + c.leaf[0] + i + L, p);
    x = lp::permute(x, LR, TL);
  }
  uint32_t idx = idx0;
  const uint64_t cur = row_climb(c, base + c.path[0], 0, c.depth0, p, LR, TL, L < 4 ? x : 0, idx);
  const bool ok = key_row_cap_ok(c, kk, idx, cur, L);
  if (L == 0) mk_at(c, 0, q, p) = ok ? 1 : 0;
  if (ok && c.kmode == 1) {   // row-uniform
    const int64_t r = known_row(c, kk, idx0);
    uint32_t old = P2V_KNOWN_VALID;
    if (L == 0) old = atomicCAS(c.kvalid + r, P2V_KNOWN_EMPTY, P2V_KNOWN_BUSY);
    old = (uint32_t)rp::get_word((uint64_t)old, 0);
    known_insert(c, r, q, p, L, 16, old == P2V_KNOWN_EMPTY);
  }
}
};
// Like k_merkle_fix: the row form for a short list (the usual one: the few openings of a warm batch
// that are new or wrong), the lane form for a long one (a cold table, a batch of garbage)
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) k_merkle_known_miss(DevCircuit c) {
  const int64_t nmiss = min((int64_t)*c.kmissn, (int64_t)c.Q * c.B);
  if (blockIdx.x == 0 && threadIdx.x == 0) {   // every opening of the run was probed once
    atomicAdd(c.kstat, (unsigned long long)((int64_t)c.Q * c.n - nmiss));
    atomicAdd(c.kstat + 1, (unsigned long long)nmiss);
  }
  list_entries<MissList>(c, nmiss);
}

// Latency mode (small batches, api_run.cpp): the same paths in the row form of the permutation
// (lposeidon.h: 16 lanes per path, lane L < 12 holding word L), four paths per wave.  A path is a
// chain of dependent compressions; one lane per path issues at the single-wave latency (~53 us
// per compression, lat.hip), the row form at ~14 us.  Row = path (tree position, query, proof),
// proofs fastest.
extern "C" __global__ void __launch_bounds__(256) k_merkle_row(DevCircuit c) {
  __shared__ TLdsAny T;
  tlds_fill_form(T, 16);
  __builtin_amdgcn_s_setprio(3);   // the batch's critical path in this mode
  lp::Row LR;
  lp::init(LR, T.l, threadIdx.x);
  const int L = LR.L;
  const int path = (int)((blockIdx.x * 256 + threadIdx.x) >> 4);
  const int npaths = c.Q * c.T * c.n;
  const bool live = path < npaths;   // idle rows still run the permutation (its DPP ops span the row)
  const int pp = live ? path : 0;
  const int p = pp % c.n, qt = pp / c.n;
  const int q = qt % c.Q, t = c.merkle_order[qt / c.Q];
  int depth; int64_t poff; uint32_t idx;
  tree_path(c, t, q, p, depth, poff, idx);
  uint64_t cur = L < 4 ? c.leafdig[((int64_t)(q * c.T + t) * 4 + L) * c.B + p] : 0;
  cur = row_climb(c, poff, 0, depth, p, LR, T.l, cur, idx);
  const bool ok = row_cap_ok(c, t, idx, cur, p, L);
  if (live && L == 0) mk_at(c, t, q, p) = ok ? 1 : 0;
}
