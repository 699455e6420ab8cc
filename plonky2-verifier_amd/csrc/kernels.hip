// kernels.hip — gfx950 kernels of the batch verifier: phase 1 (transcripts and leaf hashing).  The
// Merkle path kernels live in merkle.hip, the vanishing / gate-constraint kernels in vanish*.hip,
// the FRI queries and the status in fri.hip, the self-tests in selftest.hip.
//
// Data layout: the caller's proof-major batch ([n][words]) is read in place (devcommon.h ld()).
// In every kernel lane i of a wave handles proof (64*pb + i) and all other indices (query, tree,
// step, word) are wave-uniform: control flow never diverges and the Poseidon round constants are
// scalar operands.
//
//   k_phase1      transcript waves (a row or quad of lanes per proof, ~115 sequential permutations,
//                 Challenge/Verifier.hs:58-103 + Challenge/FRI.hs:65-104) run in the SAME
//                 launch as the leaf-hash waves (one lane per (proof, query, tree) sponge,
//                 Hash/Sponge.hs:26-31) which do not depend on the challenges
#include "leafhash.h"
#include "kernels.h"

using namespace p2d;
using gl::E;

// ------------------------------------------------------------------------ helpers
__device__ __forceinline__ void leaf_hash_unit(const DevCircuit& c, int unit, int lane) {
  const int NPB = c.B >> 6;
  const int pb = unit % NPB, qt = unit / NPB;   // (position, query)-major: costly trees first
  const int q = qt % c.Q, t = c.leaf_order[qt / c.Q];   // (a run with known openings: the order without tree 0)
  const int p = pb * 64 + lane;
  const int64_t base = c.q0 + (int64_t)q * c.qstride;
  int64_t off; int len;
  if (t < 4) { off = base + c.leaf[t]; len = c.lwidth[t]; }
  else { int s = t - 4; off = base + c.step_evals[s]; len = 2 << c.arity[s]; }
  uint64_t st[12];
  leaf_sponge(c, off, len, p, st);
  uint64_t* dst = c.leafdig + ((int64_t)(q * c.T + t) * 4) * c.B + p;
#pragma unroll
  for (int i = 0; i < 4; i++) dst[(int64_t)i * c.B] = st[i];
}

// The transcript (Challenge/Verifier.hs:58-103, Challenge/FRI.hs:65-104) is a fixed
// sequence of absorbs and squeezes for a given circuit; the host compiles it into an op
// program and one interpreter (transcript() below) runs it for each of the three lane layouts
// of a proof's duplex state (the forms below).  The ~115 permutations form a strictly serial
// chain, so per-permutation latency, not throughput, is what counts until the batch's leaf
// hashing outlasts the chain.
//
// the row form's fold of the reduced openings: DPP row rotations (rposeidon.h)
template <int D>
__device__ __forceinline__ uint64_t row_up(uint64_t v, bool plus) {   // value of lane L + D (mod 16)
  const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  const uint32_t l = plus ? rp::ror32<D>(lo) : rp::ror32<16 - D>(lo);
  const uint32_t h = plus ? rp::ror32<D>(hi) : rp::ror32<16 - D>(hi);
  return ((uint64_t)h << 32) | l;
}
template <int D>
__device__ __forceinline__ E row_fold(E h, E ad, bool plus) {   // h_L + alpha^D h_{L+D}
  return gl::eadd(h, gl::emul(ad, E{row_up<D>(h.a, plus), row_up<D>(h.b, plus)}));
}

// sum_m y_{S m + lane} * as^m over the F^2 openings at `off` (n of them), Horner from the top;
// eight terms' loads are issued ahead of their multiply-adds so the HBM latency overlaps the chain
template <int S>
__device__ __forceinline__ E horner_strided(const DevCircuit& c, int64_t off, int64_t n, int lane, int p, E as) {
  const int64_t M = (n + S - 1) / S;
  E h = gl::e0();
  for (int64_t m0 = M - 1; m0 >= 0; m0 -= 8) {
    E ys[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int64_t i = S * (m0 - u) + lane;
      ys[u] = (m0 - u >= 0 && i < n) ? lde(c, off + 2 * i, p) : gl::e0();
    }
#pragma unroll
    for (int u = 0; u < 8; u++)
      if (m0 - u >= 0) h = gl::eadd(gl::emul(h, as), ys[u]);
  }
  return h;
}

// The three lane layouts of a proof's duplex state.  A form says how many lanes share a proof
// (2^LOG; lane t of them owns the W state words W t .. W t + W - 1, so t == 0 holds word 0 and
// writes the challenges), how the state is permuted, how a word (wave-uniform position) reaches
// every lane, and how the lanes' partial sums of the reduced openings fold into lane 0.  The flags
// keep each form's load shapes, which is what keeps k_phase1 at 128 VGPRs without scratch:
//   LOAD_FIRST  an absorbed chunk's loads are issued before the pending permutation, so their
//               latency hides under it (else after it: no registers held across it)
//   CLAMP       a lane loads from a clamped address and selects (else loads only what it owns)
//   SUMS_FIRST  both reduced-opening sums are formed before either is folded

// Row form: lposeidon.h (LDS exchange, merged partial blocks, chain rows on the idle lanes: 6.6-6.8
// us per dependent permutation, profiles/r06p_row_par.txt); lanes 12..15 own no word.  The ~115
// permutations form a strictly serial chain, so this form has the lowest latency.
struct RowForm {
  static constexpr int W = 1, LOG = 4;
  static constexpr bool LOAD_FIRST = true, CLAMP = false, SUMS_FIRST = false;
  const lp::Row& LR;
  const lp::TLdsL& TL;
  const int t;
  const bool plus;   // the row rotation's direction, for the fold (rposeidon.h)
  __device__ __forceinline__ RowForm(const lp::Row& lr, const lp::TLdsL& tl) : LR(lr), TL(tl), t(lr.L), plus(rp::ror_plus(lr.L)) {}
  __device__ __forceinline__ void permute(uint64_t (&x)[1]) const { x[0] = lp::permute(x[0], LR, TL); }
  __device__ __forceinline__ uint64_t get_word(const uint64_t (&x)[1], int pos) const { return rp::get_word(x[0], pos); }
  // a block of public inputs (k left, from proof word a) into the rate positions
  __device__ __forceinline__ void load_pis(const DevCircuit& c, int p, int64_t a, int k, uint64_t (&x)[1]) const {
    if (t < 8 && t < k) x[0] = ld(c, a + t, p);
  }
  __device__ __forceinline__ E fold(E h, const E (&ap)[5]) const {   // a 4-level DPP tree: sum_t alpha^t H_t in lane 0
    h = row_fold<1>(h, ap[0], plus);
    h = row_fold<2>(h, ap[1], plus);
    h = row_fold<4>(h, ap[2], plus);
    return row_fold<8>(h, ap[3], plus);
  }
};

// Quad form (qposeidon.h): higher per-permutation latency than the row form but ~2.3x fewer issue
// slots in total, which is what matters once the batch is large enough that the transcript hides
// behind the leaf hashing sharing its launch (the host picks the form, see api_run.cpp).
struct QuadForm {
  static constexpr int W = 3, LOG = 2;
  static constexpr bool LOAD_FIRST = true, CLAMP = true, SUMS_FIRST = true;
  const int t;
  const qp::TLds& T;
  __device__ __forceinline__ void permute(uint64_t (&x)[3]) const { qp::permute(x, t, T); }
  __device__ __forceinline__ uint64_t get_word(const uint64_t (&x)[3], int pos) const { return qp::get_word(x, pos); }
  __device__ __forceinline__ void load_pis(const DevCircuit& c, int p, int64_t a, int k, uint64_t (&x)[3]) const {
    for (int j = 0; j < 8 && j < k; j++) qp::set_word(x, t, j, ld(c, a + j, p));
  }
  __device__ __forceinline__ E fold(E h, const E (&ap)[3]) const {
    const E alpha = ap[0];
    E h1{qp::bcast64(h.a, 1), qp::bcast64(h.b, 1)};
    E h2{qp::bcast64(h.a, 2), qp::bcast64(h.b, 2)};
    E h3{qp::bcast64(h.a, 3), qp::bcast64(h.b, 3)};
    E h0{qp::bcast64(h.a, 0), qp::bcast64(h.b, 0)};
    return gl::eadd(h0, gl::emul(alpha, gl::eadd(h1, gl::emul(alpha, gl::eadd(h2, gl::emul(alpha, h3))))));
  }
};

// Lane form: the whole state in one lane's registers, the throughput permutation.  About half of
// the quad form's VALU instructions per proof (85.9 M against 169.4 M per 4096 proofs, DESIGN.md
// §7.0), but a chain ~3.5x longer (a lone wave issues its dependent permutation at its own
// latency): for launches whose leaf hashing outlasts it (api_run.cpp, P2V_TRANSCRIPT=lane).
struct LaneForm {
  static constexpr int W = 12, LOG = 0;
  static constexpr bool LOAD_FIRST = false, CLAMP = false, SUMS_FIRST = false;
  static constexpr int t = 0;
  __device__ __forceinline__ void permute(uint64_t (&x)[12]) const { p2::permute_dev<false>(x); }
  __device__ __forceinline__ void load_pis(const DevCircuit& c, int p, int64_t a, int k, uint64_t (&x)[12]) const {
#pragma unroll
    for (int j = 0; j < 8; j++) if (j < k) x[j] = ld(c, a + j, p);
  }
  __device__ __forceinline__ uint64_t get_word(const uint64_t (&x)[12], int pos) const {
    switch (pos) {   // uniform: a switch, not a dynamically indexed (scratch) array
      case 0: return x[0];
      case 1: return x[1];
      case 2: return x[2];
      case 3: return x[3];
      case 4: return x[4];
      case 5: return x[5];
      case 6: return x[6];
      default: return x[7];
    }
  }
  __device__ __forceinline__ E fold(E h, const E (&)[1]) const { return h; }
};

// The interpreter, written once for the three forms: ONE permutation call site per duplex rule.
// KEYED (a parameter of the launch, api_run.cpp): the digest is the lane's key's (devcommon.h
// lane_key()), placed into the empty sponge before the op loop -- the program's first op is always
// the digest absorb (api_workspace.cpp transcript_ops), 4 words into rate positions 0..3 of a zero state --
// so it holds no register beyond the state's.  The unkeyed kernels keep the digest as a scalar
// operand of the interpreter, and their registers.
template <bool KEYED, class F>
__device__ __forceinline__ void transcript(const DevCircuit& c, int p, const F& f) {
  const bool leader = f.t == 0;
  constexpr int RW = F::W < 8 ? F::W : 8;   // a lane's words that can be rate positions
  uint64_t x[F::W];
#pragma unroll
  for (int i = 0; i < F::W; i++) x[i] = 0;
  for (int i = 0; i < c.num_pis; i += 8) {   // public inputs hash, Hash/Sponge.hs:26-31 (sponge [] = zero digest)
    f.load_pis(c, p, c.pis + i, c.num_pis - i, x);
    f.permute(x);
  }
  uint64_t pih[4];
#pragma unroll
  for (int w = 0; w < 4; w++) {
    pih[w] = f.get_word(x, w);
    if (leader) chal(c, CH_PI(c) + w, p) = pih[w];
  }
#pragma unroll
  for (int i = 0; i < F::W; i++) x[i] = 0;
  int nbuf = 0, outpos = -1;
  bool absorbing = true;
  const uint64_t qmask = (1ULL << c.lde_bits) - 1;
  uint64_t fa0 = 0, fa1 = 0;   // FRI alpha, kept in registers for the reduced openings below
  if constexpr (KEYED) {
    // one address per lane and constant offsets from it: a lane's words past position 3 read on
    // into the table (at most 6 words past the key: the table ends in 8 words of padding, dev.h)
    // and are dropped by the select
    const int first = F::W * f.t < 4 ? F::W * f.t : 4;
    const uint64_t* kd = lane_key(c, p) + 4 * c.cap_len + first;
#pragma unroll
    for (int j = 0; j < RW; j++) {
      const uint64_t u = kd[j];
      x[j] = first + j < 4 ? u : 0;
    }
    nbuf = 4;
  }
  for (int o = KEYED ? 1 : 0; o < c.ntops; o++) {
    const int type = c.tops[3 * o], a = c.tops[3 * o + 1], n = c.tops[3 * o + 2];
    if (type == TOP_COPY) {   // mkLookupDeltaList (betas ++ gammas ++ ...), Challenge/Verifier.hs:36-40,82-86
      if (leader) for (int k = 0; k < n; k++) chal(c, a + k, p) = chal(c, a - 3 * c.r + k, p);
      continue;
    }
    if (type == TOP_ZERO) {
      if (leader) for (int k = 0; k < n; k++) chal(c, a + k, p) = 0;
      continue;
    }
    if (type <= TOP_ABSORB_DIGEST) {   // absorb n words, chunk by chunk (lazy duplex, Challenge/Pure.hs:38-69)
      if (!absorbing) { absorbing = true; nbuf = 0; }
      for (int k = 0; k < n;) {
        const int start = nbuf == 8 ? 0 : nbuf;
        const int take = (8 - start) < (n - k) ? (8 - start) : (n - k);
        // word k + pos - start of the source replaces rate position pos, start <= pos < start + take;
        // before that the pending permutation of a full block (overwrite mode: the rate part is replaced)
        const bool full = nbuf == 8;
        if (full && !F::LOAD_FIRST) f.permute(x);
        uint64_t v[RW];
        bool mine[RW];
#pragma unroll
        for (int j = 0; j < RW; j++) {
          const int pos = F::W * f.t + j, w = k + pos - start;
          mine[j] = pos >= start && pos < start + take;
          v[j] = 0;
          if (type == TOP_ABSORB_SOA) {
            if constexpr (F::CLAMP) { const uint64_t u = ld(c, (int64_t)a + (mine[j] ? w : 0), p); v[j] = mine[j] ? u : 0; }
            else { if (mine[j]) v[j] = ld(c, (int64_t)a + w, p); }
          } else if (type == TOP_ABSORB_PIH) { const int q = w & 3; v[j] = q == 0 ? pih[0] : q == 1 ? pih[1] : q == 2 ? pih[2] : pih[3]; }
          else if constexpr (!KEYED) v[j] = c.digest[w & 3];
        }
        if (full && F::LOAD_FIRST) f.permute(x);
#pragma unroll
        for (int j = 0; j < RW; j++) x[j] = mine[j] ? v[j] : x[j];   // selects, not divergent stores: x stays in registers
        nbuf = start + take;
        k += take;
      }
      continue;
    }
    for (int k = 0; k < n; k++) {   // squeeze: output order state[7], state[6], ... (reverse of take 8)
      if (absorbing || outpos < 0) { f.permute(x); absorbing = false; outpos = 7; }   // duplex / re-permute
      uint64_t w = f.get_word(x, outpos);
      outpos--;
      if (type == TOP_SQUEEZE_IDX) w &= qmask;
      if (a + k == CH_FRI_ALPHA(c)) fa0 = w;
      if (a + k == CH_FRI_ALPHA(c) + 1) fa1 = w;
      if (leader) chal(c, a + k, p) = w;
    }
  }
  // precomputeReducedOpenings, Plonk/FRI.hs:128-134: Y = sum alpha^i y_i.  Lane t of the S = 2^LOG
  // lanes sums the terms i = t (mod S) in powers of alpha^S (Horner from the top), then the form
  // folds Y = sum_t alpha^t H_t into lane 0.  ap[s] = alpha^(2^s)
  E ap[F::LOG + 1] = {E{fa0, fa1}};
#pragma unroll
  for (int s = 1; s <= F::LOG; s++) ap[s] = gl::emul(ap[s - 1], ap[s - 1]);
  E H[2];
#pragma unroll
  for (int b = 0; b < 2 * F::SUMS_FIRST; b++) H[b] = horner_strided<1 << F::LOG>(c, b == 0 ? c.o_const : c.o_zs_next, b == 0 ? c.n_this : c.n_next, f.t, p, ap[F::LOG]);
#pragma unroll
  for (int b = 0; b < 2; b++) {
    if constexpr (!F::SUMS_FIRST) H[b] = horner_strided<1 << F::LOG>(c, b == 0 ? c.o_const : c.o_zs_next, b == 0 ? c.n_this : c.n_next, f.t, p, ap[F::LOG]);
    const E y = f.fold(H[b], ap);
    if (leader) { chal(c, (b == 0 ? CH_Y0(c) : CH_Y1(c)), p) = y.a; chal(c, (b == 0 ? CH_Y0(c) : CH_Y1(c)) + 1, p) = y.b; }
  }
}

// one workgroup of transcripts: `tl` lanes per proof (16: row form, 4: quad form); FORM 1: the
// lane form (kernels of its own, so that its register demand does not touch the others')
template <int FORM = 0, bool KEYED = false>
__device__ __forceinline__ void transcript_block(const DevCircuit& c, int tl, TLdsAny& U) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if constexpr (FORM == 1) {
    if (g < c.B) transcript<KEYED>(c, g, LaneForm{});
  } else if (tl == 16) {
    lp::Row LR;
    lp::init(LR, U.l, threadIdx.x);
    if ((g >> 4) < c.B) transcript<KEYED>(c, g >> 4, RowForm(LR, U.l));
  } else {
    if ((g >> 2) < c.B) transcript<KEYED>(c, g >> 2, QuadForm{g & 3, U.q});
  }
}

// ------------------------------------------------------------------------ phase 1
// blocks [0, nt_blocks): transcripts, `tl` lanes per proof (16: row form, 4: quad form) at
// raised wave priority so co-resident leaf waves do not stretch the serial chain; the
// rest: leaf hashing, 4 units per block.  Transcript blocks come first so they start first.
template <int FORM, bool KEYED = false>
__device__ __forceinline__ void phase1_body(const DevCircuit& c, int nt_blocks, int tl) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ TLdsAny T;
  if ((int)blockIdx.x < nt_blocks) {   // block-uniform branch: the whole workgroup fills T
    __builtin_amdgcn_s_setprio(3);
    if constexpr (FORM == 0) tlds_fill_form(T, tl);
    transcript_block<FORM, KEYED>(c, tl, T);
    return;
  }
  const int unit = ((int)blockIdx.x - nt_blocks) * 4 + wave;
  const int units = c.Q * c.nleaf * (c.B >> 6);
  if (unit < units) leaf_hash_unit(c, unit, lane);
}
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) k_phase1(DevCircuit c, int nt_blocks, int tl) {
  phase1_body<0>(c, nt_blocks, tl);
}
// the lane-form transcript (P2V_TRANSCRIPT=lane) with the leaf hashing
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) k_phase1_lane(DevCircuit c, int nt_blocks, int tl) {
  phase1_body<1>(c, nt_blocks, tl);
}
// the two with per-proof verifier keys (p2v_verifier_run_keyed)
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) k_phase1_keyed(DevCircuit c, int nt_blocks, int tl) {
  phase1_body<0, true>(c, nt_blocks, tl);
}
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) k_phase1_lane_keyed(DevCircuit c, int nt_blocks, int tl) {
  phase1_body<1, true>(c, nt_blocks, tl);
}

// The same two halves as separate launches, for the transcript lookahead (P2V_FLAG_LOOKAHEAD,
// api_run.cpp): the transcript on a stream of its own, one batch ahead of the leaf hashing.  (As the
// default form of phase 1 they measured slower: DESIGN.md "Retired run-time switches".)
extern "C" __global__ void __launch_bounds__(256) k_transcript(DevCircuit c, int tl) {
  __builtin_amdgcn_s_setprio(3);
  __shared__ TLdsAny T;
  tlds_fill_form(T, tl);
  transcript_block(c, tl, T);
}
// the lane form on its own
extern "C" __global__ void __launch_bounds__(256) k_transcript_lane(DevCircuit c, int tl) {
  __builtin_amdgcn_s_setprio(3);
  __shared__ TLdsAny T;
  transcript_block<1>(c, tl, T);
}
// and with per-proof verifier keys
extern "C" __global__ void __launch_bounds__(256) k_transcript_keyed(DevCircuit c, int tl) {
  __builtin_amdgcn_s_setprio(3);
  __shared__ TLdsAny T;
  tlds_fill_form(T, tl);
  transcript_block<0, true>(c, tl, T);
}
extern "C" __global__ void __launch_bounds__(256) k_transcript_lane_keyed(DevCircuit c, int tl) {
  __builtin_amdgcn_s_setprio(3);
  __shared__ TLdsAny T;
  transcript_block<1, true>(c, tl, T);
}
extern "C" __global__ void __launch_bounds__(256) k_leaf(DevCircuit c) {
  const int unit = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit < c.Q * c.nleaf * (c.B >> 6)) leaf_hash_unit(c, unit, threadIdx.x & 63);
}
