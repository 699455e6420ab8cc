// kernels.hip — gfx950 kernels of the batch verifier: phase 1 (transcripts and leaf hashing), the
// FRI queries, the status and the self-tests.  The Merkle path kernels live in merkle.hip, the
// vanishing / gate-constraint kernels in vanish*.hip.
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
//   k_fri         combineInitial + folding steps + final polynomial, one lane per
//                 (proof, query)  (Plonk/FRI.hs:151-407)
//   k_status      reference evaluation order -> int8 status (+ optional trace)
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

// ------------------------------------------------------------------------ FRI query
// foldCosetWith (Plonk/FRI.hs:263-279) for arity 2^AB: the coset values (received order v,
// bit-reversed coset order vals[rev k] = v[k]) are interpolated and evaluated at beta.
// c_k = sum_j vals_j w^{-jk} is a DIT FFT applied to v directly (v is already the
// bit-reversal of vals); P(beta) = (1/2^AB) sum_k c_k (beta/ofs)^k.
template <int AB>
__device__ __forceinline__ E fold_regs(const DevCircuit& c, int s, int64_t off, int p, E beta_over_ofs) {
  constexpr int AR = 1 << AB;
  E a[AR];
#pragma unroll
  for (int k = 0; k < AR; k++) a[k] = lde(c, off + 2 * k, p);
  const uint64_t* tw = c.twiddles + 256 * s;   // omega^{-j}
#pragma unroll
  for (int len = 2; len <= AR; len <<= 1) {
#pragma unroll
    for (int i = 0; i < AR; i += len) {
#pragma unroll
      for (int k = 0; k < len / 2; k++) {
        E u = a[i + k], v = a[i + k + len / 2];
        if (k != 0) v = gl::escale(tw[k * (AR / len)], v);
        a[i + k] = gl::eadd(u, v);
        a[i + k + len / 2] = gl::esub(u, v);
      }
    }
  }
  E acc = gl::e0();
#pragma unroll
  for (int k = AR - 1; k >= 0; k--) acc = gl::eadd(gl::emul(acc, beta_over_ofs), a[k]);
  return gl::escale(c.inv_arity[s], acc);
}
// Arity 16 in two halves, so that only 8 F^2 values are live (k_fri's 96-VGPR budget held all 16
// with 152 B/lane of scratch).  The DIT's first three stages act on v[0..7] and v[8..15] alone,
// giving the 8-point transforms E, O (twiddles w^{-2jk}); the last stage is c_k = E_k + w^{-k} O_k,
// c_{k+8} = E_k - w^{-k} O_k.  With b = beta/ofs:
//   sum_{k<16} c_k b^k = (1 + b^8) sum_{k<8} E_k b^k + (1 - b^8) sum_{k<8} O_k (w^{-1} b)^k.
template <int AR>
__device__ __forceinline__ E dft8_horner(const DevCircuit& c, const uint64_t* tw, int64_t off, int p, E b) {
  E a[8];
#pragma unroll
  for (int k = 0; k < 8; k++) a[k] = lde(c, off + 2 * k, p);
#pragma unroll
  for (int len = 2; len <= 8; len <<= 1) {
#pragma unroll
    for (int i = 0; i < 8; i += len) {
#pragma unroll
      for (int k = 0; k < len / 2; k++) {
        E u = a[i + k], v = a[i + k + len / 2];
        if (k != 0) v = gl::escale(tw[k * (AR / len)], v);
        a[i + k] = gl::eadd(u, v);
        a[i + k + len / 2] = gl::esub(u, v);
      }
    }
  }
  E acc = gl::e0();
#pragma unroll
  for (int k = 7; k >= 0; k--) acc = gl::eadd(gl::emul(acc, b), a[k]);
  return acc;
}
__device__ __forceinline__ E fold16_halves(const DevCircuit& c, int s, int64_t off, int p, E b) {
  const uint64_t* tw = c.twiddles + 256 * s;
  const E lo = dft8_horner<16>(c, tw, off, p, b);
  __builtin_amdgcn_sched_barrier(0);   // keep the halves apart: one half's 8 values live at a time
  const E hi = dft8_horner<16>(c, tw, off + 16, p, gl::escale(tw[1], b));
  const E b2 = gl::emul(b, b), b4 = gl::emul(b2, b2), b8 = gl::emul(b4, b4);
  const E one = gl::eb(1);
  const E acc = gl::eadd(gl::emul(gl::eadd(one, b8), lo), gl::emul(gl::esub(one, b8), hi));
  return gl::escale(c.inv_arity[s], acc);
}
// generic arity: direct O(arity^2) evaluation of the same interpolant
__device__ E fold_generic(const DevCircuit& c, int s, int ab, int64_t off, int p, E beta_over_ofs) {
  const int ar = 1 << ab;
  const uint64_t* tw = c.twiddles + 256 * s;
  E acc = gl::e0();
  for (int k = ar - 1; k >= 0; k--) {
    E ck = gl::e0();
    for (int j = 0; j < ar; j++) {
      const int jj = (int)gl::rev_bits(ab, (uint32_t)j);   // vals[j] = v[rev j]
      ck = gl::eadd(ck, gl::escale(tw[(j * k) & (ar - 1)], lde(c, off + 2 * jj, p)));
    }
    acc = gl::eadd(gl::emul(acc, beta_over_ofs), ck);
  }
  return gl::escale(c.inv_arity[s], acc);
}

// ---- combineInitial's reduceWithPowers (Goldilocks.hs:180-183, Plonk/FRI.hs:151-207):
// sum_v alpha^v y_v over a list of base-field leaf words (up to 5 contiguous segments of the
// query's leaves, ascending), alpha in F^2.  Round 4 ran one F^2 Horner step per word (a full
// emul, ~100 VALU).  Round 5: Horner in chunks of 8, g <- g alpha^8 + sum_{k<8} y_{j+k} alpha^k,
// with alpha^1..alpha^8 in registers; the inner sum's base-field products y alpha^k (2 per word,
// one per component) are accumulated unreduced in 128 + 3 bits and reduced once per chunk and
// component.  The same field element (exact arithmetic).
struct Acc3 { uint64_t lo, hi; uint32_t top; };   // lo + hi 2^64 + top 2^128
__device__ __forceinline__ void acc_mul(Acc3& A, uint64_t y, uint64_t c) {
  uint64_t h, l;
  gl::mul128(y, c, h, l);
  const uint64_t lo2 = A.lo + l;
  const uint64_t c0 = lo2 < l ? 1 : 0;
  const uint64_t hi2 = A.hi + h;
  const uint32_t c1 = hi2 < h ? 1u : 0u;
  const uint64_t hi3 = hi2 + c0;
  const uint32_t c2 = hi3 < c0 ? 1u : 0u;
  A.lo = lo2; A.hi = hi3; A.top += c1 + c2;
}
// lo + hi 2^64 + top 2^128 mod p, canonical: 2^128 == (2^32 - 1)^2 == -2^32 (mod p), top <= 8
__device__ __forceinline__ uint64_t acc_reduce(const Acc3& A) {
  return gl::sub(gl::reduce128(A.hi, A.lo), (uint64_t)A.top << 32);
}
struct Segs { int64_t off[5]; int n[5]; int ns; };
__device__ __forceinline__ int64_t seg_addr(const Segs& S, int v) {   // v wave-uniform: scalar code
  for (int s = 0; s < S.ns; s++) {
    if (v < S.n[s]) return S.off[s] + v;
    v -= S.n[s];
  }
  return S.off[0];
}
__device__ __forceinline__ E reduce_powers(const DevCircuit& c, const Segs& S, int p, E alpha, const E* ap) {
  int N = 0;
  for (int s = 0; s < S.ns; s++) N += S.n[s];
  E g = gl::e0();
  const int rem = N & 7;
  for (int v = N - 1; v >= N - rem; v--) g = gl::eadd(gl::emul(g, alpha), gl::eb(ld(c, seg_addr(S, v), p)));
  for (int j = N - rem - 8; j >= 0; j -= 8) {
    uint64_t y[8];
#pragma unroll
    for (int k = 0; k < 8; k++) y[k] = ld(c, seg_addr(S, j + k), p);
    Acc3 A{y[0], 0, 0}, B{0, 0, 0};   // alpha^0 = 1
#pragma unroll
    for (int k = 1; k < 8; k++) { acc_mul(A, y[k], ap[k].a); acc_mul(B, y[k], ap[k].b); }
    g = gl::eadd(gl::emul(g, ap[8]), E{acc_reduce(A), acc_reduce(B)});
  }
  return g;
}
// alpha^0..alpha^8 for reduce_powers
__device__ __forceinline__ void alpha_powers(E alpha, E* ap) {
  ap[0] = gl::eb(1); ap[1] = alpha;
#pragma unroll
  for (int k = 2; k <= 8; k++) ap[k] = gl::emul(ap[k - 1], alpha);
}
// one folding step of arity 2^ab: the form k_fri runs at each arity
__device__ __forceinline__ E fold_step(const DevCircuit& c, int s, int ab, int64_t off, int p, E beta_over_ofs) {
  E nv;
  switch (ab) {
    case 1: nv = fold_regs<1>(c, s, off, p, beta_over_ofs); break;
    case 2: nv = fold_regs<2>(c, s, off, p, beta_over_ofs); break;
    case 3: nv = fold_regs<3>(c, s, off, p, beta_over_ofs); break;
    case 4: nv = fold16_halves(c, s, off, p, beta_over_ofs); break;
    default: nv = fold_generic(c, s, ab, off, p, beta_over_ofs); break;
  }
  return nv;
}

// k_fri runs on the side stream beside k_merkle (see vanish.hip P2V_SIDE_WAVES): 5 waves per SIMD
// caps it at 96 VGPRs, so a wave fits where one k_merkle wave retired (0: compiler default, 122)
#ifndef P2V_FRI_WAVES
#define P2V_FRI_WAVES 5
#endif
#if P2V_FRI_WAVES > 0
#define P2V_FRI_ATTR __attribute__((amdgpu_waves_per_eu(P2V_FRI_WAVES)))
#else
#define P2V_FRI_ATTR
#endif
extern "C" __global__ void __launch_bounds__(256) P2V_FRI_ATTR k_fri(DevCircuit c) {
  const int lane = threadIdx.x & 63;
  const int unit = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int NPB = c.B >> 6;
  if (unit >= c.Q * NPB) return;
  __builtin_amdgcn_s_setprio(2);   // side stream, concurrent with k_merkle (see k_vanish)
  const int pb = unit % NPB, q = unit / NPB;
  const int p = pb * 64 + lane;
  const int64_t base = c.q0 + (int64_t)q * c.qstride;
  const int r = c.r;
  uint32_t idx = (uint32_t)chal(c, CH_QIDX(c) + q, p);
  const E alpha = chal_e(c, CH_FRI_ALPHA(c), p);
  const E zeta = chal_e(c, CH_ZETA(c), p);
  // combineInitial, Plonk/FRI.hs:151-207.  firstBatch = consts|sigmas, wires, pp part,
  // quotient, lookup part; secondBatch = first r of the pp part, lookup part.
  const int npp_all = r * ((c.num_routed + c.qdf - 1) / c.qdf);
  const int64_t l0 = base + c.leaf[0], l1 = base + c.leaf[1], l2 = base + c.leaf[2], l3 = base + c.leaf[3];
  // ascending lists: firstBatch =
  // leaf0 | leaf1 | leaf2[0, npp_all) | leaf3 | leaf2[npp_all, w2); secondBatch = leaf2[0, r') |
  // leaf2[npp_all, w2)
  E ap[9];
  alpha_powers(alpha, ap);
  const int rr = r < npp_all ? r : npp_all;
  Segs s0{{l0, l1, l2, l3, l2 + npp_all}, {c.width[0], c.width[1], npp_all, c.width[3], c.width[2] - npp_all}, 5};
  Segs s1{{l2, l2 + npp_all, 0, 0, 0}, {rr, c.width[2] - npp_all, 0, 0, 0}, 2};
  const E g0 = reduce_powers(c, s0, p, alpha, ap);
  const E g1 = reduce_powers(c, s1, p, alpha, ap);
  const int len2 = (r < npp_all ? r : npp_all) + (c.width[2] - npp_all);
  const uint64_t px = gl::mul(gl::MULT_GEN, pow_root(c, c.lde_bits, gl::rev_bits(c.lde_bits, idx)));
  const uint64_t omega = c.root_pow2[32 - c.degree_bits];
  E d0 = gl::esub(gl::eb(px), zeta), d1 = gl::esub(gl::eb(px), gl::escale(omega, zeta));
  E i0, i1; einv2(d0, d1, i0, i1);
  const E one = gl::emul(gl::esub(g0, chal_e(c, CH_Y0(c), p)), i0);
  const E two = gl::emul(gl::esub(g1, chal_e(c, CH_Y1(c), p)), i1);
  E cur = gl::eadd(gl::emul(epow_u(alpha, (uint32_t)len2), one), two);
  uint64_t* qv = c.qvals + (int64_t)q * 6 * c.B + p;
  qv[0] = cur.a; qv[(int64_t)c.B] = cur.b;
  // folding steps, Plonk/FRI.hs:306-323
  uint32_t bits = 0;
  int logn = c.lde_bits;
  for (int s = 0; s < c.S; s++) {
    const int ab = c.arity[s];
    const int64_t eoff = base + c.step_evals[s];
    const uint32_t pos = idx & ((1u << ab) - 1);
    const E at = lde(c, eoff + 2 * pos, p);   // evals !! (idx mod arity)
    if (gl::eeq(at, cur)) bits |= 1u << s;
    // coset offset shift * eta^{rev((idx >> a) << a)}, and its inverse without an inversion
    const uint32_t start = gl::rev_bits(logn, (idx >> ab) << ab);
    const uint32_t nmask = (logn >= 32) ? 0xFFFFFFFFu : ((1u << logn) - 1);
    const uint64_t ofs_inv = gl::mul(c.step_shift_inv[s], pow_root(c, logn, (0u - start) & nmask));
    const E beta = chal_e(c, CH_FRI_BETA(c) + 2 * s, p);
    const E bo = gl::escale(ofs_inv, beta);
    cur = fold_step(c, s, ab, eoff, p, bo);
    idx >>= ab; logn -= ab;
  }
  qv[2 * (int64_t)c.B] = cur.a; qv[3 * (int64_t)c.B] = cur.b;
  // final polynomial at x = shift * eta^{rev idx}, Plonk/FRI.hs:288-291,325-327
  const uint64_t xf = gl::mul(c.step_shift[c.S], pow_root(c, logn, gl::rev_bits(logn, idx)));
  E acc = gl::e0();
  for (int k = c.final_len - 1; k >= 0; k--) acc = gl::eadd(gl::escale(xf, acc), lde(c, c.final_poly + 2 * k, p));
  qv[4 * (int64_t)c.B] = acc.a; qv[5 * (int64_t)c.B] = acc.b;
  if (gl::eeq(acc, cur)) bits |= 1u << 31;
  c.fri_bits[(int64_t)q * c.B + p] = bits;
}

// ------------------------------------------------------------------------ status
// verifyProof = eqs_ok && (pow_ok && and [rounds in order]) with the reference's error
// precedence inside a round (Plonk/Verifier.hs:62, Plonk/FRI.hs:370-407, 105-117, 306-313).
extern "C" __global__ void __launch_bounds__(256) k_status(DevCircuit c, int8_t* __restrict__ results, uint64_t* __restrict__ trace,
                                                           int64_t trace_words) {
  // a few short waves that gate the workspace's next batch: ahead of co-resident phase-1 waves
  __builtin_amdgcn_s_setprio(3);
  if (c.kmode && blockIdx.x == 0 && threadIdx.x == 0) *c.kmissn = 0;   // the next run's (its readers joined before this launch)
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= c.n) return;
  const bool eqs_ok = c.van[p] != 0;
  const uint64_t resp = chal(c, CH_POW(c), p);
  const int pb = c.pow_bits;
  const uint64_t mask = pb <= 0 ? 0ULL : (pb >= 64 ? ~0ULL : (((1ULL << pb) - 1) << (64 - pb)));
  const bool pow_ok = (resp & mask) == 0;
  int8_t st = 1;
  if (!eqs_ok || !pow_ok) st = 0;
  else {
    for (int q = 0; q < c.Q && st == 1; q++) {
      const uint8_t* mk = c.mk_ok + (int64_t)q * c.T * c.B + p;
      bool init_ok = mk[0] && mk[c.B] && mk[2 * (int64_t)c.B] && mk[3 * (int64_t)c.B];
      if (!init_ok) { st = -1; break; }
      const uint32_t bits = c.fri_bits[(int64_t)q * c.B + p];
      for (int s = 0; s < c.S; s++) {
        if (!mk[(int64_t)(4 + s) * c.B]) { st = -2; break; }
        if (!((bits >> s) & 1u)) { st = -3; break; }
      }
      if (st != 1) break;
      if (!((bits >> 31) & 1u)) st = 0;
    }
  }
  // a key id past the circuit's table (the kernels verified against a clamped id): no such
  // VerifierCircuitData, whatever the proof holds
  if (c.key_id && c.key_id[p] >= (uint32_t)c.nkeys) st = -6;   // P2V_ERR_CIRCUIT
  results[p] = st;
  if (trace) {
    uint64_t* tr = trace + (int64_t)p * trace_words;
    const int r = c.r, S = c.S, Q = c.Q;
    int64_t k = 0;
    for (int64_t w = 0; w < CH_QIDX(c) + Q; w++) tr[k++] = chal(c, w, p);
    for (int i = 0; i < 4 * r; i++) tr[k++] = c.van[(int64_t)(1 + i) * c.B + p];   // C_i then quotient_i
    for (int j = 0; j < 3; j++)
      for (int q = 0; q < Q; q++) {
        const uint64_t* qv = c.qvals + (int64_t)q * 6 * c.B + p;
        tr[k++] = qv[(int64_t)(2 * j) * c.B];
        tr[k++] = qv[(int64_t)(2 * j + 1) * c.B];
      }
    tr[k++] = (uint64_t)(eqs_ok ? 1 : 0) | ((uint64_t)(pow_ok ? 1 : 0) << 1);
    for (int i = 0; i < r * c.nluts; i++) tr[k++] = c.lutre[(int64_t)i * c.B + p];
    (void)S;
  }
}

// Self-test of the device field and hash primitives the verifier kernels are built from
// (p2v_selftest): op 0 gl::mul (canonical a b mod p, Goldilocks.hs:126-133), op 3 the S-box
// multiply form (gl::mul_nc_dev_v<2>, canonicalised), op 1 the
// Poseidon permutation (permute_dev, Hash/Poseidon.hs:42-46; a = n states of 12 words),
// op 2 the 2-to-1 compression form (permute_dev(s, zh, gm = words 0..3), Hash/Merkle.hs:21-24;
// a = n states whose words 8..11 are ignored and taken as 0), op 4 one MDS layer + constants
// (the permutation's row reduction with its grouped carry fix-up).  One lane per item.
// ops 5-8: the S-box forms x -> x^7 (Hash/Poseidon.hs:92-96) with their rare -2^64 fix-ups
// (ADVICE r4): 5 sbox_n<1> (throughput permutation, partial rounds), 6 sbox_n<2> on the pair
// (a[i], b[i]) (full rounds; out[2i], out[2i+1]), 7 lp::sbox (the row and quad forms' full rounds),
// 8 lp::sbox_u (their chain S-box, split over a lane pair); canonical outputs.  Op 8 runs two lanes
// per item (lanes 2i, 2i + 1 hold a[i], the even one stores): sbox_u swaps with its DPP neighbour,
// so every lane of a launched wave runs it, lanes past n on a copy of item n - 1.
extern "C" __global__ void __launch_bounds__(256) k_selftest(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (op == 8) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int64_t item = i >> 1;
    const uint64_t x = lp::sbox_u(a[item < n ? item : n - 1], (int)(i & 1));
    if (item < n && !(i & 1)) out[item] = gl::canon(x);
#endif
    return;
  }
  if (i >= n) return;
  if (op >= 5 && op <= 7) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (op == 5) { uint64_t x = a[i]; p2::dv::sbox_n<1>(&x); out[i] = gl::canon(x); }
    else if (op == 6) { uint64_t x[2] = {a[i], b[i]}; p2::dv::sbox_n<2>(x); out[2 * i] = gl::canon(x[0]); out[2 * i + 1] = gl::canon(x[1]); }
    else out[i] = gl::canon(lp::sbox(a[i]));
#endif
  } else if (op == 0) {
    out[i] = gl::mul(a[i], b[i]);
  } else if (op == 3) {
#if defined(__HIP_DEVICE_COMPILE__)
    out[i] = gl::canon(gl::mul_nc_dev_v<2>(a[i], b[i]));
#endif
  } else if (op == 4) {
    // one MDS layer plus the next round's constants, exactly as the permutation runs it
    // (poseidon.h: 32-bit-half accumulators, the rare carry fix-up in one uniform branch per
    // group of 4 rows); b = the constants' halves kl[12], kh[12], shared by every item
#if defined(__HIP_DEVICE_COMPILE__)
    uint64_t st[12], t[12], kl[12], kh[12];
#pragma unroll
    for (int k = 0; k < 12; k++) { st[k] = a[12 * i + k]; kl[k] = b[k]; kh[k] = b[12 + k]; }
    p2::dv::mds_group<0>(st, t, kl, kh);
    p2::dv::mds_group<4>(st, t, kl, kh);
    p2::dv::mds_group<8>(st, t, kl, kh);
#pragma unroll
    for (int k = 0; k < 12; k++) out[12 * i + k] = t[k];
#endif
  } else {
    uint64_t s[12];
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = op == 2 && k >= 8 ? 0 : a[12 * i + k];
    if (op == 1) p2::permute_dev(s);
    else p2::permute_dev(s, true, 1);
#pragma unroll
    for (int k = 0; k < 12; k++) out[12 * i + k] = op == 2 && k >= 4 ? 0 : s[k];
  }
}

// The latency forms of the permutation on caller-chosen states (p2v_selftest ops 9-10; ADVICE
// r4): 9 the row form (lposeidon.h; 16 lanes per state), 10 the quad form (qposeidon.h, 4 lanes).
// Every lane of a group takes part in the DPP moves, so lanes past n compute on a copy of state
// n - 1 and store nothing.  a, out: n states of 12 words.
// Op 22: the leading merged unit of the throughput form alone (poseidon.h PFTab, dv::pblock<3, true>),
// one lane per item: a = the 12 S-box outputs u of full round 3 (any u64), out = the state entering
// round 6, canonical.  u cannot be steered through a whole permutation, so the unit's row
// reductions and their rare carry fix-ups are driven here.
extern "C" __global__ void __launch_bounds__(256) k_selftest_forms(int op, const uint64_t* a, uint64_t* out, int64_t n) {
  if (op == 22) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint64_t u[12], t[12];
#pragma unroll
    for (int k = 0; k < 12; k++) u[k] = a[12 * i + k];
    p2::dv::pblock<3, true>(u, t, p2::c_pf.lead);
#pragma unroll
    for (int k = 0; k < 12; k++) out[12 * i + k] = gl::canon(t[k]);
#endif
    return;
  }
  __shared__ TLdsAny T;
  tlds_fill_form(T, op == 9 ? 16 : 4);
  const int lanes = op == 9 ? 16 : 4;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t item = g / lanes, src = item < n ? item : n - 1;
  const int t = (int)(g % lanes);
  const uint64_t* s = a + 12 * src;
  uint64_t* o = out + 12 * item;
  if (op == 9) {
    lp::Row LR;
    lp::init(LR, T.l, threadIdx.x);
    const uint64_t x = lp::permute(LR.L < 12 ? s[LR.L] : 0, LR, T.l);
    if (item < n && LR.L < 12) o[LR.L] = x;
  } else {
    uint64_t x[3] = {s[3 * t], s[3 * t + 1], s[3 * t + 2]};
    qp::permute(x, t, T.q);
    if (item < n) for (int k = 0; k < 3; k++) o[3 * t + k] = x[k];
  }
}

// The F / F^2 arithmetic and the FRI query code that k_fri and the vanishing kernels are built
// from, on caller-chosen items (p2v_selftest ops 12-20, include/p2v.h).  One lane per item; the
// items are read as k_fri reads a proof, through ld / lde on a DevCircuit whose batch is the item
// array (c.soa, c.words the item stride, c.n items), so lanes past n re-read item n - 1; they store
// nothing.  c carries the production tables of a circuit with FRI arity bits 1..8 (root_pow2,
// twiddles and inv_arity of step s = ab - 1).  b: the op's shared words.
extern "C" __global__ void __launch_bounds__(256) k_selftest_field(int op, DevCircuit c, const uint64_t* b, uint64_t* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int p = (int)i;
  const bool live = i < c.n;
  if (op == 12) {
    const uint64_t x = ld(c, 0, p), y = ld(c, 1, p);
    const uint64_t r[5] = {gl::add(x, y), gl::sub(x, y), gl::neg(x), gl::mul_small(x, 7), gl::mul_small(x, (uint32_t)y)};
    if (live) for (int k = 0; k < 5; k++) out[5 * i + k] = r[k];
  } else if (op == 13) {
    const E x = lde(c, 0, p), y = lde(c, 2, p);
    const E r = gl::eeq(x, y) ? gl::esqr(x) : gl::emul(x, y);
    if (live) { out[2 * i] = r.a; out[2 * i + 1] = r.b; }
  } else if (op == 14) {
    const uint64_t r = inv_chain(ld(c, 0, p));
    if (live) out[i] = r;
  } else if (op == 15) {
    const E r = einv(lde(c, 0, p));
    if (live) { out[2 * i] = r.a; out[2 * i + 1] = r.b; }
  } else if (op == 16) {
    E iu, iv;
    einv2(lde(c, 0, p), lde(c, 2, p), iu, iv);
    if (live) { out[4 * i] = iu.a; out[4 * i + 1] = iu.b; out[4 * i + 2] = iv.a; out[4 * i + 3] = iv.b; }
  } else if (op == 17) {
    const uint64_t r = pow_root(c, (int)b[0], (uint32_t)ld(c, 0, p));
    if (live) out[i] = r;
  } else if (op == 18) {
    const E r = epow_u(lde(c, 0, p), (uint32_t)b[0]);
    if (live) { out[2 * i] = r.a; out[2 * i + 1] = r.b; }
  } else if (op == 19) {
    // b = item stride, segment count, 5 offsets (item words), 5 lengths; alpha at item words 0..1
    Segs S;
    S.ns = (int)b[1];
    for (int k = 0; k < 5; k++) { S.off[k] = (int64_t)b[2 + k]; S.n[k] = (int)b[7 + k]; }
    const E alpha = lde(c, 0, p);
    E ap[9];
    alpha_powers(alpha, ap);
    const E r = reduce_powers(c, S, p, alpha, ap);
    if (live) { out[2 * i] = r.a; out[2 * i + 1] = r.b; }
  } else if (op == 20) {
    // b[0] = arity bits ab; beta / ofs at item words 0..1, the 2^ab coset values after it
    const int ab = (int)b[0];
    const E r = fold_step(c, ab - 1, ab, 2, p, lde(c, 0, p));
    if (live) { out[2 * i] = r.a; out[2 * i + 1] = r.b; }
  }
}
