// selftest.hip — the kernels of p2v_selftest (api_selftest.cpp, include/p2v.h): the device field and
// hash primitives, the latency forms of the permutation and the FRI query code on caller-chosen
// items.  They instantiate what the verifier kernels are built from a second time, in a unit of
// their own so that no shipped kernel is compiled beside them.  (Op 21's kernel, k_selftest_prog,
// is in vanish_prog.hip with the interpreter it runs.)
#include "leafhash.h"
#include "fri.h"
#include "kernels.h"

using namespace p2d;
using gl::E;

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
// round 6, canonical.  The unit's row reductions and their rare carry fix-ups are driven here on u
// itself; inside a whole permutation u is steered by running the rounds before it backwards (every
// round is invertible: tests/poseidon_steer.py), which is how op 23 reaches them.
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

// The template instances of the throughput permutation that production runs, and the leaf sponge
// that picks among them (p2v_selftest ops 23-24, include/p2v.h), in a kernel of their own so that
// k_selftest keeps its registers.  One lane per item; the items are read as a proof batch is
// (k_selftest_field below), so lanes past n re-read item n - 1 and store nothing.
// Op 23: b = form, zh, gm.  form 0 permute_dev<true, true> (the leaf sponge, the transcript's
// throughput form), 1 permute_dev<true, false> (k_merkle: PM_SCHED's blocks, pblock<2>), 2
// permute_dev<false, true> (the lane transcript).  zh: words 8..11 are taken as 0.  Output groups
// outside gm are returned as 0: the device leaves them undefined.
// Op 24: b = len, noop_leaves (the latter arrives as c.noop_leaves): leaf_sponge over the item's len
// words, out = the 4 digest words.
extern "C" __global__ void __launch_bounds__(256) k_selftest_hash(int op, DevCircuit c, const uint64_t* b, uint64_t* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int p = (int)i;
  const bool live = i < c.n;
  uint64_t s[12];
  if (op == 23) {
    const int form = (int)b[0], gm = (int)b[2];
    const bool zh = b[1] != 0;
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = zh && k >= 8 ? 0 : ld(c, k, p);
    if (form == 0) p2::permute_dev<true, true>(s, zh, gm);
    else if (form == 1) p2::permute_dev<true, false>(s, zh, gm);
    else p2::permute_dev<false, true>(s, zh, gm);
    if (live) {
#pragma unroll
      for (int k = 0; k < 12; k++) out[12 * i + k] = (gm >> (k >> 2)) & 1 ? s[k] : 0;
    }
  } else {
    leaf_sponge(c, 0, (int)b[0], p, s);
    if (live) {
#pragma unroll
      for (int k = 0; k < 4; k++) out[4 * i + k] = s[k];
    }
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
