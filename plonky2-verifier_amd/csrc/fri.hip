// fri.hip — the FRI query kernel and the status kernel of the batch verifier (data layout and lane
// mapping: kernels.hip).
//
//   k_fri         combineInitial + folding steps + final polynomial, one lane per
//                 (proof, query)  (Plonk/FRI.hs:151-407)
//   k_status      reference evaluation order -> int8 status (+ optional trace)
#include "fri.h"
#include "kernels.h"

using namespace p2d;
using gl::E;

// ------------------------------------------------------------------------ FRI query
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
