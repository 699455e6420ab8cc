// fri.h — the FRI query device functions: the folding step of every arity and combineInitial's
// reduceWithPowers.  k_fri (fri.hip) is built from them and the self-tests (selftest.hip, ops 19-20)
// run them on caller-chosen items.
#pragma once
#include "devcommon.h"

namespace p2d {

// the radix-2 DIT stages of an N-point transform inside an AR-point one, in place: a holds N values
// in bit-reversed order, tw[j] = omega^{-j} for the AR-th root omega, so a stage of span len takes
// its twiddles at stride AR / len (N = AR: the whole transform; N < AR: its first log2 N stages)
template <int N, int AR>
__device__ __forceinline__ void dit(E (&a)[N], const uint64_t* tw) {
#pragma unroll
  for (int len = 2; len <= N; len <<= 1) {
#pragma unroll
    for (int i = 0; i < N; i += len) {
#pragma unroll
      for (int k = 0; k < len / 2; k++) {
        E u = a[i + k], v = a[i + k + len / 2];
        if (k != 0) v = gl::escale(tw[k * (AR / len)], v);
        a[i + k] = gl::eadd(u, v);
        a[i + k + len / 2] = gl::esub(u, v);
      }
    }
  }
}

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
  dit<AR, AR>(a, tw);
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
  dit<8, AR>(a, tw);
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

}  // namespace p2d
