// leafhash.h — what kernels.hip (phase 1), merkle.hip (the Merkle path kernels) and selftest.hip
// need in common: the leaf sponge, and the LDS constant tables of the transcript forms that the
// row form of the permutation runs on.
#pragma once
#include "devcommon.h"
#include "qposeidon.h"
#include "rposeidon.h"
#include "lposeidon.h"

namespace p2d {

// The leaf sponge (Hash/Sponge.hs:26-31) of the len words at proof word off of lane p: st[0..3]
// is the digest.  leaf_hash_unit calls it with a wave-uniform off, k_merkle_known_miss with the
// lane's own.
__device__ __forceinline__ void leaf_sponge(const DevCircuit& c, int64_t off, int len, int p, uint64_t (&st)[12]) {
#pragma unroll
  for (int i = 0; i < 12; i++) st[i] = 0;
  if (c.noop_leaves && len <= 4) {   // P2V_EXT_HASH_OR_NOOP: plonky2 hash_or_noop, the leaf zero-padded
#pragma unroll
    for (int j = 0; j < 4; j++) if (j < len) st[j] = ld(c, off + j, p);
    len = 0;
  }
  // sponge, overwrite mode, no padding.  One 8-word block per trip, its words loaded one
  // permutation ahead (during the previous block's permutation, into the registers that block has
  // just been copied out of), so no wave waits for its row at the top of a trip; one permutation
  // call site (round 6; the two-blocks-per-trip form of round 5: DESIGN.md "Retired build options")
  uint64_t nb[8];
#pragma unroll
  for (int j = 0; j < 8; j++) nb[j] = j < len ? ld(c, off + j, p) : 0;
  for (int i = 0; i < len; i += 8) {
    const int k = len - i;
#pragma unroll
    for (int j = 0; j < 8; j++) if (j < k) st[j] = nb[j];
#pragma unroll
    for (int j = 0; j < 8; j++) nb[j] = 8 + j < k ? ld(c, off + i + 8 + j, p) : 0;
    // words the rest of the sponge reads: the digest (0..3) after the last block, else the
    // words the next block does not overwrite (nx.. 11); state words 8..11 are 0 in block 0
    const int nx = k - 8;
    p2::permute_dev<true>(st, i == 0, nx <= 0 ? 1 : (nx >= 8 ? 4 : ((7 << (nx >> 2)) & 7)));   // block 0: the folded zh round 0
  }
}

// the constant tables of the transcript forms, in LDS (qposeidon.h TLds, lposeidon.h TLdsL)
union TLdsAny { qp::TLds q; lp::TLdsL l; };

// the constant tables of the transcript form in use (tl uniform: 16 the row form, else quad)
__device__ __forceinline__ void tlds_fill_form(TLdsAny& T, int tl) {
  if (tl == 16) lp::tlds_fill(T.l, threadIdx.x, 256);
  else qp::tlds_fill(T.q, threadIdx.x, 256);
}

}  // namespace p2d
