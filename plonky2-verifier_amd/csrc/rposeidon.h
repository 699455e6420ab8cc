// rposeidon.h — DPP helpers for a Poseidon-12 state spread over a 16-lane row (device only):
// lane L < 12 of the row holds state word L, lanes 12..15 are idle.
//
// The row form's permutation itself is lposeidon.h (LDS exchange, merged partial rounds).  The
// permutation that lived here, the MDS as a sum over the 16 DPP row rotations with four selectable
// S-boxes, is retired (DESIGN.md "Retired build options"); what remains is what the row-form
// kernels use around the permutation: the row rotation, the word broadcast and the rotation's
// direction.  Row still carries that permutation's coefficient table, which nothing reads any
// more: without init's (dead) code the compiler allocates k_merkle_fix's registers differently, and
// the change that retired the permutation kept every kernel's instructions as they were.
#pragma once
#include "gl.h"
#include "poseidon.h"

namespace rp {

static __constant__ uint32_t c_mds_circ[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};

template <int M>
__device__ __forceinline__ uint32_t ror32(uint32_t v) {
  if constexpr (M == 0) return v;
  else return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x120 + M, 0xf, 0xf, true);   // row_ror:M (all lanes valid)
}
template <int S>
__device__ __forceinline__ uint32_t nbcast32(uint32_t v) {   // row_newbcast:S (lane S of each row)
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x150 + S, 0xf, 0xf, true);
}
template <int S>
__device__ __forceinline__ uint64_t nbcast64(uint64_t v) {
  return ((uint64_t)nbcast32<S>((uint32_t)(v >> 32)) << 32) | nbcast32<S>((uint32_t)v);
}
// broadcast word `pos` (wave-uniform, 0..11) of the row
__device__ __forceinline__ uint64_t get_word(uint64_t x, int pos) {
  switch (pos) {
    case 0: return nbcast64<0>(x);
    case 1: return nbcast64<1>(x);
    case 2: return nbcast64<2>(x);
    case 3: return nbcast64<3>(x);
    case 4: return nbcast64<4>(x);
    case 5: return nbcast64<5>(x);
    case 6: return nbcast64<6>(x);
    case 7: return nbcast64<7>(x);
    case 8: return nbcast64<8>(x);
    case 9: return nbcast64<9>(x);
    case 10: return nbcast64<10>(x);
    default: return nbcast64<11>(x);
  }
}

struct Row {
  uint32_t coef[16];   // coef[m] = M[L][src_L(m)] (unread, see above)
  uint32_t col0;       // M[L][0] (unread)
  int L;
  bool plus;           // row_ror:m reads lane (L + m) & 15 (else (L - m) & 15)
};

__device__ __forceinline__ uint32_t mds_entry(int i, int j) {   // Hash/Constants.hs:19-25
  return c_mds_circ[(j - i + 12) % 12] + ((i == 0 && j == 0) ? 8u : 0u);
}

template <int M>
__device__ __forceinline__ void init_coef(Row& R) {
  const int src = (int)ror32<M>((uint32_t)R.L);
  R.coef[M] = (R.L < 12 && src < 12) ? mds_entry(R.L, src) : 0u;
}

// coef and plus are found by rotating the lane id itself, so nothing here depends on the direction
// convention of row_ror
__device__ __forceinline__ void init(Row& R, int lane) {
  R.L = lane & 15;
  init_coef<0>(R); init_coef<1>(R); init_coef<2>(R); init_coef<3>(R);
  init_coef<4>(R); init_coef<5>(R); init_coef<6>(R); init_coef<7>(R);
  init_coef<8>(R); init_coef<9>(R); init_coef<10>(R); init_coef<11>(R);
  init_coef<12>(R); init_coef<13>(R); init_coef<14>(R); init_coef<15>(R);
  R.col0 = R.L < 12 ? mds_entry(R.L, 0) : 0u;
  R.plus = (int)ror32<1>((uint32_t)R.L) == ((R.L + 1) & 15);
}

__device__ __forceinline__ uint64_t set_word(uint64_t x, const Row& R, int pos, uint64_t v) { return R.L == pos ? v : x; }

}  // namespace rp
