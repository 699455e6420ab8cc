// rposeidon.h — DPP helpers for a Poseidon-12 state spread over a 16-lane row (device only):
// lane L < 12 of the row holds state word L, lanes 12..15 are idle.
//
// The row form's permutation itself is lposeidon.h (LDS exchange, merged partial rounds).  Here is
// what the row-form kernels use around it: the row rotation, its direction and the word broadcast.
#pragma once
#include "gl.h"
#include "poseidon.h"

namespace rp {

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

// whether row_ror:m reads lane (L + m) & 15 (else (L - m) & 15): found by rotating the lane id
// itself, so nothing depends on the direction convention of row_ror
__device__ __forceinline__ bool ror_plus(int L) { return (int)ror32<1>((uint32_t)L) == ((L + 1) & 15); }

}  // namespace rp
