// keys.hip — each proof's verifier key from its own public inputs (include/p2v.h "self-keyed
// circuits").  plonky2's add_verifier_data_public_inputs() ends a circuit's public inputs with its
// VerifierOnlyCircuitData, [circuit_digest | constants_sigmas_cap]; k_key_resolve looks that tail
// up in the handle's key table and writes the index, the id a keyed run verifies the proof against.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/p2v.h"
#include "devcommon.h"
#include "kernels.h"

namespace {
// word t of lane p's tail, canonical as the table's keys are
__device__ __forceinline__ uint64_t tail_word(const DevCircuit& c, int64_t tail, int t, int p) {
  const uint64_t w = p2d::ld(c, tail + t, p);
  return w >= gl::P ? w - gl::P : w;
}
}  // namespace

// One lane per proof over c.B lanes (lanes past n re-read proof n - 1 and write nothing).  A key
// is cap_len + 1 digests; both passes take a digest (four words) per step so that its loads go out
// together: the kernel is a latency chain in front of phase 1, not a bandwidth load.  The tail is
// hashed in one pass (the digests' loads are independent of the hash chain, four steps unrolled)
// and not kept: each candidate's compare reads it again (68 words at cap_height 4, cache-resident
// after the first pass) against the candidate's key row and leaves at the first differing digest
// -- not at the first differing word: up to three more cached loads per candidate, for a compare
// chain of cap_len + 1 dependent steps instead of 4 cap_len + 4 (DESIGN.md §5.8 has what was
// measured: the two passes were regrouped together, the compare's share alone was not).
// The digest loops are wave-uniform; the table slot and the key row differ per lane.  A proof
// picks only its start slot: the probe ends at an empty slot, which a table of at least 2 nkeys
// slots always has, and never runs past the table's size.
// No key equals the tail, or the public inputs are shorter than a key: P2V_KEY_NONE, which
// k_status reports as P2V_ERR_CIRCUIT like any id past the table.
extern "C" __global__ void __launch_bounds__(256) k_key_resolve(DevCircuit c, uint32_t* ids) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int kw = 4 * c.cap_len + 4;
  if (c.num_pis < kw) {
    if (p < c.n) ids[p] = P2V_KEY_NONE;
    return;
  }
  const int64_t tail = c.pis + c.num_pis - kw;
  uint64_t h = 0;
#pragma unroll 4
  for (int g = 0; g <= c.cap_len; g++) {   // digest g of the key encoding
    const int t = p2v_key_tail_word(4 * g, c.cap_len);
    const uint64_t w0 = tail_word(c, tail, t, p), w1 = tail_word(c, tail, t + 1, p);
    const uint64_t w2 = tail_word(c, tail, t + 2, p), w3 = tail_word(c, tail, t + 3, p);
    h = p2v_key_hash(p2v_key_hash(p2v_key_hash(p2v_key_hash(h, w0), w1), w2), w3);
  }
  uint32_t slot = (uint32_t)h & c.key_tab_mask;
  uint32_t id = P2V_KEY_NONE;
  for (uint32_t probes = 0; probes <= c.key_tab_mask; probes++) {
    const uint32_t e = c.key_tab[slot];
    if (e == 0) break;
    const uint64_t* key = c.keys + (int64_t)(e - 1) * kw;
    int g = 0;
    for (; g <= c.cap_len; g++) {
      const int t = p2v_key_tail_word(4 * g, c.cap_len);
      const uint64_t* k4 = key + 4 * g;
      const bool same = (k4[0] == tail_word(c, tail, t, p)) & (k4[1] == tail_word(c, tail, t + 1, p)) &
                        (k4[2] == tail_word(c, tail, t + 2, p)) & (k4[3] == tail_word(c, tail, t + 3, p));
      if (!same) break;
    }
    if (g > c.cap_len) { id = e - 1; break; }
    slot = (slot + 1) & c.key_tab_mask;
  }
  if (p < c.n) ids[p] = id;
}
