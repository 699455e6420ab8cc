// Dumps the tables of the throughput permutation's own schedule (csrc/poseidon.h make_pf: the
// leading unit that folds full round 3's MDS into its partial rounds, then blocks of 4) as JSON,
// for tests/test_poseidon_fold3.py to compare with its exact-integer model.  Host build only:
//   g++ -std=c++17 -O1 -o pf_dump tools/pf_dump.cpp
#include <cstdio>
#include "../plonky2-verifier_amd/csrc/poseidon.h"

static void dump(const p2::PBlock& B) {
  std::printf("{\"cf\": [");
  for (int r = 0; r < 14; r++) {
    std::printf("%s[", r ? ", " : "");
    for (int j = 0; j < 16; j++) std::printf("%s%u", j ? ", " : "", B.cf[r][j]);
    std::printf("]");
  }
  std::printf("], \"d\": [");
  for (int k = 0; k < 16; k++) std::printf("%s%llu", k ? ", " : "", (unsigned long long)((B.dhi[k] << 32) | B.dlo[k]));
  std::printf("]}");
}

int main() {
  static const p2::PFTab T = p2::make_pf();
  std::printf("{\"lead_rounds\": %d, \"lead\": ", p2::PF_LEAD);
  dump(T.lead);
  std::printf(", \"blocks\": [");
  for (int b = 0; b < p2::PF_NB; b++) {
    if (b) std::printf(", ");
    dump(T.b[b]);
  }
  std::printf("]}\n");
  return 0;
}
