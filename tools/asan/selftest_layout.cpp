// p2v_selftest_layout under AddressSanitizer + UBSan (tools/asan/selftest_layout.sh): every op's
// sizes and the shared words it refuses, with b in heap blocks of exactly nb words so that a read
// past nb is an error.  Host code only: no device is opened.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/p2v.h"

static int failures = 0;

// the call on a copy of b that ends where nb says
static int layout(int op, const std::vector<uint64_t>* b, size_t* w) {
  uint64_t* h = nullptr;
  if (b) {
    h = (uint64_t*)malloc(b->size() * 8 + b->empty());
    if (!b->empty()) memcpy(h, b->data(), b->size() * 8);
  }
  const int rc = p2v_selftest_layout(op, h, b ? b->size() : 0, &w[0], &w[1], &w[2]);
  free(h);
  return rc;
}
static void sizes(int op, const std::vector<uint64_t>* b, size_t in, size_t out, size_t bw) {
  size_t w[3] = {99, 99, 99};
  const int rc = layout(op, b, w);
  if (rc != P2V_OK || w[0] != in || w[1] != out || w[2] != bw) {
    printf("op %d: rc %d, %zu %zu %zu, expected %zu %zu %zu\n", op, rc, w[0], w[1], w[2], in, out, bw);
    failures++;
  }
}
static void refused(int op, const std::vector<uint64_t>* b) {
  size_t w[3];
  const int rc = layout(op, b, w);
  if (rc != P2V_E_ARG) { printf("op %d: rc %d, expected P2V_E_ARG\n", op, rc); failures++; }
}

int main() {
  using V = std::vector<uint64_t>;
  const uint64_t MAGIC = P2V_WORDS_GATE_MAGIC;
  static const struct { int op; size_t in, out, b; } fixed[] = {
      {0, 1, 1, 1}, {1, 12, 12, 0}, {2, 12, 12, 0}, {3, 1, 1, 1}, {4, 12, 12, 24}, {5, 1, 1, 0}, {6, 1, 2, 1}, {7, 1, 1, 0},
      {8, 1, 1, 0}, {9, 12, 12, 0}, {10, 12, 12, 0}, {12, 2, 5, 0}, {13, 4, 2, 0}, {14, 1, 1, 0}, {15, 2, 2, 0}, {16, 4, 4, 0},
      {22, 12, 12, 0}};
  for (const auto& f : fixed) sizes(f.op, nullptr, f.in, f.out, f.b);
  const V k32{32}, e32{0xFFFFFFFFull}, w2{2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, w40{40, 5, 2, 10, 12, 20, 33, 8, 2, 8, 13, 7}, ab1{1}, ab8{8};
  sizes(17, &k32, 1, 1, 1);
  sizes(18, &e32, 2, 2, 1);
  sizes(19, &w2, 2, 2, 12);
  sizes(19, &w40, 40, 2, 12);
  sizes(20, &ab1, 6, 2, 1);
  sizes(20, &ab8, 514, 2, 1);
  const V pv0{0, 0, 7}, pv2{2, 1, 1}, leaf0{0, 0}, leaf135{135, 1}, leafmax{1ull << 20, 0};
  sizes(23, &pv0, 12, 12, 3);
  sizes(23, &pv2, 12, 12, 3);
  sizes(24, &leaf0, 0, 4, 2);
  sizes(24, &leaf135, 135, 4, 2);
  sizes(24, &leafmax, 1u << 20, 4, 2);
  for (int op : {-1, 11, 25}) refused(op, nullptr);
  const V k33{33}, e2_32{1ull << 32}, past{8, 1, 4, 0, 0, 0, 0, 5, 0, 0, 0, 0}, short19{2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, ab0{0}, ab9{9}, none{};
  refused(17, &k33);
  refused(18, &e2_32);
  refused(19, &past);
  refused(19, &short19);
  refused(20, &ab0);
  refused(20, &ab9);
  const V form3{3, 0, 7}, zh2{0, 2, 7}, gm0{0, 0, 0}, gm8{0, 0, 8}, short23{0, 1}, long24{(1ull << 20) + 1, 0}, noop2{8, 2}, short24{8};
  for (const V* b : {&form3, &zh2, &gm0, &gm8, &short23}) refused(23, b);
  for (const V* b : {&long24, &noop2, &short24}) refused(24, b);
  for (int op : {17, 18, 19, 20, 21, 23, 24}) { refused(op, nullptr); refused(op, &none); }
  // op 21: nwires, nconsts, then c0 = w2 * k1, c1 = pih3 (WIRE 2, CONST 1, MUL 0 1, COMMIT 2, PIHASH 3, COMMIT 3)
  const V prog{3, 2, MAGIC, 6, 0, 2, 1, 1, 6, 0, 1, 8, 2, 2, 3, 8, 3};
  sizes(21, &prog, 2 * (3 + 2) + 4, 2 * 2, prog.size());
  V longer = prog, magic = prog, narrow = prog, cut = prog, many = prog;
  longer.insert(longer.end(), {7, 7, 7});
  sizes(21, &longer, 14, 4, prog.size());
  magic[2] ^= 1; narrow[0] = 2; cut.pop_back(); many[3] = 1ull << 40;
  for (const V* b : {&magic, &narrow, &cut, &many}) refused(21, b);
  for (size_t nb = 0; nb < prog.size(); nb++) { const V head(prog.begin(), prog.begin() + nb); refused(21, &head); }
  printf("%s\n", failures ? "FAILED" : "selftest_layout: ok");
  return failures != 0;
}
