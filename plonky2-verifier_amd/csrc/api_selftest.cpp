// api_selftest.cpp — the device self-tests (p2v_selftest) and the measurement probes of util.hip.
#include <algorithm>
#include "api_internal.hpp"
#include "kernels.h"

// ---- the self-test ops (include/p2v.h is their specification): one row per op number.
// What the host needs to run an op: the words per item of a and of out, the words read at b, and
// (op 21) the lowered program: its check lowers the program to bound the values alive at once, so
// the result is kept for the launch (p2v_selftest_layout pays for it too, and drops it).
struct OpLayout {
  size_t in, out, b;
  std::vector<uint64_t> low;
};
// An op's check of its shared words: b holds nb of them.  P2V_E_ARG (with its message) for words
// the op refuses, b null or shorter than it reads among them; fills in the sizes that depend on b.
using SharedCheck = int (*)(const uint64_t* b, size_t nb, OpLayout& L);

static int bad_b() { return fail(P2V_E_ARG, "bad op / null argument"); }

static int shared_pow_root(const uint64_t* b, size_t nb, OpLayout&) {   // op 17
  if (!b || nb < 1) return bad_b();
  if (b[0] > 32) return fail(P2V_E_ARG, "pow_root: k > 32");
  return P2V_OK;
}
static int shared_epow_u(const uint64_t* b, size_t nb, OpLayout&) {   // op 18
  if (!b || nb < 1) return bad_b();
  if (b[0] > 0xFFFFFFFFull) return fail(P2V_E_ARG, "epow_u: e >= 2^32");
  return P2V_OK;
}
static int shared_reduce_powers(const uint64_t* b, size_t nb, OpLayout& L) {   // op 19: the kernel reads nothing outside an item
  if (!b || nb < 12) return bad_b();
  bool ok = b[0] >= 2 && b[0] <= (1u << 20) && b[1] <= 5;
  for (int k = 0; k < 5 && ok; k++) ok = b[2 + k] <= b[0] && b[7 + k] <= b[0] - b[2 + k];
  if (!ok) return fail(P2V_E_ARG, "reduce_powers: segment table outside the item");
  L.in = (size_t)b[0];
  return P2V_OK;
}
static int shared_fold(const uint64_t* b, size_t nb, OpLayout& L) {   // op 20
  if (!b || nb < 1) return bad_b();
  if (b[0] < 1 || b[0] > 8) return fail(P2V_E_ARG, "fold: arity bits outside 1..8");
  L.in = 2 + (2u << b[0]);
  return P2V_OK;
}
// op 21: b = nwires, nconsts, the program.  The program is checked as at circuit creation, so the
// kernel reads nothing outside an item and writes no slot past the file
static int shared_prog(const uint64_t* b, size_t nb, OpLayout& L) {
  if (!b || nb < 4) return bad_b();
  if (b[0] > (1u << 20) || b[1] > (1u << 20)) return fail(P2V_E_ARG, "gate program rows beyond this build's limits");
  const int64_t nw = (int64_t)b[0], nc = (int64_t)b[1];
  try {
    // the encoding's own instruction count bounds the walk: at most 3 words per instruction
    if (b[2] != P2V_WORDS_GATE_MAGIC) throw ParseError("gate program: bad magic / version");
    if (b[3] > (uint64_t)P2V_GATE_PROGRAM_MAX_INSTRS) throw CircuitError("gate program beyond this build's limits (instructions)");
    const size_t words = gate_program_extent(b + 2, std::min(nb - 2, 2 + 3 * (size_t)b[3]));
    const GateProgram g = decode_gate_program(b + 2, words);
    if (g.max_wire >= nw || g.max_const >= nc) throw CircuitError("(Array.!): gate program reads beyond the row");
    if (g.max_pih >= 4) throw CircuitError("(!!): gate program reads a public-inputs-hash word beyond 4");
    if (lower_gate_program(g, &L.low) > P2V_GATE_PROGRAM_MAX_LIVE) throw CircuitError("gate program beyond this build's limits (values alive at once)");
    L.in = (size_t)(2 * (nw + nc) + 4); L.out = 2 * (size_t)g.num_commits; L.b = 2 + words;
  } catch (const std::exception& e) { return fail(P2V_E_ARG, std::string("selftest op 21: ") + e.what()); }
  return P2V_OK;
}

// op 23: b = form, zh, gm: the template instance of permute_dev and its two uniform arguments
static int shared_perm_variant(const uint64_t* b, size_t nb, OpLayout&) {
  if (!b || nb < 3) return bad_b();
  if (b[0] > 2 || b[1] > 1 || b[2] < 1 || b[2] > 7) return fail(P2V_E_ARG, "permutation variant: form > 2, zh > 1 or gm outside 1..7");
  return P2V_OK;
}
// op 24: b = len, noop_leaves; the item is the leaf's len words
static int shared_leaf_sponge(const uint64_t* b, size_t nb, OpLayout& L) {
  if (!b || nb < 2) return bad_b();
  if (b[0] > (1u << 20) || b[1] > 1) return fail(P2V_E_ARG, "leaf_sponge: len > 2^20 or noop_leaves > 1");
  L.in = (size_t)b[0];
  return P2V_OK;
}

// K_HASH runs as K_FIELD does (its items read as a proof batch), in k_selftest_hash
enum Family : uint8_t { K_SELFTEST, K_FORMS, K_FIELD, K_HASH, K_PROG, RETIRED };
enum BKind : uint8_t { B_NONE, B_ITEM, B_SHARED };   // b: absent, b[i] beside a[i], or one block for all items
struct SelftestOp {
  Family kernel;
  uint8_t in, out;    // words per item of a and of out; 0: from the op's check
  uint8_t b;          // words at b (per item / shared); 0 with a check: from it
  BKind bkind;
  uint8_t lanes;      // per item
  bool empty_first;   // n == 0 is P2V_OK right behind the device count, b unread (else only after b passed its check:
                      // ops 12-20 behind hipSetDevice, op 21 ahead of the device count)
  SharedCheck check;  // of the shared words; ops without one only need b non-null
};
static const SelftestOp kOps[25] = {
    /*  0 gl::mul            */ {K_SELFTEST, 1, 1, 1, B_ITEM, 1, true, nullptr},
    /*  1 permutation        */ {K_SELFTEST, 12, 12, 0, B_NONE, 1, true, nullptr},
    /*  2 compression        */ {K_SELFTEST, 12, 12, 0, B_NONE, 1, true, nullptr},
    /*  3 S-box multiply     */ {K_SELFTEST, 1, 1, 1, B_ITEM, 1, true, nullptr},
    /*  4 MDS layer          */ {K_SELFTEST, 12, 12, 24, B_SHARED, 1, true, nullptr},
    /*  5 sbox_n<1>          */ {K_SELFTEST, 1, 1, 0, B_NONE, 1, true, nullptr},
    /*  6 sbox_n<2>          */ {K_SELFTEST, 1, 2, 1, B_ITEM, 1, true, nullptr},
    /*  7 lp::sbox           */ {K_SELFTEST, 1, 1, 0, B_NONE, 1, true, nullptr},
    /*  8 lp::sbox_u         */ {K_SELFTEST, 1, 1, 0, B_NONE, 2, true, nullptr},
    /*  9 row form           */ {K_FORMS, 12, 12, 0, B_NONE, 16, true, nullptr},
    /* 10 quad form          */ {K_FORMS, 12, 12, 0, B_NONE, 4, true, nullptr},
    // the retired pair form's permutation; the ops keep their numbers
    /* 11                    */ {RETIRED, 0, 0, 0, B_NONE, 0, false, nullptr},
    /* 12 add sub neg small  */ {K_FIELD, 2, 5, 0, B_NONE, 1, false, nullptr},
    /* 13 emul / esqr        */ {K_FIELD, 4, 2, 0, B_NONE, 1, false, nullptr},
    /* 14 inv_chain          */ {K_FIELD, 1, 1, 0, B_NONE, 1, false, nullptr},
    /* 15 einv               */ {K_FIELD, 2, 2, 0, B_NONE, 1, false, nullptr},
    /* 16 einv2              */ {K_FIELD, 4, 4, 0, B_NONE, 1, false, nullptr},
    /* 17 pow_root           */ {K_FIELD, 1, 1, 1, B_SHARED, 1, false, shared_pow_root},
    /* 18 epow_u             */ {K_FIELD, 2, 2, 1, B_SHARED, 1, false, shared_epow_u},
    /* 19 reduce_powers      */ {K_FIELD, 0, 2, 12, B_SHARED, 1, false, shared_reduce_powers},
    /* 20 fold_step          */ {K_FIELD, 0, 2, 1, B_SHARED, 1, false, shared_fold},
    /* 21 gate program       */ {K_PROG, 0, 0, 0, B_SHARED, 1, false, shared_prog},
    /* 22 leading merged unit*/ {K_FORMS, 12, 12, 0, B_NONE, 1, true, nullptr},
    /* 23 permutation variant*/ {K_HASH, 12, 12, 3, B_SHARED, 1, false, shared_perm_variant},
    /* 24 leaf_sponge        */ {K_HASH, 0, 4, 2, B_SHARED, 1, false, shared_leaf_sponge},
};
static const SelftestOp* selftest_op(int op) {
  return op < 0 || op > 24 || kOps[op].kernel == RETIRED ? nullptr : &kOps[op];
}
// the row's sizes, then what the op's check makes of b
static int selftest_layout(const SelftestOp& R, const uint64_t* b, size_t nb, OpLayout& L) {
  L.in = R.in; L.out = R.out; L.b = R.b;
  return R.check ? R.check(b, nb, L) : P2V_OK;
}

// the device side of every op: a and b up, the launch, out back.  launch(a, b, out) gets the device
// copies and returns a P2V_* code
#define SCK(x) HCK_AS("p2v_selftest", x)
template <class F>
static int selftest_on_device(const SelftestOp& R, const OpLayout& L, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n,
                              F launch) {
  const size_t bw = R.kernel == K_PROG ? 0 : R.bkind == B_ITEM ? n * L.b : L.b;   // op 21's b goes up lowered (OpLayout::low)
  DevBuf da, db, dout;
  SCK(da.alloc(n * L.in * 8)); SCK(db.alloc(bw * 8)); SCK(dout.alloc(n * L.out * 8));
  SCK(hipMemcpy(da.p, a, n * L.in * 8, hipMemcpyHostToDevice));
  if (bw) SCK(hipMemcpy(db.p, b, bw * 8, hipMemcpyHostToDevice));
  RCK(launch((const uint64_t*)da.p, (const uint64_t*)db.p, (uint64_t*)dout.p));
  SCK(hipGetLastError());
  SCK(hipMemcpy(out, dout.p, n * L.out * 8, hipMemcpyDeviceToHost));
  return P2V_OK;
}
// the items as a proof batch is read: one item per proof, item-major
static void items_as_batch(DevCircuit& d, const uint64_t* items, size_t words, size_t n) {
  d.soa = items; d.words = (int64_t)words; d.wstride = 1; d.tiled = 0;
  d.n = (int32_t)n; d.B = (int32_t)((n + 63) / 64 * 64);
}

extern "C" {

// p2v_selftest ops 12-20: the field and FRI query code on items read as a proof batch is, through
// a DevCircuit that holds the item array and the tables fill_scalars / fri_twiddles make for a
// circuit with FRI arity bits 1..8 (step s = ab - 1).  Ops 23-24 (K_HASH) read their items the same
// way; op 24's noop_leaves travels in the DevCircuit, where leaf_sponge looks for it.
static int selftest_field(const SelftestOp& R, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  OpLayout L;
  RCK(selftest_layout(R, b, SIZE_MAX, L));
  if (n > (size_t)INT32_MAX - 64) return fail(P2V_E_ARG, "too many items");
  if (n == 0) return P2V_OK;
  Circuit C;
  C.arities = {1, 2, 3, 4, 5, 6, 7, 8};
  C.step_depth.assign(8, 0); C.L.step_evals.assign(8, 0); C.L.step_path.assign(8, 0);
  DevCircuit d{};
  fill_scalars(C, d);
  if (op == 24) d.noop_leaves = (int32_t)b[1];
  DevBuf dtw;
  return selftest_on_device(R, L, a, b, out, n, [&](const uint64_t* da, const uint64_t* db, uint64_t* dout) {
    SCK(upload(dtw, fri_twiddles(C), d.twiddles));
    items_as_batch(d, da, L.in, n);
    const dim3 grid((unsigned)((n * R.lanes + 255) / 256));
    if (R.kernel == K_HASH) hipLaunchKernelGGL(k_selftest_hash, grid, dim3(256), 0, 0, op, d, db, dout);
    else hipLaunchKernelGGL(k_selftest_field, grid, dim3(256), 0, 0, op, d, db, dout);
    return P2V_OK;
  });
}

// p2v_selftest op 21: the gate-program interpreter (vanish_prog.hip) on items laid out as a proof's
// openings are.  Like the other ops' shared words, a b that does not pass its check is P2V_E_ARG,
// here decided before any device call.
static int selftest_prog(const SelftestOp& R, int device, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  OpLayout L;
  RCK(selftest_layout(R, b, SIZE_MAX, L));
  if (n > (size_t)INT32_MAX - 64) return fail(P2V_E_ARG, "too many items");
  const int ndev = p2v_device_count();
  if (ndev == 0) return fail(P2V_E_NODEVICE, "no HIP device");
  if (device < 0 || device >= ndev) return fail(P2V_E_ARG, "bad device index");
  if (n == 0 || L.out == 0) return P2V_OK;
  HCK(hipSetDevice(device));
  DevCircuit d{};
  d.prog_pih = (int64_t)L.in - 4;
  d.o_wires = 0; d.o_const = 2 * (int64_t)b[0];   // ngroups = nls = 0: Vars::k(i) is constant i
  DevBuf dprog;
  return selftest_on_device(R, L, a, b, out, n, [&](const uint64_t* da, const uint64_t*, uint64_t* dout) {
    SCK(upload(dprog, L.low, d.gprog));
    items_as_batch(d, da, L.in, n);
    hipLaunchKernelGGL(k_selftest_prog, dim3((unsigned)((n * R.lanes + 63) / 64)), dim3(64), 0, 0, d, dout, (int)(L.out / 2));
    return P2V_OK;
  });
}

int p2v_selftest(int device, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  const SelftestOp* R = selftest_op(op);
  // shared words with a check of their own are refused by it, null included, where the op runs it
  if (!R || (n && (!a || !out || (R->bkind != B_NONE && !R->check && !b)))) return fail(P2V_E_ARG, "bad op / null argument");
  if (R->kernel == K_PROG) return selftest_prog(*R, device, a, b, out, n);
  const int ndev = p2v_device_count();
  if (ndev == 0) return fail(P2V_E_NODEVICE, "no HIP device");
  if (device < 0 || device >= ndev) return fail(P2V_E_ARG, "bad device index");
  if (R->empty_first && n == 0) return P2V_OK;
  HCK(hipSetDevice(device));
  if (R->kernel == K_FIELD || R->kernel == K_HASH) return selftest_field(*R, op, a, b, out, n);
  OpLayout L;
  RCK(selftest_layout(*R, b, SIZE_MAX, L));
  const dim3 grid((unsigned)((n * R->lanes + 255) / 256));
  return selftest_on_device(*R, L, a, b, out, n, [&](const uint64_t* da, const uint64_t* db, uint64_t* dout) {
    if (R->kernel == K_FORMS) hipLaunchKernelGGL(k_selftest_forms, grid, dim3(256), 0, 0, op, da, dout, (int64_t)n);
    else hipLaunchKernelGGL(k_selftest, grid, dim3(256), 0, 0, op, da, db, dout, (int64_t)n);
    return P2V_OK;
  });
}
#undef SCK

int p2v_selftest_layout(int op, const uint64_t* b, size_t nb, size_t* item_words, size_t* out_words, size_t* b_words) {
  const SelftestOp* R = selftest_op(op);
  if (!R || !item_words || !out_words || !b_words) return fail(P2V_E_ARG, "bad op / null argument");
  OpLayout L;
  RCK(selftest_layout(*R, b, nb, L));
  *item_words = L.in; *out_words = L.out; *b_words = L.b;
  return P2V_OK;
}

int p2v_count_mismatches(const int8_t* results, const int8_t* expect, size_t n, uint64_t* counters, void* stream) {
  if (!counters || (n && (!results || !expect))) return fail(P2V_E_ARG, "null argument");
  const unsigned blocks = n ? (unsigned)((n + 255) / 256) : 1;
  hipLaunchKernelGGL(k_count_mismatches, dim3(blocks), dim3(256), 0, (hipStream_t)stream, results, expect, (int64_t)n,
                     (unsigned long long*)counters);
  HCK(hipGetLastError());
  return P2V_OK;
}

int p2v_clock_probe(uint64_t* stamps, int nblocks, void* stream) {
  if (!stamps || nblocks <= 0) return fail(P2V_E_ARG, "null argument / no blocks");
  hipLaunchKernelGGL(k_clock_probe, dim3((unsigned)nblocks), dim3(64), 0, (hipStream_t)stream, (unsigned long long*)stamps);
  HCK(hipGetLastError());
  return P2V_OK;
}

}  // extern "C"
