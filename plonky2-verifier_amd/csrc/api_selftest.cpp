// api_selftest.cpp — the device self-tests (p2v_selftest) and the measurement probes of util.hip.
#include "api_internal.hpp"
#include "kernels.h"

extern "C" {

// p2v_selftest ops 12-20: the field and FRI query code on items read as a proof batch is, through
// a DevCircuit that holds the item array and the tables fill_scalars / fri_twiddles make for a
// circuit with FRI arity bits 1..8 (step s = ab - 1).  b words, item words in and out per op;
// the shared words are checked here, so the kernel reads nothing outside an item.
static int selftest_field(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  static const size_t kB[9] = {0, 0, 0, 0, 0, 1, 1, 12, 1}, kIn[9] = {2, 4, 1, 2, 4, 1, 2, 0, 0}, kOut[9] = {5, 2, 1, 2, 4, 1, 2, 2, 2};
  const size_t bw = kB[op - 12], wo = kOut[op - 12];
  size_t w = kIn[op - 12];
  if (bw && !b) return fail(P2V_E_ARG, "bad op / null argument");
  if (op == 17 && b[0] > 32) return fail(P2V_E_ARG, "pow_root: k > 32");
  if (op == 18 && b[0] > 0xFFFFFFFFull) return fail(P2V_E_ARG, "epow_u: e >= 2^32");
  if (op == 19) {
    w = (size_t)b[0];
    bool ok = b[0] >= 2 && b[0] <= (1u << 20) && b[1] <= 5;
    for (int k = 0; k < 5 && ok; k++) ok = b[2 + k] <= b[0] && b[7 + k] <= b[0] - b[2 + k];
    if (!ok) return fail(P2V_E_ARG, "reduce_powers: segment table outside the item");
  }
  if (op == 20) {
    if (b[0] < 1 || b[0] > 8) return fail(P2V_E_ARG, "fold: arity bits outside 1..8");
    w = 2 + (2u << b[0]);
  }
  if (n > (size_t)INT32_MAX - 64) return fail(P2V_E_ARG, "too many items");
  if (n == 0) return P2V_OK;
  Circuit C;
  C.arities = {1, 2, 3, 4, 5, 6, 7, 8};
  C.step_depth.assign(8, 0); C.L.step_evals.assign(8, 0); C.L.step_path.assign(8, 0);
  DevCircuit d{};
  fill_scalars(C, d);
  DevBuf da, db, dout, dtw;
#define SCK(x) HCK_AS("p2v_selftest", x)
  SCK(da.alloc(n * w * 8)); SCK(db.alloc(bw * 8)); SCK(dout.alloc(n * wo * 8));
  SCK(upload(dtw, fri_twiddles(C), d.twiddles));
  SCK(hipMemcpy(da.p, a, n * w * 8, hipMemcpyHostToDevice));
  if (bw) SCK(hipMemcpy(db.p, b, bw * 8, hipMemcpyHostToDevice));
  d.soa = (const uint64_t*)da.p; d.words = (int64_t)w; d.wstride = 1; d.tiled = 0;
  d.n = (int32_t)n; d.B = (int32_t)((n + 63) / 64 * 64);
  hipLaunchKernelGGL(k_selftest_field, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, d, (const uint64_t*)db.p, (uint64_t*)dout.p);
  SCK(hipGetLastError());
  SCK(hipMemcpy(out, dout.p, n * wo * 8, hipMemcpyDeviceToHost));
#undef SCK
  return P2V_OK;
}

// p2v_selftest op 21: the gate-program interpreter (vanish_prog.hip) on items laid out as a proof's
// openings are: b = nwires, nconsts, the program.  The program is checked here as at circuit
// creation, so the kernel reads nothing outside an item and writes no slot past the file; like the
// other ops' shared words, a b that does not pass is P2V_E_ARG, decided before any device call.
static int selftest_prog(int device, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  if (!b) return fail(P2V_E_ARG, "bad op / null argument");
  if (b[0] > (1u << 20) || b[1] > (1u << 20)) return fail(P2V_E_ARG, "gate program rows beyond this build's limits");
  if (n > (size_t)INT32_MAX - 64) return fail(P2V_E_ARG, "too many items");
  const int64_t nw = (int64_t)b[0], nc = (int64_t)b[1];
  GateProgram g;
  std::vector<uint64_t> low;
  try {
    // the encoding's own instruction count bounds the walk: at most 3 words per instruction
    if (b[2] != P2V_WORDS_GATE_MAGIC) throw ParseError("gate program: bad magic / version");
    if (b[3] > (uint64_t)P2V_GATE_PROGRAM_MAX_INSTRS) throw CircuitError("gate program beyond this build's limits (instructions)");
    g = decode_gate_program(b + 2, gate_program_extent(b + 2, 2 + 3 * (size_t)b[3]));
    if (g.max_wire >= nw || g.max_const >= nc) throw CircuitError("(Array.!): gate program reads beyond the row");
    if (g.max_pih >= 4) throw CircuitError("(!!): gate program reads a public-inputs-hash word beyond 4");
    if (lower_gate_program(g, &low) > P2V_GATE_PROGRAM_MAX_LIVE) throw CircuitError("gate program beyond this build's limits (values alive at once)");
  } catch (const std::exception& e) { return fail(P2V_E_ARG, std::string("selftest op 21: ") + e.what()); }
  const int ndev = p2v_device_count();
  if (ndev == 0) return fail(P2V_E_NODEVICE, "no HIP device");
  if (device < 0 || device >= ndev) return fail(P2V_E_ARG, "bad device index");
  if (n == 0 || g.num_commits == 0) return P2V_OK;
  HCK(hipSetDevice(device));
  const size_t w = (size_t)(2 * (nw + nc) + 4), wo = 2 * (size_t)g.num_commits;
  DevCircuit d{};
  d.prog_pih = 2 * (nw + nc);
  d.o_wires = 0; d.o_const = 2 * nw;   // ngroups = nls = 0: Vars::k(i) is constant i
  d.words = (int64_t)w; d.wstride = 1; d.tiled = 0;
  d.n = (int32_t)n; d.B = (int32_t)((n + 63) / 64 * 64);
  DevBuf da, dout, dprog;
#define SCK(x) HCK_AS("p2v_selftest", x)
  SCK(da.alloc(n * w * 8)); SCK(dout.alloc(n * wo * 8));
  SCK(upload(dprog, low, d.gprog));
  SCK(hipMemcpy(da.p, a, n * w * 8, hipMemcpyHostToDevice));
  d.soa = (const uint64_t*)da.p;
  hipLaunchKernelGGL(k_selftest_prog, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, d, (uint64_t*)dout.p, g.num_commits);
  SCK(hipGetLastError());
  SCK(hipMemcpy(out, dout.p, n * wo * 8, hipMemcpyDeviceToHost));
#undef SCK
  return P2V_OK;
}

int p2v_selftest(int device, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  const bool needs_b = op == 0 || op == 3 || op == 4 || op == 6;
  // op 11 was the retired pair form's permutation; the ops keep their numbers
  if (op < 0 || op > 22 || op == 11 || (n && (!a || !out || (needs_b && !b)))) return fail(P2V_E_ARG, "bad op / null argument");
  if (op == 21) return selftest_prog(device, a, b, out, n);
  const int ndev = p2v_device_count();
  if (ndev == 0) return fail(P2V_E_NODEVICE, "no HIP device");
  if (device < 0 || device >= ndev) return fail(P2V_E_ARG, "bad device index");
  if ((op < 12 || op == 22) && n == 0) return P2V_OK;
  HCK(hipSetDevice(device));
  if (op >= 12 && op <= 20) return selftest_field(op, a, b, out, n);
  // words per item of a / b and of out
  const bool scalar = op == 0 || op == 3 || op == 5 || op == 6 || op == 7 || op == 8;
  const size_t w = scalar ? 1 : 12, wo = op == 6 ? 2 : w;
  const size_t bw = op == 4 ? 24 : scalar && needs_b ? n : 2;
  DevBuf da, db, dout;
#define SCK(x) HCK_AS("p2v_selftest", x)
  SCK(da.alloc(n * w * 8)); SCK(db.alloc(bw * 8)); SCK(dout.alloc(n * wo * 8));
  SCK(hipMemcpy(da.p, a, n * w * 8, hipMemcpyHostToDevice));
  if (needs_b) SCK(hipMemcpy(db.p, b, bw * 8, hipMemcpyHostToDevice));
  if (op >= 9) {
    const size_t lanes = op == 9 ? 16 : op == 10 ? 4 : 1;   // op 22: one lane per item
    hipLaunchKernelGGL(k_selftest_forms, dim3((unsigned)((n * lanes + 255) / 256)), dim3(256), 0, 0, op, (const uint64_t*)da.p,
                       (uint64_t*)dout.p, (int64_t)n);
  } else {
    const size_t lanes = op == 8 ? 2 : 1;   // op 8: a lane pair per item
    hipLaunchKernelGGL(k_selftest, dim3((unsigned)((n * lanes + 255) / 256)), dim3(256), 0, 0, op, (const uint64_t*)da.p,
                       (const uint64_t*)db.p, (uint64_t*)dout.p, (int64_t)n);
  }
  SCK(hipGetLastError());
  SCK(hipMemcpy(out, dout.p, n * wo * 8, hipMemcpyDeviceToHost));
#undef SCK
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
