// vanish_prog.hip — the vanishing class of the gates whose constraints are a caller's program
// (include/p2v.h "gate programs"): a wave-uniform interpreter of the lowered program
// (circuit.hpp lower_gate_program), one lane per proof, inside vanish_item's frame (Acc, the
// alpha^first start, the selector filter and alpha^G0 after the program, vparts: vanish.h).
//
// The instruction words are the same for every lane of a wave and are fetched by scalar loads
// (ProgPtr below).  The values a program keeps are in LDS, [slot][word][lane]: a per-lane array
// indexed by the instruction stream would be scratch memory.  A lane touches
// only its own column, so the accesses need no barrier and have no bank conflicts (consecutive
// lanes, consecutive u64).
// P2V_PROG_SLOTS slots of two u64 for 64 lanes: 32 KB per one-wave work-group, static.
// WIRE / CONST / PIHASH / LIT values are operand kinds and occupy no slot.
#include "vanish.h"
#include "kernels.h"

using namespace p2d;
using gl::E;

namespace {

enum { PK_SLOT = 0, PK_WIRE = 1, PK_CONST = 2, PK_PIHASH = 3, PK_LIT = 4 };   // circuit.hpp GPK_*
enum { PO_ADD = 4, PO_SUB = 5, PO_MUL = 6, PO_IMG = 7, PO_COMMIT = 8 };       // circuit.hpp GateOp

typedef uint64_t ProgSlots[P2V_PROG_SLOTS][2][64];
// the program through the constant address space: read-only for the whole launch and indexed
// uniformly, so every instruction word is a scalar load (through the plain pointer of the kernel
// argument the compiler takes vector loads, one copy per lane)
typedef const __attribute__((address_space(4))) uint64_t* ProgPtr;

__device__ __forceinline__ E prog_operand(const Vars& V, ProgSlots& S, int lane, uint32_t kind, uint64_t x) {
  const DevCircuit& c = *V.c;
  switch (kind) {
    case PK_SLOT: { const uint32_t s = (uint32_t)x & (P2V_PROG_SLOTS - 1); return E{S[s][0][lane], S[s][1][lane]}; }
    case PK_WIRE: return V.w((int64_t)x);
    case PK_CONST: return V.k((int64_t)x);
    case PK_PIHASH: return gl::eb(c.prog_pih < 0 ? chal(c, CH_PI(c) + (int64_t)x, V.p) : ld(c, c.prog_pih + (int64_t)x, V.p));
    default: return gl::eb(x);   // PK_LIT: reduced mod p by the host
  }
}

// run the lowered program at `prog`; commit(e) receives the constraints in order
template <class Commit>
__device__ __forceinline__ void prog_run(const uint64_t* program, const Vars& V, ProgSlots& S, Commit&& commit) {
  const int lane = threadIdx.x & 63;
  ProgPtr prog = (ProgPtr)program;
  const int n = (int)prog[0];
  ProgPtr ip = prog + 1;
#pragma unroll 1
  for (int i = 0; i < n; i++, ip += 3) {
    const uint32_t h = (uint32_t)ip[0];
    const uint32_t op = h & 0xFF, dst = (h >> 8) & (P2V_PROG_SLOTS - 1), ka = (h >> 16) & 0xFF, kb = h >> 24;
    const E a = prog_operand(V, S, lane, ka, ip[1]);
    if (op == PO_COMMIT) { commit(a); continue; }
    E v;
    if (op == PO_IMG) v = E{gl::mul_small(a.b, 7), a.a};   // (0, 1) (a, b) = (7 b, a), X^2 = 7
    else {
      const E b = prog_operand(V, S, lane, kb, ip[2]);
      v = op == PO_ADD ? gl::eadd(a, b) : op == PO_SUB ? gl::esub(a, b) : gl::emul(a, b);
    }
    S[dst][0][lane] = v.a; S[dst][1][lane] = v.b;
  }
}

template <int R>
__device__ __forceinline__ void gate_program(const DevCircuit& c, const Vars& V, Acc<R>& A, int g) {
  __shared__ ProgSlots slots;
  prog_run(c.gprog + c.gate_poff[g], V, slots, [&](E e) { A.push(e); });
}

}  // namespace

// One-wave work-groups beside k_merkle, like the other side-stream classes (vanish.hip).  Their
// P2V_SIDE_ATTR asks for 5 waves per SIMD; here the slot file bounds a CU at 160 / 32 = 5
// work-groups whatever the registers, so the attribute could not be met (the compiler says so)
// and is left out: what matters beside k_merkle is the register file a wave takes, <= 112 VGPRs
// like the others (68 and 100 as compiled, tools/resource_usage.py).
extern "C" __global__ void __launch_bounds__(64) k_vanish_prog_r2(DevCircuit c) { vanish_body<VK_PROG, P2V_R_STD>(c); }
extern "C" __global__ void __launch_bounds__(64) k_vanish_prog_rn(DevCircuit c) { vanish_body<VK_PROG, P2V_MAX_R>(c); }

// p2v_selftest op 21: the interpreter on caller-chosen rows, one lane per item.  c.soa holds the
// items (wires, then constants, F^2 each, then the 4 hash words at c.prog_pih), c.gprog one
// lowered program; out = [n][2 ncommit].  One-wave work-groups: the slot file is one wave's.
extern "C" __global__ void __launch_bounds__(64) k_selftest_prog(DevCircuit c, uint64_t* out, int ncommit) {
  __shared__ ProgSlots slots;
  const int p = blockIdx.x * 64 + (threadIdx.x & 63);
  const bool live = p < c.n;
  Vars V{&c, p};
  uint64_t* dst = out + (int64_t)(live ? p : 0) * 2 * ncommit;
  int k = 0;
  prog_run(c.gprog, V, slots, [&](E e) {
    if (live && k < ncommit) { dst[2 * k] = e.a; dst[2 * k + 1] = e.b; }
    k++;
  });
}
