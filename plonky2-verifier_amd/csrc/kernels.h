// kernels.h — every kernel of libp2v, declared once.  Included by the .hip file that defines a
// kernel (before the definition) and by every host unit that launches one: extern "C" names carry
// no parameter types, so only a declaration both sides see makes a signature changed on one side
// a compile error instead of a kernarg block read at the wrong offsets.  The declarations are
// plain: __launch_bounds__, amdgpu_waves_per_eu and __restrict__ stay on the definitions.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev.h"

// kernels.hip
extern "C" __global__ void k_phase1(DevCircuit, int, int);
extern "C" __global__ void k_phase1_lane(DevCircuit, int, int);
extern "C" __global__ void k_transcript(DevCircuit, int);
extern "C" __global__ void k_transcript_lane(DevCircuit, int);
extern "C" __global__ void k_phase1_keyed(DevCircuit, int, int);
extern "C" __global__ void k_phase1_lane_keyed(DevCircuit, int, int);
extern "C" __global__ void k_transcript_keyed(DevCircuit, int);
extern "C" __global__ void k_transcript_lane_keyed(DevCircuit, int);
extern "C" __global__ void k_leaf(DevCircuit);
// fri.hip
extern "C" __global__ void k_fri(DevCircuit);
extern "C" __global__ void k_status(DevCircuit, int8_t*, uint64_t*, int64_t);
// selftest.hip
extern "C" __global__ void k_selftest(int, const uint64_t*, const uint64_t*, uint64_t*, int64_t);
extern "C" __global__ void k_selftest_forms(int, const uint64_t*, uint64_t*, int64_t);
extern "C" __global__ void k_selftest_hash(int, DevCircuit, const uint64_t*, uint64_t*);
extern "C" __global__ void k_selftest_field(int, DevCircuit, const uint64_t*, uint64_t*);
// merkle.hip
extern "C" __global__ void k_merkle(DevCircuit);
extern "C" __global__ void k_merkle_row(DevCircuit);
extern "C" __global__ void k_merkle_plan(DevCircuit);
extern "C" __global__ void k_merkle_cse(DevCircuit);
extern "C" __global__ void k_merkle_fix(DevCircuit);
extern "C" __global__ void k_merkle_resolve(DevCircuit);
extern "C" __global__ void k_merkle_known(DevCircuit);
extern "C" __global__ void k_merkle_known_miss(DevCircuit);
// vanish.hip, vanish_poseidon.hip, vanish_prog.hip
extern "C" __global__ void k_vanish_r2(DevCircuit);
extern "C" __global__ void k_vanish_rn(DevCircuit);
extern "C" __global__ void k_vanish_poseidon_r2(DevCircuit);
extern "C" __global__ void k_vanish_poseidon_rn(DevCircuit);
extern "C" __global__ void k_vanish_coset_r2(DevCircuit);
extern "C" __global__ void k_vanish_coset_rn(DevCircuit);
extern "C" __global__ void k_vanish_lookup_r2(DevCircuit);
extern "C" __global__ void k_vanish_lookup_rn(DevCircuit);
extern "C" __global__ void k_vanish_prog_r2(DevCircuit);
extern "C" __global__ void k_vanish_prog_rn(DevCircuit);
// (the fourth self-test kernel stays in vanish_prog.hip, not selftest.hip: the interpreter it runs
// is file-local there on purpose, and a header for one 12-line kernel would be more machinery)
extern "C" __global__ void k_selftest_prog(DevCircuit, uint64_t*, int);
extern "C" __global__ void k_lut(DevCircuit);
extern "C" __global__ void k_vanish_final(DevCircuit);
// keys.hip
extern "C" __global__ void k_key_resolve(DevCircuit, uint32_t*);
// util.hip
extern "C" __global__ void k_count_mismatches(const int8_t*, const int8_t*, int64_t, unsigned long long*);
extern "C" __global__ void k_clock_probe(unsigned long long*);
// json_pack.hip
extern "C" __global__ void k_json_pack(const uint8_t*, const uint64_t*, int, const uint8_t*, int64_t, const int32_t*, int64_t, uint64_t*, int64_t, int8_t*);
extern "C" __global__ void k_bytes_pack(const uint8_t*, const uint64_t*, int, const int64_t*, const int64_t*, const int64_t*, int,
                                        const int64_t*, const uint8_t*, int, int64_t, int64_t, int64_t, uint64_t*, int64_t, int8_t*);
