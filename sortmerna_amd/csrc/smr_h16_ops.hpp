// smr_h16_ops.hpp -- packed f16 arithmetic for k_sw16h (smr_walk.hpp): v_pk_add_f16 and v_pk_maximum3_f16, the three-operand maximum gfx950
// has for packed halves of f16 but not for packed 16-bit integers.  Every value the Smith-Waterman recurrence puts through these is an
// integer of magnitude <= 2048, which f16 (11 significant bits) holds exactly, so sums and maxima are those of the integer kernel.
// Included as <smr_h16_ops.hpp>: the kernel emulator of the test suite puts its own file of this name in front
// (tests/emu/shim/smr_h16_ops.hpp, scalar host code on bit patterns with a correctly rounded conversion).
#pragma once
#include <stdint.h>

namespace smr {

typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ h16x2 h2_from(uint32_t v) { return __builtin_bit_cast(h16x2, v); }
__device__ __forceinline__ uint32_t h2_bits(h16x2 v) { return __builtin_bit_cast(uint32_t, v); }
// the f16 encoding of an integer (exact for |v| <= 2048) and the integer an encoding stands for
__device__ __forceinline__ uint32_t h16_of_int(int v) { return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)(float)v); }
__device__ __forceinline__ int h16_to_int(uint32_t half) { return (int)(float)__builtin_bit_cast(_Float16, (unsigned short)half); }
__device__ __forceinline__ h16x2 h2_splat(int v) { return h2_from(h16_of_int(v) * 0x00010001u); }
__device__ __forceinline__ h16x2 h2_add(h16x2 a, h16x2 b) { return a + b; }
__device__ __forceinline__ h16x2 h2_sub(h16x2 a, h16x2 b) { return a - b; }
// one v_pk_maximum3_f16 (no value here is a NaN, and none is -0: sums of integers that cancel give +0)
__device__ __forceinline__ h16x2 h2_max3(h16x2 a, h16x2 b, h16x2 c) { return __builtin_elementwise_maximum(__builtin_elementwise_maximum(a, b), c); }
// the maximum of two as max3(a, b, b): the same instruction, whose operands need no canonicalising first
__device__ __forceinline__ h16x2 h2_max(h16x2 a, h16x2 b) { return h2_max3(a, b, b); }

}  // namespace smr
