// bf16 weights as exact 13-bit codes: the container layout and the decode shared by the streaming GEMV on packed
// weights (GemvB13, p3v_gemv_b13.hip) and the pack / unpack kernels next to it.
//
// A bf16 weight s | e8 | m7 becomes s | q5 | m7: q = 0 for +-0, q = e - base + 1 (1 .. 31) for biased exponent e, `base` one per matrix.
// The 13 bits of a weight are stored in three planes:
//   low byte   q0 | m7            (the low byte of the bf16 value with the exponent's low bit replaced by the code's)
//   nibble     q >> 1
//   sign       1 bit
// A CONTAINER holds one pipeline stage of one row pair of gemv_stream_body -- rows (r0, r1), CH lane loads of 64 lanes x 8 weights each --
// as D = 13 * CH / 2 dwords per lane (39 at CH = 6, 26 at CH = 4), stored instruction-major so that every load instruction of a wave
// covers one contiguous run:
//   NS = D - 6 * CH dwords of signs per lane      one 12-byte (CH = 6) or 8-byte (CH = 4) lane load          64 * NS * 4 bytes
//   CH / 2 nibble loads of 16 bytes per lane      load i: { r0 chunk 2i, r1 chunk 2i, r0 chunk 2i+1, r1 chunk 2i+1 }, 8 nibbles a dword
//   CH low-byte loads of 16 bytes per lane        load j: { r0 weights 0-3, r0 weights 4-7, r1 weights 0-3, r1 weights 4-7 } of chunk j
// Lane l of load j holds the 8 weights of 16-byte chunk (stage * CH + j) * 64 + l of its row: exactly what the bf16 stream hands that lane.
// Within a nibble dword, nibble 2b is weight b, nibble 2b + 1 weight 4 + b (b = 0 .. 3): one AND (or shift + AND) yields the four high
// bytes of a half chunk.  Sign of weight b of half-chunk group G = row * 2 * CH + 2 * j + half sits in sign dword G / 8 at bit
// 8 * b + 7 - G % 8: one shift puts the four of a group on the top bits of the four bytes.
// Containers follow one another by (unit u, stage s): a matrix of R rows takes R * K * 13 / 8 bytes.
#pragma once
#include "p3v_common.h"

template <int CH> struct B13 {
  static_assert(CH == 4 || CH == 6, "a container is 26 or 39 dwords per lane");
  static constexpr int D = 13 * CH / 2, NS = D - 6 * CH;
  static constexpr int NIB_OFF = 64 * NS, LO_OFF = NIB_OFF + (CH / 2) * 256, DWORDS = 64 * D;   // dword offsets inside a container
  static __host__ __device__ constexpr int sign_word(int row, int j, int half) { return (row * 2 * CH + 2 * j + half) >> 3; }
  static __host__ __device__ constexpr int sign_shift(int row, int j, int half) { return (row * 2 * CH + 2 * j + half) & 7; }
};

typedef unsigned short b13_u16x2_t __attribute__((ext_vector_type(2)));

// eight weights as s | 000 | q5 | m7 in bf16 positions: lo0 / lo1 = low bytes of weights 0-3 / 4-7, nib = their 8 nibbles, sg0 / sg1 =
// the sign dword shifted so that the group's four signs are bits 7, 15, 23, 31.  Read as bf16 this is the weight times 2^-(base - 1),
// exactly: the code q (1 .. 31) is a normal number's exponent field and code 0 is +-0.  The GEMV whose activations carry 2^(base - 1)
// (GemvB13<true>) feeds it to v_dot2c as it is.
// (four scalars, not a u32x4: hipcc 7.2 folds `bit_cast<2 x u16>(v[d])` of a vector's four dwords into element 0, see p3v_dot_bf16.h)
__device__ __forceinline__ void b13_pre8(uint32_t lo0, uint32_t lo1, uint32_t nib, uint32_t sg0, uint32_t sg1, uint32_t (&pre)[4]) {
  const uint32_t hi0 = (sg0 & 0x80808080u) | (nib & 0x0f0f0f0fu), hi1 = (sg1 & 0x80808080u) | ((nib >> 4) & 0x0f0f0f0fu);
  pre[0] = __builtin_amdgcn_perm(hi0, lo0, 0x05010400u);
  pre[1] = __builtin_amdgcn_perm(hi0, lo0, 0x07030602u);
  pre[2] = __builtin_amdgcn_perm(hi1, lo1, 0x05010400u);
  pre[3] = __builtin_amdgcn_perm(hi1, lo1, 0x07030602u);
}

// eight weights back to bf16: b13_pre8 + the base, cc = ((base - 1) << 7) in both halves.  12-bit code | mantissa + cc is the
// bf16 magnitude unless the code is 0 (then the magnitude is 0): min(v, 1) * cc adds it only to the others, two weights per instruction.
__device__ __forceinline__ u32x4_t b13_decode8(uint32_t lo0, uint32_t lo1, uint32_t nib, uint32_t sg0, uint32_t sg1, uint32_t cc) {
  uint32_t pre[4];
  b13_pre8(lo0, lo1, nib, sg0, sg1, pre);
  const b13_u16x2_t c2 = __builtin_bit_cast(b13_u16x2_t, cc), one = {1, 1}, mag = {0x7fff, 0x7fff};
  u32x4_t w;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const b13_u16x2_t p = __builtin_bit_cast(b13_u16x2_t, pre[d]);
    // (as instructions: from `min(v, 1) * cc` hipcc derives a compare + select per 16-bit half, six VALU operations a dword instead of two)
    b13_u16x2_t n, r;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(n) : "v"(p & mag), "v"(one));
    asm("v_pk_mad_u16 %0, %1, %2, %3" : "=v"(r) : "v"(n), "v"(c2), "v"(p));
    w[d] = __builtin_bit_cast(uint32_t, r);
  }
  return w;
}
