// What the decode attention launchers of p3v_attention.hip and p3v_attn_family.hip share: ONE definition of the rotation of a
// new query / key chunk (the appended K row is the same bits whichever launcher appends it), of the merge launch's block size,
// and the declaration of the merge kernel (defined in p3v_attention.hip; p3v_attn_prompt.hip launches it for p3v_attention's split mode).
#pragma once
#include "p3v_common.h"

constexpr int CMB_G = 16;   // max 64-lane groups of the split-KV merge kernel
static inline int combine_threads(int n_split, int g) {       // measured at 41 splits: 8 groups beat 4 and 16
  if (g > 0) return 64 * g;                                   // g: the combine_g tuning knob (4 / 8 / 16)
  return 64 * (n_split <= 8 ? 4 : 8);
}
static inline int combine_threads(int n_split) { return combine_threads(n_split, p3v_tuning().combine_g); }
__global__ void k_attn_combine2(const float* __restrict__ ws, bf16_t* __restrict__ out, int L, int nh, int hd, int n_split);

typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_f16x2(float lo, float hi) {
  const f16x2_t r = {(_Float16)lo, (_Float16)hi};
  return __builtin_bit_cast(uint32_t, r);
}

template <bool F16 = false>
__device__ __forceinline__ u32x4_t rope_chunk(const bf16_t* head_row, int c, const float* ct, const float* st) {
  // rotated 8-wide chunk c (0..11) of a 96-wide head: low half pairs with +48, high half with -48
  constexpr int HALF = 48;
  const int d0 = c * 8, lo = d0 < HALF;
  const u32x4_t x0 = *(const u32x4_t*)(head_row + d0);
  const u32x4_t x1 = *(const u32x4_t*)(head_row + (lo ? d0 + HALF : d0 - HALF));
  const int tb = lo ? d0 : d0 - HALF;
  const float4 c0 = *(const float4*)(ct + tb), c1 = *(const float4*)(ct + tb + 4);
  const float4 s0 = *(const float4*)(st + tb), s1 = *(const float4*)(st + tb + 4);
  const float cs[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  const float sn[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
  const float sg = lo ? -1.f : 1.f;
  u32x4_t o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float v0 = bf16lo(x0[j]) * cs[2 * j] + sg * bf16lo(x1[j]) * sn[2 * j];
    const float v1 = bf16hi(x0[j]) * cs[2 * j + 1] + sg * bf16hi(x1[j]) * sn[2 * j + 1];
    o[j] = F16 ? pack_f16x2(v0, v1) : pack_bf16x2(v0, v1);
  }
  return o;
}
