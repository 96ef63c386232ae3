// Arg-max over a bf16 row (first maximum wins, a NaN row reports -1): the ONE definition shared by k_argmax / k_step_end
// (p3v_elementwise.hip) and the greedy rows of the sampler (p3v_sample.hip), so every greedy token is the same bits.
#pragma once
#include "p3v_common.h"

struct ValIdx { float v; int i; };
__device__ __forceinline__ ValIdx better(ValIdx a, ValIdx b) {   // larger value, then smaller index
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
__device__ __forceinline__ ValIdx block_argmax(ValIdx m, ValIdx* red) {
  // wave all-reduce of (value, index) on DPP + row swaps (see wave_sum in p3v_common.h)
#define P3V_ARGMAX_DPP(ctrl)                                                                             \
  {                                                                                                      \
    ValIdx t;                                                                                            \
    t.v = P3V_DPP_F32(m.v, ctrl);                                                                        \
    t.i = __builtin_amdgcn_update_dpp(0, m.i, ctrl, 0xf, 0xf, true);                                     \
    m = better(m, t);                                                                                    \
  }
  P3V_ARGMAX_DPP(0xB1) P3V_ARGMAX_DPP(0x4E) P3V_ARGMAX_DPP(0x124) P3V_ARGMAX_DPP(0x128)
#undef P3V_ARGMAX_DPP
  {
    ValIdx a, b;
    float ia, ib;
    rows_swap32(m.v, a.v, b.v);
    rows_swap32(__builtin_bit_cast(float, m.i), ia, ib);
    a.i = __builtin_bit_cast(int, ia); b.i = __builtin_bit_cast(int, ib);
    m = better(a, b);
    rows_swap16(m.v, a.v, b.v);
    rows_swap16(__builtin_bit_cast(float, m.i), ia, ib);
    a.i = __builtin_bit_cast(int, ia); b.i = __builtin_bit_cast(int, ib);
    m = better(a, b);
  }
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = m;
  __syncthreads();
  ValIdx r = red[0];
  for (int k = 1; k < nw; ++k) r = better(r, red[k]);
  return r;
}

// per-thread argmax over a bf16 row with 16-byte loads (all of a thread's loads are independent: one memory round
// trip for a 32064-wide row on 1024 threads); first maximum wins
__device__ __forceinline__ ValIdx row_argmax_partial(const bf16_t* __restrict__ r, int n) {
  ValIdx m = {-INFINITY, 0x7fffffff};
  // A NaN logit means a kernel upstream failed (the split-KV merge poisons its output when its bounded wait runs out).
  // It enters the reduction as (+inf, index -1), which beats every real entry: the row's arg-max is then -1 instead of
  // an arbitrary index, and the host loops raise on a negative token (api._rows) -- loud, not a silently wrong token.
  auto take = [&](float v, int i) {
    if (v != v) { v = INFINITY; i = -1; }
    if (v > m.v || (v == m.v && i < m.i) || m.i == 0x7fffffff) { m.v = v; m.i = i; }
  };
  if ((((size_t)r) & 15) == 0) {
    const int nv = n >> 3;
    const u32x4_t* rv = (const u32x4_t*)r;
#pragma unroll 4
    for (int c = threadIdx.x; c < nv; c += blockDim.x) {
      const u32x4_t w = rv[c];
#pragma unroll
      for (int j = 0; j < 4; ++j) { take(bf16lo(w[j]), 8 * c + 2 * j); take(bf16hi(w[j]), 8 * c + 2 * j + 1); }
    }
    for (int i = (nv << 3) + threadIdx.x; i < n; i += blockDim.x) take(bf16_to_f32(r[i]), i);
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) take(bf16_to_f32(r[i]), i);
  }
  return m;
}
