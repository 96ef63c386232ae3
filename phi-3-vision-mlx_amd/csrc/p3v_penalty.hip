// Repetition / presence / frequency penalties and logit_bias over bf16 logits: the rule written out above p3v_penalty_row_t in
// include/p3v.h.  p3v_penalize streams: per row it reads the logits (2n bytes), the seen table (4n) and, where the row has one,
// its bias (4n), and writes the adjusted row (2n) to a second buffer -- a grid over (chunk, row), every thread owning 8
// consecutive tokens: one 16-byte logits load, two 16-byte seen loads, two 16-byte bias loads, one 16-byte store.  A row whose
// bases are not all 16-byte aligned, and the last n % 8 tokens of every row, go element by element.  The thread that owns the
// fed token's index counts it before it adjusts: no atomics, no second launch.  p3v_penalty_note is the scatter that (re)builds a
// row's table from token ids: 32-bit vector atomics, behind an optional clear launch on the same stream.
// Every arithmetic step is one correctly rounded fp32 operation (no contraction: the pragma below), so NumPy in float32
// reproduces every output bit.
#include "p3v_common.h"

#define P3V_PEN_THREADS 256
#define P3V_PEN_PER_THREAD 8
#define P3V_PEN_COUNT 0x7fffffffu

__device__ __forceinline__ bf16_t penalty_adjust(bf16_t l, uint32_t seen, float bias, bool biased, const p3v_penalty_row_t& p) {
#pragma clang fp contract(off)
  float a = bf16_to_f32(l);                                               // 1.
  const uint32_t c = seen & P3V_PEN_COUNT;
  if (seen != 0 && p.repetition != 1.0f) a = a > 0.0f ? a / p.repetition : a * p.repetition;   // 2.
  const float f = p.frequency * (float)c;                                 // 3. (rounded on its own)
  a = a - f;
  if (c > 0) a = a - p.presence;                                          // 4.
  if (biased) a = a + bias;                                               // 5.
  return f32_to_bf16(a);                                                  // 6.
}

__device__ __forceinline__ bool aligned16(const void* p) { return (((size_t)p) & 15) == 0; }

__global__ void __launch_bounds__(P3V_PEN_THREADS) k_penalize(const bf16_t* __restrict__ logits, int64_t row_stride,
                                                            const p3v_penalty_row_t* __restrict__ prm, uint32_t* seen,
                                                            int64_t seen_stride, const float* __restrict__ bias, int64_t bias_stride,
                                                            const int32_t* __restrict__ fed, bf16_t* __restrict__ out,
                                                            int64_t out_stride, int n) {
  const size_t r = blockIdx.y;
  const int64_t i0 = ((int64_t)blockIdx.x * P3V_PEN_THREADS + threadIdx.x) * P3V_PEN_PER_THREAD;
  if (i0 >= n) return;
  const p3v_penalty_row_t p = prm[r];
  const bf16_t* __restrict__ src = logits + r * row_stride;
  bf16_t* __restrict__ dst = out + r * out_stride;
  const bool full = i0 + P3V_PEN_PER_THREAD <= n;
  const int m = full ? P3V_PEN_PER_THREAD : (int)(n - i0);                // tokens of this thread that exist
  if (!(p.flags & P3V_PENALTY_ACTIVE)) {                                  // 0. an inactive row: a copy of the bits
    if (full && aligned16(src) && aligned16(dst)) {
      *(u32x4_t*)(dst + i0) = *(const u32x4_t*)(src + i0);
    } else {
      for (int e = 0; e < m; ++e) dst[i0 + e] = src[i0 + e];
    }
    return;
  }
  uint32_t* sn = seen + r * seen_stride;
  const bool biased = (p.flags & P3V_PENALTY_BIAS) && bias != nullptr;
  const float* __restrict__ bs = biased ? bias + r * bias_stride : nullptr;
  const bool vec = full && aligned16(src) && aligned16(dst) && aligned16(sn) && (!biased || aligned16(bs));
  uint32_t lw[4] = {0, 0, 0, 0};                                          // the 8 logits, two per word
  uint32_t s[8];
  float b[8];
  if (vec) {
    const u32x4_t l4 = *(const u32x4_t*)(src + i0);
    const u32x4_t s0 = *(const u32x4_t*)(sn + i0), s1 = *(const u32x4_t*)(sn + i0 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { lw[e] = l4[e]; s[e] = s0[e]; s[4 + e] = s1[e]; }
    if (biased) {
      const f32x4_t b0 = *(const f32x4_t*)(bs + i0), b1 = *(const f32x4_t*)(bs + i0 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { b[e] = b0[e]; b[4 + e] = b1[e]; }
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool in = e < m;
      const uint32_t l = in ? (uint32_t)src[i0 + e] : 0u;
      lw[e >> 1] |= l << (16 * (e & 1));
      s[e] = in ? sn[i0 + e] : 0u;
      b[e] = (in && biased) ? bs[i0 + e] : 0.0f;
    }
  }
  if (!biased) {
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = 0.0f;
  }
  if (fed != nullptr) {                                                   // the token this step was fed: counted by its owner
    const int64_t f = fed[r];
    if (f >= i0 && f < i0 + m) {
      uint32_t v = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (e == (int)(f - i0)) {
          if ((s[e] & P3V_PEN_COUNT) != P3V_PEN_COUNT) s[e] += 1;
          v = s[e];
        }
      }
      sn[f] = v;
    }
  }
  uint32_t ow[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t lo = penalty_adjust((bf16_t)(lw[e] & 0xffffu), s[2 * e], b[2 * e], biased, p);
    const uint32_t hi = penalty_adjust((bf16_t)(lw[e] >> 16), s[2 * e + 1], b[2 * e + 1], biased, p);
    ow[e] = lo | (hi << 16);
  }
  if (vec) {
    const u32x4_t o4 = {ow[0], ow[1], ow[2], ow[3]};
    *(u32x4_t*)(dst + i0) = o4;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e < m) dst[i0 + e] = (bf16_t)((ow[e >> 1] >> (16 * (e & 1))) & 0xffffu);
  }
}

// seen[r, 0..n) = 0 for the given rows: 4 words per thread, 16-byte stores where the row's base allows
__global__ void __launch_bounds__(P3V_PEN_THREADS) k_penalty_clear(uint32_t* __restrict__ seen, int64_t seen_stride, int n) {
  uint32_t* sn = seen + (size_t)blockIdx.y * seen_stride;
  const int64_t i0 = ((int64_t)blockIdx.x * P3V_PEN_THREADS + threadIdx.x) * 4;
  if (i0 >= n) return;
  if (i0 + 4 <= n && aligned16(sn)) {
    const u32x4_t z = {0u, 0u, 0u, 0u};
    *(u32x4_t*)(sn + i0) = z;
  } else {
    for (int64_t i = i0; i < n && i < i0 + 4; ++i) sn[i] = 0u;
  }
}

// the scatter: a grid-stride walk over ids[r, first[r] .. first[r] + count[r]), cut to the row
__global__ void __launch_bounds__(P3V_PEN_THREADS) k_penalty_note(uint32_t* __restrict__ seen, int64_t seen_stride,
                                                                const int32_t* __restrict__ ids, int64_t ids_stride,
                                                                const int32_t* __restrict__ first, const int32_t* __restrict__ count,
                                                                int n, int as_prompt) {
  const size_t r = blockIdx.y;
  const int64_t f = first[r];
  if (f < 0 || f >= ids_stride) return;
  int64_t c = count[r];
  c = c < ids_stride - f ? c : ids_stride - f;
  uint32_t* sn = seen + r * seen_stride;
  const int32_t* row = ids + r * ids_stride + f;
  for (int64_t i = (int64_t)blockIdx.x * P3V_PEN_THREADS + threadIdx.x; i < c; i += (int64_t)gridDim.x * P3V_PEN_THREADS) {
    const int32_t id = row[i];
    if (id < 0 || id >= n) continue;
    if (as_prompt) atomicOr(sn + id, 0x80000000u);
    else atomicAdd(sn + id, 1u);
  }
}

extern "C" int p3v_penalty_note(uint32_t* seen, int64_t seen_stride, const int32_t* ids, int64_t ids_stride, const int32_t* first,
                                const int32_t* count, int rows, int n, int as_prompt, int clear, void* stream) {
  if (!seen || !ids || !first || !count || rows < 1 || rows > 65535 || n < 1 || ids_stride < 0 || seen_stride < n) return P3V_ERR_ARG;
  if (clear) {
    const unsigned chunks = (unsigned)(((int64_t)n + P3V_PEN_THREADS * 4 - 1) / (P3V_PEN_THREADS * 4));
    hipLaunchKernelGGL(k_penalty_clear, dim3(chunks, rows), dim3(P3V_PEN_THREADS), 0, (hipStream_t)stream, seen, seen_stride, n);
    P3V_CHECK_LAUNCH();
  }
  if (ids_stride == 0) return P3V_OK;
  int64_t blocks = (ids_stride + P3V_PEN_THREADS - 1) / P3V_PEN_THREADS;
  blocks = blocks > 64 ? 64 : blocks;
  hipLaunchKernelGGL(k_penalty_note, dim3((unsigned)blocks, rows), dim3(P3V_PEN_THREADS), 0, (hipStream_t)stream, seen, seen_stride, ids,
                     ids_stride, first, count, n, as_prompt);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}

extern "C" int p3v_penalize(const uint16_t* logits, int64_t row_stride, const p3v_penalty_row_t* rows_params, uint32_t* seen,
                            int64_t seen_stride, const float* bias, int64_t bias_stride, const int32_t* fed, uint16_t* out,
                            int64_t out_stride, int rows, int n, void* stream) {
  if (!logits || !rows_params || !seen || !out || out == logits || rows < 1 || rows > 65535 || n < 1 || row_stride < n ||
      seen_stride < n || out_stride < n || (bias && bias_stride < n))
    return P3V_ERR_ARG;
  const int per_block = P3V_PEN_THREADS * P3V_PEN_PER_THREAD;
  const unsigned chunks = (unsigned)(((int64_t)n + per_block - 1) / per_block);
  hipLaunchKernelGGL(k_penalize, dim3(chunks, rows), dim3(P3V_PEN_THREADS), 0, (hipStream_t)stream, logits, row_stride, rows_params,
                     seen, seen_stride, bias, bias_stride, fed, out, out_stride, n);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}
