// Token log-probabilities over bf16 logits: the rule written out above p3v_logprob_t in include/p3v.h.
// One 1024-thread workgroup per row, as k_sample (p3v_sample.hip): the row is read once with 16-byte loads and stays in registers
// as 16-bit order keys, two per register (32 values per thread up to n = 32768, 64 up to 65536).  Every (value, index) pair of a row
// fits ONE 32-bit word -- order key << 16 | (65535 - index), n <= 65536 -- whose unsigned order is the rule's order (larger value
// first, then the lower index): the rank is a count of larger words and the top-N list N rounds of a block-wide unsigned maximum
// below the previous pick.  The normaliser is step 3 of the sampling rule at T = 1: integer weights, so their sum -- and with it
// every bit of the record -- does not depend on the reduction order, the launch geometry, the batch or graph versus eager execution.
// Nothing here writes to the logits or to the step's loop state.
#include "p3v_common.h"

#define P3V_LP_THREADS 1024
#define P3V_LP_MAX_N 65536
#define P3V_LP_KEY_NINF 0x007fu     // order key of -inf
#define P3V_LP_KEY_PINF 0xff80u     // order key of +inf

// the 16-bit order key of p3v_sample.hip: orders the non-NaN bf16 values as floats do (-0 == +0); key 0 = a padding slot
__device__ __forceinline__ uint32_t lp_order_key(uint32_t b) {
  b = b == 0x8000u ? 0u : b;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}
__device__ __forceinline__ float lp_key_value(uint32_t k) {
  return bf16_to_f32((bf16_t)((k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu)));
}

// integer wave all-reduces on the DPP + row-swap pattern of wave_sum (p3v_common.h); the words travel as raw bits
__device__ __forceinline__ uint32_t lp_swap_max(uint32_t v) {
  float a, b;
  rows_swap32(__uint_as_float(v), a, b);
  v = max(__float_as_uint(a), __float_as_uint(b));
  rows_swap16(__uint_as_float(v), a, b);
  return max(__float_as_uint(a), __float_as_uint(b));
}
__device__ __forceinline__ uint32_t lp_wave_max_u32(uint32_t v) {
#define P3V_LP_DPP(ctrl) v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, 0xf, 0xf, true));
  P3V_LP_DPP(0xB1) P3V_LP_DPP(0x4E) P3V_LP_DPP(0x124) P3V_LP_DPP(0x128)
#undef P3V_LP_DPP
  return lp_swap_max(v);
}
__device__ __forceinline__ uint64_t lp_u64_of(float lo, float hi) {
  return ((uint64_t)__float_as_uint(hi) << 32) | __float_as_uint(lo);
}
__device__ __forceinline__ uint64_t lp_wave_sum_u64(uint64_t v) {
#define P3V_LP_DPP(ctrl)                                                                                    \
  {                                                                                                         \
    const uint32_t lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, ctrl, 0xf, 0xf, true);             \
    const uint32_t hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), ctrl, 0xf, 0xf, true);     \
    v += ((uint64_t)hi << 32) | lo;                                                                         \
  }
  P3V_LP_DPP(0xB1) P3V_LP_DPP(0x4E) P3V_LP_DPP(0x124) P3V_LP_DPP(0x128)
#undef P3V_LP_DPP
  float a0, b0, a1, b1;
  rows_swap32(__uint_as_float((uint32_t)v), a0, b0);
  rows_swap32(__uint_as_float((uint32_t)(v >> 32)), a1, b1);
  v = lp_u64_of(a0, a1) + lp_u64_of(b0, b1);
  rows_swap16(__uint_as_float((uint32_t)v), a0, b0);
  rows_swap16(__uint_as_float((uint32_t)(v >> 32)), a1, b1);
  return lp_u64_of(a0, a1) + lp_u64_of(b0, b1);
}

struct LogprobSmem {
  uint64_t red[2][16];        // double-buffered, one barrier per reduction: a buffer is rewritten two reductions later, after
  uint32_t ured[2][16];       // every thread has passed the barrier in between
  float fred[16];
  p3v_logprob_t rec;
};

__device__ __forceinline__ uint64_t lp_block_sum(uint64_t v, LogprobSmem& sm, int& par) {
  v = lp_wave_sum_u64(v);
  if ((threadIdx.x & 63) == 0) sm.red[par][threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t t = 0;
#pragma unroll
  for (int w = 0; w < P3V_LP_THREADS / 64; ++w) t += sm.red[par][w];
  par ^= 1;
  return t;
}
__device__ __forceinline__ uint32_t lp_block_max(uint32_t v, LogprobSmem& sm, int& par) {
  v = lp_wave_max_u32(v);
  if ((threadIdx.x & 63) == 0) sm.ured[par][threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = 0;
#pragma unroll
  for (int w = 0; w < P3V_LP_THREADS / 64; ++w) t = max(t, sm.ured[par][w]);
  par ^= 1;
  return t;
}

// The record of one row -> *out (device or pinned host memory), by 20 plain 4-byte stores.  J = 16-byte chunks per thread
// (n <= 8192 * J); slot s of a thread holds index 8 * (tid + 1024 * (s >> 3)) + (s & 7).
template <int J>
__device__ __forceinline__ void logprob_row(const bf16_t* __restrict__ row, int n, int t, int N, p3v_logprob_t* __restrict__ out,
                                            LogprobSmem& sm) {
  const int tid = threadIdx.x;
  const bool vec = (((size_t)row) & 15) == 0;
  uint32_t kp[4 * J];                                     // the order keys, two per register
  uint32_t kmax = 0, nan = 0;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int c = tid + P3V_LP_THREADS * j;
    uint32_t raw[8];
    if (vec && 8 * c + 8 <= n) {
      const u32x4_t w = ((const u32x4_t*)row)[c];
#pragma unroll
      for (int e = 0; e < 4; ++e) { raw[2 * e] = w[e] & 0xffffu; raw[2 * e + 1] = w[e] >> 16; }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) raw[e] = 8 * c + e < n ? (uint32_t)row[8 * c + e] : 0xffffffffu;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t b = raw[e];
      uint32_t k = 0;
      if (b != 0xffffffffu) {
        if ((b & 0x7fffu) > 0x7f80u) nan = 1;
        else k = lp_order_key(b);
      }
      if (e & 1) kp[4 * j + e / 2] |= k << 16;
      else kp[4 * j + e / 2] = k;
      kmax = k > kmax ? k : kmax;
    }
  }
#define P3V_LP_KEY(s) (((s) & 1) ? kp[(s) >> 1] >> 16 : kp[(s) >> 1] & 0xffffu)
#define P3V_LP_IDX(s) (8 * (tid + P3V_LP_THREADS * ((s) >> 3)) + ((s) & 7))
  // 1 / 2. NaN flag and the largest value in one reduction (keys and the flag are exact in fp32)
  const float top = block_max((float)kmax + (nan ? 65536.f : 0.f), sm.fred);
  const uint32_t ktop = (uint32_t)top;
  const float qnan = __uint_as_float(0x7fc00000u);
  const bool in_range = t >= 0 && t < n;
  float lp = qnan;
  int rank = 0, n_top = 0;
  if (tid < 8) { sm.rec.top_id[tid] = -1; sm.rec.top_logprob[tid] = qnan; }
  if (top < 65536.f && ktop < P3V_LP_KEY_PINF && ktop > P3V_LP_KEY_NINF) {
    int par = 0;
    // 3 / 4. W = the sum of the integer weights (fp64 exponential; below 2^-32 of the top token's: 0)
    const double md = (double)lp_key_value(ktop);
    uint64_t part = 0;
#pragma unroll
    for (int s = 0; s < 8 * J; ++s) {
      const uint32_t k = P3V_LP_KEY(s);
      if (k > P3V_LP_KEY_NINF) {
        const double d = (double)lp_key_value(k) - md;
        if (d >= -22.25) part += (uint64_t)floor(exp(d) * 4294967296.0);    // exp(-22.25) * 2^32 < 1
      }
    }
    const uint64_t W = lp_block_sum(part, sm, par);
    // 5. (32 ln 2: the product is exact)
    const double lse = md + log((double)W) - 32.0 * 0.6931471805599453094;
    // 6 / 7. the scored token: its log-probability, and its rank as the count of (value, index) words above its own
    if (in_range) {
      const uint32_t kt = lp_order_key(row[t]);
      const uint32_t ct = kt << 16 | (uint32_t)(65535 - t);
      uint32_t cnt = 0;
#pragma unroll
      for (int s = 0; s < 8 * J; ++s) {
        const uint32_t k = P3V_LP_KEY(s);
        cnt += k != 0 && (k << 16 | (uint32_t)(65535 - P3V_LP_IDX(s))) > ct;
      }
      rank = 1 + (int)lp_block_sum(cnt, sm, par);
      lp = (float)((double)lp_key_value(kt) - lse);
    }
    // 8. top-N: each round takes the largest word below the previous pick
    n_top = N < n ? N : n;
    uint32_t last = 0xffffffffu;
    for (int r = 0; r < n_top; ++r) {
      uint32_t best = 0;
#pragma unroll
      for (int s = 0; s < 8 * J; ++s) {
        const uint32_t k = P3V_LP_KEY(s);
        const uint32_t c = k << 16 | (uint32_t)(65535 - P3V_LP_IDX(s));
        best = (k != 0 && c < last && c > best) ? c : best;
      }
      last = lp_block_max(best, sm, par);
      if (tid == 0) {
        sm.rec.top_id[r] = 65535 - (int)(last & 0xffffu);
        sm.rec.top_logprob[r] = (float)((double)lp_key_value(last >> 16) - lse);
      }
    }
  }
#undef P3V_LP_KEY
#undef P3V_LP_IDX
  if (tid == 0) {
    sm.rec.token = t;
    sm.rec.logprob = lp;
    sm.rec.rank = rank;
    sm.rec.n_top = n_top;
  }
  __syncthreads();
  if (tid < (int)(sizeof(p3v_logprob_t) / 4)) ((uint32_t*)out)[tid] = ((const uint32_t*)&sm.rec)[tid];
}

template <int J>
__global__ void __launch_bounds__(P3V_LP_THREADS) k_logprobs(const bf16_t* __restrict__ logits, int64_t stride,
                                                            const int32_t* __restrict__ token, const int32_t* __restrict__ want,
                                                            p3v_logprob_t* __restrict__ out, int n) {
  __shared__ LogprobSmem sm;
  const size_t r = blockIdx.x;
  const int N = want[r];
  if (N < 0) return;                                       // a row nobody asked about: one early exit
  logprob_row<J>(logits + r * stride, n, token[r], N < P3V_LOGPROBS_MAX ? N : P3V_LOGPROBS_MAX, out + r, sm);
}

// the launch after a step's tail: next_tok[b] is the emitted token, *d_step already counts it
template <int J>
__global__ void __launch_bounds__(P3V_LP_THREADS) k_logprobs_step(const bf16_t* __restrict__ logits,
                                                                 const int32_t* __restrict__ next_tok,
                                                                 const int32_t* __restrict__ want, const int32_t* __restrict__ d_step,
                                                                 p3v_logprob_t* __restrict__ records, int n, int max_steps) {
  __shared__ LogprobSmem sm;
  const size_t b = blockIdx.x;
  const int N = want[b];
  const int s = *d_step - 1;
  if (N < 0 || s < 0 || s >= max_steps) return;
  logprob_row<J>(logits + b * (size_t)n, n, next_tok[b], N < P3V_LOGPROBS_MAX ? N : P3V_LOGPROBS_MAX,
                 records + b * (size_t)max_steps + s, sm);
}

extern "C" int p3v_logprobs(const uint16_t* logits, int64_t row_stride, const int32_t* token, const int32_t* want,
                            p3v_logprob_t* out, int rows, int n, void* stream) {
  if (!logits || !token || !want || !out || rows < 1 || n < 1 || n > P3V_LP_MAX_N || row_stride < n) return P3V_ERR_ARG;
  if (n <= 32768)
    hipLaunchKernelGGL(k_logprobs<4>, dim3(rows), dim3(P3V_LP_THREADS), 0, (hipStream_t)stream, logits, row_stride, token, want, out, n);
  else
    hipLaunchKernelGGL(k_logprobs<8>, dim3(rows), dim3(P3V_LP_THREADS), 0, (hipStream_t)stream, logits, row_stride, token, want, out, n);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}

extern "C" int p3v_logprobs_step(const uint16_t* logits, const int32_t* next_tok, const int32_t* want, const int32_t* d_step,
                                 p3v_logprob_t* records, int B, int n, int max_steps, void* stream) {
  if (!logits || !next_tok || !want || !d_step || !records || B < 1 || n < 1 || n > P3V_LP_MAX_N || max_steps < 1)
    return P3V_ERR_ARG;
  if (n <= 32768)
    hipLaunchKernelGGL(k_logprobs_step<4>, dim3(B), dim3(P3V_LP_THREADS), 0, (hipStream_t)stream, logits, next_tok, want, d_step,
                       records, n, max_steps);
  else
    hipLaunchKernelGGL(k_logprobs_step<8>, dim3(B), dim3(P3V_LP_THREADS), 0, (hipStream_t)stream, logits, next_tok, want, d_step,
                       records, n, max_steps);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}
