// Seeded sampling (temperature, top-k, top-p) over bf16 logits: the rule written out above p3v_sample_row_t in include/p3v.h.
// One 1024-thread workgroup per row; the row stays in registers (32 bf16 values per thread at n = 32768, loaded with the 16-byte
// loads of row_argmax_partial).  The top-k and top-p cuts are found by bisection on the 16-bit order key of the bf16 values (16
// block-wide counts / uint64 masses each -- a row's logits sit in a few exponent bins, so a 256-bin LDS histogram would serialise
// its atomics on one address), the draw by bisection on the 16-byte chunk index (12 masked sums) and a walk over the chosen chunk.
// After the fp64 weights everything is integer arithmetic and there are no float atomics: every launch gives the same bits.
// Greedy rows (T <= 0) take the arg-max through the shared reduction of p3v_argmax (p3v_argmax.h).
#include "p3v_common.h"
#include "p3v_argmax.h"

#define P3V_SAMPLE_THREADS 1024
#define P3V_SAMPLE_MAX_N 32768          // 4 chunks of 8 values per thread
#define P3V_SAMPLE_MAX_ROWS 1024
#define P3V_SAMPLE_CHUNKS (P3V_SAMPLE_MAX_N / 8)
// key of slot s, unpacked afresh at each use: the empty asm keeps the compiler from hoisting 32 unpacked keys out of the bisection
// loops (they would stay live next to the packed ones and the weights, and spill)
__device__ __forceinline__ uint32_t unpack_key(uint32_t w, int hi) {
  asm volatile("" : "+v"(w));
  return hi ? w >> 16 : w & 0xffffu;
}
#define P3V_KEY(s) unpack_key(kp[(s) >> 1], (s) & 1)

// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants), output word 0
__device__ __forceinline__ uint32_t philox4x32_10_w0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
  }
  return c0;
}

// 16-bit key that orders the non-NaN bf16 values as floats do (-0 == +0); key 0 lies below -inf (0x007f): padding slots
__device__ __forceinline__ uint32_t bf16_order_key(uint32_t b) {
  b = b == 0x8000u ? 0u : b;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}
__device__ __forceinline__ float order_key_value(uint32_t k) {
  return bf16_to_f32((bf16_t)((k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu)));
}

// uint64 wave all-reduce on the DPP + row-swap pattern of wave_sum (p3v_common.h), both halves moved as raw bits
__device__ __forceinline__ uint64_t u64_of(float lo, float hi) {
  return ((uint64_t)__float_as_uint(hi) << 32) | __float_as_uint(lo);
}
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#define P3V_DPP_U64(ctrl)                                                                                   \
  {                                                                                                         \
    const uint32_t lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, ctrl, 0xf, 0xf, true);             \
    const uint32_t hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), ctrl, 0xf, 0xf, true);     \
    v += ((uint64_t)hi << 32) | lo;                                                                         \
  }
  P3V_DPP_U64(0xB1) P3V_DPP_U64(0x4E) P3V_DPP_U64(0x124) P3V_DPP_U64(0x128)
#undef P3V_DPP_U64
  float a0, b0, a1, b1;
  rows_swap32(__uint_as_float((uint32_t)v), a0, b0);
  rows_swap32(__uint_as_float((uint32_t)(v >> 32)), a1, b1);
  v = u64_of(a0, a1) + u64_of(b0, b1);
  rows_swap16(__uint_as_float((uint32_t)v), a0, b0);
  rows_swap16(__uint_as_float((uint32_t)(v >> 32)), a1, b1);
  return u64_of(a0, a1) + u64_of(b0, b1);
}

struct SampleSmem {
  uint64_t red[2][16];        // double-buffered: one barrier per reduction (a buffer is rewritten two reductions later, after
  float fred[16];             // every thread has passed the barrier in between, i.e. finished reading it)
  ValIdx vred[16];
  int tok;
};

__device__ __forceinline__ uint64_t block_sum_u64(uint64_t v, SampleSmem& sm, int& par) {
  v = wave_sum_u64(v);
  if ((threadIdx.x & 63) == 0) sm.red[par][threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t t = 0;
#pragma unroll
  for (int w = 0; w < P3V_SAMPLE_THREADS / 64; ++w) t += sm.red[par][w];
  par ^= 1;
  return t;
}

// The token of one row (every thread returns it).  Slot s of a thread holds index 8 * (tid + 1024 * (s >> 3)) + (s & 7).
__device__ __forceinline__ int sample_row(const bf16_t* __restrict__ row, int n, const p3v_sample_row_t prm, SampleSmem& sm) {
  const int tid = threadIdx.x;
  const bool vec = (((size_t)row) & 15) == 0;
  uint32_t kp[16];                                        // the 32 order keys, two per register
  uint32_t kmax = 0, nan = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = tid + P3V_SAMPLE_THREADS * j;
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
        else k = bf16_order_key(b);
      }
      if (e & 1) kp[4 * j + e / 2] |= k << 16;
      else kp[4 * j + e / 2] = k;
      kmax = k > kmax ? k : kmax;
    }
  }
  // 1 / 2. NaN flag and the largest value in one reduction (keys and the flag are exact in fp32)
  const float top = block_max((float)kmax + (nan ? 65536.f : 0.f), sm.fred);
  const float T = prm.temperature;
  bool greedy = !(T > 0.f) || top >= 65536.f;
  float m = 0.f;
  if (!greedy) {
    m = __fdiv_rn(order_key_value((uint32_t)top), T);    // the division is monotonic: max z = z of the max logit
    greedy = !(fabsf(m) <= 3.402823466e38f);             // no finite logit, or max z overflowed
  }
  if (greedy) {                                           // 0. / NaN row: p3v_argmax's own reduction (-1 for a NaN row)
    const ValIdx a = block_argmax(row_argmax_partial(row, n), sm.vred);
    return a.i;
  }
  int par = 0;
  // 4. top-k: the k-th largest key = the largest key kk with #{key >= kk} >= k
  uint32_t kcut = 0;
  const int k = prm.top_k;
  if (k >= 1 && k < n) {
    for (int bit = 15; bit >= 0; --bit) {
      const uint32_t cand = kcut | (1u << bit);
      uint32_t cnt = 0;
#pragma unroll
      for (int s = 0; s < 32; ++s) cnt += P3V_KEY(s) >= cand;
      if (block_sum_u64(cnt, sm, par) >= (uint64_t)k) kcut = cand;
    }
  }
  // 3. integer weights of the kept tokens (fp64 exponential; below 2^-32 of the top token's: 0)
  const double md = (double)m;
  uint32_t wlo[32], whi = 0;                              // w = wlo + 2^32 * bit s of whi (w <= 2^32)
  uint64_t part = 0;
#pragma unroll
  for (int s = 0; s < 32; ++s) {
    uint64_t w = 0;
    if (P3V_KEY(s) != 0 && P3V_KEY(s) >= kcut) {
      const double d = (double)__fdiv_rn(order_key_value(P3V_KEY(s)), T) - md;
      if (d >= -22.25) w = (uint64_t)floor(exp(d) * 4294967296.0);    // exp(-22.25) * 2^32 < 1
    }
    wlo[s] = (uint32_t)w;
    whi |= (uint32_t)(w >> 32) << s;
    part += w;
  }
#define P3V_W(s) ((uint64_t)wlo[s] + ((uint64_t)((whi >> (s)) & 1u) << 32))
  uint64_t mass = block_sum_u64(part, sm, par);
  // 5. top-p over the kept tokens: the largest key pc with sum_{key >= pc} w >= ceil(p * Q)
  const float p = prm.top_p;
  if (p > 0.f && p < 1.f) {
    const uint64_t P = (uint64_t)ceil((double)p * (double)mass);
    uint32_t pcut = 0;
    for (int bit = 15; bit >= 0; --bit) {
      const uint32_t cand = pcut | (1u << bit);
      uint64_t sum = 0;
      uint32_t sel = 0;
#pragma unroll
      for (int s = 0; s < 32; ++s) {
        const bool in = P3V_KEY(s) >= cand;
        sum += in ? wlo[s] : 0u;
        sel |= (uint32_t)in << s;
      }
      sum += (uint64_t)__popc(sel & whi) << 32;    // (the 64-bit weights are never materialised: they would stay live in 64 VGPRs)
      const uint64_t tot = block_sum_u64(sum, sm, par);
      if (tot >= P) { pcut = cand; mass = tot; }
    }
#pragma unroll
    for (int s = 0; s < 32; ++s)
      if (P3V_KEY(s) < pcut) { wlo[s] = 0; whi &= ~(1u << s); }
  }
  // 6. t = floor(Q' * r / 2^32); the token is the smallest index whose inclusive kept prefix exceeds t
  const uint32_t r = philox4x32_10_w0((uint32_t)prm.counter, 0u, 0u, 0u, prm.seed_lo, prm.seed_hi);
  const uint64_t t = __umul64hi(mass, (uint64_t)r << 32);
  uint64_t cs[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    cs[j] = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) cs[j] += P3V_W(8 * j + e);
  }
  // the largest chunk C with (mass of the chunks before C) <= t: it holds the token
  int C = 0;
  uint64_t before = 0;
  for (int bit = 11; bit >= 0; --bit) {
    const int cand = C | (1 << bit);
    uint64_t sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) sum += tid + P3V_SAMPLE_THREADS * j < cand ? cs[j] : 0;
    const uint64_t tot = block_sum_u64(sum, sm, par);
    if (tot <= t) { C = cand; before = tot; }
  }
  if (tid == (C & (P3V_SAMPLE_THREADS - 1))) {
    const int jc = C / P3V_SAMPLE_THREADS;
    int tok = -1;                            // (unreachable: chunk C holds mass > t - before)
    uint64_t acc = before;
    bool found = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j != jc) continue;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        acc += P3V_W(8 * j + e);
        if (!found && acc > t) { tok = 8 * C + e; found = true; }
      }
    }
    sm.tok = tok;
  }
#undef P3V_W
  __syncthreads();
  return sm.tok;
}

__global__ void __launch_bounds__(P3V_SAMPLE_THREADS) k_sample(const bf16_t* __restrict__ logits, int64_t stride,
                                                              p3v_sample_row_t* __restrict__ prm, int32_t* __restrict__ out, int n) {
  __shared__ SampleSmem sm;
  const int b = blockIdx.x;
  const p3v_sample_row_t rp = prm[b];
  const int tok = sample_row(logits + (size_t)b * stride, n, rp, sm);
  if (threadIdx.x == 0) {
    out[b] = tok;
    prm[b].counter = rp.counter + 1;       // 7. (every thread has read the record: sample_row ends on a barrier)
  }
}

// p3v_step_end (p3v_elementwise.hip) with the sampled token: the same bookkeeping, the same relaxed ticket
__global__ void __launch_bounds__(P3V_SAMPLE_THREADS) k_sample_step_end(const bf16_t* __restrict__ logits,
                                                                       p3v_sample_row_t* __restrict__ prm, int32_t* __restrict__ next_tok,
                                                                       int32_t* __restrict__ tok, int32_t* __restrict__ hist,
                                                                       int32_t* d_step, int32_t* d_past, int32_t* ticket, int n,
                                                                       int max_steps) {
  __shared__ SampleSmem sm;
  const int b = blockIdx.x;
  const int s = *d_step;                     // read before this workgroup takes its ticket (the last one bumps it)
  const int past_now = *d_past;
  const p3v_sample_row_t rp = prm[b];
  const int t = sample_row(logits + (size_t)b * n, n, rp, sm);
  if (threadIdx.x == 0) {
    prm[b].counter = rp.counter + 1;
    next_tok[b] = t;
    tok[b] = t;
    if (s < max_steps) hist[(size_t)b * max_steps + s] = t;
    bool last = gridDim.x == 1;
    if (!last) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      last = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
    }
    if (last) {
      *d_step = s + 1;
      *d_past = past_now + 1;
      if (gridDim.x > 1) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

extern "C" int p3v_sample(const uint16_t* logits, int64_t row_stride, p3v_sample_row_t* rows_params, int32_t* out, int rows, int n,
                          void* stream) {
  if (!logits || !rows_params || !out || rows < 0 || n <= 0 || row_stride < n) return P3V_ERR_ARG;
  if (n > P3V_SAMPLE_MAX_N || rows > P3V_SAMPLE_MAX_ROWS) return P3V_ERR_UNSUPPORTED;
  if (rows == 0) return P3V_OK;
  hipLaunchKernelGGL(k_sample, dim3(rows), dim3(P3V_SAMPLE_THREADS), 0, (hipStream_t)stream, logits, row_stride, rows_params, out, n);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}

extern "C" int p3v_sample_step_end(const uint16_t* logits, p3v_sample_row_t* rows_params, int32_t* next_tok, int32_t* tok,
                                   int32_t* history, int32_t* d_step, int32_t* d_past, int32_t* ticket, int B, int n, int max_steps,
                                   void* stream) {
  if (!logits || !rows_params || !next_tok || !tok || !history || !d_step || !d_past || !ticket || B <= 0 || n <= 0)
    return P3V_ERR_ARG;
  if (n > P3V_SAMPLE_MAX_N || B > P3V_SAMPLE_MAX_ROWS) return P3V_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_sample_step_end, dim3(B), dim3(P3V_SAMPLE_THREADS), 0, (hipStream_t)stream, logits, rows_params, next_tok, tok,
                     history, d_step, d_past, ticket, n, max_steps);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}
