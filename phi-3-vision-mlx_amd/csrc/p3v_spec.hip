// Speculative greedy decoding (B = 1): the head and the tail of a verify step and the prompt-lookup drafter.  The rule is
// written out in include/p3v.h ("speculative greedy decoding") and once more in plain Python (speculate.py).
//   k_spec_begin     L workgroups: embedding row of tok[j] + rotation row of position *d_past + j (one launch for what
//                    p3v_embed_gather + p3v_stage_rope do in two)
//   k_spec_end       L workgroups of 1024 threads: workgroup j takes the arg-max of logits row j (p3v_argmax's reduction) and
//                    publishes it with a write-through store; the LAST one to arrive (one relaxed ticket: at most 16 arrivals)
//                    does acceptance, the pinned-host stores, the counters, the append to ctx and the next proposal
//   k_ngram_propose  the proposal alone (one workgroup), for tests of the rule without a model
// The n-gram search runs on all 1024 lanes: lane t compares candidate positions t, t + 1024, ... and keeps its largest match;
// the largest over the workgroup is one LDS max.  No cache write-back fences, no allocation, plain vector stores.
#include "p3v_common.h"
#include "p3v_argmax.h"

#define P3V_SPEC_THREADS 1024

struct SpecSmem {
  ValIdx red[16];
  int amax[P3V_DECODE_MAX_L];
  int emit[P3V_DECODE_MAX_L];       // the tokens this step appends to ctx (read back by the proposal: ctx_at)
  int draft[P3V_DECODE_MAX_L];
  int best, last, n_emit, n_draft;
};

// ctx as the proposal sees it: ids [0, n_old) from memory, [n_old, n) from the run this workgroup has just emitted (LDS)
__device__ __forceinline__ int ctx_at(const int32_t* __restrict__ ctx, int n_old, const int* extra, int i) {
  return i < n_old ? ctx[i] : extra[i - n_old];
}

// The draft for ctx[0..n): every thread returns its length; draft[0..k) is in LDS behind a barrier.
__device__ __forceinline__ int propose_block(const int32_t* __restrict__ ctx, int n_old, const int* extra, int n, int K, int n_max,
                                             int n_min, int vocab, int* draft, int* best) {
  const int tid = threadIdx.x;
  for (int m = n_max; m >= n_min; --m) {
    if (m >= n || m < 1) continue;                     // (uniform over the workgroup)
    __syncthreads();
    if (tid == 0) *best = -1;
    __syncthreads();
    int s[P3V_SPEC_NGRAM_CAP];
#pragma unroll
    for (int e = 0; e < P3V_SPEC_NGRAM_CAP; ++e) s[e] = e < m ? ctx_at(ctx, n_old, extra, n - m + e) : 0;
    int mine = -1;
    for (int p = tid; p < n - m; p += P3V_SPEC_THREADS) {
      bool eq = true;
#pragma unroll
      for (int e = 0; e < P3V_SPEC_NGRAM_CAP; ++e)
        if (e < m) eq = eq && ctx_at(ctx, n_old, extra, p + e) == s[e];
      if (eq) mine = p;                                // p grows: the last match of a thread is its largest
    }
    if (mine >= 0) atomicMax(best, mine);              // LDS
    __syncthreads();
    const int p = *best;
    __syncthreads();                                   // (everyone has read the position before `best` carries the length)
    if (p < 0) continue;
    if (tid == 0) {
      int k = 0;
      const int end = min(p + m + K, n);
      for (int i = p + m; i < end; ++i) {
        const int t = ctx_at(ctx, n_old, extra, i);
        if (t < 0 || t >= vocab) break;
        draft[k++] = t;
      }
      *best = k;
    }
    __syncthreads();
    return *best;
  }
  return 0;
}

__global__ void __launch_bounds__(P3V_SPEC_THREADS) k_ngram_propose(const int32_t* __restrict__ ctx, int n, int K, int n_max, int n_min,
                                                                   int vocab, int32_t* __restrict__ draft_out,
                                                                   int32_t* __restrict__ n_draft_out) {
  __shared__ int draft[P3V_DECODE_MAX_L];
  __shared__ int best;
  const int k = propose_block(ctx, n, draft, n, K, n_max, n_min, vocab, draft, &best);
  if ((int)threadIdx.x < k) draft_out[threadIdx.x] = draft[threadIdx.x];
  if (threadIdx.x == 0) *n_draft_out = k;
}

__global__ void __launch_bounds__(128) k_spec_begin(const int32_t* __restrict__ tok, const u32x4_t* __restrict__ table,
                                                    u32x4_t* __restrict__ x_out, int chunks, int vocab,
                                                    const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                    const int32_t* __restrict__ d_past, float* __restrict__ cos_o,
                                                    float* __restrict__ sin_o, int tab_t, int half) {
  const int j = blockIdx.x;
  int pos = *d_past + j;
  pos = pos < 0 ? 0 : (pos >= tab_t ? tab_t - 1 : pos);   // (rows behind the table's end are dead rows of a step at the budget)
  int id = tok[j];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const u32x4_t* src = table + (size_t)id * chunks;
  u32x4_t* dst = x_out + (size_t)j * chunks;
  for (int c = threadIdx.x; c < chunks; c += blockDim.x) dst[c] = src[c];
  for (int i = threadIdx.x; i < half; i += blockDim.x) {
    cos_o[(size_t)j * half + i] = cos_t[(size_t)pos * half + i];
    sin_o[(size_t)j * half + i] = sin_t[(size_t)pos * half + i];
  }
}

__global__ void __launch_bounds__(P3V_SPEC_THREADS) k_spec_end(const bf16_t* __restrict__ logits, p3v_spec_state_t sp, int L, int V) {
  __shared__ SpecSmem sm;
  const int j = blockIdx.x, tid = threadIdx.x;
  const ValIdx a = block_argmax(row_argmax_partial(logits + (size_t)j * V, V), sm.red);
  if (tid == 0) {
    // write-through store of this row's arg-max, out before the workgroup counts itself in (gemv_step_end_tail's pattern)
    __hip_atomic_store(sp.amax + j, a.i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool last = L == 1;
    if (!last) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      last = __hip_atomic_fetch_add(sp.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == L - 1;
    }
    sm.last = last;
  }
  __syncthreads();
  if (!sm.last) return;
  // ---- the last workgroup to arrive: every row's arg-max is visible
  if (tid < L) sm.amax[tid] = __hip_atomic_load(sp.amax + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int* ctl = sp.ctl;
  const int n = ctl[P3V_SPEC_CTL_N], k = min(max(ctl[P3V_SPEC_CTL_NDRAFT], 0), L - 1), forced = ctl[P3V_SPEC_CTL_FORCED];
  const int replay = ctl[P3V_SPEC_CTL_REPLAY], n_limit = ctl[P3V_SPEC_CTL_NLIMIT];
  const int step = *sp.d_step, past = *sp.d_past;
  if (tid >= 1 && tid <= k) sm.draft[tid - 1] = sp.tok[tid];
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    while (acc < k && sm.draft[acc] == sm.amax[acc]) ++acc;
    int c = acc + 1;
    const bool failed = sm.amax[acc] < 0;                // a NaN row ends the run: reported, nothing advanced past it
    if (!failed) c = max(0, min(c, min(n_limit, sp.ctx_cap) - n));
    for (int i = 0; i < c; ++i) sm.emit[i] = sm.amax[i];
    sm.n_emit = c;
    sm.best = failed;
  }
  __syncthreads();
  const int c = sm.n_emit;
  const bool failed = sm.best != 0;
  // pinned host memory: 4-byte stores, the step's record first ([emitted, drafts in, draft ids]), then its tokens
  if (replay < sp.rec_cap) {
    int32_t* rec = sp.rec + (size_t)replay * P3V_SPEC_REC_INTS;
    if (tid >= 2 && tid < 2 + k) rec[tid] = sm.draft[tid - 2];
    if (tid == 1) rec[1] = k;
    if (tid == 0) rec[0] = c;
  }
  if (tid < c && step + tid < sp.hist_cap) sp.history[step + tid] = sm.emit[tid];
  if (tid == 0) {
    *sp.d_step = step + c;
    ctl[P3V_SPEC_CTL_REPLAY] = replay + 1;
    ctl[P3V_SPEC_CTL_ACC] = c;
    if (L > 1) __hip_atomic_store(sp.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-armed for the next replay
  }
  if (failed) {                                          // the host raises on the negative token; the next row 0 is it (as k_step_end)
    if (tid == 0) { sp.tok[0] = -1; ctl[P3V_SPEC_CTL_NDRAFT] = 0; }
    return;
  }
  const int n_new = n + c;
  if (tid < c) sp.ctx[n + tid] = sm.emit[tid];
  if (tid == 0) {
    ctl[P3V_SPEC_CTL_N] = n_new;
    *sp.d_past = past + c;
  }
  int kd = 0;
  if (!forced && c > 0) kd = propose_block(sp.ctx, n, sm.emit, n_new, L - 1, sp.n_max, sp.n_min, V, sm.draft, &sm.best);
  else if (!forced) kd = -1;                             // a step at the budget: drafts and row 0 stay as they are
  if (kd >= 0) {
    const int t0 = c > 0 ? sm.emit[c - 1] : sp.tok[0];
    if (tid < L) sp.tok[tid] = tid == 0 ? t0 : (tid <= kd ? sm.draft[tid - 1] : t0);   // padding rows: any valid id
    if (tid == 0) ctl[P3V_SPEC_CTL_NDRAFT] = kd;
  }
}

static int spec_args_ok(const p3v_spec_state_t* s, int L) {
  return s && s->tok && s->ctx && s->ctl && s->amax && s->ticket && s->history && s->rec && s->d_step && s->d_past && L >= 1 &&
         L <= P3V_DECODE_MAX_L && s->n_min >= 1 && s->n_max >= s->n_min && s->n_max <= P3V_SPEC_NGRAM_CAP && s->ctx_cap > 0 &&
         s->hist_cap >= 0 && s->rec_cap >= 0;
}

extern "C" int p3v_spec_begin(const int32_t* tok, const uint16_t* table, uint16_t* x_out, const float* cos_t, const float* sin_t,
                              const int32_t* d_past, float* cos_out, float* sin_out, int L, int hidden, int vocab, int tab_t,
                              int half_dim, void* stream) {
  if (!tok || !table || !x_out || !cos_t || !sin_t || !d_past || !cos_out || !sin_out) return P3V_ERR_ARG;
  if (L < 1 || L > P3V_DECODE_MAX_L || hidden % 8 || vocab <= 0 || tab_t <= 0 || half_dim <= 0) return P3V_ERR_ARG;
  hipLaunchKernelGGL(k_spec_begin, dim3(L), dim3(128), 0, (hipStream_t)stream, tok, (const u32x4_t*)table, (u32x4_t*)x_out, hidden / 8,
                     vocab, cos_t, sin_t, d_past, cos_out, sin_out, tab_t, half_dim);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}

extern "C" int p3v_spec_end(const uint16_t* logits, const p3v_spec_state_t* state, int L, int n, void* stream) {
  if (!logits || n <= 0 || !spec_args_ok(state, L)) return P3V_ERR_ARG;
  hipLaunchKernelGGL(k_spec_end, dim3(L), dim3(P3V_SPEC_THREADS), 0, (hipStream_t)stream, logits, *state, L, n);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}

extern "C" int p3v_ngram_propose(const int32_t* ctx, int n, int K, int n_max, int n_min, int vocab, int32_t* draft,
                                 int32_t* n_draft, void* stream) {
  if (!ctx || !draft || !n_draft || n < 0 || K < 0 || K > P3V_DECODE_MAX_L - 1 || n_min < 1 || n_max < n_min ||
      n_max > P3V_SPEC_NGRAM_CAP || vocab <= 0)
    return P3V_ERR_ARG;
  hipLaunchKernelGGL(k_ngram_propose, dim3(1), dim3(P3V_SPEC_THREADS), 0, (hipStream_t)stream, ctx, n, K, n_max, n_min, vocab, draft,
                     n_draft);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}
