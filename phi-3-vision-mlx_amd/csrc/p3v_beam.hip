// Beam search: the tail of a beam step and the K/V reorder behind it.  The rule is written out in include/p3v.h ("beam search")
// and once more in plain Python (beam.py); both kernels are held to it bit for bit.
//   k_beam_end     R workgroups of 1024 threads.  Workgroup r reads logits row r once with 16-byte loads and keeps it in registers
//                  as 16-bit order keys (p3v_logprobs.hip's packing: the helpers below restate that file's, which stays as it
//                  is), sums the row's integer weights (so the normaliser does not depend on the reduction order), takes its 2W
//                  best by 2W rounds of a block-wide maximum below the previous pick, and publishes (id, score) with write-through
//                  stores before it takes one relaxed ticket.  The LAST workgroup to arrive (k_spec_end's pattern; the ticket is
//                  left at zero) ranks the at most 128 candidates, walks the best 2W, and writes the next beams, the pinned-host
//                  record and the counters.
//   k_kv_permute   beam k continues row parent[k]: the window of suffix columns of every moved row goes through a staging
//                  buffer in two launches (gather, scatter), 16 bytes per lane.  The grid is fixed for the capacity; what
//                  lies beyond the live window exits.
// No floating-point atomics, plain vector stores, no allocation, nothing synchronised.
#include "p3v_common.h"

#define P3V_BEAM_THREADS 1024
#define P3V_BEAM_MAX_N 65536
#define P3V_BEAM_CAND (2 * P3V_BEAM_MAX)             // candidates per row
#define P3V_BEAM_KEY_NINF 0x007fu                   // order key of -inf
#define P3V_BEAM_KEY_PINF 0xff80u                   // order key of +inf

// the 16-bit order key of p3v_logprobs.hip: orders the non-NaN bf16 values as floats do (-0 == +0); key 0 = a padding slot
__device__ __forceinline__ uint32_t bm_order_key(uint32_t b) {
  b = b == 0x8000u ? 0u : b;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}
__device__ __forceinline__ float bm_key_value(uint32_t k) {
  return bf16_to_f32((bf16_t)((k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu)));
}
__device__ __forceinline__ uint32_t bm_wave_max_u32(uint32_t v) {
#define P3V_BM_DPP(ctrl) v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, 0xf, 0xf, true));
  P3V_BM_DPP(0xB1) P3V_BM_DPP(0x4E) P3V_BM_DPP(0x124) P3V_BM_DPP(0x128)
#undef P3V_BM_DPP
  float a, b;
  rows_swap32(__uint_as_float(v), a, b);
  v = max(__float_as_uint(a), __float_as_uint(b));
  rows_swap16(__uint_as_float(v), a, b);
  return max(__float_as_uint(a), __float_as_uint(b));
}
__device__ __forceinline__ uint64_t bm_u64_of(float lo, float hi) {
  return ((uint64_t)__float_as_uint(hi) << 32) | __float_as_uint(lo);
}
__device__ __forceinline__ uint64_t bm_wave_sum_u64(uint64_t v) {
#define P3V_BM_DPP(ctrl)                                                                                    \
  {                                                                                                         \
    const uint32_t lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, ctrl, 0xf, 0xf, true);             \
    const uint32_t hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), ctrl, 0xf, 0xf, true);     \
    v += ((uint64_t)hi << 32) | lo;                                                                         \
  }
  P3V_BM_DPP(0xB1) P3V_BM_DPP(0x4E) P3V_BM_DPP(0x124) P3V_BM_DPP(0x128)
#undef P3V_BM_DPP
  float a0, b0, a1, b1;
  rows_swap32(__uint_as_float((uint32_t)v), a0, b0);
  rows_swap32(__uint_as_float((uint32_t)(v >> 32)), a1, b1);
  v = bm_u64_of(a0, a1) + bm_u64_of(b0, b1);
  rows_swap16(__uint_as_float((uint32_t)v), a0, b0);
  rows_swap16(__uint_as_float((uint32_t)(v >> 32)), a1, b1);
  return bm_u64_of(a0, a1) + bm_u64_of(b0, b1);
}

struct BeamSmem {
  uint64_t red[16];
  uint32_t ured[2][16];       // double-buffered, one barrier per round: a buffer is rewritten two rounds later
  float fred[16];
  int cand_id[P3V_BEAM_CAND];
  float cand_score[P3V_BEAM_CAND];
  int all_id[P3V_BEAM_MAX * P3V_BEAM_CAND];        // the merge: slot r * 16 + place
  float all_score[P3V_BEAM_MAX * P3V_BEAM_CAND];
  int order[P3V_BEAM_CAND];                        // slot of the j-th best candidate
  int32_t rec[P3V_BEAM_REC_INTS];
  int last, failed;
};

// J = 16-byte chunks per thread (n <= 8192 * J); slot s of a thread holds index 8 * (tid + 1024 * (s >> 3)) + (s & 7)
template <int J>
__global__ void __launch_bounds__(P3V_BEAM_THREADS) k_beam_end(const bf16_t* __restrict__ logits, p3v_beam_state_t st, int R, int W,
                                                              int n, int eos) {
  __shared__ BeamSmem sm;
  const int r = blockIdx.x, tid = threadIdx.x, C = 2 * W;
  const bf16_t* __restrict__ row = logits + (size_t)r * n;
  const bool vec = (((size_t)row) & 15) == 0;
  uint32_t kp[4 * J];                                     // the order keys, two per register
  uint32_t kmax = 0, nan = 0;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int c = tid + P3V_BEAM_THREADS * j;
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
        else k = bm_order_key(b);
      }
      if (e & 1) kp[4 * j + e / 2] |= k << 16;
      else kp[4 * j + e / 2] = k;
      kmax = k > kmax ? k : kmax;
    }
  }
#define P3V_BM_KEY(s) (((s) & 1) ? kp[(s) >> 1] >> 16 : kp[(s) >> 1] & 0xffffu)
#define P3V_BM_IDX(s) (8 * (tid + P3V_BEAM_THREADS * ((s) >> 3)) + ((s) & 7))
  // point 1: the NaN flag and the largest value in one reduction (keys and the flag are exact in fp32)
  const float top = block_max((float)kmax + (nan ? 65536.f : 0.f), sm.fred);
  const uint32_t ktop = (uint32_t)top;
  const bool defined = top < 65536.f && ktop < P3V_BEAM_KEY_PINF && ktop > P3V_BEAM_KEY_NINF;
  if (tid < P3V_BEAM_CAND) { sm.cand_id[tid] = -1; sm.cand_score[tid] = 0.f; }
  if (defined) {
    // steps 3 - 5 of the logprobs rule: W = the sum of the integer weights, lse in fp64
    const double md = (double)bm_key_value(ktop);
    uint64_t part = 0;
#pragma unroll
    for (int s = 0; s < 8 * J; ++s) {
      const uint32_t k = P3V_BM_KEY(s);
      if (k > P3V_BEAM_KEY_NINF) {
        const double d = (double)bm_key_value(k) - md;
        if (d >= -22.25) part += (uint64_t)floor(exp(d) * 4294967296.0);    // exp(-22.25) * 2^32 < 1
      }
    }
    part = bm_wave_sum_u64(part);
    if ((tid & 63) == 0) sm.red[tid >> 6] = part;
    __syncthreads();
    uint64_t Wsum = 0;
#pragma unroll
    for (int w = 0; w < P3V_BEAM_THREADS / 64; ++w) Wsum += sm.red[w];
    const double lse = md + log((double)Wsum) - 32.0 * 0.6931471805599453094;
    const float cum = st.cum[r];
    // point 2: the 2W best, each round the largest (value, index) word below the previous pick
    uint32_t last = 0xffffffffu;
    for (int p = 0; p < C; ++p) {
      uint32_t best = 0;
#pragma unroll
      for (int s = 0; s < 8 * J; ++s) {
        const uint32_t k = P3V_BM_KEY(s);
        const uint32_t c = k << 16 | (uint32_t)(65535 - P3V_BM_IDX(s));
        best = (k != 0 && c < last && c > best) ? c : best;
      }
      best = bm_wave_max_u32(best);
      if ((tid & 63) == 0) sm.ured[p & 1][tid >> 6] = best;
      __syncthreads();
      last = 0;
#pragma unroll
      for (int w = 0; w < P3V_BEAM_THREADS / 64; ++w) last = max(last, sm.ured[p & 1][w]);
      if (tid == 0) {
        sm.cand_id[p] = 65535 - (int)(last & 0xffffu);
        sm.cand_score[p] = cum + (float)((double)bm_key_value(last >> 16) - lse);     // ONE fp32 addition
      }
    }
  }
#undef P3V_BM_KEY
#undef P3V_BM_IDX
  __syncthreads();
  // write-through stores of this row's candidates (an undefined row: id -1), out before the workgroup counts itself in
  if (tid < C) {
    __hip_atomic_store(st.cand_id + r * P3V_BEAM_CAND + tid, sm.cand_id[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(st.cand_score + r * P3V_BEAM_CAND + tid, sm.cand_score[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  }
  __syncthreads();
  if (tid == 0) {
    bool last = R == 1;
    if (!last) last = __hip_atomic_fetch_add(st.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == R - 1;
    sm.last = last;
  }
  __syncthreads();
  if (!sm.last) return;

  // ---- the last workgroup to arrive: every row's candidates are visible
  if (tid == 0) sm.failed = 0;
  __syncthreads();
  const int n_all = R * P3V_BEAM_CAND;                     // slots r * 16 + place; place >= 2W is unused
  const bool live = tid < n_all && (tid & (P3V_BEAM_CAND - 1)) < C;
  int my_id = -1;
  float my_score = 0.f;
  if (live) {
    my_id = __hip_atomic_load(st.cand_id + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    my_score = __hip_atomic_load(st.cand_score + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (my_id < 0) sm.failed = 1;                          // (every writer stores the same value)
  }
  if (tid < n_all) { sm.all_id[tid] = my_id; sm.all_score[tid] = my_score; }
  if (tid < P3V_BEAM_REC_INTS) sm.rec[tid] = -1;
  if (tid < P3V_BEAM_CAND) sm.order[tid] = 0;              // (a NaN in `cum` breaks the order: the walk still reads valid slots)
  __syncthreads();
  const bool failed = sm.failed != 0;
  const int step = *st.d_step, past = *st.d_past;
  if (!failed) {
    // point 3: the place of a candidate in the total order = how many come before it (score descending, then the slot)
    if (live) {
      int before = 0;
      for (int o = 0; o < n_all; ++o) {
        if ((o & (P3V_BEAM_CAND - 1)) >= C) continue;
        const float so = sm.all_score[o];
        before += so > my_score || (so == my_score && o < tid);
      }
      if (before < C) sm.order[before] = tid;
    }
    __syncthreads();
    // point 4
    if (tid == 0) {
      int k = 0, nf = 0;
      for (int j = 0; j < C && k < W; ++j) {
        const int o = sm.order[j], id = sm.all_id[o];
        const float s = sm.all_score[o];
        if (id == eos) {
          if (j < W) {
            sm.rec[2 + 3 * P3V_BEAM_MAX + nf] = o / P3V_BEAM_CAND;
            sm.rec[2 + 4 * P3V_BEAM_MAX + nf] = __float_as_int(s);
            ++nf;
          }
          continue;
        }
        sm.rec[2 + k] = id;
        sm.rec[2 + P3V_BEAM_MAX + k] = o / P3V_BEAM_CAND;
        sm.rec[2 + 2 * P3V_BEAM_MAX + k] = __float_as_int(s);
        ++k;
      }
      sm.rec[0] = 0;
      sm.rec[1] = nf;
    }
  } else if (tid == 0) {
    sm.rec[0] = 1;
    sm.rec[1] = 0;
  }
  __syncthreads();
  // the next step's rows (a failed step: tok = -1, the rows and their sums stay where they are)
  if (tid < W) {
    st.tok[tid] = sm.rec[2 + tid];
    st.parent[tid] = failed ? tid : sm.rec[2 + P3V_BEAM_MAX + tid];
    if (!failed) st.cum[tid] = __int_as_float(sm.rec[2 + 2 * P3V_BEAM_MAX + tid]);
  }
  // point 6: pinned host memory, plain 4-byte stores
  if (step >= 0 && step < st.rec_cap && tid < P3V_BEAM_REC_INTS) st.rec[(size_t)step * P3V_BEAM_REC_INTS + tid] = sm.rec[tid];
  if (tid == 0) {
    *st.d_step = step + 1;                                 // point 5
    *st.d_past = past + 1;
    if (R > 1) __hip_atomic_store(st.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-armed for the next replay
  }
}

extern "C" int p3v_beam_end(const uint16_t* logits, const p3v_beam_state_t* s, int R, int W, int n, int eos, void* stream) {
  if (!logits || !s || !s->tok || !s->parent || !s->cum || !s->cand_id || !s->cand_score || !s->ticket || !s->rec || !s->d_step ||
      !s->d_past || s->rec_cap < 0)
    return P3V_ERR_ARG;
  if (W < 2 || W > P3V_BEAM_MAX || (R != 1 && R != W) || n < 2 * W) return P3V_ERR_ARG;
  if (n > P3V_BEAM_MAX_N) return P3V_ERR_UNSUPPORTED;
  if (n <= 32768)
    hipLaunchKernelGGL(k_beam_end<4>, dim3(R), dim3(P3V_BEAM_THREADS), 0, (hipStream_t)stream, logits, *s, R, W, n, eos);
  else
    hipLaunchKernelGGL(k_beam_end<8>, dim3(R), dim3(P3V_BEAM_THREADS), 0, (hipStream_t)stream, logits, *s, R, W, n, eos);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}

// ---- the reorder.  One workgroup per (layer, beam row k, kv head) and part; piece i of a unit is 16 bytes of K (the window of
// one (row, head) is one contiguous run of ncols * hd elements) and 16 bytes of V^T (run i / (ncols / 8), piece i % (ncols / 8)).
struct kvp_args_t {
  char* k; char* v; char* stage_k; char* stage_v;
  const int32_t* parent; const int32_t* d_past;
  int B, T, W, c0a, stage_cols, phase, nkv, hd, parts;
};

__global__ void __launch_bounds__(256) k_kv_permute(const kvp_args_t a) {
  const int unit = blockIdx.x, part = blockIdx.y, tid = threadIdx.x;
  const int h = unit % a.nkv, k = (unit / a.nkv) % a.W, l = unit / (a.nkv * a.W);
  const int p = a.parent[k];
  if (p == k || p < 0 || p >= a.W) return;                 // a row that stays, or a word that names no row
  int past = *a.d_past;
  past = past < 0 ? 0 : (past > a.T ? a.T : past);         // (T is a multiple of 8: the rounding below stays inside)
  int end = (past + 7) & ~7;
  end = min(end, min(a.T, a.c0a + a.stage_cols));
  const int ncols = end - a.c0a;
  if (ncols <= 0) return;
  const int hd = a.hd, vp = ncols >> 3, np = vp * hd;      // 16-byte pieces of the K window = of the V^T window
  const int row = a.phase == 0 ? p : k;                    // gather reads row parent[k], scatter writes row k
  const size_t cu = ((size_t)l * a.B + row) * a.nkv + h, su = ((size_t)l * a.W + k) * a.nkv + h;
  u32x4_t* ck = (u32x4_t*)(a.k + ((cu * a.T + a.c0a) * hd) * 2);
  u32x4_t* sk = (u32x4_t*)(a.stage_k + su * a.stage_cols * hd * 2);
  char* cv = a.v + (cu * hd * a.T + a.c0a) * 2;
  char* sv = a.stage_v + su * hd * a.stage_cols * 2;
  for (int i = part * 256 + tid; i < np; i += a.parts * 256) {
    const int d = i / vp, j = i - d * vp;
    u32x4_t* cvp = (u32x4_t*)(cv + (size_t)d * a.T * 2) + j;
    u32x4_t* svp = (u32x4_t*)(sv + (size_t)d * a.stage_cols * 2) + j;
    if (a.phase == 0) { sk[i] = ck[i]; *svp = *cvp; }
    else { ck[i] = sk[i]; *cvp = *svp; }
  }
}

extern "C" int p3v_kv_permute(void* k, void* v, int B, int T, const int32_t* parent, int W, int c0a, const int32_t* d_past,
                              void* stage_k, void* stage_v, int stage_cols, int phase, int nl, int nkv, int hd, int elem_size,
                              void* stream) {
  if (!k || !v || !parent || !d_past || !stage_k || !stage_v) return P3V_ERR_ARG;
  if (nl <= 0 || nkv <= 0 || hd <= 0 || T <= 0 || W < 2 || W > P3V_BEAM_MAX || B < W || (phase != 0 && phase != 1)) return P3V_ERR_ARG;
  if (elem_size != 2 || (hd * 2) % 16 || T % 8) return P3V_ERR_UNSUPPORTED;
  if (c0a < 0 || c0a > T || c0a % 8 || stage_cols < 8 || stage_cols % 8) return P3V_ERR_ARG;
  if (((uintptr_t)k | (uintptr_t)v | (uintptr_t)stage_k | (uintptr_t)stage_v) & 15) return P3V_ERR_ARG;
  if ((long)nl * nkv * W > 0x7fffffffL) return P3V_ERR_ARG;
  kvp_args_t a;
  a.k = (char*)k, a.v = (char*)v, a.stage_k = (char*)stage_k, a.stage_v = (char*)stage_v;
  a.parent = parent, a.d_past = d_past;
  a.B = B, a.T = T, a.W = W, a.c0a = c0a, a.stage_cols = stage_cols, a.phase = phase, a.nkv = nkv, a.hd = hd;
  // fixed for the capacity: four pieces of each tensor per lane when the window is full, at most 8 parts per unit
  const int cap = min(stage_cols, T - c0a);
  const int parts = p3v_cdiv((long)(cap >> 3) * hd, 1024);
  a.parts = parts < 1 ? 1 : (parts > 8 ? 8 : parts);
  hipLaunchKernelGGL(k_kv_permute, dim3(nl * nkv * W, a.parts), dim3(256), 0, (hipStream_t)stream, a);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}
