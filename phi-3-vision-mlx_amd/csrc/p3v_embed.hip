// Embeddings and retrieval: p3v_embed_pool (final RMSNorm + last / mean pooling + L2 normalisation, fp32 out) and
// p3v_sim_topk (fp32 scores of <= 16 bf16 queries against N bf16 rows and the k best per query, the score matrix never
// written).  include/p3v.h holds the rules; this file holds to them with FIXED summation orders: no floating-point atomics,
// every output a function of its own row alone.
#include "p3v_common.h"

typedef unsigned long long u64_t;

// ---------------------------------------------------------------- pooling
// One 8-wide chunk of a bf16 row.  hidden % 8 == 0: one 16-byte load, as p3v_rmsnorm reads it.  hidden % 8 == 4 (rows are
// then 8-byte aligned only): two 8-byte loads, the row's last chunk zero-filled in its upper half.
__device__ __forceinline__ u32x4_t pool_chunk(const bf16_t* row, int c, int hidden, bool a16) {
  if (a16) return ((const u32x4_t*)row)[c];
  const u32x2_t* p = (const u32x2_t*)(row + 8 * (size_t)c);
  const u32x2_t lo = p[0];
  u32x2_t hi = {0u, 0u};
  if (8 * c + 4 < hidden) hi = p[1];
  return (u32x4_t){lo[0], lo[1], hi[0], hi[1]};
}

__device__ __forceinline__ int pool_first_row(const int32_t* start, int b, int L, int mode) {
  if (mode == P3V_POOL_LAST) return L - 1;
  const int s = start[b];
  return s < 0 ? 0 : (s > L - 1 ? L - 1 : s);     // out-of-contract counts never move a read outside the row block
}

// 1 / rms of every live row, one wave per row: k_rmsnorm's loop, lane by lane (p3v_elementwise.hip), so r has its bits.
__global__ void __launch_bounds__(256) k_pool_rstd(const bf16_t* __restrict__ x, const int32_t* __restrict__ start,
                                                   float* __restrict__ rstd, int L, int hidden, int mode, float inv_h, float eps) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int t0 = pool_first_row(start, b, L, mode);
  const int t = mode == P3V_POOL_LAST ? L - 1 : (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (t >= L || t < t0) return;
  const bool a16 = hidden % 8 == 0;
  const int chunks = (hidden + 7) / 8;
  const bf16_t* xr = x + ((size_t)b * L + t) * hidden;
  float ss = 0.f;
  for (int c = lane; c < chunks; c += 64) {
    const u32x4_t v = pool_chunk(xr, c, hidden, a16);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float a = bf16lo(v[j]), bb = bf16hi(v[j]);
      ss += a * a + bb * bb;
    }
  }
  ss = wave_sum(ss);
  rstd[mode == P3V_POOL_LAST ? b : (size_t)b * L + t] = rsqrtf(ss * inv_h + eps);
}

// p = (sum over live rows of f32(y_t)) / count for 512 columns of one batch row: wave v of 16 sums rows t0 + v, t0 + v + 16, ...
// in that order, wave 0 adds the 16 partial sums in wave order and divides once.  The order depends on (start[b], L) alone.
#define POOL_WAVES 16
__global__ void __launch_bounds__(64 * POOL_WAVES) k_pool_sum(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                              const int32_t* __restrict__ start, const float* __restrict__ rstd,
                                                              float* __restrict__ out, int L, int hidden, int mode) {
  __shared__ float red[POOL_WAVES * 8 * 64];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane, chunks = (hidden + 7) / 8;
  const bool a16 = hidden % 8 == 0, active = c < chunks;
  const int t0 = pool_first_row(start, b, L, mode);
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (active) {
    const u32x4_t g = pool_chunk(w, c, hidden, a16);
#pragma unroll 4
    for (int t = t0 + wv; t < L; t += POOL_WAVES) {
      const u32x4_t v = pool_chunk(x + ((size_t)b * L + t) * hidden, c, hidden, a16);
      const float r = rstd[mode == P3V_POOL_LAST ? b : (size_t)b * L + t];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t o = rms_pair(v[j], r, g[j]);
        acc[2 * j] += bf16lo(o);
        acc[2 * j + 1] += bf16hi(o);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[(wv * 8 + j) * 64 + lane] = acc[j];
  __syncthreads();
  if (wv != 0 || !active) return;
  const float cnt = (float)(L - t0);
  float p[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float s = red[j * 64 + lane];
    for (int v = 1; v < POOL_WAVES; ++v) s += red[(v * 8 + j) * 64 + lane];
    p[j] = s / cnt;
  }
  float* o = out + (size_t)b * hidden + 8 * (size_t)c;
  *(float4*)o = make_float4(p[0], p[1], p[2], p[3]);
  if (8 * c + 4 < hidden) *(float4*)(o + 4) = make_float4(p[4], p[5], p[6], p[7]);
}

// e = p / sqrt(sum p^2) in place, one workgroup per row; a zero row stays zero, a NaN reaches every element.
__global__ void __launch_bounds__(256) k_pool_l2(float* __restrict__ out, int hidden) {
  __shared__ float red[16];
  float* o = out + (size_t)blockIdx.x * hidden;
  float ss = 0.f;
  for (int j = threadIdx.x; j < hidden; j += 256) {
    const float v = o[j];
    ss += v * v;
  }
  const float tot = block_sum(ss, red);
  if (tot == 0.f) return;
  const float d = sqrtf(tot);
  for (int j = threadIdx.x; j < hidden; j += 256) o[j] = o[j] / d;
}

extern "C" int64_t p3v_embed_pool_ws_bytes(int B, int L, int hidden, int mode) {
  if (B < 1 || L < 1 || hidden < 1 || (mode != P3V_POOL_LAST && mode != P3V_POOL_MEAN)) return 0;
  return 4 * (int64_t)B * (mode == P3V_POOL_LAST ? 1 : L);
}

extern "C" int p3v_embed_pool(const uint16_t* x, const uint16_t* w, const int32_t* start, float* out, int B, int L, int hidden,
                              float eps, int mode, int normalize, void* ws, int64_t ws_bytes, void* stream) {
  if (!x || !w || !out || !ws || B < 1 || B > 65535 || L < 1 || hidden < 4 || hidden % 4) return P3V_ERR_ARG;
  if (mode != P3V_POOL_LAST && mode != P3V_POOL_MEAN) return P3V_ERR_ARG;
  if (mode == P3V_POOL_MEAN && !start) return P3V_ERR_ARG;
  if (normalize != 0 && normalize != 1) return P3V_ERR_ARG;
  const uintptr_t in_align = hidden % 8 ? 7 : 15;
  if (((uintptr_t)x & in_align) || ((uintptr_t)w & in_align) || ((uintptr_t)out & 15) || ((uintptr_t)ws & 3)) return P3V_ERR_ARG;
  if (ws_bytes < p3v_embed_pool_ws_bytes(B, L, hidden, mode)) return P3V_ERR_ARG;
  const hipStream_t s = (hipStream_t)stream;
  const int chunks = (hidden + 7) / 8;
  hipLaunchKernelGGL(k_pool_rstd, dim3(mode == P3V_POOL_LAST ? 1 : p3v_cdiv(L, 4), B), dim3(mode == P3V_POOL_LAST ? 64 : 256), 0, s,
                     x, start, (float*)ws, L, hidden, mode, 1.0f / hidden, eps);
  P3V_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_pool_sum, dim3(p3v_cdiv(chunks, 64), B), dim3(64 * POOL_WAVES), 0, s, x, w, start, (const float*)ws, out, L,
                     hidden, mode);
  P3V_CHECK_LAUNCH();
  if (normalize) {
    hipLaunchKernelGGL(k_pool_l2, dim3(B), dim3(256), 0, s, out, hidden);
    P3V_CHECK_LAUNCH();
  }
  return P3V_OK;
}

// ---------------------------------------------------------------- similarity top-k
// A candidate is one 64-bit key, LARGER = BETTER: the score as an order-preserving unsigned (NaN -> 0, -0 -> +0) above the
// complemented row index, so a plain integer compare is the rule's (-s, i) order; 0 is the empty slot (idx -1, score -inf).
#define SIM_WG_ROWS 256      // rows_per_wg is a multiple of it: 4 waves x 2 passes
#define SIM_TT 2             // 16-row MFMA blocks of one wave's pass over D, against the same query fragment
#define SIM_U 8              // 32-wide blocks of D loaded ahead: TT x U = 16 index loads of 16 bytes per lane in flight, 512 bytes of a row
#define SIM_ROW_TILE (16 * SIM_TT)
#define SIM_WG_TARGET 512    // workgroups of a full-size launch (two 4-wave workgroups per CU)
#define SIM_Q_MAX 16

__device__ __forceinline__ uint32_t sim_ord(float s) {
  if (s != s) return 0u;
  const uint32_t u = s == 0.f ? 0u : __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sim_unord(uint32_t o) {
  if (o == 0u) return __uint_as_float(0x7fc00000u);
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
__device__ __forceinline__ u64_t sim_key(float s, uint32_t row) { return ((u64_t)sim_ord(s) << 32) | (uint32_t)~row; }

// One wave inserts one key (wave-uniform) into its own descending list of k: lane l holds entry l, the ballot of the better
// entries is the position, the tail moves down by one.  LDS operations of one wave execute in order.
__device__ __forceinline__ void sim_insert(volatile u64_t* list, int k, u64_t key, int lane) {
  const u64_t e = lane < k ? list[lane] : 0ull;
  const int pos = __popcll(__ballot(lane < k && e > key));
  if (pos < k) {
    if (lane >= pos && lane < k - 1) list[lane + 1] = e;
    if (lane == pos) list[pos] = key;
  }
}

__device__ __forceinline__ u64_t sim_bcast(u64_t v, int src) {
  const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, src), hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
  return ((u64_t)hi << 32) | lo;
}

// The k best of n_lists descending lists of k (LDS, `stride` entries apart) by rank: entry e's place is the number of better
// entries, equal (empty) keys ordered by position.  One wave; calls `put(rank, key)` for ranks 0 .. k-1, each once.
template <typename Put>
__device__ __forceinline__ void sim_rank_merge(const volatile u64_t* lists, int stride, int n_lists, int k, int lane, Put put) {
  for (int e = lane; e < n_lists * k; e += 64) {
    const u64_t key = lists[(e / k) * stride + e % k];
    int rank = 0, o = 0;
    for (int l = 0; l < n_lists; ++l)
      for (int i = 0; i < k; ++i, ++o) {
        const u64_t ko = lists[l * stride + i];
        rank += (ko > key || (ko == key && o < e)) ? 1 : 0;
      }
    if (rank < k) put(rank, key);
  }
}

// Scores: s(i, q) = sum over 32-wide blocks of D, in order, of one v_mfma_f32_16x16x32_bf16 (index rows on M, queries on N):
// the order inside a block is the instruction's, the same for every row and column; the blocks follow each other in one
// fp32 accumulator.  Nothing else enters: not N, not Q, not k, not the split.
// Plain loads: a wave instruction takes 64 bytes of 16 rows, the other half of each 128-byte line goes to the NEXT instruction --
// with the non-temporal hint that half was fetched again (1564 us against 1205 us for the 6.4 GB of N = 2^20, tools/embed_time.py).
template <int TT, int U>
__global__ void __launch_bounds__(256) k_sim_topk(const bf16_t* __restrict__ index, const bf16_t* __restrict__ queries,
                                                  u64_t* __restrict__ ws, int N, int Q, int k, int D, int rows_per_wg, int n_wg) {
  __shared__ u64_t lists[4 * SIM_Q_MAX * P3V_SIM_TOPK_MAX];      // [wave][query][rank]: 16 KiB
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = lane & 15, g = lane >> 4;
  volatile u64_t* mine = lists + wv * SIM_Q_MAX * P3V_SIM_TOPK_MAX;
  for (int i = lane; i < SIM_Q_MAX * P3V_SIM_TOPK_MAX; i += 64) mine[i] = 0ull;
  const long wg_base = (long)blockIdx.x * rows_per_wg;
  const long wg_end = wg_base + rows_per_wg < N ? wg_base + rows_per_wg : N;
  const bf16_t* qp = queries + (size_t)(q < Q ? q : Q - 1) * D + g * 8;
  const int full = D / 32;
  for (long tile = wg_base + wv * (16 * TT); tile < wg_end; tile += 4 * 16 * TT) {
    const bf16_t* ap[TT];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
      long row = tile + tt * 16 + q;
      row = row < N ? row : N - 1;
      ap[tt] = index + (size_t)row * D + g * 8;
    }
    f32x4_t acc[TT];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) acc[tt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    int kb = 0;
    for (; kb + U <= full; kb += U) {           // TT x U index loads of 16 bytes per lane in flight, then their MFMAs in block order
      u32x4_t a[U][TT];
      bf16x8_t bq[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        bq[u] = __builtin_bit_cast(bf16x8_t, *(const u32x4_t*)(qp + (kb + u) * 32));
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
          a[u][tt] = *(const u32x4_t*)(ap[tt] + (kb + u) * 32);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
          acc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a[u][tt]), bq[u], acc[tt], 0, 0, 0);
    }
    for (; kb < full; ++kb) {
      const bf16x8_t bq = __builtin_bit_cast(bf16x8_t, *(const u32x4_t*)(qp + kb * 32));
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) {
        const u32x4_t a = *(const u32x4_t*)(ap[tt] + kb * 32);
        acc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), bq, acc[tt], 0, 0, 0);
      }
    }
    if (full * 32 < D) {                      // D % 32 in {8, 16, 24}: the lane groups past D multiply zeros
      const bool in = full * 32 + g * 8 < D;
      const u32x4_t z = {0u, 0u, 0u, 0u};
      const bf16x8_t bq = __builtin_bit_cast(bf16x8_t, in ? *(const u32x4_t*)(qp + full * 32) : z);
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) {
        const u32x4_t a = in ? *(const u32x4_t*)(ap[tt] + full * 32) : z;
        acc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), bq, acc[tt], 0, 0, 0);
      }
    }
    // lane (q, g) holds query q's scores of rows tile + 16 tt + 4 g + j
    volatile u64_t* lq = mine + q * P3V_SIM_TOPK_MAX;
    u64_t thr = lq[k - 1];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long row = tile + tt * 16 + 4 * g + j;
        const u64_t key = sim_key(acc[tt][j], (uint32_t)row);
        u64_t m = __ballot(q < Q && row < wg_end && key > thr);
        if (m) {
          while (m) {
            const int src = __builtin_ctzll(m);
            m &= m - 1;
            sim_insert(mine + (src & 15) * P3V_SIM_TOPK_MAX, k, sim_bcast(key, src), lane);
          }
          thr = lq[k - 1];
        }
      }
  }
  __syncthreads();
  for (int qq = wv; qq < Q; qq += 4)
    sim_rank_merge(lists + qq * P3V_SIM_TOPK_MAX, SIM_Q_MAX * P3V_SIM_TOPK_MAX, 4, k, lane, [&](int rank, u64_t key) {
      ws[((size_t)qq * k + rank) * n_wg + blockIdx.x] = key;       // [query][rank][workgroup]: the merge reads the best ranks first
    });
}

// One workgroup per query: each wave filters its share of the n_wg * k candidates into its own list, wave 0 merges the four.
__global__ void __launch_bounds__(256) k_sim_merge(const u64_t* __restrict__ ws, int n_wg, int k, int32_t* __restrict__ idx,
                                                   float* __restrict__ score) {
  __shared__ u64_t lists[4 * P3V_SIM_TOPK_MAX];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), qq = blockIdx.x;
  volatile u64_t* mine = lists + wv * P3V_SIM_TOPK_MAX;
  if (lane < P3V_SIM_TOPK_MAX) mine[lane] = 0ull;
  const u64_t* src_q = ws + (size_t)qq * k * n_wg;
  const long n = (long)k * n_wg;
  for (long base = (long)wv * 512; base < n; base += 4 * 512) {
    u64_t key[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const long e = base + u * 64 + lane;
      key[u] = e < n ? src_q[e] : 0ull;
    }
    u64_t thr = mine[k - 1];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      u64_t m = __ballot(key[u] > thr);
      if (m) {
        while (m) {
          const int src = __builtin_ctzll(m);
          m &= m - 1;
          sim_insert(mine, k, sim_bcast(key[u], src), lane);
        }
        thr = mine[k - 1];
      }
    }
  }
  __syncthreads();
  if (wv != 0) return;
  sim_rank_merge(lists, P3V_SIM_TOPK_MAX, 4, k, lane, [&](int rank, u64_t key) {
    idx[(size_t)qq * k + rank] = key ? (int32_t)~(uint32_t)key : -1;
    score[(size_t)qq * k + rank] = key ? sim_unord((uint32_t)(key >> 32)) : -INFINITY;
  });
}

static bool sim_shape_ok(int N, int Q, int k, int D) {
  return N >= 0 && Q >= 1 && Q <= SIM_Q_MAX && k >= 1 && k <= P3V_SIM_TOPK_MAX && D >= 8 && D <= 8192 && D % 8 == 0;
}

extern "C" int p3v_sim_topk_plan(int N, int Q, int k, int D, int* rows_per_wg, int* n_wg, int* row_tile) {
  if (!sim_shape_ok(N, Q, k, D) || !rows_per_wg || !n_wg || !row_tile) return P3V_ERR_ARG;
  const long per = p3v_cdiv(p3v_cdiv(N, SIM_WG_ROWS), SIM_WG_TARGET);
  *rows_per_wg = (int)(SIM_WG_ROWS * (per > 1 ? per : 1));
  *n_wg = p3v_cdiv(N, *rows_per_wg);
  *row_tile = SIM_ROW_TILE;
  return P3V_OK;
}

extern "C" int64_t p3v_sim_topk_ws_bytes(int N, int Q, int k, int D) {
  int rows_per_wg, n_wg, row_tile;
  if (p3v_sim_topk_plan(N, Q, k, D, &rows_per_wg, &n_wg, &row_tile) != P3V_OK) return 0;
  return 8 * (int64_t)n_wg * Q * k;
}

extern "C" int p3v_sim_topk(const uint16_t* index, const uint16_t* queries, int32_t* idx, float* score, int N, int Q, int k, int D,
                            void* ws, int64_t ws_bytes, void* stream) {
  int rows_per_wg, n_wg, row_tile;
  if (!queries || !idx || !score || p3v_sim_topk_plan(N, Q, k, D, &rows_per_wg, &n_wg, &row_tile) != P3V_OK) return P3V_ERR_ARG;
  if (N > 0 && (!index || !ws || ((uintptr_t)index & 15) || ((uintptr_t)ws & 7))) return P3V_ERR_ARG;
  if (((uintptr_t)queries & 15) || ws_bytes < p3v_sim_topk_ws_bytes(N, Q, k, D)) return P3V_ERR_ARG;
  const hipStream_t s = (hipStream_t)stream;
  if (n_wg > 0) {
    hipLaunchKernelGGL((k_sim_topk<SIM_TT, SIM_U>), dim3(n_wg), dim3(256), 0, s, index, queries, (u64_t*)ws, N, Q, k, D, rows_per_wg, n_wg);
    P3V_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_sim_merge, dim3(Q), dim3(256), 0, s, (const u64_t*)ws, n_wg, k, idx, score);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}
