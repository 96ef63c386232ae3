// LoRA adapter inference (reference: LoRALinear.__call__, phi.py:129-133)
//   y = linear(x)                      frozen projection, bf16 (any p3v_gemm / p3v_gemv launch, plain epilogue)
//   z = (x @ lora_a) @ lora_b          fp32 (lora_a [K, r], lora_b [r, N] are fp32 in adapters.safetensors)
//   out = (y + scale * z).astype(bf16)
// as two small launches around the frozen projection: p3v_lora_down (t = x @ lora_a, [M, r] fp32) and
// p3v_lora_up (rank-r update of y, fused with the epilogue the frozen projection would have carried).
// Both are bandwidth-trivial next to the projection they decorate (r <= 64): rows of x stream once, lora_a /
// lora_b stay L2-resident.
#include "p3v_common.h"

__global__ void __launch_bounds__(256) k_lora_down(const bf16_t* __restrict__ x, const float* __restrict__ a,
                                                   float* __restrict__ t, int K, int r) {
  __shared__ float red[4][8];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bf16_t* xr = x + (size_t)m * K;
  for (int rc = 0; rc < r; rc += 8) {
    const int nr = min(8, r - rc);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = tid; k < K; k += 256) {
      const float xv = bf16_to_f32(xr[k]);
      const float* ar = a + (size_t)k * r + rc;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < nr) acc[j] += xv * ar[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = wave_sum(acc[j]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) red[wave][j] = acc[j];
    }
    __syncthreads();
    if (tid < nr) t[(size_t)m * r + rc + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
  }
}

extern "C" int p3v_lora_down(const uint16_t* x, const float* lora_a, float* t, int M, int K, int r, void* stream) {
  if (!x || !lora_a || !t || M < 0 || K <= 0 || r <= 0 || r > 64) return P3V_ERR_ARG;
  if (M == 0) return P3V_OK;
  hipLaunchKernelGGL(k_lora_down, dim3(M), dim3(256), 0, (hipStream_t)stream, x, lora_a, t, K, r);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}

// MODE 0: out = v;  1: out = bf16(resid + v);  2: out[n] = silu(v[n]) * v[n + N/2] with the per-op bf16 rounding of
// the fused SiLU epilogue (phi.py:469-471).  v = bf16(y + scale * (t @ lora_b)).
template <int MODE>
__global__ void __launch_bounds__(256) k_lora_up(const bf16_t* __restrict__ y, const float* __restrict__ t,
                                                 const float* __restrict__ b, float scale, const bf16_t* __restrict__ resid,
                                                 bf16_t* __restrict__ out, int N, int r) {
  __shared__ float ts[64];
  const int m = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x < r) ts[threadIdx.x] = t[(size_t)m * r + threadIdx.x];
  __syncthreads();
  const int n_out = MODE == 2 ? N / 2 : N;
  if (n >= n_out) return;
  auto upd = [&](int col) {
    float z = 0.f;
    for (int j = 0; j < r; ++j) z += ts[j] * b[(size_t)j * N + col];
    return bf16_round(bf16_to_f32(y[(size_t)m * N + col]) + scale * z);
  };
  if (MODE == 2) {
    const float g = upd(n), u = upd(n + n_out);
    out[(size_t)m * n_out + n] = f32_to_bf16(bf16_round(g * bf16_round(1.f / (1.f + __expf(-g)))) * u);
  } else {
    const float v = upd(n);
    out[(size_t)m * N + n] = f32_to_bf16(MODE == 1 ? bf16_to_f32(resid[(size_t)m * N + n]) + v : v);
  }
}

extern "C" int p3v_lora_up(const uint16_t* y, const float* t, const float* lora_b, float scale, int epilogue,
                           const uint16_t* resid, uint16_t* out, int M, int N, int r, void* stream) {
  if (!y || !t || !lora_b || !out || M < 0 || N <= 0 || r <= 0 || r > 64) return P3V_ERR_ARG;
  if (epilogue == P3V_EPI_RESID_BF16 && !resid) return P3V_ERR_ARG;
  if (epilogue == P3V_EPI_SILU_MUL && (N & 1)) return P3V_ERR_ARG;
  if (M == 0) return P3V_OK;
  hipStream_t s = (hipStream_t)stream;
  const int n_out = epilogue == P3V_EPI_SILU_MUL ? N / 2 : N;
  const dim3 grid(p3v_cdiv(n_out, 256), M);
  switch (epilogue) {
    case P3V_EPI_NONE: hipLaunchKernelGGL(k_lora_up<0>, grid, dim3(256), 0, s, y, t, lora_b, scale, resid, out, N, r); break;
    case P3V_EPI_RESID_BF16: hipLaunchKernelGGL(k_lora_up<1>, grid, dim3(256), 0, s, y, t, lora_b, scale, resid, out, N, r); break;
    case P3V_EPI_SILU_MUL: hipLaunchKernelGGL(k_lora_up<2>, grid, dim3(256), 0, s, y, t, lora_b, scale, resid, out, N, r); break;
    default: return P3V_ERR_UNSUPPORTED;
  }
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}

// ---------------------------------------------------------------- adapter bank: per-row ("gathered") forms (include/p3v.h)
// One bank table per adapted projection and one row table per state, both in device memory and read here -- never launch
// arguments -- so a captured decode step serves whatever adapters its rows name at replay time.
// K is cut into fixed slices of P3V_LORA_SLICE_K elements, one workgroup per (row, slice): a decode-sized call is
// M * K/256 workgroups instead of M.  Slice s of row m writes its partial to t[m, s, :rank]; k_lora_up_rows adds a row's slices in
// slice order before it uses them.  The slice boundaries and both summation orders depend on K and the rank alone, so a row's
// bits do not depend on M, on its position, or on its neighbours.
struct lora_entry_t { const float* a; const float* b; int32_t rank; float scale; };   // == p3v_lora_entry_t
static_assert(sizeof(lora_entry_t) == 24, "p3v_lora_entry_t layout");

// e keeps the entry's own rank -- the row stride of lora_a [K, rank] --, r is the number of columns in use, min(rank, r_max)
__device__ __forceinline__ bool lora_row_entry(const lora_entry_t* __restrict__ table, const int32_t* __restrict__ row_adapter,
                                               int m, int n_slots, int r_max, lora_entry_t& e, int& r) {
  const int slot = row_adapter[m];
  if (slot < 0 || slot >= n_slots) return false;
  e = table[slot];
  r = min(e.rank, r_max);
  return r > 0 && e.a && e.b;
}

template <bool NORM>
__global__ void __launch_bounds__(256) k_lora_down_rows(const bf16_t* __restrict__ x, const bf16_t* __restrict__ norm_w, float eps,
                                                        const lora_entry_t* __restrict__ table,
                                                        const int32_t* __restrict__ row_adapter, float* __restrict__ t, int K,
                                                        int r_max, int n_slots, int slices) {
  __shared__ float red[4][8];
  __shared__ float rs;
  const int m = blockIdx.x / slices, s = blockIdx.x - m * slices;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  lora_entry_t e;
  int r;
  if (!lora_row_entry(table, row_adapter, m, n_slots, r_max, e, r)) return;  // (uniform over the workgroup)
  const bf16_t* xr = x + (size_t)m * K;
  const int k = s * P3V_LORA_SLICE_K + tid;
  float xv = k < K ? bf16_to_f32(xr[k]) : 0.f;
  if (NORM) {
    // the row's 1/rms exactly as k_rmsnorm computes it: one wave, lane l sums 16-byte chunks l, l + 64, .. in that order
    if (wave == 0) {
      const u32x4_t* xc = (const u32x4_t*)xr;
      const int chunks = K / 8;
      float ss = 0.f;
      for (int c = lane; c < chunks; c += 64) {
        u32x4_t v = xc[c];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float a = bf16lo(v[j]), b = bf16hi(v[j]);
          ss += a * a + b * b;
        }
      }
      ss = wave_sum(ss);
      if (lane == 0) rs = rsqrtf(ss * (1.0f / K) + eps);
    }
    __syncthreads();
    if (k < K) xv = bf16_round(bf16_round(xv * rs) * bf16_to_f32(norm_w[k]));   // rms_pair's two roundings
  }
  const float* ar = e.a + (size_t)(k < K ? k : 0) * e.rank;
  float* tr = t + ((size_t)m * slices + s) * r_max;
  for (int rc = 0; rc < r; rc += 8) {
    const int nr = min(8, r - rc);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = j < nr ? xv * ar[rc + j] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = wave_sum(acc[j]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) red[wave][j] = acc[j];
    }
    __syncthreads();
    if (tid < nr) tr[rc + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
  }
}

extern "C" int p3v_lora_rows_slices(int K) { return K > 0 ? p3v_cdiv(K, P3V_LORA_SLICE_K) : 0; }

extern "C" int p3v_lora_down_rows(const uint16_t* x, const uint16_t* norm_w, float eps, const p3v_lora_entry_t* table,
                                  const int32_t* row_adapter, float* t, int M, int K, int r_max, int n_slots, void* stream) {
  if (!x || !table || !row_adapter || !t || M < 0 || K <= 0 || r_max <= 0 || r_max > 64 || n_slots <= 0) return P3V_ERR_ARG;
  if (norm_w && K % 8) return P3V_ERR_ARG;
  if (M == 0) return P3V_OK;
  const int slices = p3v_lora_rows_slices(K);
  if ((long)M * slices > 0x7fffffffL) return P3V_ERR_UNSUPPORTED;
  const lora_entry_t* tb = (const lora_entry_t*)table;
  if (norm_w)
    hipLaunchKernelGGL(k_lora_down_rows<true>, dim3(M * slices), dim3(256), 0, (hipStream_t)stream, x, norm_w, eps, tb, row_adapter, t,
                       K, r_max, n_slots, slices);
  else
    hipLaunchKernelGGL(k_lora_down_rows<false>, dim3(M * slices), dim3(256), 0, (hipStream_t)stream, x, norm_w, eps, tb, row_adapter, t,
                       K, r_max, n_slots, slices);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}

// MODE as k_lora_up.  A row without an adapter (slot -1, rank 0) passes y through the epilogue untouched.
template <int MODE>
__global__ void __launch_bounds__(256) k_lora_up_rows(const bf16_t* __restrict__ y, const float* __restrict__ t,
                                                      const lora_entry_t* __restrict__ table,
                                                      const int32_t* __restrict__ row_adapter, const bf16_t* __restrict__ resid,
                                                      bf16_t* __restrict__ out, int N, int r_max, int n_slots, int slices, int nblk) {
  __shared__ float ts[64];
  const int m = blockIdx.x / nblk, n = (blockIdx.x - m * nblk) * 256 + threadIdx.x;
  lora_entry_t e;
  int rr = 0;
  const bool on = lora_row_entry(table, row_adapter, m, n_slots, r_max, e, rr);
  const int r = on ? rr : 0;
  if ((int)threadIdx.x < r) {                                   // the row's K slices, added in slice order
    const float* tr = t + (size_t)m * slices * r_max + threadIdx.x;
    float v = 0.f;
    for (int s = 0; s < slices; ++s) v += tr[(size_t)s * r_max];
    ts[threadIdx.x] = v;
  }
  __syncthreads();
  const int n_out = MODE == 2 ? N / 2 : N;
  if (n >= n_out) return;
  auto upd = [&](int col) {
    const float yv = bf16_to_f32(y[(size_t)m * N + col]);
    if (r == 0) return yv;
    float z = 0.f;
    for (int j = 0; j < r; ++j) z += ts[j] * e.b[(size_t)j * N + col];
    return bf16_round(yv + e.scale * z);
  };
  if (MODE == 2) {
    const float g = upd(n), u = upd(n + n_out);
    out[(size_t)m * n_out + n] = f32_to_bf16(bf16_round(g * bf16_round(1.f / (1.f + __expf(-g)))) * u);
  } else {
    const float v = upd(n);
    out[(size_t)m * N + n] = f32_to_bf16(MODE == 1 ? bf16_to_f32(resid[(size_t)m * N + n]) + v : v);
  }
}

extern "C" int p3v_lora_up_rows(const uint16_t* y, const float* t, const p3v_lora_entry_t* table, const int32_t* row_adapter,
                                int epilogue, const uint16_t* resid, uint16_t* out, int M, int N, int K, int r_max, int n_slots,
                                void* stream) {
  if (!y || !t || !table || !row_adapter || !out || M < 0 || N <= 0 || K <= 0 || r_max <= 0 || r_max > 64 || n_slots <= 0)
    return P3V_ERR_ARG;
  if (epilogue == P3V_EPI_RESID_BF16 && !resid) return P3V_ERR_ARG;
  if (epilogue == P3V_EPI_SILU_MUL && (N & 1)) return P3V_ERR_ARG;
  if (M == 0) return P3V_OK;
  hipStream_t s = (hipStream_t)stream;
  const int n_out = epilogue == P3V_EPI_SILU_MUL ? N / 2 : N;
  const int nblk = p3v_cdiv(n_out, 256), slices = p3v_lora_rows_slices(K);
  if ((long)M * nblk > 0x7fffffffL) return P3V_ERR_UNSUPPORTED;
  const lora_entry_t* tb = (const lora_entry_t*)table;
  const dim3 grid(M * nblk);
#define P3V_UP_ROWS(MODE) hipLaunchKernelGGL(k_lora_up_rows<MODE>, grid, dim3(256), 0, s, y, t, tb, row_adapter, resid, out, N, r_max, \
                                             n_slots, slices, nblk)
  switch (epilogue) {
    case P3V_EPI_NONE: P3V_UP_ROWS(0); break;
    case P3V_EPI_RESID_BF16: P3V_UP_ROWS(1); break;
    case P3V_EPI_SILU_MUL: P3V_UP_ROWS(2); break;
    default: return P3V_ERR_UNSUPPORTED;
  }
#undef P3V_UP_ROWS
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}
