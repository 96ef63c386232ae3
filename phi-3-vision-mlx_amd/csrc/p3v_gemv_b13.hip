// The B = 1 decode projections on bf16 weights stored as exact 13-bit codes (p3v_dot_b13.h): the streaming GEMV
// that every weight format shares (gemv_stream_body, p3v_gemv3_body.h) with the GemvB13 policy below -- 13/16 of the bf16 stream's
// bytes, the same eight weights per lane and lane load, so the same v_dot2c sequence and the same bits out -- plus the load-time
// pack kernels and the unpack kernel the tests use.
#include <type_traits>

#include "p3v_common.h"
#include "p3v_dot_b13.h"
#include "p3v_dot_bf16.h"
#include "p3v_gemv3_body.h"

struct GemvB13P {
  const bf16_t* x; const uint32_t* W; void* out; const bf16_t* resid; const bf16_t* norm_w;
  float eps;
  int M, N, K, epi, units;
  uint32_t cc;                       // ((base - 1) << 7) in both 16-bit halves
};

// ---------------------------------------------------------------- M = 1 streaming: what gemv_stream_body needs to know about the packing
// a stage is one container: 1 sign load + CH / 2 nibble loads + CH low-byte loads per lane (10 against 12 at CH = 6, 7 against 8 at CH = 4)
#ifdef P3V_GEMV_TIMING                                         // tools/gemv_timeline.py: 100 MHz stamps per wave (entry, exit, first dot)
__device__ long long p3v_gemv_b13_tbuf[4096 * 3];
extern "C" int p3v_gemv_b13_timing_read(long long* out, int n) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(p3v_gemv_b13_tbuf), sizeof(long long) * n) == hipSuccess ? 0 : -1;
}
#define B13MARK(k) do { if ((threadIdx.x & 63) == 0 && blockIdx.x < 1024) p3v_gemv_b13_tbuf[(blockIdx.x * 4 + (threadIdx.x >> 6)) * 3 + (k)] = wall_clock64(); } while (0)
#else
#define B13MARK(k)
#endif
// SCALED: the activations staged in LDS carry the matrix's 2^(base - 1) (stage_x below), so the codes go to v_dot2c as b13_pre8 leaves
// them -- every product w' * x' is the real number w * x, both factors normal bf16 values, and the sums come out bit for bit.  An x
// row with an element that does not take the factor (it would overflow, is Inf or NaN, or a bf16 denormal) makes the workgroup restage
// the row as it was and run the exact decode for that launch (dot_exact: the body's second, plain loop).
template <int CH, bool WITH_CC> struct B13Stage { uint32_t sg[B13<CH>::NS]; u32x4_t nib[CH / 2]; u32x4_t lo[CH]; uint32_t cc; };   // (cc: uniform, rides along for dot)
template <int CH> struct B13Stage<CH, false> { uint32_t sg[B13<CH>::NS]; u32x4_t nib[CH / 2]; u32x4_t lo[CH]; };
template <bool SCALED> struct GemvB13 {
  typedef GemvB13P P;
  static constexpr int WPL = 8, MAX_MT = 1, MIN_WG = 4;
  static constexpr bool XSUM = false, XSCALE = SCALED;
  // 4 workgroups a CU (at most 128 VGPRs): the decode's VALU operations want the fourth wave of a SIMD (gemv_route puts it there)
  template <int CH> using Stage = B13Stage<CH, !SCALED>;   // (the scaled form needs no base in the pipeline)
  static __device__ __forceinline__ void mark(int k) { B13MARK(k); }
  template <int K, int CH>
  static __device__ __forceinline__ void load(const P& p, int r0, int, int c0, Stage<CH>& st) {
    typedef B13<CH> L;
    constexpr int NST = K / (CH * 512);
    const int u = p.epi == P3V_EPI_SILU_MUL ? r0 : r0 >> 1, lane = c0 & 63, s = (c0 >> 6) / CH;
    const uint32_t* cp = p.W + (size_t)(u * NST + s) * L::DWORDS;
    if constexpr (L::NS == 3) {
      const uint32_t* sp = cp + lane * 3;
      st.sg[0] = __builtin_nontemporal_load(sp);
      st.sg[1] = __builtin_nontemporal_load(sp + 1);
      st.sg[2] = __builtin_nontemporal_load(sp + 2);
    } else {
      const u32x2_t v = __builtin_nontemporal_load((const u32x2_t*)cp + lane);
      st.sg[0] = v[0];
      st.sg[1] = v[1];
    }
    const u32x4_t* np = (const u32x4_t*)(cp + L::NIB_OFF) + lane;
    const u32x4_t* lp = (const u32x4_t*)(cp + L::LO_OFF) + lane;
#pragma unroll
    for (int i = 0; i < CH / 2; ++i) st.nib[i] = __builtin_nontemporal_load(np + i * 64);
#pragma unroll
    for (int j = 0; j < CH; ++j) st.lo[j] = __builtin_nontemporal_load(lp + j * 64);
    if constexpr (!SCALED) st.cc = p.cc;
  }
  // the weights of lane load j of one row: as bf16 (EXACT: + the base, cc) or times 2^-(base - 1)
  template <bool EXACT, int CH>
  static __device__ __forceinline__ u32x4_t weights_as(const Stage<CH>& st, uint32_t cc, int j, int row) {
    typedef B13<CH> L;
    const uint32_t lo0 = st.lo[j][2 * row], lo1 = st.lo[j][2 * row + 1], nib = st.nib[j >> 1][(j & 1) * 2 + row];
    const uint32_t sg0 = st.sg[L::sign_word(row, j, 0)] << L::sign_shift(row, j, 0), sg1 = st.sg[L::sign_word(row, j, 1)] << L::sign_shift(row, j, 1);
    if constexpr (EXACT) return b13_decode8(lo0, lo1, nib, sg0, sg1, cc);
    else {
      uint32_t pre[4];
      b13_pre8(lo0, lo1, nib, sg0, sg1, pre);
      return (u32x4_t){pre[0], pre[1], pre[2], pre[3]};
    }
  }
  template <int CH>
  static __device__ __forceinline__ u32x4_t weights(const Stage<CH>& st, int j, int row) {
    static_assert(!SCALED, "the bf16 weights: the exact form only");
    return weights_as<true>(st, st.cc, j, row);
  }
  template <int CH>
  static __device__ __forceinline__ void dot(const Stage<CH>& st, int j, const u32x4_t* x, const float*, int c, float& a0, float& a1) {
    const u32x4_t xa = x[c];
    if constexpr (SCALED) {
      a0 = dot8(weights_as<false>(st, 0u, j, 0), xa, a0);
      a1 = dot8(weights_as<false>(st, 0u, j, 1), xa, a1);
    } else {
      a0 = dot8(weights(st, j, 0), xa, a0);
      a1 = dot8(weights(st, j, 1), xa, a1);
    }
  }
  // (XSCALE) the exact decode on the scaled form's stages, for a launch whose x row does not take the factor
  template <int CH>
  static __device__ __forceinline__ void dot_exact(const P& p, const Stage<CH>& st, int j, const u32x4_t* x, const float*, int c, float& a0, float& a1) {
    const u32x4_t xa = x[c];
    a0 = dot8(weights_as<true>(st, p.cc, j, 0), xa, a0);
    a1 = dot8(weights_as<true>(st, p.cc, j, 1), xa, a1);
  }
  // XSCALE: one staged activation pair (already rounded to bf16) times 2^(base - 1), in integers: cc = (base - 1) << 7 added to the
  // exponent field of every non-zero element (min(magnitude, 1) * cc, as b13_decode8 adds it to the codes) -- exact for a normal number
  // that stays finite.  acc[0] / acc[1] collect the largest magnitude and the smallest magnitude - 1 (a zero wraps to 0xffff) of the
  // row, per 16-bit half; x_unfit then says whether the row must keep the exact decode: an element at or above 2^(128 - (base - 1))
  // (Inf and NaN with them: they are not worth a form of their own) or a bf16 denormal.  Six VALU operations a pair.
  static __device__ __forceinline__ uint32_t stage_x(const P& p, uint32_t x2, uint32_t (&acc)[2]) {
    const b13_u16x2_t one = {1, 1};
    const uint32_t mag = x2 & 0x7fff7fffu;
    uint32_t nz, y2, m1;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(nz) : "v"(mag), "v"(one));
    asm("v_pk_mad_u16 %0, %1, %2, %3" : "=v"(y2) : "v"(nz), "v"(p.cc), "v"(x2));
    asm("v_pk_max_u16 %0, %1, %2" : "=v"(acc[0]) : "v"(acc[0]), "v"(mag));
    asm("v_pk_sub_u16 %0, %1, %2" : "=v"(m1) : "v"(mag), "v"(one));
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(acc[1]) : "v"(acc[1]), "v"(m1));
    return y2;
  }
  static __device__ __forceinline__ bool x_unfit(const P& p, const uint32_t (&acc)[2]) {
    const uint32_t top = 0x7f80u - (p.cc & 0xffffu);                      // (255 - (base - 1)) << 7: the first exponent that overflows
    const uint32_t mx = max(acc[0] & 0xffffu, acc[0] >> 16), mn = min(acc[1] & 0xffffu, acc[1] >> 16);
    return mx >= top || mn < 0x7fu;
  }
  template <int CH> static __device__ __forceinline__ float finish(float v, const Stage<CH>&, int) { return v; }
};

// ---------------------------------------------------------------- pack (load time) / unpack (tests)
// info[4]: [0] status (0 = packed, non-zero = the matrix does not fit and `out` holds nothing), [1] base, [2] / [3] smallest / largest
// biased exponent of the non-zero weights.  Pass 1 finds the range and flags denormals, Inf and NaN; pass 2 packs one container per lane.
#define B13_BAD_VALUE 1
#define B13_BAD_RANGE 2

__global__ void k_b13_init(int32_t* info) { info[0] = 0; info[1] = 1; info[2] = 255; info[3] = 0; }

__global__ void __launch_bounds__(256) k_b13_range(const u32x4_t* __restrict__ W, long chunks, int32_t* info) {
  int emin = 255, emax = 0, bad = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (long)gridDim.x * 256) {
    const u32x4_t w = W[i];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t h = (w[k >> 1] >> (16 * (k & 1))) & 0xffffu, e = (h >> 7) & 0xffu, m = h & 0x7fu;
      if (e == 255u || (e == 0u && m != 0u)) bad = 1;               // Inf / NaN, denormal
      if (e != 0u) { emin = min(emin, (int)e); emax = max(emax, (int)e); }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    emin = min(emin, __shfl_xor(emin, off, 64));
    emax = max(emax, __shfl_xor(emax, off, 64));
    bad |= __shfl_xor(bad, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(info + 2, emin);
    atomicMax(info + 3, emax);
    if (bad) atomicOr(info, B13_BAD_VALUE);
  }
}

template <int CH>
__global__ void __launch_bounds__(256) k_b13_pack(const u32x4_t* __restrict__ W, uint32_t* __restrict__ out, int32_t* info, int rows, int nst,
                                                  int silu_pairs, long n_lanes) {
  typedef B13<CH> L;
  const int emin = info[2], emax = info[3];
  const int base = max(1, emax - 30);                     // the window's 31 binades end at the largest exponent
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t == 0) {
    info[1] = base;
    if (emin < base) atomicOr(info, B13_BAD_RANGE);
  }
  if (t >= n_lanes || emin < base) return;
  const long ci = t >> 6;
  const int lane = (int)(t & 63), u = (int)(ci / nst), s = (int)(ci % nst), xch = nst * CH * 64;
  const int r[2] = {silu_pairs ? u : 2 * u, silu_pairs ? u + rows / 2 : 2 * u + 1};
  uint32_t sg[L::NS] = {};
  u32x4_t nib[CH / 2], lo[CH];
#pragma unroll
  for (int i = 0; i < CH / 2; ++i) nib[i] = (u32x4_t){0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < CH; ++j) lo[j] = (u32x4_t){0, 0, 0, 0};
#pragma unroll
  for (int row = 0; row < 2; ++row)
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const u32x4_t w = W[(size_t)r[row] * xch + (s * CH + j) * 64 + lane];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint32_t h = (w[k >> 1] >> (16 * (k & 1))) & 0xffffu, e = (h >> 7) & 0xffu, m = h & 0x7fu, sign = h >> 15;
        const uint32_t q = e == 0u ? 0u : (e - (uint32_t)base + 1u) & 31u;
        const int half = k >> 2, b = k & 3;
        lo[j][2 * row + half] |= (((q & 1u) << 7) | m) << (8 * b);
        nib[j >> 1][(j & 1) * 2 + row] |= (q >> 1) << (4 * (2 * b + half));
        sg[L::sign_word(row, j, half)] |= sign << (8 * b + 7 - L::sign_shift(row, j, half));
      }
    }
  uint32_t* cp = out + (size_t)ci * L::DWORDS;
#pragma unroll
  for (int i = 0; i < L::NS; ++i) cp[lane * L::NS + i] = sg[i];
#pragma unroll
  for (int i = 0; i < CH / 2; ++i) ((u32x4_t*)(cp + L::NIB_OFF))[i * 64 + lane] = nib[i];
#pragma unroll
  for (int j = 0; j < CH; ++j) ((u32x4_t*)(cp + L::LO_OFF))[j * 64 + lane] = lo[j];
}

// the GEMV's own loads and decode (GemvB13::load / weights), written back as bf16 rows
template <int K, int CH>
__global__ void __launch_bounds__(256) k_b13_unpack(GemvB13P p, u32x4_t* __restrict__ out, int rows, long n_lanes) {
  constexpr int NST = K / (CH * 512);
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_lanes) return;
  const long ci = t >> 6;
  const int lane = (int)(t & 63), u = (int)(ci / NST), s = (int)(ci % NST);
  const bool silu = p.epi == P3V_EPI_SILU_MUL;
  const int r[2] = {silu ? u : 2 * u, silu ? u + rows / 2 : 2 * u + 1};
  GemvB13<false>::Stage<CH> st;
  GemvB13<false>::load<K, CH>(p, r[0], r[1], s * CH * 64 + lane, st);
#pragma unroll
  for (int row = 0; row < 2; ++row)
#pragma unroll
    for (int j = 0; j < CH; ++j) out[(size_t)r[row] * (K / 8) + (s * CH + j) * 64 + lane] = GemvB13<false>::weights(st, j, row);
}

static bool b13_shape_ok(int rows, int K) { return rows > 0 && rows % 2 == 0 && (K == 3072 || K == 8192); }
static uint32_t b13_cc(int base) { const uint32_t c = (uint32_t)(base - 1) << 7; return c | (c << 16); }

extern "C" int p3v_pack_b13(const uint16_t* W, int rows, int K, int silu_pairs, void* out, int32_t* info, void* stream) {
  if (!W || !out || !info) return P3V_ERR_ARG;
  if (!b13_shape_ok(rows, K)) return P3V_ERR_UNSUPPORTED;
  if (((uintptr_t)W | (uintptr_t)out) & 15) return P3V_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const long chunks = (long)rows * (K / 8), n_lanes = chunks / (K == 3072 ? 12 : 8);   // a lane packs 2 rows x CH chunks
  hipLaunchKernelGGL(k_b13_init, dim3(1), dim3(1), 0, s, info);
  hipLaunchKernelGGL(k_b13_range, dim3(min(4096, p3v_cdiv(chunks, 256))), dim3(256), 0, s, (const u32x4_t*)W, chunks, info);
  if (K == 3072) hipLaunchKernelGGL(k_b13_pack<6>, dim3(p3v_cdiv(n_lanes, 256)), dim3(256), 0, s, (const u32x4_t*)W, (uint32_t*)out, info, rows, 1, silu_pairs, n_lanes);
  else hipLaunchKernelGGL(k_b13_pack<4>, dim3(p3v_cdiv(n_lanes, 256)), dim3(256), 0, s, (const u32x4_t*)W, (uint32_t*)out, info, rows, 4, silu_pairs, n_lanes);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}

extern "C" int p3v_unpack_b13(const void* packed, int rows, int K, int silu_pairs, int exp_base, uint16_t* out, void* stream) {
  if (!packed || !out || exp_base < 1 || exp_base > 224) return P3V_ERR_ARG;
  if (!b13_shape_ok(rows, K)) return P3V_ERR_UNSUPPORTED;
  if (((uintptr_t)packed | (uintptr_t)out) & 15) return P3V_ERR_ARG;
  GemvB13P p = {nullptr, (const uint32_t*)packed, nullptr, nullptr, nullptr, 0.f, 1, rows, K, silu_pairs ? P3V_EPI_SILU_MUL : P3V_EPI_NONE, rows / 2, b13_cc(exp_base)};
  const long n_lanes = (long)rows * (K / 8) / (K == 3072 ? 12 : 8);
  hipStream_t s = (hipStream_t)stream;
  if (K == 3072) hipLaunchKernelGGL((k_b13_unpack<3072, 6>), dim3(p3v_cdiv(n_lanes, 256)), dim3(256), 0, s, p, (u32x4_t*)out, rows, n_lanes);
  else hipLaunchKernelGGL((k_b13_unpack<8192, 4>), dim3(p3v_cdiv(n_lanes, 256)), dim3(256), 0, s, p, (u32x4_t*)out, rows, n_lanes);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}

// ---------------------------------------------------------------- entry points: the twins of p3v_gemv_fp8 / p3v_gemv_fp8_step, one row only
// every instantiation they can launch, found by what gemv_route chose (the scaled form at K = 8192 is not built: see the route)
static GemvStreamKernel b13_stream[] = {GEMV_STREAM_STEPS(GemvB13<true>, 1, 1, 6), GEMV_STREAM_STEPS(GemvB13<false>, 0, 1, 6), GEMV_STREAM_STEPS(GemvB13<false>, 0, 4, 4)};

// what the entries ask of their own pointers beyond null checks: the container's alignment, and the row pairing, which is part of the packing
static bool b13_own_ok(const p3v_gemv_b13_args_t* a) { return !((uintptr_t)a->W & 15) && (a->silu_pairs != 0) == (a->epilogue == P3V_EPI_SILU_MUL); }
static GemvB13P b13_params(const p3v_gemv_b13_args_t* a) {
  return {a->x, (const uint32_t*)a->W, a->out, a->resid, a->norm_w, a->norm_eps, a->M, a->N, a->K, a->epilogue,
          a->epilogue == P3V_EPI_SILU_MUL ? a->N : a->N / 2, b13_cc(a->exp_base)};
}

extern "C" int p3v_gemv_b13_plan(int N, int K, int epilogue, int n_cu, int* out) {
  if (!out || N <= 0 || n_cu <= 0) return P3V_ERR_ARG;
  p3v_gemv_route_t r;
  gemv_route({P3V_GEMV_FMT_B13, P3V_GEMV_STEP_NONE, 1, N, K, epilogue == P3V_EPI_SILU_MUL ? P3V_EPI_SILU_MUL : P3V_EPI_NONE, 0, 0, 1, n_cu}, &r);
  if (r.status) return r.status;
  out[0] = r.upw; out[1] = r.waves; out[2] = r.wpw; out[3] = r.grid;
  return P3V_OK;
}

extern "C" int p3v_gemv_b13_step(const p3v_gemv_b13_args_t* a, const p3v_gemv_step_t* st, void* stream) {
  if (!a || !st || !a->W || !a->out) return P3V_ERR_ARG;
  p3v_gemv_route_t r; GemvStepP sp;
  if (const int rc = gemv_step_route(P3V_GEMV_FMT_B13, a, a->exp_base, st, r, sp, b13_own_ok(a))) return rc;
  GemvB13P p = b13_params(a);
  return launch_gemv_stream(b13_stream, r, p, &sp, (hipStream_t)stream);
}

extern "C" int p3v_gemv_b13(const p3v_gemv_b13_args_t* a, void* stream) {
  if (!a || !a->x || !a->W || !a->out) return P3V_ERR_ARG;
  p3v_gemv_route_t r;
  gemv_route({P3V_GEMV_FMT_B13, P3V_GEMV_STEP_NONE, a->M, a->N, a->K, a->epilogue, a->norm_w != nullptr, a->resid != nullptr, a->exp_base, 0}, &r);
  if (r.status) return r.status;
  if (!b13_own_ok(a)) return P3V_ERR_ARG;
  GemvB13P p = b13_params(a);
  return launch_gemv_stream(b13_stream, r, p, nullptr, (hipStream_t)stream);
}
