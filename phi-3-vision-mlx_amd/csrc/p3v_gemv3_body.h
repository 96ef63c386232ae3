// The streaming M = 1 GEMV of the decode step, written ONCE for every weight format: gemv_stream_body, the two kernels around it
// (k_gemv3 / k_gemv3_step), their launch from a table of instantiations and what the p3v_gemv*_step entry points do alike.  A weight format is a policy
// struct F -- GemvBf16 (p3v_gemv.hip), GemvF8 (p3v_gemv_fp8.hip), GemvQ4 (p3v_gemv_q4.hip) -- that supplies only what differs:
//   P           the kernel's parameter struct (x, W, out, resid, norm_w, eps, M, N, K, epi, units + the format's own pointers)
//   WPL         weights per lane load (8 bf16 / 16 e4m3 in 16 bytes, 16 nibbles in 8 bytes);  MAX_MT: x rows it can carry (1 unless bf16)
//   Stage<CH>   one pipeline stage of a row pair in registers: w[2][CH] lane loads + what travels with them (e4m3: the two fp32 row
//               scales; 4-bit: CH scale | bias words per row)
//   load        requests a Stage, in the order that format's stream wants;  dot: folds lane load j of both rows into the two
//               accumulators from the activations in LDS;  finish: applied to a row's sum after wave_sum (the e4m3 row scale)
//   XSUM        the 4-bit form needs the sum of every 16 activations: one more pass over LDS between staging and streaming
//   XSCALE      the scaled 13-bit form (GemvB13<true>, p3v_gemv_b13.hip) wants the staged activations times its matrix's factor: stage_x
//               (a pair on its way to LDS), x_unfit (does this thread's part of the row take the factor?) and dot_exact, the dot of
//               the plain second loop that a workgroup with an unfit row runs on the row as it was
//   mark        timing stamp hook (tools/gemv_timeline.py: bf16 and the 13-bit codes; 0 entry, 1 exit, 2 first dot)
//   MIN_WG      workgroups per CU the kernels are compiled to fit (__launch_bounds__): 1 = whatever the registers allow; the STEP_END
//               launch keeps the default bound (the waves per CU of every launch are gemv_route's, p3v_gemv_route.hip)
// (fo_project, the o_proj stage of the fused attention launches in p3v_attention.hip, repeats this arithmetic from the p3v_dot_*.h
// helpers; it does not share the body.  Two fused launches that did were removed in round 4: DESIGN.md section 3.1.)
#pragma once
#include <type_traits>

#include "p3v_common.h"

typedef std::integral_constant<int, 0> IC0;
typedef std::integral_constant<int, 1> IC1;

// Round 6: the two ends of a replayed greedy decode step ride in the step's first and last projection (p3v_gemv_step):
//  STEP_BEGIN  x row m = embed_table[clamp(tok[m])] (what p3v_step_begin gathered into x_out); workgroup 0 also writes the rows to
//              x_out -- the residual stream the later launches update in place -- and stages the rotation rows of position *d_past.
//  STEP_END    arg-max of the output rows (first maximum of the bf16 values; a NaN row reports -1) + p3v_step_end's bookkeeping:
//              every workgroup publishes its (value, index) candidates write-through and takes a ticket, the LAST one reduces them.
enum { STEP_NONE = 0, STEP_BEGIN = 1, STEP_END = 2 };
struct GemvStepP {
  const int32_t* tok; const bf16_t* table; int vocab; bf16_t* x_out;
  const float* cos_t; const float* sin_t; const int32_t* d_past_in; float* cos_o; float* sin_o; int tab_t, half;
  int32_t* next_tok; int32_t* tok_out; int32_t* hist; int32_t* d_step; int32_t* d_past; int32_t* ticket; float* amax_ws; int max_steps;
};
struct ArgMaxVI { float v; int i; };
__device__ __forceinline__ ArgMaxVI amax_better(ArgMaxVI a, ArgMaxVI b) {   // larger value, then smaller index (k_argmax's order)
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
__device__ __forceinline__ void amax_take(ArgMaxVI& m, float v, int i) {
  if (v != v) { v = INFINITY; i = -1; }                         // a NaN logit: (+inf, -1) beats every real entry (api._rows raises)
  if (v > m.v || (v == m.v && i < m.i) || m.i == 0x7fffffff) { m.v = v; m.i = i; }
}

// ---- the two ends of a replayed greedy step, carried by its first / last projection (p3v_gemv_step, p3v_gemv_fp8_step):
// 5a. (workgroup 0 of the first qkv launch) the gathered embedding rows become the residual stream the later launches update in place
// (re-read from the table: L2-hot, and nothing has to keep them in registers), and the rotation rows of position *d_past are staged for
// the attention launches -- what p3v_step_begin did
template <int MT>
__device__ __forceinline__ void gemv_step_begin_tail(const GemvStepP* sp, const bf16_t* const* xrow, int M, int chunks, int tid) {
#pragma unroll
  for (int m = 0; m < MT; ++m)
    if (m < M)
      for (int c = tid; c < chunks; c += 256) ((u32x4_t*)(sp->x_out + (size_t)m * (chunks * 8)))[c] = ((const u32x4_t*)xrow[m])[c];
  const int past = *sp->d_past_in;
  for (int i = tid; i < M * sp->half; i += 256) {
    const int b = i / sp->half, d = i - b * sp->half;
    sp->cos_o[i] = sp->cos_t[((size_t)b * sp->tab_t + past) * sp->half + d];
    sp->sin_o[i] = sp->sin_t[((size_t)b * sp->tab_t + past) * sp->half + d];
  }
}

// 5b. (every workgroup of the vocabulary head) arg-max + loop bookkeeping without a launch of their own -- what p3v_argmax +
// p3v_step_end did: `best` = each wave's candidates (lane 0's copy counts); the last workgroup to finish reduces all of them
template <int MT>
__device__ __forceinline__ void gemv_step_end_tail(const GemvStepP* sp, const ArgMaxVI (&best)[MT], int M, int bx, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  __shared__ ArgMaxVI wbest[4][MT];
  __shared__ int s_last;
  if (lane == 0) {
#pragma unroll
    for (int m = 0; m < MT; ++m) wbest[wave][m] = best[m];
  }
  __syncthreads();
  const int n_wg = gridDim.x;
  if (tid == 0) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      ArgMaxVI r = wbest[0][m];
#pragma unroll
      for (int w = 1; w < 4; ++w) r = amax_better(r, wbest[w][m]);
      // one 8-byte write-through store per row: a (value, index) pair is never seen half-written by the reducer below
      const unsigned long long rec = (unsigned long long)__builtin_bit_cast(uint32_t, r.v) | ((unsigned long long)(uint32_t)r.i << 32);
      __hip_atomic_store((unsigned long long*)sp->amax_ws + ((size_t)bx * MT + m), rec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // the candidates are out before this workgroup counts itself in
    // Arrival in two levels (MI355X_MICROARCH.md, fanin: ~12 ns per atomic on one word -- the 1002 workgroups of the e4m3 vocabulary head
    // finish together and queued for ~10 us on a single ticket): workgroup b counts on counter b % 8 (b % 8 is also its XCD), the last of
    // each group on the top counter; the last of those has seen everything.  Counters: behind the records, 128 bytes apart, left zero.
    int* ctr = (int*)((unsigned long long*)sp->amax_ws + P3V_GEMV_STEP_MAX_WG * MT);
    const int grp = bx & 7, n_grp = min(8, n_wg), in_grp = (n_wg - grp + 7) >> 3;
    int last = 0;
    if (__hip_atomic_fetch_add(ctr + 32 * grp, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == in_grp - 1)
      last = __hip_atomic_fetch_add(ctr + 32 * 8, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == n_grp - 1;
    s_last = last;
  }
  __syncthreads();
  if (s_last) {                                              // the last workgroup to finish: every other candidate is visible
    __shared__ ArgMaxVI fin[4][MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      ArgMaxVI r = ArgMaxVI{-INFINITY, 0x7fffffff};
      for (int g = tid; g < n_wg; g += 256) {
        const unsigned long long rec = __hip_atomic_load((const unsigned long long*)sp->amax_ws + ((size_t)g * MT + m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        r = amax_better(r, ArgMaxVI{__builtin_bit_cast(float, (uint32_t)rec), (int)(uint32_t)(rec >> 32)});
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        ArgMaxVI o;
        o.v = __shfl_xor(r.v, off, 64);
        o.i = __shfl_xor(r.i, off, 64);
        r = amax_better(r, o);
      }
      if (lane == 0) fin[wave][m] = r;
    }
    __syncthreads();
    if (tid == 0) {
      const int step = *sp->d_step, past_now = *sp->d_past;
#pragma unroll
      for (int m = 0; m < MT; ++m)
        if (m < M) {
          ArgMaxVI r = fin[0][m];
#pragma unroll
          for (int w = 1; w < 4; ++w) r = amax_better(r, fin[w][m]);
          const int idx = r.i == 0x7fffffff ? 0 : r.i;
          sp->next_tok[m] = idx;
          sp->tok_out[m] = idx;
          if (step < sp->max_steps) sp->hist[(size_t)m * sp->max_steps + step] = idx;
        }
      *sp->d_step = step + 1;
      *sp->d_past = past_now + 1;
      int* ctr = (int*)((unsigned long long*)sp->amax_ws + P3V_GEMV_STEP_MAX_WG * MT);
      for (int c = 0; c < 9; ++c) __hip_atomic_store(ctr + 32 * c, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-armed for the next replay
    }
  }
}

// Written so that hipcc can keep COUNTED s_waitcnt vmcnt(N) everywhere -- every load is unconditional and the pipeline body is
// branch-free (a predicated load or a branch between issue and use makes the compiler fall back to vmcnt(0), which drains the prefetch):
//   * x (+ norm weight) chunks are requested first, then the wave's first weight stage, so the RMSNorm prologue waits only for the
//     older x loads while the weights stream in;
//   * (row pair, K stage) software pipeline with two register buffers: stage s+1 is in flight (2*CH lane loads per lane) while stage s
//     is reduced; the residual needed by the epilogue travels with the stage (no dependent load at the end of a row);
//   * grid = the format's waves per CU (gemv_route), each wave owning a contiguous run of row pairs (a pure streaming read on this chip peaks at
//     2 blocks x 256 threads per CU, see tools/stream_floor.hip).
// K = NST stages x CH lane loads x 64 lanes x F::WPL weights, compile-time.
// wpw: waves of the 4-wave workgroup that take rows (4, or 3: wave 3 then only helps with the prologue).  1536 streaming waves
// (qkv, o_proj, down) as 384 four-wave workgroups put two workgroups on half of the CUs and one on the others, and the launch
// lasts as long as the doubly loaded CUs; 512 workgroups x 3 waves load every CU alike (tools/gemv_timeline.py).
template <class F, int MT, int NST, int CH, int STEP>
__device__ __forceinline__ void gemv_stream_body(const typename F::P& p, int units_per_wave, int wpw, const GemvStepP* sp) {
  static_assert(MT <= F::MAX_MT, "this weight format streams one x row only");
  constexpr int K = NST * CH * 64 * F::WPL;
  constexpr int XCH = K / 8;                            // 16-byte x chunks per row
  constexpr int XC = (XCH + 255) / 256;                 // x chunks per thread
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float red[8];
  u32x4_t* xs = (u32x4_t*)smem;                         // [MT][XCH] bf16 x (normalised)
  float* xsum = (float*)(smem + MT * K * 2);            // F::XSUM: [K / 16] sum of the 16 activations of a piece
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, bx = blockIdx.x;
  const bool silu = p.epi == P3V_EPI_SILU_MUL;
  const bool has_res = p.epi == P3V_EPI_RESID_BF16;
  const int u_begin = wave < wpw ? min(p.units, (bx * wpw + wave) * units_per_wave) : p.units;
  const int u_end = min(p.units, u_begin + units_per_wave);
  const int n_st = (u_end - u_begin) * NST;

  // (MT == 1 is launched for M == 1 only: row 0 and "m < M" are then compile-time, as the one-row kernels had them)
  const auto row = [&](int m) { return MT == 1 ? 0 : min(m, p.M - 1); };
  const auto live = [&](int m) { return MT == 1 || m < p.M; };
  // ---- 1. x / norm-weight loads (oldest in the queue)
  u32x4_t xv[MT][XC], gv[XC];
  const bf16_t* xrow[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    if (STEP == STEP_BEGIN) {
      int id = sp->tok[row(m)];                       // (uniform: a scalar load)
      id = id < 0 ? 0 : (id >= sp->vocab ? sp->vocab - 1 : id);
      xrow[m] = sp->table + (size_t)id * K;
    } else {
      xrow[m] = p.x + (size_t)row(m) * K;
    }
  }
#pragma unroll
  for (int k = 0; k < XC; ++k) {
    const int c = min(tid + k * 256, XCH - 1);
#pragma unroll
    for (int m = 0; m < MT; ++m) xv[m][k] = ((const u32x4_t*)xrow[m])[c];
    gv[k] = p.norm_w ? ((const u32x4_t*)p.norm_w)[c] : (u32x4_t){0, 0, 0, 0};
  }

  // ---- 2. weight pipeline state
  typename F::template Stage<CH> wbuf[2];
  uint32_t rbuf[2][MT];                                  // residual pair (2 bf16) of the row pair, per x row
  auto issue = [&](int gs, auto bufc) {
    constexpr int buf = decltype(bufc)::value;
    const int u = min(u_begin + gs / NST, p.units - 1), s = gs % NST;
    const int r0 = silu ? u : 2 * u;
    const int r1 = silu ? u + p.N : min(2 * u + 1, p.N - 1);
    F::template load<K, CH>(p, r0, r1, s * CH * 64 + lane, wbuf[buf]);
#pragma unroll
    for (int m = 0; m < MT; ++m) {                       // 4-byte aligned: r0 = 2u is even, N is even on this path
      const bf16_t* rp = p.resid + (size_t)row(m) * p.N + 2 * u;
      rbuf[buf][m] = !has_res ? 0u : *(const uint32_t*)rp;
    }
  };
  if (n_st > 0) issue(0, IC0{});

  // ---- 3. RMSNorm prologue (waits for the x loads only) -> LDS
  // (F::XSCALE: what goes to LDS is F::stage_x of the rounded activations; `xkeep` holds them as they were and F::x_unfit says
  // whether an element of this thread's does not take the format's factor -- see 3b)
  [[maybe_unused]] u32x4_t xkeep[F::XSCALE ? MT : 1][F::XSCALE ? XC : 1];
  [[maybe_unused]] uint32_t xacc[2] = {0u, 0xffffffffu};    // (what F::stage_x folds the row into, for F::x_unfit)
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    float r = 1.f;
    if (p.norm_w) {
      float ss = 0.f;
#pragma unroll
      for (int k = 0; k < XC; ++k) {
        if (tid + k * 256 < XCH) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { const float a = bf16lo(xv[m][k][j]), b = bf16hi(xv[m][k][j]); ss += a * a + b * b; }
        }
      }
      ss = wave_sum(ss);
      if (lane == 0) red[wave + 4 * (m & 1)] = ss;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      const float* rr = red + 4 * (m & 1);
      r = rsqrtf(((rr[0] + rr[1]) + (rr[2] + rr[3])) / (float)K + p.eps);
    }
#pragma unroll
    for (int k = 0; k < XC; ++k) {
      const int c = tid + k * 256;
      if (c < XCH) {
        u32x4_t o = xv[m][k];
        if (p.norm_w) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            o[j] = rms_pair(xv[m][k][j], r, gv[k][j]);
        }
        if constexpr (F::XSCALE) {
          xkeep[m][k] = o;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = F::stage_x(p, o[j], xacc);
        }
        xs[m * XCH + c] = live(m) ? o : (u32x4_t){0, 0, 0, 0};
      }
    }
  }
  // ---- 3b. (F::XSCALE) one wave-vote per wave rides on the staging barrier; a workgroup with an unfit element -- uniform, cold --
  // puts the rows back as they were and takes the exact copy of the pipeline below
  [[maybe_unused]] bool x_exact = false;
  if constexpr (F::XSCALE) {
    __shared__ int s_unfit[4];
    const bool any = __builtin_amdgcn_ballot_w64(F::x_unfit(p, xacc)) != 0;
    if (lane == 0) s_unfit[wave] = any;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    x_exact = ((s_unfit[0] | s_unfit[1]) | (s_unfit[2] | s_unfit[3])) != 0;
    if (x_exact) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int k = 0; k < XC; ++k)
          if (tid + k * 256 < XCH) xs[m * XCH + tid + k * 256] = live(m) ? xkeep[m][k] : (u32x4_t){0, 0, 0, 0};
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  } else {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  if constexpr (F::XSUM) {
    for (int pc = tid; pc < K / 16; pc += 256) {         // X of every piece, from the (rounded) activations the dots see
      const u32x4_t a = xs[2 * pc], b = xs[2 * pc + 1];
      float t = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) t += (bf16lo(a[j]) + bf16hi(a[j])) + (bf16lo(b[j]) + bf16hi(b[j]));
      xsum[pc] = t;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

  // ---- 4. pipeline
  F::mark(2);
  float a0[MT], a1[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) a0[m] = a1[m] = 0.f;
  ArgMaxVI best[MT];                                         // STEP_END: this wave's arg-max candidates (lane 0's copy counts)
#pragma unroll
  for (int m = 0; m < MT; ++m) best[m] = ArgMaxVI{-INFINITY, 0x7fffffff};
  auto compute = [&](int gs, auto bufc, auto exactc) {           // exactc: IC1 = F::dot_exact (F::XSCALE, 3b), IC0 = F::dot
    constexpr int buf = decltype(bufc)::value;
    const int s = gs % NST;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        if constexpr (F::XSCALE) {
          if constexpr (decltype(exactc)::value) F::dot_exact(p, wbuf[buf], j, xs + m * XCH, xsum, (s * CH + j) * 64 + lane, a0[m], a1[m]);
          else F::dot(wbuf[buf], j, xs + m * XCH, xsum, (s * CH + j) * 64 + lane, a0[m], a1[m]);
        } else {
          F::dot(wbuf[buf], j, xs + m * XCH, xsum, (s * CH + j) * 64 + lane, a0[m], a1[m]);
        }
      }
    }
    if (s == NST - 1) {                                   // row pair complete (compile-time true when NST == 1)
      const int u = u_begin + gs / NST;
#pragma unroll
      for (int m = 0; m < MT; ++m) { a0[m] = F::finish(wave_sum(a0[m]), wbuf[buf], 0); a1[m] = F::finish(wave_sum(a1[m]), wbuf[buf], 1); }
      if (lane == 0) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          if (live(m)) {
            if (silu) {
              const float g = bf16_round(a0[m]), up = bf16_round(a1[m]);
              const float sg = bf16_round(g * bf16_round(1.f / (1.f + __expf(-g))));
              bf16_t* dst = (bf16_t*)p.out + (size_t)m * p.N + u;
              *dst = f32_to_bf16(sg * up);
            } else if (p.epi == P3V_EPI_F32) {
              ((float*)p.out)[(size_t)m * p.N + 2 * u] = a0[m];
              ((float*)p.out)[(size_t)m * p.N + 2 * u + 1] = a1[m];
            } else {
              float v0 = a0[m], v1 = a1[m];
              if (has_res) { v0 = bf16lo(rbuf[buf][m]) + bf16_round(v0); v1 = bf16hi(rbuf[buf][m]) + bf16_round(v1); }
              uint32_t* dst = (uint32_t*)((bf16_t*)p.out + (size_t)m * p.N + 2 * u);
              *dst = pack_bf16x2(v0, v1);
              if (STEP == STEP_END) {                          // on the values just stored (bf16)
                amax_take(best[m], bf16_round(v0), 2 * u);
                if (2 * u + 1 < p.N) amax_take(best[m], bf16_round(v1), 2 * u + 1);
              }
            }
          }
        }
      }
#pragma unroll
      for (int m = 0; m < MT; ++m) a0[m] = a1[m] = 0.f;
    }
  };
  int gs = 0;
  if constexpr (F::XSCALE) {                              // 3b: the exact form of the loop below, chosen once.  Cold: one stage at a
    if (x_exact) {                                        // time through buffer 0 (which holds stage 0 already), so that it costs the
      for (; gs < n_st; ++gs) {                           // pipelined loop neither registers nor much code
        if (gs > 0) issue(gs, IC0{});
        compute(gs, IC0{}, IC1{});
      }
    }
  }
  while (gs + 2 < n_st) {                                 // branch-free body: counted vmcnt survives
    issue(gs + 1, IC1{});
    compute(gs, IC0{}, IC0{});
    issue(gs + 2, IC0{});
    compute(gs + 1, IC1{}, IC0{});
    gs += 2;
  }
  if (gs + 1 < n_st) {
    issue(gs + 1, IC1{});
    compute(gs, IC0{}, IC0{});
    compute(gs + 1, IC1{}, IC0{});
  } else if (gs < n_st) {
    compute(gs, IC0{}, IC0{});
  }
  if (STEP == STEP_BEGIN && bx == 0) gemv_step_begin_tail<MT>(sp, xrow, MT == 1 ? 1 : p.M, XCH, tid);
  if (STEP == STEP_END) gemv_step_end_tail<MT>(sp, best, MT == 1 ? 1 : p.M, bx, tid);
}

template <class F, int MT, int NST, int CH>
__global__ void __launch_bounds__(256, F::MIN_WG) k_gemv3(typename F::P p, int units_per_wave, int wpw) {
  F::mark(0);
  gemv_stream_body<F, MT, NST, CH, STEP_NONE>(p, units_per_wave, wpw, nullptr);
  F::mark(1);
}

// (the arg-max tail of STEP_END does not fit the registers of a MIN_WG > 1 bound without scratch: it keeps the default)
template <class F, int MT, int NST, int CH, int STEP>
__global__ void __launch_bounds__(256, STEP == STEP_END ? 1 : F::MIN_WG) k_gemv3_step(typename F::P p, int units_per_wave, int wpw, GemvStepP sp) {
  gemv_stream_body<F, MT, NST, CH, STEP>(p, units_per_wave, wpw, &sp);
}

// ---- launching: gemv_route (p3v_gemv_route.hip) holds every rule of what a decode projection call launches; an entry point checks the
// pointers it was given, asks it and launches what it says from its tables of instantiations (below).  A kernel the route names and
// no table holds is an error, never another kernel.
void gemv_route(const p3v_gemv_route_query_t& q, p3v_gemv_route_t* r);

struct GemvKernel { const void* fn; bool lds_raised; };       // one instantiation, and whether its dynamic-LDS limit has been raised
static inline int gemv_launch(GemvKernel& k, const p3v_gemv_route_t& r, void** args, hipStream_t s) {
  return p3v_launch(k.fn, k.lds_raised, r.lds_cap, dim3(r.grid), dim3(r.block), args, r.lds_bytes, s);
}
// the instantiations <SILU, NW, NST> of a rows kernel
struct GemvRowsKernel { int NW, NST; GemvKernel k[2]; };
#define GEMV_ROWS_KERNEL(f, NW, NST) {NW, NST, {{(const void*)f<false, NW, NST>}, {(const void*)f<true, NW, NST>}}}
template <int n>
static int launch_gemv_rows(GemvRowsKernel (&tab)[n], const p3v_gemv_route_t& r, void** args, hipStream_t s) {
  for (GemvRowsKernel& e : tab)
    if (e.NW == r.NW && e.NST == r.NST) return gemv_launch(e.k[r.silu], r, args, s);
  return P3V_ERR_UNSUPPORTED;
}
// the instantiations of the streaming kernel for one format: k[step] (one row: k_gemv3 and the two k_gemv3_step; more rows: k_gemv3)
struct GemvStreamKernel { int MT, NST, CH, scaled; GemvKernel k[3]; };
#define GEMV_STREAM_STEPS(F, scaled, NST, CH) \
  {1, NST, CH, scaled, {{(const void*)k_gemv3<F, 1, NST, CH>}, {(const void*)k_gemv3_step<F, 1, NST, CH, STEP_BEGIN>}, {(const void*)k_gemv3_step<F, 1, NST, CH, STEP_END>}}}
#define GEMV_STREAM_ROWS(F, MT, NST, CH) {MT, NST, CH, 0, {{(const void*)k_gemv3<F, MT, NST, CH>}, {nullptr}, {nullptr}}}
template <class P, int n>
static int launch_gemv_stream(GemvStreamKernel (&tab)[n], const p3v_gemv_route_t& r, P& p, GemvStepP* sp, hipStream_t s) {
  const int step = !sp ? STEP_NONE : sp->tok ? STEP_BEGIN : STEP_END;
  int upw = r.upw, wpw = r.wpw;
  void* args[] = {&p, &upw, &wpw, sp};
  for (GemvStreamKernel& e : tab)
    if (e.MT == r.MT && e.NST == r.NST && e.CH == r.CH && e.scaled == r.scaled && e.k[step].fn) return gemv_launch(e.k[step], r, args, s);
  return P3V_ERR_UNSUPPORTED;
}

// What the four p3v_gemv*_step entries do alike once their own pointers are known to be there, A = that entry point's argument struct:
// exactly one end, the route of that end (anything but the one-row streaming kernel reports P3V_ERR_UNSUPPORTED and the caller keeps
// the separate launches), the step struct's own pointers (`own_ok`: what the entry asks of its own beyond them).  P3V_OK: `r` is
// the launch, `sp` is filled.
template <class A>
static int gemv_step_route(int format, const A* a, int exp_base, const p3v_gemv_step_t* st, p3v_gemv_route_t& r, GemvStepP& sp, bool own_ok = true) {
  const bool begin = st->tok != nullptr;
  if (begin == (st->next_tok != nullptr)) return P3V_ERR_ARG;   // exactly one of the two ends
  gemv_route({format, begin ? P3V_GEMV_STEP_BEGIN : P3V_GEMV_STEP_END, a->M, a->N, a->K, a->epilogue, a->norm_w != nullptr, a->resid != nullptr, exp_base, 0}, &r);
  if (r.status && !r.late) return r.status;
  if (begin) {
    if (!st->embed_table || !st->x_out || !st->cos_t || !st->sin_t || !st->d_past || !st->cos_out || !st->sin_out || st->vocab <= 0) return P3V_ERR_ARG;
    if (((uintptr_t)st->embed_table | (uintptr_t)st->x_out) & 15) return P3V_ERR_ARG;
  } else {
    if (!a->x || !st->tok_out || !st->history || !st->d_step || !st->d_past || !st->ticket || !st->amax_ws) return P3V_ERR_ARG;
    if ((uintptr_t)st->amax_ws & 7) return P3V_ERR_ARG;
  }
  if (!own_ok) return P3V_ERR_ARG;
  sp = {st->tok, st->embed_table, st->vocab, st->x_out, st->cos_t, st->sin_t, st->d_past, st->cos_out, st->sin_out, st->tab_t,
        st->half_dim, st->next_tok, st->tok_out, st->history, st->d_step, st->d_past, st->ticket, st->amax_ws, st->max_steps};
  return r.status;
}
