// The decode projections' route (host only): every rule that decides what p3v_gemv / p3v_gemv_fp8 / p3v_gemv_q4 / p3v_gemv_b13 and
// their _step entries launch, stated ONCE -- for the eight entry points (which check their pointers, ask gemv_route and launch what it
// says from their tables of instantiations), for p3v_gemv_b13_plan and for p3v_gemv_route.  A new K is a row of one of the tables below.
#include <stdio.h>

#include "p3v_common.h"

// K -> (NST, CH) of the streaming kernel, per format: K = NST stages x CH lane loads x 64 lanes x `wpl` weights per lane load (8 bf16 or
// 13-bit codes / 16 e4m3 in 16 bytes, 16 nibbles in 8 bytes); `xsum`: the 4-bit form keeps the sum of every 16 activations behind x in LDS
struct GemvShape { int K, a, b; };
static const struct { int wpl; bool xsum; GemvShape k[2]; } stream_fmt[P3V_GEMV_FMT_COUNT] = {
    {8, false, {{3072, 1, 6}, {8192, 4, 4}}},            // bf16 (8192 = 4 stages x 4 chunks: keeps 2 waves/SIMD resident)
    {16, false, {{3072, 1, 3}, {8192, 2, 4}}},           // e4m3
    {16, true, {{3072, 1, 3}, {8192, 2, 4}}},            // 4-bit
    {8, false, {{3072, 1, 6}, {8192, 4, 4}}}};           // 13-bit codes
// K -> (NW, NST) of the persistent 8-row MFMA kernels: K = NW waves x NST stages x 256 -- and (NW, NL) of the e4m3 one: NL 128-element
// lines per wave slice
static const GemvShape mfma8_k[] = {{1024, 4, 1}, {2048, 4, 2}, {3072, 4, 3}, {4096, 8, 2}, {8192, 8, 4}};
static const GemvShape mfma8_f8_k[] = {{3072, 4, 6}, {8192, 8, 8}};
static const GemvShape rows_q4_k[] = {{3072, 4, 3}, {8192, 8, 4}};   // k_gemv8_q4 and k_gemm_rows_q4: 4 waves x 3 blocks, 8 waves x 4 blocks
template <int n> static const GemvShape* shape_of(const GemvShape (&tab)[n], int K) {
  for (const GemvShape& s : tab) if (s.K == K) return &s;
  return nullptr;
}

// The only device fact a GEMV launcher uses, read once per process
static int device_cus() {
  static int n_cu = 0;
  if (!n_cu) {
    int dev = 0;
    hipDeviceProp_t pr;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&pr, dev) != hipSuccess) return 0;
    n_cu = pr.multiProcessorCount;
  }
  return n_cu;
}

// The scaled form (GemvB13<true>) serves a matrix whose factor 2^(base - 1) leaves the activations room: base - 1 <= 96, so that every
// |x| < 2^32 fits (a row that does not falls back inside the kernel) -- at K = 3072 (qkv, gate_up, the vocabulary head).  K = 8192
// (down) keeps the exact decode: its waves stage 16 KB of x for ONE row pair each, the staging sits in front of the first dot and the
// loop's VALU work hides behind the stream either way (measured 8.86 -> 9.02 us scaled, profiles/pack13_xscale_step_trace_summary.txt),
// so that instantiation is not built.  gemv_b13_xscale = 0 keeps the exact decode everywhere.
#define B13_XSCALE_MAX_SHIFT 96

void gemv_route(const p3v_gemv_route_query_t& q, p3v_gemv_route_t* r) {
  const P3vTuning& t = p3v_tuning();
  const int M = q.M, N = q.N, K = q.K, epi = q.epilogue, fmt = q.format;
  const bool silu = epi == P3V_EPI_SILU_MUL, f32 = epi == P3V_EPI_F32;
  *r = {};
  if (fmt < 0 || fmt >= P3V_GEMV_FMT_COUNT || q.step < P3V_GEMV_STEP_NONE || q.step > P3V_GEMV_STEP_END) { r->status = P3V_ERR_ARG; return; }
  const auto refuse = [&](int status, int late = 0) { *r = {}, r->status = status, r->late = late; };
  const auto launch = [&](int kernel, int grid, int block, size_t lds, bool raise, int cap) {
    r->kernel = kernel, r->grid = grid, r->block = block, r->lds_bytes = (int)lds, r->lds_cap = raise ? cap : 0;
    r->silu = silu && kernel != P3V_GEMV_K_GEMV && kernel != P3V_GEMV_K_GEMV3;             // (those two read the epilogue at run time)
  };
  const bool epi_ok = epi == P3V_EPI_NONE || epi == P3V_EPI_RESID_BF16 || silu || f32;      // what every GEMV kernel's epilogue holds
  const bool resid_missing = epi == P3V_EPI_RESID_BF16 && !q.has_resid;
  const GemvShape* const ss = shape_of(stream_fmt[fmt].k, K);
  const bool b13_scaled = fmt == P3V_GEMV_FMT_B13 && t.gemv_b13_xscale != 0 && q.exp_base - 1 <= B13_XSCALE_MAX_SHIFT && K == 3072;

  // ---- the streaming kernel (one row; bf16: up to four): `units` row pairs on waves-per-CU x CUs waves.  Wave i owns row pairs
  // [i * upw, (i + 1) * upw), cut at `units`; a workgroup is 4 waves of which wpw (4 or 3, p3v_gemv_wpw) stream rows.
  const auto stream = [&](int MT) {
    const int n_cu = q.cu_count > 0 ? q.cu_count : device_cus();
    if (n_cu <= 0) return refuse(P3V_ERR_HIP);
    // waves per CU.  e4m3: a stage is half the bytes of the bf16 kernel's: twice the waves keep as many in flight; 8: 1.321, 16: 1.301,
    // 24: 1.333 ms/step.  13-bit codes: 4 workgroups a CU (at most 128 VGPRs): the decode's VALU operations want the fourth wave of a
    // SIMD, and gemv_b13_wpc = 16 puts it there (gate_up: 4096 waves, all resident); the vocabulary head's fold runs at gemv_b13_wpc_end:
    // 16 waves a CU would not be resident (that kernel is not bounded to 4 workgroups a CU: its arg-max tail does not fit the registers).
    const int wpc = fmt == P3V_GEMV_FMT_BF16 ? t.gemv_wpc : fmt == P3V_GEMV_FMT_FP8 ? t.gemv_f8_wpc : fmt == P3V_GEMV_FMT_Q4 ? t.gemv_q4_wpc :
                    q.step == P3V_GEMV_STEP_END ? t.gemv_b13_wpc_end : t.gemv_b13_wpc;
    const int units = silu ? N : (N + 1) / 2;
    r->upw = p3v_cdiv(units, (long)n_cu * (wpc < 1 ? 1 : wpc));
    if (r->upw < 1) r->upw = 1;
    r->waves = p3v_cdiv(units, r->upw);
    r->wpw = p3v_gemv_wpw(r->waves, n_cu, t.gemv_wpw);
    const int grid = p3v_cdiv(r->waves, r->wpw);
    if (q.step && grid > P3V_GEMV_STEP_MAX_WG) return refuse(P3V_ERR_UNSUPPORTED, 1);    // (amax_ws holds one candidate per workgroup and row)
    const size_t lds = (size_t)MT * K * 2 + (stream_fmt[fmt].xsum ? K / 4 : 0);          // x as bf16 (+ the piece sums)
    launch(P3V_GEMV_K_GEMV3, grid, 256, lds, lds > 48 * 1024, 160 * 1024 - 256);         // (bf16, four x rows of K = 8192)
    r->MT = MT, r->NST = ss->a, r->CH = ss->b, r->scaled = b13_scaled;
  };
  // one row on the streaming kernel: where p3v_gemv* runs it, and so the only place a step's end can be folded in
  const bool stream_one = M == 1 && N % 2 == 0 && ss && (fmt != P3V_GEMV_FMT_BF16 || t.gemv_variant == 3);   // gemv_variant 1: generic kernel only; 3: streaming kernel where it applies
  // ---- the persistent kernels: n_sets row sets of 16 outputs (SiLU: 8 gate + 8 up rows) on <= max_wg workgroups (one per CU: 192-256
  // VGPRs per wave), each walking `per` strided sets (576 sets -> 192 x 3, 1024 -> 256 x 4, 2004 -> 251 x 8, 192 -> 192 x 1)
  const auto persistent = [&](int kernel, const GemvShape* s, int max_wg, size_t lds, bool raise) {
    const int n_sets = p3v_cdiv(N, silu ? 8 : 16), per = p3v_cdiv(n_sets, max_wg);
    launch(kernel, p3v_cdiv(n_sets, per), s->a * 64, lds, raise, 160 * 1024 - 8704);
    r->NW = s->a, r->NST = s->b, r->n_sets = n_sets, r->sets_per_wg = per;
  };

  if (q.step) {
    // The first / last projection of a replayed greedy step with p3v_step_begin / p3v_step_end folded in: one row only: that is where
    // p3v_gemv* itself runs this kernel (2 .. 8 rows go to the MFMA kernels, whose sums associate differently -- a folded step must stay
    // bit-identical to the eager one), no epilogue; anything else the caller keeps as separate launches.
    if (M <= 0 || N <= 0 || K <= 0) return refuse(P3V_ERR_ARG);
    if (!stream_one || epi != P3V_EPI_NONE) return refuse(P3V_ERR_UNSUPPORTED);
    if (fmt == P3V_GEMV_FMT_B13 && (q.exp_base < 1 || q.exp_base > 224)) return refuse(P3V_ERR_ARG);
    return stream(1);
  }
  switch (fmt) {
    case P3V_GEMV_FMT_BF16: {
      if (M <= 0 || M > 16 || N <= 0 || K <= 0 || K % 8) return refuse(P3V_ERR_ARG);
      if (!epi_ok) return refuse(P3V_ERR_UNSUPPORTED);
      if (resid_missing) return refuse(P3V_ERR_ARG);
      const int mt = M <= 1 ? 1 : M <= 2 ? 2 : M <= 4 ? 4 : 8;
      if (stream_one) return stream(1);
      // 2 <= M <= 4: the same streaming kernel with MT activation rows in LDS (full-line weight loads, 4 v_dot2c per row and
      // 16-byte chunk): measured 2.19 vs 2.94 ms/step at B = 2 and 2.64 vs 3.26 at B = 4 against k_gemv_mfma; from M = 5 on the
      // matrix cores take over (at MT = 8 the VALU / LDS work per weight byte catches up: 4.72 ms/step at B = 8 against 4.08
      // with k_gemv_mfma and 3.27 with k_gemv_mfma8).
      // smallest M the 8-row MFMA kernel takes: 2 since it became persistent with the RMSNorm scale in the epilogue (decode step
      // at ctx 2531, B = 2 / 3 / 4: 2.08 / 2.43 / 2.66 ms with the MT-row streaming kernel, 1.99 / 2.16 / 2.35 with this one);
      // P3V_GEMV8_MIN=5 restores the round-1 split
      const int rows8_min = t.gemv8_min;
      if (t.gemv_rows && t.gemv_variant == 3 && M >= 2 && M <= 4 && M < rows8_min && N % 2 == 0 && !f32 && ss) return stream(mt);
      const GemvShape* const m8 = shape_of(mfma8_k, K);
      if (t.gemv_mfma8 && M >= rows8_min && M <= 8 && m8) {
        const size_t lds = (size_t)8 * (K * 2 + 64);
        return persistent(P3V_GEMV_K_MFMA8, m8, t.gemv8_wgs, lds, lds > 40 * 1024);
      }
      if (M >= 2 && K % 1024 == 0 && !t.gemv_no_mfma) return launch(P3V_GEMV_K_MFMA, p3v_cdiv(N, 16), 256, 0, false, 0);   // (4 waves x 8 k-steps of 32 a stage)
      const size_t lds = (size_t)mt * K * 2;
      if (M > 8 || lds > 160 * 1024 - 256) return refuse(P3V_ERR_UNSUPPORTED);
      const int blocks = p3v_cdiv(silu ? N : (N + 1) / 2, 4);                     // a wave per row pair, striding
      launch(P3V_GEMV_K_GEMV, blocks > 2048 ? 2048 : blocks, 256, lds, true, 160 * 1024 - 256);
      r->MT = mt;
      return;
    }
    case P3V_GEMV_FMT_FP8: {
      if (M <= 0 || M > 16 || N <= 0 || N % 2 || !ss) return refuse(P3V_ERR_UNSUPPORTED);
      if (!epi_ok) return refuse(P3V_ERR_UNSUPPORTED);
      if (resid_missing) return refuse(P3V_ERR_ARG);
      if (M == 1) return stream(1);
      if (M >= 5 && M <= 8 && !t.gemv_no_mfma8) {
        const GemvShape* const s = shape_of(mfma8_f8_k, K);
        const size_t lds = (size_t)8 * (K * 2 + 64);
        launch(P3V_GEMV_K_MFMA8_F8, p3v_cdiv(N, silu ? 8 : 16), s->a * 64, lds, lds > 48 * 1024, 160 * 1024 - 512);
        r->NW = s->a, r->NST = s->b;
        return;
      }
      return launch(P3V_GEMV_K_MFMA_F8, p3v_cdiv(N, 16), 256, 0, false, 0);
    }
    case P3V_GEMV_FMT_Q4: {
      const GemvShape* const s = shape_of(rows_q4_k, K);
      if (M >= 2 && M <= 16 && s && (!q.has_norm || M <= 8) && N > 0) {
        // 2 .. 8 rows: k_gemv8_q4 (input RMSNorm optional); 9 .. 16: k_gemm_rows_q4 (the caller normalises)
        if (N % (silu ? 8 : 16)) return refuse(P3V_ERR_UNSUPPORTED);
        if (!epi_ok) return refuse(P3V_ERR_UNSUPPORTED);
        if (resid_missing) return refuse(P3V_ERR_ARG);
        if (M <= 8 && t.gemv_q4_rows8) {
          const size_t lds = (size_t)8 * (K * 2 + 32);
          return persistent(P3V_GEMV_K_GEMV8_Q4, s, t.gemv_q4_rows_wgs, lds, lds > 40 * 1024);
        }
        if (q.has_norm) return refuse(P3V_ERR_UNSUPPORTED, 1);
        return persistent(P3V_GEMV_K_ROWS_Q4, s, t.gemv_q4_rows_wgs, 0, false);
      }
      if (M != 1 || N <= 0 || N % 2 || !ss) return refuse(P3V_ERR_UNSUPPORTED);
      if (!epi_ok) return refuse(P3V_ERR_UNSUPPORTED);
      if (resid_missing) return refuse(P3V_ERR_ARG);
      return stream(1);
    }
    default: {                                                                   // the 13-bit codes: one row only
      if (!epi_ok) return refuse(P3V_ERR_UNSUPPORTED);
      if (resid_missing) return refuse(P3V_ERR_ARG);
      if (M <= 0 || N <= 0) return refuse(P3V_ERR_ARG);
      if (M != 1 || N % 2 || !ss) return refuse(P3V_ERR_UNSUPPORTED);
      if (q.exp_base < 1 || q.exp_base > 224) return refuse(P3V_ERR_ARG);
      return stream(1);
    }
  }
}

extern "C" int p3v_gemv_route(const p3v_gemv_route_query_t* query, p3v_gemv_route_t* route) {
  if (!query || !route) return P3V_ERR_ARG;
  gemv_route(*query, route);
  static const char* const fmt_name[] = {"GemvBf16", "GemvF8", "GemvQ4", "GemvB13<false>", "GemvB13<true>"};
  const p3v_gemv_route_t& r = *route;
  const char* const b = r.silu ? "true" : "false";
  char* const s = route->name;
  const size_t n = sizeof route->name;
  switch (r.kernel) {
    case P3V_GEMV_K_GEMV: snprintf(s, n, "k_gemv<%d>", r.MT); break;
    case P3V_GEMV_K_GEMV3: {
      const char* const f = fmt_name[query->format + r.scaled];
      if (query->step) snprintf(s, n, "k_gemv3_step<%s, %d, %d, %d, %d>", f, r.MT, r.NST, r.CH, query->step);
      else snprintf(s, n, "k_gemv3<%s, %d, %d, %d>", f, r.MT, r.NST, r.CH);
      break;
    }
    case P3V_GEMV_K_MFMA: snprintf(s, n, "k_gemv_mfma<%s>", b); break;
    case P3V_GEMV_K_MFMA8: snprintf(s, n, "k_gemv_mfma8<%s, %d, %d>", b, r.NW, r.NST); break;
    case P3V_GEMV_K_MFMA_F8: snprintf(s, n, "k_gemv_mfma_f8<%s>", b); break;
    case P3V_GEMV_K_MFMA8_F8: snprintf(s, n, "k_gemv_mfma8_f8<%s, %d, %d>", b, r.NW, r.NST); break;
    case P3V_GEMV_K_GEMV8_Q4: snprintf(s, n, "k_gemv8_q4<%s, %d, %d>", b, r.NW, r.NST); break;
    case P3V_GEMV_K_ROWS_Q4: snprintf(s, n, "k_gemm_rows_q4<%s, %d, %d>", b, r.NW, r.NST); break;
    default: break;
  }
  return P3V_OK;
}
