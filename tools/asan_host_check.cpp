// Host-side AddressSanitizer check of libp3v.so's LAUNCHER code ("optional -fsanitize=address host build").
// Runs on a box WITHOUT a GPU: every call below returns from the launcher's host-side argument validation or is a pure host
// function (workspace sizes, tuning table, version), so no kernel is launched; ASan watches the launchers' own reads of the
// argument structs, the tuning table's string handling and the static state.  Build + run: tools/asan_host_build.sh
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/p3v.h"

static int fails = 0;
#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); ++fails; } \
  } while (0)

int main() {
  EXPECT(p3v_version() > 0);
  // workspace sizing: pure host arithmetic
  EXPECT(p3v_attention_ws_bytes(1, 1, 32, 96, 21) == (int64_t)1 * 32 * 21 * 16 * 98 * 4);
  EXPECT(p3v_attention_ws_bytes(1, 64, 32, 96, 4) == 0);
  EXPECT(p3v_gemm_ws_bytes(128, 3072, 3072, P3V_EPI_NONE) >= 0);
  EXPECT(p3v_gemm_ws_bytes(0, 3072, 3072, P3V_EPI_NONE) == 0);
  p3v_gemm_route_query_t rq = {P3V_GEMM_ENTRY_GEMM, 128, 3072, 8192, 8192, 8192, P3V_EPI_RESID_BF16, 0, 0, 0, 0, 0, 0, 0, 256};
  p3v_gemm_route_t rt;
  EXPECT(p3v_gemm_route(&rq, &rt) == P3V_OK && rt.status == P3V_OK && rt.n_launches == 1 && rt.S == 1 && rt.ws_bytes > 0 && rt.ws_short == 1);
  // tuning table: names are matched as C strings
  int v = -123;
  EXPECT(p3v_get_tuning("gemm_persistent", &v) == P3V_OK);
  EXPECT(p3v_set_tuning("gemm_persistent", v) == P3V_OK);
  EXPECT(p3v_get_tuning("no_such_knob", &v) != P3V_OK);
  EXPECT(p3v_set_tuning("", 1) != P3V_OK);
  std::vector<char> longname(4096, 'x');
  longname.back() = 0;
  EXPECT(p3v_set_tuning(longname.data(), 1) != P3V_OK);
  // argument validation of the launchers: null pointers, bad sizes, misaligned operands -> error codes, no launch
  EXPECT(p3v_gemm(nullptr, nullptr) == P3V_ERR_ARG);
  p3v_gemm_args_t g;
  std::memset(&g, 0, sizeof g);
  EXPECT(p3v_gemm(&g, nullptr) == P3V_ERR_ARG);
  alignas(16) static uint16_t buf[4096];
  g.A = buf; g.W = buf; g.out = buf; g.M = 16; g.N = 64; g.K = 63; g.lda = 63; g.ldw = 63; g.ldo = 64;   // K % 64 != 0
  EXPECT(p3v_gemm(&g, nullptr) == P3V_ERR_ARG);
  g.K = 64; g.lda = 64; g.ldw = 64; g.A = buf + 1;                                                          // misaligned A
  EXPECT(p3v_gemm(&g, nullptr) == P3V_ERR_ARG);
  g.A = buf; g.epilogue = P3V_EPI_RESID_BF16; g.resid = nullptr;                                            // residual missing
  EXPECT(p3v_gemm(&g, nullptr) == P3V_ERR_ARG);
  g.epilogue = 99;
  EXPECT(p3v_gemm(&g, nullptr) == P3V_ERR_ARG);
  g.epilogue = P3V_EPI_NONE; g.M = 0;                                                                        // empty problem: OK, no launch
  EXPECT(p3v_gemm(&g, nullptr) == P3V_OK);
  EXPECT(p3v_rmsnorm(nullptr, nullptr, nullptr, 1, 3072, 1e-5f, nullptr) == P3V_ERR_ARG);
  EXPECT(p3v_rmsnorm(buf, buf, buf, 0, 3072, 1e-5f, nullptr) == P3V_OK);
  EXPECT(p3v_rmsnorm(buf, buf, buf, 1, 3071, 1e-5f, nullptr) == P3V_ERR_ARG);
  EXPECT(p3v_log_softmax(nullptr, buf, 1, 8, nullptr) == P3V_ERR_ARG);
  EXPECT(p3v_log_softmax(buf, buf, 0, 8, nullptr) == P3V_OK);
  EXPECT(p3v_attention(nullptr, nullptr) == P3V_ERR_ARG);
  p3v_attn_args_t a;
  std::memset(&a, 0, sizeof a);
  EXPECT(p3v_attention(&a, nullptr) == P3V_ERR_ARG);
  // the prompt attention's route: null arguments, one shape per kernel, an unsupported head dim (host arithmetic, no device)
  p3v_attn_prompt_route_t pr;
  p3v_attn_prompt_query_t pq = {1, 300, 2, 2, 96, 0, 320, 0, 1, 1, 0, -1, -1, -1, -1, -1, -1};
  EXPECT(p3v_attention_route(nullptr, &pr) == P3V_ERR_ARG && p3v_attention_route(&pq, nullptr) == P3V_ERR_ARG);
  const struct { int L, n_split, has_ws, new_is_cache, attn_old, attn_pp, attn_il, attn_il_waves, kernel; const char* name; } shapes[] = {
      {16, 4, 1, 1, 0, -1, -1, -1, P3V_ATTN_PK_ATTN, "k_attn<96>"},          {300, 0, 0, 1, 1, -1, -1, -1, P3V_ATTN_PK_ATTN, "k_attn<96>"},
      {300, 0, 0, 0, 0, -1, -1, -1, P3V_ATTN_PK_PREFILL, "k_attn_prefill<96>"}, {300, 0, 0, 1, 0, 0, 0, -1, P3V_ATTN_PK_DMA, "k_attn_prefill_dma<96, true>"},
      {300, 0, 0, 1, 0, 1, 0, -1, P3V_ATTN_PK_PP, "k_attn_prefill_pp<96, true>"}, {300, 0, 0, 1, 0, -1, 1, 4, P3V_ATTN_PK_IL4, "k_attn_prefill_il<96, 4>"},
      {300, 0, 0, 1, 0, -1, 1, 8, P3V_ATTN_PK_IL8, "k_attn_prefill_il<96, 8>"}};
  for (const auto& s : shapes) {
    pq.L = s.L, pq.past_t = (s.L + 63) / 64 * 64, pq.n_split = s.n_split, pq.has_ws = s.has_ws, pq.new_is_cache = s.new_is_cache;
    pq.attn_old = s.attn_old, pq.attn_pp = s.attn_pp, pq.attn_il = s.attn_il, pq.attn_il_waves = s.attn_il_waves;
    EXPECT(p3v_attention_route(&pq, &pr) == P3V_OK && pr.status == P3V_OK && pr.kernel == s.kernel && !std::strcmp(pr.kernel_name, s.name));
    EXPECT(pr.merge == (s.n_split > 1) && (pr.lds_bytes > 0) == (s.kernel != P3V_ATTN_PK_ATTN));
  }
  pq.hd = 80;
  EXPECT(p3v_attention_route(&pq, &pr) == P3V_OK && pr.status == P3V_ERR_UNSUPPORTED && pr.kernel == P3V_ATTN_PK_NONE && !pr.kernel_name[0]);
  // the decode projections' route: null arguments, one shape per kernel, a refused shape (cu_count given: host arithmetic, no device)
  p3v_gemv_route_t gr;
  p3v_gemv_route_query_t gq = {P3V_GEMV_FMT_BF16, P3V_GEMV_STEP_NONE, 1, 264, 3072, P3V_EPI_NONE, 0, 1, 0, 256};
  EXPECT(p3v_gemv_route(nullptr, &gr) == P3V_ERR_ARG && p3v_gemv_route(&gq, nullptr) == P3V_ERR_ARG);
  const struct { int format, step, M, N, K, epilogue, exp_base, kernel; const char* name; } gshapes[] = {
      {P3V_GEMV_FMT_BF16, 0, 1, 101, 520, P3V_EPI_NONE, 0, P3V_GEMV_K_GEMV, "k_gemv<1>"},
      {P3V_GEMV_FMT_BF16, 0, 1, 264, 3072, P3V_EPI_NONE, 0, P3V_GEMV_K_GEMV3, "k_gemv3<GemvBf16, 1, 1, 6>"},
      {P3V_GEMV_FMT_B13, 2, 1, 4102, 3072, P3V_EPI_NONE, 97, P3V_GEMV_K_GEMV3, "k_gemv3_step<GemvB13<true>, 1, 1, 6, 2>"},
      {P3V_GEMV_FMT_BF16, 0, 9, 264, 1024, P3V_EPI_SILU_MUL, 0, P3V_GEMV_K_MFMA, "k_gemv_mfma<true>"},
      {P3V_GEMV_FMT_BF16, 0, 8, 264, 8192, P3V_EPI_NONE, 0, P3V_GEMV_K_MFMA8, "k_gemv_mfma8<false, 8, 4>"},
      {P3V_GEMV_FMT_FP8, 0, 2, 24, 3072, P3V_EPI_NONE, 0, P3V_GEMV_K_MFMA_F8, "k_gemv_mfma_f8<false>"},
      {P3V_GEMV_FMT_FP8, 0, 5, 24, 8192, P3V_EPI_SILU_MUL, 0, P3V_GEMV_K_MFMA8_F8, "k_gemv_mfma8_f8<true, 8, 8>"},
      {P3V_GEMV_FMT_Q4, 0, 8, 272, 3072, P3V_EPI_NONE, 0, P3V_GEMV_K_GEMV8_Q4, "k_gemv8_q4<false, 4, 3>"},
      {P3V_GEMV_FMT_Q4, 0, 9, 272, 8192, P3V_EPI_NONE, 0, P3V_GEMV_K_ROWS_Q4, "k_gemm_rows_q4<false, 8, 4>"}};
  for (const auto& s : gshapes) {
    gq.format = s.format, gq.step = s.step, gq.M = s.M, gq.N = s.N, gq.K = s.K, gq.epilogue = s.epilogue, gq.exp_base = s.exp_base;
    EXPECT(p3v_gemv_route(&gq, &gr) == P3V_OK && gr.status == P3V_OK && gr.kernel == s.kernel && !std::strcmp(gr.name, s.name));
    EXPECT(gr.grid > 0 && gr.block > 0 && (gr.upw > 0) == (s.kernel == P3V_GEMV_K_GEMV3));
  }
  gq.format = P3V_GEMV_FMT_Q4, gq.step = 0, gq.M = 2, gq.N = 100, gq.K = 3072;                                 // N % 16
  EXPECT(p3v_gemv_route(&gq, &gr) == P3V_OK && gr.status == P3V_ERR_UNSUPPORTED && gr.kernel == P3V_GEMV_K_NONE && !gr.name[0]);
  gq.format = 7;
  EXPECT(p3v_gemv_route(&gq, &gr) == P3V_OK && gr.status == P3V_ERR_ARG);
  p3v_gemv_args_t gv;
  std::memset(&gv, 0, sizeof gv);
  EXPECT(p3v_gemv(nullptr, nullptr) == P3V_ERR_ARG && p3v_gemv(&gv, nullptr) == P3V_ERR_ARG);
  gv.x = buf; gv.W = buf; gv.out = buf; gv.M = 17; gv.N = 16; gv.K = 3072;                                   // more rows than any kernel takes
  EXPECT(p3v_gemv(&gv, nullptr) == P3V_ERR_ARG);
  gv.M = 9; gv.K = 520;                                                                                      // no kernel for this shape
  EXPECT(p3v_gemv(&gv, nullptr) == P3V_ERR_UNSUPPORTED);
  p3v_attn_decode_args_t d;
  std::memset(&d, 0, sizeof d);
  EXPECT(p3v_attention_decode(&d, nullptr) != P3V_OK);
  std::printf(fails ? "asan host check: %d FAILED\n" : "asan host check: all launcher argument paths clean (%d failures)\n", fails);
  return fails ? 1 : 0;
}
