/* p3v.h -- C ABI of the MI355X (gfx950) Phi-3-Vision hot path.
 *
 * The reference (JosefAlbers/Phi-3-Vision-MLX) has no native layer: every
 * tensor op on its hot path is a call into the third-party `mlx` wheel.  Each
 * entry point below therefore replaces one MLX call site (or a fused group of
 * them) in the reference's `phi.py` / `phi_3_vision_mlx.py`; the call site is
 * cited as file:line next to each declaration.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless
 *     marked `host`; bf16 travels as uint16_t;
 *   - `stream` is a hipStream_t passed as void*; launches are stream-ordered,
 *     never synchronise and never allocate (callers pass workspaces);
 *   - return 0 on success, a negative P3V_ERR_* code otherwise; nothing throws;
 *   - re-entrant across streams.  Weights are [out_features, in_features]
 *     row-major (the HF layout the reference loads).
 */
#ifndef P3V_H
#define P3V_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P3V_VERSION 600
#define P3V_OK 0
#define P3V_ERR_ARG (-22)         /* bad shape / null pointer / unsupported size */
#define P3V_ERR_LAUNCH (-5)       /* hipGetLastError() != hipSuccess after launch */
#define P3V_ERR_UNSUPPORTED (-95) /* combination not implemented */
#define P3V_ERR_HIP (-14)         /* a HIP runtime call failed */

typedef struct {
  int cu_count, lds_per_cu, wave_size, clock_khz, mem_clock_khz, mem_bus_bits;
  int64_t hbm_bytes;
  char arch[32];
} p3v_props_t;

int p3v_version(void);
int p3v_device_props(int device, p3v_props_t* out /* host */);
const char* p3v_strerror(int code);

/* Launch-policy knobs ("gemm_big_rows", "gemm_no_splitk", "gemv_wpc", ... -- the table in csrc/p3v_runtime.hip).  Each is
 * read ONCE, on first use, from the environment variable P3V_<NAME IN UPPER CASE>; afterwards only these calls change
 * it (kernel tests pin a kernel variant with them).  No launch reads the environment.  Process-wide, not thread-safe
 * against concurrent launches: set before launching.  P3V_ERR_ARG for an unknown name. */
int p3v_set_tuning(const char* name /* host */, int value);
int p3v_get_tuning(const char* name /* host */, int* value /* host */);

/* ---- embedding gather: nn.Embedding, phi.py:568,577.  Negative ids (image
 * slots, phi.py:270) are clamped to 0; their rows are overwritten later. */
int p3v_embed_gather(const int32_t* ids, const uint16_t* table, uint16_t* out,
                     int n_tok, int hidden, int vocab, void* stream);

/* ---- nn.RMSNorm (= mx.fast.rms_norm), phi.py:478-479,571: y = bf16(bf16(x*rsqrt(mean(x^2)+eps)) * w) -- fp32 statistics, the
 *      normalised row is rounded to bf16 before the weight multiply (pinned by tests/golden/ref_model_tiny.npz) */
int p3v_rmsnorm(const uint16_t* x, const uint16_t* w, uint16_t* y, int rows, int hidden, float eps, void* stream);

/* ---- nn.LayerNorm, phi.py:165,167,212: fp32 in (ViT residual stream); bf16 out (feeds a
 * projection) or fp32 out (pre_layrnorm, which IS the residual stream; may be in place) */
int p3v_layernorm(const float* x, const uint16_t* w, const uint16_t* b, void* y, int out_f32,
                  int rows, int hidden, float eps, void* stream);

/* ---- dense projection  C[M,N] = A[M,K] * W[N,K]^T (+ epilogue), bf16 MFMA, fp32 accumulate.
 * Replaces every nn.Linear on the path (phi.py:140-149,154-159,391,437-438,
 * 465-466,604) and the k=14,s=14 patch conv (phi.py:186-192,199). */
enum {
  P3V_EPI_NONE = 0,        /* out bf16 = acc                                              */
  P3V_EPI_BIAS = 1,        /* out bf16 = acc + bias                                       */
  P3V_EPI_BIAS_QGELU = 2,  /* out bf16 = g(acc+bias), g(x)=x*sigmoid(1.702x)  phi.py:154  */
  P3V_EPI_BIAS_GELU = 3,   /* out bf16 = gelu_erf(acc+bias)                   phi.py:391  */
  P3V_EPI_BIAS_RESID_F32 = 4, /* out f32  = resid_f32 + acc + bias            phi.py:170-171 */
  P3V_EPI_RESID_BF16 = 5,  /* out bf16 = resid + bf16(acc)                    phi.py:460,483-485 */
  P3V_EPI_SILU_MUL = 6,    /* W = [gate;up] (2N rows): out bf16[M,N] = silu(g)*u  phi.py:469-471 */
  P3V_EPI_PATCH = 7,       /* out f32 row (m/P)*(P+1)+1+m%P = acc + pos[1+m%P]   phi.py:199-205 */
  P3V_EPI_F32 = 8          /* out f32 = acc (+ bias if given)                               */
};
/* The roundings every projection kernel makes (p3v_gemm, p3v_gemv and the entry points tied to them bit for bit; pinned on exact-sum
 * inputs by tests/test_proj_kernels_gpu.py).  acc is the fp32 sum over K; bf16() rounds to nearest, ties to even; every other step is
 * one fp32 operation.
 *   NONE, BIAS, BIAS_QGELU, BIAS_GELU: one rounding, of the whole fp32 expression (acc + bias, g(acc + bias)).
 *   RESID_BF16: out = bf16(resid + bf16(acc)) -- TWO roundings: the Linear's output is a bf16 tensor before the residual add.
 *   SILU_MUL:   g = bf16(acc_gate), u = bf16(acc_up); out = bf16(bf16(g * bf16(sigmoid(g))) * u), sigmoid(g) = 1 / (1 + exp(-g)) in
 *               fp32 -- every elementwise op of the reference is a bf16 op (FOUR roundings after the two sums).
 *   BIAS_RESID_F32, PATCH, F32: no rounding; fp32 adds of acc, bias, resid / pos.
 * K slices (the split-K paths) keep their partial sums in fp32 and add them in slice order before any of the above. */
typedef struct {
  const uint16_t* A;   /* [M, lda] bf16 */
  const uint16_t* W;   /* [N or 2N, ldw] bf16 */
  void* out;           /* bf16 or f32, row stride ldo elements */
  const uint16_t* bias;  /* [N] bf16 or null */
  const void* resid;   /* bf16 or f32 [M, ldo] or null; may alias out */
  const uint16_t* pos; /* P3V_EPI_PATCH: position embedding [(P+1), N] bf16 */
  int M, N, K;         /* K % 64 == 0 */
  int lda, ldw, ldo;
  int epilogue;
  int patches_per_img; /* P3V_EPI_PATCH: P (=576) */
  void* ws;            /* caller-owned device workspace (16-byte aligned) or null */
  int64_t ws_bytes;    /* its size; see p3v_gemm_ws_bytes */
} p3v_gemm_args_t;
/* Operands are addressed with 32-bit byte offsets: M * lda * 2 and rows(W) * ldw * 2 must stay below 4 GiB
 * (P3V_ERR_UNSUPPORTED otherwise).  Which kernels a call takes is p3v_gemm_route's answer (below).  Short prompts run split
 * over K through fp32 partials in `ws`: p3v_gemm_ws_bytes(M, N, K, epilogue) is the size that path needs, the route's ws_bytes
 * (0 = the shape does not use a workspace).  The library never allocates, frees or synchronises: with ws == null or too small the same
 * shape runs on the one-pass kernel (slower for short prompts, same results up to fp32 summation order).  The workspace
 * is only live between the two launches of one call, so calls on ONE stream may share it; concurrent streams need their
 * own.  Graph-capturable. */
int p3v_gemm(const p3v_gemm_args_t* args /* host */, void* stream);
int64_t p3v_gemm_ws_bytes(int M, int N, int K, int epilogue);
/* Round 6: 9 .. 32 rows of A on bf16 weights with K = 3072 or 8192 (a 9 .. 32-sequence decode batch; the reference's batched benchmark
 * runs 15, phi_3_vision_mlx.py:1226-1243) take a register-streaming kernel inside p3v_gemm / p3v_gemm_resid_norm (weights HBM ->
 * registers in whole lines, A resident as MFMA fragments): this query says how -- 0 = not that kernel's shape, 1 = one pass,
 * S > 1 = S K slices through the `ws` partials + the reduction launch (the rows kernel's line of the route's split rule).  Host-only. */
int p3v_gemm_rows_slices(int M, int N, int K, int epilogue);

/* ---- skinny projection for decode: y[M,N] = x[M,K] * W[N,K]^T, M <= 16, weight-streaming
 * (M == 1: VALU dot products; 2 <= M <= 16: the weight rows go straight from HBM into MFMA fragments).
 * Same call sites as p3v_gemm when L*B is small.  Optional fused RMSNorm of x
 * (norm_w != null: x is normalised with norm_w/eps before use, phi.py:482,484).
 * Epilogues: NONE, RESID_BF16, SILU_MUL (W = [gate;up]), F32.  Which kernel a shape takes, and which shapes none takes
 * (P3V_ERR_UNSUPPORTED), is p3v_gemv_route's answer (below) -- for this entry and for the other formats' twins. */
typedef struct {
  const uint16_t* x;      /* [M, K] bf16 */
  const uint16_t* W;      /* [N or 2N, K] bf16 */
  void* out;              /* [M, N] bf16 (or f32 for P3V_EPI_F32) */
  const uint16_t* resid;  /* [M, N] bf16 or null; may alias out */
  const uint16_t* norm_w; /* [K] bf16 or null */
  float norm_eps;
  int M, N, K;            /* M <= 16, K % 8 == 0 (otherwise P3V_ERR_ARG); the rest: p3v_gemv_route */
  int epilogue;
} p3v_gemv_args_t;
int p3v_gemv(const p3v_gemv_args_t* args /* host */, void* stream);

/* ---- fp8 (OCP e4m3fn) weight-only projections (quantize_model=True; replaces the int4 `nn.quantize` of
 * phi_3_vision_mlx.py:264,296): W is u8 [N or 2N, K] bit patterns, w = fp8 * w_scale[row]; x, accumulation
 * and outputs as in p3v_gemv.  Shapes and kernels: p3v_gemv_route (P3V_GEMV_FMT_FP8).  Every kernel behind it sums x * fp8 in fp32 first (an e4m3 value
 * is exact in bf16, so each product is) and multiplies the sum by w_scale[row] afterwards, one fp32 rounding; the epilogue's roundings
 * are p3v_gemm's.  p3v_dequant_fp8 expands rows to bf16 (prefill). */
typedef struct {
  const uint16_t* x; const uint8_t* W; const float* w_scale; void* out;
  const uint16_t* resid; const uint16_t* norm_w;
  float norm_eps;
  int M, N, K;
  int epilogue;
} p3v_gemv_fp8_args_t;
int p3v_gemv_fp8(const p3v_gemv_fp8_args_t* args /* host */, void* stream);
int p3v_dequant_fp8(const uint8_t* w8, const float* w_scale, uint16_t* out_bf16, int rows, int K, void* stream);

/* ---- bf16 weights as exact 13-bit codes: the B = 1 decode projections stream 13/16 of the bytes and
 * compute the same bits.  A weight s|e8|m7 is stored as s|q5|m7: q = 0 for +-0, q = e - base + 1 (1 .. 31), one `base` per matrix --
 * 31 consecutive binades ending at the matrix's largest exponent (real checkpoints keep almost everything within 20 .. 30 binades;
 * 4 code bits would only hold the synthetic weights).  A matrix with a value below that window, a denormal, Inf or NaN does not fit.
 * p3v_pack_b13: W [rows, K] bf16 -> `out` (rows * K * 13 / 8 bytes, 16-byte aligned), K = 3072 or 8192, rows even.  The packing follows
 * the row PAIRS the streaming kernel walks: silu_pairs = 0: rows (2u, 2u + 1); silu_pairs = 1: rows (u, u + rows / 2), the gate / up
 * pairs of P3V_EPI_SILU_MUL.  info: 4 int32 on the device, written by the launches: [0] status (0 = packed; non-zero = W does not fit
 * and `out` is undefined), [1] base, [2] / [3] smallest / largest biased exponent of the non-zero weights.  The caller reads info once,
 * at load time.  p3v_unpack_b13 restores the bf16 rows bit for bit (tests). */
int p3v_pack_b13(const uint16_t* W, int rows, int K, int silu_pairs, void* out, int32_t* info, void* stream);
int p3v_unpack_b13(const void* packed, int rows, int K, int silu_pairs, int exp_base, uint16_t* out_bf16, void* stream);
/* p3v_gemv on packed weights: M = 1 only (P3V_ERR_UNSUPPORTED otherwise: the caller keeps the bf16 copy for more rows; shapes and
 * the form of the kernel: p3v_gemv_route, P3V_GEMV_FMT_B13), every epilogue and the fused RMSNorm of p3v_gemv; bit-identical to p3v_gemv on the bf16 matrix.
 * silu_pairs must be what the matrix was packed with and equal (epilogue == P3V_EPI_SILU_MUL).
 * Knob gemv_b13_xscale (default 1): for a matrix with K = 3072 and exp_base - 1 <= 96 the kernel does not add the base back to every weight; it
 * multiplies the activations it stages by 2^(exp_base - 1) once (a power of two: every product is the same number) and feeds the
 * codes to the dot product as they are.  That holds for a row of zeros and normal numbers with |x| * 2^(exp_base - 1) finite --
 * every |x| < 2^32; a row with any other element (larger, Inf, NaN, a bf16 denormal) is served by the exact decode inside the same
 * launch, as are matrices with a larger base, K = 8192 (measured slower there) and everything at gemv_b13_xscale = 0.  The bits out do
 * not depend on which form ran. */
typedef struct {
  const uint16_t* x; const void* W; void* out;
  const uint16_t* resid; const uint16_t* norm_w;
  float norm_eps;
  int M, N, K;
  int epilogue;
  int exp_base, silu_pairs;
} p3v_gemv_b13_args_t;
int p3v_gemv_b13(const p3v_gemv_b13_args_t* args /* host */, void* stream);
/* How p3v_gemv_b13 / p3v_gemv_b13_step cut a launch of N outputs (as in `args`) on `n_cu` compute units at the current knobs
 * (gemv_b13_wpc, gemv_wpw; the end fold of p3v_gemv_b13_step runs at gemv_b13_wpc_end instead) -- a projection of p3v_gemv_route, callable without a GPU.  out[0] row pairs per wave, out[1] waves that
 * take rows (wave i: row pairs [i * out[0], (i + 1) * out[0]), cut at the end), out[2] row-streaming waves per 4-wave workgroup,
 * out[3] workgroups. */
int p3v_gemv_b13_plan(int N, int K, int epilogue, int n_cu, int* out /* host, 4 ints */);

/* ---- W8A8 projection on the fp8 matrix cores (BASELINE config 5, prompt-sized inputs; the same call sites:
 * QuantizedLinear, phi_3_vision_mlx.py:264,291-305, under `quantize_model=True`).
 *   out[M, N] = epilogue((a_scale[m] * w_scale[n]) * sum_k A8[m,k] * W8[n,k])     A8 [M, lda], W8 [N or 2N, ldw]: e4m3 bytes
 * on v_mfma_scale_f32_16x16x128_f8f6f4 (block scales 1.0).  epilogue: P3V_EPI_NONE, P3V_EPI_RESID_BF16 (resid bf16 [M, ldo]),
 * P3V_EPI_SILU_MUL (W8 / w_scale hold the N gate rows then the N up rows; out [M, N]).  K % 128 == 0, N % 128 == 0 (every
 * epilogue: an N that is no multiple of 256 runs on the 256 x 128 tile, which the launcher also picks where the wide one would
 * leave most of the chip idle; knob gemm_f8_narrow = 0 / 1 pins the tile where both fit), lda, ldw >= K and % 16 == 0, ldo % 8 == 0,
 * 16-byte aligned pointers.  The sum over k is exact products added in fp32; it is multiplied ONCE by the fp32 product
 * a_scale[m] * w_scale[n], then the epilogue's roundings are p3v_gemm's (pinned on exact-sum inputs by tests/test_qproj_kernels_gpu.py).
 * p3v_quant_fp8_rows makes A8 / a_scale from bf16 rows: one scale s per row = max|h| / 448, codes e4m3(h * (1 / s)),
 * h = x or, with norm_w,
 * h = bf16(x * rsqrt(mean x^2 + eps) * norm_w) (nn.RMSNorm, phi.py:478-479), so the norm costs no extra pass. */
typedef struct {
  const uint8_t* A; const float* a_scale; const uint8_t* W; const float* w_scale;
  uint16_t* out; const uint16_t* resid;
  int M, N, K, lda, ldw, ldo, epilogue;
} p3v_gemm_fp8_args_t;
int p3v_gemm_fp8(const p3v_gemm_fp8_args_t* args /* host */, void* stream);
int p3v_quant_fp8_rows(const uint16_t* x, const uint16_t* norm_w /* optional */, float eps, uint8_t* q, float* scale,
                       int rows, int K, void* stream);

/* ---- SuRoPE tables, phi.py:487-504: cos/sin[n_pos, half] = {cos,sin}(pos*inv_freq)*scale (fp32) */
int p3v_rope_table(const float* pos, const float* inv_freq, float scale, float* cos_out, float* sin_out,
                   int n_pos, int half_dim, void* stream);

/* ---- split + RoPE + KV append, phi.py:443-452 and 542-548.
 * qkv [B*L, (nh+2*nkv)*hd] bf16 -> q_out [B, nh, L, hd] bf16 (rotated),
 * K (rotated) -> k_dst[b, h, dst_off + l, :]   (K   layout [B, nkv, dst_t, hd]),
 * V           -> v_dst[b, h, :, dst_off + l]   (V^T layout [B, nkv, hd, dst_t]: the PV product
 * then reads 8 consecutive keys per lane with one 16-byte load, like QK^T does for K).
 * cos/sin tables are [B/tab_div, tab_t, hd/2]; position of (b,l) is past+l.
 * cos_t == sin_t == NULL: no rotation, plain head split (CLIP q/k/v, phi.py:147).
 * `d_past` (device int32, may be null) overrides `past` -- used under graph replay.
 * q_scale: rotated queries are multiplied by it BEFORE their one rounding to bf16 (phi.py:454 scales q before the
 * product too); 1.0f = plain.  With q_scale = scale * log2(e) the attention call takes q_prescaled = 1 and its softmax
 * needs no multiply per score.  Applies to the plain head split as well (q = bf16(q * q_scale), bit for bit; the ViT path
 * does not use it: tests only).  Prompt-sized calls (L >= 32) run the split / rotation and the V transpose as ONE launch. */
int p3v_rope_kv_append(const uint16_t* qkv, const float* cos_t, const float* sin_t,
                       uint16_t* q_out, uint16_t* k_dst, uint16_t* v_dst,
                       int B, int L, int n_heads, int n_kv, int hd,
                       int past, const int32_t* d_past, int dst_t, int dst_off_is_past,
                       int tab_t, int tab_div, float q_scale, void* stream);

/* ---- a residual projection whose consumer is an RMSNorm, as one launch sequence (round 5; phi.py:478-484: `r + o_proj(...)` followed
 *      by `post_attention_layernorm`, `r + down_proj(...)` followed by the next layer's `input_layernorm`):
 *      p3v_gemm_resid_norm(g, w, eps, normed) == p3v_gemm(g) with P3V_EPI_RESID_BF16 + p3v_rmsnorm(g->out, w, normed, M, N, eps), bit
 *      for bit, where the route (p3v_gemm_route, entry P3V_GEMM_ENTRY_RESID_NORM) runs the projection as K slices: the fp32 partials are
 *      summed, the residual added, the row normalised by the SAME launch.  P3V_ERR_UNSUPPORTED -- nothing launched, the caller runs the
 *      two calls -- wherever the route says so (no split, no workspace of p3v_gemm_ws_bytes(), N > 3072).  normed: bf16 [M, N] contiguous. */
int p3v_gemm_resid_norm(const p3v_gemm_args_t* gemm /* host */, const uint16_t* norm_w, float eps, uint16_t* normed, void* stream);

/* ---- the qkv projection with the split, the rotation and the KV append in its EPILOGUE (round 5):
 *      p3v_gemm_qkv(g, s) == p3v_gemm(g) into a scratch [M, N] + p3v_rope_kv_append(scratch, ...) with s's arguments, bit for bit, in the
 *      GEMM's launches alone (phi.py:437-452 / 140-147: `qkv_proj` + `split` + `_rotate_half` + KVCache append; CLIP: q/k/v projections
 *      + head split).  g: A [B*L, K], W [(nh + 2 nkv) * hd, K] (q rows, k rows, v rows), epilogue P3V_EPI_NONE or P3V_EPI_BIAS; out /
 *      resid / ws unused.  P3V_ERR_UNSUPPORTED (nothing launched) wherever the route (p3v_gemm_route, entry P3V_GEMM_ENTRY_QKV)
 *      says so -- callers then run the two calls.  Batch rows of ANY length: B * L > 8 is all the route asks of B and L, every token
 *      lands at its own (b, l) however many row ends an 8-token V^T run crosses (L < 8), and nothing outside q_out, k_dst[.., dst_off ..
 *      dst_off + L, :] and v_dst[.., :, dst_off .. dst_off + L] is written.  Heads of 32, 64, 96 and 128 dimensions (p3v_rope_kv_append
 *      stops at 96: at 128 there are no two calls to compare with). */
typedef struct {
  const float* cos_t; const float* sin_t;          /* as p3v_rope_kv_append; both null: plain head split */
  uint16_t* q_out; uint16_t* k_dst; uint16_t* v_dst;
  int B, L, n_heads, n_kv, hd;
  int past, dst_t, dst_off_is_past, tab_t, tab_div;
  float q_scale;
} p3v_qkv_split_t;
int p3v_gemm_qkv(const p3v_gemm_args_t* gemm /* host */, const p3v_qkv_split_t* split /* host */, void* stream);

/* ---- the bf16 prefill GEMM's route: what p3v_gemm / p3v_gemm_resid_norm / p3v_gemm_qkv launch for a call.  The shape must pass the
 * entry points' own checks (K % 64, N % 8, lda and ldw >= K and multiples of 8; qkv: N == (n_heads + 2 n_kv) * hd) or the answer
 * is P3V_ERR_ARG; pointers are not its business.  The three entry points ask this one function and launch what it says; p3v_gemm_ws_bytes and
 * p3v_gemm_rows_slices are projections of it (host-only, no launch).  The `gemm_*` knobs are read from the library's current settings
 * (p3v_set_tuning works without a device).  cu_count <= 0 asks the current device, as the entry points do, and only where a
 * 256 x 256-tile launch is part of the route: with cu_count given the function touches no device (tests/test_gemm_route_cpu.py). */
typedef enum { P3V_GEMM_ENTRY_GEMM = 0, P3V_GEMM_ENTRY_RESID_NORM = 1, P3V_GEMM_ENTRY_QKV = 2 } p3v_gemm_entry_t;
typedef enum {
  P3V_GEMM_K_ROWS = 0,          /* k_gemm_rows: 9 .. 32 rows, weights straight to registers (tile_m = 16 or 32 rows held) */
  P3V_GEMM_K_SKINNY,            /* k_gemm_skinny: tile_m (64 or 128) x 64 tiles, weight-streaming */
  P3V_GEMM_K_SKINNY_QKV,        /*   ... with the qkv epilogue */
  P3V_GEMM_K_128,               /* k_gemm: 128 x 128 tiles (S > 1: fp32 K-slice partials) */
  P3V_GEMM_K_128_QKV,
  P3V_GEMM_K_256,               /* k_gemm256: 256 x 256 tiles */
  P3V_GEMM_K_256_QKV,
  P3V_GEMM_K_REDUCE,            /* k_splitk_reduce: adds the S partials, applies the epilogue */
  P3V_GEMM_K_REDUCE_NORM,       /* k_splitk_reduce_norm: ... and the RMSNorm of p3v_gemm_resid_norm */
  P3V_GEMM_K_COUNT
} p3v_gemm_kernel_t;
typedef struct {
  int entry;                    /* p3v_gemm_entry_t */
  int M, N, K, lda, ldw;
  int epilogue, has_bias;
  int64_t ws_bytes;             /* the workspace offered (0: none) */
  int n_heads, n_kv, hd;        /* P3V_GEMM_ENTRY_QKV */
  int dst_off, dst_t;           /*   the append offset (past if dst_off_is_past, else 0) and the cache's row length */
  int cu_count;
} p3v_gemm_route_query_t;
typedef struct {
  int kernel;                   /* p3v_gemm_kernel_t */
  int grid[3], block;
  int row0, rows;               /* the rows of A the launch covers (a reduction: the rows of the partials it finishes) */
  int tile_m;                   /* rows of A per workgroup */
  char name[48];                /* as a profiler prints it: "k_gemm_skinny<5, true, 64, 128>" (filled by p3v_gemm_route only) */
} p3v_gemm_launch_t;
typedef struct {
  int status;                   /* P3V_OK, or P3V_ERR_UNSUPPORTED (then no launch); P3V_ERR_HIP: no device answered for cu_count */
  int n_launches;
  p3v_gemm_launch_t launch[3];  /* in order */
  int S;                        /* K slices the launches run (1: one pass) */
  int64_t ws_bytes;             /* the workspace the shape's split needs, whatever was offered (0: no split): p3v_gemm_ws_bytes */
  int ws_short;                 /* 1: ws_bytes > 0 and the workspace offered is smaller: the call runs without that split */
} p3v_gemm_route_t;
int p3v_gemm_route(const p3v_gemm_route_query_t* query /* host */, p3v_gemm_route_t* route /* host */);

/* ---- attention, phi.py:454-457 (decoder, causal + left-pad, Mask4D phi.py:550-563)
 * and phi.py:148 (CLIP, no mask).  q [B, nh, L, hd]; keys/values come from two
 * segments: positions [0,past) from (k_past,v_past) batch row b/past_div
 * (K [.., past_t, hd], V^T [.., hd, past_t]), positions [past,past+L) from
 * (k_new,v_new) batch row b (K [.., new_t, hd], V^T [.., hd, new_t]) -- or, with
 * new_is_cache, from (k_past,v_past) as well (the normal case: rows were just
 * appended to the cache).  V^T columns beyond the valid keys must hold finite values.
 * out [B, L, nh*hd] bf16.
 * Query i sees key t iff (!causal || t <= past+i) && t >= pad_len[b]; a query
 * that is itself padding outputs 0.  hd in {64, 96}.
 * What the prompt path (L > P3V_DECODE_MAX_L) rounds: the scores q . k accumulate in fp32 and are not rounded; with
 * q_prescaled, P = 2^(s - r) is taken against a per-query exponent reference r -- the row maximum of the query's first
 * visible 64-key tile, raised to the running row maximum at the latest when a score exceeds it by more than 8 (so r <= max s <= r + 8
 * at the end of every tile, P <= 2^8) -- and ROUNDED TO bf16 before P x V; the row sum is taken over the same rounded P
 * and, like P x V, accumulated in fp32; the output P x V / sum P is rounded to bf16 ONCE.  Nothing is read outside
 * [pad_len[b], past + L) for its value: finite K rows / V^T columns in the dead positions of a walked tile do not reach
 * the output, and no buffer but `out` is written (tests/test_attn_prefill_probe_gpu.py holds the pre-scaled kernels to
 * this against plain fp64). */
typedef struct {
  const uint16_t* q;
  const uint16_t* k_past; const uint16_t* v_past;
  const uint16_t* k_new;  const uint16_t* v_new;
  uint16_t* out;
  const int32_t* pad_len;   /* [B/past_div... indexed by b/pad_div] or null */
  const int32_t* d_past;    /* device override of `past` or null */
  float* ws;                /* split-KV workspace (decode path) or null */
  int B, L, n_heads, n_kv, hd;
  int past, past_t, past_div, new_t, pad_div;
  int causal;
  float scale;
  int n_split;              /* decode path: KV splits (<=1: no split) */
  int new_is_cache;         /* 1: (k_new,v_new) ignored, rows [past,past+L) are read from (k_past,v_past) too --
                               used with d_past, when the append offset is only known on the device */
  int q_prescaled;          /* 1: q already carries scale * log2(e) (p3v_rope_kv_append's q_scale); `scale` is then unused */
} p3v_attn_args_t;
int p3v_attention(const p3v_attn_args_t* args /* host */, void* stream);
/* bytes of workspace p3v_attention needs for the decode (L<=P3V_DECODE_MAX_L) path */
int64_t p3v_attention_ws_bytes(int B, int L, int n_heads, int hd, int n_split);
#define P3V_DECODE_MAX_L 16
/* ---- p3v_attention's route: which kernel a call launches, with what grid, block and dynamic LDS, and whether a merge launch
 * follows -- p3v_attention asks this one function and launches what it says (host-only, no launch).  It depends on no device
 * property and touches no device (tests/test_attn_prompt_route_cpu.py).  A negative knob means the library's current setting
 * (p3v_set_tuning), which for attn_pp, attn_il, attn_il_waves and combine_g may itself be -1: by shape. */
typedef enum {
  P3V_ATTN_PK_NONE = -1,        /* nothing is launched: a refused call, or B * L == 0 */
  P3V_ATTN_PK_ATTN = 0,         /* k_attn: 64 queries per workgroup; split mode (L <= P3V_DECODE_MAX_L, n_split > 1) and attn_old */
  P3V_ATTN_PK_PREFILL,          /* k_attn_prefill: 128 queries, tiles through registers: keys outside the cache, ragged capacity */
  P3V_ATTN_PK_DMA,              /* k_attn_prefill_dma: 128 queries, LDS-DMA tiles */
  P3V_ATTN_PK_PP,               /* k_attn_prefill_pp: 256 queries, ping-pong wave groups */
  P3V_ATTN_PK_IL4,              /* k_attn_prefill_il<hd, 4>: interleaved, 128 queries (pre-scaled Q only) */
  P3V_ATTN_PK_IL8,              /* k_attn_prefill_il<hd, 8>: interleaved, 256 queries */
  P3V_ATTN_PK_COUNT
} p3v_attn_prompt_kernel_t;
typedef struct {
  int B, L, n_heads, n_kv, hd, past, past_t, n_split, new_is_cache, q_prescaled;   /* as in p3v_attn_args_t */
  int has_ws;                   /* nonzero: the call brings a workspace */
  int attn_old, attn_no_dma, attn_pp, attn_il, attn_il_waves, combine_g;            /* the tuning knobs the route depends on */
} p3v_attn_prompt_query_t;
typedef struct {
  int status;                   /* what p3v_attention returns for these fields: P3V_OK, P3V_ERR_UNSUPPORTED (hd), P3V_ERR_ARG */
  int kernel;                   /* p3v_attn_prompt_kernel_t */
  int grid[3], block;
  int lds_bytes;                /* dynamic LDS of the launch (0: k_attn) */
  int head_group;               /* dma / pp / il: heads whose query blocks are interleaved in launch order (0 elsewhere) */
  int merge;                    /* 1: a k_attn_combine2 launch follows (split mode), else 0 */
  int merge_grid, merge_block;
  const char* kernel_name;      /* as a profiler prints them: "k_attn_prefill_dma<96, true>", "k_attn_combine2"; "" for no launch */
  const char* merge_name;
} p3v_attn_prompt_route_t;
int p3v_attention_route(const p3v_attn_prompt_query_t* query /* host */, p3v_attn_prompt_route_t* route /* host */);

/* ---- fused decode-step attention (L <= P3V_DECODE_MAX_L new tokens, no beams): head split +
 * _rotate_half + KVCache append + split-KV attention + merge in one call (phi.py:443-457, 542-548).
 * qkv [B*L, (nh+2*nkv)*hd] is the raw projection; positions [past, past+L) of the caches
 * (K [B, nkv, cache_t, hd], V^T [B, nkv, hd, cache_t], cache_t % 64 == 0) are written,
 * positions [0, past) read.  cos_t/sin_t point at the rows of the NEW positions: row
 * (b, r) = b*rope_bstride + r, r in [0, L) (either a view into the prompt tables at `past`, or
 * the compact buffers p3v_stage_rope fills when `past` only lives on the device);
 * ws >= p3v_attention_ws_bytes(B, L, nh, hd, n_split) even when n_split == 1.  hd == 96.
 * Key ranges of the splits are a static function of cache_t, so loads start before d_past arrives.
 * `past` with d_past != NULL: a LOWER BOUND of *d_past known when the launch is recorded (a captured decode step: the prompt
 * length), or negative for "none".  The 128-key kernel requests tiles below the bound at once; tiles at or beyond it wait
 * for *d_past and fetch nothing when they lie wholly past the live keys (the capacity is prompt + max_tokens).
 * Query row i of batch row b sees key t iff pad_len[b] <= t <= past + i.  Every other position of the caches -- the left padding
 * [0, pad_len[b]) and everything at or beyond the live length past + L -- must hold FINITE values and is otherwise ignored: whatever
 * finite K rows / V^T columns lie there, however large, the output does not depend on them (nothing is promised for NaN or
 * infinities), and no byte outside [past, past + L) is written.  Splits that hold no live key contribute nothing.
 * (tests/test_attn_probe_gpu.py pins this against fp64 with 1e4 in every dead position, at 640 .. 33,280 keys of capacity.) */
typedef struct {
  const uint16_t* qkv; const float* cos_t; const float* sin_t;
  uint16_t* k_cache; uint16_t* v_cache; uint16_t* out;
  const int32_t* pad_len; const int32_t* d_past; float* ws;
  int B, L, n_heads, n_kv, hd, past, cache_t, rope_bstride, n_split;
  float scale;
  int merge_in_launch; /* nonzero: the split-KV partials are merged by the last split of each (b, head) INSIDE the attention
                          launch; 0 = a separate merge launch.  Either way `ws` must hold 0xFF in every byte before its first use
                          (hipMemset) and every launch leaves it so: a partial word is valid when it is not the all-ones pattern */
  /* optional (round 4): the layer's o_proj + residual in the SAME launch (phi.py:460, 483), for shapes
   * p3v_attention_decode_can_fuse_oproj() accepts.  o_proj_w [o_n, n_heads * hd] bf16; o_proj_x [o_n] bf16 is the residual row,
   * updated in place: x += bf16(W_o . attention output), bit-identical to p3v_gemv with P3V_EPI_RESID_BF16 on `out`.  `out` must
   * hold 0xFF in every byte when the launch starts (the projecting workgroups poll its words); `o_rearm` (n_heads * hd bf16) is
   * set to 0xFF by the launch: callers alternate two output buffers between consecutive layers.  NULL o_proj_w = plain attention. */
  const void* o_proj_w; uint16_t* o_proj_x; uint16_t* o_rearm; int o_n;
  /* ... or on MLX 4-bit group-64 weights (the device layout p3v_gemv_q4 takes): o_proj_w = W4 [o_n, n_heads * hd / 8] u32 and
   * o_proj_sb != NULL = its scale | bias words [o_n, n_heads * hd / 64]; bit-identical to p3v_gemv_q4 with P3V_EPI_RESID_BF16. */
  const uint32_t* o_proj_sb;
} p3v_attn_decode_args_t;
int p3v_attention_decode(const p3v_attn_decode_args_t* args /* host */, void* stream);
/* Does p3v_attention_decode take `o_proj_w` for this shape on this device (host query, no launch)?  0 = no; 1 = attention + o_proj +
 * residual in ONE launch (merge_in_launch = 1, the 128-key one-tile plan); 2 (round 6) = merge_in_launch = 0: the launch that merges
 * the split-KV partials also carries the o_proj + residual (long contexts, 64-key plans) -- same arguments, same bits. */
int p3v_attention_decode_can_fuse_oproj(int B, int L, int n_heads, int hd, int n_split, int cache_t, int o_n, int merge_in_launch);
/* Which role workgroup `wg` of the fused launch's 1-D grid (n_heads * n_split workgroups) plays under placement `map` (the
 * attn_fo_map tuning knob: 2 = default, 1 = the round's first form): out[0] = key split, out[1] = head, out[2] / out[3] = its
 * projection units (rows [8 u, 8 u + 8) of o_proj; -1 = none).  Split n_split - 1 of a head is its merging workgroup.  Workgroups
 * L and L +- 256 share a CU on this part (round-robin dispatch), which is what the placement is built on: mergers sit alone with
 * one tile-only workgroup, projection units ride on the last workgroup of every other CU.  Returns P3V_ERR_UNSUPPORTED for shapes
 * the placement does not cover (the launch then uses the (split, head) grid).  Host-only, no GPU needed: tests/test_abi.py. */
int p3v_attention_decode_fused_role(int wg, int n_heads, int n_split, int o_n, int map, int* out4);
/* ---- shared-prefix decode attention: p3v_attention_decode for L == 1 on the bf16 cache, plus a FAMILY TABLE that names the rows
 * whose caches are identical up to a column (the rows p3v_kv_fork filled from one prefill).  The prompt keys of a family are read
 * once, from its leader's cache, for all of its members; `out` and the caches come out bit for bit as with a table of single rows.
 * `family`: DEVICE memory, int32 [B, P3V_FAMILY_INTS], read by the kernel when it runs (a captured launch follows a rewritten table).
 * Row b = {lead, share_end, member[P3V_FAMILY_MAX]}:
 *   lead       the row whose cache the shared keys are read from; lead == b for a leader and for a single row;
 *   share_end  caches of the family are identical in columns [pad, share_end); share_end <= past; the same on every row of a family
 *              (0 on a single row);
 *   member[]   on a leader's row: the rows of its family, the leader included, each once, in any order, unused entries -1.
 *              Ignored on a follower's row.  A single row lists itself or nothing.
 * With chunk = round_up_64(ceil(cache_t / n_split)), the launcher's keys per split, split s of row b is SHARED iff b's family has
 * at least two members and (s + 1) * chunk <= share_end.  A shared split is computed by the leader's workgroup alone: keys from the
 * leader's cache, member j's own rotated query and own pad_len[member j], member j's partial written to ITS workspace record; the
 * followers' workgroups of that split fetch nothing and write nothing.  Every other split -- the one that contains share_end, all
 * later ones, all splits of single rows -- runs as in p3v_attention_decode: own cache, own new position appended at `past`.
 * So for a FOLLOWER columns [0, floor(share_end / chunk) * chunk) of its own cache are dead positions in the sense above: they must
 * hold finite values, and the output does not depend on them.  Nothing outside column `past` of the caches is written.
 * Same arguments, workspace and sentinel rule as p3v_attention_decode; the partials are merged by its merge launch.
 * P3V_ERR_UNSUPPORTED, nothing written, nothing launched: L != 1, hd != 96, a non-null o_proj_w, merge_in_launch != 0, and -- read
 * from `family_host`, the HOST's copy of the table, when it is not NULL -- a lead or a member outside [0, B), more than
 * P3V_FAMILY_MAX rows naming one leader, a share_end beyond `past` when d_past is NULL.  P3V_ERR_ARG for a host copy that
 * contradicts itself (a leader that follows another row, a row missing from or twice in its leader's list, a listed row that names
 * another leader, two share_end in one family) and for null / misaligned pointers.  family_host == NULL skips those checks (a
 * table the host has validated before, e.g. while a step is being captured); the kernel then still reads no row outside [0, B): an
 * entry out of range names nobody, and share_end counts up to `past` at most.
 * An unvalidated table that contradicts itself (a follower its leader does not list, a leader with one member, ...) yields
 * UNDEFINED OUTPUT for the rows involved -- typically NaN: the follower's workspace record stays at the sentinel -- and nothing worse.
 * (tests/test_attn_family_gpu.py pins out / cache bit equality against the all-singles table and the unread follower columns.) */
#define P3V_FAMILY_MAX 16                       /* members of one family: P3V_KV_FORK_MAX_DST + the source row */
#define P3V_FAMILY_INTS (2 + P3V_FAMILY_MAX)
int p3v_attention_decode_family(const p3v_attn_decode_args_t* args /* host */, const int32_t* family /* device */,
                                const int32_t* family_host /* host or NULL */, void* stream);
/* cos/sin rows of positions [past, past+L) of each batch row ([B, tab_t, half] tables) -> [B, L, half] */
int p3v_stage_rope(const float* cos_t, const float* sin_t, int past, const int32_t* d_past,
                   float* cos_out, float* sin_out, int B, int L, int tab_t, int half_dim, void* stream);

/* ---- int8 KV cache (quantize_cache=True; replaces the 4-bit prompt cache of phi.py:528-540).
 * Bytes are offset-binary u = round(x/s)+128 with one fp32 scale per (batch row, kv head, token):
 * K8 [B*nkv, dst_t, hd], V8^T [B*nkv, hd, dst_t], scales [B*nkv, dst_t].
 * p3v_kv_quantize converts rows [t0, t0+n_tok) of a bf16 K [BH, src_t, hd] / V^T [BH, hd, src_t] pair. */
int p3v_kv_quantize(const uint16_t* k, const uint16_t* vt, uint8_t* k8, uint8_t* v8t, float* k_scale, float* v_scale,
                    int BH, int hd, int src_t, int dst_t, int t0, int n_tok, void* stream);
/* p3v_attention_decode on the int8 cache: same contract; the step's own new rows are quantised,
 * appended, and attended in their quantised form (one representation per key, whenever it is read).
 * Dead positions (left padding, at or beyond past + L): any codes with FINITE scales, otherwise ignored, as for the bf16 cache. */
/* the inverse, tokens [0, n_tok) of every (batch row, kv head): bf16 K [BH, dst_t, hd] / V^T [BH, hd, dst_t] = (code - 128) * scale.
 * For cached calls with more than 16 new tokens on the int8 cache (they attend through p3v_attention on this copy). */
int p3v_kv_dequantize(const uint8_t* k8, const uint8_t* v8t, const float* k_scale, const float* v_scale, uint16_t* k,
                      uint16_t* vt, int BH, int hd, int src_t, int dst_t, int n_tok, void* stream);

/* ---- the reference's OWN quantised cache, as an opt-in (load(..., quantize_cache=True, cache_format="mlx4")): phi.py:528-540 -- on the
 * first call mx.quantize(keys.reshape(B*N, -1), group_size=32) (4 bits): every token's hd values are hd / 32 affine groups; later
 * calls attend on mx.dequantize of them, later tokens stay unquantised.  Tokens [0, n_tok) of a bf16 K [BH, cache_t, hd] /
 * V^T [BH, hd, cache_t] pair -> codes k4 / v4 [BH, n_tok, hd / 32, 4] (uint32, MLX's packing: code k of a word at bits [4k, 4k+4)),
 * k_sb / v_sb [BH, n_tok, hd / 32, 2] fp32 (scale, bias), and the rows REWRITTEN IN PLACE with scale * q + bias (one rounding to
 * bf16): what every later call of the reference attends on.  hd % 32 == 0.
 * qkv != null: the keys are quantised from their EXACT fp32 values, as the reference's are (RoPE promotes k to fp32, phi.py:451) --
 * recomputed from the layer's projection output qkv [B * n_tok, (n_heads + 2 n_kv) * hd] (the first call: L = n_tok) and the rotation
 * tables (positions past + t), with p3v_rope_kv_append's arithmetic; null: from the cache rows (already rounded to bf16). */
int p3v_kv_quantize_mlx4(uint16_t* k, uint16_t* vt, uint32_t* k4, uint32_t* v4, float* k_sb, float* v_sb, int BH, int hd,
                         int cache_t, int n_tok, const uint16_t* qkv, const float* cos_t, const float* sin_t, int n_heads, int n_kv,
                         int past, int tab_t, int tab_div, void* stream);

typedef struct {
  const uint16_t* qkv; const float* cos_t; const float* sin_t;
  uint8_t* k8; uint8_t* v8t; float* k_scale; float* v_scale; uint16_t* out;
  const int32_t* pad_len; const int32_t* d_past; float* ws;
  int B, L, n_heads, n_kv, hd, past, cache_t, rope_bstride, n_split;
  float scale;
  int merge_in_launch;    /* as p3v_attn_decode_args_t.merge_in_launch (honoured with one tile per split and n_split <= 16 on
                             the 64-key plan, always on the 128-key plan; otherwise the merge launch runs) */
  /* optional (round 4), as p3v_attn_decode_args_t's o_proj_* fields but for e4m3 weights: o_proj_w8 [o_n, n_heads * hd] bytes with
   * one fp32 scale per row; x += bf16(scale * (W8 . attention output)), bit-identical to p3v_gemv_fp8 with P3V_EPI_RESID_BF16.
   * For shapes p3v_attention_decode_q8_can_fuse_oproj() accepts; `out` all 0xFF on entry, `o_rearm` set to 0xFF. */
  const uint8_t* o_proj_w8; const float* o_proj_scale; uint16_t* o_proj_x; uint16_t* o_rearm; int o_n;
} p3v_attn_decode_q8_args_t;
int p3v_attention_decode_q8(const p3v_attn_decode_q8_args_t* args /* host */, void* stream);
int p3v_attention_decode_q8_can_fuse_oproj(int B, int L, int n_heads, int hd, int n_split, int cache_t, int o_n, int merge_in_launch);

/* ---- the decode attention's route: what p3v_attention_decode / p3v_attention_decode_q8 launch for a call, and what the two
 * can_fuse functions answer -- all four ask this one function (host-only, no launch).  A negative knob means the library's current
 * setting (p3v_set_tuning); a negative `capacity` / `cu_count` asks the current device, as the entry points do, and only where
 * the answer depends on it: with both given the function touches no device and runs without a GPU (tests/test_attn_route_cpu.py). */
typedef enum { P3V_ATTN_O_NONE = 0, P3V_ATTN_O_BF16 = 1, P3V_ATTN_O_F8 = 2, P3V_ATTN_O_Q4 = 3 } p3v_attn_oproj_t;
typedef enum {
  P3V_ATTN_K_DECODE = 0,        /* bf16 cache: one 64-key tile per workgroup */
  P3V_ATTN_K_DECODE128,         /*   one 128-key tile per workgroup */
  P3V_ATTN_K_DECODE128_O,       /*   ... + the bf16 o_proj + residual */
  P3V_ATTN_K_DECODE128_O4,      /*   ... + the 4-bit o_proj + residual */
  P3V_ATTN_K_DECODE_STREAM,     /*   single-wave workgroups walking several tiles */
  P3V_ATTN_K_DECODE_Q8,         /* int8 cache: single-wave workgroups (never merges in the launch) */
  P3V_ATTN_K_DECODE_Q8S,        /*   one 64-key tile per 4-wave workgroup */
  P3V_ATTN_K_DECODE128_Q8,      /*   one 128-key tile per workgroup */
  P3V_ATTN_K_DECODE128_Q8_O,    /*   ... + the e4m3 o_proj + residual */
  P3V_ATTN_K_COUNT
} p3v_attn_kernel_t;
typedef enum { P3V_ATTN_MERGE_IN_LAUNCH = 0, P3V_ATTN_MERGE_COMBINE2 = 1, P3V_ATTN_MERGE_COMBINE_O = 2 } p3v_attn_merge_t;
typedef struct {
  int kv_int8;                  /* 0: the bf16 cache (p3v_attention_decode), 1: the int8 cache (p3v_attention_decode_q8) */
  int B, L, n_heads, hd, n_split, cache_t, merge_in_launch;
  int o_proj;                   /* p3v_attn_oproj_t: the format of the o_proj the call carries */
  int o_n;
  int q8_old, attn_fo_map, attn_fo_map_q8;   /* the tuning knobs the route depends on */
  int64_t capacity;             /* workgroups of the fused attention + o_proj launch that are resident at once */
  int cu_count;                 /* compute units (the merge launch that carries the o_proj: one workgroup per CU) */
} p3v_attn_route_query_t;
typedef struct {
  int status;                   /* P3V_OK, or P3V_ERR_UNSUPPORTED: an o_proj that no launch of this call can carry */
  int kernel;                   /* p3v_attn_kernel_t */
  int grid[3], block;
  int merge;                    /* p3v_attn_merge_t */
  int merge_grid, merge_block;  /* of the merge launch (0 with P3V_ATTN_MERGE_IN_LAUNCH) */
  int fuse_form;                /* 0: no o_proj in this call, 1: in the attention launch, 2: in the merge launch (the can_fuse answer) */
  int fo_remap;                 /* fuse_form 1: the 1-D grid's placement (p3v_attention_decode_fused_role's `map`), 0 = the (split, head) grid */
  const char* kernel_name;      /* as a profiler prints them: "k_attn_decode128_q8<true>", "k_attn_combine_o<1>", "" for no merge launch */
  const char* merge_name;
} p3v_attn_route_t;
int p3v_attention_decode_route(const p3v_attn_route_query_t* query /* host */, p3v_attn_route_t* route /* host */);

/* ---- CLIP patch unfold: pixel_values [N,3,S,S] f32 -> patches [N*P, kpad] bf16, (c,ky,kx) order, zero padded */
int p3v_im2col_patches(const float* pix, uint16_t* patches, int n_img, int img, int patch, int kpad, void* stream);
/* ---- CLS rows: x[n, 0, :] = class_emb + pos[0]  (phi.py:202-205); x [N, P+1, D] f32 */
int p3v_clip_cls_rows(float* x, const uint16_t* cls, const uint16_t* pos, int n_img, int tokens, int dim, void* stream);

/* ---- HD merge, phi.py:403-407: ViT features [n_crops, P+1, C] f32 (CLS at row 0 skipped)
 * -> rows [n_out, 4C] bf16 in the reference's order: sub crops (h*12 rows of
 * w*12 tokens, each row followed by sub_GN), glb_GN, global crop (12 rows of 12 + sub_GN). */
int p3v_hd_merge(const float* feats, const uint16_t* sub_gn, const uint16_t* glb_gn, uint16_t* out,
                 int h_crops, int w_crops, int grid /* 24 */, int C, void* stream);

/* ---- argmax over the last axis of bf16 logits (first maximum wins), phi_3_vision_mlx.py:386,392 */
int p3v_argmax(const uint16_t* logits, int32_t* out, int rows, int n, int64_t row_stride, void* stream);
/* ---- nn.log_softmax = x - logsumexp(x), phi_3_vision_mlx.py:92,476,511,541: bf16 io; the fp32 log-sum-exp is rounded to bf16
 *      (it is an array of its own in the reference) and the subtraction rounds once more */
int p3v_log_softmax(const uint16_t* x, uint16_t* y, int rows, int n, void* stream);
/* ---- top-k (k<=8) by (-value, index), replaces mx.argpartition phi_3_vision_mlx.py:507 */
int p3v_topk(const uint16_t* x, int32_t* idx_out, int rows, int n, int k, int64_t row_stride, void* stream);

/* ---- 4-bit group-64 affine weights = the reference's `quantize_model=True` (nn.quantize(model, 64, 4),
 * phi_3_vision_mlx.py:264,297-305; w = scale * q + bias per 64 input columns, mx.quantized_matmul).
 * W [N or 2N, K/8] u32 in the DEVICE nibble order (weights 8d..8d+7 at bits 0,16,4,20,8,24,12,28 of dword d;
 * weights.q4_repack converts MLX's sequential order), sb [N or 2N, K/64] u32 = scale bf16 | bias bf16 << 16.
 * p3v_gemv_q4: decode projection, K = 3072 or 8192.  M = 1: same norm / epilogue options as p3v_gemv.  2 <= M <= 16 (round 6: a
 *   decode batch, a constrained-decoding step; N % 16 == 0 (SiLU: % 8)): the packed weights are dequantised in registers (fp16
 *   scale * q + bias, two weights per instruction) in front of the fp16 MFMA -- 0.5 byte per weight from HBM at every batch size, as
 *   the reference's QuantizedLinear (phi_3_vision_mlx.py:296).  norm_w: up to 8 rows the input RMSNorm may ride along (the rows are
 *   normalised to the bf16 values p3v_rmsnorm writes while the first weights are in flight); 9 .. 16 rows: must be NULL
 *   (P3V_ERR_UNSUPPORTED otherwise -- the caller runs p3v_rmsnorm first).
 *   What a weight is: M = 1 adds scale * (D - 128 X) + bias * X per 16 weights in fp32 (D = sum x (128 + q), X = sum x): scale * q + bias
 *   with its full bf16 scale and bias.  2 <= M <= 16 multiplies fp16(x) by w = fp16(scale * q + bias) -- ONE rounding to 11 bits, scale
 *   and bias converted to fp16 first -- with exact products and fp32 sums.  That path therefore holds what fp16 holds and no more:
 *   an activation with |x| > 65504 becomes Inf; activations, scales and biases below 2^-14 are fp16 subnormals (steps of 2^-24), exact
 *   while their 8 bits stay at or above 2^-24 -- down to 2^-17 -- and rounded below that (zero under 2^-25), where the M = 1 path
 *   keeps them as bf16.  Checkpoints quantised from bf16 weights sit far inside (scales around 2^-7); tests/test_qproj_kernels_gpu.py
 *   runs both paths on scales in [2^-17, 2^-14) and activations in [2^-14, 2^15].
 * p3v_dequant_q4: -> bf16 [rows, K] (prefill / batched decode run the bf16 kernels on a dequantised scratch). */
typedef struct {
  const uint16_t* x; const uint32_t* W; const uint32_t* sb; void* out;
  const uint16_t* resid; const uint16_t* norm_w; float norm_eps;
  int M, N, K;
  int epilogue;
} p3v_gemv_q4_args_t;
int p3v_gemv_q4(const p3v_gemv_q4_args_t* args /* host */, void* stream);
int p3v_dequant_q4(const uint32_t* w4, const uint32_t* sb, uint16_t* out_bf16, int rows, int K, void* stream);

/* ---- on-device image preprocessing (Phi3VImageProcessor, phi.py:283-372), bit-compatible with the host path.
 * p3v_resample_u8: one pass of Pillow's 8-bit ImagingResample (what `img.resize(..., Image.BILINEAR)` phi.py:301 runs):
 *   in [outer, in_len, inner] u8 -> out [outer, out_len, inner]; coeffs [out_len, ksize] 22-bit fixed point and
 *   bounds [out_len, 2] = (first input index, tap count) are computed on the host (processor.pil_bilinear_coeffs).
 *   Horizontal pass: outer = rows, inner = 3; vertical pass: outer = 1, inner = 3 * width.
 * p3v_hd_preprocess: resized image [rh, rw, 3] u8 -> pixel_values [n_slots, 3, 336, 336] f32: white padding of `top` rows
 *   above / (hp - rh - top) below (phi.py:302-306), transpose back if `portrait` (:307-308), normalisation through
 *   lut [3][256] f64 = (v / 255 - mean) / std (:309), crop grid into slots 1.. (:313-314), degenerate-bicubic global view
 *   into slot 0 with taps hw/ww [336][2] f32, hi/wi [336][2] i32 (:331-372), remaining slots zero (:315-316). */
int p3v_resample_u8(const uint8_t* in, uint8_t* out, int outer, int in_len, int out_len, int inner,
                    const int32_t* coeffs, const int32_t* bounds, int ksize, void* stream);
int p3v_hd_preprocess(const uint8_t* resized, int rh, int rw, int top, int hp, int portrait, const double* lut,
                      const float* hw, const int32_t* hi, const float* ww, const int32_t* wi, float* pixel_values,
                      int n_slots, void* stream);

/* ---- LoRA adapter inference, LoRALinear.__call__ (phi.py:129-133):
 *   y = linear(x); z = (x @ lora_a) @ lora_b; out = (y + scale*z).astype(bf16),  scale = cfg.scale * alpha / rank (phi.py:120)
 * lora_a [K, r] and lora_b [r, N] are the fp32 tensors of adapters.safetensors, r <= 64.
 * p3v_lora_down: t[M, r] (f32) = x[M, K] (bf16) @ lora_a.
 * p3v_lora_up:   v = bf16(y + scale * (t @ lora_b)) with y[M, N] the frozen projection's plain bf16 output, then the
 *   epilogue that projection would have carried: P3V_EPI_NONE out[M,N] = v; P3V_EPI_RESID_BF16 out = resid + v;
 *   P3V_EPI_SILU_MUL (N = 2*I, gate rows first) out[M, I] = silu(v[:, :I]) * v[:, I:]. */
int p3v_lora_down(const uint16_t* x, const float* lora_a, float* t, int M, int K, int r, void* stream);
int p3v_lora_up(const uint16_t* y, const float* t, const float* lora_b, float scale, int epilogue,
                const uint16_t* resid, uint16_t* out, int M, int N, int r, void* stream);

/* ---- adapter bank: the per-row ("gathered") forms of the pair above.  Added after round 6, no version change.
 * N adapters stay resident beside one set of frozen weights; every row of a call names the one it wants.
 * A BANK TABLE per adapted projection (device memory): one p3v_lora_entry_t per bank slot -- lora_a [K, rank] and
 * lora_b [rank, N] fp32, rank 1..64 (0, or a null pointer: this adapter leaves this projection alone), scale.
 * A ROW TABLE row_adapter[M] (device memory, int32): the bank slot of each row; -1 (or any value outside 0..n_slots-1) = no
 * adapter.  Both tables are READ BY THE KERNELS and are not launch arguments: a captured step keeps working when rows change
 * adapter, or when entries change, between replays.
 * The rule, for row m with entry e = table[row_adapter[m]] and rank r = min(e.rank, r_max):
 *   h      = x[m], or with norm_w: RMSNorm(x[m]) * norm_w with exactly the arithmetic and rounding of p3v_rmsnorm
 *            (computed inside the launch: the frozen projection keeps its own fused norm, no materialised copy is needed);
 *   K is cut into S = p3v_lora_rows_slices(K) = ceil(K / P3V_LORA_SLICE_K) slices, one workgroup per (row, slice):
 *   t[m, s, j] = sum over the slice's k of h[k] * e.lora_a[k, j]          fp32, j < r   (p3v_lora_down_rows; t is [M, S, r_max])
 *   T[j]       = t[m, 0, j] + t[m, 1, j] + .. + t[m, S-1, j]              fp32, in slice order   (prologue of p3v_lora_up_rows)
 *   v[n]       = bf16(y[m, n] + e.scale * sum_{j < r} T[j] * e.lora_b[j, n])   j ascending
 *   out[m]     = epilogue(v) as p3v_lora_up (none / residual / SiLU * up, same per-op rounding).
 * A row without an adapter (slot -1, rank 0) does no work in the down launch and gets epilogue(y[m]) with v = y[m] bit for
 * bit.  The slice boundaries and every summation order depend on K and r alone: a row's output bits depend only on its own
 * input, its own entry and (K, N, epilogue) -- not on M, on the row's position, on other rows' slots, or on eager versus
 * graph execution.  Any M >= 0 (decode rows and prompt-sized token rows), mixed ranks within one call.
 * P3V_ERR_ARG: a null pointer, r_max outside 1..64, n_slots < 1, norm_w with K % 8 != 0.
 * Call sites: model.py `_proj` with an adapter bank attached (set_adapter_bank / set_row_adapters). */
#define P3V_LORA_SLICE_K 256
typedef struct {
  const float* lora_a;
  const float* lora_b;
  int32_t rank;
  float scale;
} p3v_lora_entry_t;
int p3v_lora_rows_slices(int K);
int p3v_lora_down_rows(const uint16_t* x, const uint16_t* norm_w /* or NULL */, float eps, const p3v_lora_entry_t* table,
                       const int32_t* row_adapter, float* t, int M, int K, int r_max, int n_slots, void* stream);
int p3v_lora_up_rows(const uint16_t* y, const float* t, const p3v_lora_entry_t* table, const int32_t* row_adapter,
                     int epilogue, const uint16_t* resid, uint16_t* out, int M, int N, int K, int r_max, int n_slots,
                     void* stream);

/* ---- decode-step helpers (device-resident loop state for graph replay) */
int p3v_add_i32(int32_t* x, int n, int delta, void* stream);
/* history[b, *d_step] = tok[b]; if tok_next != NULL also tok_next[b] = tok[b] (feeds the next replayed step) */
int p3v_store_token(const int32_t* tok, int32_t* history, const int32_t* d_step, int32_t* tok_next,
                    int B, int max_steps, void* stream);
/* fused head of a replayed greedy step: x_out[b] = table[tok[b]] (p3v_embed_gather, phi.py:597) and the rotation
 * rows of position *d_past -> cos_out/sin_out [B, 1, half] (p3v_stage_rope with L = 1) */
int p3v_step_begin(const int32_t* tok, const uint16_t* table, uint16_t* x_out, const float* cos_t, const float* sin_t,
                   const int32_t* d_past, float* cos_out, float* sin_out, int B, int hidden, int vocab, int tab_t,
                   int half_dim, int32_t* zero_buf /* optional: n_zero int32 cleared (in-launch flags of the step) */,
                   int n_zero, void* stream);
/* fused tail: next_tok[b] = tok[b] = argmax(logits[b]) (phi_3_vision_mlx.py:392), history[b, *d_step] = it,
 * then *d_step += 1 and *d_past += 1 (done once, by the last workgroup; `ticket` is a zero-initialised int32) */
int p3v_step_end(const uint16_t* logits, int32_t* next_tok, int32_t* tok, int32_t* history, int32_t* d_step,
                 int32_t* d_past, int32_t* ticket, int B, int n, int max_steps, void* stream);

/* Round 6: the same two stages WITHOUT launches of their own -- folded into the step's first projection (layer 0's RMSNorm + qkv)
 * and its last (final norm + lm_head, phi.py:597-608, phi_3_vision_mlx.py:386-393): p3v_gemv with
 *   begin (tok != NULL):      x row b = embed_table[clamp(tok[b])] instead of args->x; the rows are also written to x_out (the residual
 *                             stream) and the rotation rows of position *d_past staged into cos_out / sin_out, as p3v_step_begin does;
 *   end (next_tok != NULL):   next_tok[b] = tok_out[b] = argmax(out[b]) (first maximum of the bf16 values; a NaN row reports -1),
 *                             history[b, *d_step] = it, then *d_step += 1, *d_past += 1 -- by the last workgroup to finish (every
 *                             workgroup publishes its candidates into amax_ws and counts itself in: one arrival counter per XCD, then
 *                             one for the eight group-last workgroups -- a thousand workgroups finishing together on ONE counter
 *                             serialise for ~10 us; amax_ws: P3V_GEMV_STEP_WS_BYTES bytes, 8-byte aligned: P3V_GEMV_STEP_MAX_WG
 *                             candidate records (contents irrelevant) + nine counters, 128 bytes apart, that must be ZERO before
 *                             the first launch and are left zero by every launch; `ticket` is not touched).
 * Exactly one of the two.  Where p3v_gemv_route (step set) names the one-row streaming kernel; otherwise
 * P3V_ERR_UNSUPPORTED and the caller
 * keeps p3v_step_begin / p3v_step_end.  Bit-identical to the separate launches. */
#define P3V_GEMV_STEP_MAX_WG 1024
#define P3V_GEMV_STEP_WS_BYTES (P3V_GEMV_STEP_MAX_WG * 8 + 9 * 128)
typedef struct {
  const int32_t* tok; const uint16_t* embed_table; int vocab; uint16_t* x_out;
  const float* cos_t; const float* sin_t; float* cos_out; float* sin_out; int tab_t, half_dim;
  int32_t* next_tok; int32_t* tok_out; int32_t* history; int32_t* d_step; int32_t* ticket; float* amax_ws; int max_steps;
  int32_t* d_past;            /* begin: read (position of the rows to stage); end: incremented */
} p3v_gemv_step_t;
int p3v_gemv_step(const p3v_gemv_args_t* args /* host */, const p3v_gemv_step_t* step /* host */, void* stream);
/* the same on e4m3 weights (config 5: `args` as for p3v_gemv_fp8, one row, no epilogue) */
int p3v_gemv_fp8_step(const p3v_gemv_fp8_args_t* args /* host */, const p3v_gemv_step_t* step /* host */, void* stream);
/* the same on 13-bit packed bf16 weights (`args` as for p3v_gemv_b13, silu_pairs = 0) */
int p3v_gemv_b13_step(const p3v_gemv_b13_args_t* args /* host */, const p3v_gemv_step_t* step /* host */, void* stream);
/* and on MLX 4-bit group-64 weights (`args` as for p3v_gemv_q4, one row, no epilogue) */
int p3v_gemv_q4_step(const p3v_gemv_q4_args_t* args /* host */, const p3v_gemv_step_t* step /* host */, void* stream);

/* ---- the decode projections' route: what p3v_gemv / p3v_gemv_fp8 / p3v_gemv_q4 / p3v_gemv_b13 and their _step entries launch for
 * a call, or the code they refuse it with.  Every rule is stated in this one function (DESIGN.md section 3.1 has the table); the eight
 * entry points check the pointers they were given, ask it and launch what it says; p3v_gemv_b13_plan is a projection of it.  The
 * `gemv*` knobs are read from the library's current settings (p3v_set_tuning works without a device).  cu_count <= 0 asks the current
 * device, as the entry points do, and only where the streaming kernel's plan is part of the answer: with cu_count given the function
 * touches no device (tests/test_gemv_route_cpu.py).  Added after round 6, no version change. */
typedef enum { P3V_GEMV_FMT_BF16 = 0, P3V_GEMV_FMT_FP8, P3V_GEMV_FMT_Q4, P3V_GEMV_FMT_B13, P3V_GEMV_FMT_COUNT } p3v_gemv_format_t;
typedef enum { P3V_GEMV_STEP_NONE = 0, P3V_GEMV_STEP_BEGIN = 1, P3V_GEMV_STEP_END = 2 } p3v_gemv_step_end_t;
typedef enum {
  P3V_GEMV_K_NONE = 0,
  P3V_GEMV_K_GEMV,              /* k_gemv<MT>: any K % 8, x staged in LDS */
  P3V_GEMV_K_GEMV3,             /* k_gemv3<F, MT, NST, CH> / k_gemv3_step<F, 1, NST, CH, step>: the streaming kernel, K = NST stages x CH lane loads */
  P3V_GEMV_K_MFMA,              /* k_gemv_mfma<SILU>: 16 rows of W per workgroup, K % 1024 */
  P3V_GEMV_K_MFMA8,             /* k_gemv_mfma8<SILU, NW, NST>: up to 8 rows of x, persistent over row sets, K = NW x NST x 256 */
  P3V_GEMV_K_MFMA_F8,           /* k_gemv_mfma_f8<SILU> */
  P3V_GEMV_K_MFMA8_F8,          /* k_gemv_mfma8_f8<SILU, NW, NL>: NL (in `NST`) 128-element lines per wave slice */
  P3V_GEMV_K_GEMV8_Q4,          /* k_gemv8_q4<SILU, NW, NST>: up to 8 rows, persistent */
  P3V_GEMV_K_ROWS_Q4,           /* k_gemm_rows_q4<SILU, NW, NST>: 9 .. 16 rows, persistent */
  P3V_GEMV_K_COUNT
} p3v_gemv_kernel_t;
typedef struct {
  int format;                   /* p3v_gemv_format_t */
  int step;                     /* p3v_gemv_step_end_t: NONE = the plain entry */
  int M, N, K, epilogue;
  int has_norm, has_resid;      /* whether the call carries norm_w / resid (a residual epilogue without one is P3V_ERR_ARG) */
  int exp_base;                 /* P3V_GEMV_FMT_B13 */
  int cu_count;
} p3v_gemv_route_query_t;
typedef struct {
  int status;                   /* P3V_OK, or the code the entry returns for this shape (then kernel is P3V_GEMV_K_NONE); P3V_ERR_HIP: no device answered for cu_count */
  int late;                     /* a refusal only: 1 = the entry reports it after the checks of its pointers' alignment (which then win), 0 = before */
  int kernel;                   /* p3v_gemv_kernel_t */
  int MT, NW, NST, CH, silu, scaled;   /* the instantiation: whichever the kernel has (scaled: GemvB13<true>), 0 otherwise */
  int grid, block, lds_bytes;
  int lds_cap;                  /* what the kernel's dynamic-LDS limit is raised to before such a launch, once per process (0: left alone) */
  int upw, waves, wpw;          /* the streaming kernel's plan: row pairs per wave, waves that take rows, row-streaming waves per workgroup */
  int n_sets, sets_per_wg;      /* the persistent kernels: row sets of the launch, and how many one workgroup walks */
  char name[64];                /* as a profiler prints it: "k_gemv3<GemvB13<true>, 1, 1, 6>" (filled by p3v_gemv_route only) */
} p3v_gemv_route_t;
int p3v_gemv_route(const p3v_gemv_route_query_t* query /* host */, p3v_gemv_route_t* route /* host */);

/* ---- seeded sampling (temperature, top-k, top-p): added after round 6, no version change.
 * One record per row, on the device; every launch reads it and increments `counter`, so a replayed graph needs no host input.
 * The rule, for one row of bf16 logits l[0..n) with temperature T, top_k k (0 = off), top_p p (1 = off), 64-bit seed
 * s = seed_hi:seed_lo and draw index c = counter (the index of this token in the row's generated sequence, 0 = the token
 * drawn from the prefill logits):
 *   0. T <= 0: the arg-max, exactly as p3v_argmax (first maximum, -1 for a NaN row).  Also when the row has no finite
 *      logit or when m (step 2) overflows to +inf.
 *   1. a NaN logit: the token is -1.
 *   2. z_i = f32(l_i) / T (IEEE fp32 division, correctly rounded); m = max z.
 *   3. w_i = floor(exp((double)z_i - (double)m) * 2^32) as uint64, computed in fp64 (a -inf logit: 0).
 *   4. top-k, when 1 <= k < n: keep i iff l_i >= the k-th largest bf16 value (every token tied at the cut is kept).
 *   5. top-p, when 0 < p < 1, over the kept tokens: Q = sum w, P = ceil((double)p * (double)Q); keep l_i >= kappa, kappa the
 *      largest bf16 value with sum_{kept, l_i >= kappa} w_i >= P (ties at kappa kept).
 *   6. r = word 0 of Philox4x32-10 with counter (c, 0, 0, 0) and key (seed_lo, seed_hi); Q' = sum_kept w;
 *      t = floor(Q' * r / 2^32) (exact 128-bit product); the token is the smallest i with sum_{kept, j <= i} w_j > t.
 *   7. counter += 1 for every row, greedy rows included.
 * Everything after step 3 is integer arithmetic: a token does not depend on the launch geometry, the batch neighbours or graph
 * versus eager execution.  n <= 32768 and rows <= 1024, otherwise P3V_ERR_UNSUPPORTED. */
typedef struct {
  float temperature;
  int32_t top_k;
  float top_p;
  uint32_t seed_lo, seed_hi;
  int32_t counter;
} p3v_sample_row_t;
/* eager form: out[r] = the token of row r (logits row r at logits + r * row_stride); rows_params[r].counter += 1 */
int p3v_sample(const uint16_t* logits, int64_t row_stride, p3v_sample_row_t* rows_params, int32_t* out, int rows, int n,
               void* stream);
/* graph tail of a sampled step: p3v_step_end's bookkeeping with the sampled token (next_tok[b] = tok[b] = it,
 * history[b, *d_step] = it, then *d_step += 1 and *d_past += 1 done once via `ticket`, which is left at zero) */
int p3v_sample_step_end(const uint16_t* logits, p3v_sample_row_t* rows_params, int32_t* next_tok, int32_t* tok,
                        int32_t* history, int32_t* d_step, int32_t* d_past, int32_t* ticket, int B, int n, int max_steps,
                        void* stream);

/* ---- token log-probabilities: added after round 6, no version change.  Read-only on the logits: no token, no loop state and
 * no number of any other entry point changes.
 * The rule, for one row of bf16 logits l[0..n), a token id t and a count N, 0 <= N <= P3V_LOGPROBS_MAX (the limit p3v_topk has;
 * a larger N counts as P3V_LOGPROBS_MAX):
 *   1. the row is UNDEFINED if it holds a NaN or a +inf, or has no finite logit: logprob = NaN, rank = 0, n_top = 0.
 *   2. m = max f32(l_i).
 *   3. w_i = floor(exp((double)l_i - (double)m) * 2^32) as uint64: step 3 of the sampling rule at T = 1 (a -inf logit: 0).
 *   4. W = sum w_i, an exact integer, 2^32 <= W < 2^48.
 *   5. lse = (double)m + log((double)W) - 32 ln 2, in fp64.
 *   6. logprob(i) = (float)((double)f32(l_i) - lse); a -inf logit: -inf.
 *   7. rank(t) = 1 + #{j : l_j > l_t} + #{j < t : l_j == l_t}, on the float values (-0 == +0): the token of p3v_argmax has rank 1.
 *   8. top: the n_top = min(N, n) tokens with the largest value, ties to the lower index (p3v_topk's order), each with its
 *      logprob.  Unused entries: id -1, logprob NaN.
 *   9. t outside [0, n) (an image-slot id, the -1 of a failed step): logprob = NaN, rank = 0; the top list is still filled.
 * These are the log-probabilities of the RAW logits: no temperature, no top-k, no top-p.  W is a sum of integers, so every bit
 * of a record is independent of the reduction order, the launch geometry, the batch neighbours and graph versus eager execution.
 * (p3v_log_softmax is the reference's bf16 composite, rounded twice: not a usable probability.) */
#define P3V_LOGPROBS_MAX 8
typedef struct {
  int32_t token;
  float   logprob;
  int32_t rank;
  int32_t n_top;
  int32_t top_id[P3V_LOGPROBS_MAX];
  float   top_logprob[P3V_LOGPROBS_MAX];
} p3v_logprob_t;   /* 80 bytes */
/* eager form: out[r] = the record of token[r] on logits row r (at logits + r * row_stride) with N = want[r]; want[r] < 0: the
 * row is skipped and out[r] is not written.  Any rows >= 1, 1 <= n <= 65536, row_stride >= n; P3V_ERR_ARG otherwise or for a
 * null pointer (`want` included). */
int p3v_logprobs(const uint16_t* logits, int64_t row_stride, const int32_t* token, const int32_t* want,
                 p3v_logprob_t* out, int rows, int n, void* stream);
/* graph form, the launch AFTER a step's tail (p3v_gemv_step's end, p3v_step_end or p3v_sample_step_end): next_tok[b] is the
 * token the step emitted and *d_step already counts it.  Row b's record (logits [B, n] contiguous) goes to
 * records[b * max_steps + (*d_step - 1)] when that index lies in [0, max_steps) and want[b] >= 0; nothing is written
 * otherwise.  `records` may be pinned host memory, as `history` is: it is written with plain 4-byte vector stores. */
int p3v_logprobs_step(const uint16_t* logits, const int32_t* next_tok, const int32_t* want, const int32_t* d_step,
                      p3v_logprob_t* records, int B, int n, int max_steps, void* stream);

/* ---- repetition / presence / frequency penalties and logit_bias: added after round 6, no version change.
 * Per-row state on the device, so a captured step adjusts its logits with no host input: a record, a table seen[0..n) of uint32
 * (bit 31: the token occurs in the row's prompt; bits 0..30: how often the row has emitted it, below 2^31) and an optional table
 * bias[0..n) of fp32.  The rule, for one row of bf16 logits l[0..n) -> the adjusted row l'[0..n), a second buffer:
 *   0. flags & 1 == 0 (an inactive row): l' is a byte copy of l (NaN payloads and -0 kept); seen is neither read nor written.
 *   1. a = f32(l_i), c = seen_i & 0x7fffffff, s = (seen_i != 0).
 *   2. repetition (the HF / vLLM convention, prompt and output): if s and repetition != 1: a = (a > 0) ? a / repetition
 *      : a * repetition (IEEE fp32, correctly rounded).
 *   3. frequency (output only): a = a - fl32(frequency * (float)c): two separately rounded fp32 operations, no FMA.
 *   4. presence (output only): if c > 0: a = a - presence.
 *   5. bias: if flags & 2 (and a bias table was passed): a = a + bias_i.  A -inf bias bans the token.
 *   6. l'_i = bf16_rne(a).  A NaN stays a NaN (its payload is not specified): the sampler then reports -1, as it does today.
 * Every operation is ONE correctly rounded fp32 operation in a fixed order: fp32 arithmetic on the host reproduces every bit
 * (penalties.reference_adjust).  The raw logits are not touched: p3v_logprobs* keep describing the RAW distribution, the sampler
 * (p3v_sample / p3v_sample_step_end) reads l', so temperature, top-k and top-p apply after the penalties and a T = 0 row takes
 * the arg-max of l' by p3v_argmax's rule. */
#define P3V_PENALTY_ACTIVE 1
#define P3V_PENALTY_BIAS 2
typedef struct { float repetition, frequency, presence; int32_t flags; } p3v_penalty_row_t;   /* 16 bytes */
/* seen[r, id] |= 1 << 31 (as_prompt != 0) or += 1 (otherwise) for id = ids[r, first[r] .. first[r] + count[r]) (row r of `ids` at
 * ids + r * ids_stride, of `seen` at seen + r * seen_stride; the run is cut to the row: first[r] < 0 skips it, the count ends at
 * ids_stride); ids outside [0, n) are skipped (image slots, the -1 of a failed step).  clear != 0 zeroes the `rows` rows first,
 * ordered before the scatter.  Duplicates and equal ids in one row are fine (32-bit vector atomics).  rows >= 1, n >= 1,
 * ids_stride >= 0, seen_stride >= n; P3V_ERR_ARG otherwise or for a null pointer. */
int p3v_penalty_note(uint32_t* seen, int64_t seen_stride, const int32_t* ids, int64_t ids_stride, const int32_t* first,
                     const int32_t* count, int rows, int n, int as_prompt, int clear, void* stream);
/* out[r] = the rule on logits row r.  fed != NULL: BEFORE reading, seen[r, fed[r]] += 1 when fed[r] lies in [0, n) and the row is
 * active (the token this step was fed = the token the row emitted last; a count stays at 2^31 - 1 once there), done by the one
 * thread that owns that index: no atomics, no second launch.  bias may be NULL (step 5 is then skipped for every row).  Every
 * pointer is device memory, so the call is capturable.  Rows whose four bases are 16-byte aligned move 16 bytes per access,
 * others (and the tail n % 8) go element by element.  1 <= rows <= 65535, n >= 1, every stride >= n, out != logits;
 * P3V_ERR_ARG otherwise or for a null logits / rows_params / seen / out. */
int p3v_penalize(const uint16_t* logits, int64_t row_stride, const p3v_penalty_row_t* rows_params, uint32_t* seen,
                 int64_t seen_stride, const float* bias /* may be NULL */, int64_t bias_stride, const int32_t* fed /* may be NULL */,
                 uint16_t* out, int64_t out_stride, int rows, int n, void* stream);

/* ---- guided decoding: a regular expression (or a choice list) walked on the device; added after round 6, no version change.
 * A GUIDE is a DFA over bytes: states 1..S, S <= P3V_GUIDE_MAX_STATES; state 0 is dead, state 1 the start; delta[s][b] a uint16
 * table, accept[s] a uint8 table.  The host guarantees that every state 1..S can reach an accepting state and has checked, against
 * the vocabulary table, that every state either accepts or allows at least one token (guide.check).
 * A VOCABULARY TABLE, one per processor, device-resident, built once: tok_off uint32 [n + 1] and tok_bytes uint8 [n_bytes], the
 * byte string of token i at tok_bytes[tok_off[i] .. tok_off[i + 1]); specials, image-slot ids and unused ids are empty.
 * PER-ROW STATE: a 16-byte record {flags, n_states, state, reserved} (state == P3V_GUIDE_DONE after EOS) and the row's own table
 * region, delta [rows, 256, 256] uint16 and accept [rows, 256] uint8, both dense: row r's tables at delta + r * 65536 and
 * accept + r * 256.  Admitting a request copies at most 128 KB into its row's region; there is no bank.
 * walk(s, bytes): s = delta[s][b] for each byte b in order, stopping at 0; an entry above n_states counts as 0.
 * The rule, for one row of bf16 logits, IN PLACE (in a step: the penalty state's adjusted rows, never the raw logits):
 *   0. flags & 1 == 0 (an inactive row): the row is not touched (NaN payloads kept); the record is neither read further nor written.
 *   1. fed != NULL and the row is active and not DONE: if fed[r] == eos the state becomes DONE; else if fed[r] lies in [0, n) and
 *      has bytes, state = walk(state, bytes(fed[r])); otherwise the state is unchanged.  BEFORE masking, as p3v_penalize counts
 *      the token the step was fed.  A fed token the guide bans leaves state 0, which step 4 reads as DONE.
 *   2. token i is allowed iff -- i == eos: the state is DONE, or accept[state] != 0; any other i: the state is not DONE, the token
 *      has bytes and walk(state, bytes(i)) != 0.
 *   3. a banned position is overwritten with bf16 -inf (0xFF80) whatever it held; an allowed position is not stored to.
 *   4. a record that points outside its tables -- n_states outside 1..255, or a state outside {-1, 1..n_states} -- is treated as
 *      DONE (only EOS allowed) and is not written.  Whatever a record holds, nothing outside the row's region and the
 *      vocabulary table is read; a token whose offsets do not lie in [0, n_bytes] in order counts as one without bytes.
 * No atomics, plain vector stores, no allocation; every pointer is device memory, so the call is capturable.  One workgroup per
 * row: the state is stored by one thread behind the barrier that follows every thread's read of it.  guide.reference_mask
 * (NumPy) gives every output bit and every state.
 *
 * THE WIDE FORM (a guide of more than 255 states: a JSON schema's, guide.compile_json).  A row is WIDE when flags &
 * P3V_GUIDE_WIDE; the record's `reserved` then carries the class count C, 1 <= C <= 256 (a narrow row's `reserved` is not read).
 * The row keeps the same region, read differently:
 *   cls    uint8  [256]          in the accept region: the class of every byte, 0 .. C-1;
 *   table  uint16 [S + 1][pitch] from the start of the delta region: row s is state s (row 0, the dead state, is never walked
 *                                from); column 0 is the state's accept flag, column 1 + c its successor on a byte of class c;
 *   pitch  = (C + 1) | 1 (the columns padded to an odd count) where (S + 1) * ((C + 1) | 1) <= P3V_GUIDE_WIDE_MAX_ENTRIES, else
 *            C + 1: a function of S and C alone, so the record needs no further field.
 * The bound is (S + 1) * (C + 1) <= P3V_GUIDE_WIDE_MAX_ENTRIES, the region the row already has.
 *   walk(s, bytes): s = table[s][1 + cls[b]] for each byte b in order, stopping at 0; a byte whose cls[b] >= C leads to 0, and an
 *   entry above S counts as 0 -- in column 0 as well: the state accepts iff its column-0 entry lies in 1..S.
 * The rule is points 0 to 4 above with this walk and this accept flag; point 4 reads: a wide record with S < 1, C outside
 * 1..256, (S + 1) * (C + 1) over the bound, or a state outside {-1, 1..S} is treated as DONE and is not written.  Whatever a
 * record holds, nothing outside the row's region and the vocabulary table is read.  Rows of both forms, inactive rows and DONE
 * rows share one launch; a row changes form by a new record and region, without a new capture. */
#define P3V_GUIDE_MAX_STATES 255
#define P3V_GUIDE_ACTIVE 1
#define P3V_GUIDE_WIDE 256                   /* bit 8 of flags (bits 1..7 are not read) */
#define P3V_GUIDE_WIDE_MAX_ENTRIES 65536     /* uint16 entries of one row's delta region */
#define P3V_GUIDE_DONE (-1)
typedef struct { int32_t flags, n_states, state, reserved; } p3v_guide_row_t;   /* 16 bytes */
/* eos: the EOS id (a launch argument; outside [0, n) there is no EOS position).  fed may be NULL (the first token, drawn from the
 * prefill logits: nothing is walked).  1 <= rows <= 65535, n >= 1, row_stride >= n, 0 <= n_bytes < 2^32, delta 16-byte aligned;
 * P3V_ERR_ARG otherwise or for a null pointer other than fed, nothing launched. */
int p3v_guide_mask(uint16_t* logits, int64_t row_stride, p3v_guide_row_t* rows_state, const uint16_t* delta, const uint8_t* accept,
                   const uint32_t* tok_off, const uint8_t* tok_bytes, int64_t n_bytes, const int32_t* fed /* may be NULL */,
                   int eos, int rows, int n, void* stream);

/* ---- prompt prefix cache: KV block copy at any column phase (added after round 6, no version change).
 * One job copies tokens [t0_src, t0_src + n_tok) of batch row b_src of a source cache to tokens [t0_dst, t0_dst + n_tok) of
 * batch row b_dst of a destination cache, for ALL nl layers and nkv heads; up to P3V_KV_COPY_MAX_JOBS jobs share ONE launch
 * (the job records are copied into the launch arguments: `jobs` is host memory, free to reuse on return).
 *   k_*   K    [nl, B, nkv, T, hd]   elem_size bytes per element (2: bf16 cache, 1: int8 cache codes); 16-byte aligned bases,
 *                                     hd * elem_size a multiple of 16
 *   v_*   V^T  [nl, B, nkv, hd, T]   hd runs of n_tok elements per (layer, head) at element offsets t0_src / t0_dst in rows of
 *                                     stride T_src / T_dst: ANY pair of offsets and strides (the destination run may start at any
 *                                     element phase relative to the source)
 *   ks_*, vs_*  fp32 scale rows [nl, B, nkv, T] of the int8 cache: all four, or all four NULL
 * B and T are per side: a compact store entry (B = 1, T = tokens rounded up to 8) on one, a slot state on the other.
 * The destination is written in [t0_dst, t0_dst + n_tok) ONLY: no byte next to a run changes.  The source may be read up to
 * 3 bytes outside a run, inside the aligned 32-bit word that holds the run's first / last byte.
 * P3V_ERR_ARG, nothing launched: null / misaligned pointers, n_jobs outside 1..P3V_KV_COPY_MAX_JOBS, elem_size other than 1 / 2,
 * a row index outside its B, a run that leaves its row ([t0, t0 + n_tok) outside [0, T)), a source that overlaps a
 * destination of the launch (its own or another job's; two different views that share memory are refused outright), two
 * destinations that overlap.  n_tok = 0 is an empty job. */
#define P3V_KV_COPY_MAX_JOBS 4
typedef struct {
  const void* k_src; const void* v_src; void* k_dst; void* v_dst;
  const float* ks_src; const float* vs_src; float* ks_dst; float* vs_dst;
  int32_t B_src, b_src, T_src, t0_src, B_dst, b_dst, T_dst, t0_dst, n_tok;
} p3v_kv_copy_job_t;
int p3v_kv_copy(const p3v_kv_copy_job_t* jobs /* host */, int n_jobs, int nl, int nkv, int hd, int elem_size, void* stream);

/* ---- n completions per prompt: KV fork, one source row to many rows (added after round 6, no version change).
 * The rule of a family of n completions of ONE prompt (api.generate(n=, best_of=), engine.n_args, the server's "n"):
 *   Prefill: the prompt is prefilled ONCE, into one batch row.  K is stored rotated by logical position and every row of a
 *   slot state keeps its own position table and pad_len, so the prompt's K/V rows are valid in any row at the same columns:
 *   the other n - 1 rows become continuations of the first by copying its K/V columns [pad, offset), its cos / sin table
 *   rows and its pad_len.
 *   Seeds: a scalar seed s gives completion j the seed (s + j) mod 2^64 (sampling.rows's batch rule); a list of n seeds is
 *   used as given; no seed draws 64 random bits once.  Every completion's draw 0 reads the ONE prefill logits row, draw i
 *   its own row of step i: each completion is the B = 1 request with its seed, on the batched step's logits.
 *   best_of = m (n <= m <= 16): m completions are generated and the n with the largest sum of RAW-logit token
 *   log-probabilities through the first EOS are returned, best first; ties go to the lower index (logprobs.rank_best_of).
 * p3v_kv_fork copies tokens [t0_src, t0_src + n_tok) of batch row b_src of the source cache to tokens
 * [t0_dst, t0_dst + n_tok) of EVERY row b_dst[0 .. n_dst) of the destination cache, all nl layers and nkv heads in ONE launch:
 * K, V^T and (all four or none) the fp32 scale rows of the int8 cache, in p3v_kv_copy's layouts.  Every 16-byte piece of
 * the source is loaded once and stored n_dst times (plain vector stores).  The destination may be another allocation (a B = 1
 * state forked into a B = n one) or the SAME tensors with B_src == B_dst and T_src == T_dst (rows of one slot state).
 * Both uses keep the run in the same columns, so only EQUAL 16-byte phase is implemented:
 * (v_src + t0_src * es) % 16 == (v_dst + t0_dst * es) % 16 with T_src * es and T_dst * es multiples of 16; anything else is
 * P3V_ERR_UNSUPPORTED with nothing launched (p3v_kv_copy takes any phase pair).  The destination is written inside its runs
 * ONLY and the source is read inside its runs only.
 * P3V_ERR_ARG, nothing launched: null / misaligned pointers (K bases 16 bytes, V^T bases elem_size, scales 4), n_dst
 * outside 1..P3V_KV_FORK_MAX_DST, elem_size other than 1 / 2, hd * elem_size not a multiple of 16, a row index outside its
 * B, a run that leaves its row, two equal destination rows, the same tensors with a destination row equal to b_src, two
 * different views that share memory (refused outright, as p3v_kv_copy does).  These are checked first; then n_tok = 0 is an
 * empty job: P3V_OK at any phase; then the phase. */
#define P3V_KV_FORK_MAX_DST 15
typedef struct {
  const void* k_src; const void* v_src; void* k_dst; void* v_dst;
  const float* ks_src; const float* vs_src; float* ks_dst; float* vs_dst;   /* all four or none (int8 cache) */
  int32_t B_src, b_src, T_src, t0_src, B_dst, T_dst, t0_dst, n_tok, n_dst;
  int32_t b_dst[P3V_KV_FORK_MAX_DST];
} p3v_kv_fork_t;
int p3v_kv_fork(const p3v_kv_fork_t* job /* host */, int nl, int nkv, int hd, int elem_size, void* stream);

/* ---- speculative greedy decoding (B = 1): prompt-lookup drafts, one verify step per replay (added after round 6, no
 * version change).  The rule (speculate.py states it once more in plain Python; the kernels are held to it exactly):
 *   State of one sequence: ctx[0..n) -- every token id so far, prompt included; the newest token ctx[n-1] is not yet in
 *   the cache; *d_past = n - 1.
 *   Propose (K, n_max, n_min; defaults P3V_SPEC_DEFAULT_K = 4, P3V_SPEC_NGRAM_MAX = 3, P3V_SPEC_NGRAM_MIN = 1): for
 *   m = n_max down to n_min, skipping m >= n: s = ctx[n-m .. n).  Take the LARGEST p < n - m with ctx[p .. p+m) == s.  If
 *   one exists the draft is ctx[p+m .. min(p+m+K, n)), cut in front of the first id outside [0, vocab) (image-slot ids
 *   are never proposed), and the search ends.  No match at any m: the draft is empty.
 *   Verify: rows 0..K of the step are ctx[n-1], d_0 .. d_{k-1} and, where k < K, padding (a valid id; those rows are
 *   causal dead weight and their K/V rows lie beyond the new offset).  a_j = arg-max of row j by p3v_argmax's rule (first
 *   maximum of the bf16 values, -1 for a NaN row).  acc = the largest i <= k with d_j == a_j for all j < i.  Emitted:
 *   a_0 .. a_acc.  If a_acc is -1 the step FAILED: a_0 .. a_acc go to the history (the host raises on the negative
 *   token), *d_step counts them, tok[0] = -1, and ctx, n and *d_past stay as they were.  Otherwise the emitted run is cut
 *   to the budget (c = min(acc + 1, n_limit - n, ctx_cap - n) tokens, possibly none), ctx grows by it, *d_past += c,
 *   *d_step += c, the next step's row 0 is the last emitted token and the next draft is proposed from the new ctx.
 * One state record describes the loop state; every pointer is device memory unless stated:
 *   tok      [L]   rows of the NEXT step: tok[0] = ctx[n-1], tok[1 .. 1+n_draft) the draft, then padding
 *   ctx      [ctx_cap]
 *   ctl      [P3V_SPEC_CTL_INTS]: n, n_draft, forced (non-zero: the tail proposes nothing and leaves n_draft = 0 -- the
 *            host writes tok[1..L) and n_draft before the next launch), replay (launches so far), n_limit, and the token
 *            count of the last launch
 *   amax     [L] scratch, ticket [1]: the arrival counter, ZERO before the first launch and left zero by every launch
 *   history  [hist_cap] PINNED HOST memory: token i of the run at history[i] (i = *d_step + 0 .. c-1)
 *   rec      [rec_cap][P3V_SPEC_REC_INTS] PINNED HOST memory: launch r writes {tokens emitted, drafts verified (k),
 *            d_0 .. d_{k-1}} to record r
 * p3v_spec_end: L = K + 1 rows of [L, n] bf16 logits; one 1024-thread workgroup per row takes its arg-max, the last one
 * to arrive does the rest.  p3v_spec_begin: x_out[j] = table[clamp(tok[j])], rotation rows of positions *d_past + j
 * (clamped to the table) into cos_out / sin_out [L, half_dim].  p3v_ngram_propose: the proposal alone, ctx[0..n) ->
 * draft[0 .. *n_draft).  L outside 1..P3V_DECODE_MAX_L, n_max outside n_min..P3V_SPEC_NGRAM_CAP, null pointers:
 * P3V_ERR_ARG, nothing launched. */
#define P3V_SPEC_DEFAULT_K 4
#define P3V_SPEC_NGRAM_MAX 3
#define P3V_SPEC_NGRAM_MIN 1
#define P3V_SPEC_NGRAM_CAP 8
#define P3V_SPEC_REC_INTS 18
#define P3V_SPEC_CTL_INTS 8
#define P3V_SPEC_CTL_N 0
#define P3V_SPEC_CTL_NDRAFT 1
#define P3V_SPEC_CTL_FORCED 2
#define P3V_SPEC_CTL_REPLAY 3
#define P3V_SPEC_CTL_NLIMIT 4
#define P3V_SPEC_CTL_ACC 5
typedef struct {
  int32_t* tok; int32_t* ctx; int32_t* ctl; int32_t* amax; int32_t* ticket;
  int32_t* history; int32_t* rec; int32_t* d_step; int32_t* d_past;
  int32_t ctx_cap, hist_cap, rec_cap, n_max, n_min;
} p3v_spec_state_t;
int p3v_spec_begin(const int32_t* tok, const uint16_t* table, uint16_t* x_out, const float* cos_t, const float* sin_t,
                   const int32_t* d_past, float* cos_out, float* sin_out, int L, int hidden, int vocab, int tab_t,
                   int half_dim, void* stream);
int p3v_spec_end(const uint16_t* logits, const p3v_spec_state_t* state /* host */, int L, int n, void* stream);
int p3v_ngram_propose(const int32_t* ctx, int n, int K, int n_max, int n_min, int vocab, int32_t* draft, int32_t* n_draft,
                      void* stream);

/* ---- beam search: the tail of a beam step and the K/V reorder behind it (added after round 6, no version change).
 * The rule (beam.py states it once more in NumPy and plain Python; the kernels are held to it bit for bit):
 *   State: W beams, 2 <= W <= P3V_BEAM_MAX, in rows 0 .. W-1 of a B = W slot state (every beam of a request has the same
 *   length, so the state's one offset fits them); cum[W] fp32, each beam's summed log-probability.
 *   Selection, step t: logits [R, n] bf16 contiguous and cum_in[R]; R = 1 at t = 0 (the one prefill row, cum_in = 0), R = W
 *   afterwards; n >= 2W.
 *   1. A row that is UNDEFINED by point 1 of the logprobs rule (a NaN, a +inf, no finite logit) FAILS the step.
 *   2. A row's candidates are its 2W tokens of largest value, ties to the lower index (p3v_topk's order); each carries
 *      logprob(i) by steps 2 - 6 of the logprobs rule and score = cum_in[r] + logprob, ONE fp32 addition (a -inf is an
 *      ordinary value).
 *   3. All R * 2W candidates are ordered by (score descending, r ascending, place in the row's list ascending): a total
 *      order, whose first 2W entries are the global best 2W.
 *   4. Walk those 2W entries, j = 0, 1, ...: a candidate whose token is `eos` is recorded as FINISHED (parent r, score) iff
 *      j < W and is ignored otherwise; any other candidate becomes the next beam k: tok[k], parent[k] = r, cum[k] = score;
 *      stop at W beams.  (W beams always exist: a row holds at most one EOS, so at most W of the 2W entries are EOS.)
 *   5. *d_step += 1 and *d_past += 1, done once, as p3v_step_end does.
 *   6. Record t (t = *d_step before point 5) goes to PINNED host memory with plain 4-byte stores, P3V_BEAM_REC_INTS words:
 *      {status, n_fin, tok[8], parent[8], cum bits[8], fin_parent[8], fin_score bits[8]}, unused entries -1; nothing is
 *      written when t lies outside [0, rec_cap).  A FAILED step writes status = 1, n_fin = 0 and -1 everywhere else; on the
 *      device tok[k] = -1 (the host raises, as on the plain step's negative token), parent[k] = k, cum stays, and the
 *      counters advance.
 *   Reorder: beam k continues row parent[k].  The prompt's columns are equal in every row (p3v_kv_fork), so only the window
 *   [c0a, min(ceil8(*d_past), T)) moves: c0a = the prompt's end rounded DOWN to 8 columns, a launch constant; *d_past is read
 *   AFTER point 5, so the column the step appended is inside.  The window is whole 8-column (16-byte) pieces on purpose:
 *   below the prompt's end the columns are equal in all rows, at or above *d_past they are not yet live, so V^T needs no
 *   sub-word edges.  Rows with parent[k] == k are not touched; every other row k < W gets row parent[k]'s window, K [T, hd]
 *   rows and V^T hd runs, all layers and kv heads.  In place that is a read / write hazard (a swap, a 3-cycle), so the move
 *   is two launches through caller-supplied staging, GATHER (phase 0): stage[k] <- row parent[k], then SCATTER (phase 1):
 *   row k <- stage[k].  No byte outside the moved rows' windows changes.
 * p3v_beam_state_t: every pointer is device memory unless stated.
 *   tok [W] the next step's rows, parent [W], cum [W] fp32 (read as cum_in[0 .. R), written in place by the last workgroup)
 *   cand_id / cand_score [P3V_BEAM_MAX * 2 * P3V_BEAM_MAX] scratch; ticket [1]: ZERO before the first launch, left zero
 *   rec [rec_cap][P3V_BEAM_REC_INTS] PINNED HOST memory
 * p3v_beam_end: R workgroups of 1024 threads, the last to arrive merges.  P3V_ERR_ARG, nothing launched: a null pointer, W
 * outside 2..P3V_BEAM_MAX, R not in {1, W}, n < 2W, rec_cap < 0; P3V_ERR_UNSUPPORTED: n > 65536.
 * p3v_kv_permute: k [nl, B, nkv, T, hd] and v [nl, B, nkv, hd, T] bf16 (p3v_kv_copy's layouts), B >= W; stage_k
 * [nl, W, nkv, stage_cols, hd], stage_v [nl, W, nkv, hd, stage_cols]; parent [W] and d_past [1] are DEVICE words, read by the
 * launch.  The grid is fixed for the capacity min(stage_cols, T - c0a); workgroups beyond the live window exit.  Defensive
 * rule: a parent[k] outside [0, W) leaves row k alone and the window is clamped to T and to c0a + stage_cols -- whatever the
 * device words hold, nothing outside the buffers is read or written.  P3V_ERR_UNSUPPORTED, nothing launched: elem_size != 2
 * (the int8 cache), hd * 2 % 16, T % 8.  P3V_ERR_ARG: null or misaligned (16 bytes) pointers, W outside 2..P3V_BEAM_MAX,
 * B < W, c0a outside [0, T] or not a multiple of 8, stage_cols < 8 or not a multiple of 8, a phase other than 0 / 1. */
#define P3V_BEAM_MAX 8
#define P3V_BEAM_REC_INTS (2 + 5 * P3V_BEAM_MAX)
typedef struct {
  int32_t* tok; int32_t* parent; float* cum; int32_t* cand_id; float* cand_score; int32_t* ticket;
  int32_t* rec; int32_t* d_step; int32_t* d_past;
  int32_t rec_cap;
} p3v_beam_state_t;
int p3v_beam_end(const uint16_t* logits, const p3v_beam_state_t* state /* host */, int R, int W, int n, int eos, void* stream);
int p3v_kv_permute(void* k, void* v, int B, int T, const int32_t* parent /* device */, int W, int c0a,
                   const int32_t* d_past /* device */, void* stage_k, void* stage_v, int stage_cols, int phase, int nl, int nkv,
                   int hd, int elem_size, void* stream);

/* ---- embeddings: final RMSNorm + pooling + L2 normalisation, fp32 out (added after round 6, no version change).
 * x [B, L, hidden] bf16 is the last layer's output BEFORE model.norm, w [hidden] bf16, start [B] int32 in device memory the
 * count of left-pad columns of each row (0 <= start[b] < L; read in P3V_POOL_MEAN only, values outside are clamped), out
 * [B, hidden] fp32.  The rule:
 *   y_t   = the bf16 row p3v_rmsnorm writes for x[b, t]: the same per-lane sum of squares, the same two roundings.
 *   LAST  : p = f32(y_{L-1}).  Row L - 1 is the only row read.
 *   MEAN  : p_j = (sum over t in [start_b, L) of f32(y_{t,j})) / (L - start_b): fp32 sums, ONE fp32 division.  The order of
 *           the sum is fixed by (start_b, L): sixteen partial sums over t = start_b + v (mod 16), added in the order of v.
 *   normalize = 1: e = p / sqrtf(sum_j p_j^2) (fp32 sum, IEEE square root and division).  A zero row stays zero, a NaN
 *           reaches every element of its row.
 * No floating-point atomics: row b's output bits depend on x[b], w and start[b] alone -- not on B, the neighbours or a
 * second launch.  hidden: every size p3v_rmsnorm takes (a multiple of 8), and multiples of 4 (8-byte loads; the rule is
 * the same with the row's last half chunk zero-extended).  ws: p3v_embed_pool_ws_bytes(B, L, hidden, mode) bytes of device
 * scratch (one fp32 per normalised row).  Three launches at most, nothing allocated, nothing synchronised.
 * Measured (profiles/embed_time.txt): a prefill that ends here costs 0.995 - 0.999x (LAST) / 1.007 - 1.015x (MEAN) the plain prefill.
 * P3V_ERR_ARG, nothing launched: a null x / w / out / ws, a null start in MEAN, B outside 1..65535, L < 1, hidden % 4,
 * pointers not 16-byte aligned (8 for hidden % 8 == 4), an unknown mode, normalize outside {0, 1}, a short workspace. */
#define P3V_POOL_LAST 0
#define P3V_POOL_MEAN 1
int64_t p3v_embed_pool_ws_bytes(int B, int L, int hidden, int mode);
int p3v_embed_pool(const uint16_t* x, const uint16_t* w, const int32_t* start, float* out, int B, int L, int hidden, float eps,
                   int mode, int normalize, void* ws, int64_t ws_bytes, void* stream);

/* ---- retrieval: scores of Q queries against N stored vectors and the k best per query (added after round 6, no version
 * change).  index [N, D] bf16 contiguous (N >= 0: the live rows of a possibly larger allocation), queries [Q, D] bf16,
 * idx [Q, k] int32, score [Q, k] fp32.  1 <= Q <= 16, 1 <= k <= P3V_SIM_TOPK_MAX, D % 8 == 0, 8 <= D <= 8192.  The rule:
 *   s(i, q) = sum_j f32(index[i, j]) * f32(queries[q, j]): exact products, an fp32 sum whose order is the kernel's own but
 *   FIXED per row -- 32-wide blocks of D in ascending order, each one v_mfma_f32_16x16x32_bf16 into the same accumulator
 *   (a last partial block is zero-extended).  s(i, q) has the same bits whatever N, Q, k or the split over workgroups.
 *   Output row q = the first k of a stable sort of the rows by (-s, i): ties go to the lower index, -0 == +0 (reported as
 *   +0), a NaN score sorts last (reported as a quiet NaN).  Where N < k the tail is idx -1 / score -inf.
 * Every index byte is read once per launch whatever Q is; the [Q, N] score matrix is never written.  Two launches: one
 * workgroup per rows_per_wg rows keeps its k candidates per query, one workgroup per query merges them out of ws
 * (p3v_sim_topk_ws_bytes(N, Q, k, D) bytes of device scratch, 8-byte aligned; may be NULL when that is 0).
 * p3v_sim_topk_plan states the split: workgroup g scores rows [g * rows_per_wg, min(N, (g + 1) * rows_per_wg)), n_wg of
 * them (0 for N = 0), each wave row_tile rows at a time.  It reads no device property: the same answer everywhere.
 * Measured at D = 3072 (profiles/embed_time.txt): N = 2^20, Q = 1: 1.09 ms at k = 1 (5.9 TB/s), 1.17 ms at k = 32; Q = 16:
 * 1.40 / 1.52 / 1.76 ms at k = 1 / 10 / 32 -- the candidate lists, not the stream, are what Q and k cost.
 * P3V_ERR_ARG, nothing launched: a shape outside the limits, null or misaligned (16 bytes) pointers, a short workspace. */
#define P3V_SIM_TOPK_MAX 32
int p3v_sim_topk_plan(int N, int Q, int k, int D, int* rows_per_wg /* host */, int* n_wg /* host */, int* row_tile /* host */);
int64_t p3v_sim_topk_ws_bytes(int N, int Q, int k, int D);
int p3v_sim_topk(const uint16_t* index, const uint16_t* queries, int32_t* idx, float* score, int N, int Q, int k, int D,
                 void* ws, int64_t ws_bytes, void* stream);

/* ---- hipGraph helpers: capture a sequence of the launches above and replay it */
int p3v_graph_begin(void* stream);
int p3v_graph_end(void* stream, void** graph_exec_out /* host */);
int p3v_graph_launch(void* graph_exec, void* stream);
int p3v_graph_destroy(void* graph_exec);

/* ---- timing with HIP events on a given stream (bench.py roofline leg) */
int p3v_event_create(void** ev /* host */);
int p3v_event_record(void* ev, void* stream);
int p3v_event_elapsed_ms(void* start, void* stop, float* ms /* host */);
int p3v_event_destroy(void* ev);

#ifdef __cplusplus
}
#endif
#endif /* P3V_H */
