// Shared-prefix decode attention (include/p3v.h: p3v_attention_decode_family).  The rows that generate(..., n=k) forks from one
// prefill hold bit-identical K / V^T in their prompt columns; a B = k decode step through p3v_attention_decode streams all k
// copies.  Here the key splits that lie wholly inside the shared columns are read ONCE, by the family leader's workgroup:
//   * k_attn_decode_stream's wave (p3v_attention.hip) has 16 query columns in its MFMA fragments, used there for the L <= 16
//     positions of one row.  Here column j of a shared split carries the L = 1 query of family member j: its own rotated query,
//     its own left padding, and its partial (o, m, l) goes to ITS workspace record (member row, head, split, slot 0);
//   * the workgroups of the followers for that split return before they request a byte, and write nothing;
//   * every other split (the one that contains share_end, everything after it, every split of a single row) runs with the row's
//     own query in column 0 against the row's own cache, patches and appends the new position: k_attn_decode_stream at L = 1.
// MFMA columns are computed independently of each other and the softmax state is per column, so a member's partial has the bits
// it would have had in column 0 of its own workgroup over its own copy: sharing changes no bit of the output.  A tile that lies
// wholly below a member's left padding leaves that column's state at (m, l, o) = (-inf, 0, 0) exactly (alpha = e = 0, finite V^T),
// which is what skipping the tile leaves: the leader may start at the smallest padding of its family.
// Splits are whole or not shared at all, so no workspace record ever has two writers, and the merge is k_attn_combine2 as it is.
// One wave per workgroup, grid (n_split, heads, B); LDS 27,136 bytes and the register budget of k_attn_decode_stream<64>
// (24 x 16-byte tile registers, 6 accumulators, 4 score fragments).
#include "p3v_common.h"
#include "p3v_attn_shared.h"       // rope_chunk, combine_threads, k_attn_combine2 (the merge launch, unchanged)

#include <limits.h>

struct AttnFamP {
  const bf16_t* qkv; const float* cos_t; const float* sin_t; bf16_t* k_cache; bf16_t* v_cache;
  const int32_t* pad_len; const int32_t* d_past; const int32_t* fam; float* ws;
  int B, nh, nkv, past, cache_t, rope_bstride, n_split;
  float scale;
  int chunk, grp, grp_magic;   // keys per split (multiple of 64), heads per kv head and ceil(2^16 / grp): as AttnDecP
};

// partial records are stored past the caches, as p3v_attention.hip stores them (the merge launch reads them from L2 / HBM)
__device__ __forceinline__ void fam_st_wt(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <int TK>
__global__ void __launch_bounds__(64) k_attn_family(AttnFamP p) {
  constexpr int HD = 96, KSTR = HD * 2 + 16, VSTR = TK * 2 + 16, NKS = 3, NDT = 6, CPR = 12;
  constexpr int KIT = TK * CPR / 64, VCH = TK / 8, VIT = HD * VCH / 64;   // 16-byte loads per lane: K, V^T
  __shared__ __attribute__((aligned(16))) unsigned char Ks[TK * KSTR];
  __shared__ __attribute__((aligned(16))) unsigned char Vt[HD * VSTR];
  const int lane = threadIdx.x, g = lane >> 4, qi = lane & 15;
  const int b = blockIdx.z, head = blockIdx.y, kvh = (head * p.grp_magic) >> 16;
  const bool kv_writer = head == kvh * p.grp;
  const float sc2 = p.scale * 1.4426950408889634f;            // scale * log2(e): softmax runs on exp2
  const int row_w = (p.nh + 2 * p.nkv) * HD;                  // qkv row width
  const int chunk = p.chunk;
  const int kv_lo = blockIdx.x * chunk, kv_hi = min(p.cache_t, kv_lo + chunk);

  // ---- this row's table entry and the cache length decide whether the split is shared: a follower must know before it
  //      requests a key, so (unlike k_attn_decode_stream) the first tile waits for these scalars
  const int32_t* fr = p.fam + (size_t)b * P3V_FAMILY_INTS;
  const int lead = fr[0], share_end = fr[1];
  const int mem = fr[2 + qi];
  const int past = p.d_past ? *p.d_past : p.past;
  const int pad_b = p.pad_len ? p.pad_len[b] : 0;
  const bool whole = kv_lo + chunk <= min(share_end, past);   // (s + 1) * chunk <= share_end; never beyond the live keys
  if (whole && lead != b && lead >= 0 && lead < p.B) return;  // a follower: its leader's workgroup writes this record

  const bool mem_ok = mem >= 0 && mem < p.B;                  // an entry outside [0, B) names nobody (memory safety does not rest on the host's check)
  const int n_mem = __builtin_popcountll(__ballot(mem_ok) & 0xffffull);
  const bool shared = whole && lead == b && n_mem >= 2;       // wave-uniform
  const int mrow = shared ? (mem_ok ? mem : -1) : (qi == 0 ? b : -1);   // the row whose query sits in this lane's column
  const bool qvalid = mrow >= 0;
  const int qrow_i = qvalid ? mrow : b;

  const bf16_t* kc = p.k_cache + ((size_t)b * p.nkv + kvh) * (size_t)p.cache_t * HD;
  bf16_t* vc = p.v_cache + ((size_t)b * p.nkv + kvh) * (size_t)HD * p.cache_t;          // V^T: [hd][cache_t]
  u32x4_t kreg[KIT], vreg[VIT];
  auto load_tile = [&](int kv0) {
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
      const int i = it * 64 + lane;
      kreg[it] = __builtin_nontemporal_load((const u32x4_t*)(kc + (size_t)(kv0 + i / CPR) * HD + (i % CPR) * 8));
    }
#pragma unroll
    for (int it = 0; it < VIT; ++it) {
      const int i = it * 64 + lane;
      vreg[it] = __builtin_nontemporal_load((const u32x4_t*)(vc + (size_t)(i / VCH) * p.cache_t + kv0 + (i % VCH) * 8));
    }
  };
  if (kv_lo < kv_hi) load_tile(kv_lo);                         // cache_t % TK == 0: the tile is always in bounds

  // every member's own left padding; the tiles start at the smallest one of the columns in use
  int pad_q = pad_b;
  if (shared) pad_q = !qvalid ? INT_MAX : p.pad_len ? p.pad_len[qrow_i] : 0;   // an unused column sees nothing
  int pad_lo = pad_b;
  if (shared) {
    pad_lo = pad_q;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) pad_lo = min(pad_lo, __shfl_xor(pad_lo, off));
    pad_lo = __builtin_amdgcn_readfirstlane(pad_lo);
  }
  const int total = past + 1;
  int kv_begin = kv_lo;
  const int kv_end = min(total, kv_hi);
  if (pad_lo > kv_begin) kv_begin = pad_lo & ~(TK - 1);
  const float* cos_b = p.cos_t + (size_t)b * p.rope_bstride * (HD / 2);
  const float* sin_b = p.sin_t + (size_t)b * p.rope_bstride * (HD / 2);

  // the new position `past`, when it falls in this tile (never in a shared split: those end at or below share_end <= past):
  // K rotated from the qkv row, V copied -- written into the LDS tile and appended to the cache by the writer head
  auto patch_new = [&](int kv0) {
    const int n0 = max(past, kv0), n1 = min(kv_end, kv0 + TK), n_new = n1 - n0;
#pragma unroll 1
    for (int w = lane; w < n_new * CPR; w += 64) {
      const int t = n0 + w / CPR, c = w % CPR;
      const bf16_t* row = p.qkv + (size_t)b * row_w;
      const u32x4_t kn = rope_chunk(row + (p.nh + kvh) * HD, c, cos_b, sin_b);
      *(u32x4_t*)(Ks + (t - kv0) * KSTR + c * 16) = kn;
      if (kv_writer) *(u32x4_t*)(p.k_cache + (((size_t)b * p.nkv + kvh) * p.cache_t + t) * HD + c * 8) = kn;
    }
#pragma unroll 1
    for (int w = lane; w < n_new * HD; w += 64) {
      const int t = n0 + w / HD, d = w % HD;
      const bf16_t val = p.qkv[(size_t)b * row_w + (p.nh + p.nkv + kvh) * HD + d];
      *(bf16_t*)(Vt + d * VSTR + (t - kv0) * 2) = val;
      if (kv_writer) vc[(size_t)d * p.cache_t + t] = val;
    }
  };
  if (kv_begin > kv_lo && kv_begin < kv_end) load_tile(kv_begin);   // left padding skipped whole tiles: reload

  bf16x8_t qf[NKS];
  {
    const bf16_t* qrow = p.qkv + (size_t)qrow_i * row_w + head * HD;
    const float* ct = p.cos_t + (size_t)qrow_i * p.rope_bstride * (HD / 2);
    const float* st = p.sin_t + (size_t)qrow_i * p.rope_bstride * (HD / 2);
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      u32x4_t v = rope_chunk(qrow, 4 * ks + g, ct, st);
      if (!qvalid) v = (u32x4_t){0, 0, 0, 0};
      qf[ks] = __builtin_bit_cast(bf16x8_t, v);
    }
  }

  float m_run = -INFINITY, l_run = 0.f;
  f32x4_t o[NDT];
#pragma unroll
  for (int d = 0; d < NDT; ++d) o[d] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  for (int kv0 = kv_begin; kv0 < kv_end; kv0 += TK) {
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
      const int i = it * 64 + lane;
      *(u32x4_t*)(Ks + (i / CPR) * KSTR + (i % CPR) * 16) = kreg[it];
    }
#pragma unroll
    for (int it = 0; it < VIT; ++it) {
      const int i = it * 64 + lane;
      *(u32x4_t*)(Vt + (i / VCH) * VSTR + (i % VCH) * 16) = vreg[it];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // this wave's LDS writes have landed (single-wave block)
    if (kv0 + TK > past) {                                     // wave-uniform: only the tile holding the new position
      patch_new(kv0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    if (kv0 + TK < kv_end) load_tile(kv0 + TK);                // next tile streams in under the MFMAs below

    f32x4_t s[TK / 16];
#pragma unroll
    for (int st = 0; st < TK / 16; ++st) {
      s[st] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const bf16x8_t kf = *(const bf16x8_t*)(Ks + (16 * st + qi) * KSTR + (32 * ks + 8 * g) * 2);
        s[st] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], s[st], 0, 0, 0);
      }
    }
    float m_t = -INFINITY;
#pragma unroll
    for (int st = 0; st < TK / 16; ++st)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = kv0 + 16 * st + 4 * g + r;
        const bool vis = t < kv_end && t >= pad_q && t <= past && past >= pad_q;    // this column's member: its own padding
        const float v = vis ? s[st][r] * sc2 : -INFINITY;               // log2 domain: scale*log2(e) folded in
        s[st][r] = v;
        m_t = fmaxf(m_t, v);
      }
    m_t = rows_max(m_t);
    const float m_new = fmaxf(m_run, m_t);
    const float m_use = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
    float l_t = 0.f;
#pragma unroll
    for (int st = 0; st < TK / 16; ++st)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f(s[st][r] - m_use);
        s[st][r] = e;
        l_t += e;
      }
    l_t = rows_sum(l_t);
    l_run = l_run * alpha + l_t;
    m_run = m_new;
#pragma unroll
    for (int d = 0; d < NDT; ++d) o[d] *= alpha;
#pragma unroll
    for (int st = 0; st < TK / 32; ++st) {
      u32x4_t pw;
      pw[0] = pack_bf16x2(s[2 * st][0], s[2 * st][1]);
      pw[1] = pack_bf16x2(s[2 * st][2], s[2 * st][3]);
      pw[2] = pack_bf16x2(s[2 * st + 1][0], s[2 * st + 1][1]);
      pw[3] = pack_bf16x2(s[2 * st + 1][2], s[2 * st + 1][3]);
      const bf16x8_t pf = __builtin_bit_cast(bf16x8_t, pw);
#pragma unroll
      for (int d = 0; d < NDT; ++d) {
        const unsigned char* vr = Vt + (16 * d + qi) * VSTR + (32 * st + 4 * g) * 2;
        const u32x2_t a0 = *(const u32x2_t*)vr, a1 = *(const u32x2_t*)(vr + 32);
        const u32x4_t aw = {a0[0], a0[1], a1[0], a1[1]};
        o[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, aw), pf, o[d], 0, 0, 0);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // LDS reads of this tile precede the next tile's writes
  }
  if (qvalid) {                                                // the member's own record: (member row, head, split, slot 0)
    float* w = p.ws + ((((size_t)mrow * p.nh + head) * p.n_split + blockIdx.x) * 16) * (HD + 2);
#pragma unroll
    for (int d = 0; d < NDT; ++d)
#pragma unroll
      for (int r = 0; r < 4; ++r) fam_st_wt(w + 16 * d + 4 * g + r, o[d][r]);
    if (g == 0) { fam_st_wt(w + HD, m_run); fam_st_wt(w + HD + 1, l_run); }
  }
}

// the host's copy of the table against the contract in p3v.h: P3V_OK, P3V_ERR_UNSUPPORTED (the refusals the header lists) or
// P3V_ERR_ARG (a table that contradicts itself)
static int fam_check(const int32_t* t, int B, int past /* < 0: only on the device */) {
  for (int b = 0; b < B; ++b) {
    const int32_t* r = t + (size_t)b * P3V_FAMILY_INTS;
    if (r[0] < 0 || r[0] >= B) return P3V_ERR_UNSUPPORTED;
    int size = 0;
    for (int o = 0; o < B; ++o) size += t[(size_t)o * P3V_FAMILY_INTS] == r[0];
    if (size > P3V_FAMILY_MAX) return P3V_ERR_UNSUPPORTED;
    if (r[0] != b) continue;
    for (int j = 0; j < P3V_FAMILY_MAX; ++j)
      if (r[2 + j] != -1 && (r[2 + j] < 0 || r[2 + j] >= B)) return P3V_ERR_UNSUPPORTED;
  }
  for (int b = 0; b < B; ++b) {
    const int32_t* r = t + (size_t)b * P3V_FAMILY_INTS;
    const int32_t* l = t + (size_t)r[0] * P3V_FAMILY_INTS;
    if (l[0] != r[0]) return P3V_ERR_ARG;                      // the row named as leader follows somebody else
    if (r[1] < 0 || r[1] != l[1]) return P3V_ERR_ARG;          // one share_end per family
    if (past >= 0 && r[1] > past) return P3V_ERR_UNSUPPORTED;
    int listed = 0, n = 0, followers = 0;
    for (int j = 0; j < P3V_FAMILY_MAX; ++j) listed += l[2 + j] == b;
    if (r[0] == b) {
      for (int j = 0; j < P3V_FAMILY_MAX; ++j) {
        if (r[2 + j] < 0) continue;
        ++n;
        if (t[(size_t)r[2 + j] * P3V_FAMILY_INTS] != b) return P3V_ERR_ARG;   // a listed member that follows another row
      }
      for (int o = 0; o < B; ++o) followers += o != b && t[(size_t)o * P3V_FAMILY_INTS] == b;
      if (n == 0 && followers == 0) continue;                  // a single row may leave its list empty
    }
    if (listed != 1) return P3V_ERR_ARG;                       // every row of a family stands once in its leader's list
  }
  return P3V_OK;
}

extern "C" int p3v_attention_decode_family(const p3v_attn_decode_args_t* a, const int32_t* family, const int32_t* family_host,
                                           void* stream) {
  if (!a || !a->qkv || !a->cos_t || !a->sin_t || !a->k_cache || !a->v_cache || !a->out || !a->ws || !family) return P3V_ERR_ARG;
  if (a->hd != 96 || a->L != 1 || a->o_proj_w || a->merge_in_launch) return P3V_ERR_UNSUPPORTED;
  if (a->B <= 0 || a->n_heads <= 0 || a->n_kv <= 0 || a->n_heads % a->n_kv) return P3V_ERR_ARG;
  if (a->n_split < 1 || a->n_split > 128 || a->cache_t <= 0 || a->cache_t % 64) return P3V_ERR_ARG;
  if (((uintptr_t)a->ws | (uintptr_t)a->out) & 15 || ((uintptr_t)family & 3)) return P3V_ERR_ARG;
  if (!a->d_past && (a->past < 0 || a->past >= a->cache_t)) return P3V_ERR_ARG;
  if (family_host) {
    const int rc = fam_check(family_host, a->B, a->d_past ? -1 : a->past);
    if (rc != P3V_OK) return rc;
  }
  const int grp = a->n_heads / a->n_kv;
  const int chunk = ((a->cache_t + a->n_split - 1) / a->n_split + 63) & ~63;
  AttnFamP p = {a->qkv, a->cos_t, a->sin_t, a->k_cache, a->v_cache, a->pad_len, a->d_past, family, a->ws,
                a->B, a->n_heads, a->n_kv, a->past, a->cache_t, a->rope_bstride, a->n_split, a->scale,
                chunk, grp, (65536 + grp - 1) / grp};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_attn_family<64>, dim3(a->n_split, a->n_heads, a->B), dim3(64), 0, s, p);
  P3V_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_attn_combine2, dim3(a->B * a->n_heads), dim3(combine_threads(a->n_split)), 0, s, a->ws, (bf16_t*)a->out, 1,
                     a->n_heads, a->hd, a->n_split);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}
