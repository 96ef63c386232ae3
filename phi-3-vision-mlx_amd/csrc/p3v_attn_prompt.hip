// Attention for the decoder (causal + left-pad, growing KV cache, head_dim 96;
// reference phi.py:454-457 with Mask4D phi.py:550-563) and for CLIP (no mask,
// head_dim 64; phi.py:148).  Scores and the mask are never materialised.
//
// One kernel, "swapped" MFMA formulation (per wave: 16 queries x 64-key tiles):
//   S^T[key,q] = K_tile[key,:] . Q[q,:]      v_mfma_f32_16x16x32_bf16, A = K rows from LDS, B = Q in VGPRs
//   online softmax: every lane owns ONE query column (q = lane&15) and 16 keys of
//     the tile, so max/sum need 15 in-lane ops + 2 shuffles and the rescale
//     factor is lane-local
//   O^T[d,q] += V^T[d,key] . P^T[key,q]      B = P straight from the S^T accumulators:
//     the MFMA k-index is permuted (k=(g,j) <-> key 32*st + 16*(j/4) + 4*g + j%4)
//     so that the P values a lane already holds ARE its B fragment; the same
//     permutation is applied when V^T is read from LDS.  P never leaves registers.
//
// Two launch shapes:
//   prefill  grid (ceil(L/64), heads, B): 4 waves = 4 query tiles sharing K/V tiles in LDS
//   decode   L <= 16: grid (n_split, heads, B): the KV range is split across
//            blocks (HBM-bound: reads 2*T*hd*2 bytes per head once); partial
//            (m, l, O) go to a workspace and `k_attn_combine` merges them.
//
// This file: the prompt-sized kernels (k_attn, k_attn_prefill, _dma, _pp, and _il from p3v_attn_il.h), the route that chooses among
// them and p3v_attention, which launches what the route says.  The decode kernels and `k_attn_combine2` are in p3v_attention.hip.
#include "p3v_common.h"
#include "p3v_attn_shared.h"       // combine_threads, k_attn_combine2 (defined in p3v_attention.hip): the split mode's merge launch

struct AttnP {
  const bf16_t* q; const bf16_t* k_past; const bf16_t* v_past; const bf16_t* k_new; const bf16_t* v_new;
  bf16_t* out; const int32_t* pad_len; const int32_t* d_past; float* ws;
  int B, L, nh, nkv, past, past_t, past_div, new_t, pad_div, causal, split_mode, n_split, new_is_cache;
  float scale;
  int head_group;              // k_attn_prefill_dma / _pp: heads whose query blocks are interleaved in launch order
  float sc2;                   // what S = Q.K^T is multiplied by before exp2: scale * log2(e), or 1 when Q arrives pre-scaled
  int q_prescaled;
};

template <int HD>
__global__ void __launch_bounds__(256) k_attn(AttnP p) {
  constexpr int KSTR = HD * 2 + 16;        // bytes per K row in LDS (padded: conflict-free b128 fragment reads)
  constexpr int VSTR = 64 * 2 + 16;        // bytes per V^T row in LDS (16-B aligned rows, conflict-free b64 reads)
  constexpr int NKS = HD / 32;             // k-steps of QK^T
  constexpr int NDT = HD / 16;             // 16-wide d tiles of O^T
  constexpr int CPR = HD / 8;              // 16-byte chunks per K/V row
  __shared__ __attribute__((aligned(16))) unsigned char Ks[64 * KSTR];
  __shared__ __attribute__((aligned(16))) unsigned char Vt[HD * VSTR];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, qi = lane & 15;
  const int b = blockIdx.z, head = blockIdx.y, kvh = head / (p.nh / p.nkv);
  const int past = p.d_past ? *p.d_past : p.past;
  const int total = past + p.L;
  const int pad = p.pad_len ? p.pad_len[b / p.pad_div] : 0;
  const float sc2 = p.sc2;                                     // scale * log2(e): softmax (and the split partials) run on exp2

  int q0, kv_begin, kv_end;
  bool active;
  if (p.split_mode) {
    q0 = 0;
    const int chunk = ((total + p.n_split - 1) / p.n_split + 63) & ~63;
    kv_begin = blockIdx.x * chunk;
    kv_end = min(total, kv_begin + chunk);
    active = wave == 0;
  } else {
    q0 = blockIdx.x * 64 + wave * 16;
    kv_begin = 0;
    kv_end = p.causal ? min(total, past + blockIdx.x * 64 + 64) : total;
    active = q0 < p.L;
  }
  if (pad > kv_begin) kv_begin = pad & ~63;       // tiles entirely inside the left padding are skipped

  const int qrow = q0 + qi;
  const bool qvalid = qrow < p.L;
  bf16x8_t qf[NKS];
  {
    const bf16_t* qp = p.q + (((size_t)b * p.nh + head) * p.L + (qvalid ? qrow : 0)) * HD + 8 * g;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      u32x4_t v = *(const u32x4_t*)(qp + 32 * ks);
      if (!qvalid) v = (u32x4_t){0, 0, 0, 0};
      qf[ks] = __builtin_bit_cast(bf16x8_t, v);
    }
  }
  const int qpos = past + qrow;                    // absolute position of this lane's query

  const bf16_t* kp_base = p.k_past + ((size_t)(b / p.past_div) * p.nkv + kvh) * (size_t)p.past_t * HD;
  const bf16_t* vp_base = p.v_past + ((size_t)(b / p.past_div) * p.nkv + kvh) * (size_t)HD * p.past_t;   // V^T: [hd][past_t]
  const bf16_t* kn_base = p.k_new + ((size_t)b * p.nkv + kvh) * (size_t)p.new_t * HD;
  const bf16_t* vn_base = p.v_new + ((size_t)b * p.nkv + kvh) * (size_t)HD * p.new_t;

  float m_run = -INFINITY, l_run = 0.f;
  f32x4_t o[NDT];
#pragma unroll
  for (int d = 0; d < NDT; ++d) o[d] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  for (int kv0 = kv_begin; kv0 < kv_end; kv0 += 64) {
    __syncthreads();
    for (int i = tid; i < 64 * CPR; i += 256) {               // K tile: 64 key rows x CPR 16-byte chunks
      const int key = i / CPR, c = i % CPR, t = kv0 + key;
      u32x4_t kv = {0, 0, 0, 0};
      if (t < kv_end) {
        const bool from_past = t < past || p.new_is_cache;
        const bf16_t* ks = from_past ? kp_base + (size_t)t * HD : kn_base + (size_t)(t - past) * HD;
        kv = *(const u32x4_t*)(ks + c * 8);
      }
      *(u32x4_t*)(Ks + key * KSTR + c * 16) = kv;
    }
    for (int i = tid; i < HD * 8; i += 256) {                 // V^T tile: HD rows x 8 chunks of 8 keys
      const int d = i >> 3, c = i & 7, t0 = kv0 + c * 8;
      u32x4_t vv = {0, 0, 0, 0};
      if (t0 < kv_end) {
        if (t0 + 8 <= past || p.new_is_cache) {
          vv = *(const u32x4_t*)(vp_base + (size_t)d * p.past_t + t0);
        } else {                                              // chunk touches the separate "new" segment (beam path)
          bf16_t e[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int t = t0 + j;
            e[j] = t < past ? vp_base[(size_t)d * p.past_t + t] : (t < kv_end ? vn_base[(size_t)d * p.new_t + (t - past)] : (bf16_t)0);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) vv[j] = (uint32_t)e[2 * j] | ((uint32_t)e[2 * j + 1] << 16);
        }
      }
      *(u32x4_t*)(Vt + d * VSTR + c * 16) = vv;
    }
    __syncthreads();
    if (!active) continue;

    // ---- S^T = K . Q^T for the 4 key sub-tiles
    f32x4_t s[4];
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      s[st] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const bf16x8_t kf = *(const bf16x8_t*)(Ks + (16 * st + qi) * KSTR + (32 * ks + 8 * g) * 2);
        s[st] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], s[st], 0, 0, 0);
      }
    }
    // ---- mask, running max
    float m_t = -INFINITY;
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = kv0 + 16 * st + 4 * g + r;
        const bool vis = t < kv_end && t >= pad && (!p.causal || t <= qpos) && qpos >= pad;
        const float v = vis ? s[st][r] * sc2 : -INFINITY;                 // log2 domain
        s[st][r] = v;
        m_t = fmaxf(m_t, v);
      }
    m_t = rows_max(m_t);
    const float m_new = fmaxf(m_run, m_t);
    const float m_use = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);       // m_run = -inf -> 0
    float l_t = 0.f;
#pragma unroll
    for (int st = 0; st < 4; ++st)
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
    // ---- O^T += V^T . P^T  (two 32-key steps; see the k-index permutation in the header)
#pragma unroll
    for (int st = 0; st < 2; ++st) {
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
  }

  if (!active || !qvalid) return;
  if (p.split_mode) {
    float* w = p.ws + ((((size_t)b * p.nh + head) * p.n_split + blockIdx.x) * 16 + qi) * (HD + 2);
#pragma unroll
    for (int d = 0; d < NDT; ++d) *(f32x4_t*)(w + 16 * d + 4 * g) = o[d];
    if (g == 0) { w[HD] = m_run; w[HD + 1] = l_run; }
  } else {
    const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
    bf16_t* op = p.out + ((size_t)b * p.L + qrow) * (size_t)(p.nh * HD) + head * HD + 4 * g;
#pragma unroll
    for (int d = 0; d < NDT; ++d) {
      u32x2_t w;
      w[0] = pack_bf16x2(o[d][0] * inv, o[d][1] * inv);
      w[1] = pack_bf16x2(o[d][2] * inv, o[d][3] * inv);
      *(u32x2_t*)(op + 16 * d) = w;
    }
  }
}

// =====================================================================================
// Prefill / CLIP attention (L > 16): 128 queries per workgroup (4 waves x 2 sub-tiles of 16), 64-key tiles,
// two LDS buffers.  The next tile's global loads are issued BEFORE the MFMAs of the current tile and written
// to the other LDS buffer after them (split stage: HBM/L2 latency hides under the matrix work), one barrier
// per tile.  K and V^T fragments read from LDS are shared by the wave's two query sub-tiles (48 MFMAs per
// 24 + 24 fragment reads).  Same swapped-MFMA formulation and masks as k_attn above.
template <int HD>
__global__ void __launch_bounds__(256, 2) k_attn_prefill(AttnP p) {
  constexpr int KSTR = HD * 2 + 16, VSTR = 64 * 2 + 16, NKS = HD / 32, NDT = HD / 16, CPR = HD / 8;
  constexpr int KTILE = 64 * KSTR, VTILE = HD * VSTR, BUF = KTILE + VTILE;
  constexpr int NLD = (64 * CPR + 255) / 256;               // 16-byte K loads per thread per tile (= V^T loads)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, qi = lane & 15;
  const int b = blockIdx.z, head = blockIdx.y, kvh = head / (p.nh / p.nkv);
  const int past = p.d_past ? *p.d_past : p.past;
  const int total = past + p.L;
  const int pad = p.pad_len ? p.pad_len[b / p.pad_div] : 0;
  const int qb0 = blockIdx.x * 128, q0 = qb0 + wave * 32;
  const int kv_end = p.causal ? min(total, past + qb0 + 128) : total;
  const int kv_begin = pad & ~63;
  const int wave_last = p.causal ? past + q0 + 31 : total;  // last key position this wave can see
  const float sc2 = p.sc2;                                            // scale * log2(e)

  bf16x8_t qf[2][NKS];
  int qpos[2];
  bool qvalid[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int qrow = q0 + u * 16 + qi;
    qvalid[u] = qrow < p.L;
    qpos[u] = past + qrow;
    const bf16_t* qp = p.q + (((size_t)b * p.nh + head) * p.L + (qvalid[u] ? qrow : 0)) * HD + 8 * g;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      u32x4_t v = *(const u32x4_t*)(qp + 32 * ks);
      if (!qvalid[u]) v = (u32x4_t){0, 0, 0, 0};
      qf[u][ks] = __builtin_bit_cast(bf16x8_t, v);
    }
  }
  const bf16_t* kp_base = p.k_past + ((size_t)(b / p.past_div) * p.nkv + kvh) * (size_t)p.past_t * HD;
  const bf16_t* vp_base = p.v_past + ((size_t)(b / p.past_div) * p.nkv + kvh) * (size_t)HD * p.past_t;
  const bf16_t* kn_base = p.k_new + ((size_t)b * p.nkv + kvh) * (size_t)p.new_t * HD;
  const bf16_t* vn_base = p.v_new + ((size_t)b * p.nkv + kvh) * (size_t)HD * p.new_t;

  u32x4_t kst[NLD], vst[NLD];
  auto stage_load = [&](int kv0) {
#pragma unroll
    for (int it = 0; it < NLD; ++it) {
      const int i = it * 256 + tid;
      kst[it] = (u32x4_t){0, 0, 0, 0};
      vst[it] = (u32x4_t){0, 0, 0, 0};
      if (i < 64 * CPR) {
        const int key = i / CPR, c = i % CPR, t = kv0 + key;
        if (t < kv_end) {
          const bool fp = t < past || p.new_is_cache;
          kst[it] = *(const u32x4_t*)((fp ? kp_base + (size_t)t * HD : kn_base + (size_t)(t - past) * HD) + c * 8);
        }
        const int d = i >> 3, c8 = i & 7, t0 = kv0 + c8 * 8;       // HD*8 == 64*CPR chunks as well
        if (t0 < kv_end) {
          if (t0 + 8 <= past || p.new_is_cache) {
            vst[it] = *(const u32x4_t*)(vp_base + (size_t)d * p.past_t + t0);
          } else {
            bf16_t e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const int t = t0 + j;
              e[j] = t < past ? vp_base[(size_t)d * p.past_t + t] : (t < kv_end ? vn_base[(size_t)d * p.new_t + (t - past)] : (bf16_t)0);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) vst[it][j] = (uint32_t)e[2 * j] | ((uint32_t)e[2 * j + 1] << 16);
          }
        }
      }
    }
  };
  auto stage_write = [&](int buf) {
    unsigned char* Ks = smem + buf * BUF;
    unsigned char* Vt = Ks + KTILE;
#pragma unroll
    for (int it = 0; it < NLD; ++it) {
      const int i = it * 256 + tid;
      if (i < 64 * CPR) {
        *(u32x4_t*)(Ks + (i / CPR) * KSTR + (i % CPR) * 16) = kst[it];
        *(u32x4_t*)(Vt + (i >> 3) * VSTR + (i & 7) * 16) = vst[it];
      }
    }
  };

  float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};
  f32x4_t o[2][NDT];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int d = 0; d < NDT; ++d) o[u][d] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  if (kv_begin < kv_end) { stage_load(kv_begin); stage_write(0); }
  __syncthreads();
  int buf = 0;
  for (int kv0 = kv_begin; kv0 < kv_end; kv0 += 64, buf ^= 1) {
    const bool more = kv0 + 64 < kv_end;
    if (more) stage_load(kv0 + 64);                         // in flight during the MFMAs below
    if (kv0 <= wave_last) {                                 // wave-uniform: tiles above this wave's diagonal are skipped
      const unsigned char* Ks = smem + buf * BUF;
      const unsigned char* Vt = Ks + KTILE;
      f32x4_t s[2][4];
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        s[0][st] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        s[1][st] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          const bf16x8_t kf = *(const bf16x8_t*)(Ks + (16 * st + qi) * KSTR + (32 * ks + 8 * g) * 2);
          s[0][st] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[0][ks], s[0][st], 0, 0, 0);
          s[1][st] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[1][ks], s[1][st], 0, 0, 0);
        }
      }
      // every key of the tile visible to every query of the wave -> no per-element mask work (wave-uniform)
      const bool interior = kv0 + 64 <= kv_end && kv0 >= pad && past + q0 >= pad && (!p.causal || kv0 + 63 <= past + q0);
      bf16x8_t pf[2][2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float m_t = -INFINITY;
        if (interior) {
#pragma unroll
          for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int r = 0; r < 4; ++r) m_t = fmaxf(m_t, s[u][st][r]);
        } else {
#pragma unroll
          for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int t = kv0 + 16 * st + 4 * g + r;
              const bool vis = t < kv_end && t >= pad && (!p.causal || t <= qpos[u]) && qpos[u] >= pad;
              const float v = vis ? s[u][st][r] : -INFINITY;
              s[u][st][r] = v;
              m_t = fmaxf(m_t, v);
            }
        }
        m_t = rows_max(m_t);
        // running max / exponentials in the log2 domain: exp(x*scale - m) = exp2(x*c - m2), c = scale*log2(e)
        const float m_new = fmaxf(m_run[u], m_t * sc2);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run[u] - m_use);
        float l_t = 0.f;
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = __builtin_amdgcn_exp2f(fmaf(s[u][st][r], sc2, -m_use));
            s[u][st][r] = e;
            l_t += e;
          }
        l_t = rows_sum(l_t);
        l_run[u] = l_run[u] * alpha + l_t;
        m_run[u] = m_new;
        if (!__all(alpha == 1.f)) {
#pragma unroll
          for (int d = 0; d < NDT; ++d) o[u][d] *= alpha;
        }
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          u32x4_t pw;
          pw[0] = pack_bf16x2(s[u][2 * st][0], s[u][2 * st][1]);
          pw[1] = pack_bf16x2(s[u][2 * st][2], s[u][2 * st][3]);
          pw[2] = pack_bf16x2(s[u][2 * st + 1][0], s[u][2 * st + 1][1]);
          pw[3] = pack_bf16x2(s[u][2 * st + 1][2], s[u][2 * st + 1][3]);
          pf[u][st] = __builtin_bit_cast(bf16x8_t, pw);
        }
      }
#pragma unroll
      for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int d = 0; d < NDT; ++d) {
          const unsigned char* vr = Vt + (16 * d + qi) * VSTR + (32 * st + 4 * g) * 2;
          const u32x2_t a0 = *(const u32x2_t*)vr, a1 = *(const u32x2_t*)(vr + 32);
          const u32x4_t aw = {a0[0], a0[1], a1[0], a1[1]};
          const bf16x8_t vf = __builtin_bit_cast(bf16x8_t, aw);
          o[0][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[0][st], o[0][d], 0, 0, 0);
          o[1][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[1][st], o[1][d], 0, 0, 0);
        }
    }
    if (more) stage_write(buf ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (!qvalid[u]) continue;
    const float inv = l_run[u] > 0.f ? 1.f / l_run[u] : 0.f;
    bf16_t* op = p.out + ((size_t)b * p.L + (q0 + u * 16 + qi)) * (size_t)(p.nh * HD) + head * HD + 4 * g;
#pragma unroll
    for (int d = 0; d < NDT; ++d) {
      u32x2_t w;
      w[0] = pack_bf16x2(o[u][d][0] * inv, o[u][d][1] * inv);
      w[1] = pack_bf16x2(o[u][d][2] * inv, o[u][d][3] * inv);
      *(u32x2_t*)(op + 16 * d) = w;
    }
  }
}

// Prefill / CLIP attention over a cache whose capacity is a multiple of 64 (every caller in the model): the K tile
// (64 rows x 2*HD bytes, contiguous) and the V^T tile (HD rows x 128 bytes) go HBM/L2 -> LDS by LDS-DMA, each wave
// issuing a quarter of the tile's 1 KiB pieces -- no staging registers, no ds_write pass, no per-tile address
// arithmetic (k_attn_prefill spends most of its issue slots there).  Bank-conflict swizzles on the source side:
//   192-byte K rows (HD = 96): chunk c ^ (-(row >> 2) & 3) (round 3: the round-2 form (row >> 2) & 3 was 2-way conflicted on ds_read_b128);   128-byte rows (K at HD = 64, V^T): chunk c ^ ((row >> 1) & 7).
// Two LDS buffers, one barrier per tile; compute part and masks identical to k_attn_prefill.
typedef const __attribute__((address_space(1))) void* pf_gptr_t;
typedef __attribute__((address_space(3))) void* pf_lptr_t;
template <int HD, bool PRE>                                    // PRE: Q arrives multiplied by scale * log2(e) (p3v_rope_kv_append's q_scale)
__global__ void __launch_bounds__(256, 2) k_attn_prefill_dma(AttnP p) {
  constexpr int KROW = HD * 2, VROW = 128, NKS = HD / 32, NDT = HD / 16, CPR = HD / 8;
  constexpr int KTILE = 64 * KROW, VTILE = HD * VROW, BUF = KTILE + VTILE;
  constexpr int NK = KTILE / 1024, NV = VTILE / 1024;         // 1 KiB DMA pieces per tile (K, V^T); NK % 4 == NV % 4 == 0
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, qi = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // Launch order (1-D over heads x query blocks): query blocks are walked from the LAST one down -- under a causal mask
  // block i costs i+1 tiles, so the dispatcher sees the longest jobs first and the tail of the launch is made of short
  // ones -- interleaving `head_group` heads at a time, so that the K/V of the heads in flight stay cache-resident
  // (all heads for short prompts; 8 or 4 when one head's K/V is megabytes).
  const int nqb = (p.L + 127) >> 7, per_group = p.head_group * nqb;
  const int grp = blockIdx.x / per_group, within = blockIdx.x - grp * per_group;
  const int qblk = nqb - 1 - within / p.head_group;
  const int b = blockIdx.z, head = grp * p.head_group + within % p.head_group, kvh = head / (p.nh / p.nkv);
  const int past = p.d_past ? *p.d_past : p.past;
  const int total = past + p.L;
  const int pad = p.pad_len ? p.pad_len[b / p.pad_div] : 0;
  const int qb0 = qblk * 128, q0 = qb0 + wave * 32;
  const int kv_end = p.causal ? min(total, past + qb0 + 128) : total;
  const int kv_begin = pad & ~63;
  const int wave_last = p.causal ? past + q0 + 31 : total;  // last key position this wave can see
  const float sc2 = p.sc2;                                            // scale * log2(e)

  bf16x8_t qf[2][NKS];
  int qpos[2];
  bool qvalid[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int qrow = q0 + u * 16 + qi;
    qvalid[u] = qrow < p.L;
    qpos[u] = past + qrow;
    const bf16_t* qp = p.q + (((size_t)b * p.nh + head) * p.L + (qvalid[u] ? qrow : 0)) * HD + 8 * g;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      u32x4_t v = *(const u32x4_t*)(qp + 32 * ks);
      if (!qvalid[u]) v = (u32x4_t){0, 0, 0, 0};
      qf[u][ks] = __builtin_bit_cast(bf16x8_t, v);
    }
  }
  const unsigned char* kbase = (const unsigned char*)(p.k_past + ((size_t)(b / p.past_div) * p.nkv + kvh) * (size_t)p.past_t * HD);
  const unsigned char* vbase = (const unsigned char*)(p.v_past + ((size_t)(b / p.past_div) * p.nkv + kvh) * (size_t)HD * p.past_t);

  // ---- per-lane DMA source offsets of this wave's pieces (piece j = wave + 4*jj covers LDS slots 64j .. 64j+63)
  unsigned koff[NK / 4];
#pragma unroll
  for (int jj = 0; jj < NK / 4; ++jj) {
    const int i = (wave + 4 * jj) * 64 + lane, row = i / CPR, pc = i - row * CPR;
    const int sw = HD == 96 ? (-(row >> 2)) & 3 : (row >> 1) & 7;   // conflict-free on ds_read_b128's lane groups (see k_attn_prefill_pp)
    koff[jj] = row * KROW + ((pc ^ sw) << 4);
  }
  const unsigned vrow = (unsigned)p.past_t * 2;
  unsigned voff[NV / 4];
#pragma unroll
  for (int jj = 0; jj < NV / 4; ++jj) {
    const int i = (wave + 4 * jj) * 64 + lane, row = i >> 3, pc = i & 7;
    voff[jj] = (unsigned)row * vrow + ((pc ^ ((row >> 1) & 7)) << 4);
  }
  // MUBUF form of the LDS-DMA (a pending `global_load_lds` makes the compiler turn every later wait into vmcnt(0) /
  // lgkmcnt(0): the fragment reads of the tile in work could not be counted while the next tile was in flight)
  const __amdgpu_buffer_rsrc_t rs_k = __builtin_amdgcn_make_buffer_rsrc((void*)kbase, 0, 0xffffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_v = __builtin_amdgcn_make_buffer_rsrc((void*)vbase, 0, 0xffffffff, 0x00020000);
  auto stage = [&](int kv0, int buf) {
    unsigned char* Ks = smem + buf * BUF;
    // (every argument of the builtin is copied into a local of non-dependent type: with a type-dependent argument -- an
    // element of an array whose size depends on HD -- the call is only checked at instantiation, fails there in the HOST pass,
    // where the builtin does not exist, and hipcc silently drops the kernel's host stub)
    const int so_k = kv0 * KROW, so_v = kv0 * 2;
#pragma unroll
    for (int jj = 0; jj < NK / 4; ++jj) {
      const unsigned vo = koff[jj];
      pf_lptr_t dst = (pf_lptr_t)(Ks + (wave + 4 * jj) * 1024);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_k, dst, 16, vo, so_k, 0, 0);
    }
#pragma unroll
    for (int jj = 0; jj < NV / 4; ++jj) {
      const unsigned vo = voff[jj];
      pf_lptr_t dst = (pf_lptr_t)(Ks + KTILE + (wave + 4 * jj) * 1024);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_v, dst, 16, vo, so_v, 0, 0);
    }
  };

  // ---- fragment read offsets
  unsigned k_rd[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int c = 4 * ks + g, sw = HD == 96 ? (-(qi >> 2)) & 3 : (qi >> 1) & 7;
    k_rd[ks] = qi * KROW + ((c ^ sw) << 4);                  // + st*16*KROW
  }
  unsigned v_rd[4];                                           // chunk (4 st + 2 h + g/2) ^ ((qi>>1)&7)
#pragma unroll
  for (int k = 0; k < 4; ++k) v_rd[k] = KTILE + qi * VROW + (((2 * k + (g >> 1)) ^ ((qi >> 1) & 7)) << 4) + (g & 1) * 8;   // + d*16*VROW

  // The row sums l ride on the matrix cores: one extra O^T tile whose V^T fragment is a register constant (row 0 all ones,
  // the other 15 rows zero), so l = P . 1 accumulates -- and is rescaled -- like any other output row, in lanes g = 0.
  // 4 MFMAs per tile instead of 32 v_add + two cross-lane reductions: the kernel is VALU-bound, the matrix pipe is 70 % idle.
  const u32x4_t ones_w = qi == 0 ? (u32x4_t){0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u} : (u32x4_t){0u, 0u, 0u, 0u};
  const bf16x8_t ones_f = __builtin_bit_cast(bf16x8_t, ones_w);
  float m_run[2] = {PRE ? 0.f : -INFINITY, PRE ? 0.f : -INFINITY};   // PRE: reference of the exponent (finite always), log2 units; else: running maximum
  unsigned long long unset[2] = {~0ull, ~0ull};              // lanes whose query has not seen a visible key yet: the next one sets the reference
  f32x4_t negm[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};   // (PRE) -reference, the C operand of the S^T products
  f32x4_t ol[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  f32x4_t o[2][NDT];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int d = 0; d < NDT; ++d) o[u][d] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  if (kv_begin < kv_end) stage(kv_begin, 0);
  int buf = 0;
  for (int kv0 = kv_begin; kv0 < kv_end; kv0 += 64, buf ^= 1) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's pieces of the tile have landed ...
    __syncthreads();                                          // ... everybody's have, and the other buffer is free
    if (kv0 + 64 < kv_end) stage(kv0 + 64, buf ^ 1);          // next tile streams in under the MFMAs below
    if (kv0 <= wave_last) {                                   // wave-uniform: tiles above this wave's diagonal are skipped
      const unsigned char* Ks = smem + buf * BUF;
      f32x4_t s[2][4];
      // the two MFMA blocks of a tile run at raised wave priority: the SIMD's other wave is usually in its softmax, and a
      // wave that has to wait for VALU slots between its MFMAs also loses the matrix pipe (8k: 650 -> 630 us)
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        s[0][st] = PRE ? negm[0] : (f32x4_t){0.f, 0.f, 0.f, 0.f};   // PRE: the accumulators START at -reference: the product IS the exponent
        s[1][st] = PRE ? negm[1] : (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          const bf16x8_t kf = *(const bf16x8_t*)(Ks + k_rd[ks] + st * 16 * KROW);
          s[0][st] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[0][ks], s[0][st], 0, 0, 0);
          s[1][st] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[1][ks], s[1][st], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
      // every key of the tile visible to every query of the wave -> no per-element mask work (wave-uniform)
      const bool interior = kv0 + 64 <= kv_end && kv0 >= pad && past + q0 >= pad && (!p.causal || kv0 + 63 <= past + q0);
      bf16x8_t pf[2][2];
      // PRE (pre-scaled Q: the decoder's prompts): softmax with a DEFERRED reference, as k_attn_prefill_pp / _il -- the S^T
      // accumulators started at -reference, so the product IS the exponent; the reference moves only on the query's first
      // visible tile and when a score exceeds it by more than 2^8 (wave-uniform slow path: O, l and the tile's scores are
      // rescaled once, in place).  Fast path: 16 max + 32 v_exp + 16 v_cvt_pk against ~280 VALU of the classic form below
      // (row maximum across lanes, new maximum, rescale factor and 28 multiplies on EVERY tile).
      // Plain Q (the ViT, external callers) keeps the classic form: the deferred form was built for it too (CLIP 62 -> 55 us)
      // and withdrawn -- correct and bit-stable once its multiply-add was written in place (as `s = fmaf(s, sc2, -m)` the
      // compiler put the results into the registers the last S^T MFMA had read and the output became NON-DETERMINISTIC:
      // 16-query halves wrong by up to 0.8 in some launches, tools/attn_determinism.py), but a different rounding sequence in
      // the ViT moves the heavy-tailed fixtures' logit error by +-40 % (chaotic amplification, profiles/r03_heavy_tail.txt)
      // past tolerances calibrated on one implementation.
      if constexpr (PRE) {
      // (the first readers of the S^T accumulators below are INLINE-ASM instructions: hipcc pads the MFMA -> reader wait states
      //  -- 12 for this 8-pass MFMA, guide 5.7 item 2 -- only for instructions it emits itself.  Today ~70 instructions of mask
      //  / interior arithmetic sit in between; the explicit pad keeps that from being an accident of the code layout.)
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_nop 7\n\ts_nop 4");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (!interior) {
          const float ninf = -INFINITY;
#pragma unroll
          for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int t = kv0 + 16 * st + 4 * g + r;
              const bool vis = t < kv_end && t >= pad && (!p.causal || t <= qpos[u]) && qpos[u] >= pad;
              const unsigned long long vm = __builtin_amdgcn_ballot_w64(vis);
              asm("v_cndmask_b32_e64 %0, %1, %0, %2" : "+v"(s[u][st][r]) : "v"(ninf), "s"(vm));      // s = vis ? s : -inf
            }
        }
        float ma, mc;                                          // this LANE's maximum over its 16 scores (no cross-lane step on the fast path)
        asm("v_max3_f32 %0, %1, %2, %3" : "=v"(ma) : "v"(s[u][0][0]), "v"(s[u][0][1]), "v"(s[u][0][2]));
        asm("v_max3_f32 %0, %1, %2, %3" : "=v"(mc) : "v"(s[u][0][3]), "v"(s[u][1][0]), "v"(s[u][1][1]));
        asm("v_max3_f32 %0, %0, %1, %2" : "+v"(ma) : "v"(s[u][1][2]), "v"(s[u][1][3]));
        asm("v_max3_f32 %0, %0, %1, %2" : "+v"(mc) : "v"(s[u][2][0]), "v"(s[u][2][1]));
        asm("v_max3_f32 %0, %0, %1, %2" : "+v"(ma) : "v"(s[u][2][2]), "v"(s[u][2][3]));
        asm("v_max3_f32 %0, %0, %1, %2" : "+v"(mc) : "v"(s[u][3][0]), "v"(s[u][3][1]));
        asm("v_max3_f32 %0, %0, %1, %2" : "+v"(ma) : "v"(s[u][3][2]), "v"(s[u][3][3]));
        asm("v_max_f32 %0, %0, %1" : "+v"(ma) : "v"(mc));
        if ((unset[u] | __builtin_amdgcn_ballot_w64(ma > 8.f)) != 0) {       // rare, wave-uniform: a reference moves
          const float m_t = rows_max(ma);
          const bool masked = m_t == -INFINITY;
          const bool un = (unset[u] >> lane) & 1;
          const float delta = un ? (masked ? 0.f : m_t) : fmaxf(m_t, 0.f);
          const float alpha = un ? 1.f : __builtin_amdgcn_exp2f(-delta);
          unset[u] &= __builtin_amdgcn_ballot_w64(masked);
          m_run[u] += delta;
          if (PRE) {
            const float nm = -m_run[u];                        // (in place: a new value would cost the fast path register copies)
#pragma unroll
            for (int r = 0; r < 4; ++r) asm("v_mov_b32 %0, %1" : "+v"(negm[u][r]) : "v"(nm));
          }
#pragma unroll
          for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int r = 0; r < 4; ++r) asm("v_sub_f32 %0, %0, %1" : "+v"(s[u][st][r]) : "v"(delta));
#pragma unroll
          for (int d = 0; d < NDT; ++d)
#pragma unroll
            for (int r = 0; r < 4; ++r) asm("v_mul_f32 %0, %0, %1" : "+v"(o[u][d][r]) : "v"(alpha));
#pragma unroll
          for (int r = 0; r < 4; ++r) asm("v_mul_f32 %0, %0, %1" : "+v"(ol[u][r]) : "v"(alpha));
        }
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
          for (int r = 0; r < 4; ++r) s[u][st][r] = __builtin_amdgcn_exp2f(s[u][st][r]);
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          u32x4_t pw;
          pw[0] = pack_bf16x2(s[u][2 * st][0], s[u][2 * st][1]);
          pw[1] = pack_bf16x2(s[u][2 * st][2], s[u][2 * st][3]);
          pw[2] = pack_bf16x2(s[u][2 * st + 1][0], s[u][2 * st + 1][1]);
          pw[3] = pack_bf16x2(s[u][2 * st + 1][2], s[u][2 * st + 1][3]);
          pf[u][st] = __builtin_bit_cast(bf16x8_t, pw);
        }
      }
      } else {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float m_t = -INFINITY;
        if (interior) {
#pragma unroll
          for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int r = 0; r < 4; ++r) m_t = fmaxf(m_t, s[u][st][r]);
        } else {
#pragma unroll
          for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int t = kv0 + 16 * st + 4 * g + r;
              const bool vis = t < kv_end && t >= pad && (!p.causal || t <= qpos[u]) && qpos[u] >= pad;
              const float v = vis ? s[u][st][r] : -INFINITY;
              s[u][st][r] = v;
              m_t = fmaxf(m_t, v);
            }
        }
        m_t = rows_max(m_t);
        const float m_new = fmaxf(m_run[u], m_t * sc2);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run[u] - m_use);
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
          for (int r = 0; r < 4; ++r) s[u][st][r] = __builtin_amdgcn_exp2f(fmaf(s[u][st][r], sc2, -m_use));
        m_run[u] = m_new;
        if (!__all(alpha == 1.f)) {
#pragma unroll
          for (int d = 0; d < NDT; ++d) o[u][d] *= alpha;
          ol[u] *= alpha;
        }
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          u32x4_t pw;
          pw[0] = pack_bf16x2(s[u][2 * st][0], s[u][2 * st][1]);
          pw[1] = pack_bf16x2(s[u][2 * st][2], s[u][2 * st][3]);
          pw[2] = pack_bf16x2(s[u][2 * st + 1][0], s[u][2 * st + 1][1]);
          pw[3] = pack_bf16x2(s[u][2 * st + 1][2], s[u][2 * st + 1][3]);
          pf[u][st] = __builtin_bit_cast(bf16x8_t, pw);
        }
      }
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int d = 0; d < NDT; ++d) {
          const u32x2_t a0 = *(const u32x2_t*)(Ks + v_rd[2 * st] + d * 16 * VROW);
          const u32x2_t a1 = *(const u32x2_t*)(Ks + v_rd[2 * st + 1] + d * 16 * VROW);
          const u32x4_t aw = {a0[0], a0[1], a1[0], a1[1]};
          const bf16x8_t vf = __builtin_bit_cast(bf16x8_t, aw);
          o[0][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[0][st], o[0][d], 0, 0, 0);
          o[1][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[1][st], o[1][d], 0, 0, 0);
        }
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        ol[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones_f, pf[0][st], ol[0], 0, 0, 0);
        ol[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones_f, pf[1][st], ol[1], 0, 0, 0);
      }
      __builtin_amdgcn_s_setprio(0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const float l_fin[2] = {rows_sum(ol[0][0]), rows_sum(ol[1][0])};   // the sum sits in the g = 0 lane of the query's column (all lanes take part)
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (!qvalid[u]) continue;
    const float inv = l_fin[u] > 0.f ? 1.f / l_fin[u] : 0.f;
    bf16_t* op = p.out + ((size_t)b * p.L + (q0 + u * 16 + qi)) * (size_t)(p.nh * HD) + head * HD + 4 * g;
#pragma unroll
    for (int d = 0; d < NDT; ++d) {
      u32x2_t w;
      w[0] = pack_bf16x2(o[u][d][0] * inv, o[u][d][1] * inv);
      w[1] = pack_bf16x2(o[u][d][2] * inv, o[u][d][3] * inv);
      *(u32x2_t*)(op + 16 * d) = w;
    }
  }
}

// =====================================================================================
// Ping-pong prefill attention (round 3).  Where k_attn_prefill_dma lost its time (in-kernel phase counters):
// per 64-key tile a wave spent 830 cycles on the 24 S^T MFMAs (384 matrix-pipe cycles), 2430 on the softmax (~700 VALU
// cycles) and 1450 on the 28 PV MFMAs (448) -- neither pipe of a SIMD was busier than ~35 %: the SIMD's two waves (one of
// each of the CU's two workgroups) drift in and out of the same phase, share the pipe they both want and leave the other
// idle.  Here the pairing is made deterministic:
//   * ONE workgroup of 8 waves per CU covers 256 queries of a (batch row, head); waves w and w + 4 share a SIMD.  Waves
//     0-3 (group A) and 4-7 (group B) run the same per-tile sequence  [PV(j-1) + S^T(j)] -> [softmax(j)]  half a tile apart:
//     in every step one wave of each SIMD is in its MATRIX phase (52 MFMAs, LDS fragment reads, DMA issue) while its
//     partner is in its VALU phase (softmax of 32 queries x 64 keys); one s_barrier per step keeps them in anti-phase.
//   * VALU work per score cut to the exponential itself: Q arrives PRE-SCALED by scale * log2(e) (the RoPE kernel
//     multiplies before its one rounding to bf16 -- same relative rounding as before), the S^T accumulators START at
//     -m (the running reference of the query's column, lane-uniform over the accumulator rows), so the MFMA result IS
//     the exponent; the reference only moves when a tile's maximum exceeds it by more than 2^8 (wave-uniform slow path
//     that rescales O and l once; P <= 256 in bf16 has the same relative precision) -- and on a query's first visible
//     tile, which sets it.  Fast path per tile and wave: 32 v_exp + 16 v_cvt_pk + ~28 max / select / swap.
//   * K / V^T tiles by LDS-DMA into a ring of four K tiles and five V^T tiles (see issue_batch for the depths), 24 (HD = 96)
//     one-KiB pieces per tile pair = 3 per wave, issued at the top of a VALU phase two to three tiles ahead of their use; counted
//     vmcnt (one batch stays in flight across every barrier), never a full drain inside the loop.  The K tile is staged in a
//     PERMUTED key order that makes every V^T fragment one ds_read_b128 (see load_k), both tiles conflict-free.
//   * fragment reads are taken off the MFMA stream: V^T(j) is read at the top of softmax(j) (lands under the VALU work), K(j+1)
//     at the top of the matrix phase, under the 28 PV MFMAs; the S^T accumulators start from a persistent -reference block.
//   * every tile of K / V^T is fetched ONCE per 256 queries (128 before): half the L2 -> LDS traffic per flop.
// What the compiler must be kept from doing (each cost 1.5-2x, found with SQ_INSTS_VALU and the in-kernel phase timeline,
// tools/attn_pp_timeline.py): conditional updates of the accumulator arrays written as C++ (-> 600 register copies per tile:
// in-place inline asm instead); sinking the exponentials past the asm barrier into the matrix phase (-> results pinned with
// empty volatile asm uses); spilling lane-constant LDS offsets (reload = scratch load = vmcnt(0) = DMA drained: recomputed per
// phase from an opaque lane id).
// Row sums ride on the matrix cores as before (ones-row V^T fragment).
#ifndef P3V_PP_DMA_IN_VALU
#define P3V_PP_DMA_IN_VALU 1
#endif
#ifndef P3V_PP_V_IN_MATRIX
#define P3V_PP_V_IN_MATRIX 1                                    // 1: both halves of the V^T fragments are read in the matrix phase
#endif
#ifdef P3V_PP_DEBUG                                             // tools/attn_pp_timeline.py: per-wave phase timestamps of ONE workgroup
__device__ unsigned long long p3v_ppdbg[8 * 128];
#define PP_T(slot) do { if (blockIdx.x == P3V_PP_DEBUG && (threadIdx.x & 63) == 0 && (slot) < 127) p3v_ppdbg[(threadIdx.x >> 6) * 128 + 1 + (slot)] = __builtin_readcyclecounter(); } while (0)
extern "C" int p3v_ppdbg_read(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(p3v_ppdbg), sizeof(unsigned long long) * 8 * 128) == hipSuccess ? 0 : -1;
}
// stamps INSIDE a phase: s_memtime into an SGPR pair (consumed at the end of the step only: no lgkmcnt wait at the stamp)
__device__ unsigned long long p3v_ppdbg2[8 * 64 * 4];
#define PP_S(k) do { __builtin_amdgcn_sched_barrier(0); asm volatile("s_memtime %0" : "=s"(pp_s[k])); __builtin_amdgcn_sched_barrier(0); } while (0)
#define PP_S_FLUSH(step) do { if (blockIdx.x == P3V_PP_DEBUG && (threadIdx.x & 63) == 0 && (step) < 64) { for (int k_ = 0; k_ < 4; ++k_) p3v_ppdbg2[((threadIdx.x >> 6) * 64 + (step)) * 4 + k_] = pp_s[k_]; } } while (0)
extern "C" int p3v_ppdbg2_read(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(p3v_ppdbg2), sizeof(unsigned long long) * 8 * 64 * 4) == hipSuccess ? 0 : -1;
}
#else
#define PP_T(slot) do { } while (0)
#define PP_S(k) do { } while (0)
#define PP_S_FLUSH(step) do { } while (0)
#endif
template <int HD, bool PRE>
__global__ void __launch_bounds__(512, 1) k_attn_prefill_pp(AttnP p) {
  constexpr int KROW = HD * 2, VROW = 128, NKS = HD / 32, NDT = HD / 16, CPR = HD / 8;
  constexpr bool DV = P3V_PP_DMA_IN_VALU;                      // DMA batches issued from the VALU phase (see issue_batch)
  constexpr int KTILE = 64 * KROW, VTILE = HD * VROW, RING = DV ? 4 : 3, VRING = DV ? 5 : 4;   // ring depths: see issue_batch
  constexpr int NK = KTILE / 1024, NV = VTILE / 1024, NPW = (NK + NV) / 8;   // DMA pieces per tile (K, V^T) and per wave and batch
  constexpr float THR = 8.f;
  static_assert((NK + NV) % 8 == 0, "pieces must divide over 8 waves");
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];   // K ring [RING][KTILE] | V^T ring [VRING][VTILE]
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, qi = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), grp = wave >> 2;
  const int nqb = (p.L + 255) >> 8, per_group = p.head_group * nqb;
  const int hgrp = blockIdx.x / per_group, within = blockIdx.x - hgrp * per_group;
  const int qblk = nqb - 1 - within / p.head_group;             // longest (last) query blocks first
  const int b = blockIdx.z, head = hgrp * p.head_group + within % p.head_group, kvh = head / (p.nh / p.nkv);
  const int past = p.d_past ? *p.d_past : p.past;
  const int total = past + p.L;
  const int pad = p.pad_len ? p.pad_len[b / p.pad_div] : 0;
  const int qb0 = qblk * 256, q0 = qb0 + wave * 32;
  const int kv_end = p.causal ? min(total, past + qb0 + 256) : total;
  const int kv_begin = min(pad & ~63, kv_end);
  const int NT = (kv_end - kv_begin + 63) >> 6;
#ifdef P3V_PP_SOLO                                               // timing experiment: group B idles
  const bool active = q0 < p.L && grp == 0;
#else
  const bool active = q0 < p.L;
#endif
  const int wave_last = p.causal ? past + q0 + 31 : total;  // last key position this wave can see
  const float sc2 = p.sc2;                                   // !PRE only
  // interior tiles of this wave: kv0 >= pad, kv0 + 64 <= kv_end, (causal) kv0 + 63 <= past + q0, and no padded query rows
  const int j_int_lo = (past + q0 >= pad) ? ((pad > kv_begin) ? 1 : 0) : (1 << 30);
  const int j_int_hi = min((kv_end - kv_begin) / 64 - 1, p.causal ? (past + q0 - 63 - kv_begin >= 0 ? (past + q0 - 63 - kv_begin) / 64 : -1) : (1 << 30));

  bf16x8_t qf[2][NKS];
  int qpos[2];
  bool qvalid[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int qrow = q0 + u * 16 + qi;
    qvalid[u] = qrow < p.L;
    qpos[u] = past + qrow;
    const bf16_t* qp = p.q + (((size_t)b * p.nh + head) * p.L + (qvalid[u] ? qrow : 0)) * HD + 8 * g;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      u32x4_t v = *(const u32x4_t*)(qp + 32 * ks);
      if (!qvalid[u]) v = (u32x4_t){0, 0, 0, 0};
      qf[u][ks] = __builtin_bit_cast(bf16x8_t, v);
    }
  }
  const unsigned char* kbase = (const unsigned char*)(p.k_past + ((size_t)(b / p.past_div) * p.nkv + kvh) * (size_t)p.past_t * HD);
  const unsigned char* vbase = (const unsigned char*)(p.v_past + ((size_t)(b / p.past_div) * p.nkv + kvh) * (size_t)HD * p.past_t);
  const __amdgpu_buffer_rsrc_t rs_k = __builtin_amdgcn_make_buffer_rsrc((void*)kbase, 0, 0xffffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_v = __builtin_amdgcn_make_buffer_rsrc((void*)vbase, 0, 0xffffffff, 0x00020000);

  // ---- this wave's DMA pieces: piece pi = wave + 8 i of the list [K_0 .. K_{NK-1}, V_0 .. V_{NV-1}]
  const unsigned vrow = (unsigned)p.past_t * 2;
  unsigned poff[NPW];
#pragma unroll
  for (int i = 0; i < NPW; ++i) {
    const int pi = wave + 8 * i;
    if (pi < NK) {
      const int e = pi * 64 + lane, row = e / CPR, pc = e - row * CPR;
      const int sw = HD == 96 ? (-(row >> 2)) & 3 : (row >> 1) & 7;
      const int blk = row >> 4, i_ = row & 15;               // LDS row (block blk, A-operand row i_) holds key pi_key of the tile
      const int key = 32 * (blk >> 1) + 8 * (i_ >> 2) + 4 * (blk & 1) + (i_ & 3);
      poff[i] = key * KROW + ((pc ^ sw) << 4);
    } else {
      const int e = (pi - NK) * 64 + lane, row = e >> 3, pc = e & 7;
      poff[i] = (unsigned)row * vrow + ((pc ^ ((row >> 1) & 7)) << 4);
    }
  }
  // batch jb = K tile jb + 2 and V^T tile jb + 2, issued at the top of the matrix phase M(jb) (group A: step 2 jb, group B:
  // step 2 jb + 1) and waited for by every wave before the barrier that ends step 2 jb + 3.  First readers: K(j) in M(j)
  // (step 2j), V^T(j) in softmax(j) (step 2j + 1) -- both after the end of step 2 (j - 2) + 3.  Last readers of the slot a
  // batch overwrites: K(jb - 1), read in M(jb - 1) (steps 2 jb - 2 / 2 jb - 1) -> three K slots; V^T(jb - 2), read in
  // softmax(jb - 2) (steps 2 jb - 3 / 2 jb - 2) -> FOUR V^T slots (with three, group A's batch jb would land on the tile
  // group B's softmax(jb - 1) is still reading in step 2 jb).  Prologue batches -2, -1 = tiles 0, 1 (clamped into [0, NT)).
  // DV (round 3, late): the matrix phase is the longer one and a DMA issue costs its wave ~100 cycles of MFMA issue, so batch
  // jb >= 1 is issued one step EARLIER, at the top of the wave's VALU phase softmax(jb - 1) (A: step 2 jb - 1, B: 2 jb); the
  // slots it overwrites must then be one tile older: K(jb - 2) (last read in M(jb - 2), steps 2 jb - 4 / 2 jb - 3) -> FOUR
  // K slots, V^T(jb - 3) (second half read in M(jb - 2)) -> FIVE V^T slots (with four, A's batch would land in step 2 jb - 1 on
  // the tile whose second half B's M(jb - 1) reads in that step).  Each wave issues its batches in order (`next_b`); what
  // may stay in flight across the barrier of an odd step is whatever it has issued beyond batch jn - 2 (end_step).
  int next_b = 0;
  auto issue_batch = [&](int jb) {
#ifdef P3V_PP_NODMA                                              // timing experiment: tiles never move
    return;
#endif
    const int tk = min(jb + 2, NT - 1), tv = tk;
    const int ks_ = (jb + 2) % RING, vs_ = (jb + 2) % VRING;
    const int so_k = (kv_begin + 64 * tk) * KROW, so_v = (kv_begin + 64 * tv) * 2;
#pragma unroll
    for (int i = 0; i < NPW; ++i) {
      const int pi = wave + 8 * i;
      const unsigned vo = poff[i];
      if (pi < NK) {
        pf_lptr_t dst = (pf_lptr_t)(smem + ks_ * KTILE + pi * 1024);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_k, dst, 16, vo, so_k, 0, 0);
      } else {
        pf_lptr_t dst = (pf_lptr_t)(smem + RING * KTILE + vs_ * VTILE + (pi - NK) * 1024);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_v, dst, 16, vo, so_v, 0, 0);
      }
    }
  };

  auto issue_at = [&](int ls) {                               // the batch a wave issues at the top of its local step ls, if any
    const int jb = DV ? (ls == 0 ? 0 : (ls & 1) ? (ls + 1) >> 1 : -1) : ((ls & 1) ? -1 : ls >> 1);
    if (jb == next_b && jb <= NT - 3) {
      issue_batch(jb);
      ++next_b;
    }
  };

  // ---- fragment read offsets (as k_attn_prefill_dma), RECOMPUTED at the top of every phase from a lane id the compiler
  // cannot see through: kept live across the tile loop they are spilled (the kernel sits at the 256-register limit of two
  // waves per SIMD), and a spill reload is a scratch load -- its compiler-inserted vmcnt(0) drains the LDS-DMA in flight
  auto lane_now = [&]() {
    unsigned l = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    asm volatile("" : "+v"(l));
    return l;
  };

  const u32x4_t ones_w = qi == 0 ? (u32x4_t){0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u} : (u32x4_t){0u, 0u, 0u, 0u};
  const bf16x8_t ones_f = __builtin_bit_cast(bf16x8_t, ones_w);
  float m_run[2] = {0.f, 0.f};                               // reference of the exponent (finite always)
  bool unset[2] = {true, true};                              // no visible key seen yet: the next one sets the reference
  f32x4_t ol[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  f32x4_t o[2][NDT];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int d = 0; d < NDT; ++d) o[u][d] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  f32x4_t s[2][4];
  bf16x8_t pf[2][2];
#ifdef P3V_PP_DEBUG
  unsigned long long pp_s[4] = {0, 0, 0, 0};
#endif

  // Key order inside a tile.  The S^T accumulator rows a lane holds (rows 4g .. 4g+3 of each 16-row block) become ITS
  // B fragment of the PV product, k index (g, 0..7) = (block 2st', rows 4g..4g+3), (block 2st'+1, rows 4g..4g+3).  The K
  // tile is staged so that A-operand row i of block b is key 32 (b >> 1) + 8 (i >> 2) + 4 (b & 1) + (i & 3) of the tile
  // (the DMA fetches 16-byte chunks from anywhere: a permuted row order is free): a lane's eight k values are then the
  // EIGHT CONSECUTIVE keys 32 st' + 8 g .. + 7, and its V^T fragment is ONE ds_read_b128 (k_attn_prefill_dma: two
  // ds_read_b64 that the compiler fuses into the half-rate ds_read2st64_b64).  Bank conflicts: none on either tile
  // (the 16-lane service groups of ds_read_b128 are {0-3,12-15,20-27}, {4-11,16-19,28-31}, ...: the K swizzle for 192-byte
  // rows is chunk ^ (-(row >> 2) & 3) inside aligned groups of four; k_attn_prefill_dma's (row >> 2) & 3 was 2-way
  // conflicted on every read, SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.50).
  f32x4_t negm[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};   // C operand of the S^T products: -reference (PRE) or 0
  bf16x8_t kfr[4][NKS];                                      // K fragments of the tile in work (loaded under the PV MFMAs)
  bf16x8_t vfr[2][NDT];                                      // V^T fragments (loaded under the softmax of the same tile)
  auto load_k = [&](int j) {
    const unsigned char* Ks = smem + (j % RING) * KTILE;
    const unsigned ln = lane_now(), g_ = ln >> 4, qi_ = ln & 15;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const unsigned c = 4 * ks + g_, sw = HD == 96 ? (0u - (qi_ >> 2)) & 3 : (qi_ >> 1) & 7;
      const unsigned off = qi_ * KROW + ((c ^ sw) << 4);
#pragma unroll
      for (int st = 0; st < 4; ++st) kfr[st][ks] = *(const bf16x8_t*)(Ks + off + st * 16 * KROW);
    }
  };
  auto load_v = [&](int j, int st) {                         // half st (keys 32 st .. 32 st + 31) of V^T(j)
    const unsigned char* Vs = smem + RING * KTILE + (j % VRING) * VTILE;
    const unsigned ln = lane_now(), g_ = ln >> 4, qi_ = ln & 15;
    const unsigned off = qi_ * VROW + (((4 * st + g_) ^ ((qi_ >> 1) & 7)) << 4);
#pragma unroll
    for (int d = 0; d < NDT; ++d) vfr[st][d] = *(const bf16x8_t*)(Vs + off + d * 16 * VROW);
  };
  auto qk = [&]() {                                          // S^T(j) = K_j . Q^T (- reference), K_j in kfr
    // the first MFMA of every accumulator takes the persistent block `negm` (-reference in all four rows) as its C
    // operand: no per-tile initialisation of the 32 accumulator registers
    // (k-slice outermost: eight independent accumulators between two MFMAs of one chain -- with the slice innermost a chain's
    //  next MFMA issued two slots after its predecessor, inside its 8-pass latency: SQ_WAIT_INST_ANY was 38 % of the wave cycles)
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
#pragma unroll
      for (int st = 0; st < 4; ++st) {
#ifdef P3V_PP_NOLDS                                              // timing experiment: no fragment reads
        const bf16x8_t kf = qf[1][ks];
#else
        const bf16x8_t kf = kfr[st][ks];
#endif
        s[0][st] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[0][ks], ks == 0 ? negm[0] : s[0][st], 0, 0, 0);
        s[1][st] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[1][ks], ks == 0 ? negm[1] : s[1][st], 0, 0, 0);
      }
    }
  };
  auto pv = [&]() {                                          // O^T += V^T_j . P^T(j), l += 1 . P^T(j), V^T_j in vfr
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int d = 0; d < NDT; ++d) {
#ifdef P3V_PP_NOLDS
        const bf16x8_t vf = qf[0][d % NKS];
#else
        const bf16x8_t vf = vfr[st][d];
#endif
        o[0][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[0][st], o[0][d], 0, 0, 0);
        o[1][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[1][st], o[1][d], 0, 0, 0);
      }
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      ol[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones_f, pf[0][st], ol[0], 0, 0, 0);
      ol[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones_f, pf[1][st], ol[1], 0, 0, 0);
    }
  };
  // Every conditional update of the big register arrays (mask, moved reference) is an IN-PLACE inline-asm instruction on
  // the array element ("+v"): written as C++ selects / multiplies the compiler gives the updated array NEW registers and
  // fills the common path with copies -- 600 v_mov per tile and wave in the first version of this kernel (SQ_INSTS_VALU
  // 734 per wave-tile against 130 of real work, profiles/r03_pmc_prefill_attn.txt).
  auto softmax = [&](int j) {
    const int kv0 = kv_begin + 64 * j;
    // every key of the tile visible to every query of the wave -> no per-element mask work (wave-uniform; the tile range
    // [j_int_lo, j_int_hi] is computed once per workgroup: two scalar compares per tile)
    const bool interior = j >= j_int_lo && j <= j_int_hi;
#ifdef P3V_PP_VALUPRIO
    __builtin_amdgcn_s_setprio(2);
#endif
    issue_at(2 * j + 1);                                     // (DV) this wave's pieces of DMA batch j + 1 (later in the phase: no gain / -4 %)
    PP_S(0);
#if !P3V_PP_V_IN_MATRIX
    load_v(j, 0);                                            // first half of V^T(j): lands under the VALU work below (the second
#endif
                                                             // half is read at the top of the matrix phase that consumes it: the
                                                             // VALU phase is the longer of the two)
    float m_t[2];
    if (!PRE) {
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
          for (int r = 0; r < 4; ++r) s[u][st][r] = fmaf(s[u][st][r], sc2, -m_run[u]);
    }
    if (!interior) {
      const float ninf = -INFINITY;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int t = kv0 + 32 * (st >> 1) + 8 * g + 4 * (st & 1) + r;      // key order of the staged tile
            const bool vis = t < kv_end && t >= pad && (!p.causal || t <= qpos[u]) && qpos[u] >= pad;
            const unsigned long long vm = __builtin_amdgcn_ballot_w64(vis);
            asm("v_cndmask_b32_e64 %0, %1, %0, %2" : "+v"(s[u][st][r]) : "v"(ninf), "s"(vm));      // s = vis ? s : -inf
          }
    }
    // (both 16-query halves in ONE basic block: their reduction chains are dependent instruction by instruction, the
    //  scheduler interleaves the two)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#ifdef P3V_PP_NOMAX
      m_t[u] = s[u][0][0];
      continue;
#endif
      float a = fmaxf(fmaxf(s[u][0][0], s[u][0][1]), s[u][0][2]);      // v_max3 chains
      float c = fmaxf(fmaxf(s[u][0][3], s[u][1][0]), s[u][1][1]);
      a = fmaxf(fmaxf(a, s[u][1][2]), s[u][1][3]);
      c = fmaxf(fmaxf(c, s[u][2][0]), s[u][2][1]);
      a = fmaxf(fmaxf(a, s[u][2][2]), s[u][2][3]);
      c = fmaxf(fmaxf(c, s[u][3][0]), s[u][3][1]);
      a = fmaxf(fmaxf(a, s[u][3][2]), s[u][3][3]);
      m_t[u] = rows_max(fmaxf(a, c));
    }
#ifdef P3V_PP_NOMAX                                              // timing experiment: no reduction, no decision (first tile only)
    const bool slow = unset[0] || unset[1];
#else
    const bool slow = unset[0] || unset[1] || m_t[0] > THR || m_t[1] > THR;
#endif
    PP_S(1);
    if (__builtin_amdgcn_ballot_w64(slow) != 0) {               // wave-uniform: a reference moves (first tile, or a jump > 2^8)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bool masked = m_t[u] == -INFINITY;
        const float delta = unset[u] ? (masked ? 0.f : m_t[u]) : fmaxf(m_t[u], 0.f);
        const float alpha = unset[u] ? 1.f : __builtin_amdgcn_exp2f(-delta);
        unset[u] = unset[u] && masked;
        m_run[u] += delta;
        if (PRE) negm[u] = (f32x4_t){-m_run[u], -m_run[u], -m_run[u], -m_run[u]};
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
          for (int r = 0; r < 4; ++r) asm("v_sub_f32 %0, %0, %1" : "+v"(s[u][st][r]) : "v"(delta));
#pragma unroll
        for (int d = 0; d < NDT; ++d)
#pragma unroll
          for (int r = 0; r < 4; ++r) asm("v_mul_f32 %0, %0, %1" : "+v"(o[u][d][r]) : "v"(alpha));
#pragma unroll
        for (int r = 0; r < 4; ++r) asm("v_mul_f32 %0, %0, %1" : "+v"(ol[u][r]) : "v"(alpha));
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int st = 0; st < 4; ++st)
#pragma unroll
#ifdef P3V_PP_NOEXP                                              // timing experiment: no transcendental (single non-packed VALU op instead)
        for (int r = 0; r < 4; ++r) asm("v_mul_f32 %0, 0.5, %0" : "+v"(s[u][st][r]));
#else
        for (int r = 0; r < 4; ++r) s[u][st][r] = __builtin_amdgcn_exp2f(s[u][st][r]);
#endif
      if (u == 1) PP_S(2);
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        u32x4_t pw;
        pw[0] = pack_bf16x2(s[u][2 * st][0], s[u][2 * st][1]);
        pw[1] = pack_bf16x2(s[u][2 * st][2], s[u][2 * st][3]);
        pw[2] = pack_bf16x2(s[u][2 * st + 1][0], s[u][2 * st + 1][1]);
        pw[3] = pack_bf16x2(s[u][2 * st + 1][2], s[u][2 * st + 1][3]);
        pf[u][st] = __builtin_bit_cast(bf16x8_t, pw);
      }
    }
    // P is USED here as far as the optimiser can tell: without this the exponentials are sunk past the step barrier (an asm
    // barrier orders memory operations only) into the matrix phase that consumes them
    asm volatile("" ::"v"(pf[0][0]), "v"(pf[0][1]), "v"(pf[1][0]), "v"(pf[1][1]));
    PP_S(3);
#ifdef P3V_PP_VALUPRIO
    __builtin_amdgcn_s_setprio(0);
#endif
  };
  auto pin_s = [&]() {                                       // likewise: the S^T MFMAs belong to the phase that issued them
    asm volatile("" ::"v"(s[0][0]), "v"(s[0][1]), "v"(s[0][2]), "v"(s[0][3]), "v"(s[1][0]), "v"(s[1][1]), "v"(s[1][2]), "v"(s[1][3]));
  };
  auto pin_o = [&]() {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      asm volatile("" ::"v"(ol[u]));
#pragma unroll
      for (int d = 0; d < NDT; ++d) asm volatile("" ::"v"(o[u][d]));
    }
  };

  // ---- the step sequence.  Global steps 0 .. 2 NT + 1, one s_barrier after each.  A wave of group g (0 = A, 1 = B) runs
  // its matrix phase M(j) = {issue DMA batch j; PV(j-1); S^T(j)} in step 2j + g and its VALU phase softmax(j) in step
  // 2j + 1 + g.  A wave works on tiles j < NTw (tiles above its diagonal are skipped; monotone in j); the steady-state loop
  // body is STRAIGHT-LINE code over the accumulators (no conditional around pv / qk / softmax: every conditional there costs
  // register copies), the edges are peeled, and a wave that is done keeps issuing its share of the DMA and the barriers.
  int step = 0;
  auto end_step = [&]() {
    // (the scheduler may move anything that is not a memory operation across an asm barrier -- it sank the whole
    //  exponential block of the softmax into the following matrix phase: fence the instruction stream as well)
    __builtin_amdgcn_sched_barrier(0);
    PP_S_FLUSH(step);
    PP_T(2 * step + 1);
    // before the barrier that ends an ODD step every wave has batch jn - 2 (tile jn: read from the next step on) in LDS
    // (group A issued it three steps ago, group B two); the batch issued since (jn - 1, if there was one: the last batch is
    // NT - 3) stays in flight
    if (step & 1) {
      const int jn = (step + 1) >> 1, newer = next_b - (jn - 1);   // batches this wave has issued beyond jn - 2
      if (newer >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NPW) : "memory");
      else if (newer == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPW) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
#ifndef P3V_PP_NOBAR                                             // (timing experiment: no step barrier)
    asm volatile("s_barrier" ::: "memory");
#endif
    ++step;
    PP_T(2 * step);
    __builtin_amdgcn_sched_barrier(0);
  };
  const int NTw = active ? max(0, min(NT, ((wave_last - kv_begin) >> 6) + 1)) : 0;
  if (NT > 0) {
    issue_batch(-2);
    issue_batch(-1);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPW) : "memory");          // batch -2 (K tile 0) has landed, batch -1 flies
    asm volatile("s_barrier" ::: "memory");
    if (grp) end_step();                                                // group B runs one step behind group A
    // M(0)
    issue_at(0);
    if (NTw > 0) {
#ifndef P3V_PP_NOPRIO
      __builtin_amdgcn_s_setprio(1);
#endif
      load_k(0);
      qk();
      pin_s();
      __builtin_amdgcn_s_setprio(0);
    }
    end_step();
    for (int j = 0; j + 1 < NTw; ++j) {
#ifndef P3V_PP_NOVALU
      softmax(j);
#endif
      end_step();
      issue_at(2 * j + 2);
#ifndef P3V_PP_NOPRIO
      __builtin_amdgcn_s_setprio(1);
#endif
      PP_S(0);
#if P3V_PP_V_IN_MATRIX
      load_v(j, 0);
#endif
      load_v(j, 1);                                                     // second half of V^T(j): under the first 12 PV MFMAs
      load_k(j + 1);                                                    // 12 ds_read_b128 in flight under the 28 PV MFMAs (reading them
      __builtin_amdgcn_sched_barrier(0);                                //  behind the first 14 instead, or raising the priority only for
      PP_S(1);                                                          //  the MFMAs: no change / -2 %)
      pv();
      PP_S(2);
      qk();
      pin_o();
      pin_s();
      PP_S(3);
      __builtin_amdgcn_s_setprio(0);
      end_step();
    }
    if (NTw > 0) {                                                      // last tile of this wave: softmax, then PV alone
#ifndef P3V_PP_NOVALU
      softmax(NTw - 1);
#endif
      end_step();
      issue_at(2 * NTw);
#if P3V_PP_V_IN_MATRIX
      load_v(NTw - 1, 0);
#endif
      load_v(NTw - 1, 1);
      pv();
      pin_o();
      end_step();
    }
    while (step <= 2 * NT + 1) {                                        // done (or never had rows): DMA share + barriers only
      const int ls = step - grp;
      if (ls >= 0) issue_at(ls);
      end_step();
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const float l_fin[2] = {rows_sum(ol[0][0]), rows_sum(ol[1][0])};   // the sum sits in the g = 0 lane of the query's column (all lanes take part)
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (!qvalid[u]) continue;
    const bool ok = l_fin[u] > 0.f;                                  // a query that is itself padding: 0 (Q7)
    const float inv = ok ? 1.f / l_fin[u] : 0.f;
    bf16_t* op = p.out + ((size_t)b * p.L + (q0 + u * 16 + qi)) * (size_t)(p.nh * HD) + head * HD + 4 * g;
#pragma unroll
    for (int d = 0; d < NDT; ++d) {
      u32x2_t w;
      w[0] = ok ? pack_bf16x2(o[u][d][0] * inv, o[u][d][1] * inv) : 0u;
      w[1] = ok ? pack_bf16x2(o[u][d][2] * inv, o[u][d][3] * inv) : 0u;
      *(u32x2_t*)(op + 16 * d) = w;
    }
  }
}

// Which prompt-sized kernel (measured, 32 heads x 96, causal, random data; profiles/r03_attn_prefill_kernels.txt; the table the
// route's rules come from sits at the rules, in prompt_route):
//   dma (128 queries, 4 waves, two workgroups per CU): every plain-Q call (the ViT, cached calls) below 3072 tokens, pre-scaled
//       prompts of several rows up to ~3500 tokens -- since it got the deferred-reference softmax: 946 TF/s at 8k (round 2: 606-623);
//   il  (interleaved; 128 or 256 queries): pre-scaled prompts -- ONE row from 768 tokens, several rows from 3584, everything from 6144;
//   pp  (ping-pong, 256 queries): what is left for it -- plain Q or head dim 64 from 3072 tokens.
#include "p3v_attn_il.h"
constexpr int P3V_ATTN_PP_MIN_L = 3072;                          // tools/attn_short_probe.py: dma / pp 65.2 / 67.5 us at 2531, 82.3 / 79.0 at 3072

// Every instantiation p3v_attention can launch, [kernel][hd == 64][q_prescaled], with its name as a profiler prints it (all take AttnP)
struct PromptKernel { const void* fn; const char* name; };
#define PK(f, ...) {(const void*)f<__VA_ARGS__>, #f "<" #__VA_ARGS__ ">"}
static const PromptKernel prompt_kernels[P3V_ATTN_PK_COUNT][2][2] = {
    {{PK(k_attn, 96), PK(k_attn, 96)}, {PK(k_attn, 64), PK(k_attn, 64)}},
    {{PK(k_attn_prefill, 96), PK(k_attn_prefill, 96)}, {PK(k_attn_prefill, 64), PK(k_attn_prefill, 64)}},
    {{PK(k_attn_prefill_dma, 96, false), PK(k_attn_prefill_dma, 96, true)}, {PK(k_attn_prefill_dma, 64, false), PK(k_attn_prefill_dma, 64, true)}},
    {{PK(k_attn_prefill_pp, 96, false), PK(k_attn_prefill_pp, 96, true)}, {PK(k_attn_prefill_pp, 64, false), PK(k_attn_prefill_pp, 64, true)}},
    {{PK(k_attn_prefill_il, 96, 4), PK(k_attn_prefill_il, 96, 4)}, {PK(k_attn_prefill_il, 64, 4), PK(k_attn_prefill_il, 64, 4)}},
    {{PK(k_attn_prefill_il, 96, 8), PK(k_attn_prefill_il, 96, 8)}, {PK(k_attn_prefill_il, 64, 8), PK(k_attn_prefill_il, 64, 8)}},
};
#undef PK

// The prompt attention's route (host): every rule that decides what a p3v_attention call launches, stated ONCE -- for p3v_attention
// and for p3v_attention_route.  `status` is what p3v_attention returns for the fields the query carries.
static void prompt_route(const p3v_attn_prompt_query_t& q, p3v_attn_prompt_route_t* r) {
  const P3vTuning& t = p3v_tuning();
  const auto knob = [](int asked, int lib) { return asked < 0 ? lib : asked; };
  *r = {P3V_OK, P3V_ATTN_PK_NONE, {0, 0, 0}, 0, 0, 0, 0, 0, 0, "", ""};
  const auto refuse = [&](int status) { r->status = status; };
  const auto kernel = [&](int k, int gx, int gy, int block, int lds) {
    r->kernel = k, r->grid[0] = gx, r->grid[1] = gy, r->grid[2] = q.B, r->block = block, r->lds_bytes = lds;
    r->kernel_name = prompt_kernels[k][q.hd == 64][q.q_prescaled != 0].name;
  };
  if (q.hd != 64 && q.hd != 96) return refuse(P3V_ERR_UNSUPPORTED);
  if (q.B < 0 || q.L < 0 || q.n_heads <= 0 || q.n_kv <= 0 || q.n_heads % q.n_kv) return refuse(P3V_ERR_ARG);
  if (q.B * q.L == 0) return;
  const int HD = q.hd, nh = q.n_heads;
  // L <= P3V_DECODE_MAX_L: 64 queries per workgroup, and with n_split > 1 the KV range split across workgroups + the merge launch
  const bool split = q.L <= P3V_DECODE_MAX_L && q.n_split > 1;
  if (split && !q.has_ws) return refuse(P3V_ERR_ARG);
  if (q.L <= P3V_DECODE_MAX_L || knob(q.attn_old, t.attn_old)) {
    kernel(P3V_ATTN_PK_ATTN, split ? q.n_split : p3v_cdiv(q.L, 64), nh, 256, 0);
    if (split)
      r->merge = 1, r->merge_grid = q.B * nh * q.L, r->merge_block = combine_threads(q.n_split, knob(q.combine_g, t.combine_g)), r->merge_name = "k_attn_combine2";
    return;
  }
  if (!(q.new_is_cache && q.past_t % 64 == 0 && !knob(q.attn_no_dma, t.attn_no_dma)))      // (the LDS-DMA kernels: every caller in the model)
    return kernel(P3V_ATTN_PK_PREFILL, p3v_cdiv(q.L, 128), nh, 256, 2 * (64 * (HD * 2 + 16) + HD * (64 * 2 + 16)));
  const size_t kv_bytes = (size_t)(q.past + q.L) * HD * 4;       // one head's K + V^T
  r->head_group = kv_bytes * nh <= (64u << 20) ? nh : (nh % 8 == 0 && kv_bytes * 8 <= (128u << 20) ? 8 : (nh % 4 == 0 ? 4 : nh));
  const int pp = knob(q.attn_pp, t.attn_pp);                     // -1: by shape; 0 / 1: pin (kernel tests run both)
  const int il = knob(q.attn_il, t.attn_il);                     // the interleaved kernel (pre-scaled Q only)
  // Which kernel for a pre-scaled prompt (tools/attn_il4_probe.py, 32 heads x 96, causal, us; dma / il 4 waves / il 8 waves):
  //   B = 1:  512: 15.9 / 16.4 / 22.2   768: 21.1 / 20.1 / 26.6   1280: 32.3 / 27.1 / 34.8   2531: 64.6 / 52.6 / 58.8
  //           3072: 81.4 / 74.6 / 69.5   4096: 119 / 114 / 108    8192: 436 / 403 / 377
  //   B = 2:  1280: 40.0 / 36.5 / 40.3   2531: 91.8 / 99.8 / 106   4096: 221 / 219 / 228   5120: 343 / 320 / 328
  //   B = 4:  2531: 168 / 183 / 190      3072: 252 / 254 / 271   4096: 426 / 410 / 418   6144: 939 / 886 / 893   8192: 1614 / 1504 / 1477
  //   B = 8:  1280: 112 / 127 / 142      2531: 385 / 396 / 414
  // -> long prompts: 256-query workgroups (half the L2 -> LDS bytes per flop); ONE row of a few thousand tokens: 128-query
  //    workgroups of the interleaved kernel (best balance, two workgroups per CU); several rows: the 128-query kernel up to ~3500 tokens.
  const bool il_auto = q.L >= 6144 || (q.B == 1 ? q.L >= 768 : q.L >= 3584);
  if (q.q_prescaled && (il > 0 || (il < 0 && pp != 0 && il_auto))) {   // (pp = 0 pins the dma kernel)
    // 128-query workgroups (two per CU) while 256-query ones would leave the launch bounded by its longest block
    const int nw = knob(q.attn_il_waves, t.attn_il_waves);
    const bool small = nw == 4 || (nw < 0 && q.L < (q.B == 1 ? 2816 : 6144));
    return kernel(small ? P3V_ATTN_PK_IL4 : P3V_ATTN_PK_IL8, nh * p3v_cdiv(q.L, small ? 128 : 256), 1, small ? 256 : 512, 3 * 64 * HD * 2 + 3 * HD * 128);
  }
  if (pp > 0 || (pp < 0 && q.L >= P3V_ATTN_PP_MIN_L && (q.q_prescaled || HD == 64)))   // (<96, plain>: 5 spilled registers, tests only)
    return kernel(P3V_ATTN_PK_PP, nh * p3v_cdiv(q.L, 256), 1, 512,
                  (P3V_PP_DMA_IN_VALU ? 4 : 3) * 64 * HD * 2 + (P3V_PP_DMA_IN_VALU ? 5 : 4) * HD * 128);   // K ring + V^T ring (issue_batch)
  kernel(P3V_ATTN_PK_DMA, nh * p3v_cdiv(q.L, 128), 1, 256, 2 * (64 * HD * 2 + HD * 128));
}

extern "C" int p3v_attention_route(const p3v_attn_prompt_query_t* query, p3v_attn_prompt_route_t* route) {
  if (!query || !route) return P3V_ERR_ARG;
  prompt_route(*query, route);
  return P3V_OK;
}

// The launch the route names.  A kernel's dynamic-LDS limit is raised before its first launch, once per process.
static int launch_prompt_kernel(const p3v_attn_prompt_route_t& r, int hd64, AttnP& p, hipStream_t s) {
  const PromptKernel& k = prompt_kernels[r.kernel][hd64][p.q_prescaled];
  static bool lds_raised[P3V_ATTN_PK_COUNT][2][2];
  void* args[] = {&p};
  return p3v_launch(k.fn, lds_raised[r.kernel][hd64][p.q_prescaled], r.lds_bytes, dim3(r.grid[0], r.grid[1], r.grid[2]), dim3(r.block), args, r.lds_bytes, s);
}

extern "C" int64_t p3v_attention_ws_bytes(int B, int L, int n_heads, int hd, int n_split) {
  if (L > P3V_DECODE_MAX_L || n_split < 1) return 0;
  return (int64_t)B * n_heads * n_split * 16 * (hd + 2) * 4;
}

extern "C" int p3v_attention(const p3v_attn_args_t* a, void* stream) {
  if (!a || !a->q || !a->out) return P3V_ERR_ARG;
  if (a->new_is_cache ? (!a->k_past || !a->v_past) : (!a->k_new || !a->v_new)) return P3V_ERR_ARG;
  p3v_attn_prompt_route_t r;
  prompt_route({a->B, a->L, a->n_heads, a->n_kv, a->hd, a->past, a->past_t, a->n_split, a->new_is_cache, a->q_prescaled, a->ws != nullptr,
                -1, -1, -1, -1, -1, -1}, &r);
  if (r.status != P3V_OK) return r.status;
  if ((a->past > 0 || a->d_past) && (!a->k_past || !a->v_past)) return P3V_ERR_ARG;
  if (r.kernel == P3V_ATTN_PK_NONE) return P3V_OK;               // B * L == 0
  AttnP p;
  p.q = a->q; p.k_past = a->k_past ? a->k_past : a->k_new; p.v_past = a->v_past ? a->v_past : a->v_new;
  p.k_new = a->new_is_cache ? a->k_past : a->k_new; p.v_new = a->new_is_cache ? a->v_past : a->v_new; p.new_is_cache = a->new_is_cache;
  p.out = a->out; p.pad_len = a->pad_len; p.d_past = a->d_past; p.ws = a->ws;
  p.B = a->B; p.L = a->L; p.nh = a->n_heads; p.nkv = a->n_kv; p.past = a->past; p.past_t = a->past_t;
  p.past_div = a->past_div > 0 ? a->past_div : 1; p.new_t = a->new_t; p.pad_div = a->pad_div > 0 ? a->pad_div : 1;
  p.causal = a->causal; p.scale = a->scale;
  p.q_prescaled = a->q_prescaled != 0;
  p.sc2 = p.q_prescaled ? 1.f : a->scale * 1.4426950408889634f;
  p.split_mode = r.merge;
  p.n_split = r.merge ? a->n_split : 1;
  p.head_group = r.head_group;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_prompt_kernel(r, a->hd == 64, p, s)) return rc;
  if (r.merge) {
    hipLaunchKernelGGL(k_attn_combine2, dim3(r.merge_grid), dim3(r.merge_block), 0, s, a->ws, a->out, a->L, a->n_heads, a->hd, p.n_split);
    P3V_CHECK_LAUNCH();
  }
  return P3V_OK;
}
