// Prompt prefix cache: move tokens [t0, t0 + n) of ONE batch row between two KV caches, all layers and kv heads in one
// launch (include/p3v.h: p3v_kv_copy).  Capture (slot / request cache -> store entry) and restore (entry -> slot) are the
// same copy with the roles swapped.
//   K    [nl, B, nkv, T, hd]: the n rows of one (layer, head) are ONE contiguous run of n * hd * es bytes on both sides, 16-byte
//        aligned (hd * es is a multiple of 16): a flat 16-byte copy.
//   V^T  [nl, B, nkv, hd, T]: hd runs of n elements per (layer, head), at element offsets t0_src / t0_dst inside rows of
//        stride T_src / T_dst.  The two byte phases are independent, so every run is cut at the DESTINATION's 16-byte grid:
//        head (< 16 bytes, element stores) | body (aligned 16-byte stores) | tail (< 16 bytes, element stores).  A body
//        chunk's source bytes sit at any element phase: they are read as the 4 or 5 ALIGNED 32-bit words that hold them
//        and shifted into place in registers.  The first / last word may reach up to 3 bytes outside the run, never
//        outside an aligned word that holds a byte of it (reads only; the allocation is a whole number of words).
//   scales [nl, B, nkv, T] fp32 (int8 cache): n floats per (layer, head), twice.
// Nothing outside the destination runs is written.
#include "p3v_common.h"

#include <string.h>
#include <type_traits>

struct kvc_args_t {
  p3v_kv_copy_job_t job[P3V_KV_COPY_MAX_JOBS];
  int nl, nkv, hd, parts;
};

template <int ES>
__global__ void __launch_bounds__(256) k_kv_copy(const kvc_args_t a) {
  const p3v_kv_copy_job_t& jb = a.job[blockIdx.z];
  const int n = jb.n_tok;
  if (n <= 0) return;
  const int unit = blockIdx.x, part = blockIdx.y, parts = a.parts, tid = threadIdx.x;
  const int l = unit / a.nkv, h = unit - l * a.nkv, hd = a.hd;
  const size_t us = ((size_t)l * jb.B_src + jb.b_src) * a.nkv + h, ud = ((size_t)l * jb.B_dst + jb.b_dst) * a.nkv + h;

  // ---- K: one aligned run
  {
    const size_t row = (size_t)hd * ES;
    const u32x4_t* s = (const u32x4_t*)((const char*)jb.k_src + (us * jb.T_src + jb.t0_src) * row);
    u32x4_t* d = (u32x4_t*)((char*)jb.k_dst + (ud * jb.T_dst + jb.t0_dst) * row);
    const int nc = (int)((size_t)n * row / 16), step = parts * 256;
    int c = part * 256 + tid;
    for (; c + 3 * step < nc; c += 4 * step) {                 // four loads in flight per lane
      const u32x4_t v0 = s[c], v1 = s[c + step], v2 = s[c + 2 * step], v3 = s[c + 3 * step];
      d[c] = v0, d[c + step] = v1, d[c + 2 * step] = v2, d[c + 3 * step] = v3;
    }
    for (; c < nc; c += step) d[c] = s[c];
  }

  // ---- scale rows of the int8 cache
  if (jb.ks_src) {
    const size_t so = us * jb.T_src + jb.t0_src, dof = ud * jb.T_dst + jb.t0_dst;
    for (int t = part * 256 + tid; t < n; t += parts * 256) {
      jb.ks_dst[dof + t] = jb.ks_src[so + t];
      jb.vs_dst[dof + t] = jb.vs_src[so + t];
    }
  }

  // ---- V^T: one wave per run
  typedef typename std::conditional<ES == 2, uint16_t, uint8_t>::type elem_t;
  const int lane = tid & 63, nbytes = n * ES;
  for (int dd = part * 4 + (tid >> 6); dd < hd; dd += parts * 4) {
    const char* S = (const char*)jb.v_src + ((us * hd + dd) * jb.T_src + jb.t0_src) * ES;
    char* D = (char*)jb.v_dst + ((ud * hd + dd) * jb.T_dst + jb.t0_dst) * ES;
    const int hb = min((int)((16 - ((uintptr_t)D & 15)) & 15), nbytes);   // bytes up to the destination's first 16-byte boundary
    const int nb = (nbytes - hb) >> 4;                         // aligned 16-byte stores
    const int tb = nbytes - hb - (nb << 4);
    const int mis = (int)((uintptr_t)(S + hb) & 3);            // wave-uniform
    const uint32_t* sw = (const uint32_t*)(S + hb - mis);
    const int sh = mis * 8;
    u32x4_t* dw = (u32x4_t*)(D + hb);
    if (sh == 0) {
      for (int j = lane; j < nb; j += 64) {
        const uint32_t* p = sw + 4 * j;
        const u32x4_t v = {p[0], p[1], p[2], p[3]};
        dw[j] = v;
      }
    } else {
      for (int j = lane; j < nb; j += 64) {
        const uint32_t* p = sw + 4 * j;
        const uint32_t w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3], w4 = p[4];
        const u32x4_t v = {(w0 >> sh) | (w1 << (32 - sh)), (w1 >> sh) | (w2 << (32 - sh)), (w2 >> sh) | (w3 << (32 - sh)),
                           (w3 >> sh) | (w4 << (32 - sh))};
        dw[j] = v;
      }
    }
    for (int e = lane * ES; e < hb + tb; e += 64 * ES) {       // head and tail: one element per lane
      const int off = e < hb ? e : e + (nb << 4);
      *(elem_t*)(D + off) = *(const elem_t*)(S + off);
    }
  }
}

static bool kvc_ranges_meet(long a0, long an, long b0, long bn) { return a0 < b0 + bn && b0 < a0 + an; }

// tensor `s` (row b_s, tokens [t0_s, +n)) against tensor `d`: true when the two runs may share bytes
static bool kvc_overlap(const void* s, long B_s, long T_s, int b_s, int t0_s, const void* d, long B_d, long T_d, int b_d, int t0_d, int n,
                        size_t per_bt /* bytes per (batch row, token) of one layer */, int nl) {
  if (!s || !d) return false;
  const uintptr_t s0 = (uintptr_t)s, s1 = s0 + (size_t)nl * B_s * T_s * per_bt;
  const uintptr_t d0 = (uintptr_t)d, d1 = d0 + (size_t)nl * B_d * T_d * per_bt;
  if (s1 <= d0 || d1 <= s0) return false;
  if (s0 != d0 || B_s != B_d || T_s != T_d) return true;       // two views of one allocation: not reasoned about, refused
  return b_s == b_d && kvc_ranges_meet(t0_s, n, t0_d, n);
}

extern "C" int p3v_kv_copy(const p3v_kv_copy_job_t* jobs, int n_jobs, int nl, int nkv, int hd, int elem_size, void* stream) {
  if (!jobs || n_jobs < 1 || n_jobs > P3V_KV_COPY_MAX_JOBS || nl <= 0 || nkv <= 0 || hd <= 0) return P3V_ERR_ARG;
  if ((elem_size != 1 && elem_size != 2) || (hd * elem_size) % 16) return P3V_ERR_ARG;
  if ((long)nl * nkv > 0x7fffffffL) return P3V_ERR_ARG;
  kvc_args_t a;
  memset(&a, 0, sizeof(a));
  int n_max = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const p3v_kv_copy_job_t& j = jobs[i];
    if (!j.k_src || !j.v_src || !j.k_dst || !j.v_dst) return P3V_ERR_ARG;
    if (((uintptr_t)j.k_src | (uintptr_t)j.k_dst) & 15) return P3V_ERR_ARG;
    if (((uintptr_t)j.v_src | (uintptr_t)j.v_dst) & (elem_size - 1)) return P3V_ERR_ARG;
    const int n_sc = !!j.ks_src + !!j.vs_src + !!j.ks_dst + !!j.vs_dst;
    if (n_sc != 0 && n_sc != 4) return P3V_ERR_ARG;
    if (n_sc && (((uintptr_t)j.ks_src | (uintptr_t)j.vs_src | (uintptr_t)j.ks_dst | (uintptr_t)j.vs_dst) & 3)) return P3V_ERR_ARG;
    if (j.B_src <= 0 || j.B_dst <= 0 || j.T_src <= 0 || j.T_dst <= 0 || j.n_tok < 0) return P3V_ERR_ARG;
    if (j.b_src < 0 || j.b_src >= j.B_src || j.b_dst < 0 || j.b_dst >= j.B_dst) return P3V_ERR_ARG;
    if (j.t0_src < 0 || j.t0_dst < 0 || (long)j.t0_src + j.n_tok > j.T_src || (long)j.t0_dst + j.n_tok > j.T_dst)
      return P3V_ERR_ARG;                                      // the run leaves its row
    const size_t kv_bt = (size_t)nkv * hd * elem_size, sc_bt = (size_t)nkv * 4;
    if (j.n_tok > 0) {
      // a job's own source against its destination, and against every other job's destination (destinations against each other too)
      for (int o = 0; o < n_jobs; ++o) {
        const p3v_kv_copy_job_t& q = jobs[o];
        if (q.n_tok <= 0) continue;
        const int n = j.n_tok > q.n_tok ? j.n_tok : q.n_tok;   // (conservative: the longer of the two runs)
        if (kvc_overlap(j.k_src, j.B_src, j.T_src, j.b_src, j.t0_src, q.k_dst, q.B_dst, q.T_dst, q.b_dst, q.t0_dst, n, kv_bt, nl) ||
            kvc_overlap(j.v_src, j.B_src, j.T_src, j.b_src, j.t0_src, q.v_dst, q.B_dst, q.T_dst, q.b_dst, q.t0_dst, n, kv_bt, nl) ||
            kvc_overlap(j.ks_src, j.B_src, j.T_src, j.b_src, j.t0_src, q.ks_dst, q.B_dst, q.T_dst, q.b_dst, q.t0_dst, n, sc_bt, nl) ||
            kvc_overlap(j.vs_src, j.B_src, j.T_src, j.b_src, j.t0_src, q.vs_dst, q.B_dst, q.T_dst, q.b_dst, q.t0_dst, n, sc_bt, nl))
          return P3V_ERR_ARG;
        if (o > i && (kvc_overlap(j.k_dst, j.B_dst, j.T_dst, j.b_dst, j.t0_dst, q.k_dst, q.B_dst, q.T_dst, q.b_dst, q.t0_dst, n, kv_bt, nl) ||
                      kvc_overlap(j.v_dst, j.B_dst, j.T_dst, j.b_dst, j.t0_dst, q.v_dst, q.B_dst, q.T_dst, q.b_dst, q.t0_dst, n, kv_bt, nl)))
          return P3V_ERR_ARG;
      }
    }
    a.job[i] = j;
    n_max = j.n_tok > n_max ? j.n_tok : n_max;
  }
  if (n_max == 0) return P3V_OK;
  a.nl = nl, a.nkv = nkv, a.hd = hd;
  // ~2048 workgroups at most, and no more parts than a (layer, head) unit has 16 KB pieces of work
  const long units = (long)nl * nkv * n_jobs, unit_bytes = 2L * n_max * hd * elem_size;
  int parts = p3v_cdiv(2048, units);
  const int by_work = p3v_cdiv(unit_bytes, 16384);
  parts = parts < by_work ? parts : by_work;
  a.parts = parts < 1 ? 1 : (parts > 24 ? 24 : parts);
  const dim3 grid(nl * nkv, a.parts, n_jobs);
  if (elem_size == 2)
    hipLaunchKernelGGL(k_kv_copy<2>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(k_kv_copy<1>, grid, dim3(256), 0, (hipStream_t)stream, a);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}
