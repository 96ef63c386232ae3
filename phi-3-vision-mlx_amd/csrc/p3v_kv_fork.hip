// n completions of one prompt: copy tokens [t0_src, t0_src + n) of ONE batch row to the same-phase columns of up to
// P3V_KV_FORK_MAX_DST rows, all layers and kv heads in one launch (include/p3v.h: p3v_kv_fork).  Every 16-byte piece of
// the source is loaded ONCE and stored n_dst times: (1 + n_dst) units of traffic where n_dst p3v_kv_copy jobs move
// 2 * n_dst.  Layouts are p3v_kv_copy's:
//   K    [nl, B, nkv, T, hd]: the n rows of one (layer, head) are one contiguous 16-byte aligned run on every side.
//   V^T  [nl, B, nkv, hd, T]: hd runs of n elements per (layer, head).  The launcher admits equal byte phase only
//        ((v_src + t0_src * es) % 16 == (v_dst + t0_dst * es) % 16, rows 16-byte multiples apart), so ONE cut serves every
//        side of a run: head (< 16 bytes, element copies) | body (aligned 16-byte loads and stores) | tail (< 16 bytes).
//        No register realignment, and the source is read inside its runs only.
//   scales [nl, B, nkv, T] fp32 (int8 cache): n floats per (layer, head), twice.
// Nothing outside the destination runs is written.
#include "p3v_common.h"

#include <string.h>
#include <type_traits>

struct kvf_args_t {
  p3v_kv_fork_t job;
  int nl, nkv, hd, parts;
};

template <int ES>
__global__ void __launch_bounds__(256) k_kv_fork(const kvf_args_t a) {
  const p3v_kv_fork_t& jb = a.job;
  const int n = jb.n_tok, m = jb.n_dst;
  const int unit = blockIdx.x, part = blockIdx.y, parts = a.parts, tid = threadIdx.x;
  const int l = unit / a.nkv, h = unit - l * a.nkv, hd = a.hd;
  const size_t us = ((size_t)l * jb.B_src + jb.b_src) * a.nkv + h;
  const size_t ud0 = (size_t)l * jb.B_dst * a.nkv + h, ud_row = (size_t)a.nkv;     // unit of destination row b: ud0 + b * ud_row

  // ---- K: one aligned run, four loads in flight per lane, each stored m times
  {
    const size_t row = (size_t)hd * ES;
    const u32x4_t* s = (const u32x4_t*)((const char*)jb.k_src + (us * jb.T_src + jb.t0_src) * row);
    const size_t dst_unit = (size_t)jb.T_dst * row;              // bytes of one (row, head) of the destination
    char* d0 = (char*)jb.k_dst + (size_t)jb.t0_dst * row;
    const int nc = (int)((size_t)n * row / 16), step = parts * 256;
    int c = part * 256 + tid;
    for (; c + 3 * step < nc; c += 4 * step) {
      const u32x4_t v0 = s[c], v1 = s[c + step], v2 = s[c + 2 * step], v3 = s[c + 3 * step];
      for (int i = 0; i < m; ++i) {
        u32x4_t* d = (u32x4_t*)(d0 + (ud0 + jb.b_dst[i] * ud_row) * dst_unit);
        d[c] = v0, d[c + step] = v1, d[c + 2 * step] = v2, d[c + 3 * step] = v3;
      }
    }
    for (; c < nc; c += step) {
      const u32x4_t v = s[c];
      for (int i = 0; i < m; ++i) ((u32x4_t*)(d0 + (ud0 + jb.b_dst[i] * ud_row) * dst_unit))[c] = v;
    }
  }

  // ---- scale rows of the int8 cache
  if (jb.ks_src) {
    const size_t so = us * jb.T_src + jb.t0_src;
    for (int t = part * 256 + tid; t < n; t += parts * 256) {
      const float ks = jb.ks_src[so + t], vs = jb.vs_src[so + t];
      for (int i = 0; i < m; ++i) {
        const size_t dof = (ud0 + jb.b_dst[i] * ud_row) * jb.T_dst + jb.t0_dst + t;
        jb.ks_dst[dof] = ks, jb.vs_dst[dof] = vs;
      }
    }
  }

  // ---- V^T: one wave per run; source and destination share the 16-byte grid
  typedef typename std::conditional<ES == 2, uint16_t, uint8_t>::type elem_t;
  const int lane = tid & 63, nbytes = n * ES;
  for (int dd = part * 4 + (tid >> 6); dd < hd; dd += parts * 4) {
    const char* S = (const char*)jb.v_src + ((us * hd + dd) * jb.T_src + jb.t0_src) * ES;
    const size_t dst_run = (size_t)jb.T_dst * ES;                // bytes of one V^T row of the destination
    char* D0 = (char*)jb.v_dst + ((size_t)dd * jb.T_dst + jb.t0_dst) * ES;           // run dd of unit 0
    const int hb = min((int)((16 - ((uintptr_t)S & 15)) & 15), nbytes);   // bytes up to the first 16-byte boundary (both sides)
    const int nb = (nbytes - hb) >> 4;                           // aligned 16-byte pieces
    const int tb = nbytes - hb - (nb << 4);
    const u32x4_t* sw = (const u32x4_t*)(S + hb);
    int j = lane;
    for (; j + 192 < nb; j += 256) {
      const u32x4_t v0 = sw[j], v1 = sw[j + 64], v2 = sw[j + 128], v3 = sw[j + 192];
      for (int i = 0; i < m; ++i) {
        u32x4_t* dw = (u32x4_t*)(D0 + (ud0 + jb.b_dst[i] * ud_row) * hd * dst_run + hb);
        dw[j] = v0, dw[j + 64] = v1, dw[j + 128] = v2, dw[j + 192] = v3;
      }
    }
    for (; j < nb; j += 64) {
      const u32x4_t v = sw[j];
      for (int i = 0; i < m; ++i) ((u32x4_t*)(D0 + (ud0 + jb.b_dst[i] * ud_row) * hd * dst_run + hb))[j] = v;
    }
    for (int e = lane * ES; e < hb + tb; e += 64 * ES) {         // head and tail: one element per lane
      const int off = e < hb ? e : e + (nb << 4);
      const elem_t v = *(const elem_t*)(S + off);
      for (int i = 0; i < m; ++i) *(elem_t*)(D0 + (ud0 + jb.b_dst[i] * ud_row) * hd * dst_run + off) = v;
    }
  }
}

// tensor `s` of the source against tensor `d` of the destination (per_bt bytes per (batch row, token) of one layer):
// 0 = two allocations, 1 = the SAME tensor (rows of one state), -1 = two different views that share memory (refused)
static int kvf_relation(const void* s, long B_s, long T_s, const void* d, long B_d, long T_d, size_t per_bt, int nl) {
  const uintptr_t s0 = (uintptr_t)s, s1 = s0 + (size_t)nl * B_s * T_s * per_bt;
  const uintptr_t d0 = (uintptr_t)d, d1 = d0 + (size_t)nl * B_d * T_d * per_bt;
  if (s1 <= d0 || d1 <= s0) return 0;
  return (s0 == d0 && B_s == B_d && T_s == T_d) ? 1 : -1;
}

extern "C" int p3v_kv_fork(const p3v_kv_fork_t* job, int nl, int nkv, int hd, int elem_size, void* stream) {
  if (!job || nl <= 0 || nkv <= 0 || hd <= 0) return P3V_ERR_ARG;
  if ((elem_size != 1 && elem_size != 2) || (hd * elem_size) % 16) return P3V_ERR_ARG;
  if ((long)nl * nkv > 0x7fffffffL) return P3V_ERR_ARG;
  const p3v_kv_fork_t& j = *job;
  if (j.n_dst < 1 || j.n_dst > P3V_KV_FORK_MAX_DST) return P3V_ERR_ARG;
  if (!j.k_src || !j.v_src || !j.k_dst || !j.v_dst) return P3V_ERR_ARG;
  if (((uintptr_t)j.k_src | (uintptr_t)j.k_dst) & 15) return P3V_ERR_ARG;
  if (((uintptr_t)j.v_src | (uintptr_t)j.v_dst) & (elem_size - 1)) return P3V_ERR_ARG;
  const int n_sc = !!j.ks_src + !!j.vs_src + !!j.ks_dst + !!j.vs_dst;
  if (n_sc != 0 && n_sc != 4) return P3V_ERR_ARG;
  if (n_sc && (((uintptr_t)j.ks_src | (uintptr_t)j.vs_src | (uintptr_t)j.ks_dst | (uintptr_t)j.vs_dst) & 3)) return P3V_ERR_ARG;
  if (j.B_src <= 0 || j.B_dst <= 0 || j.T_src <= 0 || j.T_dst <= 0 || j.n_tok < 0) return P3V_ERR_ARG;
  if (j.b_src < 0 || j.b_src >= j.B_src) return P3V_ERR_ARG;
  if (j.t0_src < 0 || j.t0_dst < 0 || (long)j.t0_src + j.n_tok > j.T_src || (long)j.t0_dst + j.n_tok > j.T_dst)
    return P3V_ERR_ARG;                                          // the run leaves its row
  for (int i = 0; i < j.n_dst; ++i) {
    if (j.b_dst[i] < 0 || j.b_dst[i] >= j.B_dst) return P3V_ERR_ARG;
    for (int o = 0; o < i; ++o)
      if (j.b_dst[o] == j.b_dst[i]) return P3V_ERR_ARG;          // two equal destination rows
  }
  // every source tensor against its destination: another allocation, or the same tensor with every destination row off b_src
  const size_t kv_bt = (size_t)nkv * hd * elem_size, sc_bt = (size_t)nkv * 4;
  const int rel[4] = {kvf_relation(j.k_src, j.B_src, j.T_src, j.k_dst, j.B_dst, j.T_dst, kv_bt, nl),
                      kvf_relation(j.v_src, j.B_src, j.T_src, j.v_dst, j.B_dst, j.T_dst, kv_bt, nl),
                      n_sc ? kvf_relation(j.ks_src, j.B_src, j.T_src, j.ks_dst, j.B_dst, j.T_dst, sc_bt, nl) : 0,
                      n_sc ? kvf_relation(j.vs_src, j.B_src, j.T_src, j.vs_dst, j.B_dst, j.T_dst, sc_bt, nl) : 0};
  for (int t = 0; t < 4; ++t) {
    if (rel[t] < 0) return P3V_ERR_ARG;
    if (rel[t] == 1)
      for (int i = 0; i < j.n_dst; ++i)
        if (j.b_dst[i] == j.b_src) return P3V_ERR_ARG;
  }
  if (j.n_tok == 0) return P3V_OK;                               // an empty job moves nothing: its phase does not matter
  // one 16-byte grid for both sides of every V^T run
  if (((long)j.T_src * elem_size) % 16 || ((long)j.T_dst * elem_size) % 16) return P3V_ERR_UNSUPPORTED;
  if ((((uintptr_t)j.v_src + (size_t)j.t0_src * elem_size) & 15) != (((uintptr_t)j.v_dst + (size_t)j.t0_dst * elem_size) & 15))
    return P3V_ERR_UNSUPPORTED;
  kvf_args_t a;
  memset(&a, 0, sizeof(a));
  a.job = j;
  a.nl = nl, a.nkv = nkv, a.hd = hd;
  // p3v_kv_copy's rule: ~2048 workgroups at most (8 of 256 threads on each of 256 CUs), and no more parts than a (layer, head)
  // unit has 16 KB pieces of SOURCE (each carries 16 KB of loads and n_dst * 16 KB of stores)
  const long units = (long)nl * nkv, unit_bytes = 2L * j.n_tok * hd * elem_size;
  int parts = p3v_cdiv(2048, units);
  const int by_work = p3v_cdiv(unit_bytes, 16384);
  parts = parts < by_work ? parts : by_work;
  a.parts = parts < 1 ? 1 : (parts > 24 ? 24 : parts);
  const dim3 grid(nl * nkv, a.parts);
  if (elem_size == 2)
    hipLaunchKernelGGL(k_kv_fork<2>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(k_kv_fork<1>, grid, dim3(256), 0, (hipStream_t)stream, a);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}
