// Guided decoding: a byte-level DFA per row, walked on the device over every token's byte string; the rule is written out above
// p3v_guide_row_t in include/p3v.h.  ONE workgroup of 1024 threads per row, so the row's state update cannot race its readers:
// every thread reads the record, the row's live table is staged into LDS, a barrier, every thread walks the fed token (the same
// bytes in every lane: broadcast loads), thread 0 stores the new state, and the threads walk their share of the vocabulary: 8
// tokens per thread and pass, 1024 apart, so a wave's offset loads, first-byte loads and -inf stores are consecutive, and the 8
// tokens' loads are in flight together.  A walk ends at the first dead state: under a narrow guide most tokens cost one LDS read.
// A row that is DONE on entry stages nothing.
// A NARROW row (S <= 255): its delta rows (states 1..S, at most 255 x 256 entries) are staged as ONE BYTE per entry (a state fits
// a byte; an entry above S is stored as 0, the dead state) -- at most 65,280 bytes; every step of a walk is one LDS read.
// A WIDE row (P3V_GUIDE_WIDE): its class-compressed table, rows 0..S of `pitch` uint16 entries, is staged as it lies in the row's
// region -- a flat copy of at most 131,072 bytes, an entry above S stored as 0 -- and the byte-to-class map behind it (256 bytes);
// every step of a walk is two LDS reads, cls[byte] and the entry.  The pitch is odd wherever the region has room for it, so lanes
// that sit in different states on one class spread over the banks instead of piling up on one.
// Both forms share ONE kernel and one launch (the branch is uniform over the workgroup) and one dynamic LDS allocation of 131,328
// bytes, above the 64 KB a kernel may declare statically: the launcher opts in once.
// Only banned positions are stored to (2-byte stores): an allowed position keeps its bits, NaN payloads included.
#include "p3v_common.h"

#define P3V_GUIDE_THREADS 1024
#define P3V_GUIDE_PER_PASS 8
#define P3V_GUIDE_NEG_INF ((bf16_t)0xFF80u)
#define P3V_GUIDE_LDS_TABLE (P3V_GUIDE_WIDE_MAX_ENTRIES * 2)      // the wide table; the narrow one (65,280 bytes) lies in the same bytes
#define P3V_GUIDE_LDS_BYTES (P3V_GUIDE_LDS_TABLE + 256)           // ... and the wide form's byte-to-class map behind it

extern __shared__ __attribute__((aligned(16))) uint8_t guide_lds[];

// The pitch of a wide table (include/p3v.h): C + 1 columns, padded to an odd count where rows 0..S still fit the region.
__device__ __forceinline__ int guide_wide_pitch(int S, int C) {
  const int odd = (C + 1) | 1;
  return (S + 1) * odd <= P3V_GUIDE_WIDE_MAX_ENTRIES ? odd : C + 1;
}

// One link of a walk from a live state s (1..S) on byte b -> the next state, 0 = dead.
template <bool WIDE>
__device__ __forceinline__ int guide_link(const uint8_t* dl, int s, uint32_t b, int pitch, int C) {
  if constexpr (WIDE) {
    const int c = dl[P3V_GUIDE_LDS_TABLE + b];                    // the byte's class, 0..C-1; anything else is dead
    return c < C ? (int)((const uint16_t*)dl)[s * pitch + 1 + c] : 0;
  } else {
    return dl[(s - 1) * 256 + b];
  }
}

// Two uint16 entries in one word, each above S replaced by 0.
__device__ __forceinline__ uint32_t guide_clamp2(uint32_t w, uint32_t S) {
  const uint32_t a = w & 0xffffu, b = w >> 16;
  return (a <= S ? a : 0u) | ((b <= S ? b : 0u) << 16);
}

template <bool WIDE>
__device__ __forceinline__ void guide_row(bf16_t* __restrict__ row, p3v_guide_row_t* __restrict__ recp, const p3v_guide_row_t rec,
                                          const uint16_t* __restrict__ delta, const uint8_t* __restrict__ accept,
                                          const uint32_t* __restrict__ tok_off, const uint8_t* __restrict__ tok_bytes, uint32_t n_bytes,
                                          const int32_t* __restrict__ fedp, int eos, int n) {
  uint8_t* dl = guide_lds;                                        // narrow: dl[(s - 1) * 256 + b] = delta[s][b], states 1..S
  const int tid = threadIdx.x;
  const int S = rec.n_states;
  const int C = WIDE ? rec.reserved : 0;
  bool good = S >= 1 && (rec.state == P3V_GUIDE_DONE || (rec.state >= 1 && rec.state <= S));
  if constexpr (WIDE)                                             // (S and C are bounded before they are multiplied)
    good = good && S < P3V_GUIDE_WIDE_MAX_ENTRIES && C >= 1 && C <= 256 && (S + 1) * (C + 1) <= P3V_GUIDE_WIDE_MAX_ENTRIES;
  else
    good = good && S <= P3V_GUIDE_MAX_STATES;
  const int pitch = WIDE && good ? guide_wide_pitch(S, C) : 0;
  int cur = good ? rec.state : P3V_GUIDE_DONE;                    // 4. a record out of range: DONE, and never written
  if (cur != P3V_GUIDE_DONE) {
    if constexpr (WIDE) {
      // rows 0..S as they lie in the region, 8 entries per load; the last load may run past row S, never past the region
      // ((S + 1) * pitch <= 65,536, a multiple of 8)
      const int total = (S + 1) * pitch;
      for (int e = tid * 8; e < total; e += P3V_GUIDE_THREADS * 8) {
        const u32x4_t w = *(const u32x4_t*)(delta + e);
        const u32x4_t o = {guide_clamp2(w[0], (uint32_t)S), guide_clamp2(w[1], (uint32_t)S), guide_clamp2(w[2], (uint32_t)S),
                           guide_clamp2(w[3], (uint32_t)S)};
        *(u32x4_t*)(dl + (size_t)e * 2) = o;
      }
      if (tid < 256) dl[P3V_GUIDE_LDS_TABLE + tid] = accept[tid];  // cls[256] (byte loads: `accept` promises no alignment)
    } else {
      const uint16_t* __restrict__ src = delta + 256;             // state 1's row (16-byte aligned: the launcher checks)
      for (int e = tid * 8; e < S * 256; e += P3V_GUIDE_THREADS * 8) {
        const u32x4_t w = *(const u32x4_t*)(src + e);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t a = w[k] & 0xffffu, b = w[k] >> 16;
          const uint32_t pa = a <= (uint32_t)S ? a : 0u, pb = b <= (uint32_t)S ? b : 0u;
          const uint32_t two = pa | (pb << 8);
          if (k < 2) lo |= two << (16 * k); else hi |= two << (16 * (k - 2));
        }
        const u32x2_t o = {lo, hi};
        *(u32x2_t*)(dl + e) = o;
      }
    }
    __syncthreads();                                              // every thread has read the record; the table is staged
    if (fedp != nullptr) {                                        // 1. the token this step was fed, before masking
      const int f = *fedp;
      int next = cur;
      if (f == eos) {
        next = P3V_GUIDE_DONE;
      } else if (f >= 0 && f < n) {
        uint32_t b0 = tok_off[f], b1 = tok_off[f + 1];
        if (b1 > n_bytes || b0 > b1) b0 = b1 = 0;
        for (uint32_t p = b0; p < b1 && next != 0; ++p) next = guide_link<WIDE>(dl, next, tok_bytes[p], pitch, C);
      }
      if (tid == 0 && next != cur) recp->state = next;
      cur = (next >= 1) ? next : P3V_GUIDE_DONE;                  // (a dead end counts as DONE: only EOS is left)
    }
  }
  const bool done = cur == P3V_GUIDE_DONE;
  bool eos_ok = done;                                             // 2. EOS
  if (!done) eos_ok = WIDE ? ((const uint16_t*)dl)[cur * pitch] != 0 : accept[cur] != 0;
  const int st0 = done ? 1 : cur;
  for (int64_t base = 0; base < n; base += (int64_t)P3V_GUIDE_THREADS * P3V_GUIDE_PER_PASS) {
    uint32_t b0[P3V_GUIDE_PER_PASS], b1[P3V_GUIDE_PER_PASS], c[P3V_GUIDE_PER_PASS];
#pragma unroll
    for (int j = 0; j < P3V_GUIDE_PER_PASS; ++j) {
      const int64_t i = base + (int64_t)j * P3V_GUIDE_THREADS + tid;
      const bool in = i < n && !done;
      b0[j] = in ? tok_off[i] : 0u;
      b1[j] = in ? tok_off[i + 1] : 0u;
      if (b1[j] > n_bytes || b0[j] > b1[j]) b0[j] = b1[j] = 0u;   // an offset outside the byte table: a token without bytes
    }
#pragma unroll
    for (int j = 0; j < P3V_GUIDE_PER_PASS; ++j) c[j] = b1[j] > b0[j] ? (uint32_t)tok_bytes[b0[j]] : 0u;
#pragma unroll
    for (int j = 0; j < P3V_GUIDE_PER_PASS; ++j) {
      const int64_t i = base + (int64_t)j * P3V_GUIDE_THREADS + tid;
      if (i >= n) continue;
      bool ok;
      if (i == eos) {
        ok = eos_ok;
      } else if (done || b1[j] == b0[j]) {
        ok = false;
      } else {
        int s = guide_link<WIDE>(dl, st0, c[j], pitch, C);
        for (uint32_t p = b0[j] + 1; p < b1[j] && s != 0; ++p) s = guide_link<WIDE>(dl, s, tok_bytes[p], pitch, C);
        ok = s != 0;
      }
      if (!ok) row[i] = P3V_GUIDE_NEG_INF;                        // 3.
    }
  }
}

__global__ void __launch_bounds__(P3V_GUIDE_THREADS) k_guide_mask(bf16_t* __restrict__ logits, int64_t row_stride,
                                                                  p3v_guide_row_t* __restrict__ recs,
                                                                  const uint16_t* __restrict__ delta,
                                                                  const uint8_t* __restrict__ accept,
                                                                  const uint32_t* __restrict__ tok_off,
                                                                  const uint8_t* __restrict__ tok_bytes, uint32_t n_bytes,
                                                                  const int32_t* __restrict__ fed, int eos, int n) {
  const size_t r = blockIdx.x;
  const p3v_guide_row_t rec = recs[r];
  if (!(rec.flags & P3V_GUIDE_ACTIVE)) return;                    // 0. (uniform over the workgroup)
  bf16_t* __restrict__ row = logits + r * row_stride;
  const uint16_t* __restrict__ d = delta + r * (size_t)(256 * 256);
  const uint8_t* __restrict__ a = accept + r * 256;
  const int32_t* __restrict__ f = fed != nullptr ? fed + r : nullptr;
  if (rec.flags & P3V_GUIDE_WIDE)                                 // (uniform over the workgroup as well)
    guide_row<true>(row, recs + r, rec, d, a, tok_off, tok_bytes, n_bytes, f, eos, n);
  else
    guide_row<false>(row, recs + r, rec, d, a, tok_off, tok_bytes, n_bytes, f, eos, n);
}

extern "C" int p3v_guide_mask(uint16_t* logits, int64_t row_stride, p3v_guide_row_t* rows_state, const uint16_t* delta,
                              const uint8_t* accept, const uint32_t* tok_off, const uint8_t* tok_bytes, int64_t n_bytes,
                              const int32_t* fed, int eos, int rows, int n, void* stream) {
  if (!logits || !rows_state || !delta || !accept || !tok_off || !tok_bytes || rows < 1 || rows > 65535 || n < 1 || row_stride < n ||
      n_bytes < 0 || n_bytes > 0xffffffffLL || (((size_t)delta) & 15) != 0)
    return P3V_ERR_ARG;
  static bool attr_set = false;                                   // more LDS than a kernel may declare statically: opt in once
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)k_guide_mask, hipFuncAttributeMaxDynamicSharedMemorySize, P3V_GUIDE_LDS_BYTES) != hipSuccess)
      return P3V_ERR_HIP;
    attr_set = true;
  }
  hipLaunchKernelGGL(k_guide_mask, dim3(rows), dim3(P3V_GUIDE_THREADS), P3V_GUIDE_LDS_BYTES, (hipStream_t)stream, logits, row_stride,
                     rows_state, delta, accept, tok_off, tok_bytes, (uint32_t)n_bytes, fed, eos, n);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}
