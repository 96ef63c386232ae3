// Guided decoding: a byte-level DFA per row, walked on the device over every token's byte string; the rule is written out above
// p3v_guide_row_t in include/p3v.h.  ONE workgroup of 1024 threads per row, so the row's state update cannot race its readers:
// every thread reads the record, the row's live delta rows (states 1..S, at most 255 x 256 entries) are staged into LDS as ONE
// BYTE per entry (a state fits a byte; an entry above S is stored as 0, the dead state) -- at most 65,280 bytes, so the full guide
// fits the 64 KB a workgroup may declare and every step of a walk is one LDS read instead of a trip to L2 --, a barrier, every
// thread walks the fed token (the same bytes in every lane: broadcast loads), thread 0 stores the new state, and the threads walk
// their share of the vocabulary: 8 tokens per thread and pass, 1024 apart, so a wave's offset loads, first-byte loads and -inf
// stores are consecutive, and the 8 tokens' loads are in flight together.  A walk ends at the first dead state: under a narrow
// guide most tokens cost one LDS read.  A row that is DONE on entry stages nothing.
// Only banned positions are stored to (2-byte stores): an allowed position keeps its bits, NaN payloads included.
#include "p3v_common.h"

#define P3V_GUIDE_THREADS 1024
#define P3V_GUIDE_PER_PASS 8
#define P3V_GUIDE_NEG_INF ((bf16_t)0xFF80u)

__global__ void __launch_bounds__(P3V_GUIDE_THREADS) k_guide_mask(bf16_t* __restrict__ logits, int64_t row_stride,
                                                                  p3v_guide_row_t* __restrict__ recs,
                                                                  const uint16_t* __restrict__ delta,
                                                                  const uint8_t* __restrict__ accept,
                                                                  const uint32_t* __restrict__ tok_off,
                                                                  const uint8_t* __restrict__ tok_bytes, uint32_t n_bytes,
                                                                  const int32_t* __restrict__ fed, int eos, int n) {
  __shared__ __attribute__((aligned(16))) uint8_t dl[P3V_GUIDE_MAX_STATES * 256];             // dl[(s - 1) * 256 + b] = delta[s][b], states 1..S
  const size_t r = blockIdx.x;
  const int tid = threadIdx.x;
  const p3v_guide_row_t rec = recs[r];
  if (!(rec.flags & P3V_GUIDE_ACTIVE)) return;                    // 0. (uniform over the workgroup)
  const int S = rec.n_states;
  const bool good = S >= 1 && S <= P3V_GUIDE_MAX_STATES && (rec.state == P3V_GUIDE_DONE || (rec.state >= 1 && rec.state <= S));
  bf16_t* __restrict__ row = logits + r * row_stride;
  int cur = good ? rec.state : P3V_GUIDE_DONE;                    // 4. a record out of range: DONE, and never written
  if (cur != P3V_GUIDE_DONE) {
    const uint16_t* __restrict__ src = delta + r * (size_t)(256 * 256) + 256;   // state 1's row (16-byte aligned: the launcher checks)
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
    __syncthreads();                                              // every thread has read the record; the table is staged
    if (fed != nullptr) {                                         // 1. the token this step was fed, before masking
      const int f = fed[r];
      int next = cur;
      if (f == eos) {
        next = P3V_GUIDE_DONE;
      } else if (f >= 0 && f < n) {
        uint32_t b0 = tok_off[f], b1 = tok_off[f + 1];
        if (b1 > n_bytes || b0 > b1) b0 = b1 = 0;
        for (uint32_t p = b0; p < b1 && next != 0; ++p) next = dl[(next - 1) * 256 + tok_bytes[p]];
      }
      if (tid == 0 && next != cur) recs[r].state = next;
      cur = (next >= 1) ? next : P3V_GUIDE_DONE;                  // (a dead end counts as DONE: only EOS is left)
    }
  }
  const bool done = cur == P3V_GUIDE_DONE;
  const bool eos_ok = done || accept[r * 256 + cur] != 0;         // 2. EOS
  const uint8_t* __restrict__ st0 = dl + (done ? 0 : (cur - 1) * 256);
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
        int s = st0[c[j]];
        for (uint32_t p = b0[j] + 1; p < b1[j] && s != 0; ++p) s = dl[(s - 1) * 256 + tok_bytes[p]];
        ok = s != 0;
      }
      if (!ok) row[i] = P3V_GUIDE_NEG_INF;                        // 3.
    }
  }
}

extern "C" int p3v_guide_mask(uint16_t* logits, int64_t row_stride, p3v_guide_row_t* rows_state, const uint16_t* delta,
                              const uint8_t* accept, const uint32_t* tok_off, const uint8_t* tok_bytes, int64_t n_bytes,
                              const int32_t* fed, int eos, int rows, int n, void* stream) {
  if (!logits || !rows_state || !delta || !accept || !tok_off || !tok_bytes || rows < 1 || rows > 65535 || n < 1 || row_stride < n ||
      n_bytes < 0 || n_bytes > 0xffffffffLL || (((size_t)delta) & 15) != 0)
    return P3V_ERR_ARG;
  hipLaunchKernelGGL(k_guide_mask, dim3(rows), dim3(P3V_GUIDE_THREADS), 0, (hipStream_t)stream, logits, row_stride, rows_state, delta,
                     accept, tok_off, tok_bytes, (uint32_t)n_bytes, fed, eos, n);
  P3V_CHECK_LAUNCH();
  return P3V_OK;
}
