// UTF-8 decoding and the block / device scans shared by the text kernels (csrc/fulltext.hip, csrc/wordpiece.hip, csrc/bpe.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace vrag {

__device__ __forceinline__ bool is_cont(unsigned c) { return (c & 0xC0u) == 0x80u; }

// Code point that starts at t[j] (bytes up to `hi` readable) and its length in bytes.  Well-formed UTF-8 decodes as usual.  A
// byte that cannot start a sequence is U+FFFD of one byte; a lead byte with the continuation bytes that follow it (at most as
// many as it announces) is U+FFFD when some are missing or the result is an overlong form, a surrogate or above U+10FFFF.
// U+FFFD is not alphanumeric.
__device__ __forceinline__ unsigned decode_at(const unsigned char* __restrict__ t, long long j, long long hi, int* len) {
  const unsigned c = t[j];
  *len = 1;
  if (c < 0x80u) return c;
  if (c < 0xC0u || c >= 0xF8u) return 0xFFFDu;
  int need;
  unsigned cp;
  if (c >= 0xF0u) {
    need = 3;
    cp = c & 0x07u;
  } else if (c >= 0xE0u) {
    need = 2;
    cp = c & 0x0Fu;
  } else {
    need = 1;
    cp = c & 0x1Fu;
  }
  int got = 0;
  while (got < need && j + 1 + got < hi && is_cont(t[j + 1 + got])) {
    cp = (cp << 6) | (t[j + 1 + got] & 0x3Fu);
    ++got;
  }
  *len = 1 + got;
  if (got != need) return 0xFFFDu;
  // overlong forms (C0 / C1 leads, E0 80-9F, F0 80-8F), encoded surrogates and values above U+10FFFF are not code points
  const unsigned least = need == 1 ? 0x80u : need == 2 ? 0x800u : 0x10000u;
  if (cp < least || (cp >= 0xD800u && cp <= 0xDFFFu) || cp > 0x10FFFFu) return 0xFFFDu;
  return cp;
}

// Does a code point of the text [lo, hi) start at byte i?  Every byte that is not a continuation byte does; a continuation
// byte does when the sequence of the nearest lead byte in front of it (within 3 bytes) does not reach it (U+FFFD of one byte).
__device__ __forceinline__ bool cp_start(const unsigned char* __restrict__ t, long long i, long long lo, long long hi) {
  if (!is_cont(t[i])) return true;
  for (int k = 1; k <= 3 && i - k >= lo; ++k)
    if (!is_cont(t[i - k])) {
      int len;
      (void)decode_at(t, i - k, hi, &len);
      return len <= k;
    }
  return true;
}

// Start byte of the code point that ends right before byte j (lo < j, j a code point start).
__device__ __forceinline__ long long prev_start(const unsigned char* __restrict__ t, long long j, long long lo, long long hi) {
  long long k = j - 1;
  int back = 0;
  while (k > lo && back < 3 && is_cont(t[k])) {
    --k;
    ++back;
  }
  int len;
  (void)decode_at(t, k, hi, &len);
  return k + len == j ? k : j - 1;
}

// Document of byte i: the last d with off[d] <= i (empty documents are skipped over).
__device__ __forceinline__ int doc_of(const long long* __restrict__ off, int n_docs, long long i) {
  int lo = 0, hi = n_docs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Exclusive scan of one value per thread over a 256-thread workgroup (wave prefix by shuffles, then the wave totals).
__device__ __forceinline__ unsigned block_scan_256(unsigned v, unsigned* total) {
  __shared__ unsigned wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  unsigned before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    before += w < wave ? wsum[w] : 0u;
    all += wsum[w];
  }
  __syncthreads();
  *total = all;
  return before + x - v;
}

inline unsigned grid_of(long long n, int nt) { return (unsigned)((n + nt - 1) / nt); }

// csrc/fulltext.hip.  out[0..n] = exclusive scan of in[0..n), out[n] = total; synchronises `st`.
hipError_t scan_u32(const unsigned* in, long long n, unsigned* out, hipStream_t st);
hipError_t read_u32(const unsigned* dev, unsigned* host, hipStream_t st);

}  // namespace vrag
