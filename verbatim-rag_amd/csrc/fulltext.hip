// Full-text (BM25) search on gfx950 + C ABI: the keyword method the reference runs inside Milvus
// (verbatim_rag/vector_stores/milvus_cloud.py: BM25 function over the raw `text` field, bm25_k1 = 1.2, bm25_b = 0.75;
// milvus_base.py: search_type="full_text" and the third RRF leg of the hybrid search).
//
// Everything byte- and integer-shaped runs here; the host only computes idf (float64, include/vrag_amd.h).
//   analyzer         tok_count_kernel / tok_emit_kernel: one pass over a batch of UTF-8 texts, 16 bytes per lane, a token =
//                    a maximal run of alphanumeric code points (unicode_word.inc), key = FNV-1a 64 of its lowercased UTF-8.
//                    Ingest and query batches go through the same two kernels.
//   segment build    (key, row, tf) records -> stable LSD radix sort on the key (radix_hist_kernel / radix_scatter_kernel,
//                    8 bits per pass) -> run-length encoding (rle_*): sorted unique keys, posting ranges, postings (row, tf)
//                    in row order.  Segments: main + tail; a fold re-expands segments into records and builds one again.
//   statistics       live_sum_kernel (N, sum dl over the liveness bitmap), kd_kernel (K_d per row), df_kernel (live rows per key).
//                    A shard of a row-sharded corpus is handed the corpus-wide (N, sum dl) by its caller
//                    (vrag_text_index_set_corpus_stats): kd_kernel then reads that pair instead of the shard's own.
//   search           ft_lookup_kernel (binary search of the query keys in every segment), ft_score_kernel (one workgroup per
//                    (query, 4096 rows): LDS accumulators, term after term with a barrier between terms, then the block's
//                    hits sorted in LDS), the per-query merge of csrc/topk.hip; k > 64 as exact pages of 64; its export
//                    (launch_topk_export) leaves one page as (score, global row) lists in device memory for the cross-GPU exchange.
// Integer work and fp32 scores without contraction (#pragma clang fp contract(off) below): the oracle restates them bit for bit.
#include "../../include/vrag_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "common.h"
#include "host_util.h"
#include "topk_kernels.h"
#include "utf8_text.h"

// Every fp32 operation of this file is rounded on its own: no a * b + c is fused into an FMA (HIP's default is
// -ffp-contract=fast, and the __fadd_rn / __fmul_rn helpers are plain operators compiled under it), so the host restatement
// reproduces the scores' bits.  Division is IEEE (correctly rounded fp32 division is the HIP default).
#pragma clang fp contract(off)

namespace vrag {

namespace uw {
#define UNICODE_WORD_STORAGE static __device__ const
#include "unicode_word.inc"
#undef UNICODE_WORD_STORAGE
}  // namespace uw

// ------------------------------------------------------------------------------------ analyzer
__device__ __forceinline__ bool is_alnum(unsigned cp) {
  if (cp < 0x80u) return (cp - '0' < 10u) || ((cp | 0x20u) - 'a' < 26u);
  int lo = 0, hi = VRAG_ALNUM_RANGES - 1;    // last range with start <= cp
  if (cp < uw::kAlnumRanges[0][0]) return false;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (uw::kAlnumRanges[mid][0] <= cp) lo = mid;
    else hi = mid - 1;
  }
  return cp <= uw::kAlnumRanges[lo][1];
}

__device__ __forceinline__ unsigned to_lower(unsigned cp) {
  if (cp < 0x80u) return (cp - 'A' < 26u) ? cp + 32u : cp;
  if (cp < (unsigned)uw::kLowerRuns[0][0]) return cp;
  int lo = 0, hi = VRAG_LOWER_RUNS - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((unsigned)uw::kLowerRuns[mid][0] <= cp) lo = mid;
    else hi = mid - 1;
  }
  const unsigned a = (unsigned)uw::kLowerRuns[lo][0], b = (unsigned)uw::kLowerRuns[lo][1];
  const unsigned stride = (unsigned)uw::kLowerRuns[lo][2];
  if (cp > b || (cp - a) % stride != 0u) return cp;
  return (unsigned)((int)cp + uw::kLowerRuns[lo][3]);
}

constexpr u64 kFnvBasis = 14695981039346656037ull, kFnvPrime = 1099511628211ull;
__device__ __forceinline__ u64 fnv_byte(u64 h, unsigned b) { return (h ^ (u64)b) * kFnvPrime; }
__device__ __forceinline__ u64 fnv_utf8(u64 h, unsigned cp) {
  if (cp < 0x80u) return fnv_byte(h, cp);
  if (cp < 0x800u) return fnv_byte(fnv_byte(h, 0xC0u | (cp >> 6)), 0x80u | (cp & 0x3Fu));
  if (cp < 0x10000u)
    return fnv_byte(fnv_byte(fnv_byte(h, 0xE0u | (cp >> 12)), 0x80u | ((cp >> 6) & 0x3Fu)), 0x80u | (cp & 0x3Fu));
  h = fnv_byte(h, 0xF0u | (cp >> 18));
  h = fnv_byte(h, 0x80u | ((cp >> 12) & 0x3Fu));
  h = fnv_byte(h, 0x80u | ((cp >> 6) & 0x3Fu));
  return fnv_byte(h, 0x80u | (cp & 0x3Fu));
}

// Is the code point that ends right before byte i (lo < i) alphanumeric?  The decoding of the document from `lo` puts a code
// point start at every byte that is not a continuation byte; the one before i is the nearest such byte within 3 if its
// sequence reaches exactly up to i, else byte i-1 is a stray continuation byte (U+FFFD).
__device__ __forceinline__ bool prev_alnum(const unsigned char* __restrict__ t, long long i, long long lo, long long hi) {
  long long j = i - 1;
  int back = 0;
  while (j > lo && back < 3 && is_cont(t[j])) {
    --j;
    ++back;
  }
  int len;
  const unsigned cp = decode_at(t, j, hi, &len);
  return j + len == i && is_alnum(cp);
}

__device__ __forceinline__ bool token_start(const unsigned char* __restrict__ t, long long i, long long lo, long long hi) {
  int len;
  if (!is_alnum(decode_at(t, i, hi, &len))) return false;
  return i == lo || !prev_alnum(t, i, lo, hi);
}

// Term key of the token that starts at byte i: FNV-1a 64 of the UTF-8 of its lowercased code points.
__device__ __forceinline__ u64 token_key(const unsigned char* __restrict__ t, long long i, long long hi) {
  u64 h = kFnvBasis;
  while (i < hi) {
    int len;
    const unsigned cp = decode_at(t, i, hi, &len);
    if (!is_alnum(cp)) break;
    h = fnv_utf8(h, to_lower(cp));
    i += len;
  }
  return h;
}

constexpr int TOK_NT = 256, TOK_BPT = 16;   // 4096 text bytes per workgroup

// Pass 1: tokens per workgroup of text bytes (tile_cnt) and per document (doc_cnt, atomics: the counts are exact).
__global__ __launch_bounds__(TOK_NT) void tok_count_kernel(const unsigned char* __restrict__ text, long long n_bytes,
                                                           const long long* __restrict__ off, int n_docs,
                                                           unsigned* __restrict__ tile_cnt, unsigned* __restrict__ doc_cnt) {
  const long long b0 = ((long long)blockIdx.x * TOK_NT + threadIdx.x) * TOK_BPT;
  unsigned mine = 0;
  if (b0 < n_bytes) {
    int d = doc_of(off, n_docs, b0);
    unsigned run = 0;   // tokens of document d among this lane's bytes
    for (long long i = b0; i < b0 + TOK_BPT && i < n_bytes; ++i) {
      while (off[d + 1] <= i) {
        if (run) atomicAdd(doc_cnt + d, run);
        mine += run;
        run = 0;
        ++d;
      }
      if (token_start(text, i, off[d], off[d + 1])) ++run;
    }
    if (run) atomicAdd(doc_cnt + d, run);
    mine += run;
  }
  unsigned total;
  (void)block_scan_256(mine, &total);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// Pass 2: every token's (key, row) at its position in text order (tile_off = exclusive scan of tile_cnt).
__global__ __launch_bounds__(TOK_NT) void tok_emit_kernel(const unsigned char* __restrict__ text, long long n_bytes,
                                                          const long long* __restrict__ off, int n_docs,
                                                          const unsigned* __restrict__ tile_off, unsigned row_base,
                                                          u64* __restrict__ keys, unsigned* __restrict__ rows,
                                                          unsigned* __restrict__ tfs) {
  const long long b0 = ((long long)blockIdx.x * TOK_NT + threadIdx.x) * TOK_BPT;
  unsigned mine = 0;
  int d0 = 0;
  if (b0 < n_bytes) {
    d0 = doc_of(off, n_docs, b0);
    int d = d0;
    for (long long i = b0; i < b0 + TOK_BPT && i < n_bytes; ++i) {
      while (off[d + 1] <= i) ++d;
      mine += token_start(text, i, off[d], off[d + 1]) ? 1u : 0u;
    }
  }
  unsigned total;
  unsigned pos = tile_off[blockIdx.x] + block_scan_256(mine, &total);
  if (mine == 0) return;
  int d = d0;
  for (long long i = b0; i < b0 + TOK_BPT && i < n_bytes; ++i) {
    while (off[d + 1] <= i) ++d;
    if (token_start(text, i, off[d], off[d + 1])) {
      keys[pos] = token_key(text, i, off[d + 1]);
      rows[pos] = row_base + (unsigned)d;
      if (tfs) tfs[pos] = 1u;
      ++pos;
    }
  }
}

// ------------------------------------------------------------------------------------ scans (u32, exclusive; out[n] = total)
constexpr int SCAN_NT = 256, SCAN_IPT = 16, SCAN_TILE = SCAN_NT * SCAN_IPT;

__global__ __launch_bounds__(SCAN_NT) void scan_reduce_kernel(const unsigned* __restrict__ in, long long n, unsigned* __restrict__ sums) {
  const long long base = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_IPT;
  unsigned s = 0;
  for (int j = 0; j < SCAN_IPT; ++j)
    if (base + j < n) s += in[base + j];
  unsigned total;
  (void)block_scan_256(s, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// One workgroup: exclusive scan of the tile sums in place, sums[nb] = total.
__global__ __launch_bounds__(SCAN_NT) void scan_sums_kernel(unsigned* __restrict__ sums, long long nb) {
  __shared__ unsigned carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (long long c = 0; c < nb; c += SCAN_NT) {
    const long long i = c + threadIdx.x;
    const unsigned v = i < nb ? sums[i] : 0u;
    unsigned total;
    const unsigned ex = block_scan_256(v, &total);
    const unsigned carry = carry_s;
    if (i < nb) sums[i] = carry + ex;
    __syncthreads();
    if (threadIdx.x == 0) carry_s = carry + total;
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[nb] = carry_s;
}

__global__ __launch_bounds__(SCAN_NT) void scan_down_kernel(const unsigned* __restrict__ in, long long n, const unsigned* __restrict__ sums,
                                                            long long nb, unsigned* __restrict__ out) {
  const long long base = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_IPT;
  unsigned s = 0;
  for (int j = 0; j < SCAN_IPT; ++j)
    if (base + j < n) s += in[base + j];
  unsigned total;
  unsigned run = sums[blockIdx.x] + block_scan_256(s, &total);
  for (int j = 0; j < SCAN_IPT; ++j)
    if (base + j < n) {
      const unsigned v = in[base + j];
      out[base + j] = run;
      run += v;
    }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = sums[nb];
}

// ------------------------------------------------------------------------------------ stable LSD radix sort (8-bit digits)
// Records are three arrays (key u64, row u32, tf u32).  Digit of pass `shift`: of the key (by_row = 0) or of the row.  A tile
// of 4096 records is ranked in 16 chunks of 256, in record order: within a wave by matching the digit over 8 ballots, across
// the 4 waves through per-wave digit counts in LDS -- equal digits keep their order (stable).
constexpr int RS_NT = 256, RS_IPT = 16, RS_TILE = RS_NT * RS_IPT;

__device__ __forceinline__ unsigned digit_of(const u64* __restrict__ key, const unsigned* __restrict__ row, long long i, int by_row,
                                             int shift) {
  return by_row ? (row[i] >> shift) & 255u : (unsigned)(key[i] >> shift) & 255u;
}

__global__ __launch_bounds__(RS_NT) void radix_hist_kernel(const u64* __restrict__ key, const unsigned* __restrict__ row, long long n,
                                                           int by_row, int shift, unsigned* __restrict__ hist, int n_tiles) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * RS_TILE;
  for (int c = 0; c < RS_IPT; ++c) {
    const long long i = base + (long long)c * RS_NT + threadIdx.x;
    if (i < n) atomicAdd(&h[digit_of(key, row, i, by_row, shift)], 1u);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];   // digit-major: one scan gives every (digit, tile) offset
}

__global__ __launch_bounds__(RS_NT) void radix_scatter_kernel(const u64* __restrict__ key, const unsigned* __restrict__ row,
                                                              const unsigned* __restrict__ tf, long long n, int by_row, int shift,
                                                              const unsigned* __restrict__ offs, int n_tiles, u64* __restrict__ key_o,
                                                              unsigned* __restrict__ row_o, unsigned* __restrict__ tf_o) {
  __shared__ unsigned base[256];
  __shared__ unsigned wcnt[4][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  base[tid] = offs[(size_t)tid * n_tiles + blockIdx.x];
  for (int w = 0; w < 4; ++w) wcnt[w][tid] = 0;
  __syncthreads();
  const u64 lt = (1ull << lane) - 1ull, le = (2ull << lane) - 1ull;   // lane 63: 2 << 63 wraps to 0, le = all lanes
  for (int c = 0; c < RS_IPT; ++c) {
    const long long i = (long long)blockIdx.x * RS_TILE + (long long)c * RS_NT + tid;
    const bool valid = i < n;
    const unsigned d = valid ? digit_of(key, row, i, by_row, shift) : 0u;
    u64 m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const u64 on = __ballot(bit);
      m &= bit ? on : ~on;
    }
    const unsigned rank = (unsigned)__popcll(m & lt);
    if (valid && (m & ~le) == 0ull) wcnt[wave][d] = (unsigned)__popcll(m);   // last lane of its digit group in this wave
    __syncthreads();
    if (valid) {
      unsigned pos = base[d] + rank;
      for (int w = 0; w < wave; ++w) pos += wcnt[w][d];
      key_o[pos] = key[i];
      row_o[pos] = row[i];
      tf_o[pos] = tf[i];
    }
    __syncthreads();
    base[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
    for (int w = 0; w < 4; ++w) wcnt[w][tid] = 0;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------ run-length encoding of sorted records
// pflag: a new (key, row) pair starts at i (a posting); kflag: a new key starts at i.
__global__ void rle_flags_kernel(const u64* __restrict__ key, const unsigned* __restrict__ row, long long n, unsigned* __restrict__ pflag,
                                 unsigned* __restrict__ kflag) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool kf = i == 0 || key[i] != key[i - 1];
  pflag[i] = (kf || row[i] != row[i - 1]) ? 1u : 0u;
  kflag[i] = kf ? 1u : 0u;
}

// Postings (row, first record) at their scanned positions; unique keys with their first posting.  pkey (query terms) = the key
// of every posting; tf from the record when `unit` is 0 (fold: every run is one record), else the run length (rle_tf_kernel).
__global__ void rle_scatter_kernel(const u64* __restrict__ key, const unsigned* __restrict__ row, const unsigned* __restrict__ tf,
                                   long long n, const unsigned* __restrict__ pflag, const unsigned* __restrict__ pscan,
                                   const unsigned* __restrict__ kflag, const unsigned* __restrict__ kscan, int unit,
                                   u64* __restrict__ ukeys, unsigned* __restrict__ pstart, unsigned* __restrict__ prow,
                                   unsigned* __restrict__ ptf, unsigned* __restrict__ ppos, u64* __restrict__ pkey) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !pflag[i]) return;
  const unsigned p = pscan[i];
  prow[p] = row[i];
  ppos[p] = (unsigned)i;
  if (!unit) ptf[p] = tf[i];
  if (pkey) pkey[p] = key[i];
  if (ukeys && kflag[i]) {
    ukeys[kscan[i]] = key[i];
    pstart[kscan[i]] = p;
  }
}

__global__ void rle_tf_kernel(const unsigned* __restrict__ ppos, long long n_post, long long n, unsigned* __restrict__ ptf) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n_post) ptf[p] = (unsigned)((p + 1 < n_post ? (long long)ppos[p + 1] : n) - (long long)ppos[p]);
}

// A segment's postings back into (key, row, tf) records (fold).
__global__ void expand_kernel(const u64* __restrict__ ukeys, const unsigned* __restrict__ pstart, long long n_keys,
                              const unsigned* __restrict__ prow, const unsigned* __restrict__ ptf, long long n_post,
                              u64* __restrict__ key, unsigned* __restrict__ row, unsigned* __restrict__ tf) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_post) return;
  long long lo = 0, hi = n_keys - 1;   // last key whose range starts at or before p
  while (lo < hi) {
    const long long mid = (lo + hi + 1) >> 1;
    if (pstart[mid] <= (unsigned)p) lo = mid;
    else hi = mid - 1;
  }
  key[p] = ukeys[lo];
  row[p] = prow[p];
  tf[p] = ptf[p];
}

// ------------------------------------------------------------------------------------ statistics
__device__ __forceinline__ bool bit_set(const unsigned* __restrict__ words, long long r) { return (words[r >> 5] >> (r & 31)) & 1u; }

// acc[0] += live rows, acc[1] += their token counts
__global__ __launch_bounds__(256) void live_sum_kernel(const unsigned* __restrict__ live, const unsigned* __restrict__ dl, long long n_rows,
                                                       unsigned long long* __restrict__ acc) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  unsigned long long cnt = 0, sum = 0;
  if (r < n_rows && bit_set(live, r)) {
    cnt = 1;
    sum = dl[r];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    sum += __shfl_xor(sum, o, 64);
  }
  if ((threadIdx.x & 63) == 0 && cnt) {
    atomicAdd(acc, cnt);
    atomicAdd(acc + 1, sum);
  }
}

// K_d = k1 * ((1 - b) + b * (dl / avgdl)), avgdl = fp32(sum dl / N) (a float64 division); every step one rounded fp32 operation
__global__ void kd_kernel(const unsigned* __restrict__ dl, long long n_rows, const unsigned long long* __restrict__ acc, float k1,
                          float one_minus_b, float b, float* __restrict__ kd) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const float avgdl = acc[0] ? (float)((double)acc[1] / (double)acc[0]) : 0.f;
  if (avgdl > 0.f) {
    const float t = (float)dl[r] / avgdl;
    kd[r] = k1 * (one_minus_b + b * t);
  } else {
    kd[r] = k1;   // no live row has a token: no row can be a hit
  }
}

// df[u] = live rows among key u's postings: one wave per key
__global__ __launch_bounds__(256) void df_kernel(const unsigned* __restrict__ pstart, long long n_keys, const unsigned* __restrict__ prow,
                                                 const unsigned* __restrict__ live, unsigned* __restrict__ df) {
  const int lane = threadIdx.x & 63;
  const long long waves = (long long)gridDim.x * 4;
  for (long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); u < n_keys; u += waves) {
    unsigned c = 0;
    for (unsigned p = pstart[u] + lane; p < pstart[u + 1]; p += 64) c += bit_set(live, prow[p]) ? 1u : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) df[u] = c;
  }
}

// ------------------------------------------------------------------------------------ search
constexpr int FT_MAXSEG = 4;   // segments a search reads (the index keeps at most 2: main + tail)
constexpr long long kMaxSegPostings = 0xFFFFFFF0ll;   // postings / records per segment build: u32 scans and offsets
struct FtSeg {
  const u64* keys;
  const unsigned* pstart;
  const unsigned* prow;
  const unsigned* ptf;
  const unsigned* df;
  long long n_keys, row_lo, row_hi;
};
struct FtSegs {
  FtSeg s[FT_MAXSEG];
  int n;
};

__device__ __forceinline__ long long find_key(const FtSeg& g, u64 key) {
  long long lo = 0, hi = g.n_keys;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (g.keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < g.n_keys && g.keys[lo] == key ? lo : -1;
}

// Query term j -> its key index in every segment (-1: absent), and its df over the live rows when `df_out` is given.
__global__ void ft_lookup_kernel(FtSegs segs, const u64* __restrict__ keys, long long n_terms, int* __restrict__ tu,
                                 long long* __restrict__ df_out) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_terms) return;
  long long df = 0;
  for (int s = 0; s < FT_MAXSEG; ++s) {
    long long u = -1;
    if (s < segs.n) u = find_key(segs.s[s], keys[j]);
    if (u >= 0) df += segs.s[s].df[u];
    tu[j * FT_MAXSEG + s] = (int)u;
  }
  if (df_out) df_out[j] = df;
}

constexpr int FT_ROWS = 4096, FT_NT = 512;

// first posting in [lo, hi) whose row is >= r (postings of a key are in row order)
__device__ __forceinline__ unsigned lower_row(const unsigned* __restrict__ prow, unsigned lo, unsigned hi, unsigned r) {
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    if (prow[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// One workgroup per (block of FT_ROWS rows, query).  acc[row] += w_t * (tf * (k1 + 1)) / (tf + K_d) for the query's terms in
// ascending key order, a barrier after every term (one posting per row and term: no two lanes touch one accumulator within a
// term).  Hits (score > 0, live, allowed, key below the page bound) are gathered, sorted descending in LDS and the best kk
// written to cand[block][q][kk] (0 = none).
__global__ __launch_bounds__(FT_NT) void ft_score_kernel(FtSegs segs, const long long* __restrict__ q_indptr, const int* __restrict__ tu,
                                                         const float* __restrict__ w, const float* __restrict__ kd,
                                                         const unsigned* __restrict__ live, const unsigned* __restrict__ allow,
                                                         long long allow_rows, long long n_rows, float k1p1, int nq, int kk, const u64* __restrict__ bound,
                                                         u64* __restrict__ cand) {
  __shared__ float acc[FT_ROWS];
  __shared__ u64 hits[FT_ROWS];
  __shared__ unsigned n_hit;
  const int tid = threadIdx.x, q = blockIdx.y;
  const unsigned r0 = blockIdx.x * FT_ROWS;
  const unsigned r1 = (unsigned)min((long long)r0 + FT_ROWS, n_rows);
  u64* out = cand + ((size_t)blockIdx.x * nq + q) * kk;
  for (int i = tid; i < FT_ROWS; i += FT_NT) acc[i] = 0.f;
  if (tid == 0) n_hit = 0;
  __syncthreads();
  bool touched = false;
  const long long j0 = q_indptr[q], j1 = q_indptr[q + 1];
  for (long long j = j0; j < j1; ++j) {
    const float wt = w[j];
    for (int s = 0; s < segs.n; ++s) {
      const int u = tu[j * FT_MAXSEG + s];
      const FtSeg& g = segs.s[s];
      if (u < 0 || g.row_hi <= r0 || g.row_lo >= r1) continue;
      const unsigned a = lower_row(g.prow, g.pstart[u], g.pstart[u + 1], r0);
      const unsigned e = lower_row(g.prow, a, g.pstart[u + 1], r1);
      touched |= a < e;
      for (unsigned p = a + tid; p < e; p += FT_NT) {
        const unsigned row = g.prow[p];
        const float tf = (float)g.ptf[p];
        const float c = wt * ((tf * k1p1) / (tf + kd[row]));
        acc[row - r0] += c;
      }
    }
    __syncthreads();
  }
  if (!touched) {   // uniform: every lane ran the same searches
    for (int i = tid; i < kk; i += FT_NT) out[i] = 0ull;
    return;
  }
  const u64 bnd = bound ? bound[q] : ~0ull;
  for (unsigned i = tid; i < r1 - r0; i += FT_NT) {
    const float sc = acc[i];
    const unsigned row = r0 + i;
    if (sc > 0.f && bit_set(live, row) && (!allow || (row < allow_rows && bit_set(allow, row)))) {
      const u64 key = make_key(sc, row);
      if (key < bnd) hits[atomicAdd(&n_hit, 1u)] = key;
    }
  }
  __syncthreads();
  const unsigned m = n_hit;
  unsigned p2 = 2;
  while (p2 < m) p2 <<= 1;
  for (unsigned i = m + tid; i < p2; i += FT_NT) hits[i] = 0ull;
  __syncthreads();
  if (m > 1) {   // bitonic sort, descending
    for (unsigned size = 2; size <= p2; size <<= 1)
      for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
        for (unsigned i = tid; i < p2 / 2; i += FT_NT) {
          const unsigned lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
          const bool desc = (lo & size) == 0;
          const u64 x = hits[lo], y = hits[hi];
          if ((x < y) == desc) {
            hits[lo] = y;
            hits[hi] = x;
          }
        }
        __syncthreads();
      }
  }
  for (int i = tid; i < kk; i += FT_NT) out[i] = (unsigned)i < m ? hits[i] : 0ull;
}

// next page's bound = the last key of this page (0 when the page was not full: the next admits nothing)
__global__ void ft_bound_kernel(const u64* __restrict__ page, int nq, int kk, u64* __restrict__ bound) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < nq) bound[q] = page[(size_t)q * kk + kk - 1];
}

}  // namespace vrag

namespace vrag {

// out[0..n] = exclusive scan of in[0..n), out[n] = total.
hipError_t scan_u32(const unsigned* in, long long n, unsigned* out, hipStream_t st) {
  const long long nb = std::max<long long>(1, (n + SCAN_TILE - 1) / SCAN_TILE);
  DevBuf sums;
  hipError_t e = sums.alloc((size_t)(nb + 1) * 4);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(scan_reduce_kernel, dim3((unsigned)nb), dim3(SCAN_NT), 0, st, in, n, sums.as<unsigned>());
  hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(SCAN_NT), 0, st, sums.as<unsigned>(), nb);
  hipLaunchKernelGGL(scan_down_kernel, dim3((unsigned)nb), dim3(SCAN_NT), 0, st, in, n, sums.as<unsigned>(), nb, out);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);   // `sums` is freed on return
  return e;
}

hipError_t read_u32(const unsigned* dev, unsigned* host, hipStream_t st) {
  hipError_t e = hipMemcpyAsync(host, dev, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e;
}

}  // namespace vrag

using namespace vrag;

namespace {

struct Segment {
  long long row_lo = 0, n_rows = 0, n_keys = 0, n_post = 0;
  DevBuf keys, pstart, prow, ptf, df;
};

// (key, row, tf) records on the device
struct Records {
  long long n = 0;
  DevBuf key, row, tf;
  hipError_t alloc(long long m) {
    n = m;
    hipError_t e = key.alloc((size_t)m * 8);
    if (e == hipSuccess) e = row.alloc((size_t)m * 4);
    if (e == hipSuccess) e = tf.alloc((size_t)m * 4);
    return e;
  }
};

// Three record arrays as raw device pointers (n elements each).
struct RecPtrs {
  u64* key;
  unsigned* row;
  unsigned* tf;
};

inline int radix_tiles(long long n) { return (int)((n + RS_TILE - 1) / RS_TILE); }

// The digit passes of the sort on raw arrays: pass after pass from `a` into `b` and back; hist holds radix_tiles(n) * 256
// words, offs one more.  *in_b = the sorted records ended in `b` (an odd number of passes).  n <= 1: nothing is launched.
hipError_t radix_passes(RecPtrs a, RecPtrs b, long long n, int by_row, int row_bits, unsigned* hist, unsigned* offs, hipStream_t st,
                        bool* in_b) {
  *in_b = false;
  if (n <= 1) return hipSuccess;
  const int n_tiles = radix_tiles(n);
  hipError_t e;
  const int bits = by_row ? row_bits : 64;
  for (int shift = 0; shift < bits; shift += 8) {
    hipLaunchKernelGGL(radix_hist_kernel, dim3(n_tiles), dim3(RS_NT), 0, st, a.key, a.row, n, by_row, shift, hist, n_tiles);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = scan_u32(hist, (long long)n_tiles * 256, offs, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(n_tiles), dim3(RS_NT), 0, st, a.key, a.row, a.tf, n, by_row, shift, offs, n_tiles,
                       b.key, b.row, b.tf);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    std::swap(a, b);
    *in_b = !*in_b;
  }
  return hipStreamSynchronize(st);
}

// Stable sort of the records by key (by_row = 0: 8 passes) or by row (passes over the bits below 2^row_bits).
hipError_t radix_sort(Records& r, int by_row, int row_bits, hipStream_t st) {
  if (r.n <= 1) return hipSuccess;
  const int n_tiles = radix_tiles(r.n);
  Records tmp;
  DevBuf hist, offs;
  hipError_t e = tmp.alloc(r.n);
  if (e == hipSuccess) e = hist.alloc((size_t)n_tiles * 256 * 4);
  if (e == hipSuccess) e = offs.alloc(((size_t)n_tiles * 256 + 1) * 4);
  if (e != hipSuccess) return e;
  bool in_tmp = false;
  e = radix_passes(RecPtrs{r.key.as<u64>(), r.row.as<unsigned>(), r.tf.as<unsigned>()},
                   RecPtrs{tmp.key.as<u64>(), tmp.row.as<unsigned>(), tmp.tf.as<unsigned>()}, r.n, by_row, row_bits, hist.as<unsigned>(),
                   offs.as<unsigned>(), st, &in_tmp);
  if (in_tmp) {
    std::swap(r.key, tmp.key);
    std::swap(r.row, tmp.row);
    std::swap(r.tf, tmp.tf);
  }
  return e;
}

// Run-length encoding of records sorted by (key, row).  Segment form (seg != null): unique keys, posting ranges, postings;
// query form (pkey != null): one posting per (query, key) run with its key.
struct Runs {
  long long n_post = 0, n_keys = 0;
  DevBuf prow, ptf, pkey;
};

// The scratch of one run-length encoding of n records: flags [n] and their exclusive scans [n + 1].
struct RleScratch {
  unsigned *pflag, *kflag, *pscan, *kscan;
};

// First half on raw arrays: the flags, their scans, and the counts the outputs are sized by.
hipError_t rle_count(RecPtrs r, long long n, RleScratch s, unsigned* n_post, unsigned* n_keys, hipStream_t st) {
  hipError_t e;
  if (n) hipLaunchKernelGGL(rle_flags_kernel, dim3(grid_of(n, 256)), dim3(256), 0, st, r.key, r.row, n, s.pflag, s.kflag);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = scan_u32(s.pflag, n, s.pscan, st)) != hipSuccess) return e;
  if ((e = scan_u32(s.kflag, n, s.kscan, st)) != hipSuccess) return e;
  if ((e = read_u32(s.pscan + n, n_post, st)) != hipSuccess) return e;
  return read_u32(s.kscan + n, n_keys, st);
}

// Second half: prow, ptf, ppos [n_post]; pkey [n_post] or null; ukeys [n_keys] and pstart [n_keys + 1], both or neither.
// *n_post_p is copied to pstart[n_keys] on the stream: it must stay where it is until the caller has synchronised.
hipError_t rle_emit(RecPtrs r, long long n, RleScratch s, int unit, const unsigned* n_post_p, unsigned n_keys, u64* ukeys,
                    unsigned* pstart, unsigned* prow, unsigned* ptf, unsigned* ppos, u64* pkey, hipStream_t st) {
  const unsigned n_post = *n_post_p;
  if (n)
    hipLaunchKernelGGL(rle_scatter_kernel, dim3(grid_of(n, 256)), dim3(256), 0, st, r.key, r.row, r.tf, n, s.pflag, s.pscan, s.kflag,
                       s.kscan, unit, ukeys, pstart, prow, ptf, ppos, pkey);
  if (unit && n_post) hipLaunchKernelGGL(rle_tf_kernel, dim3(grid_of(n_post, 256)), dim3(256), 0, st, ppos, (long long)n_post, n, ptf);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && pstart) e = hipMemcpyAsync(pstart + n_keys, n_post_p, 4, hipMemcpyHostToDevice, st);
  return e;
}

hipError_t rle(const Records& r, int unit, Segment* seg, Runs* runs, hipStream_t st) {
  DevBuf pflag, kflag, pscan, kscan, ppos;
  hipError_t e = pflag.alloc((size_t)r.n * 4);
  if (e == hipSuccess) e = kflag.alloc((size_t)r.n * 4);
  if (e == hipSuccess) e = pscan.alloc((size_t)(r.n + 1) * 4);
  if (e == hipSuccess) e = kscan.alloc((size_t)(r.n + 1) * 4);
  if (e != hipSuccess) return e;
  const RecPtrs rec{r.key.as<u64>(), r.row.as<unsigned>(), r.tf.as<unsigned>()};
  const RleScratch scr{pflag.as<unsigned>(), kflag.as<unsigned>(), pscan.as<unsigned>(), kscan.as<unsigned>()};
  unsigned n_post = 0, n_keys = 0;
  if ((e = rle_count(rec, r.n, scr, &n_post, &n_keys, st)) != hipSuccess) return e;
  DevBuf prow, ptf, pkey, ukeys, pstart;
  e = prow.alloc((size_t)n_post * 4);
  if (e == hipSuccess) e = ptf.alloc((size_t)n_post * 4);
  if (e == hipSuccess) e = ppos.alloc((size_t)n_post * 4);
  if (e == hipSuccess && runs) e = pkey.alloc((size_t)n_post * 8);
  if (e == hipSuccess && seg) e = ukeys.alloc((size_t)n_keys * 8);
  if (e == hipSuccess && seg) e = pstart.alloc((size_t)(n_keys + 1) * 4);
  if (e != hipSuccess) return e;
  if ((e = rle_emit(rec, r.n, scr, unit, &n_post, n_keys, seg ? ukeys.as<u64>() : nullptr, seg ? pstart.as<unsigned>() : nullptr,
                    prow.as<unsigned>(), ptf.as<unsigned>(), ppos.as<unsigned>(), runs ? pkey.as<u64>() : nullptr, st)) != hipSuccess)
    return e;
  if (seg) {
    seg->n_keys = n_keys;
    seg->n_post = n_post;
    seg->keys = std::move(ukeys);
    seg->pstart = std::move(pstart);
    seg->prow = std::move(prow);
    seg->ptf = std::move(ptf);
    if ((e = seg->df.alloc((size_t)n_keys * 4)) != hipSuccess) return e;
  }
  if (runs) {
    runs->n_post = n_post;
    runs->n_keys = n_keys;
    runs->prow = std::move(prow);
    runs->ptf = std::move(ptf);
    runs->pkey = std::move(pkey);
  }
  return hipStreamSynchronize(st);
}

// Tokens of n_docs texts (host bytes, doc_off[0] = 0) as records (key, row_base + document, 1) in text order, plus the token
// count of every document (device, optional).
int tokenize(const uint8_t* text, const int64_t* doc_off, int n_docs, unsigned row_base, hipStream_t st, Records& rec, DevBuf* counts) {
  const long long n_bytes = doc_off[n_docs];
  const long long n_tiles = std::max<long long>(1, (n_bytes + TOK_NT * TOK_BPT - 1) / (TOK_NT * TOK_BPT));
  DevBuf d_text, d_off, tile_cnt, tile_off, doc_cnt;
  HIP_TRY(d_text.alloc((size_t)n_bytes + 16));
  HIP_TRY(d_off.alloc((size_t)(n_docs + 1) * 8));
  HIP_TRY(tile_cnt.alloc((size_t)n_tiles * 4));
  HIP_TRY(tile_off.alloc((size_t)(n_tiles + 1) * 4));
  HIP_TRY(doc_cnt.alloc((size_t)n_docs * 4));
  if (n_bytes) HIP_TRY(hipMemcpyAsync(d_text.p, text, (size_t)n_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_off.p, doc_off, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(doc_cnt.p, 0, (size_t)n_docs * 4, st));
  hipLaunchKernelGGL(tok_count_kernel, dim3((unsigned)n_tiles), dim3(TOK_NT), 0, st, d_text.as<unsigned char>(), n_bytes, d_off.as<long long>(),
                     n_docs, tile_cnt.as<unsigned>(), doc_cnt.as<unsigned>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(scan_u32(tile_cnt.as<unsigned>(), n_tiles, tile_off.as<unsigned>(), st));
  unsigned n_tok = 0;
  HIP_TRY(read_u32(tile_off.as<unsigned>() + n_tiles, &n_tok, st));
  HIP_TRY(rec.alloc(n_tok));
  if (n_tok)
    hipLaunchKernelGGL(tok_emit_kernel, dim3((unsigned)n_tiles), dim3(TOK_NT), 0, st, d_text.as<unsigned char>(), n_bytes,
                       d_off.as<long long>(), n_docs, tile_off.as<unsigned>(), row_base, rec.key.as<u64>(), rec.row.as<unsigned>(),
                       rec.tf.as<unsigned>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  if (counts) *counts = std::move(doc_cnt);
  return VRAG_OK;
}

int check_docs(const uint8_t* text, const int64_t* doc_off, int32_t n_docs) {
  ARG_CHECK(doc_off && n_docs >= 0, "bad arguments");
  ARG_CHECK(doc_off[0] == 0, "doc_off[0] must be 0");
  for (int32_t d = 0; d < n_docs; ++d) ARG_CHECK(doc_off[d + 1] >= doc_off[d], "doc_off must be non-decreasing (document %d)", d);
  ARG_CHECK(doc_off[n_docs] < 0xFFFFFFF0ll, "a batch holds at most 4 GiB of text");
  ARG_CHECK(doc_off[n_docs] == 0 || text, "null text");
  return VRAG_OK;
}

}  // namespace

struct vrag_text_index {
  int device = 0;
  float k1 = 1.2f, b = 0.75f;
  hipStream_t stream = nullptr;
  std::mutex mu;
  std::vector<Segment> segs;   // disjoint, ascending row ranges: main [+ tail]
  long long n_rows = 0;
  DevBuf dl, live, kd, acc;    // token count / liveness bit / K_d per row; acc = {N, sum dl} of this index, then the caller's pair
  size_t rows_cap = 0;
  std::vector<unsigned> h_live;   // host copy of the bitmap
  bool stats_dirty = true;
  bool kd_dirty = false;          // only K_d is stale (the corpus-wide pair changed)
  unsigned long long h_acc[2] = {0, 0};
  unsigned long long corpus[2] = {0, 0};   // vrag_text_index_set_corpus_stats: {N, sum dl} of the whole corpus, N = 0 = not set
  hipEvent_t lists_done = nullptr;   // recorded behind a device-resident search: later work on the workspace / K_d waits for it
  // search workspace
  DevBuf q_indptr, q_keys, q_w, q_tu, cand, page, bound;
  DevBuf allow;
};

namespace {

// A segment as raw device pointers.
struct SegPtrs {
  u64* keys;
  unsigned *pstart, *prow, *ptf, *df;
  long long n_keys, n_post, row_lo, n_rows;
};

SegPtrs ptrs_of(const Segment& g) {
  return SegPtrs{g.keys.as<u64>(), g.pstart.as<unsigned>(), g.prow.as<unsigned>(), g.ptf.as<unsigned>(), g.df.as<unsigned>(),
                 g.n_keys, g.n_post, g.row_lo, g.n_rows};
}

FtSegs seg_view(const SegPtrs* segs, int n) {
  FtSegs v{};
  v.n = n;
  for (int s = 0; s < n; ++s) {
    const SegPtrs& g = segs[s];
    v.s[s] = FtSeg{g.keys, g.pstart, g.prow, g.ptf, g.df, g.n_keys, g.row_lo, g.row_lo + g.n_rows};
  }
  return v;
}

FtSegs seg_view(const vrag_text_index* ix) {
  SegPtrs p[FT_MAXSEG];
  const int n = (int)ix->segs.size();
  for (int s = 0; s < n; ++s) p[s] = ptrs_of(ix->segs[s]);
  return seg_view(p, n);
}

// Segment of the sorted records (records sorted by key, rows ascending within a key).
int build_segment(Records& rec, int unit, long long row_lo, long long n_rows, hipStream_t st, Segment& seg) {
  HIP_TRY(radix_sort(rec, 0, 0, st));
  seg.row_lo = row_lo;
  seg.n_rows = n_rows;
  HIP_TRY(rle(rec, unit, &seg, nullptr, st));
  return VRAG_OK;
}

// One segment holding the postings of `parts` (consecutive row ranges): their records in row order, sorted stably by key.
// The postings of the parts, part after part, back into records (rec holds the sum of their n_post).
hipError_t expand_parts(const SegPtrs* parts, int n_parts, RecPtrs rec, hipStream_t st) {
  long long at = 0;
  for (int i = 0; i < n_parts; ++i) {
    const SegPtrs& g = parts[i];
    if (g.n_post)
      hipLaunchKernelGGL(expand_kernel, dim3(grid_of(g.n_post, 256)), dim3(256), 0, st, g.keys, g.pstart, g.n_keys, g.prow, g.ptf, g.n_post,
                         rec.key + at, rec.row + at, rec.tf + at);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    at += g.n_post;
  }
  return hipSuccess;
}

int fold(const std::vector<const Segment*>& parts, hipStream_t st, Segment& out) {
  long long total = 0;
  for (const Segment* g : parts) total += g->n_post;
  Records rec;
  HIP_TRY(rec.alloc(total));
  std::vector<SegPtrs> raw;
  for (const Segment* g : parts) raw.push_back(ptrs_of(*g));
  HIP_TRY(expand_parts(raw.data(), (int)raw.size(), RecPtrs{rec.key.as<u64>(), rec.row.as<unsigned>(), rec.tf.as<unsigned>()}, st));
  const long long row_lo = parts.front()->row_lo;
  const long long n_rows = parts.back()->row_lo + parts.back()->n_rows - row_lo;
  return build_segment(rec, 0, row_lo, n_rows, st, out);
}

// The statistics pass.  stats_dirty: N / sum dl / df of this index's live rows and K_d; kd_dirty alone (the caller's
// corpus-wide pair changed): K_d only.  K_d reads {N, sum dl} from acc[0..1], or from the caller's pair at acc[2..3].
// The launches of the statistics pass on raw arrays.  own: N / sum dl into acc[0..1] (zeroed by the caller) and df of every
// segment with keys; K_d of the n rows always, from the pair at kd_stats.
hipError_t stats_launch(const unsigned* live, const unsigned* dl, long long n, bool own, unsigned long long* acc,
                        const unsigned long long* kd_stats, float k1, float b, float* kd, const SegPtrs* segs, int n_segs, hipStream_t st) {
  if (own) hipLaunchKernelGGL(live_sum_kernel, dim3(grid_of(n, 256)), dim3(256), 0, st, live, dl, n, acc);
  hipLaunchKernelGGL(kd_kernel, dim3(grid_of(n, 256)), dim3(256), 0, st, dl, n, kd_stats, k1, 1.0f - b, b, kd);
  if (own)
    for (int s = 0; s < n_segs; ++s) {
      const SegPtrs& g = segs[s];
      if (g.n_keys)
        hipLaunchKernelGGL(df_kernel, dim3((unsigned)std::min<long long>(4096, (g.n_keys + 3) / 4)), dim3(256), 0, st, g.pstart, g.n_keys,
                           g.prow, live, g.df);
    }
  return hipGetLastError();
}

int refresh_stats(vrag_text_index* ix) {
  if (!ix->stats_dirty && !ix->kd_dirty) return VRAG_OK;
  hipStream_t st = ix->stream;
  const long long n = ix->n_rows;
  const bool own = ix->stats_dirty;
  if (ix->lists_done) HIP_TRY(hipStreamWaitEvent(st, ix->lists_done, 0));   // a device-resident search may still be reading K_d
  if (own) HIP_TRY(hipMemsetAsync(ix->acc.p, 0, 16, st));
  const unsigned long long* kd_stats = ix->acc.as<unsigned long long>();
  if (ix->corpus[0]) {
    HIP_TRY(hipMemcpyAsync(ix->acc.as<unsigned long long>() + 2, ix->corpus, 16, hipMemcpyHostToDevice, st));
    kd_stats += 2;
  }
  if (n) {
    if (own) HIP_TRY(hipMemcpyAsync(ix->live.p, ix->h_live.data(), ix->h_live.size() * 4, hipMemcpyHostToDevice, st));
    SegPtrs segs[FT_MAXSEG];
    const int n_segs = (int)ix->segs.size();
    for (int s = 0; s < n_segs; ++s) segs[s] = ptrs_of(ix->segs[s]);
    HIP_TRY(stats_launch(ix->live.as<unsigned>(), ix->dl.as<unsigned>(), n, own, ix->acc.as<unsigned long long>(), kd_stats, ix->k1, ix->b,
                         ix->kd.as<float>(), segs, n_segs, st));
  }
  if (own) HIP_TRY(hipMemcpyAsync(ix->h_acc, ix->acc.p, 16, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  ix->stats_dirty = ix->kd_dirty = false;
  return VRAG_OK;
}

// per-row arrays (dl, live, K_d) with room for `need` rows; contents kept
int grow_rows(vrag_text_index* ix, long long need) {
  if ((size_t)need <= ix->rows_cap) return VRAG_OK;
  const size_t cap = std::max<size_t>(1024, std::max<size_t>((size_t)need, ix->rows_cap * 3 / 2));
  DevBuf dl, live, kd;
  HIP_TRY(dl.alloc(cap * 4));
  HIP_TRY(live.alloc((cap + 31) / 32 * 4));
  HIP_TRY(kd.alloc(cap * 4));
  if (ix->n_rows) HIP_TRY(hipMemcpyAsync(dl.p, ix->dl.p, (size_t)ix->n_rows * 4, hipMemcpyDeviceToDevice, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  ix->dl = std::move(dl);
  ix->live = std::move(live);
  ix->kd = std::move(kd);
  ix->rows_cap = cap;
  ix->stats_dirty = true;   // fresh liveness / K_d buffers
  return VRAG_OK;
}

// The shape of a query batch: q_indptr from 0 and non-decreasing, every query's keys strictly ascending.
int check_queries(const char* fn, const int64_t* q_indptr, const uint64_t* keys, const float* weights, int32_t nq) {
  ARG_CHECK(q_indptr[0] == 0, "%s: q_indptr[0] must be 0", fn);
  for (int32_t q = 0; q < nq; ++q) {
    ARG_CHECK(q_indptr[q + 1] >= q_indptr[q], "%s: q_indptr must be non-decreasing", fn);
    ARG_CHECK(q_indptr[q + 1] == q_indptr[q] || keys, "%s: null keys / weights", fn);
    for (int64_t j = q_indptr[q] + 1; j < q_indptr[q + 1]; ++j)
      ARG_CHECK(keys[j] > keys[j - 1], "%s: the keys of query %d must be strictly ascending", fn, q);
  }
  const int64_t n_terms = nq ? q_indptr[nq] : 0;
  ARG_CHECK(n_terms == 0 || (keys && weights), "%s: null keys / weights", fn);
  return VRAG_OK;
}

// Search workspace for nq queries and lists of k, and the batch (terms, weights, filter bitmap) uploaded on `st`.
int search_upload(vrag_text_index* ix, const int64_t* q_indptr, const uint64_t* keys, const float* weights, int32_t nq, int32_t k,
                  const uint32_t* allow, int64_t allow_rows, hipStream_t st, const unsigned** d_allow, long long* allow_n) {
  const int64_t n_terms = q_indptr[nq];
  const int n_blocks = (int)((ix->n_rows + FT_ROWS - 1) / FT_ROWS);
  const int kk = std::min(k, 64), pages = (k + 63) / 64;
  HIP_TRY(ix->q_indptr.reserve((size_t)(nq + 1) * 8));
  HIP_TRY(ix->q_keys.reserve((size_t)n_terms * 8));
  HIP_TRY(ix->q_w.reserve((size_t)n_terms * 4));
  HIP_TRY(ix->q_tu.reserve((size_t)n_terms * FT_MAXSEG * 4));
  HIP_TRY(ix->cand.reserve((size_t)n_blocks * nq * kk * 8));
  HIP_TRY(ix->page.reserve((size_t)pages * nq * kk * 8));
  HIP_TRY(ix->bound.reserve((size_t)nq * 8));
  HIP_TRY(hipMemcpyAsync(ix->q_indptr.p, q_indptr, (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ix->q_keys.p, keys, (size_t)n_terms * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ix->q_w.p, weights, (size_t)n_terms * 4, hipMemcpyHostToDevice, st));
  *d_allow = nullptr;
  // rows at or beyond allow_rows (e.g. added after the caller built its filter) are not allowed
  *allow_n = allow ? std::min<long long>(allow_rows, ix->n_rows) : 0;
  if (allow) {
    const size_t words = (size_t)(*allow_n + 31) / 32;   // the caller's bitmap holds at least these
    HIP_TRY(ix->allow.reserve(words * 4));
    if (words) HIP_TRY(hipMemcpyAsync(ix->allow.p, allow, words * 4, hipMemcpyHostToDevice, st));
    *d_allow = ix->allow.as<unsigned>();
  }
  return VRAG_OK;
}

// The kernels of one search on the uploaded batch: term lookup, then per page of 64 the scoring pass and the per-query merge;
// page p of the result is ix->page[p][nq][min(k, 64)] (keys, 0 = none).
inline int score_blocks(long long n_rows) { return (int)((n_rows + FT_ROWS - 1) / FT_ROWS); }

// Term lookup on raw arrays: tu[n_terms][FT_MAXSEG], df_out [n_terms] or null.
hipError_t lookup_launch(const FtSegs& segs, const u64* keys, long long n_terms, int* tu, long long* df_out, hipStream_t st) {
  hipLaunchKernelGGL(ft_lookup_kernel, dim3(grid_of(n_terms, 256)), dim3(256), 0, st, segs, keys, n_terms, tu, df_out);
  return hipGetLastError();
}

// One page of the scoring pass on raw arrays: cand[score_blocks(n_rows)][nq][kk].
hipError_t score_launch(const FtSegs& segs, const long long* q_indptr, const int* tu, const float* w, const float* kd, const unsigned* live,
                        const unsigned* allow, long long allow_n, long long n_rows, float k1p1, int nq, int kk, const u64* bound, u64* cand,
                        hipStream_t st) {
  hipLaunchKernelGGL(ft_score_kernel, dim3(score_blocks(n_rows), nq), dim3(FT_NT), 0, st, segs, q_indptr, tu, w, kd, live, allow, allow_n,
                     n_rows, k1p1, nq, kk, bound, cand);
  return hipGetLastError();
}

int search_launch(vrag_text_index* ix, int32_t nq, int64_t n_terms, int32_t k, const unsigned* d_allow, long long allow_n, hipStream_t st) {
  const int n_blocks = score_blocks(ix->n_rows);
  const int kk = std::min(k, 64), pages = (k + 63) / 64;
  const FtSegs segs = seg_view(ix);
  HIP_TRY(lookup_launch(segs, ix->q_keys.as<u64>(), (long long)n_terms, ix->q_tu.as<int>(), nullptr, st));
  const float k1p1 = ix->k1 + 1.0f;
  for (int p = 0; p < pages; ++p) {
    u64* page = ix->page.as<u64>() + (size_t)p * nq * kk;
    HIP_TRY(score_launch(segs, ix->q_indptr.as<long long>(), ix->q_tu.as<int>(), ix->q_w.as<float>(), ix->kd.as<float>(),
                         ix->live.as<unsigned>(), d_allow, allow_n, ix->n_rows, k1p1, nq, kk, p ? ix->bound.as<u64>() : nullptr,
                         ix->cand.as<u64>(), st));
    HIP_TRY(launch_topk_merge(ix->cand.as<u64>(), n_blocks, nq, kk, page, st));
    if (p + 1 < pages) hipLaunchKernelGGL(ft_bound_kernel, dim3(grid_of(nq, 256)), dim3(256), 0, st, page, nq, kk, ix->bound.as<u64>());
    HIP_TRY(hipGetLastError());
  }
  return VRAG_OK;
}

}  // namespace

extern "C" {

int vrag_text_tokenize(const uint8_t* text, const int64_t* doc_off, int32_t n_docs, int32_t device, int64_t cap, int32_t* counts,
                       uint64_t* keys, int64_t* n_tokens) {
  ARG_CHECK(counts && n_tokens && cap >= 0 && (keys || cap == 0), "vrag_text_tokenize: bad arguments");
  int rc = check_docs(text, doc_off, n_docs);
  if (rc != VRAG_OK) return rc;
  DEVICE_CHECK(device);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  Records rec;
  DevBuf cnt;
  rc = n_docs ? tokenize(text, doc_off, n_docs, 0u, st, rec, &cnt) : VRAG_OK;
  hipError_t e = hipSuccess;
  if (rc == VRAG_OK) {
    *n_tokens = rec.n;
    if (n_docs) e = hipMemcpyAsync(counts, cnt.p, (size_t)n_docs * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && rec.n && rec.n <= cap) e = hipMemcpyAsync(keys, rec.key.p, (size_t)rec.n * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  }
  (void)hipStreamDestroy(st);
  if (rc != VRAG_OK) return rc;
  HIP_TRY(e);
  if (rec.n > cap) {
    set_error("vrag_text_tokenize: %lld tokens, cap %lld", (long long)rec.n, (long long)cap);
    return VRAG_ERR_CAPACITY;
  }
  return VRAG_OK;
}

int vrag_text_index_create(float k1, float b, int32_t device, vrag_text_index** out) {
  ARG_CHECK(out, "vrag_text_index_create: null out");
  *out = nullptr;
  ARG_CHECK(k1 >= 0.f && b >= 0.f && b <= 1.f, "vrag_text_index_create: need k1 >= 0 and 0 <= b <= 1 (got %g, %g)", k1, b);
  DEVICE_CHECK(device);
  HIP_TRY(hipSetDevice(device));
  auto* ix = new vrag_text_index();
  ix->device = device;
  ix->k1 = k1;
  ix->b = b;
  hipError_t e = hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = ix->acc.alloc(32);
  if (e != hipSuccess) {
    vrag_text_index_destroy(ix);
    HIP_TRY(e);
  }
  *out = ix;
  return VRAG_OK;
}

void vrag_text_index_destroy(vrag_text_index* ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->device);
  if (ix->stream) (void)hipStreamSynchronize(ix->stream);
  hipStream_t st = ix->stream;
  if (ix->lists_done) {
    (void)hipEventSynchronize(ix->lists_done);
    (void)hipEventDestroy(ix->lists_done);
  }
  delete ix;   // DevBufs free themselves
  if (st) (void)hipStreamDestroy(st);
}

int vrag_text_index_add(vrag_text_index* ix, const uint8_t* text, const int64_t* doc_off, int32_t n_docs, int32_t fold_all) {
  ARG_CHECK(ix, "vrag_text_index_add: null handle");
  int rc = check_docs(text, doc_off, n_docs);
  if (rc != VRAG_OK) return rc;
  if (n_docs == 0) return VRAG_OK;
  std::lock_guard<std::mutex> lock(ix->mu);
  ARG_CHECK(ix->n_rows + n_docs < 0xFFFFFF00ll, "vrag_text_index_add: more than 2^32 rows");
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t st = ix->stream;
  // a device-resident search may still be reading the segments and the per-row arrays this call replaces
  if (ix->lists_done) HIP_TRY(hipEventSynchronize(ix->lists_done));
  if ((rc = grow_rows(ix, ix->n_rows + n_docs)) != VRAG_OK) return rc;
  // Everything is built on the side; the index changes only once the whole call has succeeded (a failed add leaves it as it
  // was, and the same rows can be added again).
  Records rec;
  DevBuf cnt;
  if ((rc = tokenize(text, doc_off, n_docs, (unsigned)ix->n_rows, st, rec, &cnt)) != VRAG_OK) return rc;
  const size_t keep = fold_all ? 0 : std::min<size_t>(ix->segs.size(), 1);   // the main segment stays unless everything folds
  long long post = rec.n;                 // bounds the postings of the segment this call builds (u32 offsets)
  for (size_t g = keep; g < ix->segs.size(); ++g) post += ix->segs[g].n_post;
  if (post >= kMaxSegPostings) {
    set_error("vrag_text_index_add: a segment would hold up to %lld postings (limit %lld)", post, kMaxSegPostings);
    return VRAG_ERR_CAPACITY;
  }
  HIP_TRY(hipMemcpyAsync(ix->dl.as<unsigned>() + ix->n_rows, cnt.p, (size_t)n_docs * 4, hipMemcpyDeviceToDevice, st));
  Segment seg;
  if ((rc = build_segment(rec, 1, ix->n_rows, n_docs, st, seg)) != VRAG_OK) return rc;
  std::vector<const Segment*> parts;
  for (size_t g = keep; g < ix->segs.size(); ++g) parts.push_back(&ix->segs[g]);
  parts.push_back(&seg);
  Segment merged;
  if (parts.size() > 1 && (rc = fold(parts, st, merged)) != VRAG_OK) return rc;
  ix->segs.resize(keep);                  // commit
  ix->segs.push_back(parts.size() > 1 ? std::move(merged) : std::move(seg));
  const long long n_new = ix->n_rows + n_docs;
  ix->h_live.resize((size_t)(n_new + 31) / 32, 0u);
  for (long long r = ix->n_rows; r < n_new; ++r) ix->h_live[r >> 5] |= 1u << (r & 31);   // new rows are live
  ix->n_rows = n_new;
  ix->stats_dirty = true;
  return VRAG_OK;
}

int vrag_text_index_set_live(vrag_text_index* ix, const uint32_t* words, int64_t n_rows) {
  ARG_CHECK(ix && words, "vrag_text_index_set_live: bad arguments");
  std::lock_guard<std::mutex> lock(ix->mu);
  ARG_CHECK(n_rows == ix->n_rows, "vrag_text_index_set_live: %lld rows given, the index holds %lld", (long long)n_rows, ix->n_rows);
  const size_t n_words = (size_t)(n_rows + 31) / 32;
  std::memcpy(ix->h_live.data(), words, n_words * 4);
  if (n_rows & 31) ix->h_live[n_words - 1] &= (1u << (n_rows & 31)) - 1u;
  ix->stats_dirty = true;
  return VRAG_OK;
}

int vrag_text_index_set_corpus_stats(vrag_text_index* ix, int64_t n_live_total, int64_t sum_dl_total) {
  ARG_CHECK(ix, "vrag_text_index_set_corpus_stats: null handle");
  ARG_CHECK(n_live_total >= 0 && sum_dl_total >= 0 && (n_live_total > 0 || sum_dl_total == 0),
            "vrag_text_index_set_corpus_stats: need n_live_total >= 0, sum_dl_total >= 0 and no tokens without rows (got %lld, %lld)",
            (long long)n_live_total, (long long)sum_dl_total);
  std::lock_guard<std::mutex> lock(ix->mu);
  if ((unsigned long long)n_live_total == ix->corpus[0] && (unsigned long long)sum_dl_total == ix->corpus[1]) return VRAG_OK;
  ix->corpus[0] = (unsigned long long)n_live_total;
  ix->corpus[1] = (unsigned long long)sum_dl_total;
  ix->kd_dirty = true;
  return VRAG_OK;
}

int vrag_text_index_stats(vrag_text_index* ix, int64_t* n_rows, int64_t* n_live, int64_t* sum_dl, int64_t* n_segments, int64_t* n_postings) {
  ARG_CHECK(ix, "vrag_text_index_stats: null handle");
  std::lock_guard<std::mutex> lock(ix->mu);
  HIP_TRY(hipSetDevice(ix->device));
  const int rc = refresh_stats(ix);
  if (rc != VRAG_OK) return rc;
  long long post = 0;
  for (const Segment& g : ix->segs) post += g.n_post;
  if (n_rows) *n_rows = ix->n_rows;
  if (n_live) *n_live = (int64_t)ix->h_acc[0];
  if (sum_dl) *sum_dl = (int64_t)ix->h_acc[1];
  if (n_segments) *n_segments = (int64_t)ix->segs.size();
  if (n_postings) *n_postings = post;
  return VRAG_OK;
}

int vrag_text_index_query_terms(vrag_text_index* ix, const uint8_t* text, const int64_t* doc_off, int32_t nq, int64_t cap,
                                int64_t* q_indptr, uint64_t* keys, int32_t* counts, int64_t* df, int64_t* n_live) {
  ARG_CHECK(ix && q_indptr && n_live && cap >= 0 && (cap == 0 || (keys && counts && df)), "vrag_text_index_query_terms: bad arguments");
  int rc = check_docs(text, doc_off, nq);
  if (rc != VRAG_OK) return rc;
  std::lock_guard<std::mutex> lock(ix->mu);
  HIP_TRY(hipSetDevice(ix->device));
  if ((rc = refresh_stats(ix)) != VRAG_OK) return rc;
  *n_live = (int64_t)(ix->corpus[0] ? ix->corpus[0] : ix->h_acc[0]);
  for (int32_t q = 0; q <= nq; ++q) q_indptr[q] = 0;
  if (nq == 0) return VRAG_OK;
  hipStream_t st = ix->stream;
  Records rec;
  if ((rc = tokenize(text, doc_off, nq, 0u, st, rec, nullptr)) != VRAG_OK) return rc;
  if (rec.n == 0) return VRAG_OK;
  int row_bits = 0;
  while ((1ll << row_bits) < nq) row_bits += 8;
  HIP_TRY(radix_sort(rec, 0, 0, st));
  HIP_TRY(radix_sort(rec, 1, row_bits, st));   // (query, key) order, stable
  Runs runs;
  HIP_TRY(rle(rec, 1, nullptr, &runs, st));
  const long long P = runs.n_post;
  if (P > cap) {
    set_error("vrag_text_index_query_terms: %lld distinct query terms, cap %lld", P, (long long)cap);
    return VRAG_ERR_CAPACITY;
  }
  DevBuf tu, d_df;
  HIP_TRY(tu.alloc((size_t)P * FT_MAXSEG * 4));
  HIP_TRY(d_df.alloc((size_t)P * 8));
  HIP_TRY(lookup_launch(seg_view(ix), runs.pkey.as<u64>(), P, tu.as<int>(), d_df.as<long long>(), st));
  std::vector<unsigned> qrow((size_t)P), tf((size_t)P);
  HIP_TRY(hipMemcpyAsync(qrow.data(), runs.prow.p, (size_t)P * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(tf.data(), runs.ptf.p, (size_t)P * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(keys, runs.pkey.p, (size_t)P * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(df, d_df.p, (size_t)P * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (long long p = 0; p < P; ++p) {
    counts[p] = (int32_t)tf[p];
    ++q_indptr[qrow[p] + 1];
  }
  for (int32_t q = 0; q < nq; ++q) q_indptr[q + 1] += q_indptr[q];
  return VRAG_OK;
}

int vrag_text_index_search(vrag_text_index* ix, const int64_t* q_indptr, const uint64_t* keys, const float* weights, int32_t nq,
                           int32_t k, const uint32_t* allow, int64_t allow_rows, float* scores, int64_t* ids) {
  ARG_CHECK(ix && q_indptr && scores && ids && nq >= 0, "vrag_text_index_search: bad arguments");
  ARG_CHECK(k >= 1 && k <= 1024, "vrag_text_index_search: k must be in 1..1024, got %d", k);
  int rc = check_queries("vrag_text_index_search", q_indptr, keys, weights, nq);
  if (rc != VRAG_OK) return rc;
  const int64_t n_terms = nq ? q_indptr[nq] : 0;
  fill_no_hits(scores, ids, (size_t)nq * k);
  if (nq == 0) return VRAG_OK;
  std::lock_guard<std::mutex> lock(ix->mu);
  ARG_CHECK(!allow || allow_rows >= 0, "vrag_text_index_search: negative allow_rows");
  if (n_terms == 0 || ix->n_rows == 0) return VRAG_OK;
  HIP_TRY(hipSetDevice(ix->device));
  if ((rc = refresh_stats(ix)) != VRAG_OK) return rc;
  hipStream_t st = ix->stream;
  if (ix->lists_done) HIP_TRY(hipStreamWaitEvent(st, ix->lists_done, 0));   // a device-resident search may still be reading the workspace
  const int kk = std::min(k, 64), pages = (k + 63) / 64;
  const unsigned* d_allow = nullptr;
  long long allow_n = 0;
  if ((rc = search_upload(ix, q_indptr, keys, weights, nq, k, allow, allow_rows, st, &d_allow, &allow_n)) != VRAG_OK) return rc;
  if ((rc = search_launch(ix, nq, n_terms, k, d_allow, allow_n, st)) != VRAG_OK) return rc;
  std::vector<u64> h((size_t)pages * nq * kk);
  HIP_TRY(hipMemcpyAsync(h.data(), ix->page.p, h.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int32_t q = 0; q < nq; ++q)
    for (int32_t i = 0; i < k; ++i) {
      const u64 key = h[((size_t)(i / 64) * nq + q) * kk + i % 64];
      if (!key) break;
      decode_key(key, &scores[(size_t)q * k + i], &ids[(size_t)q * k + i]);
    }
  return VRAG_OK;
}

int vrag_text_index_search_device(vrag_text_index* ix, const int64_t* q_indptr, const uint64_t* keys, const float* weights, int32_t nq,
                                  int32_t k, const uint32_t* allow, int64_t allow_rows, const int64_t* row_map, int64_t n_map,
                                  int64_t id_base, float* out_scores, int64_t* out_ids, void* stream) {
  ARG_CHECK(ix && q_indptr && out_scores && out_ids && nq > 0, "vrag_text_index_search_device: bad arguments");
  ARG_CHECK(k >= 1 && k <= 64, "vrag_text_index_search_device: k must be in 1..64 for a device-resident search, got %d", k);
  ARG_CHECK(!row_map || n_map >= 0, "vrag_text_index_search_device: negative row map length");
  int rc = check_queries("vrag_text_index_search_device", q_indptr, keys, weights, nq);
  if (rc != VRAG_OK) return rc;
  const int64_t n_terms = q_indptr[nq];
  std::lock_guard<std::mutex> lock(ix->mu);
  ARG_CHECK(!allow || allow_rows >= 0, "vrag_text_index_search_device: negative allow_rows");
  HIP_TRY(hipSetDevice(ix->device));
  if ((rc = refresh_stats(ix)) != VRAG_OK) return rc;
  // Uploads go through the handle's own stream and are waited for (the host arrays are free on return); the kernels are
  // only enqueued on the caller's stream (NULL = the legacy default stream), which the all-gather that follows is ordered on.
  hipStream_t up = ix->stream, st = reinterpret_cast<hipStream_t>(stream);
  if (ix->lists_done) HIP_TRY(hipStreamWaitEvent(up, ix->lists_done, 0));
  const long long n = (long long)nq * k;
  if (n_terms == 0 || ix->n_rows == 0) {   // no query term or no row: every list is empty
    HIP_TRY(ix->page.reserve((size_t)n * 8));
    HIP_TRY(hipStreamSynchronize(up));
    HIP_TRY(hipMemsetAsync(ix->page.p, 0, (size_t)n * 8, st));
  } else {
    const unsigned* d_allow = nullptr;
    long long allow_n = 0;
    if ((rc = search_upload(ix, q_indptr, keys, weights, nq, k, allow, allow_rows, up, &d_allow, &allow_n)) != VRAG_OK) return rc;
    HIP_TRY(hipStreamSynchronize(up));
    if ((rc = search_launch(ix, nq, n_terms, k, d_allow, allow_n, st)) != VRAG_OK) return rc;
  }
  HIP_TRY(launch_topk_export(ix->page.as<u64>(), n, row_map, n_map, id_base, out_scores, out_ids, st));
  HIP_TRY(record_event(ix->lists_done, st));
  return VRAG_OK;
}

}  // extern "C"

#ifdef VRAG_DEBUG_API
// ------------------------------------------------------------------------------------ unit-test hook (harness build only)
#include "../../include/vrag_amd_debug.h"
#include "debug_bufs.h"

namespace {

constexpr long long kDbgMax = 1ll << 22;   // every count of the hook: sizes and u32 offsets stay far inside their types

// The segments of the argument block as the kernels must find them (see the header); rows_total < 0 = no bound on the rows.
int dbg_check_segs(const vrag_debug_text_args* a, bool need_ptf, bool need_df, long long rows_total) {
  ARG_CHECK(a->n_segs >= 1 && a->n_segs <= FT_MAXSEG, "n_segs (%d) must be in 1..%d", a->n_segs, FT_MAXSEG);
  long long next_row = 0;
  for (int s = 0; s < a->n_segs; ++s) {
    const long long nk = a->seg_n_keys[s], np = a->seg_n_post[s], lo = a->seg_row_lo[s], nr = a->seg_n_rows[s];
    ARG_CHECK(nk >= 0 && nk <= kDbgMax && np >= 0 && np <= kDbgMax && nr >= 0 && nr <= kDbgMax, "segment %d: a count is negative or above 2^22", s);
    ARG_CHECK(lo == next_row, "segment %d: row_lo (%lld) does not follow its predecessor (%lld)", s, lo, next_row);
    next_row = lo + nr;
    ARG_CHECK(rows_total < 0 || next_row <= rows_total, "segment %d reaches row %lld of %lld", s, next_row, rows_total);
    ARG_CHECK(a->seg_pstart[s] && (nk == 0 || a->seg_keys[s]) && (np == 0 || (a->seg_prow[s] && (!need_ptf || a->seg_ptf[s]))) &&
                  (!need_df || nk == 0 || a->seg_df[s]),
              "segment %d: null array", s);
    ARG_CHECK(nk > 0 || np == 0, "segment %d: %lld postings without a key", s, np);
    const uint32_t* ps = a->seg_pstart[s];
    ARG_CHECK(ps[0] == 0u, "segment %d: pstart[0] = %u", s, ps[0]);
    ARG_CHECK((long long)ps[nk] == np, "segment %d: pstart[n_keys] = %u, n_post = %lld", s, ps[nk], np);
    for (long long u = 0; u < nk; ++u) {
      ARG_CHECK(ps[u] <= ps[u + 1] && (long long)ps[u + 1] <= np, "segment %d: pstart decreases or leaves the postings at key %lld", s, u);
      for (uint32_t p = ps[u]; p < ps[u + 1]; ++p) {
        const long long r = a->seg_prow[s][p];
        ARG_CHECK(r >= lo && r < lo + nr, "segment %d: posting %u has row %lld outside [%lld, %lld)", s, p, r, lo, lo + nr);
        ARG_CHECK(p == ps[u] || a->seg_prow[s][p - 1] < a->seg_prow[s][p], "segment %d: the rows of key %lld are not strictly ascending", s, u);
      }
    }
  }
  return VRAG_OK;
}

// Device copies of the segments; df_out: df goes back to the caller (STATS).
void dbg_stage_segs(const vrag_debug_text_args* a, DbgBufs& B, bool df_out, SegPtrs* segs) {
  for (int s = 0; s < a->n_segs; ++s) {
    const size_t nk = (size_t)a->seg_n_keys[s], np = (size_t)a->seg_n_post[s];
    SegPtrs& g = segs[s];
    g.keys = B.in<u64>(a->seg_keys[s], a->seg_keys[s] ? nk : 0, "seg_keys");
    g.pstart = B.in<unsigned>(a->seg_pstart[s], nk + 1, "seg_pstart");
    g.prow = B.in<unsigned>(a->seg_prow[s], a->seg_prow[s] ? np : 0, "seg_prow");
    g.ptf = B.in<unsigned>(a->seg_ptf[s], a->seg_ptf[s] ? np : 0, "seg_ptf");
    g.df = df_out ? B.inout<unsigned>(a->seg_df[s], a->seg_df[s] ? nk : 0, "seg_df") : B.in<unsigned>(a->seg_df[s], a->seg_df[s] ? nk : 0, "seg_df");
    g.n_keys = (long long)nk;
    g.n_post = (long long)np;
    g.row_lo = a->seg_row_lo[s];
    g.n_rows = a->seg_n_rows[s];
  }
}

// SORT by key / row of n records held in `a` (scratch from B); returns the set that holds the result.
hipError_t dbg_sort(DbgBufs& B, RecPtrs a, long long n, int by_row, int row_bits, RecPtrs* sorted) {
  const size_t tiles = (size_t)radix_tiles(n), m = (size_t)n;
  RecPtrs b{B.scratch<u64>(m, "sort scratch key"), B.scratch<unsigned>(m, "sort scratch row"), B.scratch<unsigned>(m, "sort scratch tf")};
  unsigned* hist = B.scratch<unsigned>(tiles * 256, "sort hist");
  unsigned* offs = B.scratch<unsigned>(tiles * 256 + 1, "sort offs");
  *sorted = a;
  if (B.staged() != hipSuccess) return B.err;
  bool in_b = false;
  const hipError_t e = radix_passes(a, b, n, by_row, row_bits, hist, offs, nullptr, &in_b);
  if (in_b) *sorted = b;
  return e;
}

// RLE of n records into the caller's output buffers (device copies sized post_buf / keys_buf, checked >= n by the caller).
// n_post_host stays alive until finish() has synchronised.
hipError_t dbg_rle(DbgBufs& B, vrag_debug_text_args* a, RecPtrs r, long long n, int unit, bool seg_form, bool query_form,
                   unsigned* n_post_host) {
  const size_t m = (size_t)n, pb = (size_t)a->post_buf, kb = (size_t)a->keys_buf;
  RleScratch scr{B.scratch<unsigned>(m, "rle pflag"), B.scratch<unsigned>(m, "rle kflag"), B.scratch<unsigned>(m + 1, "rle pscan"),
                 B.scratch<unsigned>(m + 1, "rle kscan")};
  unsigned* ppos = B.scratch<unsigned>(pb, "rle ppos");
  unsigned* prow = B.inout<uint32_t>(a->prow, pb, "prow");
  unsigned* ptf = B.inout<uint32_t>(a->ptf, pb, "ptf");
  u64* pkey = query_form ? B.inout<u64>(a->pkey, pb, "pkey") : nullptr;
  u64* ukeys = seg_form ? B.inout<u64>(a->ukeys, kb, "ukeys") : nullptr;
  unsigned* pstart = seg_form ? B.inout<uint32_t>(a->pstart, kb + 1, "pstart") : nullptr;
  if (B.staged() != hipSuccess) return B.err;
  unsigned n_keys = 0;
  hipError_t e = rle_count(r, n, scr, n_post_host, &n_keys, nullptr);
  if (e != hipSuccess) return e;
  a->n_post = *n_post_host;
  a->n_keys = n_keys;
  if ((long long)*n_post_host > n || (long long)n_keys > n) return hipErrorUnknown;   // the scans' totals exceed the flags: nothing may rest on them
  return rle_emit(r, n, scr, unit, n_post_host, n_keys, ukeys, pstart, prow, ptf, ppos, pkey, nullptr);
}

}  // namespace

extern "C" {

int vrag_debug_text_run(vrag_debug_text_args* a, int32_t device) {
  ARG_CHECK(a, "null arguments");
  const int op = a->op;
  ARG_CHECK(op >= VRAG_DEBUG_TEXT_SCAN && op <= VRAG_DEBUG_TEXT_SCORE, "op %d is not a full-text stage", op);
  ARG_CHECK(device >= 0, "bad device %d", device);
  const bool scan = op == VRAG_DEBUG_TEXT_SCAN, sort = op == VRAG_DEBUG_TEXT_SORT, rle_op = op == VRAG_DEBUG_TEXT_RLE;
  const bool fold_op = op == VRAG_DEBUG_TEXT_FOLD, stats = op == VRAG_DEBUG_TEXT_STATS, lookup = op == VRAG_DEBUG_TEXT_LOOKUP;
  const bool score = op == VRAG_DEBUG_TEXT_SCORE;
  long long total = 0;   // fold: the parts' postings
  if (scan || sort || rle_op) ARG_CHECK(a->n >= 0 && a->n <= kDbgMax, "n (%lld) must be in 0..2^22", (long long)a->n);
  if (scan) {
    ARG_CHECK(a->out && (a->n == 0 || a->in), "scan needs in and out");
    ARG_CHECK(a->n_buf >= a->n && a->n_buf <= kDbgMax, "scan: n_buf (%lld) below n (%lld)", (long long)a->n_buf, (long long)a->n);
  }
  if (sort) {
    ARG_CHECK(a->n == 0 || (a->key && a->row && a->tf), "sort needs key, row and tf");
    ARG_CHECK(!a->by_row || (a->row_bits >= 0 && a->row_bits <= 32 && a->row_bits % 8 == 0), "sort: row_bits (%d) must be 0, 8, 16, 24 or 32",
              a->row_bits);
  }
  if (rle_op) {
    ARG_CHECK(a->n == 0 || (a->key && a->row && a->tf), "rle needs key, row and tf");
    ARG_CHECK((a->ukeys != nullptr) == (a->pstart != nullptr), "rle: ukeys and pstart come together");
    ARG_CHECK(a->ukeys || a->pkey, "rle: neither the segment form (ukeys, pstart) nor the query form (pkey) is asked for");
  }
  if (fold_op) {
    ARG_CHECK(a->ukeys && a->pstart, "fold needs ukeys and pstart");
    const int rc = dbg_check_segs(a, true, false, -1);
    if (rc != VRAG_OK) return rc;
    for (int s = 0; s < a->n_segs; ++s) total += a->seg_n_post[s];
    ARG_CHECK(total <= kDbgMax, "fold: %lld postings are too many for the hook", total);
  }
  if (rle_op || fold_op) {
    const long long need = rle_op ? (long long)a->n : total;
    ARG_CHECK(a->prow && a->ptf, "%s needs prow and ptf", rle_op ? "rle" : "fold");
    ARG_CHECK(a->post_buf >= need && a->post_buf <= kDbgMax, "post_buf (%lld) below the records (%lld)", (long long)a->post_buf, need);
    ARG_CHECK(a->keys_buf >= need && a->keys_buf <= kDbgMax, "keys_buf (%lld) below the records (%lld)", (long long)a->keys_buf, need);
  }
  if (stats || score) ARG_CHECK(a->n_rows >= 1 && a->n_rows <= kDbgMax, "n_rows (%lld) must be in 1..2^22", (long long)a->n_rows);
  if (stats) {
    ARG_CHECK(a->dl && a->live && a->acc && a->kd, "stats needs dl, live, acc and kd");
    ARG_CHECK(a->rows_buf >= a->n_rows && a->rows_buf <= kDbgMax, "stats: rows_buf (%lld) below n_rows (%lld)", (long long)a->rows_buf, (long long)a->n_rows);
    ARG_CHECK(a->k1 >= 0.f && a->b >= 0.f && a->b <= 1.f, "stats: need k1 >= 0 and 0 <= b <= 1 (got %g, %g)", a->k1, a->b);
    ARG_CHECK(a->corpus_n >= 0 && a->corpus_sum_dl >= 0 && (a->corpus_n > 0 || a->corpus_sum_dl == 0), "stats: a corpus pair with tokens but no rows (%lld, %lld)",
              (long long)a->corpus_n, (long long)a->corpus_sum_dl);
    const int rc = dbg_check_segs(a, false, true, a->n_rows);
    if (rc != VRAG_OK) return rc;
  }
  if (lookup) {
    ARG_CHECK(a->n_terms >= 1 && a->n_terms <= kDbgMax, "lookup: n_terms (%lld) must be in 1..2^22", (long long)a->n_terms);
    ARG_CHECK(a->terms_buf >= a->n_terms && a->terms_buf <= kDbgMax, "lookup: terms_buf (%lld) below n_terms (%lld)", (long long)a->terms_buf, (long long)a->n_terms);
    ARG_CHECK(a->qkeys && a->tu, "lookup needs qkeys and tu");
    const int rc = dbg_check_segs(a, false, true, -1);
    if (rc != VRAG_OK) return rc;
  }
  int n_blocks = 0;
  if (score) {
    ARG_CHECK(a->q_indptr && a->kd && a->live && a->cand, "score needs q_indptr, kd, live and cand");
    ARG_CHECK(a->nq >= 1 && a->nq <= 65535, "score: nq (%d) must be in 1..65535", a->nq);
    ARG_CHECK(a->kk >= 1 && a->kk <= 64, "score: kk (%d) must be in 1..64", a->kk);
    ARG_CHECK(a->n_terms >= 0 && a->n_terms <= kDbgMax, "score: n_terms (%lld) must be in 0..2^22", (long long)a->n_terms);
    ARG_CHECK(a->n_terms == 0 || (a->tu && a->w), "score needs tu and w");
    const int rc = dbg_check_segs(a, true, false, a->n_rows);
    if (rc != VRAG_OK) return rc;
    ARG_CHECK(a->q_indptr[0] == 0, "score: q_indptr[0] must be 0");
    for (int q = 0; q < a->nq; ++q) ARG_CHECK(a->q_indptr[q + 1] >= a->q_indptr[q], "score: q_indptr decreases at query %d", q);
    ARG_CHECK(a->q_indptr[a->nq] == a->n_terms, "score: q_indptr ends at %lld, n_terms = %lld", (long long)a->q_indptr[a->nq], (long long)a->n_terms);
    for (long long j = 0; j < a->n_terms; ++j)
      for (int s = 0; s < FT_MAXSEG; ++s) {
        const long long u = a->tu[j * FT_MAXSEG + s];
        ARG_CHECK(s < a->n_segs ? (u >= -1 && u < a->seg_n_keys[s]) : u == -1, "score: tu[%lld][%d] = %lld is no key of that segment", j, s, u);
      }
    ARG_CHECK(!a->allow || (a->allow_rows >= 0 && a->allow_rows <= a->n_rows), "score: allow_rows (%lld) outside [0, n_rows = %lld]",
              (long long)a->allow_rows, (long long)a->n_rows);
    n_blocks = score_blocks(a->n_rows);
    ARG_CHECK(a->cand_buf >= (long long)n_blocks * a->nq * a->kk && a->cand_buf <= (1ll << 26), "score: cand_buf (%lld) below blocks * nq * kk (%lld)",
              (long long)a->cand_buf, (long long)n_blocks * a->nq * a->kk);
  }
  if (const int rc = use_device(device); rc != VRAG_OK) return rc;

  DbgBufs B;
  hipError_t e = hipSuccess;
  unsigned n_post_host = 0;   // rle_emit copies it on the stream: alive until B.finish()
  SegPtrs segs[FT_MAXSEG];
  switch (op) {
    case VRAG_DEBUG_TEXT_SCAN: {
      const unsigned* in = B.in<uint32_t>(a->in, (size_t)a->n, "in");
      unsigned* out = B.inout<uint32_t>(a->out, (size_t)a->n_buf + 1, "out");
      if ((e = B.staged()) == hipSuccess) e = scan_u32(in, a->n, out, nullptr);
      break;
    }
    case VRAG_DEBUG_TEXT_SORT: {
      const size_t n = (size_t)a->n;
      RecPtrs r{B.in<u64>(a->key, n, "key"), B.in<uint32_t>(a->row, n, "row"), B.in<uint32_t>(a->tf, n, "tf")};
      RecPtrs sorted = r;
      if ((e = B.staged()) == hipSuccess) e = dbg_sort(B, r, a->n, a->by_row, a->row_bits, &sorted);
      if (e == hipSuccess) e = hipDeviceSynchronize();
      if (e == hipSuccess && n) e = hipMemcpy(a->key, sorted.key, n * 8, hipMemcpyDeviceToHost);
      if (e == hipSuccess && n) e = hipMemcpy(a->row, sorted.row, n * 4, hipMemcpyDeviceToHost);
      if (e == hipSuccess && n) e = hipMemcpy(a->tf, sorted.tf, n * 4, hipMemcpyDeviceToHost);
      break;
    }
    case VRAG_DEBUG_TEXT_RLE: {
      const size_t n = (size_t)a->n;
      RecPtrs r{B.in<u64>(a->key, n, "key"), B.in<uint32_t>(a->row, n, "row"), B.in<uint32_t>(a->tf, n, "tf")};
      if ((e = B.staged()) == hipSuccess) e = dbg_rle(B, a, r, a->n, a->unit, a->ukeys != nullptr, a->pkey != nullptr, &n_post_host);
      break;
    }
    case VRAG_DEBUG_TEXT_FOLD: {
      dbg_stage_segs(a, B, false, segs);
      const size_t n = (size_t)total;
      RecPtrs r{B.scratch<u64>(n, "fold key"), B.scratch<unsigned>(n, "fold row"), B.scratch<unsigned>(n, "fold tf")};
      RecPtrs sorted = r;
      if ((e = B.staged()) == hipSuccess) e = expand_parts(segs, a->n_segs, r, nullptr);
      if (e == hipSuccess) e = dbg_sort(B, r, total, 0, 0, &sorted);   // build_segment: by key, then RLE with the records' tf
      if (e == hipSuccess) e = dbg_rle(B, a, sorted, total, 0, true, false, &n_post_host);
      break;
    }
    case VRAG_DEBUG_TEXT_STATS: {
      const size_t n = (size_t)a->n_rows, words = (n + 31) / 32;
      dbg_stage_segs(a, B, true, segs);
      const unsigned* dl = B.in<uint32_t>(a->dl, n, "dl");
      const unsigned* live = B.in<uint32_t>(a->live, words, "live");
      float* kd = B.inout<float>(a->kd, (size_t)a->rows_buf, "kd");
      unsigned long long pair[4] = {0, 0, (unsigned long long)a->corpus_n, (unsigned long long)a->corpus_sum_dl};   // as refresh_stats lays acc out
      unsigned long long* acc = B.in<unsigned long long>(pair, 4, "acc");
      if ((e = B.staged()) == hipSuccess)
        e = stats_launch(live, dl, a->n_rows, true, acc, acc + (a->corpus_n ? 2 : 0), a->k1, a->b, kd, segs, a->n_segs, nullptr);
      if (e == hipSuccess) e = hipDeviceSynchronize();
      if (e == hipSuccess) e = hipMemcpy(a->acc, acc, 16, hipMemcpyDeviceToHost);
      break;
    }
    case VRAG_DEBUG_TEXT_LOOKUP: {
      dbg_stage_segs(a, B, false, segs);
      const u64* qk = B.in<u64>(a->qkeys, (size_t)a->n_terms, "qkeys");
      int* tu = B.inout<int32_t>(a->tu, (size_t)a->terms_buf * FT_MAXSEG, "tu");
      long long* df = B.inout_opt<long long>(a->df_out, (size_t)a->terms_buf, "df_out");
      if ((e = B.staged()) == hipSuccess) e = lookup_launch(seg_view(segs, a->n_segs), qk, a->n_terms, tu, df, nullptr);
      break;
    }
    default: {
      const size_t n = (size_t)a->n_rows, nt = (size_t)a->n_terms;
      dbg_stage_segs(a, B, false, segs);
      const long long* qi = B.in<long long>(a->q_indptr, (size_t)a->nq + 1, "q_indptr");
      const int* tu = B.in<int32_t>(a->tu, nt * FT_MAXSEG, "tu");
      const float* w = B.in<float>(a->w, nt, "w");
      const float* kd = B.in<float>(a->kd, n, "kd");
      const unsigned* live = B.in<uint32_t>(a->live, (n + 31) / 32, "live");
      const unsigned* allow = B.in_opt<uint32_t>(a->allow, ((size_t)a->allow_rows + 31) / 32, "allow");
      const u64* bound = B.in_opt<u64>(a->bound, (size_t)a->nq, "bound");
      u64* cand = B.inout<u64>(a->cand, (size_t)a->cand_buf, "cand");
      if ((e = B.staged()) == hipSuccess)
        e = score_launch(seg_view(segs, a->n_segs), qi, tu, w, kd, live, allow, allow ? a->allow_rows : 0, a->n_rows, a->k1p1, a->nq, a->kk, bound,
                         cand, nullptr);
      break;
    }
  }
  return B.finish("text", e);
}

int vrag_debug_text_index_read(vrag_text_index* ix, vrag_debug_text_index_state* s) {
  ARG_CHECK(ix && s, "vrag_debug_text_index_read: null arguments");
  std::lock_guard<std::mutex> lock(ix->mu);
  HIP_TRY(hipSetDevice(ix->device));
  const int rc = refresh_stats(ix);
  if (rc != VRAG_OK) return rc;
  const int n_segs = (int)ix->segs.size();
  if (!s->with_data) {
    s->n_segs = n_segs;
    s->n_rows = ix->n_rows;
    s->n_live = (int64_t)ix->h_acc[0];
    s->sum_dl = (int64_t)ix->h_acc[1];
    for (int g = 0; g < 2; ++g) {
      const Segment* seg = g < n_segs ? &ix->segs[g] : nullptr;
      s->row_lo[g] = seg ? seg->row_lo : 0;
      s->seg_rows[g] = seg ? seg->n_rows : 0;
      s->n_keys[g] = seg ? seg->n_keys : 0;
      s->n_post[g] = seg ? seg->n_post : 0;
    }
    return VRAG_OK;
  }
  ARG_CHECK(s->n_segs == n_segs && s->n_rows == ix->n_rows, "vrag_debug_text_index_read: the index changed between the two calls");
  for (int g = 0; g < n_segs; ++g)
    ARG_CHECK(s->row_lo[g] == ix->segs[g].row_lo && s->seg_rows[g] == ix->segs[g].n_rows && s->n_keys[g] == ix->segs[g].n_keys &&
                  s->n_post[g] == ix->segs[g].n_post,
              "vrag_debug_text_index_read: the index changed between the two calls (segment %d)", g);
  hipStream_t st = ix->stream;
  auto get = [&](void* dst, const DevBuf& src, size_t bytes) -> hipError_t {
    return dst && bytes ? hipMemcpyAsync(dst, src.p, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
  };
  for (int g = 0; g < n_segs; ++g) {
    const Segment& seg = ix->segs[g];
    HIP_TRY(get(s->keys[g], seg.keys, (size_t)seg.n_keys * 8));
    HIP_TRY(get(s->pstart[g], seg.pstart, (size_t)(seg.n_keys + 1) * 4));
    HIP_TRY(get(s->prow[g], seg.prow, (size_t)seg.n_post * 4));
    HIP_TRY(get(s->ptf[g], seg.ptf, (size_t)seg.n_post * 4));
    HIP_TRY(get(s->df[g], seg.df, (size_t)seg.n_keys * 4));
  }
  const size_t n = (size_t)ix->n_rows;
  HIP_TRY(get(s->dl, ix->dl, n * 4));
  HIP_TRY(get(s->kd, ix->kd, n * 4));
  HIP_TRY(get(s->live, ix->live, (n + 31) / 32 * 4));
  HIP_TRY(hipStreamSynchronize(st));
  return VRAG_OK;
}

}  // extern "C"
#endif  // VRAG_DEBUG_API
