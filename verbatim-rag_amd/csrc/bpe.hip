// Byte-level BPE tokenisation on gfx950 + C ABI: the ids HF `tokenizers` returns for [NFC] -> ByteLevel(use_regex) -> BPE ->
// `<cls> $A <sep>` (include/vrag_amd.h states the rules).  One batch of UTF-8 texts (blob + doc_off):
//   runs      bpe_tile_runs_kernel: U+0020 bytes at the head and at the tail of every 4096-byte tile, so that the length of a
//             space run is known however many tiles it spans (a lane walks lanes in LDS, lane 0 walks tiles).
//   bounds    bpe_bounds_kernel<false / true>: 16 text bytes per lane, 4096 per workgroup.  Every code point is classed by
//             the committed table (bpe_table.inc); uncovered code points and a failed NFC quick check flag the text.  A space
//             looks its whole run up and finds its place in the greedy cut into space-run tokens; every other code point
//             decides "a pre-token starts here" from its class, its neighbours' and the contraction rule -- at most 4 code
//             points back and 1 ahead, read from the text itself, so tiles need no halo copy.  Counting pass, block scan + scan
//             of the tile counts, then the same pass writes (start byte, text, space-run token?) of every pre-token in order.
//   merge     bpe_merge_kernel: one pre-token per wave64, one symbol per lane.  Every round each lane looks its pair
//             (symbol, right neighbour) up in an open-addressing table {left, right, rank, merged} in HBM (a dependent,
//             L2-resident gather: hidden by occupancy -- the kernel holds no LDS and a handful of registers), a butterfly
//             takes the minimum of (rank, lane), the winning lane takes the merged id and the lanes behind it move up.
//   pack      token_frame.h, shared with csrc/wordpiece.hip: tokenizer_encode checks and uploads the batch, calls the passes above
//             and launches the packing kernels of token_pack.h.
// vrag_bpe_encode_offsets adds, on its own route only (vrag_bpe_encode launches what it always did):
//   leads     offsets_lead_count_kernel: UTF-8 lead bytes per 16-byte lane, block scan; with the scan of the tile totals this is the
//             number of code points in front of any byte (lane prefix + tile prefix + a popcount inside the lane's 16 bytes).
//   merge     offsets_merge_kernel (merge_word<true>) carries a byte width per symbol lane next to `sym`; a wave prefix sum of the surviving widths
//             gives every id its bytes, the lead counts turn them into code points of its own text.
//   pack      the frame's second pack_gather_kernel moves the (start, end) pairs as the first moved the ids.
// Integer work only; vector stores only.
#include "../../include/vrag_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "common.h"
#include "host_util.h"
#include "token_frame.h"
#include "utf8_text.h"

namespace vrag {
namespace bpe {
#define BPE_TABLE_STORAGE static __device__ const
#include "bpe_table.inc"
#undef BPE_TABLE_STORAGE

constexpr unsigned C_O = 0, C_L = 1, C_N = 2, C_W = 3, C_QC = 4, C_NOTCOV = 8;
constexpr int P_NONE = 4, P_SPACE = 5;   // what stands in front of a code point: a class, nothing (segment start), an ordinary U+0020
constexpr int NT = 256, BPT = 16;
static_assert(NT * BPT == VRAG_BPE_TILE_BYTES, "the header exports the tile size");
static_assert(VRAG_BPE_MAX_WORD_BYTES == 64, "one symbol per lane of a wave64");
constexpr int kMaxRunTiles = 256;    // tiles a space run may span before its text is given up
constexpr int kSlowLookBack = 256;   // spaces counted byte by byte in front of a contraction that lies across a tile boundary
constexpr unsigned kNoRank = 0xFFFFFFFFu;
constexpr unsigned kHashBase = 0x01000193u;

__device__ __forceinline__ unsigned cell_of(unsigned cp) {
  const unsigned page = kBpePage[cp >> VRAG_BPE_PAGE_SHIFT];
  return kBpeCell[(page << VRAG_BPE_PAGE_SHIFT) | (cp & ((1u << VRAG_BPE_PAGE_SHIFT) - 1u))];
}

__host__ __device__ inline unsigned fmix32(unsigned h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
__host__ __device__ inline unsigned pair_hash(unsigned a, unsigned b) { return fmix32(a * 0x9E3779B1u ^ fmix32(b + 0x7F4A7C15u)); }

// The greedy cut of a run of U+0020 into space-run tokens (device memory): lg[x] = the largest n of S with n <= x (0: none),
// x <= 64; cons[x] = how many of x < M spaces the greedy steps consume; M = the largest n of S (0: S is empty).
struct Greedy {
  const unsigned char* lg;
  const unsigned char* cons;
  int M;
};
__device__ __forceinline__ long long consumed(const Greedy& g, long long r) {
  return g.M ? (r / g.M) * g.M + g.cons[r % g.M] : 0;
}
// Space k of a run of r, k < consumed(r): the length of the token that starts there, 0 inside a token.
__device__ __forceinline__ int token_at(const Greedy& g, long long r, long long k) {
  const long long q = (r / g.M) * g.M;
  if (k < q) return k % g.M == 0 ? g.M : 0;
  long long pos = q;
  for (;;) {
    const int n = g.lg[r - pos];   // r - pos < M here, and n > 0 because k < consumed(r)
    if (k == pos) return n;
    if (k < pos + n || n == 0) return 0;
    pos += n;
  }
}

// U+0020 bytes at the head / tail of the lane's 16 bytes (bytes at or beyond n_bytes are not spaces).
__device__ __forceinline__ void lane_runs(const unsigned char* __restrict__ t, long long b0, long long n_bytes, unsigned* lead, unsigned* trail) {
  unsigned m = 0;   // bit j: byte b0 + j is a space
  if (b0 < n_bytes) {
    const uint4 v = *reinterpret_cast<const uint4*>(t + b0);   // the buffer is 16-byte aligned and 16 bytes longer than the text
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < BPT; ++j)
      if (((w[j >> 2] >> ((j & 3) * 8)) & 0xFFu) == 0x20u && b0 + j < n_bytes) m |= 1u << j;
  }
  *lead = (unsigned)__builtin_ctz(~m & 0x1FFFFu | 0x10000u);
  *trail = (unsigned)__builtin_clz(~(m << 16) | 0x8000u);
}

__global__ __launch_bounds__(NT) void bpe_tile_runs_kernel(const unsigned char* __restrict__ text, long long n_bytes,
                                                           unsigned* __restrict__ tile_lead, unsigned* __restrict__ tile_trail) {
  __shared__ unsigned char s_lead[NT], s_trail[NT];
  const long long b0 = ((long long)blockIdx.x * NT + threadIdx.x) * BPT;
  unsigned lead, trail;
  lane_runs(text, b0, n_bytes, &lead, &trail);
  s_lead[threadIdx.x] = (unsigned char)lead;
  s_trail[threadIdx.x] = (unsigned char)trail;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned acc = 0;
    for (int m = 0; m < NT; ++m) {
      acc += s_lead[m];
      if (s_lead[m] < BPT) break;
    }
    tile_lead[blockIdx.x] = acc;
    acc = 0;
    for (int m = NT - 1; m >= 0; --m) {
      acc += s_trail[m];
      if (s_trail[m] < BPT) break;
    }
    tile_trail[blockIdx.x] = acc;
  }
}

// What the lanes of a bounds workgroup share about space runs.
struct Runs {
  const unsigned char* text;
  long long n_bytes, ts;              // ts = first byte of the tile
  const unsigned char* lead;          // LDS, per lane
  const unsigned char* trail;
  long long tile_back, tile_fwd;      // spaces right in front of / right behind the tile
};
// U+0020 bytes that end right in front of byte i, ts <= i <= ts + tile (document bounds not looked at).
__device__ __forceinline__ long long spaces_before(const Runs& R, long long i) {
  long long p = i;
  while ((p & (BPT - 1)) && R.text[p - 1] == 0x20u) --p;
  if (p & (BPT - 1)) return i - p;
  for (int m = (int)((p - R.ts) / BPT) - 1; m >= 0; --m) {
    const unsigned tr = R.trail[m];
    p -= tr;
    if (tr < BPT) return i - p;
  }
  return i - p + R.tile_back;
}
// U+0020 bytes from byte i + 1 on, ts <= i < ts + tile.
__device__ __forceinline__ long long spaces_after(const Runs& R, long long i) {
  long long p = i + 1;
  while ((p & (BPT - 1)) && p < R.n_bytes && R.text[p] == 0x20u) ++p;
  if (p & (BPT - 1)) return p - i - 1;
  for (int m = (int)((p - R.ts) / BPT); m < NT; ++m) {
    const unsigned ld = R.lead[m];
    p += ld;
    if (ld < BPT) return p - i - 1;
  }
  return p - i - 1 + R.tile_fwd;
}

__device__ __forceinline__ unsigned class_at(const unsigned char* __restrict__ t, long long j, long long hi) {
  int len;
  return cell_of(decode_at(t, j, hi, &len)) & 3u;
}

// What stands in front of the code point at byte i of the text [lo, hi): P_NONE at the start of a segment (the text's start, or
// behind a space-run token), P_SPACE for a U+0020 that is ordinary text, else the class of the code point.
__device__ __forceinline__ int prev_kind(const Runs& R, const Greedy& g, long long i, long long lo, long long hi, unsigned char* __restrict__ needs) {
  if (i <= lo) return P_NONE;
  if (R.text[i - 1] != 0x20u) return (int)class_at(R.text, prev_start(R.text, i, lo, hi), hi);
  long long r;
  if (i >= R.ts) {
    r = spaces_before(R, i);
  } else {   // up to 3 bytes in front of the tile (a contraction across its boundary): count byte by byte
    r = 0;
    while (i - r > lo && R.text[i - r - 1] == 0x20u) {
      if (++r > kSlowLookBack) {
        *needs = 1;
        return P_SPACE;
      }
    }
  }
  r = min(r, i - lo);
  return consumed(g, r) == r ? P_NONE : P_SPACE;
}

// Bytes of the contraction that the apostrophe at byte j begins ('s 't 'm 'd: 2; 're 've 'll: 3), 0 when there is none or the
// apostrophe is not active.
__device__ __forceinline__ int contraction_at(const Runs& R, const Greedy& g, long long j, long long lo, long long hi, unsigned char* __restrict__ needs) {
  const unsigned c1 = j + 1 < hi ? R.text[j + 1] : 0u, c2 = j + 2 < hi ? R.text[j + 2] : 0u;
  const int len = (c1 == 's' || c1 == 't' || c1 == 'm' || c1 == 'd') ? 2
                  : ((c1 == 'r' && c2 == 'e') || (c1 == 'v' && c2 == 'e') || (c1 == 'l' && c2 == 'l')) ? 3 : 0;
  if (!len) return 0;
  const int pk = prev_kind(R, g, j, lo, hi, needs);
  return (pk == P_NONE || pk == (int)C_L || pk == (int)C_N || pk == (int)C_W) ? len : 0;
}

// The letter at byte i: 1 = inside a contraction that began in front of it, 2 = a contraction ends right in front of it, 0 = neither.
__device__ __forceinline__ int contraction_state(const Runs& R, const Greedy& g, long long i, long long lo, long long hi, unsigned char* __restrict__ needs) {
  const unsigned char* t = R.text;
  if (i - 1 >= lo && t[i - 1] == '\'' && contraction_at(R, g, i - 1, lo, hi, needs)) return 1;
  if (i - 2 >= lo && t[i - 2] == '\'') {
    const int n = contraction_at(R, g, i - 2, lo, hi, needs);
    if (n) return n == 3 ? 1 : 2;
  }
  if (i - 3 >= lo && t[i - 3] == '\'' && contraction_at(R, g, i - 3, lo, hi, needs) == 3) return 2;
  return 0;
}

// EMIT = false: pre-tokens per workgroup (tile_cnt) and needs_host of every text the device cannot vouch for.
// EMIT = true: (start byte, text, is a space-run token) of every pre-token at its position in text order.
template <bool EMIT>
__global__ __launch_bounds__(NT) void bpe_bounds_kernel(const unsigned char* __restrict__ text, long long n_bytes,
                                                        const long long* __restrict__ off, int n_docs, int flags, Greedy g,
                                                        const unsigned* __restrict__ tile_lead, const unsigned* __restrict__ tile_trail,
                                                        long long n_tiles, unsigned* __restrict__ tile_cnt, unsigned char* __restrict__ needs,
                                                        const unsigned* __restrict__ tile_off, unsigned* __restrict__ wstart,
                                                        unsigned* __restrict__ wdoc, unsigned char* __restrict__ wspace) {
  __shared__ unsigned char s_lead[NT], s_trail[NT];
  __shared__ long long s_back, s_fwd;
  const long long ts = (long long)blockIdx.x * VRAG_BPE_TILE_BYTES;
  const long long b0 = ts + (long long)threadIdx.x * BPT;
  {
    unsigned lead, trail;
    lane_runs(text, b0, n_bytes, &lead, &trail);
    s_lead[threadIdx.x] = (unsigned char)lead;
    s_trail[threadIdx.x] = (unsigned char)trail;
  }
  if (threadIdx.x == 0) {
    long long acc = 0;
    int steps = 0;
    for (long long u = (long long)blockIdx.x - 1; u >= 0; --u) {
      const unsigned tr = tile_trail[u];
      acc += tr;
      if (tr < (unsigned)VRAG_BPE_TILE_BYTES) break;
      if (++steps > kMaxRunTiles) {
        if (!EMIT) needs[doc_of(off, n_docs, ts)] = 1;
        break;
      }
    }
    s_back = acc;
    acc = 0;
    steps = 0;
    for (long long u = (long long)blockIdx.x + 1; u < n_tiles; ++u) {
      const unsigned ld = tile_lead[u];
      acc += ld;
      if (ld < (unsigned)VRAG_BPE_TILE_BYTES) break;
      if (++steps > kMaxRunTiles) {
        if (!EMIT) needs[doc_of(off, n_docs, min(ts + VRAG_BPE_TILE_BYTES, n_bytes) - 1)] = 1;
        break;
      }
    }
    s_fwd = acc;
  }
  __syncthreads();
  Runs R{text, n_bytes, ts, s_lead, s_trail, s_back, s_fwd};
  const bool nfc = (flags & VRAG_BPE_NFC) != 0;
  unsigned starts = 0, spaces = 0;   // bit j: a pre-token starts at byte b0 + j / and it is a space-run token
  unsigned docs[BPT];
  if (b0 < n_bytes) {
    int d = doc_of(off, n_docs, b0);
    int pk = -1;       // what stands in front of the next code point; -1 = not known (looked up when needed)
    for (int j = 0; j < BPT && b0 + j < n_bytes; ++j) {
      const long long i = b0 + j;
      while (off[d + 1] <= i) ++d;
      docs[j] = (unsigned)d;
      const long long lo = off[d], hi = off[d + 1];
      if (i == lo) pk = P_NONE;
      if (!cp_start(text, i, lo, hi)) continue;
      unsigned char* nd = needs + d;
      unsigned char drop = 0;   // the emitting pass decides as the counting pass did; only the counting pass reports
      if (EMIT) nd = &drop;
      int len;
      const unsigned cp = decode_at(text, i, hi, &len);
      const unsigned cell = cell_of(cp);
      const unsigned cls = cell & 3u;
      if (!EMIT) {
        if (cell & C_NOTCOV) *nd = 1;
        if (nfc) {
          if (cell & C_QC) *nd = 1;
          const unsigned ccc = cell >> 8;
          if (ccc && i > lo) {
            int l2;
            const unsigned before = cell_of(decode_at(text, prev_start(text, i, lo, hi), hi, &l2)) >> 8;
            if (before > ccc) *nd = 1;
          }
        }
      }
      bool start;
      if (cp == 0x20u) {
        const long long B = min(spaces_before(R, i), i - lo), F = min(spaces_after(R, i), hi - i - 1);
        const long long r = B + 1 + F, k = B, c = consumed(g, r);
        if (k < c) {
          start = token_at(g, r, k) != 0;
          if (start) spaces |= 1u << j;
        } else {
          const bool prev_ws = k > c ? true : k > 0 ? false : (i > lo && class_at(text, prev_start(text, i, lo, hi), hi) == C_W);
          const bool next_text = k == r - 1 && i + 1 < hi && class_at(text, i + 1, hi) != C_W;
          start = !prev_ws || next_text;
        }
        pk = c == r ? P_NONE : P_SPACE;   // read by the code point behind the run only
      } else {
        if (pk < 0) pk = prev_kind(R, g, i, lo, hi, nd);
        if (cls == C_W) {
          const long long q = i + len;
          const bool next_text = q < hi && text[q] != 0x20u && class_at(text, q, hi) != C_W;
          start = !(pk == P_SPACE || pk == (int)C_W) || next_text;
        } else {
          const int cs = cls == C_L ? contraction_state(R, g, i, lo, hi, nd) : 0;
          start = cs == 1 ? false : cs == 2 ? true : !(pk == (int)cls || pk == P_SPACE);
        }
        pk = (int)cls;
      }
      if (start) starts |= 1u << j;
    }
  }
  unsigned total;
  unsigned pos = block_scan_256((unsigned)__popc(starts), &total);
  if (!EMIT) {
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
    return;
  }
  pos += tile_off[blockIdx.x];
#pragma unroll
  for (int j = 0; j < BPT; ++j)
    if ((starts >> j) & 1u) {
      wstart[pos] = (unsigned)(b0 + j);
      wdoc[pos] = docs[j];
      wspace[pos] = (unsigned char)((spaces >> j) & 1u);
      ++pos;
    }
}

// Code points in front of a byte, per text blob: lane[g] = lead bytes of the tile in front of 16-byte lane g, tile[u] = lead bytes in
// front of tile u.
struct LeadIndex {
  const unsigned* lane;
  const unsigned* tile;
};
// bit j: byte b0 + j is no continuation byte (b0 16-byte aligned, the buffer is 16 bytes longer than the text)
__device__ __forceinline__ unsigned lead_mask16(const unsigned char* __restrict__ t, long long b0) {
  const uint4 v = *reinterpret_cast<const uint4*>(t + b0);
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < BPT; ++j)
    if (((w[j >> 2] >> ((j & 3) * 8)) & 0xC0u) != 0x80u) m |= 1u << j;
  return m;
}
// Lead bytes among bytes 0 .. x of the blob (x < n_bytes).
__device__ __forceinline__ unsigned leads_upto(const unsigned char* __restrict__ t, const LeadIndex& li, long long x) {
  const long long g = x >> 4;
  return li.tile[x / VRAG_BPE_TILE_BYTES] + li.lane[g] + (unsigned)__popc(lead_mask16(t, g << 4) & ((2u << (unsigned)(x & 15)) - 1u));
}

__global__ __launch_bounds__(NT) void offsets_lead_count_kernel(const unsigned char* __restrict__ text, long long n_bytes,
                                                            unsigned* __restrict__ lane_lead, unsigned* __restrict__ tile_cnt) {
  const long long g = (long long)blockIdx.x * NT + threadIdx.x, b0 = g * BPT;
  unsigned m = 0;
  if (b0 < n_bytes) {
    m = lead_mask16(text, b0);
    if (n_bytes - b0 < BPT) m &= (1u << (unsigned)(n_bytes - b0)) - 1u;
  }
  unsigned total;
  const unsigned before = block_scan_256((unsigned)__popc(m), &total);
  if (b0 < n_bytes) lane_lead[g] = before;
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

struct Tables {
  const uint4* merges;          // {left, right, rank, merged}; left = 0xFFFFFFFF: empty; linear probing
  unsigned merge_mask;
  const int* byte_id;           // [256]
  const int* space_id;          // [65]
  const uint2* whole;           // {key, entry + 1} (0 = empty), linear probing; only with VRAG_BPE_IGNORE_MERGES
  unsigned whole_mask;
  const unsigned char* whole_blob;
  const unsigned* whole_off;
  const int* whole_id;
};

__device__ __forceinline__ unsigned wave_min(unsigned v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o, 64));
  return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}
__host__ __device__ inline unsigned pow_base(unsigned e) {
  unsigned p = 1u, b = kHashBase;
  for (; e; e >>= 1) {
    if (e & 1u) p *= b;
    b *= b;
  }
  return p;
}
// Key of a byte string in the `whole` table: sum of (byte + 1) * base^position, mixed with the length.
__host__ __device__ inline unsigned whole_key(unsigned sum, unsigned n) { return fmix32(sum + n * 0x9E3779B1u) | 1u; }

// One wave per pre-token (bpe_merge_kernel, offsets_merge_kernel): tok[wstart[w] + j] = its j-th id, tok_cnt[w] = how many, body[d] += tok_cnt[w].
// OFFS: span[wstart[w] + j] = the code points [start, end) of text d that hold the bytes of that id (include/vrag_amd.h).
template <bool OFFS>
__device__ __forceinline__ void merge_word(const unsigned char* __restrict__ text, const long long* __restrict__ off, int flags, const Tables& tb,
                                           const unsigned* __restrict__ wstart, const unsigned* __restrict__ wdoc,
                                           const unsigned char* __restrict__ wspace, long long n_words, int* __restrict__ tok,
                                           unsigned* __restrict__ tok_cnt, unsigned* __restrict__ body, unsigned char* __restrict__ needs,
                                           const LeadIndex& li, int2* __restrict__ span) {
  const int lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n_words) return;   // the whole wave leaves
  const unsigned d = wdoc[w];
  const long long b = wstart[w];
  const long long e = (w + 1 < n_words && wdoc[w + 1] == d) ? (long long)wstart[w + 1] : off[d + 1];
  const long long len = e - b;
  int* out = tok + b;
  // bytes [x0, x1) of the blob as code points of text d; base = code points of the blob in front of the text (wave-uniform)
  const unsigned base = OFFS && off[d] ? leads_upto(text, li, off[d] - 1) : 0u;
  auto cp_span = [&](long long x0, long long x1) {
    return make_int2((int)(leads_upto(text, li, x0) - 1u - base), (int)(leads_upto(text, li, x1 - 1) - base));
  };
  if (wspace[w]) {
    if (lane == 0) {
      if (OFFS) span[b] = cp_span(b, e);
      out[0] = tb.space_id[min(len, (long long)VRAG_BPE_MAX_SPACE_RUN)];
      tok_cnt[w] = 1u;
      atomicAdd(body + d, 1u);
    }
    return;
  }
  if (len > VRAG_BPE_MAX_WORD_BYTES || len <= 0) {
    if (lane == 0) {
      needs[d] = 1;
      tok_cnt[w] = 0u;
    }
    return;
  }
  int n = (int)len;
  const unsigned byte = lane < n ? text[b + lane] : 0u;
  if (flags & VRAG_BPE_IGNORE_MERGES) {
    const unsigned key = whole_key(wave_sum(lane < n ? (byte + 1u) * pow_base((unsigned)lane) : 0u), (unsigned)n);
    for (unsigned slot = key & tb.whole_mask;; slot = (slot + 1u) & tb.whole_mask) {
      const uint2 sl = tb.whole[slot];   // the same address in every lane
      if (sl.y == 0u) break;
      if (sl.x != key) continue;
      const unsigned a = tb.whole_off[sl.y - 1u], z = tb.whole_off[sl.y];
      const bool same = z - a == (unsigned)n && (lane >= n || tb.whole_blob[a + lane] == byte);
      if (__all(same)) {
        if (lane == 0) {
          if (OFFS) span[b] = cp_span(b, e);
          out[0] = tb.whole_id[sl.y - 1u];
          tok_cnt[w] = 1u;
          atomicAdd(body + d, 1u);
        }
        return;
      }
    }
  }
  unsigned sym = lane < n ? (unsigned)tb.byte_id[byte] : 0u;
  unsigned wid = lane < n ? 1u : 0u;   // OFFS: bytes of the lane's symbol
  while (n > 1) {
    const unsigned right = (unsigned)__shfl_down((int)sym, 1, 64);
    unsigned rank = kNoRank, merged = 0u;
    if (lane + 1 < n) {
      for (unsigned slot = pair_hash(sym, right) & tb.merge_mask;; slot = (slot + 1u) & tb.merge_mask) {
        const uint4 sl = tb.merges[slot];
        if (sl.x == 0xFFFFFFFFu) break;
        if (sl.x == sym && sl.y == right) {   // the full key: a collision cannot change an id
          rank = sl.z;
          merged = sl.w;
          break;
        }
      }
    }
    const unsigned best = wave_min(rank == kNoRank ? kNoRank : (rank << 6) | (unsigned)lane);
    if (best == kNoRank) break;
    const int at = (int)(best & 63u);
    const unsigned m = (unsigned)__shfl((int)merged, at, 64);
    sym = lane < at ? sym : lane == at ? m : right;
    if (OFFS) {
      const unsigned rw = (unsigned)__shfl_down((int)wid, 1, 64);
      wid = lane < at ? wid : lane == at ? wid + rw : rw;
    }
    --n;
  }
  if (lane < n) out[lane] = (int)sym;
  if (OFFS) {
    unsigned x = lane < n ? wid : 0u;   // inclusive wave prefix sum of the surviving widths
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned y = (unsigned)__shfl_up((int)x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane < n) span[b + lane] = cp_span(b + x - wid, b + x);
  }
  if (lane == 0) {
    tok_cnt[w] = (unsigned)n;
    atomicAdd(body + d, (unsigned)n);
  }
}

__global__ __launch_bounds__(256) void bpe_merge_kernel(const unsigned char* __restrict__ text, const long long* __restrict__ off, int flags,
                                                        Tables tb, const unsigned* __restrict__ wstart, const unsigned* __restrict__ wdoc,
                                                        const unsigned char* __restrict__ wspace, long long n_words, int* __restrict__ tok,
                                                        unsigned* __restrict__ tok_cnt, unsigned* __restrict__ body,
                                                        unsigned char* __restrict__ needs) {
  merge_word<false>(text, off, flags, tb, wstart, wdoc, wspace, n_words, tok, tok_cnt, body, needs, LeadIndex{nullptr, nullptr}, nullptr);
}
__global__ __launch_bounds__(256) void offsets_merge_kernel(const unsigned char* __restrict__ text, const long long* __restrict__ off, int flags,
                                                            Tables tb, const unsigned* __restrict__ wstart, const unsigned* __restrict__ wdoc,
                                                            const unsigned char* __restrict__ wspace, long long n_words, int* __restrict__ tok,
                                                            unsigned* __restrict__ tok_cnt, unsigned* __restrict__ body,
                                                            unsigned char* __restrict__ needs, LeadIndex li, int2* __restrict__ span) {
  merge_word<true>(text, off, flags, tb, wstart, wdoc, wspace, n_words, tok, tok_cnt, body, needs, li, span);
}

}  // namespace bpe
}  // namespace vrag

using namespace vrag;
using namespace vrag::bpe;

struct vrag_bpe : TokenizerBase {
  Tables tb{};
  Greedy greedy{};
  DevArray<uint4> merges;
  DevArray<int> byte_id, space_id, whole_id;
  DevArray<unsigned char> lg, cons, whole_blob;
  DevArray<uint2> whole;
  DevArray<unsigned> whole_off;
  // workspace of one call beside the frame's, grown on demand
  DevArray<unsigned char> wspace;
  DevArray<unsigned> tile_lead, tile_trail;
  // vrag_bpe_encode_offsets only
  DevArray<unsigned> lane_lead, tile_lead_cnt, tile_lead_off;
  DevArray<int2> span, offs;
};

extern "C" {

int vrag_bpe_create(int32_t n_vocab, const int32_t* merge_left, const int32_t* merge_right, const int32_t* merge_id, int32_t n_merges,
                    const int32_t* byte_id, const int32_t* space_run_id, const uint8_t* whole_blob, const int64_t* whole_off,
                    const int32_t* whole_id, int32_t n_whole, int32_t cls_id, int32_t sep_id, int32_t flags, int32_t device, vrag_bpe** out) {
  ARG_CHECK(out, "vrag_bpe_create: null out");
  *out = nullptr;
  ARG_CHECK(n_vocab > 0 && n_merges >= 0 && n_merges < (1 << 26) && byte_id && space_run_id && (n_merges == 0 || (merge_left && merge_right && merge_id)),
            "vrag_bpe_create: bad arguments");
  ARG_CHECK((flags & ~3) == 0, "vrag_bpe_create: unknown flags 0x%x", flags);
  ARG_CHECK(cls_id >= 0 && cls_id < n_vocab && sep_id >= 0 && sep_id < n_vocab, "vrag_bpe_create: cls / sep id outside the vocabulary of %d ids",
            n_vocab);
  const bool ignore = (flags & VRAG_BPE_IGNORE_MERGES) != 0;
  ARG_CHECK(n_whole >= 0 && (!ignore || n_whole == 0 || (whole_blob && whole_off && whole_id)), "vrag_bpe_create: bad whole-token arguments");
  if (!ignore) n_whole = 0;
  std::vector<int> bytes(byte_id, byte_id + 256), spaces(space_run_id, space_run_id + VRAG_BPE_MAX_SPACE_RUN + 1);
  for (int b = 0; b < 256; ++b) ARG_CHECK(bytes[b] >= 0 && bytes[b] < n_vocab, "vrag_bpe_create: byte_id[%d] outside the vocabulary", b);
  ARG_CHECK(spaces[0] < 0 && spaces[1] < 0, "vrag_bpe_create: space_run_id[0] and [1] must be -1");
  std::vector<unsigned char> lg(VRAG_BPE_MAX_SPACE_RUN + 1, 0), cons(VRAG_BPE_MAX_SPACE_RUN, 0);
  int M = 0;
  for (int n = 0; n <= VRAG_BPE_MAX_SPACE_RUN; ++n) {
    ARG_CHECK(spaces[n] < n_vocab, "vrag_bpe_create: space_run_id[%d] outside the vocabulary", n);
    if (spaces[n] >= 0) M = n;
    lg[n] = (unsigned char)M;
  }
  for (int x = 0; x < VRAG_BPE_MAX_SPACE_RUN; ++x) {
    int rem = x;
    while (lg[rem]) rem -= lg[rem];
    cons[x] = (unsigned char)(x - rem);
  }
  unsigned n_slots = 16;
  while (n_slots < 2u * (unsigned)n_merges) n_slots <<= 1;
  std::vector<uint4> slots(n_slots, make_uint4(0xFFFFFFFFu, 0u, 0u, 0u));
  for (int32_t r = 0; r < n_merges; ++r) {
    const int32_t a = merge_left[r], b = merge_right[r], m = merge_id[r];
    ARG_CHECK(a >= 0 && a < n_vocab && b >= 0 && b < n_vocab && m >= 0 && m < n_vocab, "vrag_bpe_create: merge %d has an id outside the vocabulary", r);
    unsigned slot = pair_hash((unsigned)a, (unsigned)b) & (n_slots - 1);
    for (; slots[slot].x != 0xFFFFFFFFu; slot = (slot + 1) & (n_slots - 1))
      ARG_CHECK(!(slots[slot].x == (unsigned)a && slots[slot].y == (unsigned)b), "vrag_bpe_create: merges %u and %d have the same pair", slots[slot].z, r);
    slots[slot] = make_uint4((unsigned)a, (unsigned)b, (unsigned)r, (unsigned)m);
  }
  unsigned w_slots = 16;
  while (w_slots < 2u * (unsigned)n_whole) w_slots <<= 1;
  std::vector<uint2> wslots(w_slots, make_uint2(0u, 0u));
  std::vector<unsigned> woff((size_t)n_whole + 1, 0u);
  std::vector<int> wid(whole_id, whole_id + n_whole);
  std::vector<unsigned char> wblob;
  if (n_whole) {
    ARG_CHECK(whole_off[0] == 0 && whole_off[n_whole] < 0x7FFFFFF0ll, "vrag_bpe_create: whole_off must start at 0 and stay below 2 GiB");
    for (int32_t i = 0; i < n_whole; ++i) {
      const int64_t a = whole_off[i], z = whole_off[i + 1];
      ARG_CHECK(z > a && z - a <= VRAG_BPE_MAX_WORD_BYTES, "vrag_bpe_create: whole entry %d must have 1..%d bytes", i, VRAG_BPE_MAX_WORD_BYTES);
      ARG_CHECK(wid[i] >= 0 && wid[i] < n_vocab, "vrag_bpe_create: whole_id[%d] outside the vocabulary", i);
      unsigned sum = 0;
      for (int64_t q = a; q < z; ++q) sum += (whole_blob[q] + 1u) * pow_base((unsigned)(q - a));
      const unsigned key = whole_key(sum, (unsigned)(z - a));
      unsigned slot = key & (w_slots - 1);
      for (; wslots[slot].y; slot = (slot + 1) & (w_slots - 1)) {
        const unsigned j = wslots[slot].y - 1;
        const bool same = whole_off[j + 1] - whole_off[j] == z - a && std::memcmp(whole_blob + whole_off[j], whole_blob + a, (size_t)(z - a)) == 0;
        ARG_CHECK(!same, "vrag_bpe_create: whole entries %u and %d are the same", j, i);
      }
      wslots[slot] = make_uint2(key, (unsigned)i + 1u);
      woff[i + 1] = (unsigned)z;
    }
    wblob.assign(whole_blob, whole_blob + whole_off[n_whole]);
  }
  DEVICE_CHECK(device);
  HIP_TRY(hipSetDevice(device));
  auto* h = new vrag_bpe();
  h->device = device;
  h->flags = flags;
  h->cls_id = cls_id;
  h->sep_id = sep_id;
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = upload(h->merges, slots, h->stream);
  if (e == hipSuccess) e = upload(h->byte_id, bytes, h->stream);
  if (e == hipSuccess) e = upload(h->space_id, spaces, h->stream);
  if (e == hipSuccess) e = upload(h->lg, lg, h->stream);
  if (e == hipSuccess) e = upload(h->cons, cons, h->stream);
  if (e == hipSuccess) e = upload(h->whole, wslots, h->stream);
  if (e == hipSuccess) e = upload(h->whole_off, woff, h->stream);
  if (e == hipSuccess) e = upload(h->whole_id, wid, h->stream);
  if (e == hipSuccess) e = upload(h->whole_blob, wblob, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    vrag_bpe_destroy(h);
    HIP_TRY(e);
  }
  h->tb = Tables{h->merges.p, n_slots - 1, h->byte_id.p, h->space_id.p, h->whole.p, w_slots - 1, h->whole_blob.p, h->whole_off.p, h->whole_id.p};
  h->greedy = Greedy{h->lg.p, h->cons.p, M};
  *out = h;
  return VRAG_OK;
}

void vrag_bpe_destroy(vrag_bpe* h) { tokenizer_destroy(h); }

// vrag_bpe_encode (offsets == nullptr, `fn` names the entry in messages) and vrag_bpe_encode_offsets.
static int bpe_encode(const char* fn, vrag_bpe* h, const EncodeArgs& a, int32_t* offsets) {
  const int n_docs = a.n_docs;
  auto count_pass = [&](hipStream_t st, long long n_bytes, long long n_tiles) -> int {
    HIP_TRY(h->tile_lead.grow((size_t)n_tiles));
    HIP_TRY(h->tile_trail.grow((size_t)n_tiles));
    hipLaunchKernelGGL(bpe_tile_runs_kernel, dim3((unsigned)n_tiles), dim3(NT), 0, st, h->text.p, n_bytes, h->tile_lead.p, h->tile_trail.p);
    hipLaunchKernelGGL(bpe_bounds_kernel<false>, dim3((unsigned)n_tiles), dim3(NT), 0, st, h->text.p, n_bytes, h->off.p, n_docs, h->flags,
                       h->greedy, h->tile_lead.p, h->tile_trail.p, n_tiles, h->tile_cnt.p, h->needs.p, (const unsigned*)nullptr,
                       (unsigned*)nullptr, (unsigned*)nullptr, (unsigned char*)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(scan_u32(h->tile_cnt.p, n_tiles, h->tile_off.p, st));
    if (offsets) {
      HIP_TRY(h->lane_lead.grow((size_t)n_tiles * NT));
      HIP_TRY(h->tile_lead_cnt.grow((size_t)n_tiles));
      HIP_TRY(h->tile_lead_off.grow((size_t)n_tiles + 1));
      hipLaunchKernelGGL(offsets_lead_count_kernel, dim3((unsigned)n_tiles), dim3(NT), 0, st, h->text.p, n_bytes, h->lane_lead.p, h->tile_lead_cnt.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(scan_u32(h->tile_lead_cnt.p, n_tiles, h->tile_lead_off.p, st));
    }
    return VRAG_OK;
  };
  auto word_pass = [&](hipStream_t st, long long n_bytes, long long n_tiles, long long n_words) -> int {
    HIP_TRY(h->wspace.grow((size_t)n_words));
    hipLaunchKernelGGL(bpe_bounds_kernel<true>, dim3((unsigned)n_tiles), dim3(NT), 0, st, h->text.p, n_bytes, h->off.p, n_docs, h->flags,
                       h->greedy, h->tile_lead.p, h->tile_trail.p, n_tiles, (unsigned*)nullptr, h->needs.p, h->tile_off.p, h->wstart.p,
                       h->wdoc.p, h->wspace.p);
    if (offsets) {
      HIP_TRY(h->span.grow((size_t)n_bytes));
      hipLaunchKernelGGL(offsets_merge_kernel, dim3(grid_of(n_words, 4)), dim3(256), 0, st, h->text.p, h->off.p, h->flags, h->tb, h->wstart.p,
                         h->wdoc.p, h->wspace.p, n_words, h->tok.p, h->tok_cnt.p, h->body.p, h->needs.p,
                         LeadIndex{h->lane_lead.p, h->tile_lead_off.p}, h->span.p);
    } else {
      hipLaunchKernelGGL(bpe_merge_kernel, dim3(grid_of(n_words, 4)), dim3(256), 0, st, h->text.p, h->off.p, h->flags, h->tb, h->wstart.p,
                         h->wdoc.p, h->wspace.p, n_words, h->tok.p, h->tok_cnt.p, h->body.p, h->needs.p);
    }
    return VRAG_OK;
  };
  ARG_CHECK(h, "%s: bad arguments", fn);
  const EncodeOffsets o{offsets, h->span, h->offs};
  return tokenizer_encode(fn, VRAG_BPE_MAX_BATCH_BYTES, VRAG_BPE_TILE_BYTES, h, a, offsets ? &o : nullptr, count_pass, word_pass);
}

int vrag_bpe_encode(vrag_bpe* h, const uint8_t* text, const int64_t* doc_off, int32_t n_docs, int32_t add_special_tokens, int32_t max_length,
                    int64_t cap, int32_t* ids, int32_t* seq_lens, uint8_t* needs_host, int64_t* n_ids) {
  return bpe_encode("vrag_bpe_encode", h, {text, doc_off, n_docs, add_special_tokens, max_length, cap, ids, seq_lens, needs_host, n_ids}, nullptr);
}

int vrag_bpe_encode_offsets(vrag_bpe* h, const uint8_t* text, const int64_t* doc_off, int32_t n_docs, int32_t add_special_tokens,
                            int32_t max_length, int64_t cap, int32_t* ids, int32_t* offsets, int32_t* seq_lens, uint8_t* needs_host,
                            int64_t* n_ids) {
  ARG_CHECK(offsets, "vrag_bpe_encode_offsets: null offsets");
  return bpe_encode("vrag_bpe_encode_offsets", h, {text, doc_off, n_docs, add_special_tokens, max_length, cap, ids, seq_lens, needs_host, n_ids},
                    offsets);
}

}  // extern "C"
