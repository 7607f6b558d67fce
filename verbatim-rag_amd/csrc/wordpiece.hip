// WordPiece tokenisation on gfx950 + C ABI: the ids HF `tokenizers` returns for BertNormalizer -> BertPreTokenizer ->
// WordPiece -> `[CLS] $A [SEP]` (include/vrag_amd.h states the rules).  One batch of UTF-8 texts (blob + doc_off):
//   words     wp_words_kernel<false / true>: 16 text bytes per lane, 4096 per workgroup.  Every code point is classed by the
//             committed table (wordpiece_table.inc): vanishes / separator / a word of its own / word character.  A lane
//             carries "inside a word" along its bytes; what it is at the lane's first byte comes from looking back over the
//             code points in front of it (one, unless vanished code points sit there), so a word or a multi-byte character may
//             straddle lanes and workgroups.  Counting pass, block scan + scan of the tile counts, then the same pass writes
//             (start byte, text) of every word in text order.
//   match     wp_match_kernel: one lane per word.  The word's normalised code points and their polynomial prefix hashes
//             live in the lane's scratch, so the hash of any [s, e) is two multiply-adds; greedy longest match probes an
//             open-addressing table {hash, id} in HBM and confirms every hit against the piece's stored bytes.  A word's
//             ids go to a scratch array at its start byte (a word never has more ids than source bytes).
//   pack      token_frame.h, shared with csrc/bpe.hip: tokenizer_encode checks and uploads the batch, calls the two passes above
//             and launches token_pack.h -- pack_seq_len_kernel (ids per text after truncation), scans, pack_gather_kernel (one
//             lane per word copies its ids that survive truncation), pack_special_kernel ([CLS] / [SEP]).
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
namespace wp {
#define WORDPIECE_TABLE_STORAGE static __device__ const
#include "wordpiece_table.inc"
#undef WORDPIECE_TABLE_STORAGE

constexpr unsigned C_WS = 1, C_PUNCT = 2, C_CJK = 4, C_NOTCOV = 8, C_REMOVE = 16, N_IDENT = 255;
constexpr int WP_NT = 256, WP_BPT = 16;
static_assert(WP_NT * WP_BPT == VRAG_WORDPIECE_TILE_BYTES, "the header exports the tile size");
constexpr int kMaxChars = VRAG_WP_MAX_CHARS_PER_WORD;
constexpr int kMaxPrefix = 16;    // bytes of the continuing-subword prefix
constexpr int kLookBack = 64;     // vanished code points a word-start decision looks back over before it gives the text up
constexpr unsigned kHashBase = 0x01000193u;

enum Kind { K_SKIP = 0, K_SEP = 1, K_SOLO = 2, K_WORD = 3 };

// The table word of code point cp under variant v: class | n << 8 | off << 16.
__device__ __forceinline__ unsigned rec_of(unsigned cp, int v) {
  const unsigned page = kWpPage[cp >> VRAG_WP_PAGE_SHIFT];
  const unsigned cell = kWpCell[(page << VRAG_WP_PAGE_SHIFT) | (cp & ((1u << VRAG_WP_PAGE_SHIFT) - 1u))];
  return kWpRec[cell][v];
}

__device__ __forceinline__ int kind_of(unsigned w, int flags, bool* notcov) {
  const unsigned cls = w & 0xFFu, n = (w >> 8) & 0xFFu;
  if (cls & C_NOTCOV) {
    *notcov = true;
    return K_SEP;   // the text goes to the host: its ids here are not used
  }
  if ((flags & VRAG_WP_CLEAN_TEXT) && (cls & C_REMOVE)) return K_SKIP;
  if (cls & C_WS) return K_SEP;
  if (n == 0u) return K_SKIP;
  if (((flags & VRAG_WP_CHINESE_CHARS) && (cls & C_CJK)) || (cls & C_PUNCT)) return K_SOLO;
  return K_WORD;
}

// Is the nearest code point in front of byte i that does not vanish a word character?  Gives the text up (needs_host)
// when more than kLookBack vanished code points sit there.
__device__ __forceinline__ bool in_word_before(const unsigned char* __restrict__ t, long long i, long long lo, long long hi, int v,
                                               int flags, unsigned char* __restrict__ needs) {
  long long j = i;
  for (int step = 0; j > lo; ++step) {
    if (step > kLookBack) {
      *needs = 1;
      return false;
    }
    j = prev_start(t, j, lo, hi);
    int len;
    bool nc = false;
    const int k = kind_of(rec_of(decode_at(t, j, hi, &len), v), flags, &nc);
    if (k != K_SKIP) return k == K_WORD;
  }
  return false;
}

// EMIT = false: words per workgroup (tile_cnt) and needs_host of every text with a code point the table does not cover.
// EMIT = true: (start byte, text) of every word at its position in text order (tile_off = exclusive scan of tile_cnt).
template <bool EMIT>
__global__ __launch_bounds__(WP_NT) void wp_words_kernel(const unsigned char* __restrict__ text, long long n_bytes,
                                                         const long long* __restrict__ off, int n_docs, int flags,
                                                         unsigned* __restrict__ tile_cnt, unsigned char* __restrict__ needs,
                                                         const unsigned* __restrict__ tile_off, unsigned* __restrict__ wstart,
                                                         unsigned* __restrict__ wdoc) {
  const long long b0 = ((long long)blockIdx.x * WP_NT + threadIdx.x) * WP_BPT;
  const int v = ((flags & VRAG_WP_STRIP_ACCENTS) ? 2 : 0) | ((flags & VRAG_WP_LOWERCASE) ? 1 : 0);
  unsigned starts = 0;   // bit j: a word starts at byte b0 + j
  unsigned docs[WP_BPT];
  if (b0 < n_bytes) {
    int d = doc_of(off, n_docs, b0);
    int state = -1;      // inside a word: 1 / 0, -1 = not known yet (decided by the code points in front of the lane)
    for (int j = 0; j < WP_BPT && b0 + j < n_bytes; ++j) {
      const long long i = b0 + j;
      while (off[d + 1] <= i) ++d;
      docs[j] = (unsigned)d;
      const long long lo = off[d], hi = off[d + 1];
      if (i == lo) state = 0;
      if (!cp_start(text, i, lo, hi)) continue;
      int len;
      bool nc = false;
      const int k = kind_of(rec_of(decode_at(text, i, hi, &len), v), flags, &nc);
      if (!EMIT && nc) needs[d] = 1;
      if (k == K_SKIP) continue;
      if (k == K_WORD) {
        if (state < 0) state = in_word_before(text, i, lo, hi, v, flags, needs + d) ? 1 : 0;
        if (state == 0) starts |= 1u << j;
        state = 1;
      } else {
        if (k == K_SOLO) starts |= 1u << j;
        state = 0;
      }
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
  for (int j = 0; j < WP_BPT; ++j)
    if ((starts >> j) & 1u) {
      wstart[pos] = (unsigned)(b0 + j);
      wdoc[pos] = docs[j];
      ++pos;
    }
}

struct Vocab {
  const unsigned char* blob;      // the pieces' UTF-8, back to back
  const unsigned* piece_off;      // [n_vocab + 1]
  const uint2* slots;             // {hash, id + 1} (0 = empty), linear probing
  const unsigned* pw;             // kHashBase ^ k, k <= kMaxChars
  unsigned mask;
  unsigned prefix_hash, prefix_cps, prefix_len;
  unsigned char prefix[kMaxPrefix];
  int max_piece_cps, max_chars, unk_id;
};

__host__ __device__ inline unsigned fmix32(unsigned h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
// Polynomial hash of a code point sequence: h <- h * base + (cp + 1); the table key mixes the length in.
__host__ __device__ inline unsigned hash_step(unsigned h, unsigned cp) { return h * kHashBase + (cp + 1u); }
__host__ __device__ inline unsigned hash_key(unsigned h, unsigned n_cps) { return fmix32(h + n_cps * 0x9E3779B1u); }

// Do the stored bytes of piece `id` equal [prefix +] UTF-8 of cps[s .. e)?
__device__ __forceinline__ bool piece_equals(const Vocab& vc, unsigned id, const unsigned* cps, int s, int e, bool with_prefix) {
  const unsigned char* p = vc.blob + vc.piece_off[id];
  const unsigned plen = vc.piece_off[id + 1] - vc.piece_off[id];
  unsigned at = 0;
  if (with_prefix) {
    if (plen < vc.prefix_len) return false;
    for (; at < vc.prefix_len; ++at)
      if (p[at] != vc.prefix[at]) return false;
  }
  for (int i = s; i < e; ++i) {
    const unsigned cp = cps[i];
    unsigned char b[4];
    unsigned n;
    if (cp < 0x80u) {
      b[0] = (unsigned char)cp;
      n = 1;
    } else if (cp < 0x800u) {
      b[0] = (unsigned char)(0xC0u | (cp >> 6));
      b[1] = (unsigned char)(0x80u | (cp & 0x3Fu));
      n = 2;
    } else if (cp < 0x10000u) {
      b[0] = (unsigned char)(0xE0u | (cp >> 12));
      b[1] = (unsigned char)(0x80u | ((cp >> 6) & 0x3Fu));
      b[2] = (unsigned char)(0x80u | (cp & 0x3Fu));
      n = 3;
    } else {
      b[0] = (unsigned char)(0xF0u | (cp >> 18));
      b[1] = (unsigned char)(0x80u | ((cp >> 12) & 0x3Fu));
      b[2] = (unsigned char)(0x80u | ((cp >> 6) & 0x3Fu));
      b[3] = (unsigned char)(0x80u | (cp & 0x3Fu));
      n = 4;
    }
    if (at + n > plen) return false;
    for (unsigned q = 0; q < n; ++q)
      if (p[at + q] != b[q]) return false;
    at += n;
  }
  return at == plen;
}

// One lane per word: tok[wstart[w] + j] = its j-th id, tok_cnt[w] = how many, body[d] += tok_cnt[w].
__global__ __launch_bounds__(256) void wp_match_kernel(const unsigned char* __restrict__ text, long long n_bytes,
                                                       const long long* __restrict__ off, int flags, Vocab vc,
                                                       const unsigned* __restrict__ wstart, const unsigned* __restrict__ wdoc,
                                                       long long n_words, int* __restrict__ tok, unsigned* __restrict__ tok_cnt,
                                                       unsigned* __restrict__ body) {
  const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_words) return;
  const int v = ((flags & VRAG_WP_STRIP_ACCENTS) ? 2 : 0) | ((flags & VRAG_WP_LOWERCASE) ? 1 : 0);
  const long long b = wstart[w];
  const unsigned d = wdoc[w];
  const long long hi = off[d + 1];
  unsigned cps[kMaxChars];
  unsigned pre[kMaxChars + 1];   // pre[k] = polynomial hash of cps[0 .. k)
  int n = 0;                     // code points of the word (counted beyond the buffer as well)
  long long i = b;
  while (i < hi) {
    int len;
    bool nc = false;
    const unsigned cp = decode_at(text, i, hi, &len);
    const unsigned r = rec_of(cp, v);
    const int k = kind_of(r, flags, &nc);
    i += len;
    if (k == K_SKIP) continue;
    if (k == K_SEP || (k == K_SOLO && n > 0)) break;
    const unsigned cnt = (r >> 8) & 0xFFu;
    if (cnt == N_IDENT) {
      if (n < kMaxChars) cps[n] = cp;
      ++n;
    } else {
      for (unsigned q = 0; q < cnt; ++q) {
        if (n < kMaxChars) cps[n] = kWpOut[(r >> 16) + q];
        ++n;
      }
    }
    if (k == K_SOLO) break;
  }
  int* out = tok + b;
  const long long room = n_bytes - b;   // a word has no more ids than source bytes; never write past the scratch
  unsigned n_tok = 0;
  bool bad = n > vc.max_chars || n == 0;
  if (!bad) {
    pre[0] = 0u;
    for (int q = 0; q < n; ++q) pre[q + 1] = hash_step(pre[q], cps[q]);
    int s = 0;
    while (s < n && !bad) {
      const bool cont = s > 0;
      int e = min(n, s + vc.max_piece_cps);
      int hit = -1;
      for (; e > s; --e) {
        const unsigned len = (unsigned)(e - s);
        unsigned h = pre[e] - pre[s] * vc.pw[len];
        unsigned total = len;
        if (cont) {
          h += vc.prefix_hash * vc.pw[len];
          total += vc.prefix_cps;
        }
        const unsigned key = hash_key(h, total);
        for (unsigned slot = key & vc.mask;; slot = (slot + 1u) & vc.mask) {
          const uint2 sl = vc.slots[slot];
          if (sl.y == 0u) break;
          if (sl.x == key && piece_equals(vc, sl.y - 1u, cps, s, e, cont)) {
            hit = (int)(sl.y - 1u);
            break;
          }
        }
        if (hit >= 0) break;
      }
      if (hit < 0) {
        bad = true;
      } else {
        if ((long long)n_tok < room) out[n_tok] = hit;
        ++n_tok;
        s = e;
      }
    }
  }
  if (bad) {
    n_tok = n == 0 ? 0u : 1u;
    if (n_tok && room > 0) out[0] = vc.unk_id;
  }
  tok_cnt[w] = n_tok;
  if (n_tok) atomicAdd(body + d, n_tok);
}

}  // namespace wp
}  // namespace vrag

using namespace vrag;
using namespace vrag::wp;

struct vrag_wordpiece : TokenizerBase {
  Vocab vc{};
  DevArray<unsigned char> blob;
  DevArray<unsigned> piece_off, pw;
  DevArray<uint2> slots;
};

namespace {

// Strict UTF-8 of one piece -> code points; false when malformed.
bool decode_piece(const uint8_t* p, size_t n, std::vector<unsigned>& out) {
  out.clear();
  for (size_t i = 0; i < n;) {
    const unsigned c = p[i];
    int need;
    unsigned cp;
    if (c < 0x80u) {
      need = 0, cp = c;
    } else if (c >= 0xC2u && c < 0xE0u) {
      need = 1, cp = c & 0x1Fu;
    } else if (c >= 0xE0u && c < 0xF0u) {
      need = 2, cp = c & 0x0Fu;
    } else if (c >= 0xF0u && c < 0xF5u) {
      need = 3, cp = c & 0x07u;
    } else {
      return false;
    }
    if (i + need >= n + (need ? 0 : 1)) return false;
    for (int k = 1; k <= need; ++k) {
      if ((p[i + k] & 0xC0u) != 0x80u) return false;
      cp = (cp << 6) | (p[i + k] & 0x3Fu);
    }
    const unsigned least = need <= 1 ? (need ? 0x80u : 0u) : need == 2 ? 0x800u : 0x10000u;
    if (cp < least || (cp >= 0xD800u && cp <= 0xDFFFu) || cp > 0x10FFFFu) return false;
    out.push_back(cp);
    i += 1 + need;
  }
  return true;
}

unsigned hash_of(const std::vector<unsigned>& cps) {
  unsigned h = 0;
  for (unsigned cp : cps) h = hash_step(h, cp);
  return h;
}

}  // namespace

extern "C" {

int vrag_wordpiece_create(const uint8_t* vocab_blob, const int64_t* piece_off, int32_t n_vocab, int32_t unk_id, int32_t cls_id,
                          int32_t sep_id, const char* prefix, int32_t max_chars_per_word, int32_t flags, int32_t device,
                          vrag_wordpiece** out) {
  ARG_CHECK(out, "vrag_wordpiece_create: null out");
  *out = nullptr;
  ARG_CHECK(vocab_blob && piece_off && prefix && n_vocab > 0, "vrag_wordpiece_create: bad arguments");
  ARG_CHECK(unk_id >= 0 && unk_id < n_vocab && cls_id >= 0 && cls_id < n_vocab && sep_id >= 0 && sep_id < n_vocab,
            "vrag_wordpiece_create: unk / cls / sep id outside the vocabulary of %d pieces", n_vocab);
  ARG_CHECK(max_chars_per_word >= 1 && max_chars_per_word <= kMaxChars, "vrag_wordpiece_create: max_chars_per_word must be in 1..%d, got %d",
            kMaxChars, max_chars_per_word);
  ARG_CHECK((flags & ~15) == 0, "vrag_wordpiece_create: unknown flags 0x%x", flags);
  const size_t prefix_len = std::strlen(prefix);
  ARG_CHECK(prefix_len <= (size_t)kMaxPrefix, "vrag_wordpiece_create: the prefix has more than %d bytes", kMaxPrefix);
  ARG_CHECK(piece_off[0] == 0 && piece_off[n_vocab] < 0xFFFFFFF0ll, "vrag_wordpiece_create: piece_off must start at 0 and stay below 4 GiB");
  std::vector<unsigned> cps, pcps;
  ARG_CHECK(decode_piece(reinterpret_cast<const uint8_t*>(prefix), prefix_len, pcps), "vrag_wordpiece_create: the prefix is not UTF-8");
  unsigned n_slots = 16;
  while (n_slots < 2u * (unsigned)n_vocab) n_slots <<= 1;
  std::vector<uint2> slots(n_slots, make_uint2(0u, 0u));
  std::vector<unsigned> off32((size_t)n_vocab + 1);
  int max_piece = 1;
  for (int32_t i = 0; i < n_vocab; ++i) {
    const int64_t a = piece_off[i], b = piece_off[i + 1];
    ARG_CHECK(b > a, "vrag_wordpiece_create: piece %d is empty or piece_off decreases", i);
    ARG_CHECK(decode_piece(vocab_blob + a, (size_t)(b - a), cps), "vrag_wordpiece_create: piece %d is not well-formed UTF-8", i);
    max_piece = std::max(max_piece, (int)cps.size());
    const unsigned key = hash_key(hash_of(cps), (unsigned)cps.size());
    unsigned slot = key & (n_slots - 1);
    for (; slots[slot].y; slot = (slot + 1) & (n_slots - 1)) {
      const unsigned j = slots[slot].y - 1;
      const bool same = slots[slot].x == key && piece_off[j + 1] - piece_off[j] == b - a &&
                        std::memcmp(vocab_blob + piece_off[j], vocab_blob + a, (size_t)(b - a)) == 0;
      ARG_CHECK(!same, "vrag_wordpiece_create: pieces %u and %d are the same", j, i);
    }
    slots[slot] = make_uint2(key, (unsigned)i + 1u);
    off32[i] = (unsigned)a;
  }
  off32[n_vocab] = (unsigned)piece_off[n_vocab];
  std::vector<unsigned> pw(kMaxChars + 1);
  pw[0] = 1u;
  for (int k = 1; k <= kMaxChars; ++k) pw[k] = pw[k - 1] * kHashBase;
  DEVICE_CHECK(device);
  HIP_TRY(hipSetDevice(device));
  auto* h = new vrag_wordpiece();
  h->device = device;
  h->flags = flags;
  h->cls_id = cls_id;
  h->sep_id = sep_id;
  const std::vector<unsigned char> blob(vocab_blob, vocab_blob + piece_off[n_vocab]);
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = upload(h->blob, blob, h->stream);
  if (e == hipSuccess) e = upload(h->piece_off, off32, h->stream);
  if (e == hipSuccess) e = upload(h->pw, pw, h->stream);
  if (e == hipSuccess) e = upload(h->slots, slots, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    vrag_wordpiece_destroy(h);
    HIP_TRY(e);
  }
  Vocab& vc = h->vc;
  vc.blob = h->blob.p;
  vc.piece_off = h->piece_off.p;
  vc.slots = h->slots.p;
  vc.pw = h->pw.p;
  vc.mask = n_slots - 1;
  vc.prefix_hash = hash_of(pcps);
  vc.prefix_cps = (unsigned)pcps.size();
  vc.prefix_len = (unsigned)prefix_len;
  std::memcpy(vc.prefix, prefix, prefix_len);
  vc.max_piece_cps = max_piece;
  vc.max_chars = max_chars_per_word;
  vc.unk_id = unk_id;
  *out = h;
  return VRAG_OK;
}

void vrag_wordpiece_destroy(vrag_wordpiece* h) { tokenizer_destroy(h); }

int vrag_wordpiece_encode(vrag_wordpiece* h, const uint8_t* text, const int64_t* doc_off, int32_t n_docs, int32_t add_special_tokens,
                          int32_t max_length, int64_t cap, int32_t* ids, int32_t* seq_lens, uint8_t* needs_host, int64_t* n_ids) {
  auto count_pass = [&](hipStream_t st, long long n_bytes, long long n_tiles) -> int {
    hipLaunchKernelGGL(wp_words_kernel<false>, dim3((unsigned)n_tiles), dim3(WP_NT), 0, st, h->text.p, n_bytes, h->off.p, (int)n_docs, h->flags,
                       h->tile_cnt.p, h->needs.p, (const unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(scan_u32(h->tile_cnt.p, n_tiles, h->tile_off.p, st));
    return VRAG_OK;
  };
  auto word_pass = [&](hipStream_t st, long long n_bytes, long long n_tiles, long long n_words) -> int {
    hipLaunchKernelGGL(wp_words_kernel<true>, dim3((unsigned)n_tiles), dim3(WP_NT), 0, st, h->text.p, n_bytes, h->off.p, (int)n_docs, h->flags,
                       (unsigned*)nullptr, h->needs.p, h->tile_off.p, h->wstart.p, h->wdoc.p);
    hipLaunchKernelGGL(wp_match_kernel, dim3(grid_of(n_words, 256)), dim3(256), 0, st, h->text.p, n_bytes, h->off.p, h->flags, h->vc,
                       h->wstart.p, h->wdoc.p, n_words, h->tok.p, h->tok_cnt.p, h->body.p);
    return VRAG_OK;
  };
  return tokenizer_encode("vrag_wordpiece_encode", VRAG_WP_MAX_BATCH_BYTES, VRAG_WORDPIECE_TILE_BYTES, h,
                          {text, doc_off, n_docs, add_special_tokens, max_length, cap, ids, seq_lens, needs_host, n_ids}, nullptr,
                          count_pass, word_pass);
}

}  // extern "C"
