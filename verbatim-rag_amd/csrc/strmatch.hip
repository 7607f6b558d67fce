// String leaves of the row filter answered on the device: the columns' string dictionaries in HBM and the kernel that makes a
// leaf's answer table from one (include/vrag_amd.h, vrag_row_filter_append_strings / _strings / _match; csrc/rowfilter.hip launches
// the same kernel from vrag_row_filter_eval_matched).
//
// What it replaces: store_columns.MetaColumn.string_table applies a comparison in Python once per DISTINCT stored string for every
// new (operator, text).  That is the right shape for `source != "web"` and the wrong one for what LIKE is used on -- titles, paths,
// ids -- where there are about as many distinct strings as rows.
//
// str_match_kernel: one lane per dictionary string, one wave per group of 64 codes, waves stride over the groups.
//   program   the operand (comparisons) or the compiled pattern (LIKE) is a by-value kernel argument, copied to LDS once per
//             workgroup: lanes stand at different positions of it, so it is indexed divergently -- a private array indexed at run
//             time would go to scratch, the scalar cache serves only wave-uniform reads
//   compare   bytewise, a proper prefix is smaller: for valid UTF-8 that is the order of the code points, Python's str order
//   LIKE      no backtracking.  The pattern is split at its unescaped `%` into segments of literal bytes and `_`; every segment
//             consumes a fixed number of code points, so the leftmost match of a segment also ends earliest, and taking it is
//             exact.  A first segment not behind a `%` matches at byte 0; each floating segment at the leftmost code-point boundary
//             at or behind the current position; a last segment not in front of a `%` is placed by walking its code points back
//             from the string's end and must start at or behind the current position.  `_` consumes one lead byte and its
//             continuation bytes (10xxxxxx).  The host has validated both sides as UTF-8, so literal bytes compare whole code points
//   result    the wave's 64 answers are one ballot; lanes 0 and 1 store its two words, the second only where the table has it (a
//             table of n codes is ceil(n / 32) words, and the next leaf's table may follow directly).  Lanes at and beyond n_codes
//             read nothing and are masked out of the ballot: the tail bits of the last word are zero
// A single very long string makes one lane walk alone while its wave waits; profiles/like_filter_probe.txt has what that costs.
#include "../../include/vrag_amd.h"

#include <algorithm>
#include <vector>

#include "rowfilter.h"

namespace vrag {
namespace {

constexpr int SM_WAVES = 4;   // waves of a workgroup
constexpr int SM_MAX_BLOCKS = 4096;
constexpr int SM_PROG_WORDS = (int)(sizeof(MatchProg) / 4);

__device__ __forceinline__ bool is_continuation(unsigned b) { return (b & 0xC0u) == 0x80u; }

// Segment `seg` at byte `at` of s[0 .. len) (a code-point boundary): true and `end` = the byte behind it, or false.
__device__ __forceinline__ bool segment_at(const MatchProg& p, int seg, const unsigned char* __restrict__ s, int len, int at, int& end) {
  int q = at;
  const int e1 = p.seg_begin[seg + 1];
  for (int e = p.seg_begin[seg]; e < e1; ++e) {
    if (q >= len) return false;
    const unsigned want = p.elem[e];
    if (want == MATCH_ANY_ONE) {
      ++q;
      while (q < len && is_continuation(s[q])) ++q;
    } else {
      if (s[q] != want) return false;
      ++q;
    }
  }
  end = q;
  return true;
}

__device__ bool like_answer(const MatchProg& p, const unsigned char* __restrict__ s, int len) {
  int pos = 0;
  if (!(p.flags & MATCH_HAS_PCT)) return segment_at(p, 0, s, len, 0, pos) && pos == len;
  int seg = 0;
  if (p.flags & MATCH_FRONT) {
    if (!segment_at(p, 0, s, len, 0, pos)) return false;
    seg = 1;
  }
  const int floating_end = (p.flags & MATCH_BACK) ? p.n_seg - 1 : p.n_seg;
  for (; seg < floating_end; ++seg) {
    int start = pos;
    for (;;) {
      if (segment_at(p, seg, s, len, start, pos)) break;
      if (start >= len) return false;
      ++start;
      while (start < len && is_continuation(s[start])) ++start;
    }
  }
  if (p.flags & MATCH_BACK) {
    int start = len;
    for (int k = p.seg_cp[p.n_seg - 1]; k > 0; --k) {
      if (start <= pos) return false;   // fewer code points left than the segment consumes
      --start;
      while (start > pos && is_continuation(s[start])) --start;
    }
    int end = 0;
    return start >= pos && segment_at(p, p.n_seg - 1, s, len, start, end) && end == len;
  }
  return true;
}

__device__ bool compare_answer(const MatchProg& p, const unsigned char* __restrict__ s, int len) {
  const int m = len < p.text_len ? len : p.text_len;
  int i = 0;
  while (i < m && s[i] == p.elem[i]) ++i;
  const int c = i < m ? (int)s[i] - (int)p.elem[i] : len - p.text_len;   // < 0, 0, > 0
  switch (p.op) {   // wave-uniform
    case VRAG_FILTER_MATCH_EQ: return c == 0;
    case VRAG_FILTER_MATCH_NE: return c != 0;
    case VRAG_FILTER_MATCH_LT: return c < 0;
    case VRAG_FILTER_MATCH_LE: return c <= 0;
    case VRAG_FILTER_MATCH_GT: return c > 0;
    default: return c >= 0;
  }
}

__global__ __launch_bounds__(64 * SM_WAVES) void str_match_kernel(const MatchProg a, const unsigned char* __restrict__ bytes,
                                                                   const long long* __restrict__ off, long long n_codes,
                                                                   long long n_groups, long long n_words, unsigned* __restrict__ out) {
  __shared__ MatchProg p;
  {
    const unsigned* src = reinterpret_cast<const unsigned*>(&a);
    unsigned* dst = reinterpret_cast<unsigned*>(&p);
    for (int i = threadIdx.x; i < SM_PROG_WORDS; i += 64 * SM_WAVES) dst[i] = src[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * SM_WAVES;
  for (long long g = (long long)blockIdx.x * SM_WAVES + (threadIdx.x >> 6); g < n_groups; g += stride) {
    const long long c = g * 64 + lane;
    bool hit = false;
    if (c < n_codes) {
      const long long b0 = off[c];
      const int len = (int)(off[c + 1] - b0);   // < 2 GiB per string, checked when it was appended
      const unsigned char* s = bytes + b0;
      hit = p.op == VRAG_FILTER_MATCH_LIKE ? like_answer(p, s, len) : compare_answer(p, s, len);
    }
    const u64 m = __ballot(hit);   // every lane of the wave is here: the group loop is wave-uniform
    if (lane == 0) out[2 * g] = (unsigned)(m & 0xffffffffull);
    if (lane == 1 && 2 * g + 1 < n_words) out[2 * g + 1] = (unsigned)(m >> 32);
  }
}

// Strict UTF-8: no overlong forms, no surrogates, nothing above U+10FFFF.  Returns the offset of the first bad byte, or -1.
long long utf8_bad_at(const uint8_t* s, long long n) {
  long long i = 0;
  while (i < n) {
    const unsigned b = s[i];
    int more;
    unsigned lo = 0x80, hi = 0xBF;
    if (b < 0x80) more = 0;
    else if (b >= 0xC2 && b <= 0xDF) more = 1;
    else if (b >= 0xE0 && b <= 0xEF) more = 2, lo = b == 0xE0 ? 0xA0 : 0x80, hi = b == 0xED ? 0x9F : 0xBF;
    else if (b >= 0xF0 && b <= 0xF4) more = 3, lo = b == 0xF0 ? 0x90 : 0x80, hi = b == 0xF4 ? 0x8F : 0xBF;
    else return i;
    if (more > n - i - 1) return i;
    for (int k = 1; k <= more; ++k) {
      const unsigned cb = s[i + k];
      if (cb < (k == 1 ? lo : 0x80u) || cb > (k == 1 ? hi : 0xBFu)) return i;
    }
    i += 1 + more;
  }
  return -1;
}

// Device array `a` holding `have` elements grown to hold `need`: geometric, the elements held move into the new array.
template <typename T>
int grow_keeping(DevArray<T>& a, size_t have, size_t need, size_t least, hipStream_t st) {
  if (need <= a.n) return VRAG_OK;
  DevArray<T> bigger;
  HIP_TRY(bigger.grow(std::max<size_t>(need, std::max<size_t>(2 * a.n, least))));
  if (have) {
    HIP_TRY(hipMemcpyAsync(bigger.p, a.p, have * sizeof(T), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // the old array is freed by the assignment below
  }
  a = std::move(bigger);
  return VRAG_OK;
}

}  // namespace

int match_compile(const char* who, int32_t op, const uint8_t* text, int32_t text_len, MatchProg* out) {
  ARG_CHECK(op >= VRAG_FILTER_MATCH_EQ && op <= VRAG_FILTER_MATCH_LIKE, "%s: %d is no VRAG_FILTER_MATCH_* operator", who, op);
  ARG_CHECK(text_len >= 0 && (text_len == 0 || text), "%s: bad operand text (%d bytes)", who, text_len);
  ARG_CHECK(text_len <= VRAG_FILTER_MATCH_MAX_PATTERN, "%s: the operand text has %d bytes (at most %d)", who, text_len,
            VRAG_FILTER_MATCH_MAX_PATTERN);
  const long long bad = utf8_bad_at(text, text_len);
  ARG_CHECK(bad < 0, "%s: the operand text is not valid UTF-8 at byte %lld", who, bad);
  MatchProg p = {};
  p.op = op;
  if (op != VRAG_FILTER_MATCH_LIKE) {
    p.text_len = text_len;
    std::copy(text, text + text_len, p.elem);
    *out = p;
    return VRAG_OK;
  }
  int n_elem = 0, seg_elems = 0, seg_cp = 0;
  bool last_was_pct = false;
  auto close_segment = [&]() {
    if (seg_elems) {   // empty runs (`%%`, a leading or trailing `%`) are no segments
      p.seg_cp[p.n_seg] = (unsigned short)seg_cp;
      p.seg_begin[++p.n_seg] = (unsigned short)n_elem;
    }
    seg_elems = seg_cp = 0;
  };
  for (int i = 0; i < text_len; ++i) {
    unsigned char b = text[i];
    last_was_pct = false;
    if (b == '%') {
      close_segment();
      p.flags |= MATCH_HAS_PCT;
      last_was_pct = true;
      continue;
    }
    bool literal = true;
    if (b == '\\') {
      ARG_CHECK(i + 1 < text_len, "%s: the LIKE pattern ends in a lone backslash", who);
      b = text[++i];
    } else if (b == '_') {
      literal = false;
    }
    if (seg_elems == 0)
      ARG_CHECK(p.n_seg < VRAG_FILTER_MATCH_MAX_SEGMENTS, "%s: the LIKE pattern has more than %d segments between its %%", who,
                VRAG_FILTER_MATCH_MAX_SEGMENTS);
    p.elem[n_elem++] = literal ? b : MATCH_ANY_ONE;
    ++seg_elems;
    seg_cp += literal ? ((b & 0xC0u) != 0x80u) : 1;
  }
  const bool leading_pct = text_len > 0 && text[0] == '%';
  if (!(p.flags & MATCH_HAS_PCT)) {
    p.seg_cp[0] = (unsigned short)seg_cp;   // the one segment, possibly empty: the whole string
    p.seg_begin[1] = (unsigned short)n_elem;
    p.n_seg = 1;
    p.flags = MATCH_FRONT | MATCH_BACK;
  } else {
    close_segment();
    if (!leading_pct) p.flags |= MATCH_FRONT;
    if (!last_was_pct) p.flags |= MATCH_BACK;
  }
  *out = p;
  return VRAG_OK;
}

hipError_t match_launch(const FilterColumn& c, const MatchProg& prog, long long n_codes, unsigned* d_words, hipStream_t st) {
  if (n_codes <= 0) return hipSuccess;
  const long long n_groups = (n_codes + 63) / 64, n_words = (n_codes + 31) / 32;
  const unsigned blocks = (unsigned)std::min<long long>((n_groups + SM_WAVES - 1) / SM_WAVES, SM_MAX_BLOCKS);
  hipLaunchKernelGGL(str_match_kernel, dim3(blocks), dim3(64 * SM_WAVES), 0, st, prog, c.str_bytes.p, c.str_off.p, n_codes, n_groups,
                     n_words, d_words);
  return hipGetLastError();
}

}  // namespace vrag

using namespace vrag;

extern "C" {

int vrag_row_filter_append_strings(vrag_row_filter* f, int32_t col, const uint8_t* bytes, const int64_t* off, int64_t n) {
  ARG_CHECK(f, "null argument");
  ARG_CHECK(n >= 0 && (n == 0 || off), "vrag_row_filter_append_strings: need n >= 0 and the offsets");
  std::lock_guard<std::mutex> lk(f->mu);
  ARG_CHECK(col >= 0 && col < (int)f->cols.size(), "vrag_row_filter_append_strings: no column %d (the filter holds %d)", col,
            (int)f->cols.size());
  if (n == 0) return VRAG_OK;
  ARG_CHECK(off[0] == 0, "vrag_row_filter_append_strings: off[0] = %lld (must be 0)", (long long)off[0]);
  for (int64_t i = 0; i < n; ++i)
    ARG_CHECK(off[i + 1] >= off[i] && off[i + 1] - off[i] <= 0x7fffffffll,
              "vrag_row_filter_append_strings: off[%lld] = %lld behind off[%lld] = %lld (offsets ascend; a string is shorter than 2 GiB)",
              (long long)i + 1, (long long)off[i + 1], (long long)i, (long long)off[i]);
  const int64_t n_new = off[n];
  ARG_CHECK(n_new == 0 || bytes, "vrag_row_filter_append_strings: null bytes");
  for (int64_t i = 0; i < n; ++i) {   // per string: a boundary between two strings is a boundary between two code points
    const long long bad = utf8_bad_at(bytes + off[i], off[i + 1] - off[i]);
    ARG_CHECK(bad < 0, "vrag_row_filter_append_strings: string %lld is not valid UTF-8 at its byte %lld", (long long)i, bad);
  }
  FilterColumn& c = f->cols[col];
  HIP_TRY(hipSetDevice(f->device));
  std::vector<long long> abs_off((size_t)n + 1);   // offsets into the column's blob; abs_off[0] rewrites the end held so far
  for (int64_t i = 0; i <= n; ++i) abs_off[(size_t)i] = c.n_bytes + off[i];
  int rc = grow_keeping(c.str_bytes, (size_t)c.n_bytes, (size_t)(c.n_bytes + n_new), 4096, f->stream);
  if (rc != VRAG_OK) return rc;
  rc = grow_keeping(c.str_off, c.n_codes ? (size_t)c.n_codes + 1 : 0, (size_t)(c.n_codes + n) + 1, 257, f->stream);
  if (rc != VRAG_OK) return rc;
  if (n_new) HIP_TRY(hipMemcpyAsync(c.str_bytes.p + c.n_bytes, bytes, (size_t)n_new, hipMemcpyHostToDevice, f->stream));
  HIP_TRY(hipMemcpyAsync(c.str_off.p + c.n_codes, abs_off.data(), ((size_t)n + 1) * sizeof(long long), hipMemcpyHostToDevice, f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));   // the caller's arrays and abs_off are free again
  c.n_codes += n, c.n_bytes += n_new;
  return VRAG_OK;
}

int vrag_row_filter_strings(vrag_row_filter* f, int32_t col, int64_t* n_codes, int64_t* n_bytes) {
  ARG_CHECK(f && n_codes && n_bytes, "null argument");
  std::lock_guard<std::mutex> lk(f->mu);
  ARG_CHECK(col >= 0 && col < (int)f->cols.size(), "vrag_row_filter_strings: no column %d (the filter holds %d)", col, (int)f->cols.size());
  *n_codes = f->cols[col].n_codes, *n_bytes = f->cols[col].n_bytes;
  return VRAG_OK;
}

int vrag_row_filter_match(vrag_row_filter* f, int32_t col, int32_t op, const uint8_t* text, int32_t text_len, int64_t n_codes,
                          uint32_t* out_words, void* stream) {
  ARG_CHECK(f, "null argument");
  MatchProg prog;
  const int rc = match_compile("vrag_row_filter_match", op, text, text_len, &prog);
  if (rc != VRAG_OK) return rc;
  ARG_CHECK(n_codes >= 0 && n_codes <= 0xffffffffll, "vrag_row_filter_match: n_codes = %lld out of range", (long long)n_codes);
  ARG_CHECK(n_codes == 0 || out_words, "vrag_row_filter_match: null out_words");
  std::lock_guard<std::mutex> lk(f->mu);
  ARG_CHECK(col >= 0 && col < (int)f->cols.size(), "vrag_row_filter_match: no column %d (the filter holds %d)", col, (int)f->cols.size());
  const FilterColumn& c = f->cols[col];
  ARG_CHECK(n_codes <= c.n_codes, "vrag_row_filter_match: n_codes = %lld but column %d's dictionary holds %lld", (long long)n_codes, col,
            c.n_codes);
  if (n_codes == 0) return VRAG_OK;
  HIP_TRY(hipSetDevice(f->device));
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : f->stream;
  const size_t n_words = (size_t)((n_codes + 31) / 32);
  HIP_TRY(f->d_tables.grow(n_words));
  HIP_TRY(match_launch(c, prog, n_codes, f->d_tables.p, st));
  HIP_TRY(hipMemcpyAsync(out_words, f->d_tables.p, n_words * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return VRAG_OK;
}

}  // extern "C"
