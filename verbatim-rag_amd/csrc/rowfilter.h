// The row-filter handle as its two sources see it: csrc/rowfilter.hip (columns, the program, the eval kernel) and
// csrc/strmatch.hip (the columns' string dictionaries and the kernel that makes a string leaf's answer table from them).
#pragma once
#include <mutex>
#include <vector>

#include "common.h"
#include "compact.h"
#include "host_util.h"

namespace vrag {

struct FilterColumn {
  DevArray<unsigned char> kinds;
  DevArray<u64> payload;
  long long n = 0;   // rows held; the arrays' capacity is kinds.n
  // The dictionary of the column's strings: code c is the UTF-8 bytes str_bytes[str_off[c] .. str_off[c + 1]).  Appended to only,
  // geometric growth like the rows; str_off holds n_codes + 1 offsets once a string has arrived.
  DevArray<unsigned char> str_bytes;
  DevArray<long long> str_off;
  long long n_codes = 0, n_bytes = 0;
};

// One string leaf compiled for the match kernel (a by-value kernel argument, copied to LDS once per workgroup).
//   comparisons  elem[0 .. text_len) is the operand
//   LIKE         the pattern split at its unescaped `%` into n_seg non-empty segments; segment i is elem[seg_begin[i] ..
//                seg_begin[i + 1]): a literal byte each, or MATCH_ANY_ONE (0xFF, no byte of valid UTF-8) for `_`; seg_cp[i] = the
//                code points it consumes.  flags: MATCH_HAS_PCT the pattern holds a `%`, MATCH_FRONT segment 0 stands at byte 0,
//                MATCH_BACK the last segment ends at the string's end.  Without a `%` there is exactly one segment (possibly
//                empty) and it is the whole string.
constexpr unsigned char MATCH_ANY_ONE = 0xFF;
constexpr int MATCH_HAS_PCT = 1, MATCH_FRONT = 2, MATCH_BACK = 4;
struct MatchProg {
  int op, text_len, n_seg, flags;
  unsigned short seg_begin[VRAG_FILTER_MATCH_MAX_SEGMENTS + 1];
  unsigned short seg_cp[VRAG_FILTER_MATCH_MAX_SEGMENTS + 1];
  unsigned char elem[VRAG_FILTER_MATCH_MAX_PATTERN];
};
static_assert(sizeof(MatchProg) % 4 == 0 && sizeof(MatchProg) <= 512, "copied to LDS word by word");

// csrc/strmatch.hip.  match_compile validates (op, text) and fills `out`: VRAG_OK, or VRAG_ERR_INVALID with the message set
// (`who` = the calling entry point's name).  match_launch enqueues the kernel over codes [0, n_codes) of `c`'s dictionary (the
// caller has checked n_codes <= c.n_codes) and writes ceil(n_codes / 32) words at d_words; nothing behind them.
int match_compile(const char* who, int32_t op, const uint8_t* text, int32_t text_len, MatchProg* out);
hipError_t match_launch(const FilterColumn& c, const MatchProg& prog, long long n_codes, unsigned* d_words, hipStream_t st);

}  // namespace vrag

struct vrag_row_filter {
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  std::vector<vrag::FilterColumn> cols;
  vrag::DevArray<unsigned> d_tables, d_out;   // scratch of one eval (grown on demand)
  vrag::CompactScratch compact;               // vrag_row_filter_compact: its bitmap, row list and bounce buffer
};
