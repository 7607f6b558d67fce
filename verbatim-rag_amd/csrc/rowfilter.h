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
  // The LIST part (csrc/listfilter.hip): rows whose value is a list, as CSR.  Row r's elements are [list_off[r], list_off[r + 1])
  // of elem_kinds / elem_payload, encoded exactly like kinds / payload (strings through the same dictionary); a row that holds no
  // list has an empty range.  list_off holds n_list_rows + 1 offsets once a row has arrived.  Geometric growth like the rows.
  DevArray<long long> list_off;
  DevArray<unsigned char> elem_kinds;
  DevArray<u64> elem_payload;
  long long n_list_rows = 0, n_elems = 0;
};

// The program as the eval kernels take it: a by-value kernel argument (csrc/rowfilter.hip explains the layout).
constexpr int RF_WAVES = 4;            // waves of a workgroup
constexpr int RF_MAX_BLOCKS = 4096;
constexpr unsigned char RF_AND = 64, RF_OR = 65, RF_NOT = 66;   // op bytes; 0 .. 63 = push leaf
constexpr unsigned char RF_LIST_ANY = 128;                      // 128 .. 191 = push the OR of leaf (op - 128) over the row's list elements

struct LeafDev {
  double bound;
  unsigned table_off, table_codes;
  unsigned char slot, num_op, str_mode, bits;   // slot: index into EvalArgs' columns; bits: bit 0 other, bit 1 bool false, bit 2 bool true
  unsigned pad;
};

struct EvalArgs {
  const unsigned char* kinds[VRAG_FILTER_MAX_COLUMNS];
  const u64* payload[VRAG_FILTER_MAX_COLUMNS];
  LeafDev leaves[VRAG_FILTER_MAX_LEAVES];
  unsigned ops[VRAG_FILTER_MAX_OPS / 4];   // four op bytes per word, op i in byte i % 4 of word i / 4
  int n_ops;
};
static_assert(sizeof(EvalArgs) <= 3072, "the program travels as a kernel argument");

// One number comparison of a leaf (IEEE f64: -0.0 == 0.0, infinities ordered, NaN unordered); shared by the two eval kernels.
__device__ __forceinline__ bool num_answer(int op, double x, double bound) {
  switch (op) {   // wave-uniform
    case VRAG_FILTER_NUM_ALWAYS: return true;
    case VRAG_FILTER_NUM_EQ: return x == bound;
    case VRAG_FILTER_NUM_NE: return x != bound;
    case VRAG_FILTER_NUM_LT: return x < bound;
    case VRAG_FILTER_NUM_LE: return x <= bound;
    case VRAG_FILTER_NUM_GT: return x > bound;
    case VRAG_FILTER_NUM_GE: return x >= bound;
    default: return false;
  }
}

// The list parts of the same column slots, for a program with a list op (csrc/listfilter.hip); null for a slot no list op names.
struct ListArgs {
  const long long* list_off[VRAG_FILTER_MAX_COLUMNS];
  const unsigned char* elem_kinds[VRAG_FILTER_MAX_COLUMNS];
  const u64* elem_payload[VRAG_FILTER_MAX_COLUMNS];
};
static_assert(sizeof(EvalArgs) + sizeof(ListArgs) <= 3584, "both travel as kernel arguments (4 KB per launch)");

// csrc/listfilter.hip: the eval kernel for a program with RF_LIST_ANY ops, enqueued on `st`; same grid, same output as
// row_filter_eval_kernel (two words per group of 64 rows at d_out).
hipError_t list_eval_launch(const EvalArgs& a, const ListArgs& l, const unsigned* d_tables, long long n_rows, unsigned* d_out,
                            hipStream_t st);

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
