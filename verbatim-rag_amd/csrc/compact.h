// Row compaction under a keep-bitmap, shared by the handles that hold per-row arrays in HBM: the dense index (fp32 / bf16 rows and
// the bf16 prefilter image), the SQ8 index (codes at their padded stride, scales) and the row filter (kinds, payload).  The
// kernels and the two host routines live in csrc/compact.hip; each handle's C entry point stays with its struct.
//
// Contract.  A bitmap has bit r % 32 of word r / 32 set for every row r that stays (the layout of the `allow` masks).  Rows that
// stay keep their relative order and become rows 0 .. kept - 1 of the SAME array: nothing is reallocated and no second copy of the
// array exists at any time.  A row's destination (its rank among the kept rows) is never behind its source, so the one hazard is
// a store landing on a row that has not been read yet.  It is excluded by STREAM ORDER alone: rows travel in waves of at most
// VRAG_COMPACT_BOUNCE_BYTES through a bounce buffer -- one launch gathers a wave's rows into the buffer, the next launch stores
// them at their destination, and every later wave's sources lie behind everything stored so far.  No workgroup waits for another.
// The rows in front of the first cleared bit are not touched; a bitmap without a cleared bit launches nothing.
#pragma once
#include <vector>

#include "host_util.h"

// Bytes of the bounce buffer (one per handle, allocated by the handle's first compaction that moves a row).
#define VRAG_COMPACT_BOUNCE_BYTES (32u << 20)

namespace vrag {

constexpr int FWORDS = 1024;   // bitmap words per workgroup of the row-list kernels (256 threads x one 16-byte load)

// Host staging of a caller's bitmap: the words of rows [0, n_rows) with the bits at and beyond n_rows cleared, then zero words up
// to a multiple of `pad`.  Returns the number of set bits.
long long stage_bitmap(std::vector<unsigned>& h, const uint32_t* words, long long n_rows, size_t pad);

// d_words (device, n_blk * FWORDS words staged as above) -> d_list: the ascending list of the rows whose bit is set (popcount +
// prefix scan, no atomic appends: the same list on every run).  d_blk: 2 * n_blk + 1 words of scratch -- [n_blk] counts per
// workgroup, then [n_blk + 1] offsets whose last one is the list's length.  Three launches on `st`, nothing else.
hipError_t bitmap_row_list(const unsigned* d_words, int n_blk, unsigned* d_blk, unsigned* d_list, hipStream_t st);

// What one compaction needs, owned by the handle: the staged bitmap, the kept rows' list (list[j] = the source row of destination
// j) and the bounce buffer.
struct CompactScratch {
  std::vector<unsigned> h_words;
  DevArray<unsigned> d_words, d_blk, d_list;
  DevArray<char> bounce;
  long long n_rows = 0, n_keep = 0, first_hole = 0;   // of the staged bitmap; first_hole = n_rows when no bit is cleared
  long long kept_before(long long row) const;         // set bits among rows [0, row)
};

// Stages `keep_words` for rows [0, n_rows) and, when a row has to move, builds the list on `st`.  VRAG_OK or VRAG_ERR_HIP.
int compact_plan(CompactScratch& s, const uint32_t* keep_words, long long n_rows, hipStream_t st);

// Compacts rows [0, n_src) (n_src <= the plan's n_rows) of the array at `base`, `row_bytes` apart, in place on `st`; returns with
// the launches enqueued.  Rows of a multiple of 16 bytes move as 16-byte pieces per lane (`base` 16-byte aligned), rows of 1, 4 or
// 8 bytes as one element per lane.
int compact_rows(CompactScratch& s, void* base, size_t row_bytes, long long n_src, hipStream_t st);

}  // namespace vrag
