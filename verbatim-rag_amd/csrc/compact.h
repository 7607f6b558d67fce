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
#include <initializer_list>
#include <vector>

#include "host_util.h"

// Bytes of the bounce buffer (one per handle, allocated by the handle's first compaction that moves a row).
#define VRAG_COMPACT_BOUNCE_BYTES (32u << 20)

namespace vrag {

constexpr int FWORDS = 1024;   // bitmap words per workgroup of the row-list kernels (256 threads x one 16-byte load)

// Host staging of a caller's bitmap: the words of rows [0, n_rows) with the bits at and beyond n_rows cleared, then zero words up
// to a multiple of `pad`.  Returns the number of set bits.
long long stage_bitmap(std::vector<unsigned>& h, const uint32_t* words, long long n_rows, size_t pad);

// The ascending list of the rows whose bit is set in a bitmap, in device memory, with the scratch that builds it (popcount +
// prefix scan, no atomic appends: the same list on every run).  Owned by the handle that searches or compacts under the bitmap.
class RowList {
 public:
  // h: a bitmap staged by stage_bitmap with pad = FWORDS; n_set: its set bits, at least one.
  // reserve: every allocation of a build (a reallocation frees, and a free waits for the device), nothing enqueued -- for a caller
  // that has work in flight it must not wait behind; build calls it itself.
  hipError_t reserve(const std::vector<unsigned>& h, long long n_set);
  // Uploads the words and builds the list: one copy and three launches on `st`, no wait -- `h` stays as it is until the stream has
  // passed them (the caller syncs `st` before it lets go of `h`, on its error paths too).
  hipError_t build(const std::vector<unsigned>& h, long long n_set, hipStream_t st);
  const unsigned* rows() const { return d_list.p; }   // [n_set] ascending
  const unsigned* count() const { return d_count; }   // the device word that holds n_set once the build has run

 private:
  DevArray<unsigned> d_words, d_blk, d_list;
  const unsigned* d_count = nullptr;
};

// What one compaction needs, owned by the handle: the staged bitmap, the kept rows' list (list[j] = the source row of destination
// j) and the bounce buffer.
struct CompactScratch {
  std::vector<unsigned> h_words;
  RowList list;
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

// The compaction entry of a handle whose per-row arrays all hold `*size` rows, under the handle's lock: checks the bitmap (it
// covers exactly the handle's rows), plans, and -- when a row is dropped -- waits for the device (a search that only enqueued may
// still be reading the rows on a caller's stream), compacts every array on `st` (a null base: an array the handle does not hold),
// drains `st` and only then publishes the new size.  *new_size = *size on every VRAG_OK return; *dropped (nullable) = rows were
// dropped, so whatever the handle derived from the old row numbers is stale.
struct CompactArray {
  void* base;
  size_t row_bytes;
};
int compact_arrays(CompactScratch& s, int device, hipStream_t st, const uint32_t* keep_words, int64_t n_keep, int64_t* size,
                   int64_t* new_size, std::initializer_list<CompactArray> arrays, bool* dropped = nullptr);

}  // namespace vrag
