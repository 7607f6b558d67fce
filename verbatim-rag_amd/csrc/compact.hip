// In-place, order-preserving row compaction under a keep-bitmap (csrc/compact.h states the contract), and the bitmap-to-row-list
// kernels (RowList) it shares with the filtered and the grouped dense search (csrc/topk.hip, csrc/grouped.hip).
//
// Why bounce waves.  Compaction moves row list[j] to row j with list[j] >= j.  A single launch that did this in place would need
// every workgroup to know that the rows it overwrites have been read -- a flag another workgroup sets, and a workgroup that spins
// on a flag whose producer is not resident never ends.  Instead the order is the stream's: wave w gathers the sources of the
// destinations [j0, j1) into the bounce buffer (launch 1), then stores them (launch 2).  The stores of wave w land on rows < j1; every
// later wave reads rows list[j] >= j >= j1.  The gather of wave w + 1 reuses the buffer only after the store of wave w has drained it.
// Cost: every moved byte is read twice and written twice, all of it streaming, and the HBM held beside the array is the buffer.
#include "compact.h"

#include <cstring>

#include "common.h"

namespace vrag {
namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// words: the bitmap padded with zero words to a multiple of FWORDS (the host clears the bits at and beyond the row count), so no
// kernel below tests a bound.  blk_cnt[b] = set bits of workgroup b's words.
__global__ __launch_bounds__(256) void filter_count_kernel(const unsigned* __restrict__ words, unsigned* __restrict__ blk_cnt) {
  __shared__ unsigned red[4];
  const int tid = threadIdx.x;
  const u32x4 w = reinterpret_cast<const u32x4*>(words)[(size_t)blockIdx.x * 256 + tid];
  unsigned c = __popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) blk_cnt[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// Inclusive prefix sum of one value per thread over the 256 threads of a workgroup (wave scans + the four wave totals in LDS).
__device__ __forceinline__ unsigned block_scan_incl(unsigned v, unsigned* wave_tot) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  if (lane == 63) wave_tot[wave] = v;
  __syncthreads();
  unsigned base = 0;
  for (int w = 0; w < wave; ++w) base += wave_tot[w];
  __syncthreads();   // wave_tot may be rewritten by the caller's next round
  return v + base;
}

// One workgroup: blk_off[b] = passing rows in front of workgroup b's words, blk_off[n_blk] = all of them (the list's count).
__global__ __launch_bounds__(256) void filter_scan_kernel(const unsigned* __restrict__ blk_cnt, int n_blk, unsigned* __restrict__ blk_off) {
  __shared__ unsigned wave_tot[4];
  __shared__ unsigned carry_s;
  const int tid = threadIdx.x;
  if (tid == 0) carry_s = 0u;
  __syncthreads();
  for (int b0 = 0; b0 < n_blk; b0 += 256) {
    const int b = b0 + tid;
    const unsigned c = b < n_blk ? blk_cnt[b] : 0u;
    const unsigned incl = block_scan_incl(c, wave_tot);
    const unsigned carry = carry_s;
    if (b < n_blk) blk_off[b] = carry + incl - c;
    __syncthreads();
    if (tid == 255) carry_s = carry + incl;
    __syncthreads();
  }
  if (tid == 0) blk_off[n_blk] = carry_s;
}

// The list itself: thread t of workgroup b writes the rows of its four words behind blk_off[b] + (set bits of the threads in
// front of it) -- words ascending, bits ascending, so the list is ascending.  A workgroup without a set bit leaves before its
// loads (a zero word costs the one load of the count pass).
__global__ __launch_bounds__(256) void filter_emit_kernel(const unsigned* __restrict__ words, const unsigned* __restrict__ blk_cnt,
                                                           const unsigned* __restrict__ blk_off, unsigned* __restrict__ list) {
  __shared__ unsigned wave_tot[4];
  if (blk_cnt[blockIdx.x] == 0u) return;
  const int tid = threadIdx.x;
  const size_t w0 = ((size_t)blockIdx.x * 256 + tid) * 4;
  const u32x4 w = reinterpret_cast<const u32x4*>(words)[(size_t)blockIdx.x * 256 + tid];
  const unsigned c = __popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]);
  size_t pos = (size_t)blk_off[blockIdx.x] + block_scan_incl(c, wave_tot) - c;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned bits = w[j];
    while (bits) {
      list[pos++] = (unsigned)((w0 + j) * 32) + (unsigned)__builtin_ctz(bits);
      bits &= bits - 1u;
    }
  }
}

// One half of a wave: `n` rows of `upr` pieces of type T each, dst row i <- src row (list ? list[i] : i).  The gather reads the
// array through the list and writes the bounce buffer densely; the store reads the buffer and writes the array densely -- never
// the same buffer on both sides, hence __restrict__.  2^shift lanes share a row (the smallest power of two that covers upr, at
// most 256) and 256 >> shift rows share a workgroup step; workgroups stride over the steps.
template <typename T>
__global__ __launch_bounds__(256) void compact_move_kernel(T* __restrict__ dst, const T* __restrict__ src, const unsigned* __restrict__ list,
                                                           long long n, unsigned upr, int shift) {
  const unsigned tid = threadIdx.x, sub = tid & ((1u << shift) - 1u), lanes = 1u << shift;
  const long long rows_per_step = 256 >> shift;
  for (long long i = (long long)blockIdx.x * rows_per_step + (tid >> shift); i < n; i += (long long)gridDim.x * rows_per_step) {
    const T* from = src + (size_t)(list ? (long long)list[i] : i) * upr;
    T* to = dst + (size_t)i * upr;
#pragma unroll 4
    for (unsigned c = sub; c < upr; c += lanes) to[c] = from[c];
  }
}

template <typename T>
hipError_t move_rows(void* dst, const void* src, const unsigned* list, long long n, size_t row_bytes, hipStream_t st) {
  const unsigned upr = (unsigned)(row_bytes / sizeof(T));
  int shift = 0;
  while (shift < 8 && (1u << shift) < upr) ++shift;
  const long long rows_per_step = 256 >> shift;
  const unsigned grid = (unsigned)std::min<long long>((n + rows_per_step - 1) / rows_per_step, 2048);
  hipLaunchKernelGGL(compact_move_kernel<T>, dim3(grid), dim3(256), 0, st, reinterpret_cast<T*>(dst), reinterpret_cast<const T*>(src), list, n,
                     upr, shift);
  return hipGetLastError();
}

hipError_t move_rows_any(void* dst, const void* src, const unsigned* list, long long n, size_t row_bytes, hipStream_t st) {
  if (row_bytes % 16 == 0) return move_rows<u32x4>(dst, src, list, n, row_bytes, st);
  if (row_bytes == 8) return move_rows<unsigned long long>(dst, src, list, n, row_bytes, st);
  if (row_bytes == 4) return move_rows<unsigned>(dst, src, list, n, row_bytes, st);
  return move_rows<unsigned char>(dst, src, list, n, row_bytes, st);
}

}  // namespace

long long stage_bitmap(std::vector<unsigned>& h, const uint32_t* words, long long n_rows, size_t pad) {
  const size_t n_words = (size_t)((n_rows + 31) / 32);
  h.assign((n_words + pad - 1) / pad * pad, 0u);
  if (n_words) std::memcpy(h.data(), words, n_words * sizeof(unsigned));
  if (n_rows % 32) h[n_words - 1] &= (1u << (n_rows % 32)) - 1u;
  long long n_pass = 0;
  for (size_t i = 0; i < n_words; ++i) n_pass += __builtin_popcount(h[i]);
  return n_pass;
}

// d_blk: [n_blk] counts per workgroup, then [n_blk + 1] offsets whose last one is the list's length.
hipError_t RowList::reserve(const std::vector<unsigned>& h, long long n_set) {
  hipError_t e = d_words.grow(h.size());
  if (e == hipSuccess) e = d_blk.grow((size_t)2 * (h.size() / FWORDS) + 1);
  if (e == hipSuccess) e = d_list.grow((size_t)n_set);
  return e;
}

hipError_t RowList::build(const std::vector<unsigned>& h, long long n_set, hipStream_t st) {
  const int n_blk = (int)(h.size() / FWORDS);
  hipError_t e = reserve(h, n_set);
  if (e == hipSuccess) e = hipMemcpyAsync(d_words.p, h.data(), h.size() * sizeof(unsigned), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  unsigned* blk_cnt = d_blk.p;
  unsigned* blk_off = d_blk.p + n_blk;
  d_count = blk_off + n_blk;
  hipLaunchKernelGGL(filter_count_kernel, dim3(n_blk), dim3(256), 0, st, d_words.p, blk_cnt);
  hipLaunchKernelGGL(filter_scan_kernel, dim3(1), dim3(256), 0, st, blk_cnt, n_blk, blk_off);
  hipLaunchKernelGGL(filter_emit_kernel, dim3(n_blk), dim3(256), 0, st, d_words.p, blk_cnt, blk_off, d_list.p);
  return hipGetLastError();
}

long long CompactScratch::kept_before(long long row) const {
  row = std::min(std::max(row, 0ll), n_rows);
  long long c = 0;
  const size_t full = (size_t)(row / 32);
  for (size_t i = 0; i < full; ++i) c += __builtin_popcount(h_words[i]);
  if (row % 32) c += __builtin_popcount(h_words[full] & ((1u << (row % 32)) - 1u));
  return c;
}

int compact_plan(CompactScratch& s, const uint32_t* keep_words, long long n_rows, hipStream_t st) {
  s.n_rows = n_rows;
  s.n_keep = stage_bitmap(s.h_words, keep_words, n_rows, FWORDS);
  s.first_hole = n_rows;
  for (size_t i = 0; i < (size_t)((n_rows + 31) / 32); ++i) {
    const unsigned holes = ~s.h_words[i];
    if (holes) {
      s.first_hole = std::min<long long>(n_rows, (long long)i * 32 + __builtin_ctz(holes));
      break;
    }
  }
  if (s.n_keep == n_rows || s.n_keep == s.first_hole) return VRAG_OK;   // nothing is cleared, or nothing behind the first hole stays
  HIP_TRY(s.list.build(s.h_words, s.n_keep, st));
  return VRAG_OK;
}

int compact_rows(CompactScratch& s, void* base, size_t row_bytes, long long n_src, hipStream_t st) {
  ARG_CHECK(base && row_bytes >= 1 && row_bytes <= VRAG_COMPACT_BOUNCE_BYTES && n_src >= 0 && n_src <= s.n_rows, "compact_rows: bad arguments");
  const long long j_end = s.kept_before(n_src);
  if (s.first_hole >= j_end) return VRAG_OK;   // every kept row of this array already stands at its destination
  const long long wave_rows = (long long)(VRAG_COMPACT_BOUNCE_BYTES / row_bytes);
  HIP_TRY(s.bounce.grow(VRAG_COMPACT_BOUNCE_BYTES));
  char* rows = reinterpret_cast<char*>(base);
  for (long long j = s.first_hole; j < j_end; j += wave_rows) {
    const long long n = std::min(wave_rows, j_end - j);
    HIP_TRY(move_rows_any(s.bounce.p, rows, s.list.rows() + j, n, row_bytes, st));
    HIP_TRY(move_rows_any(rows + (size_t)j * row_bytes, s.bounce.p, nullptr, n, row_bytes, st));
  }
  return VRAG_OK;
}

int compact_arrays(CompactScratch& s, int device, hipStream_t st, const uint32_t* keep_words, int64_t n_keep, int64_t* size,
                   int64_t* new_size, std::initializer_list<CompactArray> arrays, bool* dropped) {
  ARG_CHECK(n_keep >= 0 && (keep_words || n_keep == 0), "bad row bitmap (null words or a negative length)");
  ARG_CHECK(n_keep == *size, "the bitmap covers %lld rows, the index holds %lld", (long long)n_keep, (long long)*size);
  *new_size = *size;
  if (n_keep == 0) return VRAG_OK;
  HIP_TRY(hipSetDevice(device));
  int rc;
  if ((rc = compact_plan(s, keep_words, n_keep, st))) return rc;
  if (s.n_keep == n_keep) return VRAG_OK;   // nothing to drop: no launch
  HIP_TRY(hipDeviceSynchronize());
  for (const CompactArray& a : arrays)
    if (a.base && (rc = compact_rows(s, a.base, a.row_bytes, n_keep, st))) return rc;
  HIP_TRY(hipStreamSynchronize(st));   // the new size is published once every row stands where it belongs
  *size = *new_size = s.n_keep;
  if (dropped) *dropped = true;
  return VRAG_OK;
}

}  // namespace vrag
