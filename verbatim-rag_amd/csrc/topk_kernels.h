// Launchers of the tiled batched dense search's own kernels (csrc/topk.hip; the score stage itself is launch_gemm(EPI_TOPK, ...)
// of csrc/gemm_bf16.h).  Declared here so that the unit-test hook (csrc/debug_api.hip, vrag_debug_topk_run) launches the product's
// own kernels with the product's own grids and dynamic LDS sizes: dense_tiled_search goes through the same functions.  None of
// them checks its arguments; the launch's status is returned.
#pragma once
#include <cmath>
#include <mutex>
#include <vector>

#include "common.h"
#include "host_util.h"

namespace vrag {

constexpr int KMAX = 64;        // list length of one device pass

// Paged search (k > KMAX): page p+1 only admits keys strictly below the last key of page p; keys are unique per
// (score, row), so the pages are disjoint and their concatenation is the exact top-(pages * KMAX).
__device__ __forceinline__ u64 make_key_below(float s, unsigned row, u64 bound) {
  const u64 key = make_key(s, row);
  return key < bound ? key : 0ull;
}

// Sorted (descending) insert into list[0..k) held in LDS; called by ONE lane.
__device__ __forceinline__ void insert_key(u64* list, int k, u64 key) {
  if (key <= list[k - 1]) return;
  int i = k - 1;
  while (i > 0 && list[i - 1] < key) {
    list[i] = list[i - 1];
    --i;
  }
  list[i] = key;
}

// ------------------------------------------------------------------------------------ the result path (host)
// Every search handle ends here: merged keys [nq][k] in a device buffer -> the caller's (score, id) lists.

// The answer where nothing passes (an empty index, an all-zero bitmap): n slots of -inf / -1, without a launch.
inline void fill_no_hits(float* scores, int64_t* ids, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    scores[i] = -INFINITY;
    ids[i] = -1;
  }
}

// The key format, read on the host: a non-zero key -> its score and row.
inline void decode_key(u64 key, float* score, int64_t* row) {
  *score = unorderable((unsigned)(key >> 32));
  *row = (int64_t)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFu));
}

// Merged keys [nq][k] of a search -> the caller's lists: score and id (perm[row], or base + row), missing hits (key 0) -1 / -inf.
inline void decode_keys(const std::vector<u64>& keys, int nq, int k, int64_t base, const int64_t* perm, float* scores,
                        int64_t* ids) {
  for (size_t i = 0; i < (size_t)nq * k; ++i) {
    if (keys[i] == 0ull) {
      fill_no_hits(scores + i, ids + i, 1);
    } else {
      int64_t row;
      decode_key(keys[i], scores + i, &row);
      ids[i] = perm ? perm[row] : base + row;
    }
  }
}

// The keys [nq][k] that the work enqueued on `st` leaves at d_keys -> the caller's lists: one copy back, ONE stream sync, decode.
// Whatever else the caller copies back rides on that sync when it is enqueued first.
inline int read_lists(const u64* d_keys, int nq, int k, hipStream_t st, float* scores, int64_t* ids) {
  std::vector<u64> keys((size_t)nq * k);
  HIP_TRY(hipMemcpyAsync(keys.data(), d_keys, keys.size() * sizeof(u64), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  decode_keys(keys, nq, k, 0, nullptr, scores, ids);
  return VRAG_OK;
}

// k > KMAX: ceil(k / KMAX) passes of KMAX; `run_page(bound)` leaves the merged page keys [nq][KMAX] in d_out.
// After each page the last key of a full page becomes that query's exclusive bound (0 = exhausted: nothing passes).
template <typename RunPage>
int paged_search(int nq, int k, DevArray<u64>& d_bound, const DevArray<u64>& d_out, hipStream_t st, RunPage run_page,
                 float* scores, int64_t* ids) {
  int rc;
  HIP_TRY(d_bound.grow((size_t)nq));
  std::vector<u64> bound((size_t)nq, ~0ull), page((size_t)nq * KMAX), all((size_t)nq * k, 0ull);
  for (int k0 = 0; k0 < k; k0 += KMAX) {
    HIP_TRY(hipMemcpyAsync(d_bound.p, bound.data(), (size_t)nq * sizeof(u64), hipMemcpyHostToDevice, st));
    if ((rc = run_page(d_bound.p))) return rc;
    HIP_TRY(hipMemcpyAsync(page.data(), d_out.p, page.size() * sizeof(u64), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    bool more = false;
    for (int q = 0; q < nq; ++q) {
      const int take = std::min(KMAX, k - k0);
      for (int j = 0; j < take; ++j) all[(size_t)q * k + k0 + j] = page[(size_t)q * KMAX + j];
      bound[q] = page[(size_t)q * KMAX + KMAX - 1];   // 0 when the page was not full
      more = more || bound[q] != 0ull;
    }
    if (!more) break;
  }
  decode_keys(all, nq, k, 0, nullptr, scores, ids);
  return VRAG_OK;
}

// The common case: `run_page(bound)` enqueues one page on `st` into d_out [nq][min(k, KMAX)] (bound: per-query exclusive key
// bounds, null = none); the caller's lists come back.  k <= KMAX is one page and read_lists, larger k goes through paged_search.
template <typename RunPage>
int search_lists(int nq, int k, DevArray<u64>& d_bound, const DevArray<u64>& d_out, hipStream_t st, RunPage run_page, float* scores,
                 int64_t* ids) {
  if (k > KMAX) return paged_search(nq, k, d_bound, d_out, st, run_page, scores, ids);
  if (const int rc = run_page(nullptr)) return rc;
  return read_lists(d_out.p, nq, k, st, scores, ids);
}

constexpr int kTiledSelectMaxCap = 4096;   // the largest candidate buffer a selection sorts in LDS (the prefilter's lists)
constexpr int kTiledRescueMaxSlices = 64;  // workgroups per flagged query of the rescue pass, at most

// fp32 queries [nq, dim] -> the score GEMM's W operand [n_cols_pad, dim] bf16.  pairs: rows (2q, 2q + 1) =
// (bf16(q), bf16(q - bf16(q))); rows beyond the queries are zero.  One workgroup per row of w.
hipError_t launch_tiled_queries(const float* q, int nq, int dim, int pairs, int n_cols_pad, bf16_t* w, hipStream_t st);
// One workgroup per query: the first min(cnt[q], cap) keys of buf[q] (direct_n > 0: the first min(direct_n, cap)) sorted descending,
// the best k kept in buf[q][0, k) and written to out[q][0, k) (nullable), cnt[q] = min(n, k), (thr_key, thr_score)[q] = the k-th
// key and its score, (0, -inf) while fewer than k keys exist; ovf[q] = 1 where the count exceeded cap.  cap: a power of two,
// 2 <= cap <= kTiledSelectMaxCap (cap keys of dynamic LDS); k <= cap.
hipError_t launch_tiled_select(u64* buf, unsigned* cnt, int cap, int k, u64* thr_key, float* thr_score, u64* out, unsigned* ovf,
                               int direct_n, int nq, hipStream_t st);
// The first stage's selection: n keys per query at src[q * src_stride] (0 = no key) -> the same outputs, through windows that grow
// 16x (k <= 16) / 4x from a first window of 256 / 1 024 keys; more than cap - k survivors of one window raise ovf[q].  cap: a power
// of two, at least the first window and k, at most kTiledSelectMaxCap.
hipError_t launch_tiled_select_direct(const u64* src, int src_stride, int n, u64* buf, unsigned* cnt, int cap, int k, u64* thr_key,
                                      float* thr_score, u64* out, unsigned* ovf, int nq, hipStream_t st);
// Flagged queries (ovf[q] != 0) re-answered over rows [n_rows, dim] bf16 by `slices` workgroups each (<= kTiledRescueMaxSlices):
// out[q][0, k) = the exact best k; part [slices][nq][k] scratch; done [nq] slice counters, zero before and after.
hipError_t launch_dense_tiled_rescue(const bf16_t* rows, long long n_rows, int dim, const float* queries, int nq, int k,
                                     const unsigned* ovf, u64* part, unsigned* done, u64* out, int slices, hipStream_t st);
// Collect form: thr_score[q] -= 2 eps[q] (-inf stays), thr_key[q] = 0, cnt[q] = 0, flag[q] = 0.
hipError_t launch_tiled_tau(int nq, u64* thr_key, float* thr_score, const float* eps, unsigned* cnt, unsigned* flag, hipStream_t st);
// cand [n_wg][nq][k]: per-workgroup lists sorted descending, zero tails, keys unique -> out [nq][k] the best k (also csrc/fulltext.hip).
hipError_t launch_topk_merge(const u64* cand, int n_wg, int nq, int k, u64* out, hipStream_t st);
// Device-resident lists (what a rank contributes to the cross-GPU exchange): n merged keys decoded in device memory as decode_keys
// decodes them on the host -- id = row_map[row] (a row at or beyond n_map, or mapped to a negative id: -1 / -inf) or, without a
// map, id_base + row; missing hits -1 / -inf.
hipError_t launch_topk_export(const u64* keys, long long n, const int64_t* row_map, int64_t n_map, int64_t id_base, float* out_scores,
                              int64_t* out_ids, hipStream_t st);


// What another handle may know of a dense index (csrc/ivf.hip lays an inverted-file overlay over the resident rows): the rows'
// device address, their layout and how many are in place, read under the index's lock.  dtype: 0 = bf16 rows, 1 = fp32 rows (an
// index created with dtype 2 reports 1: `rows` are its fp32 rows).  The address is fixed for the index's lifetime; rows [0, size)
// are never rewritten.
struct DenseView {
  const void* rows;
  int dim, dtype, device;
  long long size;
};

}  // namespace vrag

struct vrag_dense_index;
namespace vrag {
DenseView dense_index_view(vrag_dense_index* ix);
// For a search of the index's rows that lives in another file (csrc/grouped.hip): the index's lock, held for the whole call like
// the searches of csrc/topk.hip hold it -- a compaction, which moves rows in place, waits -- and the view read under it.
std::unique_lock<std::mutex> dense_index_lock(vrag_dense_index* ix);
DenseView dense_index_view_locked(vrag_dense_index* ix);
}  // namespace vrag
