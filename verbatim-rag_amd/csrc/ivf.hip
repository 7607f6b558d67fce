// IVF_FLAT as an OVERLAY over a resident dense index (csrc/topk.hip) + C ABI.
//
// Serves what the reference configures on its Milvus stores (verbatim_rag/vector_stores/milvus_base.py:40-50,
// milvus_local.py:109-117: index_type="IVF_FLAT", nlist; search_params={"nprobe": N}).  The inverted file is no second image of
// the rows: it is `nlist` fp32 centroids, `list_off[nlist + 1]` and `list_rows[n]` -- the row numbers of the base index grouped
// by list, ascending inside a list -- 4 bytes per row next to a shard of 1.5 - 3 KB per row.  A search gathers whole rows of the
// base by number; on this part gathered rows of 1 - 2 KB read about as fast as a contiguous stream, so
// a copy in list order would buy little and cost the shard's size again.  Filters, deletes and appends keep acting on the one shard.
//
// Assignment rule (training, sync and probing alike):  list(x) = argmax_c ( x.c - 1/2 |c|^2 ), the lowest list on ties -- the
// nearest centroid in L2 without the |x|^2 term every list shares.  Those scores are plain fp32 sums in a register-tiled order
// (ivf_tile_kernel); only the SCAN's scores are bit-defined.
//
// Search, per slice of the queries:
//   probe   ivf_tile_kernel<.., false> scores every (query, list); ivf_select_kernel sorts one query's nlist packed keys
//           (make_key(score, list): score desc, list asc) in LDS -- 16 384 keys = 128 KB of the CU's 160 KiB -- and keeps the
//           first nprobe.  nprobe >= nlist: every list, no scores and no selection.
//   invert  (query, list) pairs -> per-list groups of up to IVF_QG queries (integer atomics for a pair's place in its list's
//           group sequence; no result depends on that place), ivf_groups_kernel numbers the groups, ivf_fill_kernel writes them
//   scan    ivf_scan_kernel: one work item per (list, query group) x row split; rows of the list staged through LDS in
//           16-byte pieces (bf16 widened to fp32), thread (row, query) runs  acc = fmaf(x[c], q[c], acc), c ascending  -- the
//           chain of filtered_score_kernel and of the oracle, so with nprobe == nlist the result equals
//           vrag_dense_index_search_filtered under an all-ones bitmap bit for bit.  Lists leave as cand[probe rank][split][query][k]
//   merge   launch_topk_merge (csrc/topk.hip) per slice.
// Row split: a work item's rows are cut into `split` ranges (blockIdx.y) -- enough to put some 4 096 workgroups behind a call with
// few (query, list) pairs, and, when not every list is probed, enough that the largest list is cut into ranges of at most 2 048 rows
// (k-means lists are uneven: a list forty times the mean is one workgroup's serial tail otherwise); never ranges under 128 rows,
// at most 64, and never more than the key bound below allows.  Measured against a split of at most 8 in profiles/ivf_probe.txt (one
// query, nprobe 8, largest list 39 x the mean: 1.13 -> 0.36 ms); the constants themselves are a first choice, not swept.
// Scratch bound: a slice holds at most IVF_SLICE_KEYS = 2^22 candidate keys (32 MB; nprobe * k * split <= 2^22, so a slice always
// holds at least one query), at most IVF_SLICE_SCORES = 2^24 probe scores (64 MB) and at most 4 096 queries; the group tables take
// 72 bytes per (query, list) pair (<= 2^22 / k pairs).
//
// Over an SQ8 base (vrag_ivf_index_create_sq8; csrc/sq8_kernels.h) the overlay is the same handle: training and assignment read the
// int8 rows as  x^[c] = fl((float)code[c] * scale)  (ROWS_SQ8 forms of ivf_tile_kernel and ivf_mean_kernel), the handle's column
// count is the rows' stride (centroids and queries are padded with zero columns on their way in), the queries are quantised once
// per search by sq8_query_kernel and the scan stage is ivf_sq8_scan_kernel (csrc/ivf_sq8.hip); probe, invert and merge are unchanged.
#include "../../include/vrag_amd.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "common.h"
#include "host_util.h"
#include "ivf_kernels.h"
#include "sq8_kernels.h"
#include "topk_kernels.h"

namespace vrag {
namespace {

constexpr int IVF_NLIST_MAX = 16384;
constexpr int IVF_CH = 256;                 // columns per LDS stage of the scan (filtered_score_kernel's shape; IVF_ROWS rows a step)
constexpr long long IVF_SLICE_KEYS = 1ll << 22, IVF_SLICE_SCORES = 1ll << 24;
constexpr int IVF_SLICE_QUERIES = 4096;
constexpr int IVF_SCAN_WGS = 2048;
constexpr int IVF_SPLIT_MAX = 64, IVF_SPLIT_WGS = 4096, IVF_SPLIT_ROWS_MAX = 2048, IVF_SPLIT_ROWS_MIN = 128;

// What the rows of the base are (the handle's `dtype`): bf16 or fp32 rows of a dense index, or the int8 codes of an SQ8 index, which
// stand for  x^[c] = fl((float)code[c] * scale)  wherever a row is trained on or assigned (never in the scan: csrc/ivf_sq8.hip).
enum RowKind : int { ROWS_BF16 = 0, ROWS_F32 = 1, ROWS_SQ8 = 2 };

__device__ __forceinline__ float sq8_code(const i32x4& v, int j) { return (float)(int)(signed char)((unsigned)v[j >> 2] >> (8 * (j & 3))); }

// Row number of sample item i: row0 + i * num / den (num >= den >= 1: strictly increasing; 1 / 1 = consecutive rows).
struct RowMap {
  long long row0, num, den;
  __device__ __forceinline__ long long at(long long i) const { return row0 + i * num / den; }
};

// ------------------------------------------------------------------------------------ centroids
// half[c] = 1/2 |c|^2: one wave per centroid, a fixed reduction order.
__global__ __launch_bounds__(64) void ivf_half_norm_kernel(const float* __restrict__ cent, int dim, float* __restrict__ half) {
  const float* c = cent + (size_t)blockIdx.x * dim;
  float s = 0.f;
  for (int i = threadIdx.x; i < dim; i += 64) s = fmaf(c[i], c[i], s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) half[blockIdx.x] = 0.5f * s;
}

// ------------------------------------------------------------------------------------ assignment / probe scores
// S[i][c] = x_i . cent_c - half[c] for a tile of TM items x TN centroids per step: 256 threads as 16 x 16, a 4 x 4 register tile
// each, TK columns of both operands staged transposed in LDS (a step reads two 16-byte vectors per 16 fmaf).
// ROWS_SQ8: `dim` is the rows' stride (a multiple of 16; pad codes are zero, the centroids' pad columns too), x_scale their scales.
// ARGMAX: grid = item tiles; the workgroup walks every centroid tile and keeps, per item, the best (score desc, list asc) ->
// assign[i].  Otherwise: grid = (item tiles, centroid tiles) and the scores leave as scores[i][nlist].
constexpr int TM = 64, TN = 64, TK = 32;
template <int RK, bool ARGMAX>
__global__ __launch_bounds__(256) void ivf_tile_kernel(const void* __restrict__ x_v, const float* __restrict__ x_scale, RowMap map,
                                                        long long n_items, int dim,
                                                        const float* __restrict__ cent, const float* __restrict__ half, int nlist,
                                                        unsigned* __restrict__ assign, float* __restrict__ scores) {
  __shared__ __attribute__((aligned(16))) float sx[TK][TM + 4];
  __shared__ __attribute__((aligned(16))) float sc[TK][TN + 4];
  __shared__ float sbest[TM][16];
  __shared__ unsigned sbidx[TM][16];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const long long i0 = (long long)blockIdx.x * TM;
  float best[4];
  unsigned bidx[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) best[a] = -INFINITY, bidx[a] = 0u;
  const int ct_lo = ARGMAX ? 0 : blockIdx.y, ct_hi = ARGMAX ? (nlist + TN - 1) / TN : blockIdx.y + 1;
  constexpr int PW = RK == ROWS_F32 ? 4 : RK == ROWS_BF16 ? 8 : 16;   // columns of a 16-byte piece of an item's row
  for (int ct = ct_lo; ct < ct_hi; ++ct) {
    const int c0 = ct * TN;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
    for (int k0 = 0; k0 < dim; k0 += TK) {
      const int w = min(TK, dim - k0);   // dim % 8 == 0
      __syncthreads();                   // the previous step's reads are done
      for (int p = tid; p < TM * (w / PW); p += 256) {
        const int m = p / (w / PW), kk = PW * (p % (w / PW));
        const long long r = map.at(min(i0 + m, n_items - 1));   // items behind the end re-read the last one; their results are dropped
        if constexpr (RK == ROWS_F32) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(x_v) + (size_t)r * dim + k0 + kk);
#pragma unroll
          for (int j = 0; j < 4; ++j) sx[kk + j][m] = v[j];
        } else if constexpr (RK == ROWS_SQ8) {
          const i32x4 v = *reinterpret_cast<const i32x4*>(reinterpret_cast<const signed char*>(x_v) + (size_t)r * dim + k0 + kk);
          const float s = x_scale[r];
#pragma unroll
          for (int j = 0; j < 16; ++j) sx[kk + j][m] = __fmul_rn(sq8_code(v, j), s);
        } else {
          const bf16x8 v = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16_t*>(x_v) + (size_t)r * dim + k0 + kk);
#pragma unroll
          for (int j = 0; j < 8; ++j) sx[kk + j][m] = (float)v[j];
        }
      }
      for (int p = tid; p < TN * (w / 4); p += 256) {
        const int n = p / (w / 4), kk = 4 * (p % (w / 4));
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (c0 + n < nlist) v = *reinterpret_cast<const f32x4*>(cent + (size_t)(c0 + n) * dim + k0 + kk);
#pragma unroll
        for (int j = 0; j < 4; ++j) sc[kk + j][n] = v[j];
      }
      __syncthreads();
#pragma unroll 8
      for (int kk = 0; kk < w; ++kk) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(&sx[kk][ty * 4]);
        const f32x4 cv = *reinterpret_cast<const f32x4*>(&sc[kk][tx * 4]);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] = fmaf(xv[a], cv[b], acc[a][b]);
      }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int c = c0 + tx * 4 + b;
      if (c >= nlist) continue;
      const float h = half[c];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const float s = acc[a][b] - h;
        if constexpr (ARGMAX) {
          if (s > best[a]) best[a] = s, bidx[a] = (unsigned)c;   // this thread's lists ascend: the first maximum stays
        } else {
          const long long i = i0 + ty * 4 + a;
          if (i < n_items) scores[(size_t)i * nlist + c] = s;
        }
      }
    }
  }
  if constexpr (ARGMAX) {
#pragma unroll
    for (int a = 0; a < 4; ++a) sbest[ty * 4 + a][tx] = best[a], sbidx[ty * 4 + a][tx] = bidx[a];
    __syncthreads();
    if (tid < TM && i0 + tid < n_items) {
      float bs = sbest[tid][0];
      unsigned bi = sbidx[tid][0];
      for (int t = 1; t < 16; ++t) {
        const float s = sbest[tid][t];
        const unsigned i = sbidx[tid][t];
        if (s > bs || (s == bs && i < bi)) bs = s, bi = i;
      }
      assign[i0 + tid] = bi;
    }
  }
}

// Lloyd update of one list per workgroup: thread t owns columns t, t + 256, ...; the members (base row numbers, ascending) are
// summed one after the other in fp32 -- no atomics, the same bits on every run -- and divided by their count.  An empty list
// keeps its centroid.
template <int RK>
__global__ __launch_bounds__(256) void ivf_mean_kernel(const void* __restrict__ rows_v, const float* __restrict__ row_scale, int dim,
                                                        const unsigned* __restrict__ off, const unsigned* __restrict__ members,
                                                        float* __restrict__ cent) {
  const unsigned lo = off[blockIdx.x], hi = off[blockIdx.x + 1];
  if (lo == hi) return;
  const float n = (float)(hi - lo);
  for (int c = threadIdx.x; c < dim; c += 256) {
    float s = 0.f;
#pragma unroll 4
    for (unsigned m = lo; m < hi; ++m) {
      const size_t at = (size_t)members[m] * dim + c;
      if constexpr (RK == ROWS_SQ8) s += __fmul_rn((float)reinterpret_cast<const signed char*>(rows_v)[at], row_scale[members[m]]);   // x^: no fused step
      else s += RK == ROWS_F32 ? reinterpret_cast<const float*>(rows_v)[at] : (float)reinterpret_cast<const bf16_t*>(rows_v)[at];
    }
    cent[(size_t)blockIdx.x * dim + c] = s / n;
  }
}

// ------------------------------------------------------------------------------------ probe selection
// One workgroup per query: its nlist scores as packed keys (zero keys pad to `cap`, a power of two) sorted descending in LDS by a
// bitonic network; probe[q][r] = the list of the r-th key, r < nprobe (< nlist: every kept key is a real one).
__global__ __launch_bounds__(1024) void ivf_select_kernel(const float* __restrict__ scores, int nlist, int cap, int nprobe,
                                                           unsigned* __restrict__ probe) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u64* keys = reinterpret_cast<u64*>(smem);
  const int q = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < cap; i += 1024) keys[i] = i < nlist ? make_key(scores[(size_t)q * nlist + i], (unsigned)i) : 0ull;
  __syncthreads();
  for (int size = 2; size <= cap; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (cap >> 1); t += 1024) {
        const int lo = ((t / stride) * stride << 1) + (t % stride), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const u64 a = keys[lo], b = keys[hi];
        if ((a < b) == desc) keys[lo] = b, keys[hi] = a;
      }
      __syncthreads();
    }
  }
  for (int r = tid; r < nprobe; r += 1024) probe[(size_t)q * nprobe + r] = 0xFFFFFFFFu - (unsigned)(keys[r] & 0xFFFFFFFFull);
}

// ------------------------------------------------------------------------------------ invert
// Pair p = (query p / nprobe, rank p % nprobe); its list is probe[p], or the rank itself when every list is probed.
__device__ __forceinline__ unsigned pair_list(const unsigned* probe, long long p, int nprobe) {
  return probe ? probe[p] : (unsigned)(p % nprobe);
}

// place[p] = the pair's place among the pairs of its list (arrival order); cnt[list] = pairs of the list; scanned[q] += rows of the list.
__global__ __launch_bounds__(256) void ivf_count_kernel(const unsigned* __restrict__ probe, long long n_pairs, int nprobe,
                                                         const unsigned* __restrict__ list_off, unsigned* __restrict__ cnt,
                                                         unsigned* __restrict__ place, unsigned long long* __restrict__ scanned) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n_pairs) return;
  const unsigned l = pair_list(probe, p, nprobe);
  place[p] = atomicAdd(cnt + l, 1u);
  atomicAdd(scanned + p / nprobe, (unsigned long long)(list_off[l + 1] - list_off[l]));
}

// One workgroup: goff[l] = work items (groups of IVF_QG pairs) in front of list l, goff[nlist] = all of them.
__global__ __launch_bounds__(256) void ivf_groups_kernel(const unsigned* __restrict__ cnt, int nlist, unsigned* __restrict__ goff) {
  __shared__ unsigned part[256];
  const int tid = threadIdx.x, per = (nlist + 255) / 256, lo = min(nlist, tid * per), hi = min(nlist, lo + per);
  unsigned s = 0;
  for (int l = lo; l < hi; ++l) s += (cnt[l] + IVF_QG - 1) / IVF_QG;
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    unsigned run = 0;
    for (int t = 0; t < 256; ++t) {
      const unsigned v = part[t];
      part[t] = run;
      run += v;
    }
    goff[nlist] = run;
  }
  __syncthreads();
  unsigned run = part[tid];
  for (int l = lo; l < hi; ++l) {
    goff[l] = run;
    run += (cnt[l] + IVF_QG - 1) / IVF_QG;
  }
}

// item = goff[list] + place / IVF_QG: item_list[item] = list, item_n[item] = its pairs, item_pair[item][place % IVF_QG] = the pair.
__global__ __launch_bounds__(256) void ivf_fill_kernel(const unsigned* __restrict__ probe, long long n_pairs, int nprobe,
                                                        const unsigned* __restrict__ cnt, const unsigned* __restrict__ place,
                                                        const unsigned* __restrict__ goff, unsigned* __restrict__ item_list,
                                                        unsigned* __restrict__ item_n, unsigned* __restrict__ item_pair) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n_pairs) return;
  const unsigned l = pair_list(probe, p, nprobe), at = place[p], item = goff[l] + at / IVF_QG, slot = at % IVF_QG;
  item_pair[(size_t)item * IVF_QG + slot] = ((unsigned)(p / nprobe) << IVF_RANK_BITS) | (unsigned)(p % nprobe);
  if (slot == 0) {
    item_list[item] = l;
    item_n[item] = min((unsigned)IVF_QG, cnt[l] - at);
  }
}

// ------------------------------------------------------------------------------------ scan
// filtered_score_kernel's step over the rows of ONE list for the queries of ONE group: IVF_ROWS rows x IVF_QG queries per step, all
// 256 threads stage IVF_CH columns of the rows and of the queries through LDS (row stride IVF_CH + 4 words), thread (row, query)
// runs one serial chain; the step's keys go through LDS to one lane per query (insert_key).  blockIdx.y cuts the list's row
// groups into gridDim.y ranges.  Workgroups stride over the work items; every (rank, split, query) list is written, empty ones as zeros.
template <bool F32>
__global__ __launch_bounds__(256) void ivf_scan_kernel(const void* __restrict__ rows_v, int dim, const unsigned* __restrict__ list_off,
                                                        const unsigned* __restrict__ list_rows, const float* __restrict__ queries,
                                                        int nq, int k, const unsigned* __restrict__ n_items_p,
                                                        const unsigned* __restrict__ item_list, const unsigned* __restrict__ item_n,
                                                        const unsigned* __restrict__ item_pair, u64* __restrict__ cand) {
  __shared__ __attribute__((aligned(16))) float srow[IVF_ROWS][IVF_CH + 4];
  __shared__ __attribute__((aligned(16))) float sq[IVF_QG][IVF_CH + 4];
  __shared__ u64 lists[IVF_QG][KMAX];
  __shared__ u64 skey[IVF_QG][IVF_ROWS];
  __shared__ unsigned srid[IVF_ROWS];
  __shared__ unsigned spair[IVF_QG];
  const int tid = threadIdx.x, r = tid & (IVF_ROWS - 1), qi = tid >> 4;
  const unsigned n_items = *n_items_p;
  constexpr int PW = F32 ? 4 : 8;   // columns of a 16-byte piece of a row
  for (unsigned item = blockIdx.x; item < n_items; item += gridDim.x) {
    const unsigned l = item_list[item];
    const int nqt = (int)item_n[item];
    const unsigned begin = list_off[l], end = list_off[l + 1];
    const unsigned n_groups = (end - begin + IVF_ROWS - 1) / IVF_ROWS;
    const unsigned g_lo = (unsigned)((unsigned long long)n_groups * blockIdx.y / gridDim.y);
    const unsigned g_hi = (unsigned)((unsigned long long)n_groups * (blockIdx.y + 1) / gridDim.y);
    __syncthreads();   // the previous item's lists have been written out
    if (tid < nqt) spair[tid] = item_pair[(size_t)item * IVF_QG + tid];
    for (int i = tid; i < IVF_QG * k; i += 256) lists[i / k][i % k] = 0ull;
    for (unsigned g = g_lo; g < g_hi; ++g) {
      const unsigned base = begin + g * IVF_ROWS;
      __syncthreads();   // spair / lists are set; the previous step's chains and insertions are done with srid / skey
      if (tid < IVF_ROWS) srid[tid] = list_rows[min(base + tid, end - 1u)];   // slots behind the list re-read its last row; their keys are dropped
      __syncthreads();
      float acc = 0.f;
      for (int c0 = 0; c0 < dim; c0 += IVF_CH) {
        const int w = min(IVF_CH, dim - c0);   // dim % 8 == 0 (vrag_dense_index_create)
        const int ppr = w / PW, total = IVF_ROWS * ppr;
        for (int p = tid; p < total; p += 256) {
          const int rr = p / ppr, cc = PW * (p % ppr);
          if constexpr (F32) {
            *reinterpret_cast<f32x4*>(&srow[rr][cc]) =
                *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(rows_v) + (size_t)srid[rr] * dim + c0 + cc);
          } else {
            const bf16x8 v = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16_t*>(rows_v) + (size_t)srid[rr] * dim + c0 + cc);
            f32x4 lo, hi;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              lo[j] = (float)v[j];
              hi[j] = (float)v[4 + j];
            }
            *reinterpret_cast<f32x4*>(&srow[rr][cc]) = lo;
            *reinterpret_cast<f32x4*>(&srow[rr][cc + 4]) = hi;
          }
        }
        const int qpr = w / 4;
        for (int p = tid; p < nqt * qpr; p += 256) {
          const int qq = p / qpr, cc = 4 * (p % qpr);
          *reinterpret_cast<f32x4*>(&sq[qq][cc]) =
              *reinterpret_cast<const f32x4*>(queries + (size_t)(spair[qq] >> IVF_RANK_BITS) * dim + c0 + cc);
        }
        __syncthreads();
        if (qi < nqt) {
#pragma unroll 8
          for (int c = 0; c < w; c += 4) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(&srow[r][c]);
            const f32x4 qv = *reinterpret_cast<const f32x4*>(&sq[qi][c]);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __fmaf_rn(xv[j], qv[j], acc);
          }
        }
        __syncthreads();
      }
      skey[qi][r] = (qi < nqt && base + r < end) ? make_key_below(acc, srid[r], ~0ull) : 0ull;
      __syncthreads();
      if (r == 0 && qi < nqt) {
        for (int i = 0; i < IVF_ROWS; ++i) insert_key(lists[qi], k, skey[qi][i]);
      }
    }
    __syncthreads();
    for (int i = tid; i < nqt * k; i += 256) {
      const unsigned pr = spair[i / k];
      const size_t slot = ((size_t)(pr & ((1u << IVF_RANK_BITS) - 1u)) * gridDim.y + blockIdx.y) * nq + (pr >> IVF_RANK_BITS);
      cand[slot * k + i % k] = lists[i / k][i % k];
    }
  }
}

}  // namespace
}  // namespace vrag

using namespace vrag;

struct vrag_ivf_index {
  vrag_dense_index* base = nullptr;   // the base, not owned, which must outlive this handle: a dense index ...
  vrag_sq8_index* sq8_base = nullptr; // ... or an SQ8 index (dtype == ROWS_SQ8); exactly one of the two is set
  const void* rows = nullptr;         // the base's rows or codes (a fixed address), their layout
  const float* row_scales = nullptr;  // ROWS_SQ8: the rows' scales
  int dim = 0;                        // columns the kernels walk = pitch of rows, centroids and queries: the SQ8 stride over an SQ8 base
  int user_dim = 0;                   // columns of the caller's centroids and queries (== dim over a dense base)
  int dtype = 0, device = 0;          // dtype: RowKind
  int nlist = 0;
  bool have_centroids = false, synced = false;
  long long n_assigned = 0, largest = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  DevArray<float> d_cent, d_half;            // [nlist][dim], [nlist]
  DevArray<unsigned> d_off, d_rows;          // list_off [nlist + 1], list_rows [n_assigned]
  std::vector<unsigned> h_assign, h_off, h_rows;   // list of every assigned row; the lists' host copies
  // scratch (grown on demand)
  DevArray<unsigned> d_assign;               // assignments of one training / sync pass
  DevArray<unsigned> d_toff, d_tmem;         // training: the sample's lists
  DevArray<float> d_q, d_scores;             // queries [nq][dim]; probe scores of a slice
  DevArray<unsigned> d_probe, d_cnt, d_place, d_goff, d_item_list, d_item_n, d_item_pair;
  DevArray<unsigned long long> d_scanned;    // [nq]
  DevArray<u64> d_cand, d_out;
  DevArray<signed char> d_qc;                // ROWS_SQ8: the queries' codes [nq][dim] and scales [nq]
  DevArray<float> d_qs;
};

namespace {

// What both kinds of base tell the overlay, read under the base's lock.
struct BaseView {
  const void* rows;
  int dim;
  long long size;
};
BaseView base_view(vrag_ivf_index* ix) {
  if (ix->sq8_base) {
    const Sq8View v = sq8_index_view(ix->sq8_base);
    return BaseView{v.codes, v.dim, v.size};
  }
  const DenseView v = dense_index_view(ix->base);
  return BaseView{v.rows, v.dim, v.size};
}

// `height` rows of `width` bytes between a host array and a device array of other pitch (the SQ8 stride pads the columns).
hipError_t copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind, hipStream_t st) {
  if (dpitch == width && spitch == width) return hipMemcpyAsync(dst, src, width * height, kind, st);
  return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, kind, st);
}

hipError_t half_norms(vrag_ivf_index* ix, hipStream_t st) {
  hipLaunchKernelGGL(ivf_half_norm_kernel, dim3(ix->nlist), dim3(64), 0, st, ix->d_cent.p, ix->dim, ix->d_half.p);
  return hipGetLastError();
}

// assign[i] = list of item i (base rows map.at(i), i < n) into ix->d_assign.
hipError_t assign_rows(vrag_ivf_index* ix, RowMap map, long long n, hipStream_t st) {
  hipError_t e = ix->d_assign.grow((size_t)n);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((n + TM - 1) / TM));
  const auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, ix->rows, ix->row_scales, map, n, ix->dim, ix->d_cent.p, ix->d_half.p, ix->nlist,
                       ix->d_assign.p, (float*)nullptr);
  };
  if (ix->dtype == ROWS_F32) launch(ivf_tile_kernel<ROWS_F32, true>);
  else if (ix->dtype == ROWS_SQ8) launch(ivf_tile_kernel<ROWS_SQ8, true>);
  else launch(ivf_tile_kernel<ROWS_BF16, true>);
  return hipGetLastError();
}

// Stable counting sort: items 0 .. n - 1 with lists a[i] -> off[nlist + 1], out[j] = value(i) grouped by list, item order kept.
template <typename Value>
long long lists_of(const unsigned* a, long long n, int nlist, std::vector<unsigned>& off, std::vector<unsigned>& out, Value value) {
  off.assign((size_t)nlist + 1, 0u);
  for (long long i = 0; i < n; ++i) ++off[std::min<unsigned>(a[i], (unsigned)nlist - 1u) + 1];
  long long largest = 0;
  for (int l = 0; l < nlist; ++l) {
    largest = std::max<long long>(largest, off[l + 1]);
    off[l + 1] += off[l];
  }
  out.resize((size_t)n);
  std::vector<unsigned> at(off.begin(), off.end() - 1);
  for (long long i = 0; i < n; ++i) out[at[std::min<unsigned>(a[i], (unsigned)nlist - 1u)]++] = value(i);
  return largest;
}

// The lists of the first `size` rows from their assignments (h_assign), on the host and in HBM; under the lock.
int publish_lists(vrag_ivf_index* ix, long long size, hipStream_t st) {
  ix->largest = lists_of(ix->h_assign.data(), size, ix->nlist, ix->h_off, ix->h_rows, [](long long i) { return (unsigned)i; });
  if ((size_t)size > ix->d_rows.n) HIP_TRY(ix->d_rows.grow((size_t)size + (size_t)size / 2));
  HIP_TRY(hipMemcpyAsync(ix->d_off.p, ix->h_off.data(), ix->h_off.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
  if (size) HIP_TRY(hipMemcpyAsync(ix->d_rows.p, ix->h_rows.data(), (size_t)size * sizeof(unsigned), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  ix->n_assigned = size;
  ix->synced = true;
  return VRAG_OK;
}

// The device arrays and the stream of a handle whose base fields are set; on failure the handle is destroyed.
int ivf_open(vrag_ivf_index* ix, vrag_ivf_index** out) {
  hipError_t e = hipSetDevice(ix->device);
  if (e == hipSuccess) e = ix->d_cent.grow((size_t)ix->nlist * ix->dim);
  if (e == hipSuccess && ix->dim != ix->user_dim) e = hipMemset(ix->d_cent.p, 0, (size_t)ix->nlist * ix->dim * sizeof(float));   // the pad columns stay zero
  if (e == hipSuccess) e = ix->d_half.grow((size_t)ix->nlist);
  if (e == hipSuccess) e = ix->d_off.grow((size_t)ix->nlist + 1);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    set_error("ivf index allocation failed: %s", hipGetErrorString(e));
    vrag_ivf_index_destroy(ix);
    return VRAG_ERR_HIP;
  }
  *out = ix;
  return VRAG_OK;
}

}  // namespace

extern "C" {

int vrag_ivf_index_create(vrag_dense_index* base, int32_t nlist, vrag_ivf_index** out) {
  ARG_CHECK(out, "null argument");
  *out = nullptr;
  ARG_CHECK(base, "null base index");
  ARG_CHECK(nlist >= 1 && nlist <= IVF_NLIST_MAX, "nlist must be in [1, %d] (got %d)", IVF_NLIST_MAX, nlist);
  const DenseView v = dense_index_view(base);
  auto* ix = new vrag_ivf_index();
  ix->base = base;
  ix->rows = v.rows, ix->dim = ix->user_dim = v.dim, ix->dtype = v.dtype, ix->device = v.device;
  ix->nlist = nlist;
  return ivf_open(ix, out);
}

int vrag_ivf_index_create_sq8(vrag_sq8_index* base, int32_t nlist, vrag_ivf_index** out) {
  ARG_CHECK(out, "null argument");
  *out = nullptr;
  ARG_CHECK(base, "null base index");
  ARG_CHECK(nlist >= 1 && nlist <= IVF_NLIST_MAX, "nlist must be in [1, %d] (got %d)", IVF_NLIST_MAX, nlist);
  const Sq8View v = sq8_index_view(base);
  auto* ix = new vrag_ivf_index();
  ix->sq8_base = base;
  ix->rows = v.codes, ix->row_scales = v.scales, ix->dim = v.stride, ix->user_dim = v.dim, ix->dtype = ROWS_SQ8, ix->device = v.device;
  ix->nlist = nlist;
  return ivf_open(ix, out);
}

void vrag_ivf_index_destroy(vrag_ivf_index* ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->device);
  (void)hipDeviceSynchronize();
  if (ix->stream) (void)hipStreamDestroy(ix->stream);
  delete ix;   // the device arrays free themselves; the base index is the caller's
}

int vrag_ivf_index_set_centroids(vrag_ivf_index* ix, const float* centroids) {
  ARG_CHECK(ix && centroids, "null argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(copy_rows(ix->d_cent.p, ix->dim * sizeof(float), centroids, ix->user_dim * sizeof(float), ix->user_dim * sizeof(float),
                    (size_t)ix->nlist, hipMemcpyHostToDevice, ix->stream));
  HIP_TRY(half_norms(ix, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  ix->have_centroids = true;
  ix->synced = false;   // the lists belong to the previous centroids
  ix->n_assigned = 0, ix->largest = 0;
  ix->h_assign.clear();
  return VRAG_OK;
}

int vrag_ivf_index_train(vrag_ivf_index* ix, int32_t iters, int64_t max_train_rows) {
  ARG_CHECK(ix, "null argument");
  ARG_CHECK(iters >= 0 && iters <= 1000, "iters must be in [0, 1000] (got %d)", iters);
  ARG_CHECK(max_train_rows >= 1, "max_train_rows must be positive");
  std::lock_guard<std::mutex> lk(ix->mu);
  const long long size = base_view(ix).size;
  ARG_CHECK(size >= 1, "the base index holds no rows to train on");
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t st = ix->stream;
  const long long n_train = std::min<long long>(size, max_train_rows);
  const int nlist = ix->nlist, dim = ix->dim;
  const RowMap sample{0, size, n_train};   // sample item i = base row i * size / n_train
  auto update = [&]() -> hipError_t {   // every non-empty list of (d_toff, d_tmem) -> its mean
    const auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(nlist), dim3(256), 0, st, ix->rows, ix->row_scales, dim, ix->d_toff.p, ix->d_tmem.p, ix->d_cent.p);
    };
    if (ix->dtype == ROWS_F32) launch(ivf_mean_kernel<ROWS_F32>);
    else if (ix->dtype == ROWS_SQ8) launch(ivf_mean_kernel<ROWS_SQ8>);
    else launch(ivf_mean_kernel<ROWS_BF16>);
    return hipGetLastError();
  };
  std::vector<unsigned> a((size_t)n_train), off((size_t)nlist + 1), mem((size_t)nlist);
  HIP_TRY(ix->d_tmem.grow((size_t)std::max<long long>(n_train, nlist)));
  HIP_TRY(ix->d_toff.grow((size_t)nlist + 1));
  // initial centroids: list c = the one sample item c * n_train / nlist (items repeat when the sample is smaller than nlist: ties go
  // to the lowest list, so the repeats end up empty and keep their centroid); the mean of one row is the row
  for (int c = 0; c < nlist; ++c) mem[c] = (unsigned)(((long long)c * n_train / nlist) * size / n_train), off[c] = (unsigned)c;
  off[nlist] = (unsigned)nlist;
  HIP_TRY(hipMemcpyAsync(ix->d_toff.p, off.data(), off.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ix->d_tmem.p, mem.data(), mem.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
  HIP_TRY(update());
  HIP_TRY(hipStreamSynchronize(st));   // `off` and `mem` are rewritten below
  for (int it = 0; it < iters; ++it) {
    HIP_TRY(half_norms(ix, st));
    HIP_TRY(assign_rows(ix, sample, n_train, st));
    HIP_TRY(hipMemcpyAsync(a.data(), ix->d_assign.p, a.size() * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lists_of(a.data(), n_train, nlist, off, mem, [&](long long i) { return (unsigned)(i * size / n_train); });
    HIP_TRY(hipMemcpyAsync(ix->d_toff.p, off.data(), off.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ix->d_tmem.p, mem.data(), mem.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    HIP_TRY(update());
    HIP_TRY(hipStreamSynchronize(st));   // `off` and `mem` are rewritten by the next round
  }
  HIP_TRY(half_norms(ix, st));
  HIP_TRY(hipStreamSynchronize(st));
  ix->have_centroids = true;
  ix->synced = false;
  ix->n_assigned = 0, ix->largest = 0;
  ix->h_assign.clear();
  return VRAG_OK;
}

int vrag_ivf_index_sync(vrag_ivf_index* ix) {
  ARG_CHECK(ix, "null argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  ARG_CHECK(ix->have_centroids, "ivf index has no centroids yet (set_centroids or train first)");
  const long long size = base_view(ix).size;   // read under the base's lock; rows [0, size) are in place
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t st = ix->stream;
  if (size > ix->n_assigned) {
    const long long fresh = size - ix->n_assigned;
    HIP_TRY(assign_rows(ix, RowMap{ix->n_assigned, 1, 1}, fresh, st));
    ix->h_assign.resize((size_t)size);
    HIP_TRY(hipMemcpyAsync(ix->h_assign.data() + ix->n_assigned, ix->d_assign.p, (size_t)fresh * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return publish_lists(ix, size, st);
}

int vrag_ivf_index_remap(vrag_ivf_index* ix, const uint32_t* keep_words, int64_t n_keep) {
  ARG_CHECK(ix, "null argument");
  ARG_CHECK(n_keep >= 0 && (keep_words || n_keep == 0), "bad row bitmap (null words or a negative length)");
  std::lock_guard<std::mutex> lk(ix->mu);
  ARG_CHECK(ix->synced, "ivf index has no lists yet (sync first)");
  ARG_CHECK(n_keep >= ix->n_assigned, "the bitmap covers %lld rows, the lists hold %lld", (long long)n_keep, (long long)ix->n_assigned);
  // The lists are built from the per-row assignments (h_assign, row order): the assignments of the rows that stay, in order, are
  // the assignments of the renumbered rows -- the map is monotonic, so every list keeps its rows' ascending order.
  long long kept = 0;
  for (long long r = 0; r < ix->n_assigned; ++r)
    if ((keep_words[r >> 5] >> (r & 31)) & 1u) ix->h_assign[(size_t)kept++] = ix->h_assign[(size_t)r];
  ix->h_assign.resize((size_t)kept);
  HIP_TRY(hipSetDevice(ix->device));
  return publish_lists(ix, kept, ix->stream);
}

int vrag_ivf_index_stats(vrag_ivf_index* ix, int32_t* nlist, int64_t* n_assigned, int64_t* largest_list) {
  ARG_CHECK(ix, "null argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (nlist) *nlist = ix->nlist;
  if (n_assigned) *n_assigned = ix->n_assigned;
  if (largest_list) *largest_list = ix->largest;
  return VRAG_OK;
}

int vrag_ivf_index_read(vrag_ivf_index* ix, float* centroids, uint32_t* list_off, uint32_t* list_rows) {
  ARG_CHECK(ix, "null argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  ARG_CHECK(!centroids || ix->have_centroids, "ivf index has no centroids yet");
  ARG_CHECK(!(list_off || list_rows) || ix->synced, "ivf index has no lists yet (sync first)");
  HIP_TRY(hipSetDevice(ix->device));
  if (centroids) {
    HIP_TRY(copy_rows(centroids, ix->user_dim * sizeof(float), ix->d_cent.p, ix->dim * sizeof(float), ix->user_dim * sizeof(float),
                      (size_t)ix->nlist, hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
  }
  if (list_off) HIP_TRY(hipMemcpy(list_off, ix->d_off.p, ((size_t)ix->nlist + 1) * sizeof(unsigned), hipMemcpyDeviceToHost));
  if (list_rows && ix->n_assigned)
    HIP_TRY(hipMemcpy(list_rows, ix->d_rows.p, (size_t)ix->n_assigned * sizeof(unsigned), hipMemcpyDeviceToHost));
  return VRAG_OK;
}

int vrag_ivf_index_search(vrag_ivf_index* ix, const float* queries, int32_t nq, int32_t k, int32_t nprobe, float* scores, int64_t* ids,
                          int64_t* scanned_rows, void* stream) {
  ARG_CHECK(ix && queries && scores && ids && nq > 0, "bad arguments");
  ARG_CHECK(k >= 1 && k <= KMAX, "k must be in [1, %d] for an ivf search (got %d)", KMAX, k);
  ARG_CHECK(nprobe >= 1, "nprobe must be positive (got %d)", nprobe);
  std::lock_guard<std::mutex> lk(ix->mu);
  ARG_CHECK(ix->synced, "ivf index has no lists yet (sync first)");
  {
    const BaseView v = base_view(ix);
    ARG_CHECK(v.dim == ix->user_dim && v.rows == ix->rows, "the base index does not match the one this overlay was created on");
  }
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : ix->stream;
  const int dim = ix->dim, nlist = ix->nlist;
  const int np = std::min<int>(nprobe, nlist);
  const bool all = np == nlist;
  const auto ceil_div = [](long long a, long long b) { return (a + b - 1) / b; };
  long long want = ceil_div(IVF_SPLIT_WGS, (long long)nq * np);                       // few pairs: more workgroups per work item
  if (!all) want = std::max(want, ceil_div(ix->largest, IVF_SPLIT_ROWS_MAX));         // an oversized list: bounded row ranges
  want = std::min(want, std::max<long long>(1, ceil_div(ix->largest, IVF_SPLIT_ROWS_MIN)));
  want = std::min(want, std::max<long long>(1, IVF_SLICE_KEYS / ((long long)np * k)));
  const int split = (int)std::max<long long>(1, std::min<long long>(want, IVF_SPLIT_MAX));
  long long per = std::min<long long>(IVF_SLICE_QUERIES, IVF_SLICE_KEYS / ((long long)np * k * split));
  if (!all) per = std::min<long long>(per, std::max<long long>(1, IVF_SLICE_SCORES / nlist));
  const int nqs_max = (int)std::min<long long>(nq, std::max<long long>(1, per));
  const long long pairs_max = (long long)nqs_max * np;
  int cap = 2;
  while (cap < nlist) cap <<= 1;
  HIP_TRY(ix->d_q.grow((size_t)nq * dim));
  HIP_TRY(ix->d_out.grow((size_t)nq * k));
  HIP_TRY(ix->d_scanned.grow((size_t)nq));
  HIP_TRY(ix->d_cand.grow((size_t)pairs_max * split * k));
  HIP_TRY(ix->d_cnt.grow((size_t)nlist));
  HIP_TRY(ix->d_goff.grow((size_t)nlist + 1));
  HIP_TRY(ix->d_place.grow((size_t)pairs_max));
  HIP_TRY(ix->d_item_list.grow((size_t)pairs_max));
  HIP_TRY(ix->d_item_n.grow((size_t)pairs_max));
  HIP_TRY(ix->d_item_pair.grow((size_t)pairs_max * IVF_QG));
  if (!all) {
    HIP_TRY(ix->d_scores.grow((size_t)nqs_max * nlist));
    HIP_TRY(ix->d_probe.grow((size_t)pairs_max));
    HIP_TRY((set_max_dynamic_lds<ivf_select_kernel>(IVF_NLIST_MAX * (int)sizeof(u64))));
  }
  const bool sq8 = ix->dtype == ROWS_SQ8;
  if (dim != ix->user_dim) HIP_TRY(hipMemsetAsync(ix->d_q.p, 0, (size_t)nq * dim * sizeof(float), st));   // pad columns: zero
  HIP_TRY(copy_rows(ix->d_q.p, dim * sizeof(float), queries, ix->user_dim * sizeof(float), ix->user_dim * sizeof(float), (size_t)nq,
                    hipMemcpyHostToDevice, st));
  if (sq8) {   // the queries by the rows' rule, once per search; the zero pad columns change neither the scale nor a code
    HIP_TRY(ix->d_qc.grow((size_t)nq * dim));
    HIP_TRY(ix->d_qs.grow((size_t)nq));
    HIP_TRY(launch_sq8_query(ix->d_q.p, nq, dim, dim, ix->d_qc.p, ix->d_qs.p, st));
  }
  HIP_TRY(hipMemsetAsync(ix->d_scanned.p, 0, (size_t)nq * sizeof(unsigned long long), st));
  for (int q0 = 0; q0 < nq; q0 += nqs_max) {
    const int nqs = std::min(nqs_max, nq - q0);
    const long long pairs = (long long)nqs * np;
    const float* dq = ix->d_q.p + (size_t)q0 * dim;
    const unsigned* probe = nullptr;
    if (!all) {
      const dim3 grid((nqs + TM - 1) / TM, (nlist + TN - 1) / TN);
      hipLaunchKernelGGL((ivf_tile_kernel<ROWS_F32, false>), grid, dim3(256), 0, st, dq, (const float*)nullptr, RowMap{0, 1, 1}, (long long)nqs,
                         dim, ix->d_cent.p, ix->d_half.p, nlist, (unsigned*)nullptr, ix->d_scores.p);
      hipLaunchKernelGGL(ivf_select_kernel, dim3(nqs), dim3(1024), (size_t)cap * sizeof(u64), st, ix->d_scores.p, nlist, cap, np, ix->d_probe.p);
      HIP_TRY(hipGetLastError());
      probe = ix->d_probe.p;
    }
    HIP_TRY(hipMemsetAsync(ix->d_cnt.p, 0, (size_t)nlist * sizeof(unsigned), st));
    const dim3 pgrid((unsigned)((pairs + 255) / 256));
    hipLaunchKernelGGL(ivf_count_kernel, pgrid, dim3(256), 0, st, probe, pairs, np, ix->d_off.p, ix->d_cnt.p, ix->d_place.p, ix->d_scanned.p + q0);
    hipLaunchKernelGGL(ivf_groups_kernel, dim3(1), dim3(256), 0, st, ix->d_cnt.p, nlist, ix->d_goff.p);
    hipLaunchKernelGGL(ivf_fill_kernel, pgrid, dim3(256), 0, st, probe, pairs, np, ix->d_cnt.p, ix->d_place.p, ix->d_goff.p, ix->d_item_list.p,
                       ix->d_item_n.p, ix->d_item_pair.p);
    const dim3 sgrid((unsigned)std::min<long long>(pairs, IVF_SCAN_WGS), split);
    if (sq8)
      HIP_TRY(launch_ivf_sq8_scan(sgrid, reinterpret_cast<const signed char*>(ix->rows), ix->row_scales, dim, ix->d_off.p, ix->d_rows.p,
                                  ix->d_qc.p + (size_t)q0 * dim, ix->d_qs.p + q0, nqs, k, ix->d_goff.p + nlist, ix->d_item_list.p,
                                  ix->d_item_n.p, ix->d_item_pair.p, ix->d_cand.p, st));
    else if (ix->dtype == ROWS_F32)
      hipLaunchKernelGGL(ivf_scan_kernel<true>, sgrid, dim3(256), 0, st, ix->rows, dim, ix->d_off.p, ix->d_rows.p, dq, nqs, k, ix->d_goff.p + nlist,
                         ix->d_item_list.p, ix->d_item_n.p, ix->d_item_pair.p, ix->d_cand.p);
    else
      hipLaunchKernelGGL(ivf_scan_kernel<false>, sgrid, dim3(256), 0, st, ix->rows, dim, ix->d_off.p, ix->d_rows.p, dq, nqs, k, ix->d_goff.p + nlist,
                         ix->d_item_list.p, ix->d_item_n.p, ix->d_item_pair.p, ix->d_cand.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_topk_merge(ix->d_cand.p, np * split, nqs, k, ix->d_out.p + (size_t)q0 * k, st));
  }
  // the scanned-row counts ride on the one stream sync of read_lists: their copy is enqueued ahead of it
  std::vector<unsigned long long> scanned(scanned_rows ? (size_t)nq : 0);
  if (scanned_rows) HIP_TRY(hipMemcpyAsync(scanned.data(), ix->d_scanned.p, scanned.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  if (const int rc = read_lists(ix->d_out.p, nq, k, st, scores, ids)) return rc;
  for (size_t q = 0; q < scanned.size(); ++q) scanned_rows[q] = (int64_t)scanned[q];
  return VRAG_OK;
}

}  // extern "C"
