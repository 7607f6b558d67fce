// Grouping search over a dense index (include/vrag_amd.h, vrag_group_column_* / vrag_dense_index_search_grouped): per query the best
// n_groups groups of the passing rows, each with its best group_size rows, under the order (score desc, row asc) of every search
// in this tree.  A group is a dense int32 code per row, held by a vrag_group_column the caller keeps beside the index.
//
//   score    grouped_score_kernel: filtered_score_kernel's step (csrc/topk.hip) -- 16 rows x 16 queries, FCH columns of both staged
//            through LDS in 16-byte pieces, one serial chain  acc = fmaf(x[c], q[c], acc), c ascending  per (row, query) thread -- over
//            csrc/compact.hip's ascending list of the passing rows, or over rows 0 .. n - 1 when no bitmap is given.  Same chain,
//            same operands: the scores are vrag_dense_index_search_filtered's bit for bit.
//   reduce   levels[group_size][queries of the slice][n_codes] u64 keys (make_key: the maximum is the best hit), 0 = empty.  A key
//            enters its group's levels by the carry cascade, j ascending:  old = atomicMax(&level[j], key); key = min(old, key);
//            until the carried key is 0.  At level j every key that ever arrives leaves again except the largest, so level j receives
//            every inserted key but the j largest and ends as the (j + 1)-th largest -- whatever the interleaving: the result does
//            not depend on the order rows are scored in.  Keys are unique per (score, row), so `old == key` never happens.  A key
//            that a load shows below the group's LAST level is dropped before its atomics: levels only grow, so a stale read
//            can only let a key through, never drop one that belongs -- and a shard that is one group does not serialise on
//            group_size addresses once these hold good keys.
//   select   grouped_select_kernel: a workgroup takes SEL_KEYS codes of one query's level 0 into registers and writes their best
//            n_groups keys, sorted; launch_topk_merge (csrc/topk.hip) merges the per-workgroup lists.
//   gather   grouped_gather_kernel: the chosen groups' code and every level's (score, row).
// Queries are processed in slices whose levels fit GROUPED_SCRATCH_BYTES, GROUPED_SLICE_QUERIES at the most.
#include <cmath>
#include <cstring>

#include "common.h"
#include "compact.h"
#include "host_util.h"
#include "topk_kernels.h"

namespace vrag {

// Bytes of level keys one query slice may hold (the handle's largest allocation); one query needs 8 * group_size * n_codes.
constexpr size_t GROUPED_SCRATCH_BYTES = VRAG_GROUPED_SCRATCH_BYTES;

namespace {

constexpr int GROWS = 16, GQT = 16, GCH = 256;   // rows and queries per step, columns per LDS stage (filtered_score_kernel's shape)
constexpr int GROUPED_SLICE_QUERIES = 4096;       // queries per slice at the most (the selection's grid has one row per query)
constexpr int GROUPED_WGS = 2048;                 // most workgroups of the scoring pass per query tile
constexpr int SEL_PER = 16, SEL_KEYS = 256 * SEL_PER;   // level-0 keys per thread / per workgroup of the selection

// list == nullptr: rows 0 .. n_all - 1; else the first *cnt_p entries of list (at least one: the host launches nothing otherwise).
// levels: [gs][nq][n_codes], this slice's; queries: this slice's [nq][dim].
template <bool F32>
__global__ __launch_bounds__(256) void grouped_score_kernel(const unsigned* __restrict__ list, const unsigned* __restrict__ cnt_p,
                                                             unsigned n_all, const void* __restrict__ rows_v, int dim,
                                                             const float* __restrict__ queries, int nq, const int* __restrict__ codes,
                                                             u64* levels, int gs, long long n_codes) {
  __shared__ __attribute__((aligned(16))) float srow[GROWS][GCH + 4];
  __shared__ __attribute__((aligned(16))) float sq[GQT][GCH + 4];
  __shared__ unsigned srid[GROWS];
  __shared__ int scode[GROWS];
  const int tid = threadIdx.x, r = tid & (GROWS - 1), qi = tid >> 4;
  const int q0 = blockIdx.y * GQT, nqt = min(GQT, nq - q0);
  const unsigned n = list ? *cnt_p : n_all;
  const unsigned n_steps = (n + GROWS - 1) / GROWS;
  const size_t level_stride = (size_t)nq * (size_t)n_codes;
  constexpr int PW = F32 ? 4 : 8;   // columns of a 16-byte piece of a row
  for (unsigned g = blockIdx.x; g < n_steps; g += gridDim.x) {
    const unsigned base = g * GROWS;
    __syncthreads();   // the previous step's chains and insertions are done with srid / scode
    if (tid < GROWS) {
      const unsigned at = min(base + tid, n - 1u);   // slots behind the end re-read the last row; their keys are dropped
      const unsigned row = list ? list[at] : at;
      srid[tid] = row;
      scode[tid] = codes[row];
    }
    __syncthreads();
    float acc = 0.f;
    for (int c0 = 0; c0 < dim; c0 += GCH) {
      const int w = min(GCH, dim - c0);   // dim % 8 == 0 (vrag_dense_index_create)
      const int ppr = w / PW, total = GROWS * ppr;
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
        *reinterpret_cast<f32x4*>(&sq[qq][cc]) = *reinterpret_cast<const f32x4*>(queries + (size_t)(q0 + qq) * dim + c0 + cc);
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
    if (qi < nqt && base + r < n) {
      u64 key = make_key(acc, srid[r]);
      u64* lv = levels + (size_t)(q0 + qi) * (size_t)n_codes + (size_t)scode[r];
      // a relaxed device-scope load (read at the L2, not from this CU's vector cache): below the last level = not among the
      // group's best gs, now or later
      if (key < __hip_atomic_load(lv + (size_t)(gs - 1) * level_stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) key = 0ull;
      for (int j = 0; j < gs && key != 0ull; ++j) {
        const u64 old = atomicMax(lv + (size_t)j * level_stride, key);
        key = old < key ? old : key;
      }
    }
  }
}

// level0: [nq][n_codes] of the slice.  Workgroup (x, q): the best k keys of codes [x * SEL_KEYS, (x + 1) * SEL_KEYS) of query q,
// sorted descending with a zero tail, to cand[x][q][k].  Keys of different groups name different rows: unique, so removing the
// round's maximum removes one key.
__global__ __launch_bounds__(256) void grouped_select_kernel(const u64* __restrict__ level0, long long n_codes, int nq, int k,
                                                              u64* __restrict__ cand) {
  __shared__ u64 red[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.y;
  const u64* src = level0 + (size_t)q * (size_t)n_codes;
  const long long c0 = (long long)blockIdx.x * SEL_KEYS + tid;
  u64 keys[SEL_PER];
#pragma unroll
  for (int i = 0; i < SEL_PER; ++i) {
    const long long c = c0 + 256ll * i;
    keys[i] = c < n_codes ? src[c] : 0ull;
  }
  u64* out = cand + ((size_t)blockIdx.x * nq + q) * k;
  for (int round = 0; round < k; ++round) {
    u64 best = 0ull;
#pragma unroll
    for (int i = 0; i < SEL_PER; ++i) best = keys[i] > best ? keys[i] : best;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const u64 other = __shfl_xor(best, o, 64);
      best = other > best ? other : best;
    }
    if (lane == 0) red[round & 1][wave] = best;
    __syncthreads();   // red[round & 1] is rewritten two rounds on, behind the next round's barrier
    u64 b = red[round & 1][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) b = red[round & 1][w] > b ? red[round & 1][w] : b;
    if (b == 0ull) {   // exhausted (uniform over the workgroup): the tail stays empty
      for (int j = round + tid; j < k; j += 256) out[j] = 0ull;
      break;
    }
    if (tid == 0) out[round] = b;
#pragma unroll
    for (int i = 0; i < SEL_PER; ++i) keys[i] = keys[i] == b ? 0ull : keys[i];
  }
}

// sel: [nq][ng] merged level-0 keys of the slice (0 = no group).  One thread per (query, group): the group's code and the
// (score, row) of each of its levels; missing entries -1 / -inf, a missing group code -1.
__global__ __launch_bounds__(256) void grouped_gather_kernel(const u64* __restrict__ sel, const int* __restrict__ codes,
                                                              const u64* __restrict__ levels, int nq, int ng, int gs, long long n_codes,
                                                              float* __restrict__ scores, long long* __restrict__ ids,
                                                              int* __restrict__ groups) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nq * ng) return;
  const int q = i / ng;
  const u64 head = sel[i];
  int code = -1;
  if (head != 0ull) code = codes[0xFFFFFFFFu - (unsigned)(head & 0xFFFFFFFFull)];
  groups[i] = code;
  const size_t level_stride = (size_t)nq * (size_t)n_codes;
  for (int j = 0; j < gs; ++j) {
    const u64 key = code >= 0 ? levels[(size_t)j * level_stride + (size_t)q * (size_t)n_codes + (size_t)code] : 0ull;
    scores[(size_t)i * gs + j] = key ? unorderable((unsigned)(key >> 32)) : -INFINITY;
    ids[(size_t)i * gs + j] = key ? (long long)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)) : -1ll;
  }
}

}  // namespace
}  // namespace vrag

using namespace vrag;

struct vrag_group_column {
  int device = 0;
  int64_t size = 0;       // rows that hold a code
  int64_t n_codes = 0;    // largest code + 1
  DevArray<int> d_codes;  // [capacity >= size]
  hipStream_t stream = nullptr;
  std::mutex mu;
  // scratch of vrag_dense_index_search_grouped (grown on demand)
  std::vector<unsigned> h_allow;
  RowList allow_rows;     // the ascending list of the rows that pass the caller's bitmap
  DevArray<float> d_q, d_scores;
  DevArray<u64> d_levels, d_cand, d_sel;
  DevArray<long long> d_ids;
  DevArray<int> d_groups;
};

extern "C" {

int vrag_group_column_create(int32_t device, vrag_group_column** out) {
  ARG_CHECK(out, "null argument");
  *out = nullptr;
  ARG_CHECK(device >= 0, "vrag_group_column_create: negative device");
  DEVICE_CHECK(device);
  HIP_TRY(hipSetDevice(device));
  auto* c = new vrag_group_column();
  c->device = device;
  const hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    set_error("group column stream creation failed: %s", hipGetErrorString(e));
    vrag_group_column_destroy(c);
    return VRAG_ERR_HIP;
  }
  *out = c;
  return VRAG_OK;
}

void vrag_group_column_destroy(vrag_group_column* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamDestroy(c->stream);
  }
  delete c;   // the device arrays free themselves
}

int vrag_group_column_append(vrag_group_column* c, const int32_t* codes, int64_t n) {
  ARG_CHECK(c && n >= 0 && (codes || n == 0), "vrag_group_column_append: bad arguments");
  int32_t top = -1;
  for (int64_t i = 0; i < n; ++i) {
    ARG_CHECK(codes[i] >= 0, "vrag_group_column_append: negative group code %d at entry %lld", codes[i], (long long)i);
    top = std::max(top, codes[i]);
  }
  std::lock_guard<std::mutex> lk(c->mu);
  ARG_CHECK(c->size + n <= 0xFFFFFFFFll, "a group column holds at most 2^32 - 1 rows");
  if (n == 0) return VRAG_OK;
  HIP_TRY(hipSetDevice(c->device));
  const size_t need = (size_t)(c->size + n);
  if (need > c->d_codes.n) {   // grow with headroom, keeping the codes in place so far
    DevArray<int> bigger;
    HIP_TRY(bigger.grow(need + need / 2));
    if (c->size) HIP_TRY(hipMemcpyAsync(bigger.p, c->d_codes.p, (size_t)c->size * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->d_codes = std::move(bigger);
  }
  HIP_TRY(hipMemcpyAsync(c->d_codes.p + c->size, codes, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->size += n;
  c->n_codes = std::max<int64_t>(c->n_codes, (int64_t)top + 1);
  return VRAG_OK;
}

int64_t vrag_group_column_size(vrag_group_column* c) {
  if (!c) return 0;
  std::lock_guard<std::mutex> lk(c->mu);
  return c->size;
}

int vrag_dense_index_search_grouped(vrag_dense_index* ix, const float* queries, int32_t nq, int32_t n_groups, int32_t group_size,
                                    vrag_group_column* column, const uint32_t* allow, int64_t n_allow, float* scores, int64_t* ids,
                                    int32_t* groups, void* stream) {
  ARG_CHECK(ix && queries && column && scores && ids && groups && nq > 0, "bad arguments");
  ARG_CHECK(n_groups >= 1 && n_groups <= KMAX, "n_groups must be in [1, %d] for a grouped search (got %d)", KMAX, n_groups);
  ARG_CHECK(group_size >= 1 && group_size <= VRAG_GROUPED_MAX_SIZE, "group_size must be in [1, %d] (got %d)", VRAG_GROUPED_MAX_SIZE,
            group_size);
  ARG_CHECK(n_allow >= 0 && (allow || n_allow == 0), "bad row bitmap (null words or a negative length)");
  std::lock_guard<std::mutex> lk(column->mu);
  const std::unique_lock<std::mutex> index_lk = dense_index_lock(ix);   // column first, index second: the one order in this file
  const DenseView v = dense_index_view_locked(ix);
  ARG_CHECK(v.device == column->device, "the group column lives on device %d, the index on device %d", column->device, v.device);
  const long long n_codes = std::max<long long>(column->n_codes, 1);
  const size_t per_query = (size_t)group_size * (size_t)n_codes * sizeof(u64);
  ARG_CHECK(per_query <= GROUPED_SCRATCH_BYTES,
            "one query's levels (group_size %d x %lld group codes x 8 bytes) exceed the %zu MiB of a grouped search's scratch",
            group_size, n_codes, GROUPED_SCRATCH_BYTES >> 20);
  const size_t n_out = (size_t)nq * n_groups;
  auto no_hits = [&]() {
    fill_no_hits(scores, ids, n_out * group_size);
    for (size_t i = 0; i < n_out; ++i) groups[i] = -1;
    return VRAG_OK;
  };
  long long n_rows = std::min<long long>(v.size, column->size);
  if (allow) n_rows = std::min<long long>(n_rows, n_allow);   // rows appended after the mask was built are not in it
  const long long n_pass = !allow ? n_rows : (n_rows > 0 ? stage_bitmap(column->h_allow, allow, n_rows, FWORDS) : 0);
  if (n_pass == 0) return no_hits();   // nothing passes: no launch
  HIP_TRY(hipSetDevice(column->device));
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : column->stream;
  const int dim = v.dim, ng = n_groups, gs = group_size;
  int nqs_max = (int)std::min<size_t>(std::min<int>(nq, GROUPED_SLICE_QUERIES), GROUPED_SCRATCH_BYTES / per_query);
  if (nqs_max > GQT) nqs_max -= nqs_max % GQT;   // whole query tiles of the scoring pass
  const int n_wg = (int)std::min<long long>((n_pass + GROWS - 1) / GROWS, GROUPED_WGS);
  const int n_sel = (int)((n_codes + SEL_KEYS - 1) / SEL_KEYS);
  HIP_TRY(column->d_q.grow((size_t)nq * dim));
  HIP_TRY(column->d_levels.grow((size_t)nqs_max * gs * (size_t)n_codes));
  HIP_TRY(column->d_cand.grow((size_t)n_sel * nqs_max * ng));
  HIP_TRY(column->d_sel.grow((size_t)nqs_max * ng));
  HIP_TRY(column->d_scores.grow(n_out * gs));
  HIP_TRY(column->d_ids.grow(n_out * gs));
  HIP_TRY(column->d_groups.grow(n_out));
  HIP_TRY(hipMemcpyAsync(column->d_q.p, queries, (size_t)nq * dim * sizeof(float), hipMemcpyHostToDevice, st));
  const unsigned* list = nullptr;
  const unsigned* list_n = nullptr;
  if (allow) {
    HIP_TRY(column->allow_rows.build(column->h_allow, n_pass, st));
    list = column->allow_rows.rows();
    list_n = column->allow_rows.count();
  }
  for (int q0 = 0; q0 < nq; q0 += nqs_max) {
    const int nqs = std::min(nqs_max, nq - q0);
    HIP_TRY(hipMemsetAsync(column->d_levels.p, 0, (size_t)nqs * per_query, st));
    const dim3 grid(n_wg, (nqs + GQT - 1) / GQT);
    const float* dq = column->d_q.p + (size_t)q0 * dim;
    if (v.dtype == 1)   // dtype 2 too: the chains run over the fp32 rows, never over the bf16 image
      hipLaunchKernelGGL(grouped_score_kernel<true>, grid, dim3(256), 0, st, list, list_n, (unsigned)n_rows, v.rows, dim, dq, nqs,
                         column->d_codes.p, column->d_levels.p, gs, n_codes);
    else
      hipLaunchKernelGGL(grouped_score_kernel<false>, grid, dim3(256), 0, st, list, list_n, (unsigned)n_rows, v.rows, dim, dq, nqs,
                         column->d_codes.p, column->d_levels.p, gs, n_codes);
    hipLaunchKernelGGL(grouped_select_kernel, dim3(n_sel, nqs), dim3(256), 0, st, column->d_levels.p, n_codes, nqs, ng, column->d_cand.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_topk_merge(column->d_cand.p, n_sel, nqs, ng, column->d_sel.p, st));
    hipLaunchKernelGGL(grouped_gather_kernel, dim3((nqs * ng + 255) / 256), dim3(256), 0, st, column->d_sel.p, column->d_codes.p,
                       column->d_levels.p, nqs, ng, gs, n_codes, column->d_scores.p + (size_t)q0 * ng * gs,
                       column->d_ids.p + (size_t)q0 * ng * gs, column->d_groups.p + (size_t)q0 * ng);
    HIP_TRY(hipGetLastError());
  }
  static_assert(sizeof(long long) == sizeof(int64_t), "ids are copied out as they lie");
  HIP_TRY(hipMemcpyAsync(scores, column->d_scores.p, n_out * gs * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(ids, column->d_ids.p, n_out * gs * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(groups, column->d_groups.p, n_out * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return VRAG_OK;
}

}  // extern "C"
