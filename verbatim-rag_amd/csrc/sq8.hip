// SQ8 dense rows (vrag_sq8_index): int8 codes + one fp32 scale per row, integer-exact scores + C ABI.
//
// The rule, the score and the limits are stated in include/vrag_amd.h ("SQ8 dense rows"); this file restates none of it.  What
// matters here: with int8 rows AND int8 queries the dot product is an int32 that every summation order reproduces, and the score
// is three fp32 roundings of it -- so the two search kernels below, which walk the columns in different orders on different
// units, return the same bits.
//
// Storage: codes [capacity][stride] int8, stride = dim rounded up to 16 bytes with zero pad codes; scales [capacity] fp32.
//
// Search, per slice of up to SQ8_SLICE queries (the slice bounds the candidate scratch, not the result):
//   queries  sq8_query_kernel quantises the fp32 queries by the rows' rule -> codes [nq][stride], scales [nq]
//   scan     sq8_scan_kernel (route 1): the streaming form.  A wave step covers 8 rows: 16 lanes per row, 16 bytes of codes per lane
//            and load, two rows per lane in flight; the codes of SQ8_QG queries sit in LDS, v_dot4_i32_i8 into one int32 per
//            (row, query), a DPP sum over the row's 16 lanes.  Each wave keeps its own sorted lists in LDS (a key enters only
//            above the list's current last key; insert_key by one lane at a time), so the row loop has no barrier; the four
//            lists of a query are merged when the workgroup leaves.  More than SQ8_QG queries = more passes over the shard.
//   tile     sq8_tile_kernel (route 2): the batch form.  A workgroup step covers 256 rows x 64 query columns: each wave 64 rows
//            as four 16-row blocks of v_mfma_i32_16x16x64_i8, the rows' operand loaded straight from HBM (lane = row l & 15,
//            bytes 16 (l >> 4) .. + 16 of the 64-byte k-step), the queries' operand from an LDS image staged 512 columns at a
//            time.  Both operands take their bytes from the same columns of the same k-step, so whatever order the unit gives
//            the 64 products of a step, the int32 sum is the rule's.  Epilogue per 16-row block: keys through LDS, all 256 threads
//            mark the keys above their query's last key, one thread per query inserts the marked ones.
//   merge    launch_topk_merge (csrc/topk.hip) over the per-workgroup lists cand[workgroup][query][k].
// k > KMAX: exact pages of KMAX through make_key_below, as vrag_dense_index_search pages.
// Bitmap (search_filtered): both kernels drop the keys of rows without a bit; the pass still streams the shard.
//
// SQ8_SCAN_MAX_Q: the automatic route scans up to this many queries and tiles above.  4 = one pass of the scan kernel, kept by
// profiles/sq8_probe.txt (1.25 M x 768 rows, k = 10): 1 query 0.25 ms scan / 0.43 ms tile, 4 queries 0.40 / 0.49, 32 queries
// 2.51 / 0.64 -- a fifth query would start a second scan pass, which costs more than the one tile pass it then takes.  The
// constant changes no output: both routes return the same bits.
#include "../../include/vrag_amd.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "common.h"
#include "compact.h"
#include "host_util.h"
#include "sq8_kernels.h"
#include "topk_kernels.h"

namespace vrag {
namespace {

constexpr int SQ8_DIM_MAX = 4096;
constexpr int SQ8_SCAN_MAX_Q = 4;
constexpr int SQ8_SLICE = 64;                 // queries of one kernel launch (the tile kernel's column count)
constexpr int SQ8_QG = 4;                     // queries of one pass of the scan kernel
constexpr int SQ8_WAVE_ROWS = 8;              // rows of a wave step of the scan kernel: 4 groups of 16 lanes x 2 rows
constexpr int SQ8_TILE_ROWS = 256;            // rows of a workgroup step of the tile kernel
constexpr int SQ8_KC = 512, SQ8_PITCH = SQ8_KC + 16;   // columns of a staged query image, its LDS row pitch
constexpr int SQ8_KEY_PITCH = 65;             // u64 per query of the epilogue's key image (64 rows + 1: bank spread)
constexpr int SQ8_UNION_BYTES = SQ8_SLICE * SQ8_PITCH;   // the query image; the key image (64 * 65 * 8 bytes) fits in it
static_assert(SQ8_SLICE * SQ8_KEY_PITCH * 8 <= SQ8_UNION_BYTES, "key image larger than the query image");
constexpr int SQ8_SCAN_WGS_PER_CU = 4, SQ8_TILE_WGS_PER_CU = 2;

template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, true); }
// integer sum over each aligned group of 16 lanes, in every lane of the group (row16_sum's steps; exact in any order)
__device__ __forceinline__ int row16_sum_i32(int v) {
  v += dpp_i32<0xB1>(v);
  v += dpp_i32<0x4E>(v);
  v += dpp_i32<0x141>(v);
  v += dpp_i32<0x140>(v);
  return v;
}

__device__ __forceinline__ bool row_allowed(const unsigned* __restrict__ allow, long long row) {
  return !allow || ((allow[row >> 5] >> (unsigned)(row & 31)) & 1u);
}

// ------------------------------------------------------------------------------------ quantisation
// One wave: x[dim] -> codes[stride] (16-byte stores, pad codes zero) and the scale.  The maximum is exact in any order.
__device__ __forceinline__ void sq8_quantize_row(const float* __restrict__ x, int dim, int stride, signed char* __restrict__ codes,
                                                 float* __restrict__ scale, int lane) {
  float m = 0.f;
  for (int c = lane; c < dim; c += 64) m = fmaxf(m, fabsf(x[c]));
  m = wave_max(m);
  const float s = __fdiv_rn(m, 127.0f);
  for (int p = lane; p < stride / 16; p += 64) {
    i32x4 w;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned word = 0u;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int c = p * 16 + j * 4 + b;
        int code = 0;
        if (c < dim && m > 0.f) {
          const float r = rintf(__fdiv_rn(x[c], s));
          code = (int)fminf(fmaxf(r, -127.f), 127.f);
        }
        word |= ((unsigned)code & 0xFFu) << (8 * b);
      }
      w[j] = (int)word;
    }
    *reinterpret_cast<i32x4*>(codes + (size_t)p * 16) = w;
  }
  if (lane == 0) *scale = s;
}

// Rows [0, n) of fp32 `rows` -> codes / scales of the shard, four rows (waves) per workgroup.
__global__ __launch_bounds__(256) void sq8_quantize_kernel(const float* __restrict__ rows, long long n, int dim, int stride,
                                                            signed char* __restrict__ codes, float* __restrict__ scales) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  sq8_quantize_row(rows + (size_t)r * dim, dim, stride, codes + (size_t)r * stride, scales + r, threadIdx.x & 63);
}

// The same rule for a query batch: codes [nq][stride] row-major (both search kernels read 16-byte pieces of a query's row).
__global__ __launch_bounds__(256) void sq8_query_kernel(const float* __restrict__ queries, int nq, int dim, int stride,
                                                         signed char* __restrict__ qcodes, float* __restrict__ qscales) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  sq8_quantize_row(queries + (size_t)q * dim, dim, stride, qcodes + (size_t)q * stride, qscales + q, threadIdx.x & 63);
}

// ------------------------------------------------------------------------------------ scan (route 1)
// grid: any; workgroup b's wave w takes the wave steps (4 b + w) + i * 4 gridDim.x.  cand [gridDim.x][nq][k].
__global__ __launch_bounds__(256) void sq8_scan_kernel(const signed char* __restrict__ codes, const float* __restrict__ scales,
                                                        long long n, int stride, const signed char* __restrict__ qcodes,
                                                        const float* __restrict__ qscales, int nq, int k,
                                                        const unsigned* __restrict__ allow, const u64* __restrict__ bound,
                                                        u64* __restrict__ cand) {
  __shared__ __attribute__((aligned(16))) signed char sq[SQ8_QG][SQ8_DIM_MAX];
  __shared__ u64 lists[4][SQ8_QG][KMAX];
  __shared__ float qs[SQ8_QG];   // the group's query scales and page bounds
  __shared__ u64 bd[SQ8_QG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sub = lane & 15, grp = lane >> 4;
  const int chunks = stride / 16;
  const long long first = ((long long)blockIdx.x * 4 + wave) * SQ8_WAVE_ROWS, step = (long long)gridDim.x * 4 * SQ8_WAVE_ROWS;
  for (int q0 = 0; q0 < nq; q0 += SQ8_QG) {
    const int nqt = min(SQ8_QG, nq - q0);
    __syncthreads();   // the previous group's lists have been written out; its last reads of sq are done
    for (int p = tid; p < SQ8_QG * chunks; p += 256) {
      const int qq = p / chunks, c = p % chunks;
      i32x4 v = {0, 0, 0, 0};
      if (qq < nqt) v = *reinterpret_cast<const i32x4*>(qcodes + (size_t)(q0 + qq) * stride + (size_t)c * 16);
      *reinterpret_cast<i32x4*>(&sq[qq][c * 16]) = v;
    }
    for (int i = tid; i < 4 * SQ8_QG * KMAX; i += 256) (&lists[0][0][0])[i] = 0ull;
    if (tid < SQ8_QG) {
      qs[tid] = tid < nqt ? qscales[q0 + tid] : 0.f;
      bd[tid] = (bound && tid < nqt) ? bound[q0 + tid] : ~0ull;
    }
    __syncthreads();
    for (long long base = first; base < n; base += step) {
      const long long row0 = base + grp, row1 = base + 4 + grp;
      const signed char* p0 = codes + (size_t)min(row0, n - 1) * stride;   // rows behind the end re-read the last one; their keys are dropped
      const signed char* p1 = codes + (size_t)min(row1, n - 1) * stride;
      int acc0[SQ8_QG], acc1[SQ8_QG];
#pragma unroll
      for (int j = 0; j < SQ8_QG; ++j) acc0[j] = 0, acc1[j] = 0;
      for (int c = sub; c < chunks; c += 16) {
        const i32x4 a0 = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(p0 + (size_t)c * 16));
        const i32x4 a1 = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(p1 + (size_t)c * 16));
#pragma unroll
        for (int j = 0; j < SQ8_QG; ++j) {
          const i32x4 b = *reinterpret_cast<const i32x4*>(&sq[j][c * 16]);
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            acc0[j] = __builtin_amdgcn_sdot4(a0[w], b[w], acc0[j], false);
            acc1[j] = __builtin_amdgcn_sdot4(a1[w], b[w], acc1[j], false);
          }
        }
      }
      const bool ok0 = sub == 0 && row0 < n && row_allowed(allow, min(row0, n - 1));
      const bool ok1 = sub == 0 && row1 < n && row_allowed(allow, min(row1, n - 1));
      const float sr0 = scales[min(row0, n - 1)], sr1 = scales[min(row1, n - 1)];
#pragma unroll
      for (int j = 0; j < SQ8_QG; ++j) {
        if (j >= nqt) break;   // uniform
        const int d0 = row16_sum_i32(acc0[j]), d1 = row16_sum_i32(acc1[j]);
        u64* list = lists[wave][j];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const u64 key = (s ? ok1 : ok0) ? make_key_below(sq8_score(s ? d1 : d0, qs[j], s ? sr1 : sr0), (unsigned)(s ? row1 : row0), bd[j]) : 0ull;
          unsigned long long want = __ballot(key > list[k - 1]);   // this wave alone writes the list: the last key is current
          while (want) {
            const int b = __builtin_ctzll(want);
            want &= want - 1;
            if (lane == b) insert_key(list, k, key);
            __builtin_amdgcn_wave_barrier();
          }
        }
      }
    }
    __syncthreads();
    if (tid < nqt) {   // the four waves' lists of query q0 + tid -> one (keys are unique per row, rows are disjoint between waves)
      int h0 = 0, h1 = 0, h2 = 0, h3 = 0;
      u64* out = cand + ((size_t)blockIdx.x * nq + q0 + tid) * k;
      for (int i = 0; i < k; ++i) {
        const u64 v0 = h0 < k ? lists[0][tid][h0] : 0ull, v1 = h1 < k ? lists[1][tid][h1] : 0ull;
        const u64 v2 = h2 < k ? lists[2][tid][h2] : 0ull, v3 = h3 < k ? lists[3][tid][h3] : 0ull;
        const u64 a = v0 > v1 ? v0 : v1, b = v2 > v3 ? v2 : v3, best = a > b ? a : b;
        out[i] = best;
        if (best != 0ull) {
          if (best == v0) ++h0;
          else if (best == v1) ++h1;
          else if (best == v2) ++h2;
          else ++h3;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------ tile (route 2)
// nq <= SQ8_SLICE query columns.  Dynamic LDS: lists [SQ8_SLICE][k] u64 | query image [SQ8_SLICE][SQ8_PITCH], reused as the key
// image [SQ8_SLICE][SQ8_KEY_PITCH] u64 | marks [4][SQ8_SLICE] u16.  grid: any; workgroup b takes tiles b, b + gridDim.x, ...
// MFMA maps (16x16x64, i8): A lane l = row l & 15, B lane l = column l & 15, both with the 16 bytes 16 (l >> 4) .. of the k-step;
// D register g of lane l = row 4 (l >> 4) + g, column l & 15.
__global__ __launch_bounds__(256) void sq8_tile_kernel(const signed char* __restrict__ codes, const float* __restrict__ scales,
                                                        long long n, int stride, const signed char* __restrict__ qcodes,
                                                        const float* __restrict__ qscales, int nq, int k,
                                                        const unsigned* __restrict__ allow, const u64* __restrict__ bound,
                                                        u64* __restrict__ cand) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u64* lists = reinterpret_cast<u64*>(smem);
  char* un = smem + (size_t)SQ8_SLICE * k * sizeof(u64);
  signed char* sB = reinterpret_cast<signed char*>(un);
  u64* skey = reinterpret_cast<u64*>(un);
  unsigned short* smark = reinterpret_cast<unsigned short*>(un + SQ8_UNION_BYTES);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
  for (int i = tid; i < SQ8_SLICE * k; i += 256) lists[i] = 0ull;
  float qs[4];
  u64 bd[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int col = t * 16 + l15;
    qs[t] = col < nq ? qscales[col] : 0.f;
    bd[t] = (bound && col < nq) ? bound[col] : ~0ull;
  }
  const long long n_tiles = (n + SQ8_TILE_ROWS - 1) / SQ8_TILE_ROWS;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long row0 = tile * SQ8_TILE_ROWS + wave * 64;
    i32x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[m][t] = i32x4{0, 0, 0, 0};
    const signed char* arow[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) arow[m] = codes + (size_t)min(row0 + m * 16 + l15, n - 1) * stride;   // rows behind the end: dropped below
    for (int kc = 0; kc < stride; kc += SQ8_KC) {
      const int w = min(SQ8_KC, stride - kc), w64 = (w + 63) & ~63, pieces = w64 / 16;
      __syncthreads();   // the previous chunk's reads of the query image / the previous tile's insertions from the key image are done
      for (int p = tid; p < SQ8_SLICE * pieces; p += 256) {
        const int col = p / pieces, o = (p % pieces) * 16;
        i32x4 v = {0, 0, 0, 0};
        if (col < nq && o < w) v = *reinterpret_cast<const i32x4*>(qcodes + (size_t)col * stride + kc + o);
        *reinterpret_cast<i32x4*>(sB + col * SQ8_PITCH + o) = v;
      }
      __syncthreads();
      for (int ks = 0; ks < w64; ks += 64) {
        const int o = ks + 16 * l4;
        i32x4 a[4], b[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          a[m] = i32x4{0, 0, 0, 0};
          if (o < w) a[m] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(arow[m] + kc + o));
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) b[t] = *reinterpret_cast<const i32x4*>(sB + (t * 16 + l15) * SQ8_PITCH + o);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[m][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[m], b[t], acc[m][t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      __syncthreads();   // the image is free: the MFMA loop's reads (m = 0) / the previous block's insertions are done
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const long long row = row0 + m * 16 + l4 * 4 + g;
        const bool ok = row < n && row_allowed(allow, min(row, n - 1));
        const float sr = scales[min(row, n - 1)];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int col = t * 16 + l15;
          const u64 key = (ok && col < nq) ? make_key_below(sq8_score(acc[m][t][g], qs[t], sr), (unsigned)row, bd[t]) : 0ull;
          skey[col * SQ8_KEY_PITCH + wave * 16 + l4 * 4 + g] = key;
        }
      }
      __syncthreads();
      {
        const int q = tid & 63, part = tid >> 6;
        const u64 last = lists[q * k + k - 1];
        unsigned mark = 0u;
#pragma unroll
        for (int i = 0; i < 16; ++i) mark |= (skey[q * SQ8_KEY_PITCH + part * 16 + i] > last ? 1u : 0u) << i;
        smark[part * SQ8_SLICE + q] = (unsigned short)mark;
      }
      __syncthreads();
      if (tid < nq) {
        for (int part = 0; part < 4; ++part) {
          unsigned mark = smark[part * SQ8_SLICE + tid];
          while (mark) {
            const int i = __builtin_ctz(mark);
            mark &= mark - 1;
            insert_key(lists + tid * k, k, skey[tid * SQ8_KEY_PITCH + part * 16 + i]);
          }
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < nq * k; i += 256) cand[(size_t)blockIdx.x * nq * k + i] = lists[i];
}

constexpr int sq8_tile_lds(int k) { return SQ8_SLICE * k * (int)sizeof(u64) + SQ8_UNION_BYTES + 4 * SQ8_SLICE * (int)sizeof(unsigned short); }

}  // namespace
}  // namespace vrag

using namespace vrag;

struct vrag_sq8_index {
  int dim = 0, stride = 0, device = 0, n_cu = 0;
  int route = 0;   // vrag_sq8_index_set_route
  int64_t capacity = 0, size = 0;
  DevArray<signed char> codes;   // [capacity][stride]
  DevArray<float> scales;        // [capacity]
  DevArray<float> stage;         // device fp32 staging for add()
  size_t stage_rows = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  // scratch (grown on demand)
  DevArray<float> d_q, d_qs;
  DevArray<signed char> d_qc;
  DevArray<u64> d_cand, d_out, d_bound;
  DevArray<unsigned> d_allow;
  std::vector<unsigned> h_allow;
  CompactScratch compact;   // vrag_sq8_index_compact: its bitmap, row list and bounce buffer
};

namespace {

hipError_t sq8_quantize(vrag_sq8_index* ix, const float* d_rows, long long n, long long at, hipStream_t st) {
  hipLaunchKernelGGL(sq8_quantize_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, d_rows, n, ix->dim, ix->stride,
                     ix->codes.p + (size_t)at * ix->stride, ix->scales.p + at);
  return hipGetLastError();
}

// The device form of an append, under the lock: `n` fp32 rows at the device address `d_rows` are quantised behind the rows in
// place on `st`; the size is published after the stream has drained, so a search never sees a row that is not written yet.
int sq8_append(vrag_sq8_index* ix, const float* d_rows, int64_t n, hipStream_t st) {
  if (ix->size + n > ix->capacity) {
    set_error("sq8 index full: %lld + %lld > capacity %lld", (long long)ix->size, (long long)n, (long long)ix->capacity);
    return VRAG_ERR_CAPACITY;
  }
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(sq8_quantize(ix, d_rows, n, ix->size, st));
  HIP_TRY(hipStreamSynchronize(st));   // ingest is not the hot path
  ix->size += n;
  return VRAG_OK;
}

// The search over rows [0, n_rows) (with `allow`: those whose bit is set in the staged bitmap ix->h_allow), under the lock.
int sq8_search(vrag_sq8_index* ix, const float* queries, int nq, int k, long long n_rows, bool filtered, float* scores, int64_t* ids,
               hipStream_t st) {
  const int dim = ix->dim, stride = ix->stride, kk = std::min<int>(k, KMAX);
  const bool tile = ix->route == 2 || (ix->route == 0 && nq > SQ8_SCAN_MAX_Q);
  const int slice = std::min<int>(nq, SQ8_SLICE);
  const long long steps = tile ? (n_rows + SQ8_TILE_ROWS - 1) / SQ8_TILE_ROWS : (n_rows + 4 * SQ8_WAVE_ROWS - 1) / (4 * SQ8_WAVE_ROWS);
  const int n_wg = (int)std::min<long long>(steps, (long long)ix->n_cu * (tile ? SQ8_TILE_WGS_PER_CU : SQ8_SCAN_WGS_PER_CU));
  HIP_TRY(ix->d_q.grow((size_t)nq * dim));
  HIP_TRY(ix->d_qc.grow((size_t)nq * stride));
  HIP_TRY(ix->d_qs.grow((size_t)nq));
  HIP_TRY(ix->d_cand.grow((size_t)n_wg * slice * kk));
  HIP_TRY(ix->d_out.grow((size_t)nq * kk));
  const unsigned* d_allow = nullptr;
  if (filtered) {
    HIP_TRY(ix->d_allow.grow(ix->h_allow.size()));
    HIP_TRY(hipMemcpyAsync(ix->d_allow.p, ix->h_allow.data(), ix->h_allow.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    d_allow = ix->d_allow.p;
  }
  if (tile) HIP_TRY((set_max_dynamic_lds<sq8_tile_kernel>(sq8_tile_lds(KMAX))));
  HIP_TRY(hipMemcpyAsync(ix->d_q.p, queries, (size_t)nq * dim * sizeof(float), hipMemcpyHostToDevice, st));
  HIP_TRY(launch_sq8_query(ix->d_q.p, nq, dim, stride, ix->d_qc.p, ix->d_qs.p, st));
  // one page of kk keys per query into d_out [nq][kk]
  return search_lists(nq, k, ix->d_bound, ix->d_out, st, [&](const u64* bound) -> int {
    for (int q0 = 0; q0 < nq; q0 += SQ8_SLICE) {
      const int nqs = std::min(SQ8_SLICE, nq - q0);
      const signed char* qc = ix->d_qc.p + (size_t)q0 * stride;
      const float* qsc = ix->d_qs.p + q0;
      const u64* bd = bound ? bound + q0 : nullptr;
      if (tile)
        hipLaunchKernelGGL(sq8_tile_kernel, dim3(n_wg), dim3(256), (size_t)sq8_tile_lds(kk), st, ix->codes.p, ix->scales.p, n_rows, stride, qc,
                           qsc, nqs, kk, d_allow, bd, ix->d_cand.p);
      else
        hipLaunchKernelGGL(sq8_scan_kernel, dim3(n_wg), dim3(256), 0, st, ix->codes.p, ix->scales.p, n_rows, stride, qc, qsc, nqs, kk,
                           d_allow, bd, ix->d_cand.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(launch_topk_merge(ix->d_cand.p, n_wg, nqs, kk, ix->d_out.p + (size_t)q0 * kk, st));
    }
    return VRAG_OK;
  }, scores, ids);
}

}  // namespace

namespace vrag {

hipError_t launch_sq8_query(const float* queries, int nq, int dim, int stride, signed char* qcodes, float* qscales, hipStream_t st) {
  hipLaunchKernelGGL(sq8_query_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, queries, nq, dim, stride, qcodes, qscales);
  return hipGetLastError();
}

Sq8View sq8_index_view(vrag_sq8_index* ix) {
  std::lock_guard<std::mutex> lk(ix->mu);
  return Sq8View{ix->codes.p, ix->scales.p, ix->stride, ix->dim, ix->device, (long long)ix->size};
}

}  // namespace vrag

extern "C" {

int vrag_sq8_index_create(int32_t dim, int64_t capacity, int32_t device, vrag_sq8_index** out) {
  ARG_CHECK(out, "null argument");
  *out = nullptr;
  ARG_CHECK(dim >= 1 && dim <= SQ8_DIM_MAX, "dim must be in [1, %d] for an sq8 index (got %d)", SQ8_DIM_MAX, dim);
  ARG_CHECK(capacity > 0 && capacity < 0xFFFFFFFFll, "capacity out of range");
  ARG_CHECK(device >= 0, "device must not be negative");
  DEVICE_CHECK(device);
  HIP_TRY(hipSetDevice(device));
  auto* ix = new vrag_sq8_index();
  ix->dim = dim;
  ix->stride = (dim + 15) & ~15;
  ix->device = device;
  ix->capacity = capacity;
  hipError_t e = hipDeviceGetAttribute(&ix->n_cu, hipDeviceAttributeMultiprocessorCount, device);
  if (e == hipSuccess) e = ix->codes.grow((size_t)capacity * ix->stride);
  if (e == hipSuccess) e = ix->scales.grow((size_t)capacity);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking);
  ix->stage_rows = std::max<size_t>(1, std::min<size_t>((size_t)capacity, ((size_t)64 << 20) / ((size_t)dim * 4)));
  if (e == hipSuccess) e = ix->stage.grow(ix->stage_rows * dim);
  if (e != hipSuccess || ix->n_cu < 1) {
    set_error("sq8 index allocation failed: %s", hipGetErrorString(e));
    vrag_sq8_index_destroy(ix);
    return VRAG_ERR_HIP;
  }
  *out = ix;
  return VRAG_OK;
}

void vrag_sq8_index_destroy(vrag_sq8_index* ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->device);
  (void)hipDeviceSynchronize();
  if (ix->stream) (void)hipStreamDestroy(ix->stream);
  delete ix;   // the device arrays free themselves
}

int64_t vrag_sq8_index_size(vrag_sq8_index* ix) {
  if (!ix) return -1;
  std::lock_guard<std::mutex> lk(ix->mu);
  return ix->size;
}

int vrag_sq8_index_add_device(vrag_sq8_index* ix, const float* rows, int64_t n, void* stream) {
  ARG_CHECK(ix && rows && n > 0, "bad arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  return sq8_append(ix, rows, n, reinterpret_cast<hipStream_t>(stream));
}

int vrag_sq8_index_add(vrag_sq8_index* ix, const float* rows, int64_t n) {
  ARG_CHECK(ix && rows && n > 0, "bad arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (ix->size + n > ix->capacity) {   // all or nothing: checked before the first slab
    set_error("sq8 index full: %lld + %lld > capacity %lld", (long long)ix->size, (long long)n, (long long)ix->capacity);
    return VRAG_ERR_CAPACITY;
  }
  HIP_TRY(hipSetDevice(ix->device));
  for (int64_t r0 = 0; r0 < n; r0 += (int64_t)ix->stage_rows) {   // slabs through the staging buffer, each appended by the device form
    const int64_t nr = std::min<int64_t>((int64_t)ix->stage_rows, n - r0);
    HIP_TRY(hipMemcpyAsync(ix->stage.p, rows + (size_t)r0 * ix->dim, (size_t)nr * ix->dim * sizeof(float), hipMemcpyHostToDevice, ix->stream));
    const int rc = sq8_append(ix, ix->stage.p, nr, ix->stream);
    if (rc != VRAG_OK) return rc;
  }
  return VRAG_OK;
}

int vrag_sq8_index_read(vrag_sq8_index* ix, int64_t first_row, int64_t n, int8_t* codes, float* scales) {
  ARG_CHECK(ix && first_row >= 0 && n >= 0, "bad arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  ARG_CHECK(first_row + n <= ix->size, "rows [%lld, %lld) are not all in the index (size %lld)", (long long)first_row,
            (long long)(first_row + n), (long long)ix->size);
  if (n == 0) return VRAG_OK;
  HIP_TRY(hipSetDevice(ix->device));
  if (codes)
    HIP_TRY(hipMemcpy2D(codes, (size_t)ix->dim, ix->codes.p + (size_t)first_row * ix->stride, (size_t)ix->stride, (size_t)ix->dim, (size_t)n,
                        hipMemcpyDeviceToHost));
  if (scales) HIP_TRY(hipMemcpy(scales, ix->scales.p + first_row, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  return VRAG_OK;
}

// Drops the rows whose bit is cleared, in place (csrc/compact.h): the codes at their padded stride (a multiple of 16 bytes) and the
// scales.  Every search of this handle returns host lists and has drained its stream before it let go of the lock.
int vrag_sq8_index_compact(vrag_sq8_index* ix, const uint32_t* keep_words, int64_t n_keep, int64_t* new_size) {
  ARG_CHECK(ix && new_size, "null argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  return compact_arrays(ix->compact, ix->device, ix->stream, keep_words, n_keep, &ix->size, new_size,
                        {{ix->codes.p, (size_t)ix->stride}, {ix->scales.p, sizeof(float)}});
}

int vrag_sq8_index_set_route(vrag_sq8_index* ix, int32_t route) {
  ARG_CHECK(ix, "null argument");
  ARG_CHECK(route >= 0 && route <= 2, "route: 0 = automatic, 1 = scan kernel, 2 = tile kernel (got %d)", route);
  std::lock_guard<std::mutex> lk(ix->mu);
  ix->route = route;
  return VRAG_OK;
}

int vrag_sq8_index_search(vrag_sq8_index* ix, const float* queries, int32_t nq, int32_t k, float* scores, int64_t* ids, void* stream) {
  ARG_CHECK(ix && queries && scores && ids && nq > 0, "bad arguments");
  ARG_CHECK(k >= 1 && k <= 1024, "k must be in [1, 1024] (got %d)", k);
  std::lock_guard<std::mutex> lk(ix->mu);
  if (ix->size == 0) {
    fill_no_hits(scores, ids, (size_t)nq * k);
    return VRAG_OK;
  }
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : ix->stream;
  return sq8_search(ix, queries, nq, k, ix->size, false, scores, ids, st);
}

int vrag_sq8_index_search_filtered(vrag_sq8_index* ix, const float* queries, int32_t nq, int32_t k, const uint32_t* allow, int64_t n_allow,
                                   float* scores, int64_t* ids, void* stream) {
  ARG_CHECK(ix && queries && scores && ids && nq > 0, "bad arguments");
  ARG_CHECK(k >= 1 && k <= 1024, "k must be in [1, 1024] (got %d)", k);
  ARG_CHECK(n_allow >= 0 && (allow || n_allow == 0), "bad row bitmap (null words or a negative length)");
  std::lock_guard<std::mutex> lk(ix->mu);
  const long long n_rows = std::min<long long>(n_allow, ix->size);   // rows appended after the mask was built are not in it
  const long long n_pass = n_rows > 0 ? stage_bitmap(ix->h_allow, allow, n_rows, 1) : 0;
  if (n_pass == 0) {   // nothing passes: no launch
    fill_no_hits(scores, ids, (size_t)nq * k);
    return VRAG_OK;
  }
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : ix->stream;
  return sq8_search(ix, queries, nq, k, n_rows, true, scores, ids, st);
}

}  // extern "C"
