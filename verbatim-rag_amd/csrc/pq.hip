// PQ dense rows (vrag_pq_index): 8-bit product codes, one byte per sub-vector, scored through a per-query look-up table + C ABI.
//
// The rule (codebooks, encoding, score, training) and the limits are stated in include/vrag_amd.h ("PQ dense rows"); this file
// restates none of it.  What matters here: every chain is one lane's sequential fmaf loop and every score is one lane's m
// dependent fp32 additions in j order, so there is ONE summation order per number and the tests compare bits.  The file is
// compiled with fp contraction off (the pragma below): `chain - h` and the score's additions stay the operations the header names.
//
// Storage: codes [capacity][stride] bytes, stride = m rounded up to 16 with zero pad bytes (the array is zeroed once; encode
// writes bytes [0, m) only and compaction moves whole rows); codebooks cb [m][256][dsub] fp32 and their half norms h [m][256].
//
// Ingest and training
//   pq_half_kernel    h[j][c] = 0.5f * chain(cb[j][c], cb[j][c]), one thread per centroid.
//   pq_encode_kernel  a workgroup = one sub-space x PQ_ENC_ROWS rows.  The sub-space's 256 centroids sit transposed in LDS
//                     ([t][c]: lane c reads consecutive words), lane c runs the chain of centroid c against a row's sub-vector
//                     (broadcast reads), eight rows per round; the argmax (lowest c on ties) is a wave reduction per row and one
//                     thread per row over the four waves' winners.  add() and the training's assignment step launch it alike.
//   pq_mean_kernel    one wave per (sub-space, centroid): the wave reads the sample's codes 64 rows at a time, and walks the set
//                     bits of the match ballot in ascending row order, lanes over dsub adding the member's sub-vector -- the
//                     sequential fp32 sum of the contract -- then one correctly rounded division by (float)count.
//   Training is not the hot path: the mean kernel reads every code of the sample once per centroid (L2-resident for the
//   65 536-row samples the store trains on).
//
// Search, per slice of up to PQ_SLICE queries (the slice bounds the table and candidate scratch, not the result):
//   tables   pq_lut_kernel: LUT[q][j][c] = chain(q_j, cb[j][c]) into HBM scratch, one thread per entry.
//   scan     pq_scan_kernel, the hot path.  grid (row ranges, queries): a workgroup of 16 waves owns one query and one contiguous
//            range of rows.  It copies the query's table (m KiB) into LDS, then every lane scores PQ_R rows at a time: 16 code
//            bytes per row and load, each byte one ds_read_b32 of table segment j, the m additions of a row in j order, PQ_R
//            independent chains per lane in flight.  Keys enter per-wave sorted lists in LDS (only above the list's last key;
//            insert_key by one lane at a time, so the row loop has no barrier); the 16 lists are merged by one wave when the
//            workgroup leaves.
//   merge    launch_topk_merge (csrc/topk.hip) over the per-workgroup lists cand[range][query][k].
// k > KMAX: exact pages of KMAX through make_key_below, as vrag_sq8_index_search pages.
// Bitmap (search_filtered): the scan drops the keys of rows without a bit; the pass still streams the shard.
//
// What bounds the scan loop.  Per code byte a lane issues one ds_read_b32 at a data-dependent address inside the 1 KiB segment
// of sub-space j: the 32 lanes of a read group fall on 32 banks at random, a few deep on the fullest bank, so the LDS array --
// not the code stream (one byte of HBM traffic per look-up) and not the VALU (a shift-and-mask, an address add and the fp32 add
// per byte) -- sets the pace.  Measured (profiles/pq_probe.txt, m = 96): SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.66, a read
// group takes about three LDS cycles instead of one; 1.25 M rows cost 44 us per query.  The table takes m KiB of the CU's 160
// KiB, which caps occupancy at one workgroup per CU from m = 80 up (two below); hence 1024-thread workgroups, 4 waves per SIMD,
// which ds_read_b32 needs to reach its rate.
// Resources (tools/kernel_resources.py verbatim-rag_amd/csrc/pq.hip, gfx950; VGPRs, no AGPRs, zero scratch and zero spills in
// every kernel): pq_scan_kernel 78 (under the 128 that 16 waves per CU allow; LDS m KiB + 16 lists of k keys, 136 KiB at the most),
// pq_encode_kernel 56 (LDS (256 + 64) dsub floats, 80 KiB at the most), pq_lut_kernel 26, pq_mean_kernel 14, pq_half_kernel 6.
//
// Layout: row-major codes.  A wave's 16-byte loads of 64 consecutive rows touch 64 x stride contiguous bytes over m / 16 loads,
// every fetched line is used in full through L1/L2; a row-block-interleaved layout was not tried.
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

#pragma clang fp contract(off)

namespace vrag {
namespace {

constexpr int PQ_DIM_MAX = 4096, PQ_M_MAX = 128, PQ_DSUB_MAX = 64, PQ_KSUB = 256;
constexpr int PQ_SLICE = 64;                   // queries of one table build + scan launch
constexpr int PQ_THREADS = 1024, PQ_WAVES = PQ_THREADS / 64;
constexpr int PQ_R = 4;                        // rows a lane scores at a time (independent chains in flight)
constexpr int PQ_WG_STEP = PQ_THREADS * PQ_R;  // rows of one step of a workgroup's main loop
constexpr int PQ_WGS_PER_CU_MAX = 2;           // 2 x 16 waves = the CU's 32
constexpr int PQ_LDS_BUDGET = 160 * 1024;
constexpr int PQ_ENC_ROWS = 64, PQ_ENC_ROUND = 8;   // rows of an encode workgroup, rows of one of its rounds
constexpr int PQ_TRAIN_ITERS_MAX = 1000;

constexpr int pq_scan_lds(int m) { return m * PQ_KSUB * (int)sizeof(float) + PQ_WAVES * KMAX * (int)sizeof(u64); }
static_assert(pq_scan_lds(PQ_M_MAX) <= PQ_LDS_BUDGET, "the largest table and the lists must fit the CU's LDS");

__device__ __forceinline__ bool pq_row_allowed(const unsigned* __restrict__ allow, long long row) {
  return !allow || ((allow[row >> 5] >> (unsigned)(row & 31)) & 1u);
}

// ------------------------------------------------------------------------------------ codebook norms
__global__ __launch_bounds__(256) void pq_half_kernel(const float* __restrict__ cb, int n_cent, int dsub, float* __restrict__ half) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_cent) return;
  const float* v = cb + (size_t)i * dsub;
  float acc = 0.f;
  for (int t = 0; t < dsub; ++t) acc = fmaf(v[t], v[t], acc);
  half[i] = 0.5f * acc;
}

// ------------------------------------------------------------------------------------ encode
// grid (ceil(n / PQ_ENC_ROWS), m).  rows [n][dim] fp32 (device); codes [n][stride], byte j of every row written.
// Dynamic LDS: centroids [dsub][256] | sub-vectors [PQ_ENC_ROWS][dsub] | winners value [PQ_ENC_ROUND][4] + index [PQ_ENC_ROUND][4].
__global__ __launch_bounds__(256) void pq_encode_kernel(const float* __restrict__ rows, long long n, int dim, int dsub,
                                                         const float* __restrict__ cb, const float* __restrict__ half,
                                                         unsigned char* __restrict__ codes, int stride) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* scb = reinterpret_cast<float*>(smem);                 // [dsub][256]
  float* sx = scb + (size_t)dsub * PQ_KSUB;                    // [PQ_ENC_ROWS][dsub]
  float* wv = sx + (size_t)PQ_ENC_ROWS * dsub;                 // [PQ_ENC_ROUND][4]
  int* wi = reinterpret_cast<int*>(wv + PQ_ENC_ROUND * 4);     // [PQ_ENC_ROUND][4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = blockIdx.y;
  const long long r0 = (long long)blockIdx.x * PQ_ENC_ROWS;
  const int nr = (int)min((long long)PQ_ENC_ROWS, n - r0);
  const float* cbj = cb + (size_t)j * PQ_KSUB * dsub;
  for (int i = tid; i < PQ_KSUB * dsub; i += 256) {            // coalesced read of [c][t], transposed store
    const int c = i / dsub, t = i - c * dsub;
    scb[t * PQ_KSUB + c] = cbj[i];
  }
  for (int i = tid; i < nr * dsub; i += 256) {
    const int r = i / dsub, t = i - r * dsub;
    sx[i] = rows[(size_t)(r0 + r) * dim + (size_t)j * dsub + t];
  }
  const float h = half[j * PQ_KSUB + tid];
  __syncthreads();
  for (int b = 0; b < nr; b += PQ_ENC_ROUND) {
    float acc[PQ_ENC_ROUND];
#pragma unroll
    for (int i = 0; i < PQ_ENC_ROUND; ++i) acc[i] = 0.f;
    for (int t = 0; t < dsub; ++t) {
      const float c = scb[t * PQ_KSUB + tid];
#pragma unroll
      for (int i = 0; i < PQ_ENC_ROUND; ++i) acc[i] = fmaf(sx[min(b + i, nr - 1) * dsub + t], c, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < PQ_ENC_ROUND; ++i) {
      float v = acc[i] - h;
      int c = tid;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oc = __shfl_xor(c, o, 64);
        if (ov > v || (ov == v && oc < c)) v = ov, c = oc;
      }
      if (lane == 0) wv[i * 4 + wave] = v, wi[i * 4 + wave] = c;
    }
    __syncthreads();
    if (tid < PQ_ENC_ROUND && b + tid < nr) {
      float v = wv[tid * 4];
      int c = wi[tid * 4];
      for (int w = 1; w < 4; ++w) {      // waves hold ascending centroids: a later wave wins only when strictly greater
        const float ov = wv[tid * 4 + w];
        if (ov > v) v = ov, c = wi[tid * 4 + w];
      }
      codes[(size_t)(r0 + b + tid) * stride + j] = (unsigned char)c;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------ ordered mean (training)
// One wave per (sub-space, centroid): grid (64 waves-of-4 per sub-space, m), wave w of workgroup b = centroid 4 b + w.
// An empty cluster leaves its centroid as it is.  new_cb may not alias cb of another wave's centroid: each wave writes only its own.
__global__ __launch_bounds__(256) void pq_mean_kernel(const float* __restrict__ rows, long long n, int dim, int dsub,
                                                       const unsigned char* __restrict__ codes, int stride, float* __restrict__ cb) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6), j = blockIdx.y;
  float sum = 0.f;
  long long count = 0;
  for (long long r0 = 0; r0 < n; r0 += 64) {
    const long long r = r0 + lane;
    const bool hit = r < n && codes[(size_t)min(r, n - 1) * stride + j] == (unsigned char)c;
    unsigned long long want = __ballot(hit);
    count += __popcll(want);
    while (want) {
      const int b = __builtin_ctzll(want);
      want &= want - 1;
      if (lane < dsub) sum = sum + rows[(size_t)(r0 + b) * dim + (size_t)j * dsub + lane];
    }
  }
  if (count > 0 && lane < dsub) cb[((size_t)j * PQ_KSUB + c) * dsub + lane] = __fdiv_rn(sum, (float)count);
}

// ------------------------------------------------------------------------------------ tables
// grid (m, nq): lut[q][j][c] = chain(q_j, cb[j][c]), thread c.
__global__ __launch_bounds__(256) void pq_lut_kernel(const float* __restrict__ queries, int dim, int m, int dsub,
                                                      const float* __restrict__ cb, float* __restrict__ lut) {
  __shared__ float sq[PQ_DSUB_MAX];
  const int j = blockIdx.x, q = blockIdx.y, c = threadIdx.x;
  if (c < dsub) sq[c] = queries[(size_t)q * dim + (size_t)j * dsub + c];
  __syncthreads();
  const float* v = cb + ((size_t)j * PQ_KSUB + c) * dsub;
  float acc = 0.f;
  for (int t = 0; t < dsub; ++t) acc = fmaf(sq[t], v[t], acc);
  lut[((size_t)q * m + j) * PQ_KSUB + c] = acc;
}

// ------------------------------------------------------------------------------------ scan
// R rows of one lane: rows base + i * PQ_THREADS, i < R, of the range [.., hi); a row at or behind hi re-reads row hi - 1 and its
// key is dropped.  The additions of a row run in j order.
template <int R>
__device__ __forceinline__ void pq_scan_rows(const unsigned char* __restrict__ codes, int stride, int m, const float* __restrict__ lut,
                                             long long base, long long hi, const unsigned* __restrict__ allow, u64 bound, u64* list,
                                             int k, int lane) {
  long long row[R];
  const unsigned char* p[R];
  float acc[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    row[i] = base + (long long)i * PQ_THREADS;
    p[i] = codes + (size_t)min(row[i], hi - 1) * stride;
    acc[i] = 0.f;
  }
  const int full = m >> 4, rest = m & 15;
  for (int c = 0; c < full; ++c) {
    i32x4 v[R];
#pragma unroll
    for (int i = 0; i < R; ++i) v[i] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(p[i] + (size_t)c * 16));
    const float* t = lut + (size_t)c * 16 * PQ_KSUB;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int i = 0; i < R; ++i) acc[i] = acc[i] + t[(w * 4 + b) * PQ_KSUB + (((unsigned)v[i][w] >> (8 * b)) & 255u)];
  }
  if (rest) {   // uniform: the last, partly filled 16 bytes (pad bytes are never looked up)
    i32x4 v[R];
#pragma unroll
    for (int i = 0; i < R; ++i) v[i] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(p[i] + (size_t)full * 16));
    const float* t = lut + (size_t)full * 16 * PQ_KSUB;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (w * 4 + b >= rest) break;
#pragma unroll
        for (int i = 0; i < R; ++i) acc[i] = acc[i] + t[(w * 4 + b) * PQ_KSUB + (((unsigned)v[i][w] >> (8 * b)) & 255u)];
      }
  }
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const bool ok = row[i] < hi && pq_row_allowed(allow, min(row[i], hi - 1));
    const u64 key = ok ? make_key_below(acc[i], (unsigned)row[i], bound) : 0ull;
    unsigned long long want = __ballot(key > list[k - 1]);   // this wave alone writes the list: the last key is current
    while (want) {
      const int b = __builtin_ctzll(want);
      want &= want - 1;
      if (lane == b) insert_key(list, k, key);
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// grid (n_wg, nq): workgroup (b, q) scores rows [b * per, min(n, (b + 1) * per)) for query q.  lut [nq][m][256]; cand [n_wg][nq][k].
// Dynamic LDS: table [m][256] fp32 | lists [PQ_WAVES][k] u64.
__global__ __launch_bounds__(PQ_THREADS) void pq_scan_kernel(const unsigned char* __restrict__ codes, long long n, long long per,
                                                              int stride, int m, const float* __restrict__ lut, int nq, int k,
                                                              const unsigned* __restrict__ allow, const u64* __restrict__ bound,
                                                              u64* __restrict__ cand) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* slut = reinterpret_cast<float*>(smem);
  u64* lists = reinterpret_cast<u64*>(smem + (size_t)m * PQ_KSUB * sizeof(float));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.y;
  {
    const f32x4* src = reinterpret_cast<const f32x4*>(lut + (size_t)q * m * PQ_KSUB);
    f32x4* dst = reinterpret_cast<f32x4*>(slut);
    for (int i = tid; i < m * (PQ_KSUB / 4); i += PQ_THREADS) dst[i] = src[i];
  }
  for (int i = tid; i < PQ_WAVES * k; i += PQ_THREADS) lists[i] = 0ull;
  const u64 bd = bound ? bound[q] : ~0ull;
  __syncthreads();
  const long long lo = (long long)blockIdx.x * per, hi = min(n, lo + per);
  u64* list = lists + wave * k;
  long long wbase = lo + (tid - lane);   // the wave's first row of a round: both loops' trip counts are wave-uniform
  for (; wbase + (long long)(PQ_R - 1) * PQ_THREADS < hi; wbase += PQ_WG_STEP)   // steps of PQ_R rows per lane
    pq_scan_rows<PQ_R>(codes, stride, m, slut, wbase + lane, hi, allow, bd, list, k, lane);
  for (; wbase < hi; wbase += PQ_THREADS)   // the rest of the range, one row per lane and round
    pq_scan_rows<1>(codes, stride, m, slut, wbase + lane, hi, allow, bd, list, k, lane);
  __syncthreads();
  if (wave == 0) {   // 16-way merge: lane w < 16 walks list w; keys are unique per row and rows are disjoint between waves
    int h = 0;
    u64* out = cand + ((size_t)blockIdx.x * nq + q) * k;
    for (int i = 0; i < k; ++i) {
      const u64 v = (lane < PQ_WAVES && h < k) ? lists[lane * k + h] : 0ull;
      u64 best = v;
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        const u64 other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
      }
      best = __shfl(best, 0, 64);
      if (lane == 0) out[i] = best;
      if (best != 0ull && v == best) ++h;
    }
  }
}

}  // namespace
}  // namespace vrag

using namespace vrag;

struct vrag_pq_index {
  int dim = 0, m = 0, dsub = 0, stride = 0, device = 0, n_cu = 0;
  bool has_codebooks = false;
  int64_t capacity = 0, size = 0;
  DevArray<unsigned char> codes;   // [capacity][stride]
  DevArray<float> cb, half;        // [m][256][dsub], [m][256]
  DevArray<float> stage;           // device fp32 staging for add()
  size_t stage_rows = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  // scratch (grown on demand)
  DevArray<float> d_q, d_lut;
  DevArray<u64> d_cand, d_out, d_bound;
  DevArray<unsigned> d_allow;
  std::vector<unsigned> h_allow;
  DevArray<float> train_rows;            // vrag_pq_index_train: the sample and its codes, freed when the call returns
  DevArray<unsigned char> train_codes;
  CompactScratch compact;
};

namespace {

size_t pq_cb_floats(const vrag_pq_index* ix) { return (size_t)ix->m * PQ_KSUB * ix->dsub; }
int pq_encode_lds(int dsub) { return (PQ_KSUB * dsub + PQ_ENC_ROWS * dsub + PQ_ENC_ROUND * 8) * (int)sizeof(float); }

hipError_t pq_half(vrag_pq_index* ix, hipStream_t st) {
  const int n_cent = ix->m * PQ_KSUB;
  hipLaunchKernelGGL(pq_half_kernel, dim3((n_cent + 255) / 256), dim3(256), 0, st, ix->cb.p, n_cent, ix->dsub, ix->half.p);
  return hipGetLastError();
}

// d_rows [n][dim] fp32 on the device -> byte j < m of codes [n][stride], by the handle's codebooks.
hipError_t pq_encode(vrag_pq_index* ix, const float* d_rows, long long n, unsigned char* codes, hipStream_t st) {
  const hipError_t e = set_max_dynamic_lds<pq_encode_kernel>(pq_encode_lds(PQ_DSUB_MAX));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pq_encode_kernel, dim3((unsigned)((n + PQ_ENC_ROWS - 1) / PQ_ENC_ROWS), (unsigned)ix->m), dim3(256),
                     (size_t)pq_encode_lds(ix->dsub), st, d_rows, n, ix->dim, ix->dsub, ix->cb.p, ix->half.p, codes, ix->stride);
  return hipGetLastError();
}

// The device form of an append, under the lock (sq8_append's shape): encoded behind the rows in place on `st`, the size
// published after the stream has drained.
int pq_append(vrag_pq_index* ix, const float* d_rows, int64_t n, hipStream_t st) {
  if (ix->size + n > ix->capacity) {
    set_error("pq index full: %lld + %lld > capacity %lld", (long long)ix->size, (long long)n, (long long)ix->capacity);
    return VRAG_ERR_CAPACITY;
  }
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(pq_encode(ix, d_rows, n, ix->codes.p + (size_t)ix->size * ix->stride, st));
  HIP_TRY(hipStreamSynchronize(st));   // ingest is not the hot path
  ix->size += n;
  return VRAG_OK;
}

// Workgroups per CU the scan's LDS leaves room for, and the row ranges of one launch over n_rows rows for nqs queries: enough
// ranges to fill the device once across the launch's queries, none shorter than one row per lane.
int pq_scan_wgs_per_cu(int m) { return std::max(1, std::min(PQ_WGS_PER_CU_MAX, PQ_LDS_BUDGET / pq_scan_lds(m))); }
int pq_scan_ranges(const vrag_pq_index* ix, long long n_rows, int nqs) {
  const long long fill = std::max<long long>(1, ((long long)ix->n_cu * pq_scan_wgs_per_cu(ix->m) + nqs - 1) / nqs);
  return (int)std::min<long long>(fill, (n_rows + PQ_THREADS - 1) / PQ_THREADS);
}

// The search over rows [0, n_rows) (with `filtered`: those whose bit is set in the staged bitmap ix->h_allow), under the lock.
int pq_search(vrag_pq_index* ix, const float* queries, int nq, int k, long long n_rows, bool filtered, float* scores, int64_t* ids,
              hipStream_t st) {
  const int dim = ix->dim, m = ix->m, kk = std::min<int>(k, KMAX), slice = std::min<int>(nq, PQ_SLICE);
  int wg_max = 0;
  for (int q0 = 0; q0 < nq; q0 += PQ_SLICE) wg_max = std::max(wg_max, pq_scan_ranges(ix, n_rows, std::min(PQ_SLICE, nq - q0)) * std::min(PQ_SLICE, nq - q0));
  HIP_TRY(ix->d_q.grow((size_t)nq * dim));
  HIP_TRY(ix->d_lut.grow((size_t)slice * m * PQ_KSUB));
  HIP_TRY(ix->d_cand.grow((size_t)wg_max * kk));
  HIP_TRY(ix->d_out.grow((size_t)nq * kk));
  const unsigned* d_allow = nullptr;
  if (filtered) {
    HIP_TRY(ix->d_allow.grow(ix->h_allow.size()));
    HIP_TRY(hipMemcpyAsync(ix->d_allow.p, ix->h_allow.data(), ix->h_allow.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    d_allow = ix->d_allow.p;
  }
  HIP_TRY((set_max_dynamic_lds<pq_scan_kernel>(pq_scan_lds(PQ_M_MAX))));
  HIP_TRY(hipMemcpyAsync(ix->d_q.p, queries, (size_t)nq * dim * sizeof(float), hipMemcpyHostToDevice, st));
  // one page of kk keys per query into d_out [nq][kk]
  return search_lists(nq, k, ix->d_bound, ix->d_out, st, [&](const u64* bound) -> int {
    for (int q0 = 0; q0 < nq; q0 += PQ_SLICE) {
      const int nqs = std::min(PQ_SLICE, nq - q0);
      const int n_wg = pq_scan_ranges(ix, n_rows, nqs);
      const long long per = (n_rows + n_wg - 1) / n_wg;
      hipLaunchKernelGGL(pq_lut_kernel, dim3((unsigned)m, (unsigned)nqs), dim3(PQ_KSUB), 0, st, ix->d_q.p + (size_t)q0 * dim, dim, m, ix->dsub,
                         ix->cb.p, ix->d_lut.p);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(pq_scan_kernel, dim3((unsigned)n_wg, (unsigned)nqs), dim3(PQ_THREADS), (size_t)(m * PQ_KSUB * sizeof(float) + PQ_WAVES * kk * sizeof(u64)),
                         st, ix->codes.p, n_rows, per, ix->stride, m, ix->d_lut.p, nqs, kk, d_allow, bound ? bound + q0 : nullptr, ix->d_cand.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(launch_topk_merge(ix->d_cand.p, n_wg, nqs, kk, ix->d_out.p + (size_t)q0 * kk, st));
    }
    return VRAG_OK;
  }, scores, ids);
}

}  // namespace

extern "C" {

int vrag_pq_index_create(int32_t dim, int32_t m, int64_t capacity, int32_t device, vrag_pq_index** out) {
  ARG_CHECK(out, "null argument");
  *out = nullptr;
  ARG_CHECK(dim >= 1 && dim <= PQ_DIM_MAX, "dim must be in [1, %d] for a pq index (got %d)", PQ_DIM_MAX, dim);
  ARG_CHECK(m >= 1 && m <= PQ_M_MAX, "m must be in [1, %d] (got %d)", PQ_M_MAX, m);
  ARG_CHECK(dim % m == 0, "m must divide dim (got dim %d, m %d)", dim, m);
  ARG_CHECK(dim / m <= PQ_DSUB_MAX, "a sub-vector holds at most %d components (got dim %d / m %d = %d)", PQ_DSUB_MAX, dim, m, dim / m);
  ARG_CHECK(capacity > 0 && capacity < 0xFFFFFFFFll, "capacity out of range");
  ARG_CHECK(device >= 0, "device must not be negative");
  DEVICE_CHECK(device);
  HIP_TRY(hipSetDevice(device));
  auto* ix = new vrag_pq_index();
  ix->dim = dim;
  ix->m = m;
  ix->dsub = dim / m;
  ix->stride = (m + 15) & ~15;
  ix->device = device;
  ix->capacity = capacity;
  hipError_t e = hipDeviceGetAttribute(&ix->n_cu, hipDeviceAttributeMultiprocessorCount, device);
  if (e == hipSuccess) e = ix->codes.grow((size_t)capacity * ix->stride);
  if (e == hipSuccess) e = hipMemset(ix->codes.p, 0, (size_t)capacity * ix->stride);   // the pad bytes stay zero from here on
  if (e == hipSuccess) e = ix->cb.grow(pq_cb_floats(ix));
  if (e == hipSuccess) e = ix->half.grow((size_t)m * PQ_KSUB);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking);
  ix->stage_rows = std::max<size_t>(1, std::min<size_t>((size_t)capacity, ((size_t)64 << 20) / ((size_t)dim * 4)));
  if (e == hipSuccess) e = ix->stage.grow(ix->stage_rows * dim);
  if (e != hipSuccess || ix->n_cu < 1) {
    set_error("pq index allocation failed: %s", hipGetErrorString(e));
    vrag_pq_index_destroy(ix);
    return VRAG_ERR_HIP;
  }
  *out = ix;
  return VRAG_OK;
}

void vrag_pq_index_destroy(vrag_pq_index* ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->device);
  (void)hipDeviceSynchronize();
  if (ix->stream) (void)hipStreamDestroy(ix->stream);
  delete ix;   // the device arrays free themselves
}

int64_t vrag_pq_index_size(vrag_pq_index* ix) {
  if (!ix) return -1;
  std::lock_guard<std::mutex> lk(ix->mu);
  return ix->size;
}

int vrag_pq_index_set_codebooks(vrag_pq_index* ix, const float* cb) {
  ARG_CHECK(ix && cb, "null argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  ARG_CHECK(ix->size == 0, "the codebooks are frozen once the index holds rows (size %lld)", (long long)ix->size);
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(hipMemcpyAsync(ix->cb.p, cb, pq_cb_floats(ix) * sizeof(float), hipMemcpyHostToDevice, ix->stream));
  HIP_TRY(pq_half(ix, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  ix->has_codebooks = true;
  return VRAG_OK;
}

int vrag_pq_index_read_codebooks(vrag_pq_index* ix, float* cb) {
  ARG_CHECK(ix && cb, "null argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  ARG_CHECK(ix->has_codebooks, "the index has no codebooks yet (set_codebooks or train)");
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(hipMemcpy(cb, ix->cb.p, pq_cb_floats(ix) * sizeof(float), hipMemcpyDeviceToHost));
  return VRAG_OK;
}

int vrag_pq_index_train(vrag_pq_index* ix, const float* rows, int64_t n, int32_t iters) {
  ARG_CHECK(ix && rows && n > 0, "bad arguments");
  ARG_CHECK(iters >= 0 && iters <= PQ_TRAIN_ITERS_MAX, "iters must be in [0, %d] (got %d)", PQ_TRAIN_ITERS_MAX, iters);
  ARG_CHECK(n < 0xFFFFFFFFll, "too many sample rows");
  std::lock_guard<std::mutex> lk(ix->mu);
  ARG_CHECK(ix->size == 0, "the codebooks are frozen once the index holds rows (size %lld)", (long long)ix->size);
  HIP_TRY(hipSetDevice(ix->device));
  const int dim = ix->dim, m = ix->m, dsub = ix->dsub;
  hipStream_t st = ix->stream;
  // the initial centroid c of every sub-space: sample row c * n / 256
  std::vector<float> init(pq_cb_floats(ix));
  for (int j = 0; j < m; ++j)
    for (int c = 0; c < PQ_KSUB; ++c)
      std::memcpy(&init[((size_t)j * PQ_KSUB + c) * dsub], rows + (size_t)((int64_t)c * n / PQ_KSUB) * dim + (size_t)j * dsub, (size_t)dsub * sizeof(float));
  HIP_TRY(ix->train_rows.grow((size_t)n * dim));
  HIP_TRY(ix->train_codes.grow((size_t)n * ix->stride));
  ix->has_codebooks = false;   // until the last round has run
  int rc = VRAG_OK;
  auto run = [&]() -> int {
    HIP_TRY(hipMemcpyAsync(ix->train_rows.p, rows, (size_t)n * dim * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ix->cb.p, init.data(), init.size() * sizeof(float), hipMemcpyHostToDevice, st));
    for (int it = 0; it < iters; ++it) {
      HIP_TRY(pq_half(ix, st));
      HIP_TRY(pq_encode(ix, ix->train_rows.p, n, ix->train_codes.p, st));
      hipLaunchKernelGGL(pq_mean_kernel, dim3(PQ_KSUB / 4, (unsigned)m), dim3(256), 0, st, ix->train_rows.p, (long long)n, dim, dsub, ix->train_codes.p,
                         ix->stride, ix->cb.p);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(pq_half(ix, st));
    HIP_TRY(hipStreamSynchronize(st));
    return VRAG_OK;
  };
  rc = run();
  if (rc != VRAG_OK) (void)hipStreamSynchronize(st);   // `init` and `rows` stay until the stream has passed them
  ix->train_rows = DevArray<float>();
  ix->train_codes = DevArray<unsigned char>();
  if (rc == VRAG_OK) ix->has_codebooks = true;
  return rc;
}

int vrag_pq_index_add_device(vrag_pq_index* ix, const float* rows, int64_t n, void* stream) {
  ARG_CHECK(ix && rows && n > 0, "bad arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  ARG_CHECK(ix->has_codebooks, "the index has no codebooks yet (set_codebooks or train)");
  return pq_append(ix, rows, n, reinterpret_cast<hipStream_t>(stream));
}

int vrag_pq_index_add(vrag_pq_index* ix, const float* rows, int64_t n) {
  ARG_CHECK(ix && rows && n > 0, "bad arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  ARG_CHECK(ix->has_codebooks, "the index has no codebooks yet (set_codebooks or train)");
  if (ix->size + n > ix->capacity) {   // all or nothing: checked before the first slab
    set_error("pq index full: %lld + %lld > capacity %lld", (long long)ix->size, (long long)n, (long long)ix->capacity);
    return VRAG_ERR_CAPACITY;
  }
  HIP_TRY(hipSetDevice(ix->device));
  for (int64_t r0 = 0; r0 < n; r0 += (int64_t)ix->stage_rows) {   // slabs through the staging buffer, each appended by the device form
    const int64_t nr = std::min<int64_t>((int64_t)ix->stage_rows, n - r0);
    HIP_TRY(hipMemcpyAsync(ix->stage.p, rows + (size_t)r0 * ix->dim, (size_t)nr * ix->dim * sizeof(float), hipMemcpyHostToDevice, ix->stream));
    const int rc = pq_append(ix, ix->stage.p, nr, ix->stream);
    if (rc != VRAG_OK) return rc;
  }
  return VRAG_OK;
}

int vrag_pq_index_read(vrag_pq_index* ix, int64_t first_row, int64_t n, uint8_t* codes) {
  ARG_CHECK(ix && codes && first_row >= 0 && n >= 0, "bad arguments");
  std::lock_guard<std::mutex> lk(ix->mu);
  ARG_CHECK(first_row + n <= ix->size, "rows [%lld, %lld) are not all in the index (size %lld)", (long long)first_row,
            (long long)(first_row + n), (long long)ix->size);
  if (n == 0) return VRAG_OK;
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(hipMemcpy2D(codes, (size_t)ix->m, ix->codes.p + (size_t)first_row * ix->stride, (size_t)ix->stride, (size_t)ix->m, (size_t)n,
                      hipMemcpyDeviceToHost));
  return VRAG_OK;
}

// Drops the rows whose bit is cleared, in place (csrc/compact.h): the codes at their padded stride (a multiple of 16 bytes); the
// codebooks are untouched.  Every search of this handle returns host lists and has drained its stream before it let go of the lock.
int vrag_pq_index_compact(vrag_pq_index* ix, const uint32_t* keep_words, int64_t n_keep, int64_t* new_size) {
  ARG_CHECK(ix && new_size, "null argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  return compact_arrays(ix->compact, ix->device, ix->stream, keep_words, n_keep, &ix->size, new_size, {{ix->codes.p, (size_t)ix->stride}});
}

int vrag_pq_index_search(vrag_pq_index* ix, const float* queries, int32_t nq, int32_t k, float* scores, int64_t* ids, void* stream) {
  ARG_CHECK(ix && queries && scores && ids && nq > 0, "bad arguments");
  ARG_CHECK(k >= 1 && k <= 1024, "k must be in [1, 1024] (got %d)", k);
  std::lock_guard<std::mutex> lk(ix->mu);
  ARG_CHECK(ix->has_codebooks, "the index has no codebooks yet (set_codebooks or train)");
  if (ix->size == 0) {
    fill_no_hits(scores, ids, (size_t)nq * k);
    return VRAG_OK;
  }
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : ix->stream;
  return pq_search(ix, queries, nq, k, ix->size, false, scores, ids, st);
}

int vrag_pq_index_search_filtered(vrag_pq_index* ix, const float* queries, int32_t nq, int32_t k, const uint32_t* allow, int64_t n_allow,
                                  float* scores, int64_t* ids, void* stream) {
  ARG_CHECK(ix && queries && scores && ids && nq > 0, "bad arguments");
  ARG_CHECK(k >= 1 && k <= 1024, "k must be in [1, 1024] (got %d)", k);
  ARG_CHECK(n_allow >= 0 && (allow || n_allow == 0), "bad row bitmap (null words or a negative length)");
  std::lock_guard<std::mutex> lk(ix->mu);
  ARG_CHECK(ix->has_codebooks, "the index has no codebooks yet (set_codebooks or train)");
  const long long n_rows = std::min<long long>(n_allow, ix->size);   // rows appended after the mask was built are not in it
  const long long n_pass = n_rows > 0 ? stage_bitmap(ix->h_allow, allow, n_rows, 1) : 0;
  if (n_pass == 0) {   // nothing passes: no launch
    fill_no_hits(scores, ids, (size_t)nq * k);
    return VRAG_OK;
  }
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : ix->stream;
  return pq_search(ix, queries, nq, k, n_rows, true, scores, ids, st);
}

}  // extern "C"
