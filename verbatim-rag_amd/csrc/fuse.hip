// Weighted reciprocal-rank fusion of a batch of hybrid queries (gfx950): vrag_rrf_fuse, include/vrag_amd.h.
//
// The array form of the reference's per-query merge (vector_stores/hybrid_search.py:73-129; numpy statement: rrf_merge_rows
// in vector_stores.py), held to its float64 bits.  The caller lays the methods' ranked lists of a query side by side and
// supplies gains[p], the float64 a candidate at position p contributes, so the kernels see neither weights nor rrf_k nor
// method boundaries: they only ADD gains, in ascending position -- the reference's accumulation order (methods in insertion
// order, ranks ascending) -- and subtract the sum from 1.0 once.  No multiply, no divide: nothing for -ffp-contract to fuse.
// Queries are independent: no grid-wide synchronisation, no cross-workgroup atomics, every loop bounded by l_total.
//
// Two regimes:
//   l_total <= 64   one wave per query, one candidate per lane, FUSE_WAVES queries per workgroup (the store's normal case:
//                   2-3 methods x 2 * top_k with top_k 5-10).  Everything stays in registers.
//   l_total <= 4096 one workgroup per query: (row << 12 | position) keys sorted in LDS make the occurrences of a row
//                   contiguous with positions ascending; the first of each group adds the group's gains in that order; a second
//                   sort by (score descending, first position ascending) puts the answer in front.
#include "../../include/vrag_amd.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "host_util.h"

namespace vrag {

using u64 = unsigned long long;

constexpr int FUSE_MAX_L = 4096;     // positions fit the 12-bit field of a sort key
constexpr int FUSE_WAVES = 4;        // queries per workgroup in the one-wave regime
constexpr u64 FUSE_NO_KEY = ~0ull;   // sorts behind every (row << 12 | position) with row < 2^32

// l_total <= 64.  Lane i owns position i.  It walks the positions in order and adds gains[j] where the row at j is its own: the
// sequential sum (0.0 + g == g exactly, so starting from zero equals starting from the first gain).  It is its row's first
// occurrence when no j < i matched; its rank is the number of first occurrences that beat it on (score desc, position asc).
__global__ void __launch_bounds__(64 * FUSE_WAVES)
rrf_fuse_wave_kernel(const long long* __restrict__ rows, const double* __restrict__ gains, int nq, int l_total, int top_k,
                     long long* __restrict__ out_rows, double* __restrict__ out_dist) {
  const int lane = threadIdx.x & 63;
  const int q = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * FUSE_WAVES + (threadIdx.x >> 6)));
  if (q >= nq) return;   // the whole wave leaves
  const long long* qr = rows + (size_t)q * l_total;
  const long long mine = lane < l_total ? qr[lane] : -1;
  const bool live = mine >= 0;
  double score = 0.0;
  bool first = live;
  for (int j = 0; j < l_total; ++j) {
    if (live && qr[j] == mine) {   // qr[j]: one address for the wave
      score += gains[j];
      if (j < lane) first = false;
    }
  }
  const u64 heads = __ballot(first);
  int rank = 0;
  for (int j = 0; j < l_total; ++j) {
    const double sj = __shfl(score, j);
    if (((heads >> j) & 1ull) && (sj > score || (sj == score && j < lane))) ++rank;
  }
  long long* orow = out_rows + (size_t)q * top_k;
  double* odist = out_dist + (size_t)q * top_k;
  if (first && rank < top_k) {
    orow[rank] = mine;
    odist[rank] = 1.0 - score;
  }
  const int n_heads = __popcll(heads);
  if (lane >= n_heads && lane < top_k) {   // fewer distinct rows than top_k: the tail (top_k <= l_total <= 64 lanes)
    orow[lane] = -1;
    odist[lane] = 0.0;
  }
}

// Index of the lower element of compare-exchange pair t at distance j (j a power of two); its partner is that index | j.
__device__ __forceinline__ int bitonic_lower(int t, int j) { return ((t & ~(j - 1)) << 1) | (t & (j - 1)); }

// Whether candidate (sa, ka) comes before (sb, kb) in the answer: score descending, then position ascending.  Entries that are
// not the first of their row carry score -1.0 and so follow every first occurrence (scores are >= 0).
__device__ __forceinline__ bool fuse_before(double sa, u64 ka, double sb, u64 kb) {
  return sa > sb || (sa == sb && (ka & (FUSE_MAX_L - 1)) < (kb & (FUSE_MAX_L - 1)));
}

// 64 < l_total <= 4096.  One workgroup per query, n = l_total rounded up to a power of two, dynamic LDS = n keys + n scores.
__global__ void __launch_bounds__(1024)
rrf_fuse_block_kernel(const long long* __restrict__ rows, const double* __restrict__ gains, int l_total, int n, int top_k,
                      long long* __restrict__ out_rows, double* __restrict__ out_dist) {
  extern __shared__ u64 fuse_lds[];
  u64* key = fuse_lds;
  double* score = reinterpret_cast<double*>(fuse_lds + n);
  const int tid = threadIdx.x, nt = blockDim.x;
  const long long* qr = rows + (size_t)blockIdx.x * l_total;
  for (int i = tid; i < n; i += nt) {
    const long long r = i < l_total ? qr[i] : -1;
    key[i] = r >= 0 ? ((u64)r << 12 | (u64)i) : FUSE_NO_KEY;
  }
  __syncthreads();
  for (int k = 2; k <= n; k <<= 1)          // ascending bitonic sort of the keys
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < n / 2; t += nt) {
        const int i = bitonic_lower(t, j), p = i | j;
        const bool up = (i & k) == 0;
        const u64 a = key[i], b = key[p];
        if ((a > b) == up && a != b) key[i] = b, key[p] = a;
      }
      __syncthreads();
    }
  // the first key of a row's group adds the group's gains, positions ascending
  for (int i = tid; i < n; i += nt) {
    const u64 k = key[i];
    const u64 row = k >> 12;
    double s = -1.0;
    if (k != FUSE_NO_KEY && (i == 0 || (key[i - 1] >> 12) != row)) {
      s = 0.0;
      for (int m = i; m < n && (key[m] >> 12) == row; ++m) s += gains[key[m] & (FUSE_MAX_L - 1)];
    }
    score[i] = s;
  }
  __syncthreads();
  for (int k = 2; k <= n; k <<= 1)          // (score, key) pairs into answer order
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < n / 2; t += nt) {
        const int i = bitonic_lower(t, j), p = i | j;
        const bool up = (i & k) == 0;
        const u64 ka = key[i], kb = key[p];
        const double sa = score[i], sb = score[p];
        if (up ? fuse_before(sb, kb, sa, ka) : fuse_before(sa, ka, sb, kb)) {
          key[i] = kb, key[p] = ka;
          score[i] = sb, score[p] = sa;
        }
      }
      __syncthreads();
    }
  long long* orow = out_rows + (size_t)blockIdx.x * top_k;
  double* odist = out_dist + (size_t)blockIdx.x * top_k;
  for (int i = tid; i < top_k; i += nt) {   // top_k <= l_total <= n
    const double s = score[i];
    orow[i] = s >= 0.0 ? (long long)(key[i] >> 12) : -1;
    odist[i] = s >= 0.0 ? 1.0 - s : 0.0;
  }
}

static hipError_t launch_rrf_fuse(const long long* rows, const double* gains, int nq, int l_total, int top_k, long long* out_rows,
                                  double* out_dist, hipStream_t st) {
  if (l_total <= 64) {
    hipLaunchKernelGGL(rrf_fuse_wave_kernel, dim3((unsigned)((nq + FUSE_WAVES - 1) / FUSE_WAVES)), dim3(64 * FUSE_WAVES), 0, st, rows,
                       gains, nq, l_total, top_k, out_rows, out_dist);
  } else {
    int n = 128;
    while (n < l_total) n <<= 1;
    // at most 4096 * (8 + 8) bytes = 64 KB: inside the limit a kernel has without raising it
    hipLaunchKernelGGL(rrf_fuse_block_kernel, dim3((unsigned)nq), dim3(std::min(1024, n / 2)), (size_t)n * 16, st, rows, gains, l_total,
                       n, top_k, out_rows, out_dist);
  }
  return hipGetLastError();
}

}  // namespace vrag

using namespace vrag;

extern "C" int vrag_rrf_fuse(const int64_t* rows, const double* gains, int32_t nq, int32_t l_total, int32_t top_k, int64_t* out_rows,
                             double* out_dist, int32_t on_device, int32_t device, void* stream) {
  ARG_CHECK(rows && gains && out_rows && out_dist, "vrag_rrf_fuse: null argument");
  ARG_CHECK(nq >= 1 && l_total >= 1 && l_total <= FUSE_MAX_L, "vrag_rrf_fuse: bad list geometry (nq >= 1, 1 <= l_total <= %d; got nq %d, l_total %d)",
            FUSE_MAX_L, nq, l_total);
  ARG_CHECK(top_k >= 1 && top_k <= l_total, "vrag_rrf_fuse: top_k must be in [1, l_total = %d] (got %d)", l_total, top_k);
  ARG_CHECK(device >= 0, "vrag_rrf_fuse: negative device");
  DEVICE_CHECK(device);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t n_in = (size_t)nq * l_total, n_out = (size_t)nq * top_k;
  if (on_device) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_rrf_fuse(reinterpret_cast<const long long*>(rows), gains, nq, l_total, top_k, reinterpret_cast<long long*>(out_rows),
                            out_dist, st));
    return VRAG_OK;
  }
  for (size_t i = 0; i < n_in; ++i)
    ARG_CHECK(rows[i] <= 0xFFFFFFFFll, "vrag_rrf_fuse: row id %lld does not fit the 32-bit key field", (long long)rows[i]);
  for (int p = 0; p < l_total; ++p)
    ARG_CHECK(std::isfinite(gains[p]) && gains[p] >= 0.0, "vrag_rrf_fuse: gain %d is negative or not finite (%g)", p, gains[p]);
  HIP_TRY(hipSetDevice(device));
  DevBuf scratch;   // this call's scratch, freed on every way out: one allocation of 8-byte elements, carved into the four arrays
  HIP_TRY(scratch.alloc((n_in + (size_t)l_total + 2 * n_out) * 8));
  long long* d_rows = scratch.as<long long>();
  double* d_gains = reinterpret_cast<double*>(d_rows + n_in);
  long long* d_orows = reinterpret_cast<long long*>(d_gains + l_total);
  double* d_odist = reinterpret_cast<double*>(d_orows + n_out);
  hipError_t e = hipMemcpyAsync(d_rows, rows, n_in * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_gains, gains, (size_t)l_total * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_rrf_fuse(d_rows, d_gains, nq, l_total, top_k, d_orows, d_odist, st);
  if (e == hipSuccess) e = hipMemcpyAsync(out_rows, d_orows, n_out * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(out_dist, d_odist, n_out * 8, hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);   // also after a failure: nothing may still use the scratch when it is freed
  HIP_TRY(e);
  HIP_TRY(es);
  return VRAG_OK;
}
