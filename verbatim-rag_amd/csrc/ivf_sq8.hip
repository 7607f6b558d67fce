// The scan stage of an IVF search over SQ8 rows (index_type "IVF_SQ8"): csrc/ivf.hip's probe, invert and merge stages around a
// scan that scores int8 rows against int8 queries with the SQ8 rule (include/vrag_amd.h, "SQ8 dense rows"; csrc/sq8_kernels.h).
//
// The MFMA form: one v_mfma_i32_16x16x64_i8 accumulator is exactly the 16 rows x 16 queries of a scan step, so a work item with
// one query and one with sixteen take the same instructions; the int32 dot is the same in any order, and the score is sq8_score
// of it -- with every list probed the result is vrag_sq8_index_search's bit for bit.  A v_dot4_i32_i8 form (sq8_scan_kernel's) was
// not built; which of the two is faster for one or two queries per group is not measured.
//
// Work items are ivf_scan_kernel's: one list for one group of up to IVF_QG queries, blockIdx.y one range of the list's 16-row
// groups.  Per item the group's query codes are staged ONCE into an LDS image [IVF_QG][pitch] (pitch = stride rounded up to the
// 64-byte k-step + 16 bytes of bank spread; the bytes behind the stride are zero), 16 x 4 112 bytes at dim 4 096.  Each of the four
// waves then owns one 16-row group per workgroup step (64 rows a step): lane l takes row  list_rows[base + (l & 15)]  straight from
// HBM, 16 bytes at 16 (l >> 4) of each k-step, and query l & 15 from the image -- sq8_tile_kernel's operand maps -- with no barrier
// inside the k loop.  The stride is a multiple of 16, not of 64: in the last k-step the lanes whose 16 bytes lie behind the stride
// load nothing and contribute zero.  D register g of lane l is row slot 4 (l >> 4) + g, query l & 15; slots behind the list's end
// and columns behind the group's queries give no key.  The step's 64 x 16 keys go through LDS; wave w inserts for queries
// 4 w .. 4 w + 3 (the keys above the list's last key, one lane at a time).
#include "../../include/vrag_amd.h"

#include "common.h"
#include "host_util.h"
#include "ivf_kernels.h"
#include "sq8_kernels.h"
#include "topk_kernels.h"

namespace vrag {
namespace {

constexpr int IVF_SQ8_DIM_MAX = 4096;       // vrag_sq8_index_create
constexpr int IVF_SQ8_STEP_ROWS = 64;       // rows of a workgroup step: one 16-row group per wave
constexpr int IVF_SQ8_KEY_PITCH = IVF_SQ8_STEP_ROWS + 1;   // u64 per query of the step's key image (+ 1: bank spread)

__host__ __device__ constexpr int ivf_sq8_pitch(int stride) { return ((stride + 63) & ~63) + 16; }

__global__ __launch_bounds__(256) void ivf_sq8_scan_kernel(const signed char* __restrict__ codes, const float* __restrict__ scales,
                                                            int stride, const unsigned* __restrict__ list_off,
                                                            const unsigned* __restrict__ list_rows, const signed char* __restrict__ qcodes,
                                                            const float* __restrict__ qscales, int nq, int k,
                                                            const unsigned* __restrict__ n_items_p, const unsigned* __restrict__ item_list,
                                                            const unsigned* __restrict__ item_n, const unsigned* __restrict__ item_pair,
                                                            u64* __restrict__ cand) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  signed char* sB = reinterpret_cast<signed char*>(smem);   // [IVF_QG][pitch]
  __shared__ u64 lists[IVF_QG][KMAX];
  __shared__ u64 skey[IVF_QG][IVF_SQ8_KEY_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int pitch = ivf_sq8_pitch(stride), pieces = (pitch - 16) / 16;
  const int full = stride & ~63;   // bytes of a row that whole k-steps cover
  const unsigned n_items = *n_items_p;
  for (unsigned item = blockIdx.x; item < n_items; item += gridDim.x) {
    const unsigned l = item_list[item];
    const int nqt = (int)item_n[item];
    const unsigned* pair = item_pair + (size_t)item * IVF_QG;
    const unsigned begin = list_off[l], end = list_off[l + 1];
    const unsigned n_groups = (end - begin + IVF_ROWS - 1) / IVF_ROWS;
    const unsigned g_lo = (unsigned)((unsigned long long)n_groups * blockIdx.y / gridDim.y);
    const unsigned g_hi = (unsigned)((unsigned long long)n_groups * (blockIdx.y + 1) / gridDim.y);
    __syncthreads();   // the previous item's lists have been written out; its last reads of the image are done
    for (int p = tid; p < IVF_QG * pieces; p += 256) {
      const int col = p / pieces, o = (p % pieces) * 16;
      i32x4 v = {0, 0, 0, 0};
      if (col < nqt && o < stride) v = *reinterpret_cast<const i32x4*>(qcodes + (size_t)(pair[col] >> IVF_RANK_BITS) * stride + o);
      *reinterpret_cast<i32x4*>(sB + col * pitch + o) = v;
    }
    for (int i = tid; i < IVF_QG * k; i += 256) lists[i / k][i % k] = 0ull;
    const float qs = l15 < nqt ? qscales[pair[l15] >> IVF_RANK_BITS] : 0.f;
    __syncthreads();
    for (unsigned g0 = g_lo; g0 < g_hi; g0 += 4) {
      const unsigned g = g0 + wave;
      u64 keys[4] = {0ull, 0ull, 0ull, 0ull};
      if (g < g_hi) {   // uniform in the wave
        const unsigned base = begin + g * IVF_ROWS;
        const unsigned rid = list_rows[min(base + l15, end - 1u)];   // slots behind the list re-read its last row; their keys are dropped
        const signed char* arow = codes + (size_t)rid * stride + 16 * l4;
        const signed char* brow = sB + l15 * pitch + 16 * l4;
        i32x4 acc = {0, 0, 0, 0};
#pragma unroll 4
        for (int ks = 0; ks < full; ks += 64) {
          const i32x4 a = *reinterpret_cast<const i32x4*>(arow + ks);
          const i32x4 b = *reinterpret_cast<const i32x4*>(brow + ks);
          acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc, 0, 0, 0);
        }
        if (full < stride) {   // the partial k-step: bytes behind the stride belong to the next row (or to nobody)
          i32x4 a = {0, 0, 0, 0};
          if (full + 16 * l4 < stride) a = *reinterpret_cast<const i32x4*>(arow + full);
          const i32x4 b = *reinterpret_cast<const i32x4*>(brow + full);
          acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int slot = 4 * l4 + j;
          const unsigned row = (unsigned)__shfl((int)rid, slot, 64);   // lanes 0 .. 15 hold the rows of slots 0 .. 15
          const float sr = scales[row];
          if (base + slot < end && l15 < nqt) keys[j] = make_key_below(sq8_score(acc[j], qs, sr), row, ~0ull);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) skey[l15][wave * IVF_ROWS + 4 * l4 + j] = keys[j];
      __syncthreads();
      for (int j = 0; j < 4; ++j) {
        const int q = wave * 4 + j;
        if (q >= nqt) break;   // uniform
        u64* list = lists[q];
        const u64 key = skey[q][lane];
        unsigned long long want = __ballot(key > list[k - 1]);   // this wave alone writes the list: the last key is current
        while (want) {
          const int b = __builtin_ctzll(want);
          want &= want - 1;
          if (lane == b) insert_key(list, k, key);
          __builtin_amdgcn_wave_barrier();
        }
      }
      __syncthreads();   // the key image is free for the next step
    }
    for (int i = tid; i < nqt * k; i += 256) {
      const unsigned pr = pair[i / k];
      const size_t slot = ((size_t)(pr & ((1u << IVF_RANK_BITS) - 1u)) * gridDim.y + blockIdx.y) * nq + (pr >> IVF_RANK_BITS);
      cand[slot * k + i % k] = lists[i / k][i % k];
    }
  }
}

}  // namespace

hipError_t launch_ivf_sq8_scan(dim3 grid, const signed char* codes, const float* scales, int stride, const unsigned* list_off,
                               const unsigned* list_rows, const signed char* qcodes, const float* qscales, int nq, int k,
                               const unsigned* n_items, const unsigned* item_list, const unsigned* item_n, const unsigned* item_pair,
                               u64* cand, hipStream_t st) {
  const hipError_t e = set_max_dynamic_lds<ivf_sq8_scan_kernel>(IVF_QG * ivf_sq8_pitch(IVF_SQ8_DIM_MAX));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ivf_sq8_scan_kernel, grid, dim3(256), (size_t)IVF_QG * ivf_sq8_pitch(stride), st, codes, scales, stride, list_off,
                     list_rows, qcodes, qscales, nq, k, n_items, item_list, item_n, item_pair, cand);
  return hipGetLastError();
}

}  // namespace vrag
