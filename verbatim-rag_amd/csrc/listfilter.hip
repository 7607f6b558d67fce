// List filter: membership in list-valued metadata (`json_contains`, store_filter.py) for the row filter of csrc/rowfilter.hip + C ABI
// (include/vrag_amd.h, vrag_row_filter_append_lists / _list_rows; vrag_row_filter_eval_lists lives beside the other eval entry points).
//
// What it adds: a column's LIST PART -- the rows whose value is a list as CSR: list_off[r] .. list_off[r + 1] into elem_kinds /
// elem_payload, one (kind, payload) per element in the encoding of the scalar rows, strings through the column's one dictionary.
// 8 bytes per row + 9 bytes per element of HBM.  A row without a list has an empty range.
//
// list_filter_eval_kernel: row_filter_eval_kernel's frame (one lane per row, one wave per 64 rows, the program a by-value argument,
// the stack the bits of one register, one ballot per wave) with one more op: RF_LIST_ANY + leaf pushes the OR, over the row's
// elements, of what the leaf answers for the element's (kind, payload) -- the leaf's per-kind answers exactly as a scalar row gets
// them, so a `==` leaf states membership.  An empty range pushes 0.
//   loop      bounded by the row's element count; a lane leaves it at its first matching element.  Lanes of a wave walk lists of
//             different lengths, so the wave takes as long as its longest list: a row with a very long list makes one lane walk
//             alone -- the trade csrc/strmatch.hip states for a megabyte string.  No wave-per-row variant: the lists this is for
//             (authors, tags) hold a handful of elements
//   memory    consecutive lanes read consecutive offsets (coalesced) and, at step e of the walk, elements list_off[r] + e: for short
//             lists neighbouring lanes stay within a few lines of each other
//   registers no indexed private array, no scratch, no atomics, no LDS
// A program without a list op never comes here (csrc/rowfilter.hip, eval_program): row_filter_eval_kernel is untouched.
#include "../../include/vrag_amd.h"

#include <algorithm>
#include <vector>

#include "rowfilter.h"

namespace vrag {
namespace {

// What leaf `lf` answers for one stored (kind, payload): the four cases of row_filter_eval_kernel.
__device__ __forceinline__ bool leaf_answer(const LeafDev& lf, unsigned kind, u64 pay, const unsigned* __restrict__ tables) {
  if (kind == VRAG_FILTER_KIND_NUMBER) return num_answer(lf.num_op, __longlong_as_double((long long)pay), lf.bound);
  if (kind == VRAG_FILTER_KIND_STRING) {
    if (lf.str_mode == VRAG_FILTER_STR_TABLE && pay < (u64)lf.table_codes)
      return (tables[(size_t)lf.table_off + (size_t)(pay >> 5)] >> (unsigned)(pay & 31ull)) & 1u;
    return lf.str_mode == VRAG_FILTER_STR_ALWAYS;
  }
  if (kind == VRAG_FILTER_KIND_BOOL) return (lf.bits >> (1u + (unsigned)(pay & 1ull))) & 1u;
  return lf.bits & 1u;
}

__global__ __launch_bounds__(64 * RF_WAVES) void list_filter_eval_kernel(const EvalArgs a, const ListArgs l,
                                                                          const unsigned* __restrict__ tables, long long n_rows,
                                                                          long long n_groups, unsigned* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * RF_WAVES;
  for (long long g = (long long)blockIdx.x * RF_WAVES + (threadIdx.x >> 6); g < n_groups; g += stride) {
    const long long r = g * 64 + lane;
    const bool in = r < n_rows;
    unsigned stk = 0u;
    for (int i = 0; i < a.n_ops; ++i) {
      const unsigned op = (a.ops[i >> 2] >> ((i & 3) * 8)) & 0xffu;
      if (op < RF_AND) {
        const LeafDev& lf = a.leaves[op];
        bool bit = false;
        if (in) bit = leaf_answer(lf, a.kinds[lf.slot][r], a.payload[lf.slot][r], tables);
        stk = (stk << 1) | (bit ? 1u : 0u);
      } else if (op >= RF_LIST_ANY) {
        const LeafDev& lf = a.leaves[op - RF_LIST_ANY];
        bool bit = false;
        if (in) {
          const long long* __restrict__ off = l.list_off[lf.slot];
          const unsigned char* __restrict__ ek = l.elem_kinds[lf.slot];
          const u64* __restrict__ ep = l.elem_payload[lf.slot];
          const long long end = off[r + 1];
          for (long long e = off[r]; e < end && !bit; ++e) bit = leaf_answer(lf, ek[e], ep[e], tables);
        }
        stk = (stk << 1) | (bit ? 1u : 0u);
      } else if (op == RF_AND) {
        stk = (stk >> 1) & ((stk & 1u) | ~1u);
      } else if (op == RF_OR) {
        stk = (stk >> 1) | (stk & 1u);
      } else {
        stk ^= 1u;
      }
    }
    const u64 m = __ballot(in && (stk & 1u) != 0u);   // every lane is here again: the element loops are per lane, the op loop is uniform
    if (lane < 2) out[2 * g + lane] = lane ? (unsigned)(m >> 32) : (unsigned)(m & 0xffffffffull);
  }
}

}  // namespace

hipError_t list_eval_launch(const EvalArgs& a, const ListArgs& l, const unsigned* d_tables, long long n_rows, unsigned* d_out,
                            hipStream_t st) {
  const long long n_groups = (n_rows + 63) / 64;
  const unsigned blocks = (unsigned)std::min<long long>((n_groups + RF_WAVES - 1) / RF_WAVES, RF_MAX_BLOCKS);
  hipLaunchKernelGGL(list_filter_eval_kernel, dim3(blocks), dim3(64 * RF_WAVES), 0, st, a, l, d_tables, n_rows, n_groups, d_out);
  return hipGetLastError();
}

}  // namespace vrag

using namespace vrag;

extern "C" {

int vrag_row_filter_append_lists(vrag_row_filter* f, int32_t col, const int64_t* elem_off, const uint8_t* elem_kinds,
                                 const uint64_t* elem_payload, int64_t n) {
  ARG_CHECK(f, "null argument");
  ARG_CHECK(n >= 0 && (n == 0 || elem_off), "vrag_row_filter_append_lists: need n >= 0 and n + 1 offsets");
  std::lock_guard<std::mutex> lk(f->mu);
  ARG_CHECK(col >= 0 && col < (int)f->cols.size(), "vrag_row_filter_append_lists: no column %d (the filter holds %d)", col,
            (int)f->cols.size());
  if (n == 0) return VRAG_OK;
  ARG_CHECK(elem_off[0] == 0, "vrag_row_filter_append_lists: elem_off[0] = %lld (offsets start at 0)", (long long)elem_off[0]);
  for (int64_t i = 0; i < n; ++i)
    ARG_CHECK(elem_off[i] <= elem_off[i + 1], "vrag_row_filter_append_lists: elem_off[%lld] = %lld decreases to %lld", (long long)i,
              (long long)elem_off[i], (long long)elem_off[i + 1]);
  const int64_t m = elem_off[n];
  ARG_CHECK(m == 0 || (elem_kinds && elem_payload), "vrag_row_filter_append_lists: %lld elements but a null element array", (long long)m);
  for (int64_t e = 0; e < m; ++e)
    ARG_CHECK(elem_kinds[e] <= VRAG_FILTER_KIND_BOOL, "vrag_row_filter_append_lists: elem_kinds[%lld] = %d is no VRAG_FILTER_KIND_*",
              (long long)e, (int)elem_kinds[e]);
  FilterColumn& c = f->cols[col];
  HIP_TRY(hipSetDevice(f->device));
  const size_t need_off = (size_t)c.n_list_rows + (size_t)n + 1, need_el = (size_t)c.n_elems + (size_t)m;
  if (need_off > c.list_off.n) {   // geometric growth; what is held so far moves into the new array
    DevArray<long long> grown;
    HIP_TRY(grown.grow(std::max<size_t>(need_off, std::max<size_t>(2 * c.list_off.n, 257))));
    if (c.n_list_rows) {
      HIP_TRY(hipMemcpyAsync(grown.p, c.list_off.p, ((size_t)c.n_list_rows + 1) * sizeof(long long), hipMemcpyDeviceToDevice, f->stream));
      HIP_TRY(hipStreamSynchronize(f->stream));   // the old array is freed by the assignment below
    }
    c.list_off = std::move(grown);
  }
  if (need_el > c.elem_kinds.n) {
    const size_t cap = std::max<size_t>(need_el, std::max<size_t>(2 * c.elem_kinds.n, 256));
    DevArray<unsigned char> nk;
    DevArray<u64> np;
    HIP_TRY(nk.grow(cap));
    HIP_TRY(np.grow(cap));
    if (c.n_elems) {
      HIP_TRY(hipMemcpyAsync(nk.p, c.elem_kinds.p, (size_t)c.n_elems, hipMemcpyDeviceToDevice, f->stream));
      HIP_TRY(hipMemcpyAsync(np.p, c.elem_payload.p, (size_t)c.n_elems * sizeof(u64), hipMemcpyDeviceToDevice, f->stream));
      HIP_TRY(hipStreamSynchronize(f->stream));
    }
    c.elem_kinds = std::move(nk);
    c.elem_payload = std::move(np);
  }
  // the offsets continue from the elements held: entry n_list_rows (0 for the first append, else the end of the last row) is
  // written again with the value it has
  std::vector<long long> shifted((size_t)n + 1);
  for (int64_t i = 0; i <= n; ++i) shifted[(size_t)i] = c.n_elems + (long long)elem_off[i];
  HIP_TRY(hipMemcpyAsync(c.list_off.p + c.n_list_rows, shifted.data(), shifted.size() * sizeof(long long), hipMemcpyHostToDevice, f->stream));
  if (m) {
    HIP_TRY(hipMemcpyAsync(c.elem_kinds.p + c.n_elems, elem_kinds, (size_t)m, hipMemcpyHostToDevice, f->stream));
    HIP_TRY(hipMemcpyAsync(c.elem_payload.p + c.n_elems, elem_payload, (size_t)m * sizeof(u64), hipMemcpyHostToDevice, f->stream));
  }
  HIP_TRY(hipStreamSynchronize(f->stream));   // the caller's arrays and `shifted` are free again
  c.n_list_rows += n;
  c.n_elems += m;
  return VRAG_OK;
}

int vrag_row_filter_list_rows(vrag_row_filter* f, int32_t col, int64_t* n_rows, int64_t* n_elems) {
  ARG_CHECK(f && n_rows && n_elems, "null argument");
  std::lock_guard<std::mutex> lk(f->mu);
  ARG_CHECK(col >= 0 && col < (int)f->cols.size(), "vrag_row_filter_list_rows: no column %d (the filter holds %d)", col,
            (int)f->cols.size());
  *n_rows = f->cols[col].n_list_rows;
  *n_elems = f->cols[col].n_elems;
  return VRAG_OK;
}

}  // extern "C"
