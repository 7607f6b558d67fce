// What the two scan kernels of an IVF search share (csrc/ivf.hip: fp32 / bf16 rows; csrc/ivf_sq8.hip: SQ8 rows): the shape of a
// work item and the launcher of the SQ8 scan.  The work items themselves are built by the invert stage of csrc/ivf.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace vrag {

constexpr int IVF_QG = 16;          // queries of one scan work item
constexpr int IVF_ROWS = 16;        // rows of one scan step; a list's rows are cut into ranges (blockIdx.y) by groups of this many
constexpr int IVF_RANK_BITS = 14;   // a pair is packed (query in slice << 14) | probe rank

// ivf_sq8_scan_kernel over grid (work-item workgroups, row ranges): the rows of each work item's list (list_off / list_rows) among
// codes [..][stride] / scales, against the quantised queries qcodes [nq][stride] / qscales [nq]; cand [probe rank][range][query][k].
// No argument is checked; the launch's status (or that of raising the kernel's LDS limit) is returned.
hipError_t launch_ivf_sq8_scan(dim3 grid, const signed char* codes, const float* scales, int stride, const unsigned* list_off,
                               const unsigned* list_rows, const signed char* qcodes, const float* qscales, int nq, int k,
                               const unsigned* n_items, const unsigned* item_list, const unsigned* item_n, const unsigned* item_pair,
                               u64* cand, hipStream_t st);

}  // namespace vrag
