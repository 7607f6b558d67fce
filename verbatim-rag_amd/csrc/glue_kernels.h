// Launchers of the encoder's packing and glue kernels (csrc/capi.hip): the weight / activation converters, the LayerNorm
// statistics finalisation, the packed-row layout and the SPLADE row compaction.  Declared here so that the unit-test hook
// (csrc/debug_api.hip, vrag_debug_glue_run) launches the product's own kernels with the product's own grids.  None of them
// checks its arguments or the launch: the caller reads hipGetLastError().
#pragma once
#include "common.h"

namespace vrag {

// dst [rows_dst, cols] <- op16(src [rows_src, cols] * col_scale), zero rows beyond rows_src; interleave_I > 0 = the GeGLU row
// interleave; row_sum [rows_dst] over the rounded row; dst_lo the remainder.  One workgroup per row: grid = dim3(rows_dst).
void launch_cvt_rows(int op_dtype, dim3 grid, hipStream_t st, const float* src, bf16_t* dst, int rows_dst, int rows_src, int cols,
                     int interleave_I, const float* col_scale, float* row_sum, bf16_t* dst_lo, unsigned* f16_sat);
// dst [rows_dst, 3 cols] <- [hi | hi | lo] of src [rows_src, cols], zero rows beyond rows_src.
void launch_cvt_split3(int op_dtype, hipStream_t st, const float* src, bf16_t* dst, int rows_dst, int rows_src, int cols,
                       unsigned* f16_sat);
// part: slice-major partial sums [np][ld][2] of (h - shift_in); rows [0, rows) of mu_rel, rstd, shift_out (shift_in may alias
// it) and shift_prev_out (nullable) are written.
void launch_ln_stats_finalize(hipStream_t st, const float* part, int ld, int np, int H, float eps, int rows, float* mu_rel, float* rstd,
                              const float* shift_in, float* shift_out, float* shift_prev_out);
// ids / pos / tok_seq of rows [0, rows): the sequence's ids, position and index on its rows, (pad_id, 0, -1) on every other row.
void launch_pack_layout(hipStream_t st, const int* packed, const int* seq_row, const int* seq_src, const int* seq_len, int n_seqs,
                        int rows, int pad_id, int* ids, int* pos, int* tok_seq);
// rows [n_rows, ld] (ld % 4 == 0, ld >= V): per row the entries > thr, in index order, at most cap of them stored at row * cap;
// counts [n_rows] = the row's total, stored or not.
void launch_splade_compact(hipStream_t st, const float* rows, int n_rows, int V, int ld, float thr, int cap, int* counts, int* idx,
                           float* val);

}  // namespace vrag
