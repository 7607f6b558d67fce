// Span selection over per-token logits of the 2-label token head (csrc/spans.hip; include/vrag_amd.h states the semantics).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "host_util.h"

namespace vrag {

// Device buffers of one call, kept by their owner between calls (reserve() grows them).
struct TokenSpanScratch {
  DevBuf win, win_off, job_off, offsets, counts, spans;
};

// The arguments of vrag_encoder_read_token_spans, with the logits as a device array [n_rows, 2] and win_row[w] already a row of
// it.  Checks every table against n_rows and against the others before anything is launched; synchronises `st`.
int run_token_spans(TokenSpanScratch& ws, const float* d_logits, int64_t n_rows, const int32_t* win_job, const int32_t* win_a,
                    const int32_t* win_b, const int32_t* win_row, int32_t n_windows, const int64_t* job_off, const int32_t* offsets,
                    int32_t n_jobs, float tau, int32_t min_span_chars, int32_t merge_gap_chars, int32_t cap_per_job, int32_t* counts,
                    int32_t* spans, hipStream_t st);

}  // namespace vrag
