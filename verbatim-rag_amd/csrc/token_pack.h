// The packing step shared by the device tokenizers (csrc/wordpiece.hip, csrc/bpe.hip): ids per text after truncation, the
// surviving ids of every word at their place in the output, [CLS] / [SEP].  A word is (start byte, text); its ids lie in a
// scratch array at its start byte, and tok_scan is the exclusive scan of the words' id counts.  Launched by tokenizer_encode
// (token_frame.h) only.
#pragma once
#include <hip/hip_runtime.h>

namespace vrag {

// ids of every text after truncation, specials included
static __global__ void pack_seq_len_kernel(const unsigned* __restrict__ body, int n_docs, int special, int max_length, unsigned* __restrict__ seq_len) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n_docs) return;
  const unsigned keep = (unsigned)(special ? max_length - 2 : max_length);
  seq_len[d] = min(body[d], keep) + (special ? 2u : 0u);
}

// One lane per word: the ids of the word that lie below the text's truncation limit, at their place in the output.  T = int for
// the ids; the BPE tokenizer moves its per-id character offsets (int2) the same way.
template <typename T>
static __global__ void pack_gather_kernel(const unsigned* __restrict__ wstart, const unsigned* __restrict__ wdoc, long long n_words,
                                 const T* __restrict__ tok, const unsigned* __restrict__ tok_scan, const unsigned* __restrict__ out_off,
                                 int special, int max_length, T* __restrict__ ids) {
  const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_words) return;
  const unsigned d = wdoc[w];
  long long lo = 0, hi = w;   // first word of text d
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (wdoc[mid] < d) lo = mid + 1;
    else hi = mid;
  }
  const unsigned keep = (unsigned)(special ? max_length - 2 : max_length);
  const unsigned first = tok_scan[w] - tok_scan[lo], n = tok_scan[w + 1] - tok_scan[w];
  T* out = ids + out_off[d] + (special ? 1 : 0);
  const T* src = tok + wstart[w];
  for (unsigned j = 0; j < n && first + j < keep; ++j) out[first + j] = src[j];
}

static __global__ void pack_special_kernel(const unsigned* __restrict__ out_off, int n_docs, int cls_id, int sep_id, int* __restrict__ ids) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n_docs) return;
  ids[out_off[d]] = cls_id;
  ids[out_off[d + 1] - 1u] = sep_id;
}

}  // namespace vrag
