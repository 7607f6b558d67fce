// The host frame shared by the device tokenizers' encode entries (csrc/wordpiece.hip, csrc/bpe.hip): what a handle holds
// whatever its algorithm, and the one function that checks a batch, uploads it, asks the tokenizer for its two passes and
// packs the ids (token_pack.h) into the caller's arrays.  Host code only.
#pragma once
#include <algorithm>
#include <mutex>
#include <type_traits>

#include "host_util.h"
#include "token_pack.h"
#include "utf8_text.h"

namespace vrag {

// Head of every tokenizer handle; the handle adds its tables and the scratch only its own kernels use.
struct TokenizerBase {
  int device = 0, flags = 0, cls_id = 0, sep_id = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  // workspace of one call, grown on demand
  DevArray<unsigned char> text, needs;
  DevArray<long long> off;
  DevArray<unsigned> tile_cnt, tile_off, wstart, wdoc, tok_cnt, tok_scan, body, seq_len, out_off;
  DevArray<int> tok, ids;
};

template <typename H>
void tokenizer_destroy(H* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  hipStream_t st = h->stream;
  if (st) (void)hipStreamSynchronize(st);
  delete h;   // DevArrays free themselves
  if (st) (void)hipStreamDestroy(st);
}

// The arguments every encode entry takes (include/vrag_amd.h).
struct EncodeArgs {
  const uint8_t* text;
  const int64_t* doc_off;
  int32_t n_docs, add_special_tokens, max_length;
  int64_t cap;
  int32_t* ids;
  int32_t* seq_lens;
  uint8_t* needs_host;
  int64_t* n_ids;
};
// Per-id (start, end) next to the ids: `span` lies beside `tok` (filled by the word pass), `offs` beside `ids`, `host` is the caller's.
struct EncodeOffsets {
  int32_t* host;
  DevArray<int2>& span;
  DevArray<int2>& offs;
};

// One encode call of entry `fn` on handle `h`: a batch of at most `max_batch_bytes`, cut into tiles of `tile_bytes`.
//   count_pass(st, n_bytes, n_tiles)          everything the tokenizer queues to count the words of every tile, ending with
//                                             tile_off = scan_u32(tile_cnt) and whatever it queues behind that scan
//   word_pass(st, n_bytes, n_tiles, n_words)  (only when there are words) grows its own per-word scratch and queues the kernels that
//                                             write wstart / wdoc, the words' ids at tok[wstart[w]], tok_cnt and body
// Both return a status.  `offsets` is a const EncodeOffsets* (null: ids only) or, for a tokenizer without offsets, a literal nullptr,
// which keeps pack_gather_kernel<int2> out of its code object.
template <typename Offsets, typename Count, typename Words>
int tokenizer_encode(const char* fn, long long max_batch_bytes, int tile_bytes, TokenizerBase* h, const EncodeArgs& a, Offsets offsets,
                     Count count_pass, Words word_pass) {
  const int32_t n_docs = a.n_docs, max_length = a.max_length;
  ARG_CHECK(h && a.doc_off && a.n_ids && n_docs >= 0 && a.cap >= 0 && (a.ids || a.cap == 0), "%s: bad arguments", fn);
  ARG_CHECK(n_docs == 0 || (a.seq_lens && a.needs_host), "%s: null seq_lens / needs_host", fn);
  ARG_CHECK(max_length >= (a.add_special_tokens ? 2 : 0), "%s: max_length %d leaves no room%s", fn, max_length,
            a.add_special_tokens ? " for the two special tokens" : "");
  ARG_CHECK(a.doc_off[0] == 0, "%s: doc_off[0] must be 0", fn);
  for (int32_t d = 0; d < n_docs; ++d) ARG_CHECK(a.doc_off[d + 1] >= a.doc_off[d], "%s: doc_off must be non-decreasing (text %d)", fn, d);
  const long long n_bytes = a.doc_off[n_docs];
  ARG_CHECK(n_bytes <= max_batch_bytes, "%s: a batch holds at most %lld bytes of text, got %lld", fn, max_batch_bytes, n_bytes);
  ARG_CHECK(n_bytes + 2ll * n_docs < 0x7FFFFFF0ll, "%s: text bytes + 2 * n_docs must stay below 2^31", fn);
  ARG_CHECK(n_bytes == 0 || a.text, "%s: null text", fn);
  *a.n_ids = 0;
  if (n_docs == 0) return VRAG_OK;
  const int special = a.add_special_tokens ? 1 : 0;
  std::lock_guard<std::mutex> lock(h->mu);
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const long long n_tiles = std::max<long long>(1, (n_bytes + tile_bytes - 1) / tile_bytes);
  HIP_TRY(h->text.grow((size_t)n_bytes + 16));
  HIP_TRY(h->off.grow((size_t)n_docs + 1));
  HIP_TRY(h->needs.grow((size_t)n_docs));
  HIP_TRY(h->body.grow((size_t)n_docs));
  HIP_TRY(h->seq_len.grow((size_t)n_docs));
  HIP_TRY(h->out_off.grow((size_t)n_docs + 1));
  HIP_TRY(h->tile_cnt.grow((size_t)n_tiles));
  HIP_TRY(h->tile_off.grow((size_t)n_tiles + 1));
  if (n_bytes) HIP_TRY(hipMemcpyAsync(h->text.p, a.text, (size_t)n_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(h->off.p, a.doc_off, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(h->needs.p, 0, (size_t)n_docs, st));
  HIP_TRY(hipMemsetAsync(h->body.p, 0, (size_t)n_docs * 4, st));
  if (int rc = count_pass(st, n_bytes, n_tiles)) return rc;
  unsigned n_words = 0;
  HIP_TRY(read_u32(h->tile_off.p + n_tiles, &n_words, st));
  if (n_words) {
    HIP_TRY(h->wstart.grow(n_words));
    HIP_TRY(h->wdoc.grow(n_words));
    HIP_TRY(h->tok_cnt.grow(n_words));
    HIP_TRY(h->tok_scan.grow((size_t)n_words + 1));
    HIP_TRY(h->tok.grow((size_t)n_bytes));
    if (int rc = word_pass(st, n_bytes, n_tiles, (long long)n_words)) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(scan_u32(h->tok_cnt.p, n_words, h->tok_scan.p, st));
  }
  hipLaunchKernelGGL(pack_seq_len_kernel, dim3(grid_of(n_docs, 256)), dim3(256), 0, st, h->body.p, (int)n_docs, special, (int)max_length,
                     h->seq_len.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(scan_u32(h->seq_len.p, n_docs, h->out_off.p, st));
  unsigned total = 0;
  HIP_TRY(read_u32(h->out_off.p + n_docs, &total, st));
  *a.n_ids = total;
  HIP_TRY(hipMemcpyAsync(a.seq_lens, h->seq_len.p, (size_t)n_docs * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(a.needs_host, h->needs.p, (size_t)n_docs, hipMemcpyDeviceToHost, st));
  if ((int64_t)total <= a.cap && total) {
    HIP_TRY(h->ids.grow(total));
    if (n_words)
      hipLaunchKernelGGL(pack_gather_kernel<int>, dim3(grid_of(n_words, 256)), dim3(256), 0, st, h->wstart.p, h->wdoc.p, (long long)n_words,
                         h->tok.p, h->tok_scan.p, h->out_off.p, special, (int)max_length, h->ids.p);
    if (special)
      hipLaunchKernelGGL(pack_special_kernel, dim3(grid_of(n_docs, 256)), dim3(256), 0, st, h->out_off.p, (int)n_docs, h->cls_id, h->sep_id,
                         h->ids.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(a.ids, h->ids.p, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    if constexpr (!std::is_null_pointer_v<Offsets>) {
      if (offsets) {   // [CLS] / [SEP] keep the (0, 0) of the memset
        HIP_TRY(offsets->offs.grow(total));
        HIP_TRY(hipMemsetAsync(offsets->offs.p, 0, (size_t)total * sizeof(int2), st));
        if (n_words)
          hipLaunchKernelGGL(pack_gather_kernel<int2>, dim3(grid_of(n_words, 256)), dim3(256), 0, st, h->wstart.p, h->wdoc.p,
                             (long long)n_words, offsets->span.p, h->tok_scan.p, h->out_off.p, special, (int)max_length, offsets->offs.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(offsets->host, offsets->offs.p, (size_t)total * sizeof(int2), hipMemcpyDeviceToHost, st));
      }
    }
  }
  HIP_TRY(hipStreamSynchronize(st));
  if ((int64_t)total > a.cap) {
    set_error("%s: %u ids, cap %lld", fn, total, (long long)a.cap);
    return VRAG_ERR_CAPACITY;
  }
  return VRAG_OK;
}

}  // namespace vrag
