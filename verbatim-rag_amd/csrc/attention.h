// Packed (padding-free) bidirectional attention, global or banded |i-j| <= window (gfx950).
#pragma once
#include "common.h"

namespace vrag {

// Operand contract.  A launch reads every 64-key tile of a sequence WHOLE, the rows behind the sequence included, clamped at Tp
// (K at row min(.., Tp - 1), V^T at column min(.., Tp - 8)).  A masked key has P == 0 exactly, but 0 * V is still formed in the
// P.V MFMA, and a masked score is replaced, not skipped.  So every K row and every V^T column a launch can address -- all of
// [0, Tp) -- must be FINITE: a NaN or inf in a V^T column behind a sequence poisons that sequence's live rows.  Q rows behind a
// sequence may hold anything: they only feed dead query rows, which are never stored (their 0 / 0 stays in registers and does
// not set the fp16 clamp word: the store converts live rows only).  In the product the encoder guarantees it: dev_alloc
// zero-fills q, k and vt, and every later store there is a bf16 value of finite activations or an fp16 value clamped at
// +-65504 (Op<f16_t>::to).  The unit test (tests/test_attn_unit_gpu.py) fills those rows with finite garbage.
struct AttnParams {
  const bf16_t* q;   // [Tp, H]  RoPE'd and pre-scaled by head_dim^-1/2 * log2(e)
  const bf16_t* k;   // [Tp, H]  RoPE'd
  const bf16_t* vt;  // [H, Tp]  V transposed (row = head*64+d, col = token)
  bf16_t* o;         // [Tp, H]
  const int* blk_seq_start;  // [n_blocks] first packed token of the q-block's sequence
  const int* blk_seq_len;    // [n_blocks] sequence length S
  const int* blk_q0;         // [n_blocks] first query row of the block inside its sequence (x attention_q_block(local))
  int n_blocks;
  int H;       // hidden = nh * 64
  int nh;
  int Tp;      // padded token rows (leading dimension of vt)
  int window;  // banded layers: keep |i-j| <= window; ignored for global layers
  int op_dtype;  // kOpBf16 / kOpF16: what q, k, vt and o hold
  unsigned* f16_sat;  // clamp word (GemmParams::f16_sat); required for kOpF16
};

hipError_t launch_attention(const AttnParams& p, bool local, hipStream_t stream);
int attention_q_block(bool local);  // query rows per work item (256 on global and on banded layers)

}  // namespace vrag
