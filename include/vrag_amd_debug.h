/* vrag_amd_debug.h -- tuning / unit-test harness of the gfx950 kernels.  NOT part of the product ABI (include/vrag_amd.h):
 * these entry points exist only in libvrag_amd_dbg.so, the harness build of the same sources (verbatim-rag_amd/build.py,
 * -DVRAG_DEBUG_API: it also keeps the phase-decomposition branches of the fused kernel that the product build compiles out).
 * tools/, tests/test_attention_unit_gpu.py, tests/test_attn_unit_gpu.py, tests/test_gemm_unit_gpu.py,
 * tests/test_qkv_attn_unit_gpu.py, tests/test_qkv_attn_band_blocks_gpu.py, tests/test_rows_unit_gpu.py, tests/test_glue_unit_gpu.py, tests/test_topk_unit_gpu.py,
 * tests/test_topk_instantiations_gpu.py, tests/test_scale_gpu.py and
 * tests/test_text_unit_gpu.py load it beside the product library. */
#ifndef VRAG_AMD_DEBUG_H
#define VRAG_AMD_DEBUG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Average ms of one GEMM instantiation (epilogue id as in csrc/gemm_bf16.h, 7 = no epilogue) on synthetic [-1,1) operands. */
int vrag_debug_gemm_ms(int32_t epi, int32_t M, int32_t N, int32_t K, int32_t iters, int32_t device, float* ms_out);
/* Same for one attention launch: n_seqs sequences of S tokens (S a multiple of 8), hidden H = 64 * heads, local != 0 =
 * the banded kernel with |i - j| <= window. */
int vrag_debug_attn_ms(int32_t local, int32_t n_seqs, int32_t S, int32_t H, int32_t window, int32_t iters, int32_t device,
                       float* ms_out);
/* Same for the fused Wqkv + RoPE + attention kernel (csrc/qkv_attn.hip; S <= 512).  flags: 1 = no attention phase, 2 = no
 * main-loop MFMAs, 4 = no operand DMA, 8 = no O store, 16 = return behind the main loop (phase decomposition of the kernel's
 * time); 32 = the banded kernel runs its generic tile body for every wave, never the static in-band-block bodies (FIRST / MID /
 * LAST of csrc/qkv_attn.hip section 3): same bits, the time of the out-of-band blocks back. */
int vrag_debug_qkv_attn_ms(int32_t local, int32_t n_seqs, int32_t S, int32_t H, int32_t window, int32_t iters, int32_t flags,
                           int32_t device, float* ms_out);
/* Unit-test hook of the attention kernels alone (csrc/attention.hip), on the layout the encoder packs: sequences of any length
 * >= 1 at 8-aligned rows of a `rows`-row buffer (rows = AttnParams::Tp, a multiple of 256), anything in the rows between and
 * behind them.  Host operands in the kernels' layouts, ONE launch, o copied back; the q-block descriptors are built as
 * vrag_encoder_set_batch builds them: one block per attention_q_block(local) rows of each sequence, in list order.
 * Refused before anything is launched, each with its own message: null pointers, H % 64 != 0, rows % 256 != 0,
 * rows * H >= 2^31, seq_len < 1, seq_row negative or not a multiple of 8, seq_row + seq_len > rows, overlapping sequences, a
 * banded launch with window < 0 (or above 2^24: the band arithmetic is int), blocks_out too small for the launch.
 * Nothing the hook accepts reads or writes outside its buffers, by the kernel's own clamps: every buffer holds rows * H
 * elements.  Q and K are read at row min(seq_row + r, rows - 1) with r >= 0, columns head * 64 .. + 63 < H: inside [0, rows).
 * V^T is read at row head * 64 + d < H, 8 columns from min(seq_row + c, rows - 8) with c >= 0: inside [0, rows).  O is stored
 * at rows seq_row + g only where g < seq_len, and seq_row + seq_len <= rows is checked.  The descriptor arrays hold n_blocks
 * entries and the grid is n_blocks x H / 64.  A sequence may therefore END ON THE LAST ROW: its last 64-key tile then runs
 * past `rows` and all three clamps bite.  Every device buffer, inputs included, is followed by 4 KiB of canary; the hook fails
 * with VRAG_ERR_HIP if the launch touched any.
 * Operand contract (csrc/attention.h): every K row and V^T column of the buffer must be finite; Q rows outside the
 * sequences may hold anything. */
typedef struct vrag_debug_attn_args {
  const uint16_t* q;         /* [rows, H] bf16 / fp16 bits, pre-scaled by head_dim^-1/2 * log2 e */
  const uint16_t* k;         /* [rows, H] */
  const uint16_t* vt;        /* [H, rows] */
  uint16_t* o;               /* in / out [rows, H]: copied to the device before the launch, so a canary survives where the kernel must not write */
  const int32_t* seq_row;    /* [n_seqs] first row of each sequence */
  const int32_t* seq_len;    /* [n_seqs] */
  int32_t* blocks_out;       /* out [n_blocks][3], nullable: the q-block descriptors that ran (sequence row, sequence length, q0) */
  int32_t rows, H, n_seqs;
  int32_t local, window, f16;
  int32_t blocks_cap;        /* descriptors blocks_out can hold */
  int32_t n_blocks;          /* out */
  int32_t f16_saturated;     /* out: the clamp word, zeroed before the launch and read back after it */
} vrag_debug_attn_args;
int vrag_debug_attn_run_ex(vrag_debug_attn_args* args, int32_t device);
/* The same for the equal-length layout of tools/attn_unit.py, a thin wrapper over vrag_debug_attn_run_ex: n_seqs sequences of
 * S tokens (S a multiple of 8) back to back from row 0; q, k, o: [T, H], T = n_seqs * S; vt: [H, Tp], Tp = T rounded up to 256. */
int vrag_debug_attn_run(int32_t local, int32_t n_seqs, int32_t S, int32_t H, int32_t window, int32_t f16, const uint16_t* q,
                        const uint16_t* k, const uint16_t* vt, uint16_t* o, int32_t device);

/* Unit-test hook of the GEMM alone (csrc/gemm_bf16.h, every epilogue except the top-k search and EPI_NONE): host buffers in the
 * layouts GemmParams documents, every pointer nullable (null = the GemmParams field stays null).  Row-indexed buffers hold
 * `rows` rows (a multiple of 64, at least row0 + M rounded up to 256); the launch covers rows [row0, row0 + M) through pointers
 * offset by row0 rows, as the encoder addresses a micro-batch (byte plane: row0 * N bytes; V^T: row0 columns; statistics:
 * row0 of stats_ld = rows).  16-bit buffers hold bf16 or fp16 bits (f16).  Every buffer marked "in / out" is copied to the
 * device, and back after ONE launch.  lo_out may equal lo_in (one device buffer, as the encoder aliases them). */
typedef struct vrag_debug_gemm_args {
  const uint16_t* A;         /* [rows, K] */
  const uint16_t* W;         /* [N, K] */
  const float* bias;         /* [N] */
  const float* ln_s;         /* [N] */
  const float* stats_in;     /* [K / 64, rows, 2] */
  const float* res_mu;       /* [rows] */
  const float* res_rstd;     /* [rows] */
  const float* res_g;        /* [N] */
  const float* res_b;        /* [N] */
  const float* rope_cos;     /* [rope_rows, 32] */
  const float* rope_sin;     /* [rope_rows, 32] */
  const int32_t* pos;        /* [rows] */
  const int32_t* tok_seq;    /* [rows] */
  const uint8_t* lo_in;      /* [rows * N] */
  float* out_f32;            /* in / out [rows, N] */
  uint16_t* out_bf16;        /* in / out [rows, N] (EPI_GEGLU: [rows, N / 2]) */
  uint16_t* q;               /* in / out [rows, hidden] */
  uint16_t* k;               /* in / out [rows, hidden] */
  uint16_t* vt;              /* in / out [hidden, rows] */
  float* ln_mu;              /* in / out [rows] */
  float* ln_rstd;            /* in / out [rows] */
  float* ln_shift;           /* in / out [rows] */
  float* ln_shift_prev;      /* in / out [rows] */
  uint16_t* resid_bf16;      /* in / out [rows, N] */
  float* stats_part;         /* in / out [N / 64, rows, 2] */
  uint8_t* lo_out;           /* in / out [rows * N] */
  uint32_t* splade_rows;     /* in / out [n_seqs, N] */
  int32_t epi, M, N, K, f16, act_gelu;
  int32_t row0, rows;
  int32_t hidden, rope_rows, n_seqs;
  int32_t small_rows;        /* small-batch row threshold for this call (restored afterwards); < 0 = leave it */
  float q_scale, fin_eps;
  int32_t config[7];         /* out: the tile configuration that ran: BM, BN, WM, WN, NS, HW, KCH */
  int32_t f16_saturated;     /* out: an fp16 conversion of this launch clamped at +-65504 */
} vrag_debug_gemm_args;
int vrag_debug_gemm_run(vrag_debug_gemm_args* args, int32_t device);

/* Unit-test hook of the fused Wqkv + RoPE + attention kernel alone (csrc/qkv_attn.hip): host buffers in, ONE launch with
 * debug_flags = args->debug_flags (0, or 32: the only bit that leaves the result what it is), outputs copied back.  w and ln_s arrive in the encoder's UNPERMUTED Wqkv layout (rows q | k | v of all heads);
 * the hook runs permute_qkv_heads on them as the encoder does at load (ln_s with 64 readable floats behind the last head).
 * Refused before anything is launched: null required pointers, H != 64 * nh, rows % 256 != 0, seq_len outside 1..512,
 * seq_row % 8 != 0, overlapping sequences, and a sequence with seq_row + 64 * ceil(len / 64) > rows (a wave reads 64 WHOLE token
 * rows, whatever its sequence's length: the encoder's row slack pays for that, the hook does not hide it).
 * Every device buffer, inputs included, is followed by 4 KiB of canary; the hook fails with VRAG_ERR_HIP if a launch touched any. */
typedef struct vrag_debug_qkv_attn_args {
  const uint16_t* x;         /* [rows, H] */
  const uint16_t* w;         /* [3 H, H] */
  const float* ln_s;         /* [3 H], null without the fold */
  const float* ln_mu;        /* [rows]; null = the no-fold instantiation */
  const float* ln_rstd;      /* [rows] */
  const float* rope_cos;     /* [rope_rows, 32] */
  const float* rope_sin;     /* [rope_rows, 32] */
  uint16_t* o;               /* in / out [rows, H]: copied to the device before the launch, so a canary survives where the kernel must not write */
  const int32_t* seq_row;    /* [n_seqs] first row of each sequence */
  const int32_t* seq_len;    /* [n_seqs] */
  int32_t* groups_out;       /* out [n_seqs][8][4]: the wave descriptors that ran (QkvAttnParams::groups); the first n_groups * 8 are written */
  int32_t rows, H, nh, rope_rows, n_seqs;
  int32_t packer;            /* 0 = fused_pack_groups (first fit over consecutive sequences), 1 = the engine's best fit decreasing */
  int32_t local, window, f16;
  float q_scale;
  int32_t n_groups;          /* out */
  int32_t f16_saturated;     /* out: an fp16 conversion of this launch clamped at +-65504 */
  int32_t debug_flags;       /* 0, or 32 = generic tile body everywhere (vrag_debug_qkv_attn_ms above); anything else is refused */
} vrag_debug_qkv_attn_args;
int vrag_debug_qkv_attn_run(vrag_debug_qkv_attn_args* args, int32_t device);
/* Host only (no GPU call): the wave descriptors either packer gives n sequences (lengths 1..512); out holds [n][8][4] int32.
 * Returns the number of groups, or a negative status on bad arguments. */
int vrag_debug_pack_groups(const int32_t* seq_row, const int32_t* seq_len, int32_t n, int32_t packer, int32_t* out);

/* Unit-test hook of the row kernels alone (csrc/norm_heads.hip), one launcher per call, chosen by `op`.  Host buffers in, every
 * pointer nullable where the launcher's is (null = the launcher gets null); exactly the launches the launcher makes (one; two for
 * launch_seq_head).  Buffers marked "in / out" are copied to the device before the launch and back after it, also when the
 * launcher refuses, so a canary survives where the kernel must not write.  `rows` is what the launcher calls rows, n_ranges or
 * n_seqs.  H and rows go to the launcher UNCHECKED (H in 1..65536 and rows >= 0 only size the buffers): the launchers' own refusals
 * (H > 1024, H % 4, split3 with out_lo or without out16, fp16 without a clamp word, P without pos, launch_seq_head without w) are
 * part of what is tested.  launch_status returns the launcher's hipError_t; a refusing launcher makes the hook return
 * VRAG_ERR_INVALID with launch_status set, a refusal of the hook itself leaves launch_status untouched.
 * Refused by the hook before anything is launched, each with its own message: a null pointer the chosen kernel dereferences
 * unconditionally, h_rows < rows where rows index h, out_rows < rows, alias_f32 together with out_f32, ids / pos / type_ids /
 * first_row outside their tables, start < 0, end >= h_rows, start > end (the kernel would divide by zero), seq_len < 1,
 * seq_row < 0, seq_row + seq_len > h_rows, num_labels < 1 where a classifier runs.
 * Nothing the hook accepts reads or writes outside its buffers.  Every kernel addresses a row as base + index * H + c with
 * c + 4 <= H (c = 4 * lane + 256 * i, masked by c < H; H % 4 == 0 or the launcher refuses) and the index is: the row number below
 * `rows` (h_rows, out_rows >= rows are checked; the workgroup's rows at and beyond `rows` return before their first access); a
 * gathered index checked above against its table's row count; t in [start, end] or [seq_row, seq_row + seq_len), both ends
 * checked; a label c < num_labels into Wc / bc; k < H into WdT / Wp.  The split3 image has leading dimension 3 H and columns
 * below 3 H, and is sized so.  Every device buffer, inputs included, is followed by 4 KiB of canary: should a launcher's refusal
 * of H % 4 != 0 ever fail, the float4 that straddles the last row's end lands there and not outside the allocation.  The hook
 * fails with VRAG_ERR_HIP if a launch touched any canary. */
enum {
  VRAG_DEBUG_ROWS_EMBED_LN = 0,
  VRAG_DEBUG_ROWS_LAYERNORM = 1,
  VRAG_DEBUG_ROWS_RANGE_POOL = 2,
  VRAG_DEBUG_ROWS_LN_CLASSIFIER = 3,
  VRAG_DEBUG_ROWS_POOLER_CLASSIFIER = 4,
  VRAG_DEBUG_ROWS_SEQ_HEAD = 5
};
typedef struct vrag_debug_rows_args {
  float* h;                  /* [h_rows, H] input rows of every op but embed_ln (ln_classifier: x); in / out with alias_f32 */
  const int32_t* ids;        /* embed_ln [rows], in [0, vocab) */
  const float* E;            /* embed_ln [vocab, H] */
  const float* P;            /* embed_ln [n_pos, H]; null = no position / type rows (ModernBERT form) */
  const int32_t* pos;        /* embed_ln [rows], in [0, n_pos) */
  const float* type_row;     /* embed_ln [n_types, H] */
  const int32_t* type_ids;   /* embed_ln [rows], in [0, n_types); null = row 0 */
  const float* w;            /* [H] LayerNorm gain: embed_ln / layernorm w, lnw of the other four */
  const float* bias;         /* [H] LayerNorm bias: embed_ln / layernorm bias, ln_classifier lnb */
  const int32_t* start;      /* range_pool [rows] */
  const int32_t* end;        /* range_pool [rows], inclusive */
  const int32_t* first_row;  /* pooler_classifier [rows] */
  const int32_t* seq_row;    /* seq_head [rows] */
  const int32_t* seq_len;    /* seq_head [rows] */
  const float* Wp;           /* pooler_classifier [H, H] */
  const float* bp;           /* pooler_classifier [H] */
  const float* WdT;          /* seq_head [H, H], transposed dense weight */
  const float* bd;           /* seq_head [H] */
  const float* wn;           /* seq_head [H] */
  const float* bn;           /* seq_head [H] */
  const float* Wc;           /* [num_labels, H] */
  const float* bc;           /* [num_labels] */
  float* out_f32;            /* in / out: embed_ln h and layernorm out_f32 [out_rows, H]; range_pool out [out_rows, num_labels (mode 0) or H]; the logits of the three classifiers [out_rows, num_labels] */
  uint16_t* out16;           /* in / out: embed_ln a, layernorm out_bf16 [out_rows, H], with split3 [out_rows, 3 H] */
  uint16_t* out_lo;          /* in / out: layernorm out_lo [out_rows, H] */
  float* row_mean;           /* in / out: layernorm row_mean [out_rows] */
  float* pooled;             /* in / out: seq_head pooled [out_rows, H] */
  int32_t op, H, rows;
  int32_t h_rows, out_rows;  /* rows h holds; rows every in / out buffer holds (>= rows) */
  int32_t vocab, n_pos, n_types;
  int32_t num_labels;
  int32_t mode;              /* range_pool mode; seq_head pool_mean */
  int32_t gelu_first, split3;
  int32_t alias_f32;         /* layernorm: out_f32 = h itself (out_f32 must be null; h is copied back) */
  int32_t f16;
  int32_t no_sat;            /* the launcher gets a null clamp word (fp16: it must refuse) */
  float eps;
  int32_t launch_status;     /* out: the launcher's hipError_t */
  int32_t f16_saturated;     /* out: the clamp word, zeroed before the launch and read back after it */
} vrag_debug_rows_args;
int vrag_debug_rows_run(vrag_debug_rows_args* args, int32_t device);

/* Unit-test hook of the encoder's packing and glue kernels alone (csrc/glue_kernels.h: the launchers of csrc/capi.hip, and
 * permute_qkv_heads of csrc/qkv_attn.hip), one launcher per call, chosen by `op`.  Host buffers in, exactly the launcher's
 * launches (one), buffers marked "in / out" copied to the device before the launch and back after it, so a canary survives where
 * the kernel must not write.  fp16 launches (f16 != 0) return the clamp word, zeroed before the launch and read after it.
 * Refused by the hook before anything is launched, each with its own message: a null required pointer; rows_dst, rows_src, cols,
 * V, rows or out_rows <= 0; interleave with I <= 0; out_rows below the rows the launch covers; ld < V rounded up to 4 or
 * ld % 4 != 0; cap < 1; n_seqs < 1, seq_row negative or not ascending, seq_len < 0, a sequence running past `rows`, seq_src
 * negative or seq_src + seq_len beyond the n_packed ids; nh < 1 or H != 64 * nh; np * 64 != H; row0 < 0 or ld < row0 + rows.
 * Nothing the hook accepts reads or writes outside its buffers.  Index ranges per op:
 *   CVT_ROWS      one workgroup per row r < rows_dst (the grid).  Reads src row s < rows_src, columns c < cols (without the
 *                 interleave s = r, else s = f or I + f with f < I checked by the kernel, and s < rows_src by its guard);
 *                 col_scale[c]; writes dst / dst_lo [r, c] and row_sum[r]: rows below rows_dst <= out_rows.
 *   CVT_SPLIT3    the same rows; writes dst [r, 0 .. 3 cols): the image has leading dimension 3 cols and is sized so.
 *   LN_STATS_FINALIZE  lane r < rows reads part[(i * ld + row0 + r) * 2 + {0, 1}], i < np: below np * ld * 2 because
 *                 row0 + rows <= ld; reads shift_in and writes mu, rstd, shift_out, shift_prev at row0 + r < ld.
 *   PACK_LAYOUT   lane r < rows reads seq_row / seq_src / seq_len[lo], lo < n_seqs (the bisection keeps 0 <= lo < hi <= n_seqs),
 *                 packed[seq_src[lo] + i] with 0 <= i < seq_len[lo]: below n_packed, checked; writes ids, pos, tok_seq[r],
 *                 r < rows <= out_rows.
 *   SPLADE_COMPACT  workgroup s < rows reads src[s * ld + v .. v + 3] with v % 4 == 0 and v < V: below s * ld + align4(V) <=
 *                 (s + 1) * ld; writes counts[s] and idx / val[s * cap + off] only where off < cap.
 *   PERMUTE_QKV_HEADS  workgroup orow < 3 H reads w row (orow % 192 / 64) * H + orow / 192 * 64 + orow % 64 < 3 H, columns < H,
 *                 and s at the same index; writes w_out row orow and s_out[orow]: out_rows >= 3 H is checked.
 * Every device buffer, inputs included, is followed by 4 KiB of canary; the hook fails with VRAG_ERR_HIP if a launch touched any. */
enum {
  VRAG_DEBUG_GLUE_CVT_ROWS = 0,
  VRAG_DEBUG_GLUE_CVT_SPLIT3 = 1,
  VRAG_DEBUG_GLUE_LN_STATS_FINALIZE = 2,
  VRAG_DEBUG_GLUE_PACK_LAYOUT = 3,
  VRAG_DEBUG_GLUE_SPLADE_COMPACT = 4,
  VRAG_DEBUG_GLUE_PERMUTE_QKV_HEADS = 5
};
typedef struct vrag_debug_glue_args {
  const float* src;          /* cvt_rows / cvt_split3 [rows_src, cols]; splade_compact [rows, ld] */
  const float* col_scale;    /* cvt_rows [cols], nullable */
  uint16_t* dst;             /* in / out: cvt_rows [out_rows, cols]; cvt_split3 [out_rows, 3 cols] */
  uint16_t* dst_lo;          /* in / out: cvt_rows [out_rows, cols], nullable */
  float* row_sum;            /* in / out: cvt_rows [out_rows], nullable */
  const float* part;         /* ln_stats_finalize [np, ld, 2] */
  float* mu;                 /* in / out: ln_stats_finalize [ld] */
  float* rstd;               /* in / out: ln_stats_finalize [ld] */
  const float* shift_in;     /* ln_stats_finalize [ld], nullable (must be null with alias_shift) */
  float* shift_out;          /* in / out: ln_stats_finalize [ld]; with alias_shift also the kernel's shift_in */
  float* shift_prev;         /* in / out: ln_stats_finalize [ld], nullable */
  const int32_t* packed;     /* pack_layout [n_packed] ids back to back */
  const int32_t* seq_row;    /* pack_layout [n_seqs] first row, ascending */
  const int32_t* seq_src;    /* pack_layout [n_seqs] first id in packed */
  const int32_t* seq_len;    /* pack_layout [n_seqs] */
  int32_t* ids;              /* in / out: pack_layout [out_rows] */
  int32_t* pos;              /* in / out: pack_layout [out_rows] */
  int32_t* tok_seq;          /* in / out: pack_layout [out_rows] */
  int32_t* counts;           /* in / out: splade_compact [out_rows] */
  int32_t* idx;              /* in / out: splade_compact [out_rows, cap] */
  float* val;                /* in / out: splade_compact [out_rows, cap] */
  const uint16_t* w;         /* permute_qkv_heads [3 H, H] */
  const float* s;            /* permute_qkv_heads [3 H], nullable */
  uint16_t* w_out;           /* in / out: permute_qkv_heads [out_rows, H] */
  float* s_out;              /* in / out: permute_qkv_heads [out_rows], nullable */
  int32_t op, f16;
  int32_t rows_dst, rows_src, cols;   /* cvt_rows / cvt_split3 */
  int32_t interleave, I;     /* cvt_rows: interleave != 0 = the GeGLU interleave of I features (the launcher gets I, else 0) */
  int32_t out_rows;          /* rows every in / out buffer holds, ln_stats_finalize excepted: >= rows_dst, rows or 3 H */
  int32_t rows;              /* ln_stats_finalize, pack_layout, splade_compact: the launcher's rows / fill_to / n */
  int32_t ld, row0, H, np;   /* ln_stats_finalize: rows of the whole buffer; the launch covers [row0, row0 + rows) through offset pointers (partials + row0 * 2, the rest + row0); splade_compact: ld; permute_qkv_heads: H */
  int32_t nh;                /* permute_qkv_heads */
  int32_t alias_shift;       /* ln_stats_finalize: shift_in = shift_out, one device buffer, as the encoder passes them */
  int32_t n_seqs, n_packed, pad_id;   /* pack_layout */
  int32_t V, cap;            /* splade_compact */
  float thr, eps;            /* splade_compact; ln_stats_finalize */
  int32_t f16_saturated;     /* out: the clamp word of an fp16 cvt launch */
} vrag_debug_glue_args;
int vrag_debug_glue_run(vrag_debug_glue_args* args, int32_t device);

/* Unit-test hook of the tiled batched dense search's kernels alone (csrc/topk_kernels.h; the score stage is
 * launch_gemm(EPI_TOPK, ...) of csrc/gemm_bf16.h), one launcher per call, chosen by `op`.  Host buffers in, exactly the launcher's
 * launches (one), buffers marked "in / out" copied to the device before the launch and back after it, so a canary survives where
 * the kernel must not write.  Every per-query buffer holds nq_buf >= nq queries: the rows behind nq are the caller's canary.
 * Refused by the hook before anything is launched, each with its own message: a null required pointer; nq < 1 or nq_buf < nq;
 * k outside 1..64 or k > cap; cap < 2; K (dim) % 64 != 0; N not 64 with tile 2, 128 with tile 1 or a multiple of 256 with tile 0;
 * nq (2 nq with pairs) above N; M < 1; direct mode with cap < M; appending mode with a preset counter above cap (it is the carry);
 * row_base + M beyond corpus_rows; stride or skip (> 1) together, with M % 256 != 0, in direct / appending mode respectively
 * only, with tile 0 and N > 256 where N / 256 does not divide 256 (no whole round), or on a launch that takes a 128-row tile
 * configuration (those do not walk the map); any corpus tile the launch would read through row_base, stride, skip or tile0 at or
 * beyond the corpus's padded tiles, and with stride / skip at or beyond corpus_rows / 256; a selection's cap not a power of two or
 * above 4096; the first selection's cap below its first window (min(n, 256), k > 16: min(n, 1024), rounded up to a power of two);
 * n < 1 or n > src_stride; rescue with dim % 64 != 0, dim > 4096, n_rows < 1 or slices outside 8..64; merge with n < 1.
 * Nothing the hook accepts reads or writes outside its buffers.  Index ranges per op:
 *   SCORE_STAGE   A = corpus + row_base * K (stride / skip: corpus itself), W = w [N, K].  A launch of T = ceil(M / BM) row tiles
 *                 reads whole tiles of BM rows: rows [row_base, row_base + T * BM) -- inside the allocation, which is padded to whole
 *                 256-row tiles, checked -- or, 256-row forms with stride / skip, corpus tile t * stride / map(tile0 + t), t < M / 256,
 *                 map(d) = d + d / (skip - 1) + 1 below 256 (skip - 1) and d + 256 beyond: below corpus_rows / 256, checked.  W is
 *                 read in whole column tiles of BN | N.  The epilogue reads thr_score / thr_key[query] and adds to cnt[query] with
 *                 query < nq only; direct mode stores buf[query * cap + m], m < M <= cap; appending mode stores
 *                 buf[query * cap + slot] where slot < cap (its own test).
 *   QUERIES       workgroup r < N (the grid) reads queries[(pairs ? r / 2 : r) * K + c] where that query < nq, c < K; writes w_out[r * K + c].
 *   SELECT        workgroup q < nq reads cnt[q] and buf[q * cap + i], i < min(cnt[q], cap); sorts P <= cap keys in LDS (cap a power of
 *                 two); writes buf[q * cap + i], out[q * k + i], i < k <= cap, cnt, thr_key, thr_score, ovf[q].
 *   SELECT_DIRECT workgroup q < nq reads src[q * src_stride + i], i < n <= src_stride; LDS slots k + pos < cap by its own test, the
 *                 first window <= cap checked; writes as SELECT.
 *   RESCUE        grid (nq, slices).  Reads ovf[q]; corpus rows r < n_rows = n, 8 columns from c < K; queries[q * K + c]; writes
 *                 part[(slice * nq + q) * k + i], done[q], out[q * k + i] of flagged queries; part is the hook's own scratch.
 *   MERGE         workgroup q < nq reads src[(w * nq + q) * k + j], w < n, j < k; writes out[q * k + j].
 *   TAU           lane q < nq reads eps[q]; writes thr_key, thr_score, cnt, ovf[q].
 * Every device buffer, inputs included, is followed by 4 KiB of canary; the hook fails with VRAG_ERR_HIP if a launch touched any. */
enum {
  VRAG_DEBUG_TOPK_SCORE_STAGE = 0,
  VRAG_DEBUG_TOPK_QUERIES = 1,
  VRAG_DEBUG_TOPK_SELECT = 2,
  VRAG_DEBUG_TOPK_SELECT_DIRECT = 3,
  VRAG_DEBUG_TOPK_RESCUE = 4,
  VRAG_DEBUG_TOPK_MERGE = 5,
  VRAG_DEBUG_TOPK_TAU = 6
};
typedef struct vrag_debug_topk_args {
  const uint16_t* corpus;    /* score_stage, rescue [corpus_rows, K] bf16 bits (the hook pads the device copy to whole 256-row tiles with zeros) */
  const uint16_t* w;         /* score_stage [N, K] bf16 bits: the query operand (pairs: rows 2q, 2q + 1) */
  const float* queries;      /* queries, rescue [nq, K] */
  const float* eps;          /* tau [nq] */
  const uint64_t* src;       /* select_direct [nq, src_stride]; merge [n, nq, k] */
  uint16_t* w_out;           /* in / out: queries [N, K] */
  uint64_t* buf;             /* in / out: score_stage, select, select_direct [nq_buf, cap] */
  uint32_t* cnt;             /* in / out: score_stage, select, select_direct, tau [nq_buf] */
  uint64_t* thr_key;         /* in / out: the same ops [nq_buf] */
  float* thr_score;          /* in / out: the same ops [nq_buf] */
  uint64_t* out;             /* in / out: select, select_direct (nullable), rescue, merge [nq_buf, k] */
  uint32_t* ovf;             /* in / out: select, select_direct, tau [nq_buf]; rescue: the flags it reads */
  uint32_t* done;            /* in / out: rescue [nq_buf] slice counters */
  int32_t op;
  int32_t M, N, K;           /* score_stage: GemmParams M, N, K; queries: N = n_cols_pad, K = dim; rescue: K = dim */
  int32_t corpus_rows;
  int32_t nq, nq_buf;
  int32_t k, cap;
  int32_t pairs, direct, tile;   /* GemmParams topk_pairs, topk_direct, topk_tile */
  uint32_t row_base;         /* GemmParams topk_row_base */
  int32_t tile_stride, tile_skip, tile0;   /* GemmParams topk_tile_stride, topk_tile_skip, topk_tile0 */
  int32_t n;                 /* select_direct: keys per query; rescue: n_rows; merge: lists */
  int32_t src_stride;        /* select_direct */
  int32_t slices;            /* rescue */
  int32_t small_rows;        /* score_stage: small-batch row threshold for this call (restored afterwards); < 0 = leave it */
  int32_t config[7];         /* out, score_stage: the tile configuration that ran: BM, BN, WM, WN, NS, HW, KCH */
} vrag_debug_topk_args;
int vrag_debug_topk_run(vrag_debug_topk_args* args, int32_t device);

/* Launch log of the dense scan, prefilter, sparse and per-query merge kernels of csrc/topk.hip, which the harness build compiles
 * with a note in front of each of their launches (the product build has none).  Every vrag_dense_index_* / vrag_sparse_index_*
 * call made through THIS library appends one entry (id, p0, p1) per launch, in launch order: the kernel and the template
 * instantiation its selection code picked.  Not logged: the tiled search (vrag_debug_topk_run tests its kernels), the filtered
 * searches, IVF, SQ8, ingest and the shard merge.  The log is per process, holds 4 096 entries and drops what comes after.
 *   id                  kernel                                           p0, p1
 *   DENSE_BF16          dense_topk_kernel<false, QT, DIMC>               QT, DIMC
 *   DENSE_F32           dense_topk_kernel<true, QT, DIMC>                QT, DIMC
 *   MFMA                dense_topk_mfma_kernel                           0, 0
 *   MFMA2               dense_topk_mfma2_kernel<KT>                      KT, 0
 *   EXACT               dense_topk_exact_kernel<NSLOT>                   NSLOT, 0
 *   EXACT2              dense_topk_exact2_kernel<KT>                     KT, 0
 *   SEED_THRESHOLD      topk_seed_threshold_kernel                       0, 0
 *   PF_PREFIX           prefilter_prefix_kernel<DIMC>                    DIMC, 0
 *   PF_COLLECT          prefilter_collect_kernel<DIMC>                   DIMC, 0
 *   PF_COLLECT_MULTI    prefilter_collect_multi_kernel<DIMC32, QN>       DIMC32, QN
 *   PF_RESCORE_LIST     prefilter_rescore_list_kernel<FROM_KEYS>         FROM_KEYS, 0
 *   PF_RESCORE          prefilter_rescore_kernel                         0, 0
 *   PF_COMBINE          prefilter_combine_kernel                         0, 0
 *   SPARSE              sparse_topk_kernel<LDSQ>                         LDSQ, 0
 *   SPARSE_SCATTER      sparse_scatter_queries_kernel                    0, 0
 *   SPARSE_MULTI        sparse_topk_multi_kernel<QB, 16, PAD>            QB, PAD
 *   MERGE_LISTS         topk_merge_lists_kernel                          0, 0
 *   MERGE_SCAN          topk_merge_scan_kernel                           0, 0 */
enum {
  VRAG_DEBUG_TOPK_LAUNCH_DENSE_BF16 = 0,
  VRAG_DEBUG_TOPK_LAUNCH_DENSE_F32 = 1,
  VRAG_DEBUG_TOPK_LAUNCH_MFMA = 2,
  VRAG_DEBUG_TOPK_LAUNCH_MFMA2 = 3,
  VRAG_DEBUG_TOPK_LAUNCH_EXACT = 4,
  VRAG_DEBUG_TOPK_LAUNCH_EXACT2 = 5,
  VRAG_DEBUG_TOPK_LAUNCH_SEED_THRESHOLD = 6,
  VRAG_DEBUG_TOPK_LAUNCH_PF_PREFIX = 7,
  VRAG_DEBUG_TOPK_LAUNCH_PF_COLLECT = 8,
  VRAG_DEBUG_TOPK_LAUNCH_PF_COLLECT_MULTI = 9,
  VRAG_DEBUG_TOPK_LAUNCH_PF_RESCORE_LIST = 10,
  VRAG_DEBUG_TOPK_LAUNCH_PF_RESCORE = 11,
  VRAG_DEBUG_TOPK_LAUNCH_PF_COMBINE = 12,
  VRAG_DEBUG_TOPK_LAUNCH_SPARSE = 13,
  VRAG_DEBUG_TOPK_LAUNCH_SPARSE_SCATTER = 14,
  VRAG_DEBUG_TOPK_LAUNCH_SPARSE_MULTI = 15,
  VRAG_DEBUG_TOPK_LAUNCH_MERGE_LISTS = 16,
  VRAG_DEBUG_TOPK_LAUNCH_MERGE_SCAN = 17
};
/* Empties the log. */
void vrag_debug_topk_launch_log_reset(void);
/* Copies the first min(cap, *count) entries to entries [cap][3] (nullable with cap = 0); *count = entries logged since the last
 * reset, *overflowed != 0 = launches were dropped behind the 4 096th. */
int vrag_debug_topk_launch_log_read(int32_t* entries, int32_t cap, int32_t* count, int32_t* overflowed);

/* Unit-test hook of the full-text index build and BM25 scoring stages alone (csrc/fulltext.hip, which the harness build compiles
 * with the hook in it), one stage per call, chosen by `op`.  Host buffers in; the hook calls the host launchers the product path
 * calls (scan_u32, radix_passes, rle_count + rle_emit, expand_parts, stats_launch, lookup_launch, score_launch), so the kernels and
 * grids are the product's; buffers marked "in / out" are copied to the device before the launches and back after them, so a
 * canary survives where a kernel must not write.  Per-record, per-posting, per-key, per-row, per-term and candidate outputs are
 * sized by a `*_buf` count >= the launch's count: what lies behind the launch's count is the caller's canary.
 * Refused by the hook before anything is launched, each with its own message: a null required pointer; a count below 0 or above
 * 2^22; a `*_buf` count below the count it covers; SORT with row_bits outside {0, 8, 16, 24, 32}; RLE with neither output form,
 * with only one of ukeys / pstart, or with post_buf or keys_buf below n; n_segs outside 1..4; a segment whose pstart does not
 * start at 0, decreases or does not end at its n_post, that has postings without keys, whose rows leave [row_lo, row_lo + n_rows)
 * or are not strictly ascending within a key, or whose row range does not follow its predecessor's (the first starts at 0); FOLD
 * with post_buf or keys_buf below the parts' postings; STATS / SCORE with segments reaching beyond n_rows; STATS with n_rows < 1,
 * k1 < 0, b outside [0, 1] or a corpus pair with tokens but no rows; LOOKUP with n_terms < 1; SCORE with n_rows < 1, nq outside
 * 1..65535, kk outside 1..64, q_indptr not from 0, decreasing or not ending at n_terms, a tu entry outside [-1, n_keys) (or not -1
 * for a segment beyond n_segs), allow_rows outside [0, n_rows], cand_buf below blocks * nq * kk.
 * Nothing the hook accepts reads or writes outside its buffers.  Index ranges per op (tile = 4 096):
 *   SCAN     ceil(n / tile) workgroups (one for n = 0) read in[i], i < n (guarded); the tile sums are the launcher's own scratch;
 *            write out[i], i <= n <= n_buf.
 *   SORT     ceil(n / tile) workgroups per digit pass read key / row / tf[i], i < n (guarded), write the other record set at
 *            pos < n (pos = a digit's scanned offset + rank: a permutation of 0..n-1); hist holds tiles * 256 words, offs one more.
 *            8 passes by key, row_bits / 8 passes by row; n <= 1 launches nothing.
 *   RLE      lane i < n reads key / row[i] and [i - 1] for i > 0; writes flags[i]; the scans write [0, n]; the scatter writes
 *            prow / ptf / ppos / pkey[p], p = pscan[i] < n_post <= n <= post_buf, ukeys / pstart[u], u = kscan[i] < n_keys <= n <=
 *            keys_buf; pstart[n_keys] is written by a copy; rle_tf reads ppos[p], ppos[p + 1] for p + 1 < n_post.
 *   FOLD     expand: lane p < n_post of a part reads pstart[u], u < n_keys, ukeys[u], prow / ptf[p]; writes records at + p below the
 *            sum of the parts' postings; then SORT by key and RLE (unit 0) over that many records.
 *   STATS    lane r < n_rows reads live[r / 32], dl[r]; writes kd[r], r < n_rows <= rows_buf; acc[0..1] by atomics, the corpus pair
 *            at acc[2..3]; df: wave u < n_keys reads pstart[u], pstart[u + 1], prow[p] with p below pstart[n_keys] = n_post, checked,
 *            live[prow[p] / 32] with prow[p] < n_rows, checked; writes df[u].
 *   LOOKUP   lane j < n_terms reads qkeys[j], keys[m] with m < n_keys and df[u], u < n_keys, of the segments below n_segs; writes
 *            tu[j * 4 + s], s < 4, and df_out[j]: j < n_terms <= terms_buf.
 *   SCORE    grid (ceil(n_rows / tile), nq).  Workgroup (blk, q) reads q_indptr[q], q_indptr[q + 1], tu / w[j] for j below
 *            q_indptr[nq] = n_terms, checked; pstart[u], pstart[u + 1] with u = tu < n_keys, checked; prow / ptf[p] inside that
 *            range; kd[row] and LDS acc[row - blk * tile] for rows of the block only (the bisection over strictly ascending rows,
 *            checked); live[row / 32], row < n_rows; allow[row / 32] only where row < allow_rows <= n_rows; bound[q]; writes
 *            cand[(blk * nq + q) * kk + i], i < kk: below blocks * nq * kk <= cand_buf.
 * Every device buffer of the hook, inputs and scratch included, is followed by 4 KiB of canary; the hook fails with VRAG_ERR_HIP
 * if a launch touched any.  (The tile sums inside scan_u32 are allocated by that launcher itself.) */
enum {
  VRAG_DEBUG_TEXT_SCAN = 0,
  VRAG_DEBUG_TEXT_SORT = 1,
  VRAG_DEBUG_TEXT_RLE = 2,
  VRAG_DEBUG_TEXT_FOLD = 3,
  VRAG_DEBUG_TEXT_STATS = 4,
  VRAG_DEBUG_TEXT_LOOKUP = 5,
  VRAG_DEBUG_TEXT_SCORE = 6
};
typedef struct vrag_debug_text_args {
  const uint32_t* in;        /* scan [n] */
  uint32_t* out;             /* in / out: scan [n_buf + 1] */
  uint64_t* key;             /* sort: in / out [n]; rle: in [n] */
  uint32_t* row;             /* the same */
  uint32_t* tf;              /* the same */
  uint64_t* ukeys;           /* in / out: rle (nullable: no segment form), fold [keys_buf] */
  uint32_t* pstart;          /* in / out: rle (with ukeys), fold [keys_buf + 1] */
  uint32_t* prow;            /* in / out: rle, fold [post_buf] */
  uint32_t* ptf;             /* in / out: rle, fold [post_buf] */
  uint64_t* pkey;            /* in / out: rle (nullable: no query form) [post_buf] */
  const uint64_t* seg_keys[4];     /* fold, stats, lookup, score: [seg_n_keys] per segment */
  const uint32_t* seg_pstart[4];   /* [seg_n_keys + 1] */
  const uint32_t* seg_prow[4];     /* [seg_n_post] */
  const uint32_t* seg_ptf[4];      /* [seg_n_post] */
  uint32_t* seg_df[4];       /* stats: in / out [seg_n_keys]; lookup: in */
  const uint32_t* dl;        /* stats [n_rows] */
  const uint32_t* live;      /* stats, score [ceil(n_rows / 32)] */
  const uint32_t* allow;     /* score [ceil(allow_rows / 32)], nullable */
  uint64_t* acc;             /* out: stats [2] = {N, sum dl} */
  float* kd;                 /* stats: in / out [rows_buf]; score: in [n_rows] */
  const uint64_t* qkeys;     /* lookup [n_terms] */
  int32_t* tu;               /* lookup: in / out [terms_buf][4]; score: in [n_terms][4] */
  int64_t* df_out;           /* in / out: lookup [terms_buf], nullable */
  const int64_t* q_indptr;   /* score [nq + 1] */
  const float* w;            /* score [n_terms] */
  const uint64_t* bound;     /* score [nq], nullable */
  uint64_t* cand;            /* in / out: score [cand_buf] */
  int64_t seg_n_keys[4], seg_n_post[4], seg_row_lo[4], seg_n_rows[4];
  int64_t n, n_buf;          /* scan, sort, rle: elements / records; n_buf: scan only */
  int64_t post_buf, keys_buf;
  int64_t n_rows, rows_buf;
  int64_t allow_rows;
  int64_t n_terms, terms_buf;
  int64_t cand_buf;
  int64_t corpus_n, corpus_sum_dl;   /* stats: the corpus-wide pair K_d reads; corpus_n = 0 = none */
  int64_t n_post, n_keys;    /* out: rle, fold */
  int32_t op;
  int32_t by_row, row_bits;  /* sort */
  int32_t unit;              /* rle */
  int32_t n_segs;
  int32_t nq, kk;            /* score */
  float k1, b;               /* stats */
  float k1p1;                /* score: k1 + 1 */
} vrag_debug_text_args;
int vrag_debug_text_run(vrag_debug_text_args* args, int32_t device);

/* The whole state of a text index created through THIS library's vrag_text_index_* functions, statistics refreshed first as a
 * search refreshes them.  Two calls: with with_data = 0 only the sizes are written (n_segs, n_rows, n_live, sum_dl and the four
 * per-segment counts); with with_data != 0 the caller passes the sizes back as it got them (refused if the index changed between
 * the calls) and every non-null pointer receives its array: per segment keys [n_keys], pstart [n_keys + 1], prow, ptf [n_post],
 * df [n_keys]; dl, kd [n_rows]; live [ceil(n_rows / 32)] (the device's bitmap, as the kernels read it). */
typedef struct vrag_debug_text_index_state {
  uint64_t* keys[2];
  uint32_t* pstart[2];
  uint32_t* prow[2];
  uint32_t* ptf[2];
  uint32_t* df[2];
  uint32_t* dl;
  float* kd;
  uint32_t* live;
  int64_t row_lo[2], seg_rows[2], n_keys[2], n_post[2];
  int64_t n_rows, n_live, sum_dl;
  int32_t n_segs;
  int32_t with_data;
} vrag_debug_text_index_state;
struct vrag_text_index;
int vrag_debug_text_index_read(struct vrag_text_index* ix, vrag_debug_text_index_state* state);

/* Self-test of the hooks' device staging (csrc/debug_bufs.h): stages "a" (in, 64 bytes), "b" (in / out, 100 bytes and 28 pad
 * bytes) and "c" (scratch, empty), launches nothing, and returns what the hooks' common canary check returns.  touch 0: nothing
 * more, VRAG_OK with b copied back as it went in; 1 / 2: a host-issued one-byte hipMemset on the first / last canary byte of b,
 * VRAG_ERR_HIP naming b; 3: on the last pad byte of b, VRAG_OK.  Any other touch is VRAG_ERR_INVALID before the device check. */
int vrag_debug_canary_selftest(int32_t touch, int32_t device);

/* Unit-test hook of span selection (csrc/spans.hip): vrag_encoder_read_token_spans with a host array of packed logits
 * [n_tokens, 2] in place of an engine -- win_first[w] indexes its rows -- through the same checks and the same kernel. */
int vrag_debug_token_spans(const float* logits, int64_t n_tokens, const int32_t* win_job, const int32_t* win_a, const int32_t* win_b,
                           const int32_t* win_first, int32_t n_windows, const int64_t* job_off, const int32_t* offsets, int32_t n_jobs,
                           float tau, int32_t min_span_chars, int32_t merge_gap_chars, int32_t cap_per_job, int32_t* counts,
                           int32_t* spans, int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* VRAG_AMD_DEBUG_H */
