/* vrag_amd.h -- C ABI of the MI355X (gfx950) hot-path library `libvrag_amd.so`.
 *
 * The reference (KRLabsOrg/verbatim-rag) is pure Python and has no FFI of its own; these
 * entry points are what a Python binding (ctypes) calls in place of the
 * third-party arithmetic the reference delegates to:
 *
 *   vrag_encoder_*         <- transformers ModernBertModel.forward, called from
 *                             packages/core/verbatim_core/extractor_models/model.py:75
 *                             (QAModel.forward) and extractors.py:260-268 (legacy qa_model path)
 *   vrag_encoder_*qa*      <- QAModel sentence head, extractor_models/model.py:82-113
 *   vrag_encoder_*token*   <- ModernBertForTokenClassification head used by the v2 highlighter
 *                             `.process()` (extractors.py:213-221)
 *   vrag_encoder_*splade*  <- SparseEncoder.encode (MLM logits -> max_s log1p(relu))
 *                             verbatim_rag/embedding_providers.py:127-166
 *   vrag_encoder_*pool*    <- SentenceTransformer.encode (pool + L2 normalise)
 *                             verbatim_rag/embedding_providers.py:73-77
 *
 * Conventions: every function returns 0 (VRAG_OK) or a negative status; the message for the
 * last failure on the calling thread is vrag_last_error().  Handles are thread-safe (one
 * internal mutex per handle; callers may hit one handle from asyncio.to_thread workers like
 * extractors.py:48-54 does).  `stream` arguments are a hipStream_t passed as void* (NULL = the
 * handle's own stream).  load_* = host->device upload, run_* = device kernels only,
 * read_* = device->host (synchronises the stream).  No callbacks, no global state.
 */
#ifndef VRAG_AMD_H
#define VRAG_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VRAG_OK 0
#define VRAG_ERR_INVALID (-1) /* bad argument / shape / state */
#define VRAG_ERR_HIP (-2)     /* a HIP runtime call failed */
#define VRAG_ERR_CAPACITY (-3)/* batch does not fit the workspace the handle was created with */
#define VRAG_ERR_NO_DEVICE (-4)

#define VRAG_ABI_VERSION 6

/* MFMA operand type of an encoder handle.  bf16: fp32's exponent range (safe for any checkpoint), 8 significant bits --
 * sentence logits within 3e-4 of the fp32 reference.  fp16: 11 significant bits at the same matrix-core rate, values
 * saturate at +-65504 -- what the per-token logits of the v2 highlighter need to stay within 1e-3. */
#define VRAG_OPERAND_BF16 0
#define VRAG_OPERAND_F16 1

typedef struct vrag_encoder vrag_encoder;

typedef struct vrag_encoder_config {
  int32_t vocab_size;
  int32_t hidden_size;         /* multiple of 128, <= 1024; head_dim is fixed at 64 */
  int32_t num_layers;
  int32_t num_heads;           /* hidden_size / 64 */
  int32_t intermediate_size;   /* multiple of 64 */
  int32_t global_every;        /* layer l is global attention iff l % global_every == 0 */
  int32_t sliding_window;      /* local layers keep |i-j| <= sliding_window (ModernBERT: 64) */
  float rope_theta_global;     /* 160000 */
  float rope_theta_local;      /* 10000 */
  float norm_eps;              /* 1e-5 */
  int32_t pad_token_id;
  int32_t max_seq_len;         /* longest sequence (RoPE table rows) */
  int32_t max_tokens;          /* workspace capacity: packed tokens per batch */
  int32_t max_seqs;            /* sequences per batch */
  int32_t max_ranges;          /* sentence / pooling ranges per batch */
  int32_t micro_batch_tokens;  /* 0 = whole batch per kernel; else split (cache blocking) */
  int32_t device;              /* HIP device ordinal */
  int32_t operand_dtype;       /* VRAG_OPERAND_BF16 (default) or VRAG_OPERAND_F16: type of the MFMA operands (weights,
                                  LayerNorm outputs, q/k/v/P, GeGLU output); accumulation, the residual stream, LayerNorm,
                                  softmax, RoPE and the heads are fp32 either way */
} vrag_encoder_config;

/* Host fp32 arrays, HF layouts ([out,in] row-major for nn.Linear weights). Per-layer arrays
 * have num_layers entries; attn_norm[0] is ignored (layer 0 has no attn_norm). */
typedef struct vrag_encoder_weights {
  const float* tok_embeddings;   /* [V, H]   embeddings.tok_embeddings.weight */
  const float* emb_norm;         /* [H]      embeddings.norm.weight */
  const float* const* attn_norm; /* [L][H]   layers.i.attn_norm.weight */
  const float* const* wqkv;      /* [L][3H,H] layers.i.attn.Wqkv.weight */
  const float* const* wo;        /* [L][H,H] layers.i.attn.Wo.weight */
  const float* const* mlp_norm;  /* [L][H]   layers.i.mlp_norm.weight */
  const float* const* wi;        /* [L][2I,H] layers.i.mlp.Wi.weight */
  const float* const* wo_mlp;    /* [L][H,I] layers.i.mlp.Wo.weight */
  const float* final_norm;       /* [H]      final_norm.weight */
} vrag_encoder_weights;

/* BERT-family encoders (BERT, DistilBERT: post-LN, biased linears, learned absolute positions, GELU MLP) --
 * the checkpoints the reference names for its embedding providers (`naver/splade-v3`,
 * `opensearch-neural-sparse-encoding-doc-v2-distill`: verbatim_rag/embedding_providers.py:120, README.md:122-125;
 * BAAI/bge-base: embedding_providers.py:55).  Replaces transformers BertModel / DistilBertModel.forward
 * (models/bert/modeling_bert.py, models/distilbert/modeling_distilbert.py) underneath
 * sentence-transformers' SparseEncoder / SentenceTransformer .encode.  head_dim must be 64 or 32 (32, e.g.
 * all-MiniLM-L6-v2 -- embedding_providers.py:55 -- runs zero-padded on the head_dim-64 kernels). */
typedef struct vrag_bert_config {
  int32_t vocab_size;
  int32_t hidden_size;              /* multiple of 128, <= 1024 */
  int32_t num_layers;
  int32_t num_heads;                /* hidden_size / 64 or hidden_size / 32 */
  int32_t intermediate_size;        /* multiple of 128 */
  int32_t max_position_embeddings;  /* rows of position_embeddings */
  float norm_eps;                   /* 1e-12 */
  int32_t pad_token_id;
  int32_t max_seq_len;              /* <= max_position_embeddings */
  int32_t max_tokens;
  int32_t max_seqs;
  int32_t max_ranges;
  int32_t micro_batch_tokens;
  int32_t device;
  int32_t operand_dtype;            /* VRAG_OPERAND_BF16 / VRAG_OPERAND_F16 */
} vrag_bert_config;

/* Host fp32 arrays, HF layouts. wqkv/bqkv are the query, key, value matrices / biases concatenated
 * along the output dimension ([3H,H] / [3H]).  DistilBERT: token_type_row = NULL. */
typedef struct vrag_bert_weights {
  const float* word_embeddings;      /* [V, H] */
  const float* position_embeddings;  /* [P, H] */
  const float* token_type_row;       /* [H] = token_type_embeddings[0] (single-segment inputs) or NULL */
  const float* emb_norm_w;           /* [H] embeddings.LayerNorm.weight */
  const float* emb_norm_b;           /* [H] */
  const float* const* wqkv;          /* [L][3H,H] */
  const float* const* bqkv;          /* [L][3H] */
  const float* const* wo;            /* [L][H,H]  attention.output.dense / out_lin */
  const float* const* bo;            /* [L][H] */
  const float* const* attn_norm_w;   /* [L][H]    attention.output.LayerNorm / sa_layer_norm */
  const float* const* attn_norm_b;   /* [L][H] */
  const float* const* w1;            /* [L][I,H]  intermediate.dense / ffn.lin1 */
  const float* const* b1;            /* [L][I] */
  const float* const* w2;            /* [L][H,I]  output.dense / ffn.lin2 */
  const float* const* b2;            /* [L][H] */
  const float* const* out_norm_w;    /* [L][H]    output.LayerNorm / output_layer_norm */
  const float* const* out_norm_b;    /* [L][H] */
} vrag_bert_weights;

const char* vrag_last_error(void);
int vrag_abi_version(void);
/* Number of visible HIP devices (0 when there is no GPU); never fails. */
int vrag_device_count(void);

int vrag_encoder_create(const vrag_encoder_config* cfg, const vrag_encoder_weights* w, vrag_encoder** out);
/* Same opaque handle type: load_batch / run / load_ranges / run_pool / run_splade / read_* work on it
 * unchanged (there is no final LayerNorm to apply; pooling averages the hidden states directly). */
int vrag_bert_encoder_create(const vrag_bert_config* cfg, const vrag_bert_weights* w, vrag_encoder** out);
void vrag_encoder_destroy(vrag_encoder* enc);

/* Heads (host fp32, HF layouts). */
int vrag_encoder_set_qa_head(vrag_encoder* enc, const float* w /*[labels,H]*/, const float* b /*[labels]*/,
                             int32_t num_labels);
int vrag_encoder_set_token_head(vrag_encoder* enc, const float* dense_w /*[H,H]*/, const float* norm_w /*[H]*/,
                                const float* cls_w /*[labels,H]*/, const float* cls_b /*[labels]*/,
                                int32_t num_labels);
/* decoder_w == NULL ties the decoder to tok_embeddings (ModernBertForMaskedLM). */
int vrag_encoder_set_mlm_head(vrag_encoder* enc, const float* dense_w /*[H,H]*/, const float* norm_w /*[H]*/,
                              const float* decoder_w /*[V,H] or NULL*/, const float* decoder_b /*[V]*/);

/* MLM head with biases (BertForMaskedLM cls.predictions / DistilBertForMaskedLM vocab_transform,
 * vocab_layer_norm, vocab_projector): logits = decoder(LN(gelu(dense(h) + dense_b)) * norm_w + norm_b) + decoder_b.
 * dense_b / norm_b may be NULL (ModernBERT); decoder_w == NULL ties the decoder to the word embeddings. */
int vrag_encoder_set_mlm_head_ex(vrag_encoder* enc, const float* dense_w /*[H,H]*/, const float* dense_b /*[H]*/,
                                 const float* norm_w /*[H]*/, const float* norm_b /*[H]*/,
                                 const float* decoder_w /*[V,H] or NULL*/, const float* decoder_b /*[V]*/);

/* Operand precision of the MLM / SPLADE head GEMMs; takes effect at the NEXT vrag_encoder_set_mlm_head* (which may be called
 * again on a handle: the previous head's images are released and rebuilt in the chosen form): split_operands != 0
 * (the default) carries activations and weights as (value, remainder) pairs of the operand type -- the dense layer as
 * three accumulating GEMMs, the decoder as one GEMM over K = 3H -- so that every SPLADE weight max_s log1p(relu(logit))
 * stays within 2e-3 of the fp32 arithmetic of SparseEncoder.encode (embedding_providers.py:127-166; nothing averages
 * operand rounding away under a max); 0 = plain 16-bit operands: a third of the decoder work, weights within ~1e-2. */
int vrag_encoder_set_head_precision(vrag_encoder* enc, int32_t split_operands);

/* Sentence-pair inputs (cross-encoder reranking: sentence-transformers CrossEncoder over
 * BertForSequenceClassification, verbatim_rag/rerankers.py:109-134).  BERT-family handles only.
 * set_token_types: the whole token_type_embeddings table [n_types, H] (the creator only takes row 0).
 * load_token_types: per-token segment ids of the batch loaded last (concatenation order of load_batch);
 *   stays in effect until the next load_batch.
 * set_pair_head / run_pair_head: logits[s] = cls_w . tanh(pooler_w . h[first token of s] + pooler_b) + cls_b
 *   (BertPooler + classifier, transformers models/bert/modeling_bert.py:451-463,1115-1119). */
int vrag_encoder_set_token_types(vrag_encoder* enc, const float* table /*[n_types, H]*/, int32_t n_types);
int vrag_encoder_load_token_types(vrag_encoder* enc, const int32_t* types /*[n_tokens]*/, void* stream);
int vrag_encoder_set_pair_head(vrag_encoder* enc, const float* pooler_w /*[H,H]*/, const float* pooler_b /*[H]*/,
                               const float* cls_w /*[labels,H]*/, const float* cls_b /*[labels]*/, int32_t num_labels);
int vrag_encoder_run_pair_head(vrag_encoder* enc, void* stream);
int vrag_encoder_read_pair_logits(vrag_encoder* enc, float* logits /*[n_seqs, labels]*/, void* stream);

/* Sequence-classification head of ModernBERT handles (ModernBertForSequenceClassification: the cross-encoder rerankers of
 * the ModernBERT family, e.g. gte-reranker-modernbert-base; transformers models/modernbert/modeling_modernbert.py,
 * ModernBertPredictionHead + classifier).  Per sequence s of the batch loaded last:
 *   p = final_norm(h)[first token of s]                      pooling 0 (classifier_pooling "cls")
 *     = mean of final_norm(h) over every token of s          pooling 1 ("mean"; [CLS] and [SEP]s included)
 *   logits[s] = cls_w . LayerNorm(gelu_erf(dense_w . p + dense_b); norm_w, norm_b) + cls_b
 * dense_b / norm_b may be NULL (classifier_bias / norm_bias false); labels 1..64; all arithmetic fp32.  BERT-family
 * handles return VRAG_ERR_INVALID (their cross-encoder head is set_pair_head).  Setting the head again replaces it. */
int vrag_encoder_set_seq_head(vrag_encoder* enc, const float* dense_w /*[H,H]*/, const float* dense_b /*[H] or NULL*/,
                              const float* norm_w /*[H]*/, const float* norm_b /*[H] or NULL*/,
                              const float* cls_w /*[labels,H]*/, const float* cls_b /*[labels]*/,
                              int32_t num_labels, int32_t pooling /*0 = cls, 1 = mean*/);
int vrag_encoder_run_seq_head(vrag_encoder* enc, void* stream);
int vrag_encoder_read_seq_logits(vrag_encoder* enc, float* logits /*[n_seqs, labels]*/, void* stream);

/* Packed batch: `ids` is the plain concatenation of n_seqs unpadded sequences of lengths
 * seq_lens[i] (positions restart at 0 per sequence, like the reference's B=1 forward). */
int vrag_encoder_load_batch(vrag_encoder* enc, const int32_t* ids, const int32_t* seq_lens, int32_t n_seqs,
                            void* stream);
/* Embedding + all encoder layers; leaves the fp32 residual stream on the device. */
int vrag_encoder_run(vrag_encoder* enc, void* stream);
/* Same, stopping after `n_layers` layers (debug / per-layer parity). */
int vrag_encoder_run_layers(vrag_encoder* enc, int32_t n_layers, void* stream);

/* Inclusive token ranges inside sequences (sentence boundaries or pooling spans). */
int vrag_encoder_load_ranges(vrag_encoder* enc, const int32_t* seq_idx, const int32_t* start, const int32_t* end,
                             int32_t n_ranges, void* stream);
/* final LayerNorm + mean over each range + Linear(H, labels)  -> device logits [n_ranges, labels] */
int vrag_encoder_run_qa_head(vrag_encoder* enc, void* stream);
int vrag_encoder_read_qa_logits(vrag_encoder* enc, float* logits /*[n_ranges, labels]*/, void* stream);
/* final LayerNorm + mean over each range (+ L2 normalise) -> [n_ranges, H] */
int vrag_encoder_run_pool(vrag_encoder* enc, int32_t normalize, void* stream);
int vrag_encoder_read_pool(vrag_encoder* enc, float* out /*[n_ranges, H]*/, void* stream);

/* Token-classification head: logits for every packed token, in the caller's concatenation order. */
int vrag_encoder_run_token_head(vrag_encoder* enc, void* stream);
int vrag_encoder_read_token_logits(vrag_encoder* enc, float* logits /*[n_tokens, labels]*/, void* stream);
/* Span selection of the v2 highlighter over the token logits that vrag_encoder_run_token_head left in the workspace (2-label
 * heads only, else VRAG_ERR_INVALID): the logits stay on the device, only (start, end) character spans come back.
 *   A JOB is one (question, chunk) pair: its context tokens t = 0 .. job_off[j+1] - job_off[j] - 1 have the character offsets
 *   offsets[job_off[j] + t] = (start, end).  WINDOW w of job win_job[w] holds the context tokens [win_a[w], win_b[w]) of that job
 *   at the packed tokens win_first[w] ... (the caller's concatenation order, as read_token_logits returns them; a window lies
 *   inside one sequence).  Windows are listed job by job, and within a job ascend in win_a and in win_b.
 *   For a window token m = logit[1] - logit[0] (one fp32 subtraction); for a context token M = the maximum of m over the windows
 *   that cover it.  The token is HOT iff M > tau -- the caller passes tau = log(thr / (1 - thr)) for `softmax(logits)[1] > thr`;
 *   a covering window with a NaN m or with logit[1] = +inf (rows the host's softmax turns into NaN), or no covering window,
 *   makes it cold.  Tokens with end <= start are skipped: they neither
 *   extend nor close a run.  A maximal sequence of hot tokens that no cold token interrupts is the run [first start, max end);
 *   a run joins the span in front of it while run.start - span.end <= merge_gap_chars (the difference may be <= 0 when tokens
 *   share a character); a finished span with end - start < min_span_chars is dropped.
 * counts[j] = spans of job j, always exact; spans[j][i] = (start, end) for i < counts[j], in text order.  When a count exceeds
 * cap_per_job the call returns VRAG_ERR_CAPACITY with counts filled in and spans unspecified; the caller reads again with room.
 * Host pointers; the call synchronises the stream. */
int vrag_encoder_read_token_spans(vrag_encoder* enc, const int32_t* win_job /*[n_windows]*/, const int32_t* win_a, const int32_t* win_b,
                                  const int32_t* win_first, int32_t n_windows, const int64_t* job_off /*[n_jobs+1]*/,
                                  const int32_t* offsets /*[job_off[n_jobs], 2]*/, int32_t n_jobs, float tau, int32_t min_span_chars,
                                  int32_t merge_gap_chars, int32_t cap_per_job, int32_t* counts /*[n_jobs]*/,
                                  int32_t* spans /*[n_jobs, cap_per_job, 2]*/, void* stream);

/* SPLADE head: rows[s][v] = max over the tokens of sequence s of log1p(relu(mlm_logit)). */
int vrag_encoder_run_splade(vrag_encoder* enc, void* stream);
int vrag_encoder_read_splade(vrag_encoder* enc, float* rows /*[n_seqs, V]*/, void* stream);
/* The same rows compacted on the device: for sequence s, counts[s] entries (vocabulary index ascending, weight >
 * threshold; threshold 0 = every non-zero, the `embed_batch` rule of embedding_providers.py:161-163; 1e-6 = the
 * `embed_text` rule :141-145) at indices/values[s*cap_per_seq ...].  counts[] is always exact; if any count exceeds
 * cap_per_seq the call returns VRAG_ERR_CAPACITY (nothing is truncated silently) and the caller re-reads with a
 * larger capacity or falls back to vrag_encoder_read_splade. */
int vrag_encoder_read_splade_sparse(vrag_encoder* enc, float threshold, int32_t cap_per_seq, int32_t* counts /*[n_seqs]*/,
                                    int32_t* indices /*[n_seqs, cap_per_seq]*/, float* values /*[n_seqs, cap_per_seq]*/,
                                    void* stream);

/* Debug / parity: final-LayerNorm hidden states (or the raw residual stream), caller order. */
int vrag_encoder_read_hidden(vrag_encoder* enc, int32_t apply_final_norm, float* out /*[n_tokens, H]*/,
                             void* stream);

/* One-call convenience for the extractor path: load_batch + load_ranges + run + run_qa_head + read. */
int vrag_encoder_extract_qa(vrag_encoder* enc, const int32_t* ids, const int32_t* seq_lens, int32_t n_seqs,
                            const int32_t* rng_seq, const int32_t* rng_start, const int32_t* rng_end,
                            int32_t n_ranges, float* logits);

/* Launch-bound batches (at most 8 192 packed rows in one micro-batch -- a query's handful of chunks, the reference's call
 * shape verbatim_rag/core.py:238-255 with k = 5): the layer schedule of a (rows, attention blocks, layers) geometry is
 * captured into a HIP graph the second time it is seen and replayed afterwards; results are bit-identical to the eager
 * launches (same kernels, same arguments).  enable: 0 = eager only, > 0 = row limit for graph replay, < 0 = leave as is;
 * *replays = graph launches so far, *cached = instantiated graphs (either may be NULL).  VRAG_GRAPHS=0 disables at create. */
int vrag_encoder_graph_stats(vrag_encoder* enc, int32_t enable, int64_t* replays, int32_t* cached);

/* fp16 operands (VRAG_OPERAND_F16) saturate at +-65504 instead of overflowing.  *saturated = 1 if any fp32 -> fp16
 * operand conversion of this handle (weights at load time, LayerNorm-fold copies, q / k / v, GeGLU outputs, attention
 * outputs) has met a value outside fp16's range or NaN since the last reset: the logits computed meanwhile are not to be trusted -- re-run with
 * VRAG_OPERAND_BF16 (checkpoints with activation outliers beyond fp16's range).  The flag is per handle: other handles
 * on the same device neither see nor clear it.  Synchronises the device. */
int vrag_encoder_f16_saturated(vrag_encoder* enc, int32_t reset, int32_t* saturated);

/* Per-kernel-class timing with HIP events recorded on the launch stream.
 * classes: see VRAG_PROF_* ; ms[i] = summed event time, launches[i] = launch count since reset. */
#define VRAG_PROF_EMBED 0
#define VRAG_PROF_LAYERNORM 1
#define VRAG_PROF_GEMM_QKV 2
#define VRAG_PROF_ATTN_GLOBAL 3
#define VRAG_PROF_ATTN_LOCAL 4
#define VRAG_PROF_GEMM_WO 5
#define VRAG_PROF_GEMM_WI 6
#define VRAG_PROF_GEMM_WO_MLP 7
#define VRAG_PROF_HEAD 8
#define VRAG_PROF_QKV_ATTN_GLOBAL 9 /* fused Wqkv + RoPE + attention kernel (csrc/qkv_attn.hip), global layers */
#define VRAG_PROF_QKV_ATTN_LOCAL 10 /* the same, banded layers */
#define VRAG_PROF_COUNT 11
/* Micro-batches (cfg.micro_batch_tokens) are issued on 2 internal streams by default so that the
 * HBM-bound kernels of one overlap the MFMA-bound kernels of the other; 1 serialises them. */
int vrag_encoder_set_concurrency(vrag_encoder* enc, int32_t n_streams);
/* enabled: 0 = off, 1 = a HIP event pair around every launch, n > 1 = around every n-th launch of each class (the totals
 * vrag_encoder_read_profile returns are then the timed launches' mean x the launches issued). */
int vrag_encoder_set_profiling(vrag_encoder* enc, int32_t enabled);
/* Launch-bound configuration: GEMMs over at most `rows` token rows (a query's handful of chunks) use 128x128 / 64x64 tiles with
 * deeper LDS rings and a K split over waves instead of the 256x256 throughput tiles; 0 disables it, a negative value only
 * reads.  Process-wide; returns the threshold in effect (default 8192).  The two configurations sum fp32 partial products in
 * different orders, so tests pin one or the other through this call. */
int vrag_set_small_batch_rows(int32_t rows);
int vrag_encoder_read_profile(vrag_encoder* enc, float* ms /*[VRAG_PROF_COUNT]*/,
                              int64_t* launches /*[VRAG_PROF_COUNT]*/, int32_t reset);

/* ------------------------------------------------------------------------------------------
 * Exact dot-product top-k (what the reference delegates to Milvus:
 * verbatim_rag/vector_stores/milvus_base.py:239-259, metric types milvus_local.py:109-129).
 * Order: (score desc, id asc), ties included.  Zeros of either sign tie; the sign of a returned zero is unspecified (a tree-shaped
 * sum gives +0 where the sequential chain gives -0; every list builder, vrag_topk_merge and the SQ8, sparse, full-text and IVF
 * lists rank with the same keys and follow the same rule).  fp32 denormals are kept on every route, matrix-core kernels
 * included: a denormal score is returned bit for bit and ranks by its value (tests/test_topk_special_values_gpu.py).
 * Missing hits: id = -1, score = -inf.  1 <= k <= 1024 for the search
 * calls (Milvus' `limit`, milvus_base.py:244-277: the reference asks for top_k or 2*top_k): lists of up to 64 come from
 * one device pass, longer ones as exact pages of 64 (page p+1 admits only keys below the last key of page p) on the
 * scalar kernels with fp32 queries; `*_run_resident` re-runs a single pass (k <= 64).
 * Dense rows are stored bf16 (dtype 0) or fp32 (dtype 1); COSINE == IP on rows/queries the caller
 * L2-normalised.  ids are row numbers in insertion order (the caller adds its shard base).
 * dtype 2 = fp32 rows (every result bit-identical to dtype 1: scores are the sequential fp32 fmaf chain over the fp32 rows)
 * plus a bf16 prefilter image of them (+50 % memory): vrag_dense_index_search, for k <= 16, ranks the image first, proves
 * from the image's MEASURED error bound that its candidates contain the exact top-k (else the full fp32 scan answers that
 * query; the bound holds for every finite fp32 row -- the norms behind it are measured on the row scaled by a power of two, so
 * rows of magnitude 2^-75 or 2^+66 keep the route, and a row whose norm is beyond fp32 sends every query to the full scan)
 * and re-scores them exactly -- half the bytes for a small batch, one read of the shard per batch instead of one per 32
 * queries.  Round 6 routes every batch through it: one to four queries share ONE pass over the image that collects every row
 * within twice the bound of an entry threshold (more than 4096 of them = the full scan); 5 .. 256 queries take the same idea
 * on the tiled score GEMM (thresholds from 65 536 rows -- a sample of the shard's tiles --, one appending pass, exact re-score of the lists); larger
 * batches rank the image for 64 candidates per query with a sufficiency test.  vrag_dense_index_search_device takes the same
 * routes with the full scan enqueued behind per-query flags instead of a host decision.
 * bf16 rows (dtype 0): one query streams the shard on the scalar kernel; two or more take the tiled score GEMM (shards of >= 4 096
 * rows, dim % 64 == 0) -- the shard read once per batch -- whose scores are exact on bf16-representable data and otherwise differ
 * from the fp32 chain by summation order.
 * Dense rows and queries are expected to be finite: a NaN score is kept by the pass kernels (it becomes a key like any other score) and
 * dropped by the tiled search's epilogue (no comparison with the entry threshold holds), so the routes disagree on such rows.
 * create: dim % 8 == 0, dim <= 4096, 0 < capacity < 2^32 - 1 rows.  The suite runs every dense route, the filtered search, the IVF
 * overlay and both id forms of vrag_dense_index_search_device on shards that cross 2^32 elements (2^33 / 2^34 bytes: 1 052 929 x 4096
 * and 5 596 929 x 768 rows) and row id 2^24 (16 781 569 x 64 rows, 513 blocks of the bitmap compaction): tests/test_scale_gpu.py.
 */
typedef struct vrag_dense_index vrag_dense_index;
int vrag_dense_index_create(int32_t dim, int64_t capacity, int32_t dtype, int32_t device, vrag_dense_index** out);
void vrag_dense_index_destroy(vrag_dense_index* ix);
int64_t vrag_dense_index_size(vrag_dense_index* ix);
int vrag_dense_index_add(vrag_dense_index* ix, const float* rows /*[n,dim] host fp32*/, int64_t n);
/* The same from DEVICE memory (rows: fp32 [n, dim] on the index's device, e.g. vrag_encoder pooled embeddings that never
 * visited the host): converted / copied on `stream` (NULL = the legacy default stream); returns when the rows are in place. */
int vrag_dense_index_add_device(vrag_dense_index* ix, const float* rows /*[n,dim] device fp32*/, int64_t n, void* stream);
int vrag_dense_index_search(vrag_dense_index* ix, const float* queries /*[nq,dim] host*/, int32_t nq, int32_t k,
                            float* scores /*[nq,k]*/, int64_t* ids /*[nq,k]*/, void* stream);
/* Re-runs the kernels of the last search on the device-resident queries (no copies, no sync). */
int vrag_dense_index_run_resident(vrag_dense_index* ix, int32_t nq, int32_t k, void* stream);
/* Compaction: drops rows in place.  `keep_words` (host) holds one bit per row, bit r % 32 of word r / 32 as in the `allow`
 * masks: set = the row stays.  The rows that stay keep their relative order and become rows 0 .. new_size - 1; capacity is
 * unchanged, so the reclaimed room takes appends again.  The rows -- and the bf16 prefilter image of a dtype 2 index -- are moved
 * where they lie in HBM: nothing is re-uploaded and no second copy of the array is made.  Rows travel in waves of at most
 * VRAG_COMPACT_BOUNCE_BYTES (csrc/compact.h) through a bounce buffer in the handle's scratch (allocated by the first compaction
 * that moves a row): one launch gathers a wave, the next stores it, and the order of the moves is the stream's alone -- no
 * workgroup waits for another.  The rows in front of the first cleared bit are not touched; a bitmap without a cleared bit
 * launches nothing.  n_keep must equal the index's size: VRAG_ERR_INVALID otherwise, before anything is launched.  Runs under
 * the handle's lock; the new size is published (and returned in *new_size) after the stream has drained.  Every search
 * afterwards returns what an index freshly built from the kept rows returns, bit for bit: the prefilter's norm and error bounds
 * are left as they are -- still upper bounds, and no result depends on how tight they are.  The resident queries and lists of
 * an earlier search are invalidated: vrag_dense_index_run_resident is VRAG_ERR_INVALID until the next search.  An IVF overlay
 * over the index is renumbered with vrag_ivf_index_remap and the same bitmap, after this call. */
int vrag_dense_index_compact(vrag_dense_index* ix, const uint32_t* keep_words /*host*/, int64_t n_keep, int64_t* new_size);
/* Rows [first_row, first_row + n) as fp32 (bf16 rows widened: exact); rows beyond the size are VRAG_ERR_INVALID. */
int vrag_dense_index_read(vrag_dense_index* ix, int64_t first_row, int64_t n, float* out /*[n,dim] host*/);
/* The same search (k <= 64) with the result lists left in DEVICE memory -- what a rank contributes to the cross-GPU
 * exchange (serves verbatim_rag/vector_stores/milvus_base.py:239-259 on a row-sharded corpus):
 * out_ids[q][j] = row_map[row] when `row_map` (device int64[n_map], the caller's local row -> global row table) is
 * given -- rows at or beyond n_map become -1 -- else id_base + row; missing hits -1 / -inf.  Queries are host memory
 * (the call returns once they have been uploaded); the kernels are only enqueued on `stream`: no synchronisation and no
 * device->host copy.  `stream` = NULL means the legacy default stream here (not the handle's own stream): whatever
 * consumes the lists next -- the all-gather -- is ordered against the stream the caller named. */
int vrag_dense_index_search_device(vrag_dense_index* ix, const float* queries /*[nq,dim] host*/, int32_t nq, int32_t k,
                                   const int64_t* row_map /*device or NULL*/, int64_t n_map, int64_t id_base,
                                   float* out_scores /*[nq,k] device*/, int64_t* out_ids /*[nq,k] device*/, void* stream);
/* Filtered search over the RESIDENT rows (the reference's `filter` / delete semantics, index.py:723-739: Milvus filters before
 * it searches): the top-k of exactly the rows r < min(n_allow, size) whose bit is set in `allow` (host words, bit r % 32 of word
 * r / 32).  Rows at or beyond n_allow are excluded, so a mask built before a concurrent append stays valid.  Order, missing-hit
 * encoding, 1 <= k <= 1024 and the exact pages of 64 are those of vrag_dense_index_search.  Scores are the sequential chain
 * acc = fmaf(x[c], q[c], acc), c ascending, bit for bit on every index type: over the fp32 row (dtype 1 and 2 -- the bf16 image of
 * dtype 2 is never consulted) or the bf16 row widened to fp32 (dtype 0), against the fp32 query.  The bitmap is compacted on the
 * device into the ascending list of passing rows and the chains run over that list only: the cost follows the passing rows, not
 * the shard.  n_allow == 0 or a mask without a set bit returns -1 / -inf lists without a launch; a null `allow` with n_allow > 0,
 * k out of range or nq <= 0 is VRAG_ERR_INVALID before anything is launched or allocated.  Bitmap and row list live in the
 * handle's scratch; unfiltered searches on the handle are not affected (run_resident afterwards re-runs THESE queries). */
int vrag_dense_index_search_filtered(vrag_dense_index* ix, const float* queries /*[nq,dim] host*/, int32_t nq, int32_t k,
                                     const uint32_t* allow /*host, bit r%32 of word r/32*/, int64_t n_allow,
                                     float* scores /*[nq,k]*/, int64_t* ids /*[nq,k]*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * Grouping search over a dense index (csrc/grouped.hip; Milvus' group_by_field / group_size, which the reference's stores can pass
 * in search_params).  The semantics are this library's own and are not pinned against Milvus.
 * A vrag_group_column holds one int32 group code >= 0 per row of an index it does not own, in HBM, extended by appends (row r of
 * the column describes row r of the index); it remembers the largest code + 1 (`n_codes`) and owns the scratch, the stream and the
 * lock of the searches made with it.  Codes should be dense: a search keeps 8 * group_size * n_codes bytes of keys per query.
 *   search_grouped   Rows considered: r < min(size of the index, size of the column) -- with a bitmap (`allow`, host words, bit r % 32
 *                    of word r / 32, as in vrag_dense_index_search_filtered) r < n_allow as well and the bit set; allow == NULL (then
 *                    n_allow must be 0) means every such row.  Rank those rows by (score desc, row asc); scores are the sequential
 *                    chain acc = fmaf(x[c], q[c], acc), c ascending, of vrag_dense_index_search_filtered bit for bit (fp32 row, or
 *                    the bf16 row widened), zeros of either sign tie.  A group's rank is that of its best row.  Per query:
 *                    groups[g] = the code of the g-th group in that order, scores / ids [g][0 .. group_size) = that group's first
 *                    group_size rows in that order.  Missing entries (a group with fewer rows, fewer groups than n_groups) are
 *                    -1 / -inf, a missing group's code is -1.  The result does not depend on the order in which the device
 *                    scores the rows: two calls return the same bytes.
 *                    1 <= n_groups <= 64, 1 <= group_size <= VRAG_GROUPED_MAX_SIZE.  Queries are processed in slices whose keys fit
 *                    VRAG_GROUPED_SCRATCH_BYTES; a single query that needs more is VRAG_ERR_INVALID.  Every slice scans the passing rows.
 * Argument errors (null pointers, nq <= 0, n_groups or group_size out of range, a null bitmap with n_allow > 0, a negative code,
 * a column on another device than the index) are VRAG_ERR_INVALID before anything is launched or allocated.  The caller keeps
 * the column in step with the index: after vrag_dense_index_compact the column is rebuilt.  A search runs under the column's lock
 * and the index's (taken in that order), like the other searches of the index: a compaction waits for it. */
#define VRAG_GROUPED_MAX_SIZE 16
#define VRAG_GROUPED_SCRATCH_BYTES (256u << 20)
typedef struct vrag_group_column vrag_group_column;
int vrag_group_column_create(int32_t device, vrag_group_column** out);
void vrag_group_column_destroy(vrag_group_column* col);
int vrag_group_column_append(vrag_group_column* col, const int32_t* codes /*[n] host*/, int64_t n);
int64_t vrag_group_column_size(vrag_group_column* col);
int vrag_dense_index_search_grouped(vrag_dense_index* ix, const float* queries /*[nq,dim] host*/, int32_t nq, int32_t n_groups,
                                    int32_t group_size, vrag_group_column* column,
                                    const uint32_t* allow /*host bitmap or NULL*/, int64_t n_allow,
                                    float* scores /*[nq,n_groups,group_size]*/, int64_t* ids /*[nq,n_groups,group_size]*/,
                                    int32_t* groups /*[nq,n_groups]*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * IVF_FLAT over a dense index (csrc/ivf.hip; the reference builds every Milvus store with index_type="IVF_FLAT", nlist and
 * searches with search_params={"nprobe": N}: verbatim_rag/vector_stores/milvus_base.py:40-50, milvus_local.py:109-117,
 * index.py:571).  Opt-in and APPROXIMATE in which rows it looks at, exact in what it reports about them.
 * The handle is an overlay over a vrag_dense_index it does not own -- the base must outlive it: `nlist` fp32 centroids,
 * list_off[nlist + 1] and list_rows[n_assigned] (uint32 row numbers of the base grouped by list, ascending inside a list).  No
 * second image of the rows, 4 bytes per row of extra HBM; a search gathers the rows of the probed lists from the base.
 * Assignment rule, everywhere: list(x) = argmax_c (x . c - 1/2 |c|^2), the lowest list on ties (plain fp32 sums, order unspecified).
 *   set_centroids  takes the caller's centroids [nlist, dim] (host) instead of training; drops the lists (sync again).
 *   train          Lloyd's k-means on the device over min(size, max_train_rows) evenly strided rows of the base (sample item i =
 *                  row i * size / n_train); initial centroids = evenly strided sample items, no RNG; a centroid is the fp32 mean
 *                  of its members summed in ascending row order (no floating-point atomics: two trainings of the same rows give
 *                  the same bytes); an empty list keeps its centroid.  0 <= iters <= 1000.  Drops the lists (sync again).
 *   sync           assigns the base's rows [n_assigned, size) and rebuilds the lists; the base's size is read under the base's lock.
 *                  Rows appended to the base later are not searched until the next sync.
 *   stats / read   copy out (any pointer may be NULL); read needs centroids / a sync for what it is asked for.
 *   search         1 <= k <= 64, nprobe >= 1 (clamped to nlist), queries host fp32.  Per query: the nprobe lists with the best
 *                  assignment scores (score desc, list asc), then the exact top-k of their rows: scores are the sequential chain
 *                  acc = fmaf(x[c], q[c], acc), c ascending, of vrag_dense_index_search_filtered, bit for bit, order (score desc,
 *                  id asc), missing hits -1 / -inf -- with nprobe >= nlist the result IS that call's under an all-ones bitmap.
 *                  scanned_rows[q] (nullable) = rows in the query's probed lists.  Large nq x nprobe x k is processed in query
 *                  slices: at most 2^22 candidate keys (32 MB), 2^24 probe scores (64 MB) and 4 096 queries
 *                  per slice.
 * Argument errors (null pointers, nlist outside [1, 16384], k or nprobe out of range, search or list read before a sync, a base
 * that is not the one the overlay was created on) are VRAG_ERR_INVALID before anything is launched or allocated.  The handle
 * has its own scratch, stream and lock. */
typedef struct vrag_ivf_index vrag_ivf_index;
int vrag_ivf_index_create(vrag_dense_index* base, int32_t nlist, vrag_ivf_index** out);
void vrag_ivf_index_destroy(vrag_ivf_index* ivf);
int vrag_ivf_index_set_centroids(vrag_ivf_index* ivf, const float* centroids /*[nlist,dim] host*/);
int vrag_ivf_index_train(vrag_ivf_index* ivf, int32_t iters, int64_t max_train_rows);
int vrag_ivf_index_sync(vrag_ivf_index* ivf);
int vrag_ivf_index_stats(vrag_ivf_index* ivf, int32_t* nlist, int64_t* n_assigned, int64_t* largest_list);
int vrag_ivf_index_read(vrag_ivf_index* ivf, float* centroids /*[nlist,dim]*/, uint32_t* list_off /*[nlist+1]*/,
                        uint32_t* list_rows /*[n_assigned]*/);
/* After vrag_dense_index_compact of the base, with the same bitmap (n_keep = the base's size before it): every entry of
 * list_rows becomes its row's new number, the entries of dropped rows disappear, list_off is rebuilt and n_assigned becomes the
 * number of assigned rows that stay.  The renumbering is monotonic, so every list stays ascending; the centroids are untouched
 * and nothing is trained or assigned again.  VRAG_ERR_INVALID before a sync or when the bitmap is shorter than the lists. */
int vrag_ivf_index_remap(vrag_ivf_index* ivf, const uint32_t* keep_words /*host*/, int64_t n_keep);
int vrag_ivf_index_search(vrag_ivf_index* ivf, const float* queries /*[nq,dim] host*/, int32_t nq, int32_t k, int32_t nprobe,
                          float* scores /*[nq,k]*/, int64_t* ids /*[nq,k]*/, int64_t* scanned_rows /*[nq] or NULL*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * SQ8 dense rows (csrc/sq8.hip): a scalar-quantised dense field -- int8 codes and one fp32 scale per row, dim + 4 bytes per
 * row in HBM (the code stride is dim rounded up to 16 bytes, pad codes zero) -- searched with int8 queries.  Opt-in and
 * APPROXIMATE in what a code says about its component; everything below is exact and is the contract.
 * The rule, for an fp32 vector x[dim], a stored row and a query alike:
 *   m = max_c |x[c]|;  s = m / 127.0f (one correctly rounded fp32 division);
 *   code[c] = clamp(rintf(x[c] / s), -127, 127)  (fp32 division, round half to even);  m == 0: s = 0 and every code 0.
 * Score of query q against row r:
 *   idot = sum_c int(cq[c]) * int(cr[c])           an exact int32 (dim <= 4096: |idot| <= 4096 * 127^2 < 2^31)
 *   score = (float)idot * (s_q * s_r)              three fp32 roundings: the conversion (nearest even), the scale product,
 *                                                  the final product; no fused multiply-add, no reciprocal, no fast-math
 * so every score is defined bit for bit and every route returns the same bits.  Order (score desc, id asc), ties included;
 * missing hits -1 / -inf.  Rows and queries are expected to be finite.  A scale product that underflows to zero gives scores of
 * +0 and -0: they tie like every zero (the sign of a returned zero is unspecified).  A row whose maximum m > 0 is so small that
 * m / 127 underflows to 0 in fp32 has scale 0 and codes +-127 (a zero element of such a row divides 0 / 0: its code is outside the contract).
 *   create         1 <= dim <= 4096, 0 < capacity < 2^32 - 1.
 *   add            host fp32 rows [n, dim], staged in slabs through the device form; all of them or (VRAG_ERR_CAPACITY) none.
 *   add_device     device fp32 rows [n, dim]; quantised on the device on `stream`, which is synchronised before the call returns.
 *                  Rows [0, size) are never rewritten; the size is published under the handle's lock after the rows are in place.
 *   read           rows [first_row, first_row + n) as codes [n, dim] (without the pad) and scales [n]; either pointer may be NULL.
 *   search         1 <= k <= 1024, queries host fp32, quantised on the device by the rule.  Lists of up to 64 come from one pass;
 *                  longer ones as exact pages of 64 (a page admits only keys below the previous page's last key).
 *   search_filtered  the same over the rows r < min(n_allow, size) whose bit is set (bit r % 32 of word r / 32); rows at or
 *                  beyond n_allow are excluded; an empty mask returns -1 / -inf without a launch; a NULL mask with
 *                  n_allow > 0 is VRAG_ERR_INVALID.  The kernels skip cleared rows: the cost follows the shard, not the mask.
 *   set_route      0 = automatic, 1 = scan kernel (streaming; v_dot4_i32_i8; a few queries per pass over the shard), 2 = tile
 *                  kernel (v_mfma_i32_16x16x64_i8; up to 64 query columns per pass).  Automatic scans up to 4 queries and
 *                  tiles above.  A unit-test and tuning knob: integer arithmetic makes both routes return the same bits.
 * Argument errors are VRAG_ERR_INVALID before anything is launched or allocated; no device is VRAG_ERR_NO_DEVICE.  The handle
 * has its own scratch, stream and lock. */
typedef struct vrag_sq8_index vrag_sq8_index;
int vrag_sq8_index_create(int32_t dim, int64_t capacity, int32_t device, vrag_sq8_index** out);
void vrag_sq8_index_destroy(vrag_sq8_index* ix);
int64_t vrag_sq8_index_size(vrag_sq8_index* ix);
int vrag_sq8_index_add(vrag_sq8_index* ix, const float* rows /*[n,dim] host*/, int64_t n);
int vrag_sq8_index_add_device(vrag_sq8_index* ix, const float* rows /*[n,dim] device*/, int64_t n, void* stream);
int vrag_sq8_index_read(vrag_sq8_index* ix, int64_t first_row, int64_t n, int8_t* codes /*[n,dim] or NULL*/, float* scales /*[n] or NULL*/);
/* vrag_dense_index_compact for SQ8 rows: the codes (at their padded stride) and the scales move in place, same contract. */
int vrag_sq8_index_compact(vrag_sq8_index* ix, const uint32_t* keep_words /*host*/, int64_t n_keep, int64_t* new_size);
int vrag_sq8_index_set_route(vrag_sq8_index* ix, int32_t route);
int vrag_sq8_index_search(vrag_sq8_index* ix, const float* queries /*[nq,dim] host*/, int32_t nq, int32_t k,
                          float* scores /*[nq,k]*/, int64_t* ids /*[nq,k]*/, void* stream);
int vrag_sq8_index_search_filtered(vrag_sq8_index* ix, const float* queries /*[nq,dim] host*/, int32_t nq, int32_t k,
                                   const uint32_t* allow /*host, bit r%32 of word r/32*/, int64_t n_allow,
                                   float* scores /*[nq,k]*/, int64_t* ids /*[nq,k]*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * IVF_SQ8: the IVF overlay over an SQ8 index (csrc/ivf.hip, csrc/ivf_sq8.hip; Milvus' index_type="IVF_SQ8").  create_sq8 makes
 * a vrag_ivf_index whose base is a vrag_sq8_index; every other vrag_ivf_index_* call then works as it does over a dense base --
 * the same argument checks, locking, query slices and "the base must outlive the overlay" rule -- with two differences:
 *   the vector a row stands for, for training and assignment ONLY, is  x^[c] = fl((float)code[c] * scale), one fp32 product per
 *                  element.  The assignment rule is unchanged (argmax_c (x^ . c - 1/2 |c|^2), the lowest list on ties, plain fp32
 *                  sums in unspecified order); a trained centroid is the fp32 mean of its members' x^ summed in ascending row
 *                  order, so two trainings of the same rows give the same bytes.  Queries are probed as fp32 against the fp32
 *                  centroids, as over a dense base.
 *   search         1 <= k <= 64, nprobe >= 1 (clamped to nlist).  The queries are quantised once by the SQ8 rule; the rows of
 *                  the probed lists are scored by the SQ8 section's score, bit for bit (v_mfma_i32_16x16x64_i8 over 16 rows x 16
 *                  queries: the int32 dot is exact in any order).  Order (score desc, id asc), missing hits -1 / -inf.  With
 *                  nprobe >= nlist the result IS vrag_sq8_index_search's for the same queries, on either route of that call.
 *                  scanned_rows as above.
 *   remap          after vrag_sq8_index_compact of the base with the same bitmap: as after vrag_dense_index_compact. */
int vrag_ivf_index_create_sq8(vrag_sq8_index* base, int32_t nlist, vrag_ivf_index** out);

/* ------------------------------------------------------------------------------------------
 * PQ dense rows (csrc/pq.hip; Milvus' PQ codes, searched FLAT): a product-quantised dense field -- the vector is cut into m
 * sub-vectors of dsub = dim / m components and each is stored as the 8-bit number of the nearest of that sub-space's 256
 * centroids: m bytes per row in HBM (the code stride is m rounded up to 16 bytes, pad bytes zero).  Opt-in and APPROXIMATE in
 * what a code says about its sub-vector; everything below is exact and is the contract.
 *   chain(u, v)    acc = 0; acc = fmaf(u[t], v[t], acc) for t ascending over the dsub components (the dense oracle's chain).
 *   codebooks      cb[m][256][dsub] fp32;  h[j][c] = 0.5f * chain(cb[j][c], cb[j][c]).
 *   encoding       of sub-vector j of a vector x:  a(c) = chain(x_j, cb[j][c]) - h[j][c]  (one fp32 subtraction after the chain);
 *                  code[j] = argmax_c a(c), the lowest c on ties (the nearest centroid in L2, up to rounding).
 *   score          of query q against row r:  LUT[j][c] = chain(q_j, cb[j][c]);
 *                  score = (((0 + LUT[0][code_r[0]]) + LUT[1][code_r[1]]) + ...), fp32 additions with j ascending, never
 *                  reassociated, no fast-math -- the dot product of q with the row's centroids, defined bit for bit.
 * Order (score desc, id asc), ties included (rows with equal codes tie exactly: ties are common); missing hits -1 / -inf.  Zeros
 * tie and the sign of a returned zero is unspecified, as for SQ8.  Rows, queries and codebooks are expected to be finite.
 *   create         1 <= dim <= 4096, 1 <= m <= 128, dim % m == 0, dsub <= 64, 0 < capacity < 2^32 - 1.  No codebooks yet.
 *   set_codebooks  host cb [m, 256, dsub].  read_codebooks returns the bytes in place (set or trained).
 *   train          Lloyd's k-means per sub-space on the device over host sample rows [n, dim], 0 <= iters <= 1000, no random
 *                  numbers: the initial centroid c of every sub-space is sample row c * n / 256 (integer division); a round
 *                  assigns every sample row by the encoding rule, then a centroid becomes the sequential fp32 sum of its members'
 *                  sub-vectors in ascending row order (starting from 0), divided once (correctly rounded) by (float)count; an
 *                  empty cluster keeps its centroid.  Two trainings of the same rows give the same bytes, and so does a numpy
 *                  restatement.  set_codebooks and train are VRAG_ERR_INVALID once the index holds rows: the codes in place
 *                  were made with the codebooks in place.
 *   add, add_device, search, search_filtered   VRAG_ERR_INVALID before codebooks exist.
 *   add            host fp32 rows [n, dim], staged in slabs through the device form; all of them or (VRAG_ERR_CAPACITY) none.
 *   add_device     device fp32 rows [n, dim]; encoded on the device on `stream`, which is synchronised before the call returns.
 *                  Rows [0, size) are never rewritten; the size is published under the handle's lock after the rows are in place.
 *   read           rows [first_row, first_row + n) as codes [n, m] (without the pad).
 *   compact        vrag_sq8_index_compact's contract: the codes (at their padded stride) move in place, the codebooks stay.
 *   search         1 <= k <= 1024, queries host fp32; the tables are built on the device.  Lists of up to 64 come from one pass;
 *                  longer ones as exact pages of 64 (a page admits only keys below the previous page's last key).
 *   search_filtered  the same over the rows r < min(n_allow, size) whose bit is set (bit r % 32 of word r / 32); rows at or
 *                  beyond n_allow are excluded; an empty mask returns -1 / -inf without a launch; a NULL mask with
 *                  n_allow > 0 is VRAG_ERR_INVALID.  The kernel skips cleared rows: the cost follows the shard, not the mask.
 * Argument errors are VRAG_ERR_INVALID before anything is launched or allocated; no device is VRAG_ERR_NO_DEVICE.  The handle
 * has its own scratch, stream and lock. */
typedef struct vrag_pq_index vrag_pq_index;
int vrag_pq_index_create(int32_t dim, int32_t m, int64_t capacity, int32_t device, vrag_pq_index** out);
void vrag_pq_index_destroy(vrag_pq_index* ix);
int64_t vrag_pq_index_size(vrag_pq_index* ix);
int vrag_pq_index_set_codebooks(vrag_pq_index* ix, const float* cb /*[m,256,dsub] host*/);
int vrag_pq_index_read_codebooks(vrag_pq_index* ix, float* cb /*[m,256,dsub] host*/);
int vrag_pq_index_train(vrag_pq_index* ix, const float* rows /*[n,dim] host*/, int64_t n, int32_t iters);
int vrag_pq_index_add(vrag_pq_index* ix, const float* rows /*[n,dim] host*/, int64_t n);
int vrag_pq_index_add_device(vrag_pq_index* ix, const float* rows /*[n,dim] device*/, int64_t n, void* stream);
int vrag_pq_index_read(vrag_pq_index* ix, int64_t first_row, int64_t n, uint8_t* codes /*[n,m]*/);
int vrag_pq_index_compact(vrag_pq_index* ix, const uint32_t* keep_words /*host*/, int64_t n_keep, int64_t* new_size);
int vrag_pq_index_search(vrag_pq_index* ix, const float* queries /*[nq,dim] host*/, int32_t nq, int32_t k,
                         float* scores /*[nq,k]*/, int64_t* ids /*[nq,k]*/, void* stream);
int vrag_pq_index_search_filtered(vrag_pq_index* ix, const float* queries /*[nq,dim] host*/, int32_t nq, int32_t k,
                                  const uint32_t* allow /*host, bit r%32 of word r/32*/, int64_t n_allow,
                                  float* scores /*[nq,k]*/, int64_t* ids /*[nq,k]*/, void* stream);

/* Sparse (SPLADE) rows in CSR, term ids < vocab <= 65536; only documents sharing a term with the
 * query (score > 0) are hits, like an inverted index.  ids are CSR row numbers. */
typedef struct vrag_sparse_index vrag_sparse_index;
int vrag_sparse_index_create(int32_t vocab, int64_t n_docs, const int64_t* indptr, const int32_t* indices,
                             const float* values, int32_t device, vrag_sparse_index** out);
void vrag_sparse_index_destroy(vrag_sparse_index* ix);
int vrag_sparse_index_stats(vrag_sparse_index* ix, int64_t* n_docs, int64_t* nnz, int64_t* padded_nnz);
int vrag_sparse_index_search(vrag_sparse_index* ix, const int64_t* q_indptr, const int32_t* q_indices,
                             const float* q_values, int32_t nq, int32_t k, float* scores /*[nq,k]*/,
                             int64_t* ids /*[nq,k]*/, void* stream);
int vrag_sparse_index_run_resident(vrag_sparse_index* ix, int32_t nq, int32_t k, void* stream);
/* vrag_sparse_index_search over the documents d < min(n_allow, n_docs) whose bit is set in `allow` (as
 * vrag_dense_index_search_filtered: same bitmap, same refusals, same empty-mask answer).  The single-query SELL walk with the list
 * insertion gated by the document's bit -- scores are fmaf(value_j, q[term_j], acc) in CSR order, a hit needs a shared term --
 * and a 64-document slice without a passing document is skipped before its loads. */
int vrag_sparse_index_search_filtered(vrag_sparse_index* ix, const int64_t* q_indptr, const int32_t* q_indices,
                                      const float* q_values, int32_t nq, int32_t k, const uint32_t* allow, int64_t n_allow,
                                      float* scores /*[nq,k]*/, int64_t* ids /*[nq,k]*/, void* stream);
/* Device-resident result lists, as vrag_dense_index_search_device. */
int vrag_sparse_index_search_device(vrag_sparse_index* ix, const int64_t* q_indptr, const int32_t* q_indices,
                                    const float* q_values, int32_t nq, int32_t k, const int64_t* row_map /*device or NULL*/,
                                    int64_t n_map, int64_t id_base, float* out_scores /*[nq,k] device*/,
                                    int64_t* out_ids /*[nq,k] device*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * Full-text (BM25) search over raw texts (csrc/fulltext.hip; the reference's Milvus BM25 function over the `text` field,
 * verbatim_rag/vector_stores/milvus_cloud.py, bm25_k1 = 1.2, bm25_b = 0.75).  The analyzer is this library's own:
 *   token     = a maximal run of code points that are alphanumeric (Python str.isalnum()) under the committed table
 *               csrc/unicode_word.inc (tools/gen_unicode_word_table.py; it records its unicodedata version)
 *   lowercase = str.lower() of each code point where that is ONE code point, else the code point as it is
 *   term key  = 64-bit FNV-1a of the lowercased token's UTF-8 bytes.  Two distinct terms with one key merge; among 10^7 distinct
 *               terms the chance that any two share a key is about (10^7)^2 / 2^65 = 2.7e-6.
 *   Malformed UTF-8 decodes to U+FFFD (not alphanumeric): a byte that cannot start a sequence (one byte), and a lead byte
 *   with the continuation bytes that follow it (up to as many as it announces) when some are missing, when the sequence is
 *   an overlong form (C0 / C1 leads, E0 80-9F .., F0 80-8F ..), an encoded surrogate (U+D800-DFFF) or above U+10FFFF.
 * Statistics over the LIVE rows only (vrag_text_index_set_live; a filter does not change them), recomputed on the first call
 * after an add or a liveness change: N = live rows, avgdl = fp32(sum of their token counts / N) (a float64 division),
 * df(t) = live rows containing t.
 * Score, all fp32 without contraction:  K_d = k1 * ((1 - b) + b * (dl / avgdl))   (1 - b rounded to fp32 first)
 *   score(d) = sum over the query's distinct terms in ASCENDING key order, from 0, of  w_t * ((tf * (k1 + 1)) / (tf + K_d))
 *   with k1 + 1 an fp32 sum and w_t the caller's fp32 weight -- the store passes w_t = fp32(count of t in the query * idf64),
 *   idf64 = ln(1 + (N - df + 0.5) / (df + 0.5)) computed on the host in float64.  The device evaluates no transcendental.
 * Hits: rows with score > 0 that are live and in `allow`, ordered (score desc, row asc); missing hits id -1, score -inf.
 * Rows are numbered in insertion order across vrag_text_index_add calls.  Host pointers; every call synchronises. */
typedef struct vrag_text_index vrag_text_index;
/* The analyzer alone: token counts per document and the keys of all tokens in text order (n_tokens of them; only written when
 * n_tokens <= cap, else VRAG_ERR_CAPACITY with counts and n_tokens filled in).  doc_off[0] = 0, at most 4 GiB per call. */
int vrag_text_tokenize(const uint8_t* text, const int64_t* doc_off /*[n_docs+1]*/, int32_t n_docs, int32_t device, int64_t cap,
                       int32_t* counts /*[n_docs]*/, uint64_t* keys /*[cap]*/, int64_t* n_tokens);
int vrag_text_index_create(float k1, float b, int32_t device, vrag_text_index** out);
void vrag_text_index_destroy(vrag_text_index* ix);
/* Appends n_docs rows (live) as a new segment.  fold = 1: all segments are folded into one; fold = 0: the first (main)
 * segment stays and the new rows join the tail segment behind it. */
int vrag_text_index_add(vrag_text_index* ix, const uint8_t* text, const int64_t* doc_off /*[n_docs+1]*/, int32_t n_docs, int32_t fold);
/* Liveness of every row: bit r % 32 of words[r / 32]; n_rows must equal the rows added. */
int vrag_text_index_set_live(vrag_text_index* ix, const uint32_t* words, int64_t n_rows);
int vrag_text_index_stats(vrag_text_index* ix, int64_t* n_rows, int64_t* n_live, int64_t* sum_dl, int64_t* n_segments,
                          int64_t* n_postings /* any may be NULL */);
/* A shard of a row-sharded corpus (one index per GPU, each holding some of the rows): BM25 needs N, avgdl and df(t) of the
 * WHOLE corpus.  The caller sums (n_live, sum_dl) of vrag_text_index_stats over the shards and hands the totals back here:
 * K_d then uses avgdl = fp32(float64(sum_dl_total) / n_live_total) -- the documented formula on the summed integers, hence the
 * bits a single index over all the rows computes -- and vrag_text_index_query_terms reports n_live_total as N.  df stays this
 * shard's own (the caller sums the df vectors of the shards; query_terms lists every distinct term of every query, with
 * df = 0 for terms this shard does not hold, so the vectors of all shards line up).  vrag_text_index_stats keeps reporting
 * this index's own rows.  (0, 0) returns the index to its own statistics.  The pair survives add, set_live and folds until it
 * is set again; K_d is recomputed lazily by the statistics pass of the next call that needs it.  With the summed N and df in
 * the weights and the totals in K_d, a shard scores its rows with the same fp32 operations as the single index: merging the
 * shards' lists by (score desc, global row asc) reproduces the single index's list bit for bit. */
int vrag_text_index_set_corpus_stats(vrag_text_index* ix, int64_t n_live_total, int64_t sum_dl_total);
/* Query analysis on the device: the distinct terms of every query in ascending key order (query q: entries
 * q_indptr[q] .. q_indptr[q+1]) with their count in the query and their df; n_live = N.  VRAG_ERR_CAPACITY beyond cap terms.
 * Every distinct term is listed whether or not the index holds it (df = 0 then, also on an index without rows): the term
 * list depends on the query texts alone. */
int vrag_text_index_query_terms(vrag_text_index* ix, const uint8_t* text, const int64_t* doc_off /*[nq+1]*/, int32_t nq, int64_t cap,
                                int64_t* q_indptr /*[nq+1]*/, uint64_t* keys /*[cap]*/, int32_t* counts /*[cap]*/, int64_t* df /*[cap]*/,
                                int64_t* n_live);
/* Top-k (1 <= k <= 1024) of the queries given as (strictly ascending keys, fp32 weights) per query.  `allow` (host bitmap of
 * allow_rows rows, or NULL): rows a query may return (filters); rows at or beyond allow_rows -- added after the caller built
 * its filter -- are not allowed, and deleted rows never are. */
int vrag_text_index_search(vrag_text_index* ix, const int64_t* q_indptr /*[nq+1]*/, const uint64_t* keys, const float* weights,
                           int32_t nq, int32_t k, const uint32_t* allow, int64_t allow_rows, float* scores /*[nq,k]*/,
                           int64_t* ids /*[nq,k]*/);
/* The same search (k <= 64: one device pass) with the result lists left in DEVICE memory, as vrag_dense_index_search_device:
 * out_ids[q][j] = row_map[row] when `row_map` (device int64[n_map], local row -> global row) is given -- rows at or beyond
 * n_map become -1 / -inf -- else id_base + row; missing hits -1 / -inf.  Queries, weights and `allow` are host memory (the call
 * returns once they have been uploaded); the kernels are only enqueued on `stream` (NULL = the legacy default stream): no
 * device->host copy.  Later calls on this index order themselves behind those kernels: a search before it reuses the
 * workspace, the statistics pass (which also uploads a liveness change) before it rewrites K_d / the liveness bitmap,
 * vrag_text_index_add before it replaces segments or per-row arrays, vrag_text_index_destroy before it frees anything. */
int vrag_text_index_search_device(vrag_text_index* ix, const int64_t* q_indptr /*[nq+1]*/, const uint64_t* keys, const float* weights,
                                  int32_t nq, int32_t k, const uint32_t* allow, int64_t allow_rows,
                                  const int64_t* row_map /*device or NULL*/, int64_t n_map, int64_t id_base,
                                  float* out_scores /*[nq,k] device*/, int64_t* out_ids /*[nq,k] device*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * WordPiece tokenisation of raw texts (csrc/wordpiece.hip): the ids HF `tokenizers` returns for the BERT pipeline
 * BertNormalizer -> BertPreTokenizer -> WordPiece -> `[CLS] $A [SEP]` with truncation from the right.
 *   Code points  decoded as the full-text analyzer above decodes them (malformed UTF-8 = U+FFFD, same rules).
 *   Per code point, from the committed table csrc/wordpiece_table.inc (tools/gen_wordpiece_table.py; it records the
 *   unicodedata and tokenizers versions it was generated and verified with), in this order:
 *     clean_text          U+0000, U+FFFD and every Cc / Cf code point other than tab, LF, CR vanish; a White_Space code point is
 *                         a separator (it is one with clean_text off as well: the pre-tokenizer splits on the same set)
 *     handle_chinese_chars a code point of the CJK ranges of BertNormalizer (4E00-9FFF, 3400-4DBF, 20000-2A6DF, 2A700-2B73F,
 *                         2B740-2B81F, 2B920-2CEAF, F900-FAFF, 2F800-2FA1F) is a word of its own
 *     strip_accents       the code point is replaced by its canonical decomposition (NFD) without the Mn code points; a code
 *                         point left with nothing vanishes (it neither starts nor ends a word)
 *     lowercase           every remaining code point is replaced by its full lowercase mapping, character by character
 *                         (no context rule: capital sigma is always U+03C3)
 *     punctuation         a resulting code point that is ASCII punctuation (33-47, 58-64, 91-96, 123-126) or of a category
 *                         P* is a word of its own
 *   A word is otherwise a maximal run of code points that are none of the above; vanished code points do not interrupt it.
 *   A code point the table does not cover (unassigned or private use in the table's Unicode version, a non-zero combining
 *   class without being Mn, a disagreement between the table's two sources, Hangul syllables under strip_accents) sets
 *   needs_host for its text, as does a run of more than 64 vanished code points in front of a word: the ids written for
 *   such a text are unspecified, and the caller tokenises it on the host.
 *   Matching, per word of n code points:  n > max_chars_per_word -> one unk_id.  Otherwise from s = 0: the LONGEST e > s such
 *   that the UTF-8 of code points [s, e), with `prefix` in front when s > 0, is a vocabulary piece gives that piece's id and
 *   s = e; a position without any match turns the whole word into one unk_id.  The vocabulary is a hash table in device
 *   memory; every hit is confirmed byte for byte against the stored piece, so a hash collision cannot change an id.
 *   Packing: a text's ids are its words' ids in order, cut to max_length (add_special_tokens = 0) or to max_length - 2 with
 *   cls_id in front and sep_id behind (add_special_tokens = 1, max_length >= 2); texts are written back to back.
 * flags: VRAG_WP_LOWERCASE | VRAG_WP_STRIP_ACCENTS | VRAG_WP_CLEAN_TEXT | VRAG_WP_CHINESE_CHARS (HF's strip_accents = null
 * means "as lowercase": the caller resolves it).  Host pointers; the call synchronises; calls on one handle are serialised. */
#define VRAG_WP_LOWERCASE 1
#define VRAG_WP_STRIP_ACCENTS 2
#define VRAG_WP_CLEAN_TEXT 4
#define VRAG_WP_CHINESE_CHARS 8
#define VRAG_WP_MAX_CHARS_PER_WORD 128 /* largest max_chars_per_word a handle takes */
#define VRAG_WP_MAX_BATCH_BYTES (512ll << 20) /* text bytes one vrag_wordpiece_encode call takes */
#define VRAG_WORDPIECE_TILE_BYTES 4096 /* text bytes per workgroup of the word-boundary passes */
typedef struct vrag_wordpiece vrag_wordpiece;
/* Piece i of the vocabulary is vocab_blob[piece_off[i] .. piece_off[i+1]) (well-formed UTF-8, non-empty, no two alike) and
 * has id i; `prefix` is the NUL-terminated continuing_subword_prefix ("##"). */
int vrag_wordpiece_create(const uint8_t* vocab_blob, const int64_t* piece_off /*[n_vocab+1]*/, int32_t n_vocab, int32_t unk_id,
                          int32_t cls_id, int32_t sep_id, const char* prefix, int32_t max_chars_per_word, int32_t flags,
                          int32_t device, vrag_wordpiece** out);
void vrag_wordpiece_destroy(vrag_wordpiece* h);
/* Texts as vrag_text_tokenize takes them, at most VRAG_WP_MAX_BATCH_BYTES (512 MiB) of text per call and
 * bytes + 2 * n_docs < 2^31 (the handle keeps 4 bytes of id scratch per text byte -- 2 GiB at the limit -- and counts ids in
 * 32 bits).  seq_lens[d] = ids of text d (specials included), needs_host[d] = 1 when text d
 * must be tokenised on the host, n_ids = sum of seq_lens; ids is only written when n_ids <= cap, else VRAG_ERR_CAPACITY with
 * seq_lens, needs_host and n_ids filled in. */
int vrag_wordpiece_encode(vrag_wordpiece* h, const uint8_t* text, const int64_t* doc_off /*[n_docs+1]*/, int32_t n_docs,
                          int32_t add_special_tokens, int32_t max_length, int64_t cap, int32_t* ids /*[cap]*/,
                          int32_t* seq_lens /*[n_docs]*/, uint8_t* needs_host /*[n_docs]*/, int64_t* n_ids);

/* ------------------------------------------------------------------------------------------
 * Byte-level BPE tokenisation of raw texts (csrc/bpe.hip): the ids HF `tokenizers` returns for the pipeline
 * [NFC] -> ByteLevel(add_prefix_space = false, use_regex = true) -> BPE -> `<cls> $A <sep>` with truncation from the right.
 *   Code points  decoded as the full-text analyzer above decodes them; per code point the committed table csrc/bpe_table.inc
 *   (tools/gen_bpe_table.py; it records the unicodedata and tokenizers versions it was generated and verified with) gives the
 *   class L (general category L*), N (N*), W (the White_Space property) or O (anything else), NFC_Quick_Check and the
 *   canonical combining class.
 *   needs_host is set for a text -- its ids are then unspecified, and the caller tokenises it on the host -- that holds
 *     a code point the table does not cover (unassigned, private use or surrogate in the table's Unicode version; U+FFFD, which
 *     is also what ill-formed UTF-8 decodes to);
 *     with VRAG_BPE_NFC, a code point with NFC_Quick_Check != Yes, or a code point of combining class c > 0 behind one of a
 *     larger class (the UAX #15 quick check: any other text IS its own NFC form, and the device normalises nothing);
 *     a pre-token of more than VRAG_BPE_MAX_WORD_BYTES bytes; a run of U+0020 that spans more than 256 tiles (1 MiB); a
 *     contraction within 3 bytes behind a tile boundary that more than 256 U+0020 precede.
 *   Space runs   space_run_id[n] >= 0 (2 <= n <= 64) says that the run of n U+0020 is an added token with that id (set S).  A
 *   maximal run of r U+0020 is consumed from the left, every step taking the largest n in S that is <= what remains (HF's
 *   leftmost-longest match); what is left over is ordinary text.  These tokens cut a text into SEGMENTS.
 *   Pre-tokens   within a segment, the matches of the GPT-2 pattern
 *       's|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+
 *   as a rule local to one code point c with predecessor p and successor q in the segment.  c starts a pre-token when it
 *   starts the segment, and otherwise
 *     c in L: not when an ACTIVE contraction that begins 1 or 2 code points in front still covers c; always when one ends
 *             right in front of c; else unless p is in L or is U+0020
 *     c in N / O: unless p is of the same class or is U+0020
 *     c in W: when p is not in W, or q exists and is not in W (the last white space in front of a non-space is left over by
 *             `\s+(?!\S)`; U+0020 then joins the piece behind it by the rules above, any other stands alone)
 *   An apostrophe is ACTIVE when it starts its segment or p is in L, N or W other than U+0020 (behind U+0020 or a code point of
 *   O it is absorbed by ` ?[^\s\p{L}\p{N}]+`), and the case-sensitive suffix s, t, m, d, re, ve or ll follows it.
 *   BPE, per pre-token: one symbol per byte (byte_id), then, while any adjacent pair is in the merge table, the pair of the lowest
 *   rank -- the leftmost among equals -- is replaced by its merged id.  The merge table is a hash table in device memory keyed by
 *   (left id, right id); every hit is confirmed on the full key.  With VRAG_BPE_IGNORE_MERGES a pre-token whose bytes are a
 *   `whole` entry gets that id directly (hash of the bytes, confirmed byte for byte).
 *   Packing as vrag_wordpiece_encode.
 * Host pointers; the call synchronises; calls on one handle are serialised. */
#define VRAG_BPE_NFC 1            /* the file's normalizer is NFC: prove every text NFC or flag it */
#define VRAG_BPE_IGNORE_MERGES 2
#define VRAG_BPE_MAX_WORD_BYTES 64 /* one pre-token per wave64, one symbol per lane */
#define VRAG_BPE_MAX_SPACE_RUN 64  /* longest run of U+0020 that can be an added token */
#define VRAG_BPE_MAX_BATCH_BYTES (512ll << 20) /* text bytes one vrag_bpe_encode call takes */
#define VRAG_BPE_TILE_BYTES 4096   /* text bytes per workgroup of the boundary passes */
typedef struct vrag_bpe vrag_bpe;
/* Merge r (rank r, 0 <= r < n_merges < 2^26) replaces the adjacent ids (merge_left[r], merge_right[r]) by merge_id[r]; no two
 * merges have the same pair.  byte_id[b] is the id of byte b's character of the byte-level alphabet.  space_run_id[n] as
 * above (-1: no such token; entries 0 and 1 must be -1).  whole_*: only with VRAG_BPE_IGNORE_MERGES -- entry i is the bytes
 * whole_blob[whole_off[i] .. whole_off[i+1]) (1 .. VRAG_BPE_MAX_WORD_BYTES of them, no two alike) with id whole_id[i].  All ids
 * in 0 .. n_vocab - 1. */
int vrag_bpe_create(int32_t n_vocab, const int32_t* merge_left, const int32_t* merge_right, const int32_t* merge_id, int32_t n_merges,
                    const int32_t* byte_id /*[256]*/, const int32_t* space_run_id /*[VRAG_BPE_MAX_SPACE_RUN+1]*/,
                    const uint8_t* whole_blob, const int64_t* whole_off /*[n_whole+1]*/, const int32_t* whole_id, int32_t n_whole,
                    int32_t cls_id, int32_t sep_id, int32_t flags, int32_t device, vrag_bpe** out);
void vrag_bpe_destroy(vrag_bpe* h);
/* As vrag_wordpiece_encode: at most VRAG_BPE_MAX_BATCH_BYTES of text per call and bytes + 2 * n_docs < 2^31; seq_lens,
 * needs_host and n_ids are always filled in, ids only when n_ids <= cap (else VRAG_ERR_CAPACITY). */
int vrag_bpe_encode(vrag_bpe* h, const uint8_t* text, const int64_t* doc_off /*[n_docs+1]*/, int32_t n_docs,
                    int32_t add_special_tokens, int32_t max_length, int64_t cap, int32_t* ids /*[cap]*/,
                    int32_t* seq_lens /*[n_docs]*/, uint8_t* needs_host /*[n_docs]*/, int64_t* n_ids);
/* vrag_bpe_encode plus, for id i, offsets[i] = the half-open range of code points OF ITS OWN TEXT that HF `tokenizers` reports as
 * Encoding.offsets[i]; same capacity / needs_host protocol (offsets is written when ids is).  An id that covers the bytes
 * [b0, b1) of its text starts at the index of the code point that holds byte b0 and ends behind the code point that holds byte
 * b1 - 1: two ids that split one multi-byte character both report that character's (i, i + 1); a space-run token of t spaces
 * reports (s, s + t); a VRAG_BPE_IGNORE_MERGES whole-word hit reports its pre-token; [CLS] / [SEP] report (0, 0); truncation
 * truncates the offsets with the ids.  A text the device proves NFC is its own normalisation, so the offsets index the text as
 * given; any other text is flagged as above. */
int vrag_bpe_encode_offsets(vrag_bpe* h, const uint8_t* text, const int64_t* doc_off /*[n_docs+1]*/, int32_t n_docs,
                            int32_t add_special_tokens, int32_t max_length, int64_t cap, int32_t* ids /*[cap]*/,
                            int32_t* offsets /*[cap, 2]*/, int32_t* seq_lens /*[n_docs]*/, uint8_t* needs_host /*[n_docs]*/,
                            int64_t* n_ids);

/* Cross-shard merge of per-shard top-k lists (the reference has no sharding -- this is the step after the
 * all-gather of `[n_lists][nq][k_in]` (fp32 score, global row id) lists, each sorted by (score desc, id asc) with
 * id = -1 entries as a tail).  Writes the first k_out entries of the merged order per query (-inf / -1 padded).
 * Global ids must be < 2^32 and unique across lists.  `*_list_stride`: bytes between consecutive lists (0 = dense,
 * nq*k_in elements) -- lets the gathered buffer of one packed all-gather ([ids | scores] per rank) be merged in
 * place.  on_device = 1: all four pointers are device memory on `device` and the kernel is only enqueued on
 * `stream`; on_device = 0: host pointers, the call copies in and out and synchronises. */
int vrag_topk_merge(const float* scores, const int64_t* ids, int32_t n_lists, int32_t nq, int32_t k_in, int32_t k_out,
                    int64_t score_list_stride, int64_t id_list_stride, float* out_scores, int64_t* out_ids,
                    int32_t on_device, int32_t device, void* stream);

/* Weighted reciprocal-rank fusion of a batch of queries (hybrid_search.py:73-129 on row numbers; the array form is
 * rrf_merge_rows in vector_stores.py).  rows[q] = the methods' ranked lists of query q laid side by side, l_total
 * entries, a negative entry = a rank without a candidate (it keeps its position).  gains[p] = the float64 a candidate at
 * position p contributes (share_m * (1.0 / (rrf_k + rank + 1)), computed by the caller).  Per query and distinct row:
 * score = gains of its positions added one after the other in ascending position, starting from the first;
 * order = score descending, ties by first position ascending; out_rows / out_dist = the first top_k rows and
 * 1.0 - score, padded with -1 / 0.0.  1 <= l_total <= 4096, 1 <= top_k <= l_total, row ids < 2^32, gains finite and
 * >= 0.  on_device as vrag_topk_merge: 1 = all pointers are device memory on `device`, the work is only enqueued on
 * `stream`; 0 = host pointers, the call copies in and out and synchronises (and checks ids and gains).  The device form
 * cannot read its inputs and so verifies neither: there a row id >= 2^32 is the caller's error, and what it yields differs
 * between the regimes (l_total <= 64 compares whole ids and fuses any of them correctly; longer lists shift the id into
 * the upper 52 bits of a sort key, where an id of 2^52 - 1 or more loses bits and is grouped with other rows or dropped). */
int vrag_rrf_fuse(const int64_t* rows /*[nq, l_total]*/, const double* gains /*[l_total]*/, int32_t nq, int32_t l_total,
                  int32_t top_k, int64_t* out_rows /*[nq, top_k]*/, double* out_dist /*[nq, top_k]*/,
                  int32_t on_device, int32_t device, void* stream);

/* ------------------------------------------------------------------------------------------
 * Row filter: the store's boolean metadata filters (store_filter.py) evaluated over typed columns in device memory
 * (csrc/rowfilter.hip).  A column holds one metadata key of every row: kinds[r] (VRAG_FILTER_KIND_*, one byte) and payload[r]
 * (eight bytes: the IEEE f64 bits of a number, the dictionary code of a string, 0 / 1 of a bool, 0 otherwise) -- 9 bytes of
 * device memory per row and column.  A filter is a postfix program over LEAVES; a leaf names one column and states, per kind of
 * stored value, what it answers (each independent of the others):
 *   other    other_bit (0 / 1)                                   -- missing key, null, list, object
 *   bool     bit `value` of bool_bits (bit 0 = the answer for false, bit 1 = for true)
 *   number   num_op (VRAG_FILTER_NUM_*) against `bound`, an IEEE f64 comparison (-0.0 == 0.0, infinities ordered, NaN equals nothing)
 *   string   str_mode VRAG_FILTER_STR_NEVER / _ALWAYS, or _TABLE: bit (code % 32) of tables[table_off + code / 32] for a code
 *            < table_codes, 0 for a code at or beyond it (nothing past the leaf's table is ever read)
 * ops[i] = VRAG_FILTER_OP_LEAF | (leaf index << 8) pushes a leaf's answer, _AND / _OR pop two and push one, _NOT flips the top;
 * exactly one value must remain.  Limits: VRAG_FILTER_MAX_COLUMNS distinct columns named by the leaves, _MAX_LEAVES leaves,
 * _MAX_OPS ops, stack depth _MAX_DEPTH (the stack is the bits of one 32-bit register per row).
 *   append   host arrays; rows are appended behind the column's earlier rows, which are kept (geometric growth).  kinds > 3 invalid.
 *   eval     rows [0, n_rows) of every referenced column (each must hold at least n_rows) -> out_words (host, ceil(n_rows / 32)
 *            words, bit r % 32 of word r / 32 = row r passes, bits at and beyond n_rows zero; nothing behind those words is written).
 *            n_rows == 0: VRAG_OK without a launch.  Synchronous.
 * Everything is validated on the host before anything is launched or allocated (leaf columns, table ranges against n_table_words,
 * n_rows against the columns, the op list, the limits): VRAG_ERR_INVALID with a message, out_words untouched.  The handle has its
 * own device arrays, stream and lock.
 *
 * String leaves answered on the device (csrc/strmatch.hip).  A column may also hold the DICTIONARY of its strings: code c (the
 * payload of a string row) is the UTF-8 bytes bytes[off[c] .. off[c + 1]), appended to only, codes continuing from those held.
 * The match kernel -- one lane per dictionary string -- applies one operator and one operand text to codes [0, n_codes) and
 * writes the table a _TABLE leaf reads (bit code % 32 of word code / 32, tail bits of the last word zero):
 *   VRAG_FILTER_MATCH_EQ .. _GE   bytewise lexicographic comparison of the stored string with `text`, a proper prefix being
 *                                 smaller -- for valid UTF-8 the order of the code points
 *   VRAG_FILTER_MATCH_LIKE        `text` is a pattern as written, escapes included: `%` any run of zero or more characters, `_`
 *                                 exactly one character (one code point), a backslash makes the next character literal; over the
 *                                 whole string, case-sensitive, a newline a character like any other
 * Limits: `text` at most VRAG_FILTER_MATCH_MAX_PATTERN bytes; a pattern at most VRAG_FILTER_MATCH_MAX_SEGMENTS non-empty runs
 * between its unescaped `%`; a dictionary string shorter than 2 GiB.
 *   append_strings  host arrays, n strings: off[0] = 0, off ascending, bytes[off[i] .. off[i + 1]) valid UTF-8 each.
 *   strings         codes and bytes the column's dictionary holds.
 *   match           one table to the host (out_words: ceil(n_codes / 32) words, nothing behind them written); n_codes at most
 *                   the dictionary's codes (a prefix is fine); n_codes == 0: VRAG_OK without a launch.  Synchronous.
 *   eval_matched    eval, with some _TABLE leaves answered by the kernel: `tables` is uploaded as eval does, then for each entry
 *                   of `matches`, in order, leaf `leaf`'s table (its table_off, its table_codes codes, over its column's
 *                   dictionary) is written in device memory by one match launch with operator `op` and the text
 *                   texts[text_off .. text_off + text_len), then the program runs.  What `tables` holds in those ranges is not
 *                   read; a table made here never travels to the host.
 * VRAG_ERR_INVALID with a message, before anything is allocated or launched and with the outputs untouched, for: a column with
 * fewer dictionary codes than asked for, a text over a limit, a pattern ending in a lone backslash, invalid UTF-8 in a pattern or
 * in appended strings, offsets not ascending from 0, an unknown operator, a match whose leaf is no _TABLE leaf or whose text
 * lies outside `texts` (a leaf's table range is checked against n_table_words as in eval).
 *
 * Membership in list-valued metadata (csrc/listfilter.hip; `json_contains` in store_filter.py).  A column may also hold a LIST
 * PART: for every row the elements of its list as CSR -- row r's elements are [elem_off[r], elem_off[r + 1]) of elem_kinds /
 * elem_payload, one (kind, payload) each in exactly the encoding of kinds / payload, strings through the column's one dictionary
 * (so a _TABLE leaf and the match kernel serve elements unchanged).  A row whose value is no list has an empty range.  8 bytes
 * per row + 9 bytes per element of device memory, geometric growth.  The list part is independent of the column's rows: either
 * may be absent or shorter.
 *   append_lists  host arrays, n rows: elem_off[0] = 0, non-decreasing, elem_off[n] elements; the rows go behind the list rows
 *                 held and their offsets continue from the elements held.  n == 0: VRAG_OK, nothing read.
 *   list_rows     rows and elements the column's list part holds.
 *   eval_lists    eval_matched (same arguments, same checks, same output), and ops may also hold
 *                 VRAG_FILTER_OP_LIST_ANY | (leaf index << 8): pushes, for row r, the OR over the elements of r's list in the
 *                 leaf's column of what the leaf answers for the element's (kind, payload) -- other_bit, bool_bits, num_op / bound
 *                 and str_mode / table apply per element as they do per row; a row without elements pushes 0.  A leaf that only
 *                 LIST_ANY ops push needs its column's list part to cover n_rows, not the column's rows; a leaf that a LEAF op
 *                 pushes (or no op) needs the rows as in eval.  A program without a LIST_ANY op runs exactly as eval_matched
 *                 runs it, on the same kernel; one with a LIST_ANY op runs on a kernel of its own, one lane per row, each lane
 *                 walking its row's elements up to the first match: a row with a very long list makes one lane walk alone, as
 *                 a very long string does in the match kernel.  eval and eval_matched refuse LIST_ANY like any unknown op.
 *   compact       a vrag_row_filter_compact that drops at least one row DROPS the list part of every column (list_rows then
 *                 reports 0 rows, 0 elements; the memory is kept for reuse): the caller appends the compacted lists again before
 *                 its next list filter.  One that drops nothing leaves them.  A list part of more rows than the bitmap covers is
 *                 VRAG_ERR_INVALID like such a column.
 * VRAG_ERR_INVALID with a message, before anything is allocated or launched and with the outputs untouched, also for: offsets
 * not starting at 0 or decreasing, an element kind above 3, a LIST_ANY leaf whose column holds the lists of fewer than n_rows rows. */
#define VRAG_FILTER_MAX_COLUMNS 16
#define VRAG_FILTER_MAX_LEAVES 64
#define VRAG_FILTER_MAX_OPS 256
#define VRAG_FILTER_MAX_DEPTH 32
#define VRAG_FILTER_KIND_OTHER 0
#define VRAG_FILTER_KIND_NUMBER 1
#define VRAG_FILTER_KIND_STRING 2
#define VRAG_FILTER_KIND_BOOL 3
#define VRAG_FILTER_NUM_NEVER 0
#define VRAG_FILTER_NUM_ALWAYS 1
#define VRAG_FILTER_NUM_EQ 2
#define VRAG_FILTER_NUM_NE 3
#define VRAG_FILTER_NUM_LT 4
#define VRAG_FILTER_NUM_LE 5
#define VRAG_FILTER_NUM_GT 6
#define VRAG_FILTER_NUM_GE 7
#define VRAG_FILTER_STR_NEVER 0
#define VRAG_FILTER_STR_ALWAYS 1
#define VRAG_FILTER_STR_TABLE 2
#define VRAG_FILTER_OP_LEAF 0
#define VRAG_FILTER_OP_AND 1
#define VRAG_FILTER_OP_OR 2
#define VRAG_FILTER_OP_NOT 3
#define VRAG_FILTER_OP_LIST_ANY 4 /* vrag_row_filter_eval_lists only */
typedef struct vrag_filter_leaf {
  double bound;
  int64_t table_off;
  int64_t table_codes;
  int32_t column;
  uint8_t num_op;
  uint8_t str_mode;
  uint8_t bool_bits;
  uint8_t other_bit;
} vrag_filter_leaf;
typedef struct vrag_row_filter vrag_row_filter;
int vrag_row_filter_create(int32_t device, vrag_row_filter** out);
void vrag_row_filter_destroy(vrag_row_filter* f);
int vrag_row_filter_add_column(vrag_row_filter* f, int32_t* col_out);
int vrag_row_filter_append(vrag_row_filter* f, int32_t col, const uint8_t* kinds /*[n] host*/, const uint64_t* payload /*[n] host*/,
                           int64_t n);
int vrag_row_filter_rows(vrag_row_filter* f, int32_t col, int64_t* n);
/* Drops the rows whose bit is cleared (bit r % 32 of word r / 32) from the kinds and payload of EVERY column, in place, order
 * kept (csrc/compact.h).  A column that holds fewer rows than the bitmap covers is compacted under the bitmap's prefix; one that
 * holds more is VRAG_ERR_INVALID before anything is launched.  The string dictionaries stay as they are (codes do not change). */
int vrag_row_filter_compact(vrag_row_filter* f, const uint32_t* keep_words /*host*/, int64_t n_keep);
int vrag_row_filter_eval(vrag_row_filter* f, const vrag_filter_leaf* leaves, int32_t n_leaves, const uint32_t* ops, int32_t n_ops,
                         const uint32_t* tables /*[n_table_words] host, NULL when 0*/, int64_t n_table_words, int64_t n_rows,
                         uint32_t* out_words /*host*/, void* stream);
#define VRAG_FILTER_MATCH_EQ 0
#define VRAG_FILTER_MATCH_NE 1
#define VRAG_FILTER_MATCH_LT 2
#define VRAG_FILTER_MATCH_LE 3
#define VRAG_FILTER_MATCH_GT 4
#define VRAG_FILTER_MATCH_GE 5
#define VRAG_FILTER_MATCH_LIKE 6
#define VRAG_FILTER_MATCH_MAX_PATTERN 256 /* bytes of operand text */
#define VRAG_FILTER_MATCH_MAX_SEGMENTS 16 /* LIKE: non-empty runs between the unescaped % */
typedef struct vrag_filter_match {
  int64_t text_off;
  int32_t text_len;
  int32_t leaf;
  int32_t op;
  int32_t pad;
} vrag_filter_match;
int vrag_row_filter_append_strings(vrag_row_filter* f, int32_t col, const uint8_t* bytes /*[off[n]] host*/,
                                   const int64_t* off /*[n + 1] host, off[0] = 0*/, int64_t n);
int vrag_row_filter_strings(vrag_row_filter* f, int32_t col, int64_t* n_codes, int64_t* n_bytes);
int vrag_row_filter_match(vrag_row_filter* f, int32_t col, int32_t op, const uint8_t* text, int32_t text_len, int64_t n_codes,
                          uint32_t* out_words /*host, ceil(n_codes / 32)*/, void* stream);
int vrag_row_filter_eval_matched(vrag_row_filter* f, const vrag_filter_leaf* leaves, int32_t n_leaves, const uint32_t* ops,
                                 int32_t n_ops, const uint32_t* tables /*[n_table_words] host, NULL when 0*/, int64_t n_table_words,
                                 const vrag_filter_match* matches /*[n_matches]*/, int32_t n_matches,
                                 const uint8_t* texts /*[n_text_bytes] host*/, int64_t n_text_bytes, int64_t n_rows,
                                 uint32_t* out_words /*host*/, void* stream);
int vrag_row_filter_append_lists(vrag_row_filter* f, int32_t col, const int64_t* elem_off /*[n + 1] host, from 0, non-decreasing*/,
                                 const uint8_t* elem_kinds /*[elem_off[n]] host*/, const uint64_t* elem_payload /*[elem_off[n]] host*/,
                                 int64_t n);
int vrag_row_filter_list_rows(vrag_row_filter* f, int32_t col, int64_t* n_rows, int64_t* n_elems);
int vrag_row_filter_eval_lists(vrag_row_filter* f, const vrag_filter_leaf* leaves, int32_t n_leaves, const uint32_t* ops,
                               int32_t n_ops, const uint32_t* tables /*[n_table_words] host, NULL when 0*/, int64_t n_table_words,
                               const vrag_filter_match* matches /*[n_matches]*/, int32_t n_matches,
                               const uint8_t* texts /*[n_text_bytes] host*/, int64_t n_text_bytes, int64_t n_rows,
                               uint32_t* out_words /*host*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * The exchange step of sharded retrieval: one process per GPU, the corpus row-sharded, every rank answers the
 * (replicated) query batch on its own shard with vrag_*_index_search_device and contributes its packed lists
 *     payload = [ global ids  int64 x nq*k_in | scores fp32 x nq*k_in | pad to 8 bytes ]       (device memory)
 * to ONE RCCL all-gather over xGMI; every rank then merges the world's lists on its GPU.  RCCL is bound at run time (the
 * copy already mapped into the process -- e.g. torch's -- else the system librccl.so.1; $VRAG_RCCL_LIB overrides).
 * The host framework only has to carry the unique id from rank 0 to the other ranks (torch.distributed broadcast, MPI, a
 * file): vrag_comm_get_unique_id on rank 0, vrag_comm_create (collective: every rank calls it) everywhere.
 * Calls on one communicator must be issued in the same order on every rank (RCCL's rule). */
#define VRAG_COMM_ID_BYTES 128
typedef struct vrag_comm vrag_comm;
int vrag_comm_get_unique_id(uint8_t* id /*[VRAG_COMM_ID_BYTES]*/);
int vrag_comm_create(const uint8_t* id, int32_t rank, int32_t world, int32_t device, vrag_comm** out);
void vrag_comm_destroy(vrag_comm* comm);
int vrag_comm_info(vrag_comm* comm, int32_t* rank, int32_t* world, int32_t* rccl_version /* any may be NULL */);
/* ncclAllGather of nbytes per rank, enqueued on `stream` (NULL = the legacy default stream); recv holds world * nbytes. */
int vrag_comm_allgather(vrag_comm* comm, const void* send /*device*/, void* recv /*device*/, int64_t nbytes, void* stream);
/* The whole exchange: all-gather of `payload` into `gathered` (device scratch of world * payload bytes) + vrag_topk_merge in
 * place, both enqueued on `stream`; out_* are device [nq, k_out], identical on every rank.  No synchronisation. */
int vrag_topk_allgather_merge(vrag_comm* comm, const void* payload, void* gathered, int32_t nq, int32_t k_in, int32_t k_out,
                              float* out_scores /*device*/, int64_t* out_ids /*device*/, void* stream);

/* Sentence boundaries of a batch of chunk texts (the GPU-side sentence split): for every document the parts of
 *   re.split(r"(?<=[.!?])\s+", text), each stripped of surrounding white space, empty parts dropped
 * (packages/core/verbatim_core/extractors.py:190-195), as [start, end) BYTE offsets into the document's UTF-8 text.
 * `text` holds the documents back to back, document d is bytes doc_off[d] .. doc_off[d+1] (doc_off[0] = 0).  counts[d] is
 * the exact number of sentences; only the first `cap` of a document are stored at starts/ends[d * cap ...] -- the caller
 * re-splits a document with counts[d] > cap itself.  White space = Python's str.isspace set.  Host pointers; synchronous. */
int vrag_split_sentences(const uint8_t* text, const int64_t* doc_off /*[n_docs+1]*/, int32_t n_docs, int32_t cap,
                         int32_t* counts /*[n_docs]*/, int32_t* starts /*[n_docs, cap]*/, int32_t* ends /*[n_docs, cap]*/,
                         int32_t device);

/* Markdown chunking of a batch of documents (csrc/chunk.hip): the structural pass of the reference's default chunker
 * (MarkdownChunkerProvider._md_chunker_with_ancestor_injection, verbatim_rag/chunker_providers.py:93-213) over UTF-8 bytes.
 * All offsets are BYTE offsets inside the document; chunk borders follow a '\n', so they are code-point borders.  White space =
 * Python's str.isspace set.  For a document of n bytes:
 *   R1  lines start at byte 0 and behind every 0x0A, nowhere else;
 *   R2  a line start s is a candidate when the line opens with exactly k '#' (1 <= k <= 6) and a white-space character starts at
 *       s + k (it may be the '\n'; '#' with nothing behind it is no candidate);
 *   R3  its match is [s, e): p = first byte at or behind s + k that starts no white-space character (possibly lines further
 *       down), e = first 0x0A at or behind p, else n; title = [p, e) without trailing white space; level = k; the header's
 *       exact line = [line_start, line_end) = s's own line without its '\n';
 *   R4  in ascending order a candidate is a header iff s > e of the header accepted before it (re.finditer: a candidate inside
 *       an earlier match is swallowed);
 *   R5  no header: one chunk [0, n), header = -1 (also for n = 0);
 *   R6  include_preamble and line_start of the first header > 0: first chunk [0, that line_start), header = -1;
 *   R7  header i owns [line_start_i, block_end_i) = up to the next header's line_start or n; it becomes a chunk iff bit `level`
 *       of split_levels is set (other blocks belong to no chunk); the stack pops while its top's level >= the header's level,
 *       then takes the header, chunk or not;
 *   R8  a chunk's ancestors are the stack below its header: at most five, levels strictly rising, outermost first.
 * headers[] holds every header of the batch in document, then position order; chunks[] likewise, the chunks of document d at
 * doc_chunk_off[d] .. doc_chunk_off[d+1]; `header` and `ancestors` index headers[] (unused ancestor slots are -1).
 * Documents may be empty; doc_off[0] = 0; a document is under 2 GiB, a batch at most VRAG_MD_MAX_BATCH_BYTES; split_levels bits
 * outside 1..6 are VRAG_ERR_INVALID.  n_headers / n_chunks / doc_chunk_off are always filled in; the tables only when both fit,
 * else VRAG_ERR_CAPACITY (a document has at most one header per line that begins with '#', and one chunk more than headers).
 * Bytes that are not valid UTF-8 are ordinary non-space bytes: the call never fails on content.  Host pointers; synchronous. */
#define VRAG_MD_MAX_BATCH_BYTES (512ll << 20)
typedef struct {
  int32_t doc, level, line_start, line_end, title_start, title_end, block_end, reserved /* 0 */;
} vrag_md_header;
typedef struct {
  int32_t doc, start, end, header /* index into headers[], -1 = preamble / whole document */, n_ancestors, ancestors[5];
} vrag_md_chunk;
int vrag_chunk_markdown(const uint8_t* text, const int64_t* doc_off /*[n_docs+1]*/, int32_t n_docs, uint32_t split_levels,
                        int32_t include_preamble, int64_t header_cap, vrag_md_header* headers, int64_t chunk_cap,
                        vrag_md_chunk* chunks, int64_t* n_headers, int64_t* n_chunks, int64_t* doc_chunk_off /*[n_docs+1]*/,
                        int32_t device);

/* Host-side packer of the (question, chunk) pairs of ONE question for the sentence-classification extractor -- the layout
 *   [CLS] q [SEP] s1 [SEP] s2 ... ([SEP])   with inclusive token ranges per sentence, budget = max_length - 2, sentences that do
 * not fit dropped from the first one that does not (extractor_models/dataset.py:127-243).  The question-independent pieces of a
 * chunk are cached by the caller: tail = [SEP] s1 [SEP] s2 ... (int32) and cum[i] = tokens of the first i + 1 `[SEP] sentence`
 * groups (int64); tails[p] / cums[p] are their ADDRESSES for pair p, n_groups[p] the sentence count.  q_ids = the question's ids
 * without a trailing [SEP] (q_len of them).  Per pair: kept[p] sentences fit (0 = none: the caller's general routine decides),
 * seq_lens[p] ids are appended to ids_out, kept[p] ranges to starts_out / ends_out; totals_out = {ids, ranges} written.
 * Pure host code (no device, no allocation); VRAG_ERR_CAPACITY when an output capacity would be exceeded. */
int vrag_pack_qa_pairs(const int32_t* q_ids, int32_t q_len, int32_t n_pairs, const uint64_t* tails, const uint64_t* cums,
                       const int32_t* n_groups, int32_t budget, int32_t sep_id, int32_t* ids_out, int64_t ids_cap,
                       int64_t* starts_out, int64_t* ends_out, int64_t ranges_cap, int32_t* seq_lens /*[n_pairs]*/,
                       int32_t* kept /*[n_pairs]*/, int64_t* totals_out /*[2]*/);

/* -inf / -1 lists in device memory: the contribution of a rank that holds none of the rows. */
int vrag_topk_fill_empty(float* scores /*[n] device*/, int64_t* ids /*[n] device*/, int64_t n, int32_t device, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VRAG_AMD_H */
