// Tuning / unit-test harness of the kernels (include/vrag_amd_debug.h): synthetic-operand timing loops and the attention
// kernels', the GEMM's, the row kernels', the packing / glue kernels' and the tiled search kernels' unit-test hooks.  NOT part of the product library: compiled only into libvrag_amd_dbg.so (build.py, -DVRAG_DEBUG_API),
// which tools/ and the attention unit test load beside libvrag_amd.so.  Every hook stages its device buffers, and has their
// canaries checked, through DbgBufs (debug_bufs.h).
#include "../../include/vrag_amd.h"
#include "../../include/vrag_amd_debug.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "attention.h"
#include "debug_bufs.h"
#include "gemm_bf16.h"
#include "glue_kernels.h"
#include "host_util.h"
#include "norm_heads.h"
#include "qkv_attn.h"
#include "spans.h"
#include "topk_kernels.h"

using namespace vrag;

namespace {

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// Operands of the timing loops: pseudo-random bf16 in [-1, 1), 0x3f80 | 7 mantissa bits = [1,2), minus 1.5, times 2
void fill_bf16_lcg(std::vector<unsigned short>& h, unsigned x) {
  for (auto& v : h) {
    x = x * 1664525u + 1013904223u;
    const unsigned m = (x >> 9) & 0x7f, s = (x >> 31) << 15, ex = 0x3e80u + (((x >> 20) & 1) << 7);
    v = (unsigned short)(s | ex | m);
  }
}

// The timing protocol of the _ms hooks: three warm-up launches, then events around `iters` launches; *ms_out = ms per launch.
template <typename Launch>
int time_launches(const char* what, int iters, Launch launch, float* ms_out) {
  hipEvent_t a, b;
  (void)hipEventCreate(&a);
  (void)hipEventCreate(&b);
  hipError_t le = hipSuccess;
  for (int i = 0; i < 3 && le == hipSuccess; ++i) le = launch();
  (void)hipEventRecord(a, 0);
  for (int i = 0; i < iters && le == hipSuccess; ++i) le = launch();
  (void)hipEventRecord(b, 0);
  hipError_t se = hipEventSynchronize(b);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, a, b);
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  if (le != hipSuccess || se != hipSuccess) {
    set_error("debug %s failed: %s", what, hipGetErrorString(le != hipSuccess ? le : se));
    return VRAG_ERR_HIP;
  }
  *ms_out = ms / iters;
  return VRAG_OK;
}

// The sequences of an attention hook: at least one token each, rows aligned, inside the buffers' rows, no two overlapping.
int check_sequences(const int32_t* seq_row, const int32_t* seq_len, int n, int rows) {
  for (int s = 0; s < n; ++s) {
    const int row = seq_row[s], len = seq_len[s];
    ARG_CHECK(len >= 1, "seq_len[%d] = %d must be at least 1", s, len);
    ARG_CHECK(row >= 0 && row % kSeqAlign == 0, "seq_row[%d] = %d must be a non-negative multiple of %d", s, row, kSeqAlign);
    ARG_CHECK((int64_t)row + len <= rows, "sequence %d (row %d, %d tokens) ends past row %d", s, row, len, rows);
  }
  std::vector<int> order(n);
  for (int s = 0; s < n; ++s) order[s] = s;
  std::sort(order.begin(), order.end(), [&](int l, int r) { return seq_row[l] < seq_row[r]; });
  for (int i = 0; i + 1 < n; ++i)
    ARG_CHECK(seq_row[order[i]] + seq_len[order[i]] <= seq_row[order[i + 1]], "sequences %d and %d overlap", order[i], order[i + 1]);
  return VRAG_OK;
}

}  // namespace

extern "C" {

int vrag_debug_gemm_ms(int32_t epi, int32_t M, int32_t N, int32_t K, int32_t iters, int32_t device, float* ms_out) {
  ARG_CHECK(ms_out && M > 0 && N % 128 == 0 && K % 64 == 0 && iters > 0, "bad arguments");
  ARG_CHECK(epi == EPI_F32 || epi == EPI_BF16 || epi == EPI_RESIDUAL || epi == EPI_GEGLU || epi == EPI_QKV_ROPE ||
                epi == EPI_F32_GELU || epi == EPI_NONE,
            "unsupported epilogue for the diagnostic");
  if (const int rc = use_device(device); rc != VRAG_OK) return rc;
  const size_t Mp = (size_t)align_up(M, kRowPad);
  DevBuf A, W, outf, outb, q, kk, vt, cs, sn, pos, sat;
  hipError_t e = A.alloc(Mp * K * 2);
  if (e == hipSuccess) e = W.alloc((size_t)N * K * 2);
  if (e == hipSuccess) e = outf.alloc(Mp * N * 4);
  if (e == hipSuccess) e = outb.alloc(Mp * N * 2);
  if (e == hipSuccess) e = q.alloc(Mp * N * 2);
  if (e == hipSuccess) e = kk.alloc(Mp * N * 2);
  if (e == hipSuccess) e = vt.alloc(Mp * N * 2);
  if (e == hipSuccess) e = cs.alloc(512 * 32 * 4);
  if (e == hipSuccess) e = sn.alloc(512 * 32 * 4);
  if (e == hipSuccess) e = pos.alloc(Mp * 4);
  if (e == hipSuccess) e = sat.alloc(4);   // the fp16 clamp word (not read)
  if (e != hipSuccess) {
    set_error("debug gemm allocation failed: %s", hipGetErrorString(e));
    return VRAG_ERR_HIP;
  }
  {
    std::vector<unsigned short> h(std::max(Mp * K, (size_t)N * K));
    fill_bf16_lcg(h, 12345u);
    if (getenv("VRAG_DEBUG_GEMM_ZERO")) std::fill(h.begin(), h.end(), (unsigned short)0);   // probe: operand-data dependence of the clock
    (void)hipMemcpy(A.p, h.data(), Mp * K * 2, hipMemcpyHostToDevice);
    (void)hipMemcpy(W.p, h.data(), (size_t)N * K * 2, hipMemcpyHostToDevice);
  }
  (void)hipMemset(outf.p, 0, Mp * N * 4);
  (void)hipMemset(pos.p, 0, Mp * 4);
  (void)hipMemset(cs.p, 0, 512 * 32 * 4);
  (void)hipMemset(sn.p, 0, 512 * 32 * 4);
  GemmParams g{};
  g.op_dtype = getenv("VRAG_DEBUG_GEMM_F16") ? kOpF16 : kOpBf16;   // same bit patterns read as fp16: finite values in [2^-15, 2^-7)
  g.f16_sat = sat.as<unsigned>();
  g.A = A.as<bf16_t>();
  g.W = W.as<bf16_t>();
  g.M = M;
  g.N = N;
  g.K = K;
  g.out_f32 = outf.as<float>();
  g.out_bf16 = outb.as<bf16_t>();
  g.q = q.as<bf16_t>();
  g.k = kk.as<bf16_t>();
  g.vt = vt.as<bf16_t>();
  g.vt_ld = (int)Mp;
  g.rope_cos = cs.as<float>();
  g.rope_sin = sn.as<float>();
  g.pos = pos.as<int>();
  g.hidden = N / 3;
  g.q_scale = 0.125f;
  if (epi == EPI_RESIDUAL && !getenv("VRAG_DEBUG_GEMM_PLAIN_RESID")) {   // as the encoder launches it with the LayerNorm fold
    g.resid_bf16 = outb.as<bf16_t>();
    g.stats_part = q.as<float>();                                            // Mp * N/64 * 2 floats <= Mp * N * 2 bytes
    g.stats_ld = (int)Mp;
    if (getenv("VRAG_DEBUG_GEMM_SPLIT")) {   // the split residual stream on both sides (layers >= 1 of the encoder schedule)
      g.lo_in = kk.as<unsigned char>();
      g.lo_out = kk.as<unsigned char>();
      g.ln_shift = pos.as<float>();        // zeros
      g.ln_shift_prev = pos.as<float>();
      (void)hipMemset(kk.p, 0, Mp * N * 2);
      (void)hipMemset(outb.p, 0, Mp * N * 2);
    }
  }
  return time_launches("gemm", iters, [&] { return launch_gemm((GemmEpi)epi, g, 0); }, ms_out);
}

int vrag_debug_attn_ms(int32_t local, int32_t n_seqs, int32_t S, int32_t H, int32_t window, int32_t iters, int32_t device,
                       float* ms_out) {
  ARG_CHECK(ms_out && n_seqs > 0 && S > 0 && S % kSeqAlign == 0 && H % 64 == 0 && iters > 0, "bad arguments");
  if (const int rc = use_device(device); rc != VRAG_OK) return rc;
  const size_t T = (size_t)n_seqs * S, Tp = (size_t)align_up((int)T, kRowPad);
  const int qb = attention_q_block(local != 0);
  std::vector<int> bs, bl, bq;
  for (int s = 0; s < n_seqs; ++s)
    for (int q0 = 0; q0 < S; q0 += qb) {
      bs.push_back(s * S);
      bl.push_back(S);
      bq.push_back(q0);
    }
  DevBuf q, k, vt, o, d_bs, d_bl, d_bq, sat;
  hipError_t e = q.alloc(Tp * H * 2);
  if (e == hipSuccess) e = k.alloc(Tp * H * 2);
  if (e == hipSuccess) e = vt.alloc(Tp * H * 2);
  if (e == hipSuccess) e = o.alloc(Tp * H * 2);
  if (e == hipSuccess) e = d_bs.alloc(bs.size() * 4);
  if (e == hipSuccess) e = d_bl.alloc(bs.size() * 4);
  if (e == hipSuccess) e = d_bq.alloc(bs.size() * 4);
  if (e == hipSuccess) e = sat.alloc(4);   // the fp16 clamp word (not read)
  if (e != hipSuccess) {
    set_error("debug attention allocation failed: %s", hipGetErrorString(e));
    return VRAG_ERR_HIP;
  }
  {
    std::vector<unsigned short> h(Tp * H);
    fill_bf16_lcg(h, 777u);
    (void)hipMemcpy(q.p, h.data(), Tp * H * 2, hipMemcpyHostToDevice);
    (void)hipMemcpy(k.p, h.data(), Tp * H * 2, hipMemcpyHostToDevice);
    (void)hipMemcpy(vt.p, h.data(), Tp * H * 2, hipMemcpyHostToDevice);
    (void)hipMemcpy(d_bs.p, bs.data(), bs.size() * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(d_bl.p, bl.data(), bs.size() * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(d_bq.p, bq.data(), bs.size() * 4, hipMemcpyHostToDevice);
  }
  AttnParams ap{};
  ap.q = q.as<bf16_t>();
  ap.k = k.as<bf16_t>();
  ap.vt = vt.as<bf16_t>();
  ap.o = o.as<bf16_t>();
  ap.blk_seq_start = d_bs.as<int>();
  ap.blk_seq_len = d_bl.as<int>();
  ap.blk_q0 = d_bq.as<int>();
  ap.n_blocks = (int)bs.size();
  ap.H = H;
  ap.nh = H / 64;
  ap.Tp = (int)Tp;
  ap.window = window;
  ap.op_dtype = getenv("VRAG_DEBUG_GEMM_F16") ? kOpF16 : kOpBf16;
  ap.f16_sat = sat.as<unsigned>();
  return time_launches("attention", iters, [&] { return launch_attention(ap, local != 0, 0); }, ms_out);
}

int vrag_debug_qkv_attn_ms(int32_t local, int32_t n_seqs, int32_t S, int32_t H, int32_t window, int32_t iters, int32_t flags,
                           int32_t device, float* ms_out) {
  ARG_CHECK(ms_out && n_seqs > 0 && S > 0 && S <= kFusedMaxSeq && S % kSeqAlign == 0 && H % 64 == 0 && iters > 0, "bad arguments");
  if (const int rc = use_device(device); rc != VRAG_OK) return rc;
  const size_t T = (size_t)n_seqs * S, Tp = (size_t)align_up((int)T, kRowPad);
  const int nh = H / 64;
  std::vector<int> row(n_seqs), len(n_seqs, S);
  for (int s = 0; s < n_seqs; ++s) row[s] = s * S;
  DevBuf x, w, o, mu, rstd, lns, cs, d_row, d_len, sat;
  hipError_t e = x.alloc(Tp * H * 2);
  if (e == hipSuccess) e = w.alloc((size_t)3 * H * H * 2);
  if (e == hipSuccess) e = o.alloc(Tp * H * 2);
  if (e == hipSuccess) e = mu.alloc(Tp * 4);
  if (e == hipSuccess) e = rstd.alloc(Tp * 4);
  if (e == hipSuccess) e = lns.alloc(((size_t)3 * H + 64) * 4);
  if (e == hipSuccess) e = cs.alloc((size_t)kFusedMaxSeq * 32 * 4);
  if (e == hipSuccess) e = d_row.alloc((size_t)n_seqs * 8 * sizeof(int4));   // the groups' wave descriptors
  if (e == hipSuccess) e = d_len.alloc(n_seqs * 4);
  if (e == hipSuccess) e = sat.alloc(4);   // the fp16 clamp word (not read)
  if (e != hipSuccess) {
    set_error("debug allocation failed: %s", hipGetErrorString(e));
    return VRAG_ERR_HIP;
  }
  {
    std::vector<unsigned short> h(std::max(Tp * H, (size_t)3 * H * H));
    fill_bf16_lcg(h, 777u);
    (void)hipMemcpy(x.p, h.data(), Tp * H * 2, hipMemcpyHostToDevice);
    (void)hipMemcpy(w.p, h.data(), (size_t)3 * H * H * 2, hipMemcpyHostToDevice);
    std::vector<float> f(std::max(Tp, (size_t)kFusedMaxSeq * 32), 0.05f);
    (void)hipMemcpy(mu.p, f.data(), Tp * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(rstd.p, f.data(), Tp * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(lns.p, f.data(), (size_t)3 * H * 4, hipMemcpyHostToDevice);
    std::fill(f.begin(), f.end(), 0.7071f);
    (void)hipMemcpy(cs.p, f.data(), (size_t)kFusedMaxSeq * 32 * 4, hipMemcpyHostToDevice);
  }
  std::vector<int4> groups((size_t)n_seqs * 8);
  const int n_groups = fused_pack_groups(row.data(), len.data(), 0, n_seqs, groups.data());
  (void)hipMemcpy(d_row.p, groups.data(), (size_t)n_groups * 8 * sizeof(int4), hipMemcpyHostToDevice);
  QkvAttnParams f{};
  f.x = x.as<bf16_t>();
  f.w = w.as<bf16_t>();
  f.ln_mu = mu.as<float>();
  f.ln_rstd = rstd.as<float>();
  f.ln_s = lns.as<float>();
  f.rope_cos = cs.as<float>();
  f.rope_sin = cs.as<float>();
  f.rope_rows = kFusedMaxSeq;
  f.o = o.as<bf16_t>();
  f.groups = d_row.as<int4>();
  f.n_groups = n_groups;
  f.H = H;
  f.nh = nh;
  f.Tp = (int)Tp;
  f.window = window;
  f.op_dtype = getenv("VRAG_DEBUG_GEMM_F16") ? kOpF16 : kOpBf16;
  f.f16_sat = sat.as<unsigned>();
  f.q_scale = 0.125f * 1.4426950408889634f;
  f.debug_flags = flags;
  return time_launches("fused attention", iters, [&] { return launch_qkv_attention(f, local != 0, 0); }, ms_out);
}

int vrag_debug_attn_run_ex(vrag_debug_attn_args* a, int32_t device) {
  ARG_CHECK(a, "null arguments");
  ARG_CHECK(a->q && a->k && a->vt && a->o && a->seq_row && a->seq_len, "null required pointer");
  ARG_CHECK(a->H > 0 && a->H % 64 == 0, "H (%d) must be a positive multiple of 64", a->H);
  ARG_CHECK(a->rows > 0 && a->rows % kRowPad == 0, "rows (%d) must be a positive multiple of %d", a->rows, kRowPad);
  ARG_CHECK((int64_t)a->rows * a->H < ((int64_t)1 << 31), "rows * H must stay below 2^31");
  ARG_CHECK(a->n_seqs > 0, "n_seqs (%d) must be positive", a->n_seqs);
  ARG_CHECK(!a->local || a->window >= 0, "a banded launch needs window >= 0 (got %d)", a->window);
  ARG_CHECK(!a->local || a->window <= (1 << 24), "window (%d) above 2^24", a->window);
  ARG_CHECK(device >= 0, "bad device %d", device);
  const int n = a->n_seqs;
  if (const int rc = check_sequences(a->seq_row, a->seq_len, n, a->rows); rc != VRAG_OK) return rc;
  // the q-block descriptors, as vrag_encoder_set_batch builds them (capi.hip): one block per attention_q_block rows of each sequence
  const int qb = attention_q_block(a->local != 0);
  std::vector<int> bs, bl, bq;
  for (int s = 0; s < n; ++s)
    for (int q0 = 0; q0 < a->seq_len[s]; q0 += qb) {
      bs.push_back(a->seq_row[s]);
      bl.push_back(a->seq_len[s]);
      bq.push_back(q0);
    }
  const int n_blocks = (int)bs.size();
  ARG_CHECK(!a->blocks_out || n_blocks <= a->blocks_cap, "blocks_out holds %d descriptors, the launch has %d", a->blocks_cap, n_blocks);
  if (const int rc = use_device(device); rc != VRAG_OK) return rc;
  a->n_blocks = n_blocks;
  if (a->blocks_out)
    for (int b = 0; b < n_blocks; ++b) {
      a->blocks_out[3 * b] = bs[b];
      a->blocks_out[3 * b + 1] = bl[b];
      a->blocks_out[3 * b + 2] = bq[b];
    }
  const size_t R = (size_t)a->rows, H = (size_t)a->H;
  DbgBufs B;
  AttnParams ap{};
  ap.q = B.in<bf16_t>(a->q, R * H, "q");
  ap.k = B.in<bf16_t>(a->k, R * H, "k");
  ap.vt = B.in<bf16_t>(a->vt, R * H, "vt");
  ap.o = B.inout<bf16_t>(a->o, R * H, "o");
  ap.blk_seq_start = B.in<int>(bs.data(), (size_t)n_blocks, "blk_seq_start");
  ap.blk_seq_len = B.in<int>(bl.data(), (size_t)n_blocks, "blk_seq_len");
  ap.blk_q0 = B.in<int>(bq.data(), (size_t)n_blocks, "blk_q0");
  ap.n_blocks = n_blocks;
  ap.H = (int)H;
  ap.nh = (int)H / 64;
  ap.Tp = (int)R;
  ap.window = a->window;
  ap.op_dtype = a->f16 ? kOpF16 : kOpBf16;
  ap.f16_sat = B.clamp_word(&a->f16_saturated);
  hipError_t e = B.staged();
  if (e == hipSuccess) e = launch_attention(ap, a->local != 0, 0);
  return B.finish("attention", e);
}

// The equal-length layout of tools/attn_unit.py: n_seqs sequences of S tokens back to back from row 0, zero rows behind them.
int vrag_debug_attn_run(int32_t local, int32_t n_seqs, int32_t S, int32_t H, int32_t window, int32_t f16, const uint16_t* q,
                        const uint16_t* k, const uint16_t* vt, uint16_t* o, int32_t device) {
  ARG_CHECK(q && k && vt && o && n_seqs > 0 && S > 0 && S % kSeqAlign == 0 && H > 0 && H % 64 == 0, "bad arguments");
  ARG_CHECK((int64_t)n_seqs * S + kRowPad < ((int64_t)1 << 31) / H, "rows * H must stay below 2^31");
  const size_t T = (size_t)n_seqs * S, Tp = (size_t)align_up((int64_t)T, kRowPad);
  std::vector<uint16_t> hq(Tp * H, 0), hk(Tp * H, 0), ho(Tp * H, 0);
  std::memcpy(hq.data(), q, T * H * 2);
  std::memcpy(hk.data(), k, T * H * 2);
  std::vector<int32_t> row(n_seqs), len(n_seqs, S);
  for (int s = 0; s < n_seqs; ++s) row[s] = s * S;
  vrag_debug_attn_args a{};
  a.q = hq.data();
  a.k = hk.data();
  a.vt = vt;
  a.o = ho.data();
  a.seq_row = row.data();
  a.seq_len = len.data();
  a.rows = (int32_t)Tp;
  a.H = H;
  a.n_seqs = n_seqs;
  a.local = local;
  a.window = window;
  a.f16 = f16;
  const int status = vrag_debug_attn_run_ex(&a, device);
  if (status == VRAG_OK) std::memcpy(o, ho.data(), T * H * 2);
  return status;
}

int vrag_debug_gemm_run(vrag_debug_gemm_args* a, int32_t device) {
  ARG_CHECK(a, "null arguments");
  const int epi = a->epi, M = a->M, N = a->N, K = a->K;
  ARG_CHECK(epi == EPI_F32 || epi == EPI_BF16 || epi == EPI_F32_GELU || epi == EPI_RESIDUAL || epi == EPI_GEGLU ||
                epi == EPI_QKV_ROPE || epi == EPI_SPLADE,
            "epilogue %d is not covered by the GEMM unit hook", epi);
  ARG_CHECK(M > 0 && N > 0 && N % 128 == 0 && K > 0 && K % 64 == 0, "bad shape M=%d N=%d K=%d", M, N, K);
  const int64_t Mpad = align_up(M, kRowPad);
  ARG_CHECK(a->row0 >= 0 && a->row0 % 64 == 0 && a->rows % 64 == 0 && a->rows >= a->row0 + Mpad,
            "rows (%d) must be a multiple of 64 holding row0 (%d) + M rounded up to %d", a->rows, a->row0, kRowPad);
  ARG_CHECK(a->A && a->W, "A and W are required");
  const bool in_split = a->lo_in != nullptr, out_split = a->lo_out != nullptr;
  // every pointer the chosen epilogue dereferences must be there: the hook never launches a kernel onto a null buffer
  switch (epi) {
    case EPI_F32:
    case EPI_F32_GELU: ARG_CHECK(a->out_f32, "out_f32 required"); break;
    case EPI_BF16: ARG_CHECK(a->out_bf16, "out_bf16 required"); break;
    case EPI_GEGLU: ARG_CHECK(a->out_bf16, "out_bf16 required"); break;
    case EPI_RESIDUAL:
      ARG_CHECK(a->out_f32 || (in_split && out_split), "out_f32 required unless the stream is split on both sides");
      ARG_CHECK(!a->res_mu || (a->res_rstd && a->res_g && a->res_b), "post-LN input needs res_mu, res_rstd, res_g, res_b");
      ARG_CHECK(!(in_split || out_split) || a->resid_bf16, "the split stream needs resid_bf16");
      break;
    case EPI_QKV_ROPE:
      ARG_CHECK(a->hidden > 0 && a->hidden % 128 == 0 && N == 3 * a->hidden, "QKV: N = 3 hidden, hidden %% 128 == 0");
      ARG_CHECK(a->q && a->k && a->vt && a->rope_cos && a->rope_sin && a->pos && a->rope_rows > 0, "QKV buffers required");
      break;
    case EPI_SPLADE: ARG_CHECK(a->tok_seq && a->splade_rows && a->n_seqs > 0, "SPLADE buffers required"); break;
  }
  ARG_CHECK(!(a->ln_mu || a->ln_rstd || a->ln_s) || (a->ln_mu && a->ln_rstd && a->ln_s), "the fold needs ln_mu, ln_rstd and ln_s");
  ARG_CHECK(!a->stats_in || (a->ln_mu && a->ln_shift), "consumer finalisation needs ln_mu, ln_rstd, ln_s and ln_shift");
  ARG_CHECK(!in_split || a->ln_shift_prev, "an arriving split stream needs ln_shift_prev");
  ARG_CHECK(!out_split || a->ln_shift, "a leaving split stream needs ln_shift");
  const size_t R = (size_t)a->rows, lo = (size_t)a->row0;
  // indices the kernel gathers with are checked on the host: rows [row0, row0 + Mpad) are read
  if (a->pos)
    for (size_t r = lo; r < lo + (size_t)Mpad; ++r) ARG_CHECK(a->pos[r] >= 0 && a->pos[r] < a->rope_rows, "pos[%zu] out of range", r);
  if (a->tok_seq)
    for (size_t r = lo; r < lo + (size_t)Mpad; ++r)
      ARG_CHECK(a->tok_seq[r] >= -1 && a->tok_seq[r] < a->n_seqs, "tok_seq[%zu] out of range", r);
  if (const int rc = use_device(device); rc != VRAG_OK) return rc;

  // device copies (DbgBufs): an absent optional buffer stays a null pointer; row0 offsets are applied to the typed pointers
  const size_t H = (size_t)std::max(a->hidden, 0), NO = epi == EPI_GEGLU ? (size_t)N / 2 : (size_t)N, Ns = (size_t)N;
  const bool one_lo = a->lo_in == a->lo_out;   // the split stream updated in place: one device buffer, copied back
  DbgBufs B;
  GemmParams g{};
  g.op_dtype = a->f16 ? kOpF16 : kOpBf16;
  g.M = M;
  g.N = N;
  g.K = K;
  g.act_gelu = a->act_gelu;
  g.stats_ld = (int)R;
  g.fin_eps = a->fin_eps;
  g.hidden = (int)H;
  g.vt_ld = (int)R;
  g.q_scale = a->q_scale;
  g.A = B.in<bf16_t>(a->A, R * K, "A") + lo * K;
  g.W = B.in<bf16_t>(a->W, Ns * K, "W");
  g.bias = B.in_opt<float>(a->bias, Ns, "bias");
  g.ln_s = B.in_opt<float>(a->ln_s, Ns, "ln_s");
  g.stats_in = at(B.in_opt<float>(a->stats_in, (size_t)(K / 64) * R * 2, "stats_in"), lo * 2);
  g.res_mu = at(B.in_opt<float>(a->res_mu, R, "res_mu"), lo);
  g.res_rstd = at(B.in_opt<float>(a->res_rstd, R, "res_rstd"), lo);
  g.res_g = B.in_opt<float>(a->res_g, Ns, "res_g");
  g.res_b = B.in_opt<float>(a->res_b, Ns, "res_b");
  g.rope_cos = B.in_opt<float>(a->rope_cos, (size_t)a->rope_rows * 32, "rope_cos");
  g.rope_sin = B.in_opt<float>(a->rope_sin, (size_t)a->rope_rows * 32, "rope_sin");
  g.pos = at(B.in_opt<int>(a->pos, R, "pos"), lo);
  g.tok_seq = at(B.in_opt<int>(a->tok_seq, R, "tok_seq"), lo);
  unsigned char* lo_in = one_lo ? B.inout_opt<unsigned char>(a->lo_out, R * Ns, "lo_in") : B.in_opt<unsigned char>(a->lo_in, R * Ns, "lo_in");
  g.lo_in = at(lo_in, lo * Ns);
  g.out_f32 = at(B.inout_opt<float>(a->out_f32, R * Ns, "out_f32"), lo * Ns);
  g.out_bf16 = at(B.inout_opt<bf16_t>(a->out_bf16, R * NO, "out_bf16"), lo * NO);
  g.q = at(B.inout_opt<bf16_t>(a->q, R * H, "q"), lo * H);
  g.k = at(B.inout_opt<bf16_t>(a->k, R * H, "k"), lo * H);
  g.vt = at(B.inout_opt<bf16_t>(a->vt, H * R, "vt"), lo);
  g.ln_mu = at(B.inout_opt<float>(a->ln_mu, R, "ln_mu"), lo);
  g.ln_rstd = at(B.inout_opt<float>(a->ln_rstd, R, "ln_rstd"), lo);
  g.ln_shift = at(B.inout_opt<float>(a->ln_shift, R, "ln_shift"), lo);
  g.ln_shift_prev = at(B.inout_opt<float>(a->ln_shift_prev, R, "ln_shift_prev"), lo);
  g.resid_bf16 = at(B.inout_opt<bf16_t>(a->resid_bf16, R * Ns, "resid_bf16"), lo * Ns);
  g.stats_part = at(B.inout_opt<float>(a->stats_part, (size_t)(N / 64) * R * 2, "stats_part"), lo * 2);
  g.lo_out = at(one_lo ? lo_in : B.inout_opt<unsigned char>(a->lo_out, R * Ns, "lo_out"), lo * Ns);
  g.splade_rows = B.inout_opt<unsigned>(a->splade_rows, (size_t)a->n_seqs * Ns, "splade_rows");
  g.f16_sat = B.clamp_word(&a->f16_saturated);
  hipError_t e = B.staged();
  if (e == hipSuccess) {
    const int thr = gemm_small_m_threshold(-1);
    if (a->small_rows >= 0) gemm_small_m_threshold(a->small_rows);
    e = launch_gemm((GemmEpi)epi, g, 0);
    const GemmConfig c = gemm_last_config();
    gemm_small_m_threshold(thr);
    const int32_t cfg[7] = {c.bm, c.bn, c.wm, c.wn, c.ns, c.hw, c.kch};
    std::memcpy(a->config, cfg, sizeof(cfg));
  }
  return B.finish("gemm", e);
}

int vrag_debug_pack_groups(const int32_t* seq_row, const int32_t* seq_len, int32_t n, int32_t packer, int32_t* out) {
  ARG_CHECK(seq_row && seq_len && out && n > 0 && (packer == 0 || packer == 1), "bad arguments");
  for (int s = 0; s < n; ++s) ARG_CHECK(seq_len[s] >= 1 && seq_len[s] <= kFusedMaxSeq, "seq_len[%d] = %d outside 1..%d", s, seq_len[s], kFusedMaxSeq);
  static_assert(sizeof(int4) == 4 * sizeof(int32_t), "descriptor layout");
  int4* g = reinterpret_cast<int4*>(out);
  return packer ? pack_groups_best_fit(seq_row, seq_len, 0, n, g) : fused_pack_groups(seq_row, seq_len, 0, n, g);
}

int vrag_debug_qkv_attn_run(vrag_debug_qkv_attn_args* a, int32_t device) {
  ARG_CHECK(a, "null arguments");
  ARG_CHECK(a->x && a->w && a->rope_cos && a->rope_sin && a->o && a->seq_row && a->seq_len && a->groups_out, "null required pointer");
  ARG_CHECK(!(a->ln_mu || a->ln_rstd) || (a->ln_mu && a->ln_rstd && a->ln_s), "the fold needs ln_mu, ln_rstd and ln_s");
  ARG_CHECK(a->nh > 0 && a->H == 64 * a->nh, "H (%d) must be 64 * nh (%d)", a->H, a->nh);
  ARG_CHECK(a->rows > 0 && a->rows % kRowPad == 0, "rows (%d) must be a positive multiple of %d", a->rows, kRowPad);
  ARG_CHECK((int64_t)a->rows * a->H < ((int64_t)1 << 31), "rows * H must stay below 2^31");
  ARG_CHECK(a->rope_rows > 0 && a->n_seqs > 0 && (a->packer == 0 || a->packer == 1), "bad rope_rows / n_seqs / packer");
  ARG_CHECK(!a->local || a->window >= 0, "bad window");
  ARG_CHECK(a->debug_flags == 0 || a->debug_flags == 32, "debug_flags (%d) must be 0 or 32", a->debug_flags);
  ARG_CHECK(device >= 0, "bad device %d", device);
  const int n = a->n_seqs;
  if (const int rc = check_sequences(a->seq_row, a->seq_len, n, a->rows); rc != VRAG_OK) return rc;
  for (int s = 0; s < n; ++s) {
    const int row = a->seq_row[s], len = a->seq_len[s];
    ARG_CHECK(len <= kFusedMaxSeq, "seq_len[%d] = %d outside 1..%d", s, len, kFusedMaxSeq);
    // a wave reads 64 whole token rows, whatever its sequence's length
    ARG_CHECK((int64_t)row + 64 * ((len + 63) / 64) <= a->rows, "sequence %d (row %d, %d tokens): its last wave reads past row %d", s, row, len, a->rows);
  }
  if (const int rc = use_device(device); rc != VRAG_OK) return rc;
  const size_t R = (size_t)a->rows, H = (size_t)a->H;
  const bool fold = a->ln_mu != nullptr;
  std::vector<int4> groups((size_t)n * 8);
  const int n_groups = a->packer ? pack_groups_best_fit(a->seq_row, a->seq_len, 0, n, groups.data())
                                 : fused_pack_groups(a->seq_row, a->seq_len, 0, n, groups.data());
  std::memcpy(a->groups_out, groups.data(), (size_t)n_groups * 8 * sizeof(int4));
  a->n_groups = n_groups;

  DbgBufs B;
  bf16_t* w = B.in<bf16_t>(a->w, 3 * H * H, "w");
  float* ls = B.in_opt<float>(fold ? a->ln_s : nullptr, 3 * H, "ln_s");
  bf16_t* wh = B.scratch<bf16_t>(3 * H * H, "wh");
  float* lsh = fold ? B.scratch<float>(3 * H, "lsh", 64 * 4) : nullptr;   // the kernel's 256-float DMA of a head's 192 sums reads 64 floats on (capi.hip)
  QkvAttnParams f{};
  f.x = B.in<bf16_t>(a->x, R * H, "x");
  f.w = wh;
  f.ln_mu = B.in_opt<float>(a->ln_mu, R, "ln_mu");
  f.ln_rstd = B.in_opt<float>(a->ln_rstd, R, "ln_rstd");
  f.ln_s = lsh;
  f.rope_cos = B.in<float>(a->rope_cos, (size_t)a->rope_rows * 32, "rope_cos");
  f.rope_sin = B.in<float>(a->rope_sin, (size_t)a->rope_rows * 32, "rope_sin");
  f.rope_rows = a->rope_rows;
  f.o = B.inout<bf16_t>(a->o, R * H, "o");
  f.groups = B.in<int4>(groups.data(), (size_t)n_groups * 8, "groups");
  f.n_groups = n_groups;
  f.H = (int)H;
  f.nh = a->nh;
  f.Tp = (int)R;
  f.window = a->window;
  f.op_dtype = a->f16 ? kOpF16 : kOpBf16;
  f.q_scale = a->q_scale;
  f.debug_flags = a->debug_flags;
  f.f16_sat = B.clamp_word(&a->f16_saturated);
  hipError_t e = B.err;
  if (e == hipSuccess) e = permute_qkv_heads(w, ls, (int)H, a->nh, wh, lsh, nullptr);
  if (e == hipSuccess) e = B.staged();
  if (e == hipSuccess) e = launch_qkv_attention(f, a->local != 0, 0);
  return B.finish("fused attention", e);
}

int vrag_debug_rows_run(vrag_debug_rows_args* a, int32_t device) {
  ARG_CHECK(a, "null arguments");
  const int op = a->op, H = a->H, rows = a->rows;
  ARG_CHECK(op >= VRAG_DEBUG_ROWS_EMBED_LN && op <= VRAG_DEBUG_ROWS_SEQ_HEAD, "op %d is not a row launcher", op);
  ARG_CHECK(H >= 1 && H <= 65536, "H (%d) outside 1..65536: the buffers cannot be sized", H);
  ARG_CHECK(rows >= 0, "rows (%d) is negative: the buffers cannot be sized", rows);
  ARG_CHECK(a->out_rows >= rows, "out_rows (%d) below rows (%d)", a->out_rows, rows);
  ARG_CHECK(device >= 0, "bad device %d", device);
  const bool embed = op == VRAG_DEBUG_ROWS_EMBED_LN, ln = op == VRAG_DEBUG_ROWS_LAYERNORM, range = op == VRAG_DEBUG_ROWS_RANGE_POOL;
  const bool lncls = op == VRAG_DEBUG_ROWS_LN_CLASSIFIER, pooler = op == VRAG_DEBUG_ROWS_POOLER_CLASSIFIER;
  const bool seqh = op == VRAG_DEBUG_ROWS_SEQ_HEAD;
  const bool classifier = lncls || pooler || seqh || (range && a->mode == 0);
  // every pointer the chosen kernel dereferences unconditionally must be there
  if (embed) {
    ARG_CHECK(a->ids && a->E && a->w && a->out_f32 && a->out16, "embed_ln needs ids, E, w, out_f32 and out16");
    ARG_CHECK(a->vocab >= 1, "vocab (%d) must be positive", a->vocab);
    for (int r = 0; r < rows; ++r) ARG_CHECK(a->ids[r] >= 0 && a->ids[r] < a->vocab, "ids[%d] = %d outside the %d rows of E", r, a->ids[r], a->vocab);
    if (a->P && a->pos) {
      ARG_CHECK(a->n_pos >= 1, "n_pos (%d) must be positive", a->n_pos);
      for (int r = 0; r < rows; ++r) ARG_CHECK(a->pos[r] >= 0 && a->pos[r] < a->n_pos, "pos[%d] = %d outside the %d rows of P", r, a->pos[r], a->n_pos);
    }
    if (a->P && a->type_row) {
      ARG_CHECK(a->n_types >= 1, "n_types (%d) must be positive", a->n_types);
      if (a->type_ids)
        for (int r = 0; r < rows; ++r)
          ARG_CHECK(a->type_ids[r] >= 0 && a->type_ids[r] < a->n_types, "type_ids[%d] = %d outside the %d rows of type_row", r, a->type_ids[r], a->n_types);
    }
  } else {
    ARG_CHECK(a->h, "h is required");
    ARG_CHECK(a->h_rows >= 1, "h_rows (%d) must be positive", a->h_rows);
  }
  if (ln || lncls) ARG_CHECK(a->h_rows >= rows, "h holds %d rows, the launch reads %d", a->h_rows, rows);
  if (ln) ARG_CHECK(!(a->alias_f32 && a->out_f32), "alias_f32 makes h the fp32 output: out_f32 must be null");
  if (range) {
    ARG_CHECK(a->start && a->end && a->out_f32, "range_pool needs start, end and out_f32");
    for (int r = 0; r < rows; ++r) {
      ARG_CHECK(a->start[r] >= 0, "start[%d] = %d is negative", r, a->start[r]);
      ARG_CHECK(a->end[r] < a->h_rows, "end[%d] = %d is past the last row %d of h (end is inclusive)", r, a->end[r], a->h_rows - 1);
      ARG_CHECK(a->start[r] <= a->end[r], "range %d is empty (start %d > end %d): the kernel would divide by zero", r, a->start[r], a->end[r]);
    }
  }
  if (lncls) ARG_CHECK(a->w && a->out_f32, "ln_classifier needs w and out_f32");
  if (pooler) {
    ARG_CHECK(a->first_row && a->Wp && a->bp && a->out_f32, "pooler_classifier needs first_row, Wp, bp and out_f32");
    for (int r = 0; r < rows; ++r)
      ARG_CHECK(a->first_row[r] >= 0 && a->first_row[r] < a->h_rows, "first_row[%d] = %d outside the %d rows of h", r, a->first_row[r], a->h_rows);
  }
  if (seqh) {
    ARG_CHECK(a->seq_row && a->seq_len && a->pooled && a->WdT && a->wn && a->out_f32, "seq_head needs seq_row, seq_len, pooled, WdT, wn and out_f32");
    for (int r = 0; r < rows; ++r) {
      ARG_CHECK(a->seq_len[r] >= 1, "seq_len[%d] = %d must be at least 1", r, a->seq_len[r]);
      ARG_CHECK(a->seq_row[r] >= 0, "seq_row[%d] = %d is negative", r, a->seq_row[r]);
      ARG_CHECK((int64_t)a->seq_row[r] + a->seq_len[r] <= a->h_rows, "sequence %d (row %d, %d tokens) ends past the %d rows of h", r, a->seq_row[r], a->seq_len[r], a->h_rows);
    }
  }
  if (classifier) {
    ARG_CHECK(a->num_labels >= 1, "num_labels (%d) must be at least 1 where a classifier runs", a->num_labels);
    ARG_CHECK(a->Wc && a->bc, "the classifier needs Wc and bc");
  }
  if (const int rc = use_device(device); rc != VRAG_OK) return rc;

  // device copies (DbgBufs): what the chosen launcher does not take, and an absent optional buffer, stay null pointers
  const size_t R = (size_t)rows, OR = (size_t)a->out_rows, Hs = (size_t)H, L = (size_t)std::max(a->num_labels, 0);
  const size_t out_cols = (embed || ln || (range && a->mode != 0)) ? Hs : L;
  const bool alias = ln && a->alias_f32;   // h is the fp32 output too: in / out
  DbgBufs B;
  float* h = embed ? nullptr : alias ? B.inout<float>(a->h, (size_t)a->h_rows * Hs, "h") : B.in<float>(a->h, (size_t)a->h_rows * Hs, "h");
  int* ids = embed ? B.in_opt<int>(a->ids, R, "ids") : nullptr;
  float* E = embed ? B.in_opt<float>(a->E, (size_t)a->vocab * Hs, "E") : nullptr;
  float* P = embed ? B.in_opt<float>(a->P, (size_t)std::max(a->n_pos, 0) * Hs, "P") : nullptr;
  int* pos = embed ? B.in_opt<int>(a->pos, R, "pos") : nullptr;
  float* type_row = embed ? B.in_opt<float>(a->type_row, (size_t)std::max(a->n_types, 0) * Hs, "type_row") : nullptr;
  int* type_ids = embed ? B.in_opt<int>(a->type_ids, R, "type_ids") : nullptr;
  float* w = B.in_opt<float>(a->w, Hs, "w");
  float* bias = B.in_opt<float>(a->bias, Hs, "bias");
  int* start = range ? B.in_opt<int>(a->start, R, "start") : nullptr;
  int* end = range ? B.in_opt<int>(a->end, R, "end") : nullptr;
  int* first_row = pooler ? B.in_opt<int>(a->first_row, R, "first_row") : nullptr;
  int* seq_row = seqh ? B.in_opt<int>(a->seq_row, R, "seq_row") : nullptr;
  int* seq_len = seqh ? B.in_opt<int>(a->seq_len, R, "seq_len") : nullptr;
  float* Wp = pooler ? B.in_opt<float>(a->Wp, Hs * Hs, "Wp") : nullptr;
  float* bp = pooler ? B.in_opt<float>(a->bp, Hs, "bp") : nullptr;
  float* WdT = seqh ? B.in_opt<float>(a->WdT, Hs * Hs, "WdT") : nullptr;
  float* bd = seqh ? B.in_opt<float>(a->bd, Hs, "bd") : nullptr;
  float* wn = seqh ? B.in_opt<float>(a->wn, Hs, "wn") : nullptr;
  float* bn = seqh ? B.in_opt<float>(a->bn, Hs, "bn") : nullptr;
  float* Wc = B.in_opt<float>(a->Wc, L * Hs, "Wc");
  float* bc = B.in_opt<float>(a->bc, L, "bc");
  float* out_f32 = B.inout_opt<float>(a->out_f32, OR * out_cols, "out_f32");
  bf16_t* out16 = (embed || ln) ? B.inout_opt<bf16_t>(a->out16, OR * (ln && a->split3 ? 3 * Hs : Hs), "out16") : nullptr;
  bf16_t* out_lo = ln ? B.inout_opt<bf16_t>(a->out_lo, OR * Hs, "out_lo") : nullptr;
  float* row_mean = ln ? B.inout_opt<float>(a->row_mean, OR, "row_mean") : nullptr;
  float* pooled = seqh ? B.inout_opt<float>(a->pooled, OR * Hs, "pooled") : nullptr;
  unsigned* sat = B.clamp_word(&a->f16_saturated);
  if (B.staged() != hipSuccess) return B.finish("rows", B.err);
  const int dt = a->f16 ? kOpF16 : kOpBf16;
  unsigned* satp = a->no_sat ? nullptr : sat;
  hipError_t le = hipSuccess;
  switch (op) {
    case VRAG_DEBUG_ROWS_EMBED_LN:
      le = launch_embed_ln(ids, E, w, a->eps, H, rows, out_f32, out16, 0, P, pos, type_row, bias, type_ids, dt, satp);
      break;
    case VRAG_DEBUG_ROWS_LAYERNORM:
      le = launch_layernorm(h, w, a->eps, H, rows, out16, alias ? h : out_f32, 0, bias, row_mean, dt, out_lo, a->gelu_first, a->split3, satp);
      break;
    case VRAG_DEBUG_ROWS_RANGE_POOL:
      le = launch_range_pool(h, w, a->eps, H, start, end, rows, a->mode, Wc, bc, a->num_labels, out_f32, 0);
      break;
    case VRAG_DEBUG_ROWS_LN_CLASSIFIER:
      le = launch_ln_classifier(h, w, a->eps, H, rows, Wc, bc, a->num_labels, out_f32, 0, bias, a->gelu_first);
      break;
    case VRAG_DEBUG_ROWS_POOLER_CLASSIFIER:
      le = launch_pooler_classifier(h, H, first_row, rows, Wp, bp, Wc, bc, a->num_labels, out_f32, 0);
      break;
    default:
      le = launch_seq_head(h, w, a->eps, H, seq_row, seq_len, rows, a->mode, pooled, WdT, bd, wn, bn, Wc, bc, a->num_labels, out_f32, 0);
      break;
  }
  a->launch_status = (int32_t)le;
  // the device is synchronised and the canaries are checked whatever the launcher said: its refusal must have touched nothing
  if (const int rc = B.finish("rows", hipSuccess); rc != VRAG_OK) return rc;
  if (le != hipSuccess) {
    set_error("debug rows run: the launcher returned %s", hipGetErrorString(le));
    return le == hipErrorInvalidValue ? VRAG_ERR_INVALID : VRAG_ERR_HIP;
  }
  return VRAG_OK;
}

int vrag_debug_glue_run(vrag_debug_glue_args* a, int32_t device) {
  ARG_CHECK(a, "null arguments");
  const int op = a->op;
  ARG_CHECK(op >= VRAG_DEBUG_GLUE_CVT_ROWS && op <= VRAG_DEBUG_GLUE_PERMUTE_QKV_HEADS, "op %d is not a glue launcher", op);
  ARG_CHECK(device >= 0, "bad device %d", device);
  const bool cvt = op == VRAG_DEBUG_GLUE_CVT_ROWS, split3 = op == VRAG_DEBUG_GLUE_CVT_SPLIT3;
  const bool fin = op == VRAG_DEBUG_GLUE_LN_STATS_FINALIZE, pack = op == VRAG_DEBUG_GLUE_PACK_LAYOUT;
  const bool compact = op == VRAG_DEBUG_GLUE_SPLADE_COMPACT, permute = op == VRAG_DEBUG_GLUE_PERMUTE_QKV_HEADS;
  constexpr int kMax = 1 << 20;            // every extent, and
  constexpr int64_t kMaxElems = 1 << 28;   // every buffer's element count: the sizes below stay far inside size_t and int
  if (cvt || split3) {
    ARG_CHECK(a->src && a->dst, "%s needs src and dst", cvt ? "cvt_rows" : "cvt_split3");
    ARG_CHECK(a->rows_src > 0 && a->rows_src <= kMax, "rows_src (%d) must be in 1..%d", a->rows_src, kMax);
    ARG_CHECK(a->cols > 0 && a->cols <= kMax, "cols (%d) must be in 1..%d", a->cols, kMax);
    ARG_CHECK(a->rows_dst > 0 && a->rows_dst <= kMax, "rows_dst (%d) must be in 1..%d", a->rows_dst, kMax);
    ARG_CHECK(a->out_rows >= a->rows_dst && a->out_rows <= kMax, "out_rows (%d) below rows_dst (%d)", a->out_rows, a->rows_dst);
    ARG_CHECK((int64_t)a->rows_src * a->cols <= kMaxElems && (int64_t)a->out_rows * a->cols * 3 <= kMaxElems, "the matrices are too large for the hook");
    if (cvt && a->interleave) ARG_CHECK(a->I > 0, "interleave: I (%d) must be positive", a->I);
  }
  if (fin) {
    ARG_CHECK(a->part && a->mu && a->rstd && a->shift_out, "ln_stats_finalize needs part, mu, rstd and shift_out");
    ARG_CHECK(!(a->alias_shift && a->shift_in), "alias_shift makes shift_out the kernel's shift_in: shift_in must be null");
    ARG_CHECK(a->rows > 0 && a->rows <= kMax, "rows (%d) must be in 1..%d", a->rows, kMax);
    ARG_CHECK(a->np > 0 && a->H > 0 && (int64_t)a->np * 64 == a->H, "np (%d) * 64 must be H (%d)", a->np, a->H);
    ARG_CHECK(a->row0 >= 0 && a->ld <= kMax && (int64_t)a->ld >= (int64_t)a->row0 + a->rows,
              "ld (%d) below row0 + rows (%d + %d)", a->ld, a->row0, a->rows);
    ARG_CHECK((int64_t)a->np * a->ld * 2 <= kMaxElems, "the partials are too large for the hook");
  }
  if (pack) {
    ARG_CHECK(a->packed && a->seq_row && a->seq_src && a->seq_len && a->ids && a->pos && a->tok_seq,
              "pack_layout needs packed, seq_row, seq_src, seq_len, ids, pos and tok_seq");
    ARG_CHECK(a->n_seqs >= 1 && a->n_seqs <= kMax, "n_seqs (%d) must be in 1..%d", a->n_seqs, kMax);
    ARG_CHECK(a->rows > 0 && a->rows <= kMax, "rows (%d) must be in 1..%d", a->rows, kMax);
    ARG_CHECK(a->out_rows >= a->rows && a->out_rows <= kMax, "out_rows (%d) below rows (%d)", a->out_rows, a->rows);
    ARG_CHECK(a->n_packed >= 1 && a->n_packed <= (1 << 26), "n_packed (%d) must be in 1..2^26", a->n_packed);
    for (int i = 0; i < a->n_seqs; ++i) {
      ARG_CHECK(a->seq_row[i] >= 0, "seq_row[%d] = %d is negative", i, a->seq_row[i]);
      ARG_CHECK(i == 0 || a->seq_row[i] > a->seq_row[i - 1], "seq_row is not ascending at %d (%d after %d)", i, a->seq_row[i], a->seq_row[i - 1]);
      ARG_CHECK(a->seq_len[i] >= 0, "seq_len[%d] = %d is negative", i, a->seq_len[i]);
      ARG_CHECK((int64_t)a->seq_row[i] + a->seq_len[i] <= a->rows, "sequence %d (row %d, %d tokens) runs past rows (%d)", i, a->seq_row[i], a->seq_len[i], a->rows);
      ARG_CHECK(a->seq_src[i] >= 0 && (int64_t)a->seq_src[i] + a->seq_len[i] <= a->n_packed,
                "sequence %d: seq_src + seq_len (%d + %d) beyond the %d packed ids", i, a->seq_src[i], a->seq_len[i], a->n_packed);
    }
  }
  if (compact) {
    ARG_CHECK(a->src && a->counts && a->idx && a->val, "splade_compact needs src, counts, idx and val");
    ARG_CHECK(a->V > 0 && a->V <= kMax, "V (%d) must be in 1..%d", a->V, kMax);
    ARG_CHECK(a->ld % 4 == 0 && a->ld <= kMax && a->ld >= (int)align_up(a->V, 4), "ld (%d) must be a multiple of 4 and at least V (%d) rounded up to 4", a->ld, a->V);
    ARG_CHECK(a->cap >= 1 && a->cap <= kMax, "cap (%d) must be in 1..%d", a->cap, kMax);
    ARG_CHECK(a->rows > 0 && a->rows <= 4096, "rows (%d) must be in 1..4096", a->rows);
    ARG_CHECK(a->out_rows >= a->rows && a->out_rows <= 4096, "out_rows (%d) below rows (%d)", a->out_rows, a->rows);
    ARG_CHECK((int64_t)a->rows * a->ld <= kMaxElems && (int64_t)a->out_rows * a->cap <= kMaxElems, "the rows are too large for the hook");
  }
  if (permute) {
    ARG_CHECK(a->w && a->w_out, "permute_qkv_heads needs w and w_out");
    ARG_CHECK(!a->s == !a->s_out, "s and s_out come together");
    ARG_CHECK(a->nh >= 1 && a->nh <= 64 && a->H == 64 * a->nh, "H (%d) must be 64 * nh (%d), nh in 1..64", a->H, a->nh);
    ARG_CHECK(a->out_rows >= 3 * a->H && a->out_rows <= kMax, "out_rows (%d) below 3 H (%d)", a->out_rows, 3 * a->H);
  }
  if (const int rc = use_device(device); rc != VRAG_OK) return rc;

  // device copies (DbgBufs), staged by the case that launches on them; an absent optional buffer stays a null pointer
  const size_t OR = (size_t)a->out_rows, cols = (size_t)a->cols, ld = (size_t)a->ld, Hs = (size_t)a->H;
  const int dt = a->f16 ? kOpF16 : kOpBf16;
  DbgBufs B;
  unsigned* sat = B.clamp_word(&a->f16_saturated);
  switch (op) {
    case VRAG_DEBUG_GLUE_CVT_ROWS: {
      const float* src = B.in<float>(a->src, (size_t)a->rows_src * cols, "src");
      bf16_t* dst = B.inout<bf16_t>(a->dst, OR * cols, "dst");
      const float* scale = B.in_opt<float>(a->col_scale, cols, "col_scale");
      bf16_t* dst_lo = B.inout_opt<bf16_t>(a->dst_lo, OR * cols, "dst_lo");
      float* row_sum = B.inout_opt<float>(a->row_sum, OR, "row_sum");
      if (B.staged() == hipSuccess)
        launch_cvt_rows(dt, dim3(a->rows_dst), 0, src, dst, a->rows_dst, a->rows_src, a->cols, a->interleave ? a->I : 0, scale, row_sum, dst_lo, sat);
      break;
    }
    case VRAG_DEBUG_GLUE_CVT_SPLIT3: {
      const float* src = B.in<float>(a->src, (size_t)a->rows_src * cols, "src");
      bf16_t* dst = B.inout<bf16_t>(a->dst, OR * 3 * cols, "dst");
      if (B.staged() == hipSuccess) launch_cvt_split3(dt, 0, src, dst, a->rows_dst, a->rows_src, a->cols, sat);
      break;
    }
    case VRAG_DEBUG_GLUE_LN_STATS_FINALIZE: {
      const size_t r0 = (size_t)a->row0;   // as the encoder addresses a micro-batch
      const float* part = B.in<float>(a->part, (size_t)a->np * ld * 2, "part");
      float* mu = B.inout<float>(a->mu, ld, "mu");
      float* rstd = B.inout<float>(a->rstd, ld, "rstd");
      const float* shift_in = B.in_opt<float>(a->shift_in, ld, "shift_in");
      float* shift_out = B.inout<float>(a->shift_out, ld, "shift_out");
      float* prev = B.inout_opt<float>(a->shift_prev, ld, "shift_prev");
      if (B.staged() == hipSuccess)
        launch_ln_stats_finalize(0, part + r0 * 2, a->ld, a->np, a->H, a->eps, a->rows, mu + r0, rstd + r0,
                                 a->alias_shift ? shift_out + r0 : at(shift_in, r0), shift_out + r0, at(prev, r0));
      break;
    }
    case VRAG_DEBUG_GLUE_PACK_LAYOUT: {
      const size_t n = (size_t)a->n_seqs;
      const int* packed = B.in<int>(a->packed, (size_t)a->n_packed, "packed");
      const int* seq_row = B.in<int>(a->seq_row, n, "seq_row");
      const int* seq_src = B.in<int>(a->seq_src, n, "seq_src");
      const int* seq_len = B.in<int>(a->seq_len, n, "seq_len");
      int* ids = B.inout<int>(a->ids, OR, "ids");
      int* pos = B.inout<int>(a->pos, OR, "pos");
      int* tok_seq = B.inout<int>(a->tok_seq, OR, "tok_seq");
      if (B.staged() == hipSuccess) launch_pack_layout(0, packed, seq_row, seq_src, seq_len, a->n_seqs, a->rows, a->pad_id, ids, pos, tok_seq);
      break;
    }
    case VRAG_DEBUG_GLUE_SPLADE_COMPACT: {
      const float* src = B.in<float>(a->src, (size_t)a->rows * ld, "src");
      int* counts = B.inout<int>(a->counts, OR, "counts");
      int* idx = B.inout<int>(a->idx, OR * (size_t)a->cap, "idx");
      float* val = B.inout<float>(a->val, OR * (size_t)a->cap, "val");
      if (B.staged() == hipSuccess) launch_splade_compact(0, src, a->rows, a->V, a->ld, a->thr, a->cap, counts, idx, val);
      break;
    }
    default: {
      const bf16_t* w = B.in<bf16_t>(a->w, 3 * Hs * Hs, "w");
      const float* s = B.in_opt<float>(a->s, 3 * Hs, "s");
      bf16_t* w_out = B.inout<bf16_t>(a->w_out, OR * Hs, "w_out");
      float* s_out = B.inout_opt<float>(a->s_out, OR, "s_out");
      if (B.staged() == hipSuccess) (void)permute_qkv_heads(w, s, a->H, a->nh, w_out, s_out, nullptr);
      break;
    }
  }
  return B.finish("glue", B.err != hipSuccess ? B.err : hipGetLastError());   // the launchers return nothing
}

int vrag_debug_topk_run(vrag_debug_topk_args* a, int32_t device) {
  ARG_CHECK(a, "null arguments");
  const int op = a->op;
  ARG_CHECK(op >= VRAG_DEBUG_TOPK_SCORE_STAGE && op <= VRAG_DEBUG_TOPK_TAU, "op %d is not a tiled search launcher", op);
  ARG_CHECK(device >= 0, "bad device %d", device);
  const bool stage = op == VRAG_DEBUG_TOPK_SCORE_STAGE, queries = op == VRAG_DEBUG_TOPK_QUERIES, sel = op == VRAG_DEBUG_TOPK_SELECT;
  const bool seld = op == VRAG_DEBUG_TOPK_SELECT_DIRECT, rescue = op == VRAG_DEBUG_TOPK_RESCUE, merge = op == VRAG_DEBUG_TOPK_MERGE;
  const bool tau = op == VRAG_DEBUG_TOPK_TAU;
  constexpr int kMax = 1 << 20;            // every extent, and
  constexpr int64_t kMaxElems = 1 << 26;   // every buffer's element count: the sizes below stay far inside size_t and int
  ARG_CHECK(a->nq >= 1 && a->nq <= 4096, "nq (%d) must be in 1..4096", a->nq);
  ARG_CHECK(a->nq_buf >= a->nq && a->nq_buf <= 8192, "nq_buf (%d) below nq (%d)", a->nq_buf, a->nq);
  if (!queries && !tau) ARG_CHECK(a->k >= 1 && a->k <= 64, "k (%d) must be in 1..64", a->k);
  if (stage || sel || seld) {
    ARG_CHECK(a->buf && a->cnt && a->thr_key && a->thr_score, "%s needs buf, cnt, thr_key and thr_score", stage ? "score_stage" : "the selection");
    ARG_CHECK(a->cap >= 2 && a->cap <= kMax, "cap (%d) must be in 2..%d", a->cap, kMax);
    ARG_CHECK(a->k <= a->cap, "k (%d) above cap (%d)", a->k, a->cap);
    ARG_CHECK((int64_t)a->nq_buf * a->cap <= kMaxElems, "the candidate buffers are too large for the hook");
  }
  int bm = 256;   // rows of the tile configuration the score stage takes (launch_t of csrc/gemm_bf16.hip)
  if (stage) {
    ARG_CHECK(a->corpus && a->w, "score_stage needs corpus and w");
    ARG_CHECK(a->K >= 64 && a->K <= 4096 && a->K % 64 == 0, "K (%d) must be a multiple of 64 in 64..4096", a->K);
    ARG_CHECK((a->tile == 2 && a->N == 64) || (a->tile == 1 && a->N == 128) || (a->tile == 0 && a->N >= 256 && a->N <= 4096 && a->N % 256 == 0),
              "N (%d) must be 64 with tile 2, 128 with tile 1 or a multiple of 256 up to 4096 with tile 0 (tile %d)", a->N, a->tile);
    ARG_CHECK((a->pairs ? 2 * a->nq : a->nq) <= a->N, "%d query columns (nq %d%s) above N (%d)", a->pairs ? 2 * a->nq : a->nq, a->nq, a->pairs ? ", pairs" : "", a->N);
    ARG_CHECK(a->M >= 1 && a->M <= kMax, "M (%d) must be in 1..%d", a->M, kMax);
    ARG_CHECK(a->corpus_rows >= 1 && a->corpus_rows <= kMax && (int64_t)(a->corpus_rows + 255) * a->K <= kMaxElems,
              "corpus_rows (%d) must be positive and the corpus fit the hook", a->corpus_rows);
    ARG_CHECK(!a->direct || a->cap >= a->M, "direct mode: cap (%d) below M (%d)", a->cap, a->M);
    if (!a->direct)
      for (int q = 0; q < a->nq; ++q) ARG_CHECK(a->cnt[q] <= (uint32_t)a->cap, "cnt[%d] = %u is the carry and exceeds cap (%d)", q, a->cnt[q], a->cap);
    const int thr = a->small_rows >= 0 ? a->small_rows : gemm_small_m_threshold(-1);
    if (a->tile != 2) bm = a->M <= thr ? 128 : ((a->tile == 1 || a->N % 256 == 0) && a->M >= 256 ? 256 : 128);
    const bool stride = a->tile_stride > 1, skip = a->tile_skip > 1;
    const int64_t pad_tiles = ((int64_t)a->corpus_rows + 255) / 256, whole_tiles = a->corpus_rows / 256;
    ARG_CHECK(a->tile_stride >= 0 && a->tile_skip >= 0 && a->tile_stride <= kMax && a->tile_skip <= kMax, "negative or huge stride / skip (%d / %d)", a->tile_stride, a->tile_skip);
    if (stride || skip) {
      ARG_CHECK(!(stride && skip), "stride (%d) and skip (%d) do not come together", a->tile_stride, a->tile_skip);
      ARG_CHECK(a->M % 256 == 0, "stride / skip with M (%d) not a multiple of 256", a->M);
      ARG_CHECK(!stride || a->direct, "stride (%d) belongs to the direct stage", a->tile_stride);
      ARG_CHECK(!skip || !a->direct, "skip (%d) belongs to the appending stages", a->tile_skip);
      ARG_CHECK(!(a->tile == 0 && a->N > 256 && 256 % (a->N / 256) != 0), "stride / skip with %d column tiles: no whole round", a->N / 256);
      ARG_CHECK(bm == 256, "stride / skip on a launch that takes the 128-row tiles (M %d <= the small-batch threshold %d)", a->M, thr);
      const int64_t T = a->M / 256;
      if (stride) ARG_CHECK((T - 1) * a->tile_stride < whole_tiles, "stride %d: launch tile %lld reads corpus tile %lld of %lld", a->tile_stride, (long long)(T - 1), (long long)((T - 1) * a->tile_stride), (long long)whole_tiles);
      if (skip) {
        ARG_CHECK(a->tile0 >= 0 && a->tile0 <= kMax, "tile0 (%d) must be in 0..%d", a->tile0, kMax);
        const int64_t d = (int64_t)a->tile0 + T - 1, s1 = a->tile_skip - 1, ct = d < 256 * s1 ? d + d / s1 + 1 : d + 256;
        ARG_CHECK(ct < whole_tiles, "skip %d, tile0 %d: launch tile %lld reads corpus tile %lld of %lld", a->tile_skip, a->tile0, (long long)(T - 1), (long long)ct, (long long)whole_tiles);
      }
    } else {
      ARG_CHECK((int64_t)a->row_base + a->M <= a->corpus_rows, "row_base + M (%u + %d) beyond corpus_rows (%d)", a->row_base, a->M, a->corpus_rows);
      const int64_t last = (int64_t)a->row_base + ((int64_t)a->M + bm - 1) / bm * bm;   // whole tiles of bm rows are read
      ARG_CHECK(last <= pad_tiles * 256, "the launch reads rows up to %lld of a corpus padded to %lld", (long long)last, (long long)(pad_tiles * 256));
    }
  }
  if (queries) {
    ARG_CHECK(a->queries && a->w_out, "queries needs queries and w_out");
    ARG_CHECK(a->K >= 1 && a->K <= 4096, "K (%d) must be in 1..4096", a->K);
    ARG_CHECK(a->N >= 1 && a->N <= 4096, "N (%d) must be in 1..4096", a->N);
    ARG_CHECK((a->pairs ? 2 * a->nq : a->nq) <= a->N, "%d query columns above N (%d)", a->pairs ? 2 * a->nq : a->nq, a->N);
  }
  if (sel || seld) {
    ARG_CHECK(a->ovf, "the selection needs ovf");
    ARG_CHECK((a->cap & (a->cap - 1)) == 0 && a->cap <= kTiledSelectMaxCap, "the selection sorts in LDS: cap (%d) must be a power of two up to %d", a->cap, kTiledSelectMaxCap);
  }
  if (seld) {
    ARG_CHECK(a->src, "select_direct needs src");
    ARG_CHECK(a->n >= 1 && a->n <= kMax, "n (%d) must be in 1..%d", a->n, kMax);
    ARG_CHECK(a->n <= a->src_stride && a->src_stride <= kMax, "n (%d) above src_stride (%d)", a->n, a->src_stride);
    ARG_CHECK((int64_t)a->nq * a->src_stride <= kMaxElems, "src is too large for the hook");
    int first = std::min(a->n, a->k > 16 ? 1024 : 256), P = 2;
    while (P < first) P <<= 1;
    ARG_CHECK(P <= a->cap, "select_direct: cap (%d) below the first window (%d keys)", a->cap, P);
  }
  if (rescue) {
    ARG_CHECK(a->corpus && a->queries && a->ovf && a->done && a->out, "rescue needs corpus, queries, ovf, done and out");
    ARG_CHECK(a->K >= 64 && a->K <= 4096 && a->K % 64 == 0, "rescue: dim (%d) must be a multiple of 64 in 64..4096", a->K);
    ARG_CHECK(a->n >= 1 && a->n <= kMax && (int64_t)a->n * a->K <= kMaxElems, "rescue: n_rows (%d) must be positive and the rows fit the hook", a->n);
    ARG_CHECK(a->corpus_rows == a->n, "rescue: corpus_rows (%d) must be n_rows (%d)", a->corpus_rows, a->n);
    ARG_CHECK(a->slices >= 8 && a->slices <= kTiledRescueMaxSlices, "rescue: slices (%d) must be in 8..%d", a->slices, kTiledRescueMaxSlices);
  }
  if (merge) {
    ARG_CHECK(a->src && a->out, "merge needs src and out");
    ARG_CHECK(a->n >= 1 && a->n <= kMax && (int64_t)a->n * a->nq * a->k <= kMaxElems, "merge: %d lists must be positive and fit the hook", a->n);
  }
  if (tau) ARG_CHECK(a->thr_key && a->thr_score && a->eps && a->cnt && a->ovf, "tau needs thr_key, thr_score, eps, cnt and ovf");
  if (const int rc = use_device(device); rc != VRAG_OK) return rc;

  // device copies (DbgBufs): what the chosen launcher does not take, and an absent optional buffer, stay null pointers
  const size_t NB = (size_t)a->nq_buf, K = (size_t)a->K, k = (size_t)a->k, cap = (size_t)a->cap, nq = (size_t)a->nq;
  const size_t rows = (size_t)std::max(a->corpus_rows, 0), padded = (rows + 255) / 256 * 256;   // the last 256-row tile is read whole: zeros
  DbgBufs B;
  u64* part = rescue ? B.scratch<u64>((size_t)a->slices * nq * k, "part") : nullptr;   // the rescue's per-slice lists [slices][nq][k]
  bf16_t* corpus = (stage || rescue) ? B.in<bf16_t>(a->corpus, rows * K, "corpus", (padded - rows) * K * 2) : nullptr;
  bf16_t* w = stage ? B.in_opt<bf16_t>(a->w, (size_t)a->N * K, "w") : nullptr;
  float* queries_d = (queries || rescue) ? B.in_opt<float>(a->queries, nq * K, "queries") : nullptr;
  bf16_t* w_out = queries ? B.inout_opt<bf16_t>(a->w_out, (size_t)a->N * K, "w_out") : nullptr;
  u64* src = (seld || merge) ? B.in_opt<u64>(a->src, seld ? nq * (size_t)a->src_stride : (size_t)a->n * nq * k, "src") : nullptr;
  u64* buf = (stage || sel || seld) ? B.inout_opt<u64>(a->buf, NB * cap, "buf") : nullptr;
  const bool has_thr = stage || sel || seld || tau;
  unsigned* cnt = has_thr ? B.inout_opt<unsigned>(a->cnt, NB, "cnt") : nullptr;
  u64* thr_key = has_thr ? B.inout_opt<u64>(a->thr_key, NB, "thr_key") : nullptr;
  float* thr_score = has_thr ? B.inout_opt<float>(a->thr_score, NB, "thr_score") : nullptr;
  u64* out = (sel || seld || rescue || merge) ? B.inout_opt<u64>(a->out, NB * k, "out") : nullptr;
  unsigned* ovf = (sel || seld || rescue || tau) ? B.inout_opt<unsigned>(a->ovf, NB, "ovf") : nullptr;
  float* eps = tau ? B.in_opt<float>(a->eps, nq, "eps") : nullptr;
  unsigned* done = rescue ? B.inout_opt<unsigned>(a->done, NB, "done") : nullptr;
  hipError_t e = B.staged();
  if (e != hipSuccess) return B.finish("topk", e);
  switch (op) {
    case VRAG_DEBUG_TOPK_SCORE_STAGE: {
      GemmParams g{};
      g.op_dtype = kOpBf16;
      const bool mapped = a->tile_stride > 1 || a->tile_skip > 1;   // as dense_tiled_search: the map starts at the shard's first row
      g.A = corpus + (mapped ? (size_t)0 : (size_t)a->row_base * K);
      g.W = w;
      g.M = a->M;
      g.N = a->N;
      g.K = a->K;
      g.topk_thr_score = thr_score;
      g.topk_thr_key = thr_key;
      g.topk_cnt = cnt;
      g.topk_buf = buf;
      g.topk_cap = a->cap;
      g.topk_nq = a->nq;
      g.topk_pairs = a->pairs;
      g.topk_direct = a->direct;
      g.topk_row_base = a->row_base;
      g.topk_tile = a->tile;
      g.topk_tile_stride = a->tile_stride;
      g.topk_tile_skip = a->tile_skip;
      g.topk_tile0 = a->tile0;
      const int thr = gemm_small_m_threshold(-1);
      if (a->small_rows >= 0) gemm_small_m_threshold(a->small_rows);
      e = launch_gemm(EPI_TOPK, g, 0);
      const GemmConfig c = gemm_last_config();
      gemm_small_m_threshold(thr);
      const int32_t cfg[7] = {c.bm, c.bn, c.wm, c.wn, c.ns, c.hw, c.kch};
      std::memcpy(a->config, cfg, sizeof(cfg));
      if (e == hipSuccess && c.bm != bm) {   // the bounds above were worked out for another tile form: nothing may rest on them
        (void)hipDeviceSynchronize();
        set_error("debug topk run: the launch took %d-row tiles, the hook expected %d", c.bm, bm);
        return VRAG_ERR_HIP;
      }
      break;
    }
    case VRAG_DEBUG_TOPK_QUERIES:
      e = launch_tiled_queries(queries_d, a->nq, a->K, a->pairs, a->N, w_out, 0);
      break;
    case VRAG_DEBUG_TOPK_SELECT:
      e = launch_tiled_select(buf, cnt, a->cap, a->k, thr_key, thr_score, out, ovf, 0, a->nq, 0);
      break;
    case VRAG_DEBUG_TOPK_SELECT_DIRECT:
      e = launch_tiled_select_direct(src, a->src_stride, a->n, buf, cnt, a->cap, a->k, thr_key, thr_score, out, ovf, a->nq, 0);
      break;
    case VRAG_DEBUG_TOPK_RESCUE:
      e = launch_dense_tiled_rescue(corpus, (long long)a->n, a->K, queries_d, a->nq, a->k, ovf, part, done, out, a->slices, 0);
      break;
    case VRAG_DEBUG_TOPK_MERGE:
      e = launch_topk_merge(src, a->n, a->nq, a->k, out, 0);
      break;
    default:
      e = launch_tiled_tau(a->nq, thr_key, thr_score, eps, cnt, ovf, 0);
      break;
  }
  const int rc = B.finish("topk", e);
  return rc == VRAG_ERR_HIP && e == hipErrorInvalidValue ? VRAG_ERR_INVALID : rc;   // a launcher's refusal
}

int vrag_debug_canary_selftest(int32_t touch, int32_t device) {
  ARG_CHECK(touch >= 0 && touch <= 3, "touch (%d) must be in 0..3", touch);
  if (const int rc = use_device(device); rc != VRAG_OK) return rc;
  unsigned char ha[64], hb[100], want[100];
  for (int i = 0; i < 100; ++i) want[i] = hb[i] = (unsigned char)(i * 7 + 1);
  std::memset(ha, 0x11, sizeof(ha));
  constexpr size_t kPad = 28;
  DbgBufs B;
  B.in<unsigned char>(ha, sizeof(ha), "a");
  unsigned char* b = B.inout<unsigned char>(hb, sizeof(hb), "b", kPad);
  B.scratch<unsigned>(0, "c");
  hipError_t e = B.staged();
  std::memset(hb, 0, sizeof(hb));   // finish() brings the staged bytes back
  // a host-issued write of one byte inside b's own allocation: its first / last canary byte, or its last pad byte
  const size_t at_byte[4] = {0, sizeof(hb) + kPad, sizeof(hb) + kPad + DbgBufs::kCanary - 1, sizeof(hb) + kPad - 1};
  if (e == hipSuccess && touch) e = hipMemset(b + at_byte[touch], 0, 1);
  const int rc = B.finish("canary selftest", e);
  if (rc == VRAG_OK && std::memcmp(hb, want, sizeof(hb)) != 0) {
    set_error("debug canary selftest run: b came back changed");
    return VRAG_ERR_HIP;
  }
  return rc;
}

int vrag_debug_token_spans(const float* logits, int64_t n_tokens, const int32_t* win_job, const int32_t* win_a, const int32_t* win_b,
                           const int32_t* win_first, int32_t n_windows, const int64_t* job_off, const int32_t* offsets, int32_t n_jobs, float tau,
                           int32_t min_span_chars, int32_t merge_gap_chars, int32_t cap_per_job, int32_t* counts, int32_t* spans, int32_t device) {
  ARG_CHECK(n_tokens >= 0 && n_tokens < 0x7FFFFFF0ll && (logits || n_tokens == 0), "vrag_debug_token_spans: bad logits");
  HIP_TRY(hipSetDevice(device));
  DevBuf dl;
  HIP_TRY(dl.alloc((size_t)n_tokens * 2 * sizeof(float)));
  if (n_tokens) HIP_TRY(hipMemcpy(dl.p, logits, (size_t)n_tokens * 2 * sizeof(float), hipMemcpyHostToDevice));
  TokenSpanScratch ws;
  return run_token_spans(ws, dl.as<float>(), n_tokens, win_job, win_a, win_b, win_first, n_windows, job_off, offsets, n_jobs, tau,
                         min_span_chars, merge_gap_chars, cap_per_job, counts, spans, nullptr);
}

}  // extern "C"
