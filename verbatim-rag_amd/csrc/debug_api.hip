// Tuning / unit-test harness of the kernels (include/vrag_amd_debug.h): synthetic-operand timing loops and the attention
// kernels', the GEMM's, the row kernels', the packing / glue kernels' and the tiled search kernels' unit-test hooks.  NOT part of the product library: compiled only into libvrag_amd_dbg.so (build.py, -DVRAG_DEBUG_API),
// which tools/ and the attention unit test load beside libvrag_amd.so.
#include "../../include/vrag_amd.h"
#include "../../include/vrag_amd_debug.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "attention.h"
#include "gemm_bf16.h"
#include "glue_kernels.h"
#include "host_util.h"
#include "norm_heads.h"
#include "qkv_attn.h"
#include "spans.h"
#include "topk_kernels.h"

using namespace vrag;

static inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

extern "C" {

int vrag_debug_gemm_ms(int32_t epi, int32_t M, int32_t N, int32_t K, int32_t iters, int32_t device, float* ms_out) {
  ARG_CHECK(ms_out && M > 0 && N % 128 == 0 && K % 64 == 0 && iters > 0, "bad arguments");
  ARG_CHECK(epi == EPI_F32 || epi == EPI_BF16 || epi == EPI_RESIDUAL || epi == EPI_GEGLU || epi == EPI_QKV_ROPE ||
                epi == EPI_F32_GELU || epi == EPI_NONE,
            "unsupported epilogue for the diagnostic");
  if (vrag_device_count() <= device) {
    set_error("no HIP device %d visible", device);
    return VRAG_ERR_NO_DEVICE;
  }
  HIP_TRY(hipSetDevice(device));
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
  // pseudo-random bf16 operands in [-1, 1): 0x3f80 | 7 mantissa bits = [1,2), minus 1.5, times 2
  {
    std::vector<unsigned short> h(std::max(Mp * K, (size_t)N * K));
    unsigned x = 12345u;
    for (auto& v : h) {
      x = x * 1664525u + 1013904223u;
      const unsigned m = (x >> 9) & 0x7f, s = (x >> 31) << 15, ex = 0x3e80u + (((x >> 20) & 1) << 7);
      v = (unsigned short)(s | ex | m);
    }
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
  hipEvent_t a, b;
  (void)hipEventCreate(&a);
  (void)hipEventCreate(&b);
  hipError_t le = hipSuccess;
  for (int i = 0; i < 3 && le == hipSuccess; ++i) le = launch_gemm((GemmEpi)epi, g, 0);
  (void)hipEventRecord(a, 0);
  for (int i = 0; i < iters && le == hipSuccess; ++i) le = launch_gemm((GemmEpi)epi, g, 0);
  (void)hipEventRecord(b, 0);
  hipError_t se = hipEventSynchronize(b);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, a, b);
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  if (le != hipSuccess || se != hipSuccess) {
    set_error("debug gemm failed: %s", hipGetErrorString(le != hipSuccess ? le : se));
    return VRAG_ERR_HIP;
  }
  *ms_out = ms / iters;
  return VRAG_OK;
}

int vrag_debug_attn_ms(int32_t local, int32_t n_seqs, int32_t S, int32_t H, int32_t window, int32_t iters, int32_t device,
                       float* ms_out) {
  ARG_CHECK(ms_out && n_seqs > 0 && S > 0 && S % kSeqAlign == 0 && H % 64 == 0 && iters > 0, "bad arguments");
  if (vrag_device_count() <= device) {
    set_error("no HIP device %d visible", device);
    return VRAG_ERR_NO_DEVICE;
  }
  HIP_TRY(hipSetDevice(device));
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
    unsigned x = 777u;
    for (auto& v : h) {   // pseudo-random bf16 in about [-1, 1), as vrag_debug_gemm_ms
      x = x * 1664525u + 1013904223u;
      v = (unsigned short)(((x >> 31) << 15) | (0x3e80u + (((x >> 20) & 1) << 7)) | ((x >> 9) & 0x7f));
    }
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
  hipEvent_t a, b;
  (void)hipEventCreate(&a);
  (void)hipEventCreate(&b);
  hipError_t le = hipSuccess;
  for (int i = 0; i < 3 && le == hipSuccess; ++i) le = launch_attention(ap, local != 0, 0);
  (void)hipEventRecord(a, 0);
  for (int i = 0; i < iters && le == hipSuccess; ++i) le = launch_attention(ap, local != 0, 0);
  (void)hipEventRecord(b, 0);
  hipError_t se = hipEventSynchronize(b);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, a, b);
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  if (le != hipSuccess || se != hipSuccess) {
    set_error("debug attention failed: %s", hipGetErrorString(le != hipSuccess ? le : se));
    return VRAG_ERR_HIP;
  }
  *ms_out = ms / iters;
  return VRAG_OK;
}

int vrag_debug_qkv_attn_ms(int32_t local, int32_t n_seqs, int32_t S, int32_t H, int32_t window, int32_t iters, int32_t flags,
                           int32_t device, float* ms_out) {
  ARG_CHECK(ms_out && n_seqs > 0 && S > 0 && S <= kFusedMaxSeq && S % kSeqAlign == 0 && H % 64 == 0 && iters > 0, "bad arguments");
  if (vrag_device_count() <= device) {
    set_error("no HIP device %d visible", device);
    return VRAG_ERR_NO_DEVICE;
  }
  HIP_TRY(hipSetDevice(device));
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
    unsigned xs = 777u;
    for (auto& v : h) {   // pseudo-random bf16 in about [-1, 1), as vrag_debug_gemm_ms
      xs = xs * 1664525u + 1013904223u;
      v = (unsigned short)(((xs >> 31) << 15) | (0x3e80u + (((xs >> 20) & 1) << 7)) | ((xs >> 9) & 0x7f));
    }
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
  hipEvent_t a, b;
  (void)hipEventCreate(&a);
  (void)hipEventCreate(&b);
  hipError_t le = hipSuccess;
  for (int i = 0; i < 3 && le == hipSuccess; ++i) le = launch_qkv_attention(f, local != 0, 0);
  (void)hipEventRecord(a, 0);
  for (int i = 0; i < iters && le == hipSuccess; ++i) le = launch_qkv_attention(f, local != 0, 0);
  (void)hipEventRecord(b, 0);
  hipError_t se = hipEventSynchronize(b);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, a, b);
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  if (le != hipSuccess || se != hipSuccess) {
    set_error("debug fused attention failed: %s", hipGetErrorString(le != hipSuccess ? le : se));
    return VRAG_ERR_HIP;
  }
  *ms_out = ms / iters;
  return VRAG_OK;
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
  for (int s = 0; s < n; ++s) {
    const int row = a->seq_row[s], len = a->seq_len[s];
    ARG_CHECK(len >= 1, "seq_len[%d] = %d must be at least 1", s, len);
    ARG_CHECK(row >= 0 && row % kSeqAlign == 0, "seq_row[%d] = %d must be a non-negative multiple of %d", s, row, kSeqAlign);
    ARG_CHECK((int64_t)row + len <= a->rows, "sequence %d (row %d, %d tokens) ends past row %d", s, row, len, a->rows);
  }
  {
    std::vector<int> order(n);
    for (int s = 0; s < n; ++s) order[s] = s;
    std::sort(order.begin(), order.end(), [&](int l, int r) { return a->seq_row[l] < a->seq_row[r]; });
    for (int i = 0; i + 1 < n; ++i)
      ARG_CHECK(a->seq_row[order[i]] + a->seq_len[order[i]] <= a->seq_row[order[i + 1]], "sequences %d and %d overlap", order[i], order[i + 1]);
  }
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
  if (vrag_device_count() <= device) {
    set_error("no HIP device %d visible", device);
    return VRAG_ERR_NO_DEVICE;
  }
  HIP_TRY(hipSetDevice(device));
  a->n_blocks = n_blocks;
  if (a->blocks_out)
    for (int b = 0; b < n_blocks; ++b) {
      a->blocks_out[3 * b] = bs[b];
      a->blocks_out[3 * b + 1] = bl[b];
      a->blocks_out[3 * b + 2] = bq[b];
    }
  const size_t R = (size_t)a->rows, H = (size_t)a->H;
  constexpr size_t kCanary = 4096;   // behind o: the launch must leave it as it was
  constexpr unsigned char kCanaryByte = 0xA5;
  DevBuf dq, dk, dv, dout, d_bs, d_bl, d_bq, sat;
  hipError_t e = dq.alloc(R * H * 2);
  if (e == hipSuccess) e = dk.alloc(R * H * 2);
  if (e == hipSuccess) e = dv.alloc(R * H * 2);
  if (e == hipSuccess) e = dout.alloc(R * H * 2 + kCanary);
  if (e == hipSuccess) e = d_bs.alloc((size_t)n_blocks * 4);
  if (e == hipSuccess) e = d_bl.alloc((size_t)n_blocks * 4);
  if (e == hipSuccess) e = d_bq.alloc((size_t)n_blocks * 4);
  if (e == hipSuccess) e = sat.alloc(4);
  if (e == hipSuccess) e = hipMemset(sat.p, 0, 4);
  if (e == hipSuccess) e = hipMemcpy(dq.p, a->q, R * H * 2, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dk.p, a->k, R * H * 2, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dv.p, a->vt, R * H * 2, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dout.p, a->o, R * H * 2, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout.as<char>() + R * H * 2, kCanaryByte, kCanary);
  if (e == hipSuccess) e = hipMemcpy(d_bs.p, bs.data(), (size_t)n_blocks * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_bl.p, bl.data(), (size_t)n_blocks * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_bq.p, bq.data(), (size_t)n_blocks * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) {
    AttnParams ap{};
    ap.q = dq.as<bf16_t>();
    ap.k = dk.as<bf16_t>();
    ap.vt = dv.as<bf16_t>();
    ap.o = dout.as<bf16_t>();
    ap.blk_seq_start = d_bs.as<int>();
    ap.blk_seq_len = d_bl.as<int>();
    ap.blk_q0 = d_bq.as<int>();
    ap.n_blocks = n_blocks;
    ap.H = (int)H;
    ap.nh = (int)H / 64;
    ap.Tp = (int)R;
    ap.window = a->window;
    ap.op_dtype = a->f16 ? kOpF16 : kOpBf16;
    ap.f16_sat = sat.as<unsigned>();
    e = launch_attention(ap, a->local != 0, 0);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  unsigned saturated = 0;
  if (e == hipSuccess) e = hipMemcpy(&saturated, sat.p, 4, hipMemcpyDeviceToHost);
  std::vector<unsigned char> canary(kCanary);
  if (e == hipSuccess) e = hipMemcpy(canary.data(), dout.as<char>() + R * H * 2, kCanary, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(a->o, dout.p, R * H * 2, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    set_error("debug attention run failed: %s", hipGetErrorString(e));
    return VRAG_ERR_HIP;
  }
  if (std::any_of(canary.begin(), canary.end(), [](unsigned char v) { return v != kCanaryByte; })) {
    set_error("debug attention run: the launch wrote past the end of o");
    return VRAG_ERR_HIP;
  }
  a->f16_saturated = saturated ? 1 : 0;
  return VRAG_OK;
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
  if (vrag_device_count() <= device) {
    set_error("no HIP device %d visible", device);
    return VRAG_ERR_NO_DEVICE;
  }
  HIP_TRY(hipSetDevice(device));

  // device copies: every buffer is followed by a 4 KiB canary that the launch must leave as it was
  constexpr size_t kCanary = 4096;
  constexpr unsigned char kCanaryByte = 0xA5;
  struct Buf {
    const void* host;
    void* host_out;   // null = input only
    size_t bytes;
    const char* name;
    DevBuf dev;   // bytes + kCanary
  };
  const size_t H = (size_t)std::max(a->hidden, 0), NO = epi == EPI_GEGLU ? (size_t)N / 2 : (size_t)N;
  std::vector<Buf> bufs;
  auto add = [&](const void* h, void* h_out, size_t bytes, const char* name) -> int {
    if (!h) return -1;
    bufs.push_back(Buf{h, h_out, bytes, name, DevBuf()});
    return (int)bufs.size() - 1;
  };
  const int iA = add(a->A, nullptr, R * K * 2, "A");
  const int iW = add(a->W, nullptr, (size_t)N * K * 2, "W");
  const int ibias = add(a->bias, nullptr, (size_t)N * 4, "bias");
  const int ils = add(a->ln_s, nullptr, (size_t)N * 4, "ln_s");
  const int isin = add(a->stats_in, nullptr, (size_t)(K / 64) * R * 8, "stats_in");
  const int irmu = add(a->res_mu, nullptr, R * 4, "res_mu");
  const int irrs = add(a->res_rstd, nullptr, R * 4, "res_rstd");
  const int irg = add(a->res_g, nullptr, (size_t)N * 4, "res_g");
  const int irb = add(a->res_b, nullptr, (size_t)N * 4, "res_b");
  const int icos = add(a->rope_cos, nullptr, (size_t)a->rope_rows * 32 * 4, "rope_cos");
  const int isn = add(a->rope_sin, nullptr, (size_t)a->rope_rows * 32 * 4, "rope_sin");
  const int ipos = add(a->pos, nullptr, R * 4, "pos");
  const int itok = add(a->tok_seq, nullptr, R * 4, "tok_seq");
  const int ilo_in = add(a->lo_in, a->lo_in == a->lo_out ? a->lo_out : nullptr, R * N, "lo_in");
  const int iof = add(a->out_f32, a->out_f32, R * N * 4, "out_f32");
  const int iob = add(a->out_bf16, a->out_bf16, R * NO * 2, "out_bf16");
  const int iq = add(a->q, a->q, R * H * 2, "q");
  const int ik = add(a->k, a->k, R * H * 2, "k");
  const int ivt = add(a->vt, a->vt, H * R * 2, "vt");
  const int imu = add(a->ln_mu, a->ln_mu, R * 4, "ln_mu");
  const int irs = add(a->ln_rstd, a->ln_rstd, R * 4, "ln_rstd");
  const int ish = add(a->ln_shift, a->ln_shift, R * 4, "ln_shift");
  const int ishp = add(a->ln_shift_prev, a->ln_shift_prev, R * 4, "ln_shift_prev");
  const int ires = add(a->resid_bf16, a->resid_bf16, R * N * 2, "resid_bf16");
  const int isp = add(a->stats_part, a->stats_part, (size_t)(N / 64) * R * 8, "stats_part");
  const int ilo_out = a->lo_out == a->lo_in ? ilo_in : add(a->lo_out, a->lo_out, R * N, "lo_out");
  const int ispl = add(a->splade_rows, a->splade_rows, (size_t)a->n_seqs * N * 4, "splade_rows");
  DevBuf sat;   // the launch's fp16 clamp word, reported in f16_saturated
  hipError_t e = sat.alloc(4);
  if (e == hipSuccess) e = hipMemset(sat.p, 0, 4);
  for (Buf& b : bufs) {
    if (e == hipSuccess) e = b.dev.alloc(b.bytes + kCanary);
    if (e == hipSuccess) e = hipMemcpy(b.dev.p, b.host, b.bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(b.dev.as<char>() + b.bytes, kCanaryByte, kCanary);
  }
  auto dev = [&](int i, size_t offset_bytes) -> char* { return i < 0 ? nullptr : bufs[i].dev.as<char>() + offset_bytes; };
  GemmParams g{};
  g.op_dtype = a->f16 ? kOpF16 : kOpBf16;
  g.f16_sat = sat.as<unsigned>();
  g.M = M;
  g.N = N;
  g.K = K;
  g.act_gelu = a->act_gelu;
  g.A = (const bf16_t*)dev(iA, lo * K * 2);
  g.W = (const bf16_t*)dev(iW, 0);
  g.bias = (const float*)dev(ibias, 0);
  g.ln_s = (const float*)dev(ils, 0);
  g.stats_in = (const float*)dev(isin, lo * 8);
  g.stats_ld = (int)R;
  g.fin_eps = a->fin_eps;
  g.res_mu = (const float*)dev(irmu, lo * 4);
  g.res_rstd = (const float*)dev(irrs, lo * 4);
  g.res_g = (const float*)dev(irg, 0);
  g.res_b = (const float*)dev(irb, 0);
  g.rope_cos = (const float*)dev(icos, 0);
  g.rope_sin = (const float*)dev(isn, 0);
  g.pos = (const int*)dev(ipos, lo * 4);
  g.hidden = (int)H;
  g.vt_ld = (int)R;
  g.q_scale = a->q_scale;
  g.tok_seq = (const int*)dev(itok, lo * 4);
  g.splade_rows = (unsigned*)dev(ispl, 0);
  g.lo_in = (const unsigned char*)dev(ilo_in, lo * N);
  g.lo_out = (unsigned char*)dev(ilo_out, lo * N);
  g.out_f32 = (float*)dev(iof, lo * N * 4);
  g.out_bf16 = (bf16_t*)dev(iob, lo * NO * 2);
  g.q = (bf16_t*)dev(iq, lo * H * 2);
  g.k = (bf16_t*)dev(ik, lo * H * 2);
  g.vt = (bf16_t*)dev(ivt, lo * 2);
  g.ln_mu = (const float*)dev(imu, lo * 4);
  g.ln_rstd = (const float*)dev(irs, lo * 4);
  g.ln_shift = (const float*)dev(ish, lo * 4);
  g.ln_shift_prev = (float*)dev(ishp, lo * 4);
  g.resid_bf16 = (bf16_t*)dev(ires, lo * N * 2);
  g.stats_part = (float*)dev(isp, lo * 8);
  const int thr = gemm_small_m_threshold(-1);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) {
    if (a->small_rows >= 0) gemm_small_m_threshold(a->small_rows);
    e = launch_gemm((GemmEpi)epi, g, 0);
    const GemmConfig c = gemm_last_config();
    gemm_small_m_threshold(thr);
    const int32_t cfg[7] = {c.bm, c.bn, c.wm, c.wn, c.ns, c.hw, c.kch};
    std::memcpy(a->config, cfg, sizeof(cfg));
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  unsigned saturated = 0;
  if (e == hipSuccess) e = hipMemcpy(&saturated, sat.p, 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) a->f16_saturated = saturated ? 1 : 0;
  std::vector<unsigned char> canary(kCanary);
  const char* clobbered = nullptr;
  for (Buf& b : bufs) {
    if (e != hipSuccess) break;
    e = hipMemcpy(canary.data(), b.dev.as<char>() + b.bytes, kCanary, hipMemcpyDeviceToHost);
    if (e == hipSuccess && !clobbered && std::any_of(canary.begin(), canary.end(), [](unsigned char v) { return v != kCanaryByte; }))
      clobbered = b.name;
    if (e == hipSuccess && b.host_out) e = hipMemcpy(b.host_out, b.dev.p, b.bytes, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) {
    set_error("debug gemm run failed: %s", hipGetErrorString(e));
    return VRAG_ERR_HIP;
  }
  if (clobbered) {
    set_error("debug gemm run: the launch wrote past the end of %s", clobbered);
    return VRAG_ERR_HIP;
  }
  return VRAG_OK;
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
  for (int s = 0; s < n; ++s) {
    const int row = a->seq_row[s], len = a->seq_len[s];
    ARG_CHECK(len >= 1 && len <= kFusedMaxSeq, "seq_len[%d] = %d outside 1..%d", s, len, kFusedMaxSeq);
    ARG_CHECK(row >= 0 && row % kSeqAlign == 0, "seq_row[%d] = %d must be a non-negative multiple of %d", s, row, kSeqAlign);
    // a wave reads 64 whole token rows, whatever its sequence's length
    ARG_CHECK((int64_t)row + 64 * ((len + 63) / 64) <= a->rows, "sequence %d (row %d, %d tokens): its last wave reads past row %d", s, row, len, a->rows);
  }
  {
    std::vector<int> order(n);
    for (int s = 0; s < n; ++s) order[s] = s;
    std::sort(order.begin(), order.end(), [&](int l, int r) { return a->seq_row[l] < a->seq_row[r]; });
    for (int i = 0; i + 1 < n; ++i)
      ARG_CHECK(a->seq_row[order[i]] + a->seq_len[order[i]] <= a->seq_row[order[i + 1]], "sequences %d and %d overlap", order[i], order[i + 1]);
  }
  if (vrag_device_count() <= device) {
    set_error("no HIP device %d visible", device);
    return VRAG_ERR_NO_DEVICE;
  }
  HIP_TRY(hipSetDevice(device));
  const size_t R = (size_t)a->rows, H = (size_t)a->H;
  const bool fold = a->ln_mu != nullptr;
  std::vector<int4> groups((size_t)n * 8);
  const int n_groups = a->packer ? pack_groups_best_fit(a->seq_row, a->seq_len, 0, n, groups.data())
                                 : fused_pack_groups(a->seq_row, a->seq_len, 0, n, groups.data());
  std::memcpy(a->groups_out, groups.data(), (size_t)n_groups * 8 * sizeof(int4));
  a->n_groups = n_groups;

  constexpr size_t kCanary = 4096;   // behind o: the launch must leave it as it was
  constexpr unsigned char kCanaryByte = 0xA5;
  DevBuf x, w, wh, ls, lsh, mu, rstd, cs, sn, o, d_groups, sat;
  hipError_t e = x.alloc(R * H * 2);
  if (e == hipSuccess) e = w.alloc(3 * H * H * 2);
  if (e == hipSuccess) e = wh.alloc(3 * H * H * 2);
  if (e == hipSuccess) e = cs.alloc((size_t)a->rope_rows * 32 * 4);
  if (e == hipSuccess) e = sn.alloc((size_t)a->rope_rows * 32 * 4);
  if (e == hipSuccess) e = o.alloc(R * H * 2 + kCanary);
  if (e == hipSuccess) e = d_groups.alloc((size_t)n_groups * 8 * sizeof(int4));
  if (e == hipSuccess) e = sat.alloc(4);
  if (e == hipSuccess) e = hipMemset(sat.p, 0, 4);
  if (e == hipSuccess) e = hipMemcpy(x.p, a->x, R * H * 2, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(w.p, a->w, 3 * H * H * 2, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(cs.p, a->rope_cos, (size_t)a->rope_rows * 32 * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(sn.p, a->rope_sin, (size_t)a->rope_rows * 32 * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(o.p, a->o, R * H * 2, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(o.as<char>() + R * H * 2, kCanaryByte, kCanary);
  if (e == hipSuccess) e = hipMemcpy(d_groups.p, groups.data(), (size_t)n_groups * 8 * sizeof(int4), hipMemcpyHostToDevice);
  if (fold) {
    if (e == hipSuccess) e = ls.alloc(3 * H * 4);
    if (e == hipSuccess) e = lsh.alloc((3 * H + 64) * 4);   // the kernel's 256-float DMA of a head's 192 sums reads 64 floats on (capi.hip)
    if (e == hipSuccess) e = mu.alloc(R * 4);
    if (e == hipSuccess) e = rstd.alloc(R * 4);
    if (e == hipSuccess) e = hipMemset(lsh.p, 0, (3 * H + 64) * 4);
    if (e == hipSuccess) e = hipMemcpy(ls.p, a->ln_s, 3 * H * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(mu.p, a->ln_mu, R * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(rstd.p, a->ln_rstd, R * 4, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) e = permute_qkv_heads(w.as<bf16_t>(), fold ? ls.as<float>() : nullptr, (int)H, a->nh, wh.as<bf16_t>(),
                                             fold ? lsh.as<float>() : nullptr, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) {
    QkvAttnParams f{};
    f.x = x.as<bf16_t>();
    f.w = wh.as<bf16_t>();
    f.ln_mu = fold ? mu.as<float>() : nullptr;
    f.ln_rstd = fold ? rstd.as<float>() : nullptr;
    f.ln_s = fold ? lsh.as<float>() : nullptr;
    f.rope_cos = cs.as<float>();
    f.rope_sin = sn.as<float>();
    f.rope_rows = a->rope_rows;
    f.o = o.as<bf16_t>();
    f.groups = d_groups.as<int4>();
    f.n_groups = n_groups;
    f.H = (int)H;
    f.nh = a->nh;
    f.Tp = (int)R;
    f.window = a->window;
    f.op_dtype = a->f16 ? kOpF16 : kOpBf16;
    f.q_scale = a->q_scale;
    f.debug_flags = a->debug_flags;
    f.f16_sat = sat.as<unsigned>();
    e = launch_qkv_attention(f, a->local != 0, 0);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  unsigned saturated = 0;
  if (e == hipSuccess) e = hipMemcpy(&saturated, sat.p, 4, hipMemcpyDeviceToHost);
  std::vector<unsigned char> canary(kCanary);
  if (e == hipSuccess) e = hipMemcpy(canary.data(), o.as<char>() + R * H * 2, kCanary, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(a->o, o.p, R * H * 2, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    set_error("debug fused attention run failed: %s", hipGetErrorString(e));
    return VRAG_ERR_HIP;
  }
  if (std::any_of(canary.begin(), canary.end(), [](unsigned char v) { return v != kCanaryByte; })) {
    set_error("debug fused attention run: the launch wrote past the end of o");
    return VRAG_ERR_HIP;
  }
  a->f16_saturated = saturated ? 1 : 0;
  return VRAG_OK;
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
  if (vrag_device_count() <= device) {
    set_error("no HIP device %d visible", device);
    return VRAG_ERR_NO_DEVICE;
  }
  HIP_TRY(hipSetDevice(device));

  // device copies: every buffer is followed by a 4 KiB canary that the launch must leave as it was
  constexpr size_t kCanary = 4096;
  constexpr unsigned char kCanaryByte = 0xA5;
  struct Buf {
    const void* host;
    void* host_out;   // null = input only
    size_t bytes;
    const char* name;
    DevBuf dev;   // bytes + kCanary
  };
  std::vector<Buf> bufs;
  auto add = [&](const void* h, void* h_out, size_t bytes, const char* name) -> int {
    if (!h) return -1;
    bufs.push_back(Buf{h, h_out, bytes, name, DevBuf()});
    return (int)bufs.size() - 1;
  };
  const size_t R = (size_t)rows, OR = (size_t)a->out_rows, Hs = (size_t)H, L = (size_t)std::max(a->num_labels, 0);
  const size_t out_cols = (embed || ln || (range && a->mode != 0)) ? Hs : L;
  const bool alias = ln && a->alias_f32;
  const int ih = embed ? -1 : add(a->h, alias ? a->h : nullptr, (size_t)a->h_rows * Hs * 4, "h");
  const int iids = embed ? add(a->ids, nullptr, R * 4, "ids") : -1;
  const int iE = embed ? add(a->E, nullptr, (size_t)a->vocab * Hs * 4, "E") : -1;
  const int iP = embed ? add(a->P, nullptr, (size_t)std::max(a->n_pos, 0) * Hs * 4, "P") : -1;
  const int ipos = embed ? add(a->pos, nullptr, R * 4, "pos") : -1;
  const int ityp = embed ? add(a->type_row, nullptr, (size_t)std::max(a->n_types, 0) * Hs * 4, "type_row") : -1;
  const int itid = embed ? add(a->type_ids, nullptr, R * 4, "type_ids") : -1;
  const int iw = add(a->w, nullptr, Hs * 4, "w");
  const int ibias = add(a->bias, nullptr, Hs * 4, "bias");
  const int istart = range ? add(a->start, nullptr, R * 4, "start") : -1;
  const int iend = range ? add(a->end, nullptr, R * 4, "end") : -1;
  const int ifirst = pooler ? add(a->first_row, nullptr, R * 4, "first_row") : -1;
  const int isrow = seqh ? add(a->seq_row, nullptr, R * 4, "seq_row") : -1;
  const int islen = seqh ? add(a->seq_len, nullptr, R * 4, "seq_len") : -1;
  const int iWp = pooler ? add(a->Wp, nullptr, Hs * Hs * 4, "Wp") : -1;
  const int ibp = pooler ? add(a->bp, nullptr, Hs * 4, "bp") : -1;
  const int iWd = seqh ? add(a->WdT, nullptr, Hs * Hs * 4, "WdT") : -1;
  const int ibd = seqh ? add(a->bd, nullptr, Hs * 4, "bd") : -1;
  const int iwn = seqh ? add(a->wn, nullptr, Hs * 4, "wn") : -1;
  const int ibn = seqh ? add(a->bn, nullptr, Hs * 4, "bn") : -1;
  const int iWc = add(a->Wc, nullptr, L * Hs * 4, "Wc");
  const int ibc = add(a->bc, nullptr, L * 4, "bc");
  const int iof = add(a->out_f32, a->out_f32, OR * out_cols * 4, "out_f32");
  const int io16 = (embed || ln) ? add(a->out16, a->out16, OR * (ln && a->split3 ? 3 * Hs : Hs) * 2, "out16") : -1;
  const int ilo = ln ? add(a->out_lo, a->out_lo, OR * Hs * 2, "out_lo") : -1;
  const int imean = ln ? add(a->row_mean, a->row_mean, OR * 4, "row_mean") : -1;
  const int ipool = seqh ? add(a->pooled, a->pooled, OR * Hs * 4, "pooled") : -1;
  DevBuf sat;   // the launch's fp16 clamp word, reported in f16_saturated
  hipError_t e = sat.alloc(4);
  if (e == hipSuccess) e = hipMemset(sat.p, 0, 4);
  for (Buf& b : bufs) {
    if (e == hipSuccess) e = b.dev.alloc(b.bytes + kCanary);
    if (e == hipSuccess && b.bytes) e = hipMemcpy(b.dev.p, b.host, b.bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(b.dev.as<char>() + b.bytes, kCanaryByte, kCanary);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    set_error("debug rows run: staging failed: %s", hipGetErrorString(e));
    return VRAG_ERR_HIP;
  }
  auto fp = [&](int i) -> float* { return i < 0 ? nullptr : bufs[i].dev.as<float>(); };
  auto ip = [&](int i) -> int* { return i < 0 ? nullptr : bufs[i].dev.as<int>(); };
  auto hp = [&](int i) -> bf16_t* { return i < 0 ? nullptr : bufs[i].dev.as<bf16_t>(); };
  const int dt = a->f16 ? kOpF16 : kOpBf16;
  unsigned* satp = a->no_sat ? nullptr : sat.as<unsigned>();
  hipError_t le = hipSuccess;
  switch (op) {
    case VRAG_DEBUG_ROWS_EMBED_LN:
      le = launch_embed_ln(ip(iids), fp(iE), fp(iw), a->eps, H, rows, fp(iof), hp(io16), 0, fp(iP), ip(ipos), fp(ityp), fp(ibias), ip(itid), dt, satp);
      break;
    case VRAG_DEBUG_ROWS_LAYERNORM:
      le = launch_layernorm(fp(ih), fp(iw), a->eps, H, rows, hp(io16), alias ? fp(ih) : fp(iof), 0, fp(ibias), fp(imean), dt, hp(ilo), a->gelu_first,
                            a->split3, satp);
      break;
    case VRAG_DEBUG_ROWS_RANGE_POOL:
      le = launch_range_pool(fp(ih), fp(iw), a->eps, H, ip(istart), ip(iend), rows, a->mode, fp(iWc), fp(ibc), a->num_labels, fp(iof), 0);
      break;
    case VRAG_DEBUG_ROWS_LN_CLASSIFIER:
      le = launch_ln_classifier(fp(ih), fp(iw), a->eps, H, rows, fp(iWc), fp(ibc), a->num_labels, fp(iof), 0, fp(ibias), a->gelu_first);
      break;
    case VRAG_DEBUG_ROWS_POOLER_CLASSIFIER:
      le = launch_pooler_classifier(fp(ih), H, ip(ifirst), rows, fp(iWp), fp(ibp), fp(iWc), fp(ibc), a->num_labels, fp(iof), 0);
      break;
    default:
      le = launch_seq_head(fp(ih), fp(iw), a->eps, H, ip(isrow), ip(islen), rows, a->mode, fp(ipool), fp(iWd), fp(ibd), fp(iwn), fp(ibn), fp(iWc),
                           fp(ibc), a->num_labels, fp(iof), 0);
      break;
  }
  a->launch_status = (int32_t)le;
  e = hipDeviceSynchronize();
  unsigned saturated = 0;
  if (e == hipSuccess) e = hipMemcpy(&saturated, sat.p, 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) a->f16_saturated = saturated ? 1 : 0;
  std::vector<unsigned char> canary(kCanary);
  const char* clobbered = nullptr;
  for (Buf& b : bufs) {
    if (e != hipSuccess) break;
    e = hipMemcpy(canary.data(), b.dev.as<char>() + b.bytes, kCanary, hipMemcpyDeviceToHost);
    if (e == hipSuccess && !clobbered && std::any_of(canary.begin(), canary.end(), [](unsigned char v) { return v != kCanaryByte; }))
      clobbered = b.name;
    if (e == hipSuccess && b.host_out && b.bytes) e = hipMemcpy(b.host_out, b.dev.p, b.bytes, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) {
    set_error("debug rows run failed: %s", hipGetErrorString(e));
    return VRAG_ERR_HIP;
  }
  if (clobbered) {
    set_error("debug rows run: the launch wrote past the end of %s", clobbered);
    return VRAG_ERR_HIP;
  }
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
  if (vrag_device_count() <= device) {
    set_error("no HIP device %d visible", device);
    return VRAG_ERR_NO_DEVICE;
  }
  HIP_TRY(hipSetDevice(device));

  // device copies: every buffer is followed by a 4 KiB canary that the launch must leave as it was
  constexpr size_t kCanary = 4096;
  constexpr unsigned char kCanaryByte = 0xA5;
  struct Buf {
    const void* host;
    void* host_out;   // null = input only
    size_t bytes;
    const char* name;
    DevBuf dev;   // bytes + kCanary
  };
  std::vector<Buf> bufs;
  auto add = [&](const void* h, void* h_out, size_t bytes, const char* name) -> int {
    if (!h) return -1;
    bufs.push_back(Buf{h, h_out, bytes, name, DevBuf()});
    return (int)bufs.size() - 1;
  };
  const size_t OR = (size_t)a->out_rows, cols = (size_t)a->cols, ld = (size_t)a->ld, Hs = (size_t)a->H;
  int isrc = -1, iscale = -1, idst = -1, ilo = -1, isum = -1, ipart = -1, imu = -1, irstd = -1, ishin = -1, ishout = -1, iprev = -1;
  int ipacked = -1, isrow = -1, issrc = -1, islen = -1, iids = -1, ipos = -1, itok = -1, icnt = -1, iidx = -1, ival = -1;
  int iw = -1, is = -1, iwo = -1, iso = -1;
  if (cvt || split3) {
    isrc = add(a->src, nullptr, (size_t)a->rows_src * cols * 4, "src");
    idst = add(a->dst, a->dst, OR * (split3 ? 3 * cols : cols) * 2, "dst");
  }
  if (cvt) {
    iscale = add(a->col_scale, nullptr, cols * 4, "col_scale");
    ilo = add(a->dst_lo, a->dst_lo, OR * cols * 2, "dst_lo");
    isum = add(a->row_sum, a->row_sum, OR * 4, "row_sum");
  }
  if (fin) {
    ipart = add(a->part, nullptr, (size_t)a->np * ld * 2 * 4, "part");
    imu = add(a->mu, a->mu, ld * 4, "mu");
    irstd = add(a->rstd, a->rstd, ld * 4, "rstd");
    ishin = add(a->shift_in, nullptr, ld * 4, "shift_in");
    ishout = add(a->shift_out, a->shift_out, ld * 4, "shift_out");
    iprev = add(a->shift_prev, a->shift_prev, ld * 4, "shift_prev");
  }
  if (pack) {
    const size_t n = (size_t)a->n_seqs;
    ipacked = add(a->packed, nullptr, (size_t)a->n_packed * 4, "packed");
    isrow = add(a->seq_row, nullptr, n * 4, "seq_row");
    issrc = add(a->seq_src, nullptr, n * 4, "seq_src");
    islen = add(a->seq_len, nullptr, n * 4, "seq_len");
    iids = add(a->ids, a->ids, OR * 4, "ids");
    ipos = add(a->pos, a->pos, OR * 4, "pos");
    itok = add(a->tok_seq, a->tok_seq, OR * 4, "tok_seq");
  }
  if (compact) {
    isrc = add(a->src, nullptr, (size_t)a->rows * ld * 4, "src");
    icnt = add(a->counts, a->counts, OR * 4, "counts");
    iidx = add(a->idx, a->idx, OR * (size_t)a->cap * 4, "idx");
    ival = add(a->val, a->val, OR * (size_t)a->cap * 4, "val");
  }
  if (permute) {
    iw = add(a->w, nullptr, 3 * Hs * Hs * 2, "w");
    is = add(a->s, nullptr, 3 * Hs * 4, "s");
    iwo = add(a->w_out, a->w_out, OR * Hs * 2, "w_out");
    iso = add(a->s_out, a->s_out, OR * 4, "s_out");
  }
  DevBuf sat;   // the launch's fp16 clamp word, reported in f16_saturated
  hipError_t e = sat.alloc(4);
  if (e == hipSuccess) e = hipMemset(sat.p, 0, 4);
  for (Buf& b : bufs) {
    if (e == hipSuccess) e = b.dev.alloc(b.bytes + kCanary);
    if (e == hipSuccess && b.bytes) e = hipMemcpy(b.dev.p, b.host, b.bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(b.dev.as<char>() + b.bytes, kCanaryByte, kCanary);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    set_error("debug glue run: staging failed: %s", hipGetErrorString(e));
    return VRAG_ERR_HIP;
  }
  auto fp = [&](int i) -> float* { return i < 0 ? nullptr : bufs[i].dev.as<float>(); };
  auto ip = [&](int i) -> int* { return i < 0 ? nullptr : bufs[i].dev.as<int>(); };
  auto hp = [&](int i) -> bf16_t* { return i < 0 ? nullptr : bufs[i].dev.as<bf16_t>(); };
  const int dt = a->f16 ? kOpF16 : kOpBf16;
  switch (op) {
    case VRAG_DEBUG_GLUE_CVT_ROWS:
      launch_cvt_rows(dt, dim3(a->rows_dst), 0, fp(isrc), hp(idst), a->rows_dst, a->rows_src, a->cols, a->interleave ? a->I : 0,
                      fp(iscale), fp(isum), hp(ilo), sat.as<unsigned>());
      break;
    case VRAG_DEBUG_GLUE_CVT_SPLIT3:
      launch_cvt_split3(dt, 0, fp(isrc), hp(idst), a->rows_dst, a->rows_src, a->cols, sat.as<unsigned>());
      break;
    case VRAG_DEBUG_GLUE_LN_STATS_FINALIZE: {
      const int r0 = a->row0;   // as the encoder addresses a micro-batch
      float* prev = fp(iprev);
      launch_ln_stats_finalize(0, fp(ipart) + (size_t)r0 * 2, a->ld, a->np, a->H, a->eps, a->rows, fp(imu) + r0, fp(irstd) + r0,
                               a->alias_shift ? fp(ishout) + r0 : (ishin < 0 ? (const float*)nullptr : fp(ishin) + r0), fp(ishout) + r0,
                               prev ? prev + r0 : nullptr);
      break;
    }
    case VRAG_DEBUG_GLUE_PACK_LAYOUT:
      launch_pack_layout(0, ip(ipacked), ip(isrow), ip(issrc), ip(islen), a->n_seqs, a->rows, a->pad_id, ip(iids), ip(ipos), ip(itok));
      break;
    case VRAG_DEBUG_GLUE_SPLADE_COMPACT:
      launch_splade_compact(0, fp(isrc), a->rows, a->V, a->ld, a->thr, a->cap, ip(icnt), ip(iidx), fp(ival));
      break;
    default:
      (void)permute_qkv_heads(hp(iw), fp(is), a->H, a->nh, hp(iwo), fp(iso), nullptr);
      break;
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  unsigned saturated = 0;
  if (e == hipSuccess) e = hipMemcpy(&saturated, sat.p, 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) a->f16_saturated = saturated ? 1 : 0;
  std::vector<unsigned char> canary(kCanary);
  const char* clobbered = nullptr;
  for (Buf& b : bufs) {
    if (e != hipSuccess) break;
    e = hipMemcpy(canary.data(), b.dev.as<char>() + b.bytes, kCanary, hipMemcpyDeviceToHost);
    if (e == hipSuccess && !clobbered && std::any_of(canary.begin(), canary.end(), [](unsigned char v) { return v != kCanaryByte; }))
      clobbered = b.name;
    if (e == hipSuccess && b.host_out && b.bytes) e = hipMemcpy(b.host_out, b.dev.p, b.bytes, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) {
    set_error("debug glue run failed: %s", hipGetErrorString(e));
    return VRAG_ERR_HIP;
  }
  if (clobbered) {
    set_error("debug glue run: the launch wrote past the end of %s", clobbered);
    return VRAG_ERR_HIP;
  }
  return VRAG_OK;
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
  if (vrag_device_count() <= device) {
    set_error("no HIP device %d visible", device);
    return VRAG_ERR_NO_DEVICE;
  }
  HIP_TRY(hipSetDevice(device));

  // device copies: every buffer is followed by a 4 KiB canary that the launch must leave as it was
  constexpr size_t kCanary = 4096;
  constexpr unsigned char kCanaryByte = 0xA5;
  struct Buf {
    const void* host;
    void* host_out;   // null = input only
    size_t bytes;     // copied from the host
    size_t pad;       // zero bytes behind them (the corpus's last tile), in front of the canary
    const char* name;
    DevBuf dev;
  };
  std::vector<Buf> bufs;
  auto add = [&](const void* h, void* h_out, size_t bytes, const char* name, size_t pad = 0) -> int {
    if (!h) return -1;
    bufs.push_back(Buf{h, h_out, bytes, pad, name, DevBuf()});
    return (int)bufs.size() - 1;
  };
  const size_t NB = (size_t)a->nq_buf, K = (size_t)a->K, k = (size_t)a->k, cap = (size_t)a->cap;
  int icorpus = -1, iw = -1, iq = -1, ieps = -1, isrc = -1, iwo = -1, ibuf = -1, icnt = -1, ikey = -1, isc = -1, iout = -1, iovf = -1, idone = -1;
  if (stage || rescue) {
    const size_t rows = (size_t)a->corpus_rows, padded = (rows + 255) / 256 * 256;
    icorpus = add(a->corpus, nullptr, rows * K * 2, "corpus", (padded - rows) * K * 2);
  }
  if (stage) iw = add(a->w, nullptr, (size_t)a->N * K * 2, "w");
  if (queries || rescue) iq = add(a->queries, nullptr, (size_t)a->nq * K * 4, "queries");
  if (queries) iwo = add(a->w_out, a->w_out, (size_t)a->N * K * 2, "w_out");
  if (seld) isrc = add(a->src, nullptr, (size_t)a->nq * (size_t)a->src_stride * 8, "src");
  if (merge) isrc = add(a->src, nullptr, (size_t)a->n * (size_t)a->nq * k * 8, "src");
  if (stage || sel || seld) ibuf = add(a->buf, a->buf, NB * cap * 8, "buf");
  if (stage || sel || seld || tau) {
    icnt = add(a->cnt, a->cnt, NB * 4, "cnt");
    ikey = add(a->thr_key, a->thr_key, NB * 8, "thr_key");
    isc = add(a->thr_score, a->thr_score, NB * 4, "thr_score");
  }
  if (sel || seld || rescue || merge) iout = add(a->out, a->out, NB * k * 8, "out");
  if (sel || seld || rescue || tau) iovf = add(a->ovf, a->ovf, NB * 4, "ovf");
  if (tau) ieps = add(a->eps, nullptr, (size_t)a->nq * 4, "eps");
  if (rescue) idone = add(a->done, a->done, NB * 4, "done");
  DevBuf part;   // the rescue's per-slice lists [slices][nq][k]: scratch of the hook, with a canary of its own
  const size_t part_bytes = rescue ? (size_t)a->slices * (size_t)a->nq * k * 8 : 0;
  hipError_t e = hipSuccess;
  if (rescue) {
    e = part.alloc(part_bytes + kCanary);
    if (e == hipSuccess) e = hipMemset(part.p, 0, part_bytes);
    if (e == hipSuccess) e = hipMemset(part.as<char>() + part_bytes, kCanaryByte, kCanary);
  }
  for (Buf& b : bufs) {
    if (e == hipSuccess) e = b.dev.alloc(b.bytes + b.pad + kCanary);
    if (e == hipSuccess && b.bytes) e = hipMemcpy(b.dev.p, b.host, b.bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && b.pad) e = hipMemset(b.dev.as<char>() + b.bytes, 0, b.pad);
    if (e == hipSuccess) e = hipMemset(b.dev.as<char>() + b.bytes + b.pad, kCanaryByte, kCanary);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    set_error("debug topk run: staging failed: %s", hipGetErrorString(e));
    return VRAG_ERR_HIP;
  }
  auto fp = [&](int i) -> float* { return i < 0 ? nullptr : bufs[i].dev.as<float>(); };
  auto up = [&](int i) -> unsigned* { return i < 0 ? nullptr : bufs[i].dev.as<unsigned>(); };
  auto kp = [&](int i) -> u64* { return i < 0 ? nullptr : bufs[i].dev.as<u64>(); };
  auto hp = [&](int i) -> bf16_t* { return i < 0 ? nullptr : bufs[i].dev.as<bf16_t>(); };
  switch (op) {
    case VRAG_DEBUG_TOPK_SCORE_STAGE: {
      GemmParams g{};
      g.op_dtype = kOpBf16;
      const bool mapped = a->tile_stride > 1 || a->tile_skip > 1;   // as dense_tiled_search: the map starts at the shard's first row
      g.A = hp(icorpus) + (mapped ? (size_t)0 : (size_t)a->row_base * K);
      g.W = hp(iw);
      g.M = a->M;
      g.N = a->N;
      g.K = a->K;
      g.topk_thr_score = fp(isc);
      g.topk_thr_key = kp(ikey);
      g.topk_cnt = up(icnt);
      g.topk_buf = kp(ibuf);
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
      e = launch_tiled_queries(fp(iq), a->nq, a->K, a->pairs, a->N, hp(iwo), 0);
      break;
    case VRAG_DEBUG_TOPK_SELECT:
      e = launch_tiled_select(kp(ibuf), up(icnt), a->cap, a->k, kp(ikey), fp(isc), kp(iout), up(iovf), 0, a->nq, 0);
      break;
    case VRAG_DEBUG_TOPK_SELECT_DIRECT:
      e = launch_tiled_select_direct(kp(isrc), a->src_stride, a->n, kp(ibuf), up(icnt), a->cap, a->k, kp(ikey), fp(isc), kp(iout), up(iovf), a->nq, 0);
      break;
    case VRAG_DEBUG_TOPK_RESCUE:
      e = launch_dense_tiled_rescue(hp(icorpus), (long long)a->n, a->K, fp(iq), a->nq, a->k, up(iovf), part.as<u64>(), up(idone), kp(iout), a->slices, 0);
      break;
    case VRAG_DEBUG_TOPK_MERGE:
      e = launch_topk_merge(kp(isrc), a->n, a->nq, a->k, kp(iout), 0);
      break;
    default:
      e = launch_tiled_tau(a->nq, kp(ikey), fp(isc), fp(ieps), up(icnt), up(iovf), 0);
      break;
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  std::vector<unsigned char> canary(kCanary);
  const char* clobbered = nullptr;
  auto intact = [&]() { return std::all_of(canary.begin(), canary.end(), [](unsigned char v) { return v == kCanaryByte; }); };
  if (e == hipSuccess && rescue) {
    e = hipMemcpy(canary.data(), part.as<char>() + part_bytes, kCanary, hipMemcpyDeviceToHost);
    if (e == hipSuccess && !intact()) clobbered = "part";
  }
  for (Buf& b : bufs) {
    if (e != hipSuccess) break;
    e = hipMemcpy(canary.data(), b.dev.as<char>() + b.bytes + b.pad, kCanary, hipMemcpyDeviceToHost);
    if (e == hipSuccess && !clobbered && !intact()) clobbered = b.name;
    if (e == hipSuccess && b.host_out && b.bytes) e = hipMemcpy(b.host_out, b.dev.p, b.bytes, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) {
    set_error("debug topk run failed: %s", hipGetErrorString(e));
    return e == hipErrorInvalidValue ? VRAG_ERR_INVALID : VRAG_ERR_HIP;
  }
  if (clobbered) {
    set_error("debug topk run: the launch wrote past the end of %s", clobbered);
    return VRAG_ERR_HIP;
  }
  return VRAG_OK;
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
