// Span selection of the v2 highlighter on gfx950: per-token logits of the 2-label token head -> (start, end) character spans
// per (question, chunk) job, so that the logits never leave HBM (include/vrag_amd.h states the rule; extractors.py
// `token_spans_to_char_spans` over the window maximum is the host form).
//   token_spans_kernel: one wave64 per job, 64 context tokens per step.  A lane finds the windows that cover its token by a
//   binary search in the job's window table (windows ascend in a and b, so the covering ones are adjacent), takes the maximum
//   margin logit[1] - logit[0] over them and compares it with tau.  Two ballots (hot, cold) cut the step into runs; a scalar loop
//   over the cold bits closes them, with the open run and the last merged span carried across steps in uniform registers.
//   Lane 0 appends.  Plain vector loads and stores, no LDS, no atomics.
#include "spans.h"

#include <cmath>
#include <vector>

namespace vrag {
namespace {

__device__ __forceinline__ unsigned long long below(int p) { return p >= 64 ? ~0ull : (1ull << p) - 1ull; }

__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// win[w] = {a, b, row of the logits of context token a, -}; windows of job j: win_off[j] .. win_off[j + 1], a and b ascending.
__global__ __launch_bounds__(256) void token_spans_kernel(const float2* __restrict__ logits, const int4* __restrict__ win,
                                                          const int* __restrict__ win_off, const int* __restrict__ job_off,
                                                          const int2* __restrict__ offs, int n_jobs, float tau, int min_span, int gap,
                                                          int cap, int* __restrict__ counts, int2* __restrict__ spans) {
  const int lane = threadIdx.x & 63;
  const int job = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (job >= n_jobs) return;   // the whole wave leaves
  const int w0 = win_off[job], w1 = win_off[job + 1];
  const int t0 = job_off[job], n = job_off[job + 1] - t0;
  int2* out = spans + (size_t)job * cap;
  // uniform state: the open run [cs, ce), the last merged span [ls, le) that a later run may still extend, spans so far
  bool open = false, have = false;
  int cs = 0, ce = 0, ls = 0, le = 0, count = 0;
  auto emit = [&]() {   // the merged span is final
    if (le - ls >= min_span) {
      if (lane == 0 && count < cap) out[count] = make_int2(ls, le);
      ++count;
    }
  };
  auto close_run = [&]() {
    if (have && cs - le <= gap) {
      le = max(le, ce);
    } else {
      if (have) emit();
      ls = cs;
      le = ce;
      have = true;
    }
    open = false;
  };
  for (int base = 0; base < n; base += 64) {
    const int t = base + lane;
    bool hot = false, cold = false;
    int s = 0, e = 0;
    if (t < n) {
      const int2 o = offs[t0 + t];
      s = o.x;
      e = o.y;
      if (e > s) {   // a token without characters neither extends nor closes a run
        int lo = w0, hi = w1;   // the first window with b > t
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (win[mid].y > t) hi = mid;
          else lo = mid + 1;
        }
        float best = -INFINITY;
        bool nan = false;
        for (int w = lo; w < w1; ++w) {
          const int4 d = win[w];
          if (d.x > t) break;
          const float2 l = logits[(long long)d.z + (t - d.x)];
          const float m = l.y - l.x;
          if (m != m || l.y == INFINITY) nan = true;   // logit[1] = +inf: the host's softmax makes the row NaN
          else best = fmaxf(best, m);
        }
        hot = !nan && best > tau;
        cold = !hot;
      }
    }
    const unsigned long long hot_m = __ballot(hot), cold_m = __ballot(cold);
    int pos = 0;   // lanes below pos are done
    for (;;) {
      const unsigned long long cm = cold_m & ~below(pos);
      const int c = cm ? __builtin_ctzll(cm) : 64;   // the cold token that closes what lies in [pos, c)
      const unsigned long long seg = hot_m & ~below(pos) & below(c);
      if (seg) {
        const int first = __builtin_ctzll(seg);
        const int rs = __shfl(s, first, 64);
        const int re = wave_max_i32(((seg >> lane) & 1ull) ? e : (int)0x80000000);
        if (open) {
          ce = max(ce, re);
        } else {
          open = true;
          cs = rs;
          ce = re;
        }
      }
      if (c == 64) break;
      if (open) close_run();
      pos = c + 1;
    }
  }
  if (open) close_run();
  if (have) emit();
  if (lane == 0) counts[job] = count;
}

template <typename T>
hipError_t put(DevBuf& dst, const std::vector<T>& src, hipStream_t st) {
  hipError_t e = dst.reserve(src.size() * sizeof(T));
  if (e == hipSuccess && !src.empty()) e = hipMemcpyAsync(dst.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, st);
  return e;
}

}  // namespace

int run_token_spans(TokenSpanScratch& ws, const float* d_logits, int64_t n_rows, const int32_t* win_job, const int32_t* win_a,
                    const int32_t* win_b, const int32_t* win_row, int32_t n_windows, const int64_t* job_off, const int32_t* offsets,
                    int32_t n_jobs, float tau, int32_t min_span_chars, int32_t merge_gap_chars, int32_t cap_per_job, int32_t* counts,
                    int32_t* spans, hipStream_t st) {
  ARG_CHECK(n_jobs >= 0 && n_windows >= 0 && cap_per_job > 0 && job_off && counts && spans, "token spans: bad arguments");
  ARG_CHECK(n_windows == 0 || (win_job && win_a && win_b && win_row && d_logits), "token spans: null window table");
  ARG_CHECK(!std::isnan(tau), "token spans: tau is NaN");
  ARG_CHECK((int64_t)n_jobs * cap_per_job < 0x7FFFFFF0ll / 2, "token spans: n_jobs * cap_per_job must stay below 2^30");
  ARG_CHECK(job_off[0] == 0, "token spans: job_off[0] must be 0");
  for (int32_t j = 0; j < n_jobs; ++j) ARG_CHECK(job_off[j + 1] >= job_off[j], "token spans: job_off must be non-decreasing (job %d)", j);
  const int64_t n_tok = job_off[n_jobs];
  ARG_CHECK(n_tok < 0x7FFFFFF0ll, "token spans: at most 2^31 context tokens per call");
  ARG_CHECK(n_tok == 0 || offsets, "token spans: null offsets");
  if (n_jobs == 0) return VRAG_OK;
  std::vector<int4> win((size_t)n_windows);
  std::vector<int> woff((size_t)n_jobs + 1, 0), joff((size_t)n_jobs + 1);
  for (int32_t j = 0; j <= n_jobs; ++j) joff[j] = (int)job_off[j];
  for (int32_t w = 0; w < n_windows; ++w) {
    const int32_t j = win_job[w], a = win_a[w], b = win_b[w], row = win_row[w];
    ARG_CHECK(j >= 0 && j < n_jobs && (w == 0 || win_job[w - 1] <= j), "token spans: window %d: job %d out of range or out of order", w, j);
    ARG_CHECK(0 <= a && a <= b && b <= joff[j + 1] - joff[j], "token spans: window %d covers context tokens [%d, %d) of a job of %d", w, a, b,
              joff[j + 1] - joff[j]);
    ARG_CHECK(w == 0 || win_job[w - 1] != j || (win_a[w - 1] <= a && win_b[w - 1] <= b),
              "token spans: the windows of job %d must ascend in start and end", j);
    ARG_CHECK(row >= 0 && (int64_t)row + (b - a) <= n_rows, "token spans: window %d reads logits rows [%d, %d) of %lld", w, row, row + (b - a),
              (long long)n_rows);
    win[w] = make_int4(a, b, row, 0);
    ++woff[j + 1];
  }
  for (int32_t j = 0; j < n_jobs; ++j) woff[j + 1] += woff[j];
  // the copies read `win`, `woff`, `joff` and the caller's arrays until the stream has drained: no return in between
  auto enqueue = [&]() -> hipError_t {
    hipError_t e = put(ws.win, win, st);
    if (e == hipSuccess) e = put(ws.win_off, woff, st);
    if (e == hipSuccess) e = put(ws.job_off, joff, st);
    if (e == hipSuccess) e = ws.offsets.reserve((size_t)n_tok * 8);
    if (e == hipSuccess && n_tok) e = hipMemcpyAsync(ws.offsets.p, offsets, (size_t)n_tok * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = ws.counts.reserve((size_t)n_jobs * 4);
    if (e == hipSuccess) e = ws.spans.reserve((size_t)n_jobs * cap_per_job * 8);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(token_spans_kernel, dim3((unsigned)((n_jobs + 3) / 4)), dim3(256), 0, st, reinterpret_cast<const float2*>(d_logits),
                       ws.win.as<int4>(), ws.win_off.as<int>(), ws.job_off.as<int>(), ws.offsets.as<int2>(), (int)n_jobs, tau,
                       (int)min_span_chars, (int)merge_gap_chars, (int)cap_per_job, ws.counts.as<int>(), ws.spans.as<int2>());
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(counts, ws.counts.p, (size_t)n_jobs * 4, hipMemcpyDeviceToHost, st);
    return e;
  };
  const hipError_t queued = enqueue();
  const hipError_t drained = hipStreamSynchronize(st);   // on the error path too
  HIP_TRY(queued);
  HIP_TRY(drained);
  int worst = 0;
  for (int32_t j = 0; j < n_jobs; ++j) worst = std::max(worst, counts[j]);
  if (worst > cap_per_job) {
    set_error("token spans: a job has %d spans, capacity per job is %d", worst, cap_per_job);
    return VRAG_ERR_CAPACITY;
  }
  if (worst) {   // only the used prefix of every job's row travels
    HIP_TRY(hipMemcpy2DAsync(spans, (size_t)cap_per_job * 8, ws.spans.p, (size_t)cap_per_job * 8, (size_t)worst * 8, n_jobs,
                             hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return VRAG_OK;
}

}  // namespace vrag
