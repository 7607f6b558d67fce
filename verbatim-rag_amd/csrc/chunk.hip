// Markdown chunking of a batch of documents (gfx950): the structural pass of the reference's default chunker,
//   MarkdownChunkerProvider._md_chunker_with_ancestor_injection (verbatim_rag/chunker_providers.py:93-213),
// over UTF-8 bytes.  Rules R1-R8 are spelled out in DESIGN.md section 3 and include/vrag_amd.h; in short: a header is a line
// `#{1,6}\s+title`, found the way re.finditer finds it (the white space behind the hashes may run over line ends and swallow
// later header lines), header i owns the lines up to header i+1, blocks of the chosen levels become chunks and carry the
// stack of their ancestors.
//
// Two phases:
//   bytes   One lane per 16 bytes of the WHOLE batch (a 4 KiB slice per workgroup), so one 50 MB document spreads over the chip
//           like 5 000 small ones.  A lane finds the header candidates that START in its 16 bytes; the '#' run, the white-space
//           character behind it and the look-ahead to the end of the title line are read straight from global memory, so a slice
//           border cuts nothing.  Pass 1 counts candidates per workgroup, the host turns the counts into offsets, pass 2 writes
//           the candidate records at offset + rank inside the workgroup: position order, whichever workgroup runs first.
//   headers One lane per document walks that document's candidates (it sees headers, not bytes): drops the swallowed ones,
//           keeps the ancestor stack in six level slots, counts (pass 3) and, after the host's prefix sums, writes the header
//           and chunk tables (pass 4) at the document's own offsets.
#include "../../include/vrag_amd.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "host_util.h"
#include "text_space.h"

namespace vrag {

constexpr int CHUNK_WG = 256;            // lanes of a byte-phase workgroup
constexpr int CHUNK_LANE_BYTES = 16;     // bytes a lane owns
constexpr int CHUNK_WG_BYTES = CHUNK_WG * CHUNK_LANE_BYTES;

// The document that holds byte i of the batch (doc_off[d] <= i < doc_off[d+1]; empty documents hold no byte).  Found by a binary
// search on first use, then moved forward: a lane asks for ascending i only.
struct DocCursor {
  const long long* off;
  int n_docs;
  int d = -1;
  __device__ DocCursor(const long long* o, int n) : off(o), n_docs(n) {}
  __device__ int at(long long i) {
    if (d < 0) {
      int lo = 0, hi = n_docs;             // first j in [0, n_docs] with off[j] > i; off[n_docs] > i always
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] > i) hi = mid;
        else lo = mid + 1;
      }
      d = lo - 1;
    } else {
      while (off[d + 1] <= i) ++d;
    }
    return d;
  }
};

// R2 at a line start s with text[s] == '#': the level 1..6, or 0 when the line is no candidate.  `hi` = end of the document.
__device__ __forceinline__ int candidate_level(const unsigned char* text, long long s, long long hi) {
  int k = 1;
  while (k < 7 && s + k < hi && text[s + k] == '#') ++k;
  if (k > 6 || s + k >= hi) return 0;
  return space_len(text + s + k, hi - (s + k)) > 0 ? k : 0;
}

// First '\n' in [q, hi), else hi: 16 bytes at a time once q is aligned (the buffer is readable up to the multiple of 16 behind hi).
__device__ __forceinline__ long long find_newline(const unsigned char* __restrict__ text, long long q, long long hi) {
  for (; q < hi && (q & 15); ++q)
    if (text[q] == '\n') return q;
  for (; q < hi; q += 16) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + q);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned x = w[k] ^ 0x0A0A0A0Au;               // a zero byte where the word holds '\n'
      const unsigned z = (x - 0x01010101u) & ~x & 0x80808080u;   // its lowest set bit marks the first one
      if (z) {
        const long long at = q + 4 * k + ((__ffs(z) - 1) >> 3);
        return at < hi ? at : hi;
      }
    }
  }
  return hi;
}

// One past the last byte of [p, e) that belongs to no trailing white-space character.  Read backwards: the lead bytes of the
// white-space characters occur nowhere else in them, so their occurrences are the same from either end.
__device__ __forceinline__ long long trim_trailing_space(const unsigned char* __restrict__ text, long long p, long long e) {
  while (e > p) {
    if (space_len(text + e - 1, 1) == 1) e -= 1;
    else if (e - p >= 2 && space_len(text + e - 2, 2) == 2) e -= 2;
    else if (e - p >= 3 && space_len(text + e - 3, 3) == 3) e -= 3;
    else break;
  }
  return e;
}

// Bit j set: a candidate starts at byte base + j.  `n` = bytes of the batch; the buffer is readable (zeros) up to base + 16.
__device__ __forceinline__ unsigned slice_candidates(const unsigned char* __restrict__ text, long long n, DocCursor& cur, long long base) {
  const uint4 v = *reinterpret_cast<const uint4*>(text + base);
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
  unsigned any = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const unsigned x = w[q] ^ 0x23232323u;                 // a zero byte where the word holds '#'
    any |= (x - 0x01010101u) & ~x & 0x80808080u;
  }
  if (!any) return 0;
  unsigned mask = 0;
  unsigned prev = base > 0 ? text[base - 1] : '\n';
#pragma unroll
  for (int j = 0; j < CHUNK_LANE_BYTES; ++j) {
    const unsigned c = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
    const long long i = base + j;
    if (c == '#' && i < n) {                               // R1: a line starts behind a '\n' and where a document starts
      const int d = cur.at(i);
      if ((prev == '\n' || cur.off[d] == i) && candidate_level(text, i, cur.off[d + 1]) > 0) mask |= 1u << j;
    }
    prev = c;
  }
  return mask;
}

// Pass 1: candidates per workgroup slice.
__global__ __launch_bounds__(CHUNK_WG) void md_count_candidates_kernel(const unsigned char* __restrict__ text, long long n,
                                                                       const long long* __restrict__ doc_off, int n_docs,
                                                                       int* __restrict__ wg_count) {
  __shared__ int total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  const long long base = ((long long)blockIdx.x * CHUNK_WG + threadIdx.x) * CHUNK_LANE_BYTES;
  if (base < n) {
    DocCursor cur(doc_off, n_docs);
    const int c = __popc(slice_candidates(text, n, cur, base));
    if (c) atomicAdd(&total, c);
  }
  __syncthreads();
  if (threadIdx.x == 0) wg_count[blockIdx.x] = total;
}

// Pass 2: the candidate records, in position order.  A record is a vrag_md_header whose `reserved` holds the end of the match
// (R3's e) and whose block_end is not yet known.
__global__ __launch_bounds__(CHUNK_WG) void md_emit_candidates_kernel(const unsigned char* __restrict__ text, long long n,
                                                                      const long long* __restrict__ doc_off, int n_docs,
                                                                      const int* __restrict__ wg_base, vrag_md_header* __restrict__ cand) {
  __shared__ int scan[CHUNK_WG];
  const int t = threadIdx.x;
  const long long base = ((long long)blockIdx.x * CHUNK_WG + t) * CHUNK_LANE_BYTES;
  DocCursor cur(doc_off, n_docs);
  const unsigned mask = base < n ? slice_candidates(text, n, cur, base) : 0u;
  scan[t] = __popc(mask);
  __syncthreads();
  for (int step = 1; step < CHUNK_WG; step <<= 1) {        // inclusive scan of the lanes' counts
    const int add = t >= step ? scan[t - step] : 0;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  if (!mask) return;
  long long out = (long long)wg_base[blockIdx.x] + scan[t] - __popc(mask);
  DocCursor walk(doc_off, n_docs);
  for (unsigned m = mask; m; m &= m - 1) {
    const long long s = base + (__ffs(m) - 1);
    const int d = walk.at(s);
    const long long lo = doc_off[d], hi = doc_off[d + 1];
    const int k = candidate_level(text, s, hi);
    long long q = s + k, first_nl = -1;
    while (q < hi) {                                       // R3: the white-space run, over line ends if need be
      const int sl = space_len(text + q, hi - q);
      if (sl == 0) break;
      if (text[q] == '\n' && first_nl < 0) first_nl = q;
      q += sl;
    }
    const long long p = q;
    q = find_newline(text, p, hi);
    const long long last = trim_trailing_space(text, p, q);   // one past the last non-space byte of the title
    vrag_md_header h;
    h.doc = d;
    h.level = k;
    h.line_start = (int)(s - lo);
    h.line_end = (int)((first_nl >= 0 ? first_nl : q) - lo);
    h.title_start = (int)(p - lo);
    h.title_end = (int)(last - lo);
    h.block_end = 0;
    h.reserved = (int)(q - lo);
    cand[out++] = h;
  }
}

// The candidates of document d: records are sorted by document.
__device__ __forceinline__ long long first_of_doc(const vrag_md_header* __restrict__ cand, long long n_cand, int d) {
  long long lo = 0, hi = n_cand;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (cand[mid].doc < d) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// step(record) for the candidates of document d in order.  The walk is bound by the latency of the record loads, so eight are in
// flight at a time.
template <typename F>
__device__ __forceinline__ void for_each_candidate(const vrag_md_header* __restrict__ cand, long long n_cand, int d, F&& step) {
  long long i = first_of_doc(cand, n_cand, d);
  const long long end = first_of_doc(cand, n_cand, d + 1);
  for (; i + 8 <= end; i += 8) {
    vrag_md_header c[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) c[u] = cand[i + u];
#pragma unroll
    for (int u = 0; u < 8; ++u) step(c[u]);
  }
  for (; i < end; ++i) step(cand[i]);
}

// Pass 3: headers (R4) and chunks (R5-R7) per document.
__global__ void md_count_records_kernel(const vrag_md_header* __restrict__ cand, long long n_cand, int n_docs, unsigned split_levels,
                                        int include_preamble, int* __restrict__ n_hdr, int* __restrict__ n_chk) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n_docs) return;
  int nh = 0, nc = 0, last_e = -1, first_start = 0;
  for_each_candidate(cand, n_cand, d, [&](const vrag_md_header& c) {
    if (c.line_start <= last_e) return;                    // inside the previous header's match: swallowed
    last_e = c.reserved;
    if (nh == 0) first_start = c.line_start;
    ++nh;
    nc += (split_levels >> c.level) & 1u;
  });
  if (nh == 0) nc = 1;
  else if (include_preamble && first_start > 0) ++nc;
  n_hdr[d] = nh;
  n_chk[d] = nc;
}

// Pass 4: the tables.  The ancestor stack has strictly rising levels, so it is six slots indexed by level (no dynamic indexing).
__global__ void md_write_records_kernel(const vrag_md_header* __restrict__ cand, long long n_cand, const long long* __restrict__ doc_off,
                                        int n_docs, unsigned split_levels, int include_preamble, const long long* __restrict__ hdr_off,
                                        const long long* __restrict__ chk_off, vrag_md_header* __restrict__ headers,
                                        vrag_md_chunk* __restrict__ chunks) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n_docs) return;
  const int n = (int)(doc_off[d + 1] - doc_off[d]);
  long long h_out = hdr_off[d], c_out = chk_off[d];
  long long open_chunk = -1;                               // the chunk of the last header, its end still open
  bool any = false;
  int last_e = -1;
  int slot[7] = {-1, -1, -1, -1, -1, -1, -1};
  for_each_candidate(cand, n_cand, d, [&](vrag_md_header c) {
    if (c.line_start <= last_e) return;
    last_e = c.reserved;
    if (!any) {
      any = true;
      if (include_preamble && c.line_start > 0) {          // R6
        vrag_md_chunk pre;
        pre.doc = d, pre.start = 0, pre.end = c.line_start, pre.header = -1, pre.n_ancestors = 0;
#pragma unroll
        for (int a = 0; a < 5; ++a) pre.ancestors[a] = -1;
        chunks[c_out++] = pre;
      }
    } else {                                               // R7: the previous header's block ends at this line
      headers[h_out - 1].block_end = c.line_start;
      if (open_chunk >= 0) chunks[open_chunk].end = c.line_start;
    }
    open_chunk = -1;
    const int level = c.level;
    c.block_end = n;
    c.reserved = 0;
    headers[h_out] = c;
    if ((split_levels >> level) & 1u) {
      vrag_md_chunk k;
      k.doc = d, k.start = c.line_start, k.end = n, k.header = (int)h_out, k.n_ancestors = 0;
#pragma unroll
      for (int a = 0; a < 5; ++a) k.ancestors[a] = -1;
#pragma unroll
      for (int l = 1; l <= 5; ++l)                         // R8: the stack below this header, outermost first
        if (l < level && slot[l] >= 0) {
#pragma unroll
          for (int a = 0; a < 5; ++a)
            if (a == k.n_ancestors) k.ancestors[a] = slot[l];
          ++k.n_ancestors;
        }
      open_chunk = c_out;
      chunks[c_out++] = k;
    }
#pragma unroll
    for (int l = 1; l <= 6; ++l) {                         // pop every level >= this one, push this header
      if (l > level) slot[l] = -1;
      if (l == level) slot[l] = (int)h_out;
    }
    ++h_out;
  });
  if (!any) {                                              // R5
    vrag_md_chunk whole;
    whole.doc = d, whole.start = 0, whole.end = n, whole.header = -1, whole.n_ancestors = 0;
#pragma unroll
    for (int a = 0; a < 5; ++a) whole.ancestors[a] = -1;
    chunks[c_out] = whole;
  }
}

}  // namespace vrag

using namespace vrag;

extern "C" int vrag_chunk_markdown(const uint8_t* text, const int64_t* doc_off, int32_t n_docs, uint32_t split_levels,
                                   int32_t include_preamble, int64_t header_cap, vrag_md_header* headers, int64_t chunk_cap,
                                   vrag_md_chunk* chunks, int64_t* n_headers, int64_t* n_chunks, int64_t* doc_chunk_off,
                                   int32_t device) {
  ARG_CHECK(doc_off && n_headers && n_chunks && doc_chunk_off && n_docs > 0 && header_cap >= 0 && chunk_cap >= 0,
            "vrag_chunk_markdown: bad arguments");
  ARG_CHECK((headers || header_cap == 0) && (chunks || chunk_cap == 0), "vrag_chunk_markdown: a table with room but no address");
  ARG_CHECK((split_levels & ~0x7Eu) == 0, "vrag_chunk_markdown: split_levels has bits outside levels 1..6");
  ARG_CHECK(doc_off[0] == 0, "vrag_chunk_markdown: doc_off[0] must be 0");
  for (int d = 0; d < n_docs; ++d)
    ARG_CHECK(doc_off[d + 1] >= doc_off[d] && doc_off[d + 1] - doc_off[d] <= 0x7fffffffll,
              "vrag_chunk_markdown: document %d has a negative or > 2 GiB length", d);
  const int64_t n = doc_off[n_docs];
  ARG_CHECK(n <= VRAG_MD_MAX_BATCH_BYTES, "vrag_chunk_markdown: %lld bytes of text, at most %lld per call", (long long)n,
            (long long)VRAG_MD_MAX_BATCH_BYTES);
  ARG_CHECK(text || n == 0, "vrag_chunk_markdown: no text");
  if (vrag_device_count() <= device || device < 0) {
    set_error("no HIP device %d visible (no CPU fallback)", device);
    return VRAG_ERR_NO_DEVICE;
  }
  const int n_wg = (int)((n + CHUNK_WG_BYTES - 1) / CHUNK_WG_BYTES);
  const int doc_grid = (n_docs + 127) / 128;
  std::vector<int> wg_count(n_wg), n_hdr(n_docs), n_chk(n_docs);
  std::vector<long long> hdr_off((size_t)n_docs + 1);
  int64_t n_cand = 0, need_h = 0, need_c = 0;
  bool fits = true;
  hipStream_t st = nullptr;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  {
    DevBuf d_text, d_off, d_wg, d_cand, d_nh, d_nc, d_hoff, d_coff, d_headers, d_chunks;   // freed before the stream is destroyed
    const size_t padded = ((size_t)n + 15) / 16 * 16 + 16;  // lanes read whole 16-byte slices
    if (e == hipSuccess) e = d_text.alloc(padded);
    if (e == hipSuccess) e = d_off.alloc((size_t)(n_docs + 1) * 8);
    if (e == hipSuccess) e = d_wg.alloc((size_t)n_wg * 4);
    const size_t tail = (size_t)n / 16 * 16;                // zeros behind the text, up to the end of the last slice
    if (e == hipSuccess) e = hipMemsetAsync((char*)d_text.p + tail, 0, padded - tail, st);
    if (e == hipSuccess && n) e = hipMemcpyAsync(d_text.p, text, (size_t)n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off.p, doc_off, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && n_wg) {
      hipLaunchKernelGGL(md_count_candidates_kernel, dim3(n_wg), dim3(CHUNK_WG), 0, st, d_text.as<unsigned char>(), (long long)n,
                         d_off.as<long long>(), n_docs, d_wg.as<int>());
      e = hipGetLastError();
      if (e == hipSuccess) e = hipMemcpyAsync(wg_count.data(), d_wg.p, (size_t)n_wg * 4, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
      for (int b = 0; b < n_wg; ++b) {                      // exclusive prefix sum; at most n / 2 candidates: fits an int
        const int c = wg_count[b];
        wg_count[b] = (int)n_cand;
        n_cand += c;
      }
      e = d_cand.alloc((size_t)n_cand * sizeof(vrag_md_header));
    }
    if (e == hipSuccess && n_cand) {
      e = hipMemcpyAsync(d_wg.p, wg_count.data(), (size_t)n_wg * 4, hipMemcpyHostToDevice, st);
      if (e == hipSuccess) {
        hipLaunchKernelGGL(md_emit_candidates_kernel, dim3(n_wg), dim3(CHUNK_WG), 0, st, d_text.as<unsigned char>(), (long long)n,
                           d_off.as<long long>(), n_docs, d_wg.as<int>(), d_cand.as<vrag_md_header>());
        e = hipGetLastError();
      }
    }
    if (e == hipSuccess) e = d_nh.alloc((size_t)n_docs * 4);
    if (e == hipSuccess) e = d_nc.alloc((size_t)n_docs * 4);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(md_count_records_kernel, dim3(doc_grid), dim3(128), 0, st, d_cand.as<vrag_md_header>(), (long long)n_cand,
                         n_docs, split_levels, include_preamble, d_nh.as<int>(), d_nc.as<int>());
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(n_hdr.data(), d_nh.p, (size_t)n_docs * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(n_chk.data(), d_nc.p, (size_t)n_docs * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
      for (int d = 0; d < n_docs; ++d) {
        hdr_off[d] = need_h;
        doc_chunk_off[d] = need_c;
        need_h += n_hdr[d];
        need_c += n_chk[d];
      }
      hdr_off[n_docs] = need_h;
      doc_chunk_off[n_docs] = need_c;
      *n_headers = need_h;
      *n_chunks = need_c;
    }
    fits = need_h <= header_cap && need_c <= chunk_cap;
    if (e == hipSuccess && fits) {
      e = d_hoff.alloc((size_t)(n_docs + 1) * 8);
      if (e == hipSuccess) e = d_coff.alloc((size_t)(n_docs + 1) * 8);
      if (e == hipSuccess) e = d_headers.alloc((size_t)need_h * sizeof(vrag_md_header));
      if (e == hipSuccess) e = d_chunks.alloc((size_t)need_c * sizeof(vrag_md_chunk));
      if (e == hipSuccess) e = hipMemcpyAsync(d_hoff.p, hdr_off.data(), (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, st);
      if (e == hipSuccess) e = hipMemcpyAsync(d_coff.p, doc_chunk_off, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, st);
      if (e == hipSuccess) {
        hipLaunchKernelGGL(md_write_records_kernel, dim3(doc_grid), dim3(128), 0, st, d_cand.as<vrag_md_header>(), (long long)n_cand,
                           d_off.as<long long>(), n_docs, split_levels, include_preamble, d_hoff.as<long long>(),
                           d_coff.as<long long>(), d_headers.as<vrag_md_header>(), d_chunks.as<vrag_md_chunk>());
        e = hipGetLastError();
      }
      if (e == hipSuccess && need_h)
        e = hipMemcpyAsync(headers, d_headers.p, (size_t)need_h * sizeof(vrag_md_header), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess && need_c)
        e = hipMemcpyAsync(chunks, d_chunks.p, (size_t)need_c * sizeof(vrag_md_chunk), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
  }
  if (st) (void)hipStreamDestroy(st);
  if (e != hipSuccess) {
    set_error("vrag_chunk_markdown: %s", hipGetErrorString(e));
    return VRAG_ERR_HIP;
  }
  if (!fits) {
    set_error("vrag_chunk_markdown: %lld headers / %lld chunks do not fit header_cap %lld / chunk_cap %lld", (long long)need_h,
              (long long)need_c, (long long)header_cap, (long long)chunk_cap);
    return VRAG_ERR_CAPACITY;
  }
  return VRAG_OK;
}
