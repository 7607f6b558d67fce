// Row filter: the store's boolean metadata filters evaluated over typed columns in HBM + C ABI (include/vrag_amd.h, vrag_row_filter_*).
//
// What it replaces: one Python predicate call per stored row for every filter that is no single `==` / `in` comparison
// (vector_stores.py, GpuVectorStore._mask_locked) -- 0.5 - 0.9 s per 10^6 rows, again after every insert.  Here a metadata key named
// by a filter is a COLUMN of (kind, payload) per row -- 1 + 8 bytes -- appended to as rows arrive, the filter is a postfix program
// over leaves (store_filter.py, compile_filter), and one kernel writes the row bitmap.
//
// row_filter_eval_kernel: one lane per row, one wave per group of 64 rows, waves stride over the groups.
//   program   leaves, ops and the column addresses are a by-value kernel argument (2 KB of the 4 KB a launch may carry): every
//             access is wave-uniform, so they are read through the scalar cache and cost no LDS and no upload of their own
//   stack     the bits of ONE 32-bit register per lane: push = shift left and or, AND / OR = fold bit 0 into bit 1 and shift
//             right, NOT = flip bit 0.  Depth <= 32 is checked on the host.  No indexed private array, so nothing can go to scratch
//   columns   a leaf reads kinds[r] and payload[r] of its column, consecutive lanes consecutive rows (64 B + 512 B per wave and
//             column).  Two leaves on one column read the same lines again: those hit the vector cache, HBM sees 9 bytes per row
//             and referenced column
//   strings   a table leaf reads tables[off + code / 32] only for code < table_codes -- a code at or beyond the leaf's table (a
//             string the table was not resolved for) does not match, and nothing behind a table is read.  A table comes from the
//             host with the program or is written in place by the match kernel of csrc/strmatch.hip (vrag_row_filter_eval_matched);
//             this kernel does not know which
//   result    the wave's 64 answers are one ballot; lanes 0 and 1 store its two 32-bit words.  Lanes at and beyond n_rows read
//             nothing and are masked out of the ballot, so the tail bits of the last group are zero.  The device buffer holds two words per group; the host copies
//             ceil(n_rows / 32) of them
// Number comparisons are the hardware's IEEE f64 comparisons (-0.0 == 0.0, infinities ordered, NaN unordered).
#include "../../include/vrag_amd.h"

#include <algorithm>
#include <cstring>
#include <vector>

#include "rowfilter.h"

namespace vrag {
namespace {

constexpr int RF_MAX_HANDLE_COLUMNS = 4096;   // RF_WAVES, the op bytes, LeafDev, EvalArgs, num_answer: rowfilter.h (csrc/listfilter.hip shares them)

__global__ __launch_bounds__(64 * RF_WAVES) void row_filter_eval_kernel(const EvalArgs a, const unsigned* __restrict__ tables,
                                                                         long long n_rows, long long n_groups,
                                                                         unsigned* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * RF_WAVES;
  for (long long g = (long long)blockIdx.x * RF_WAVES + (threadIdx.x >> 6); g < n_groups; g += stride) {
    const long long r = g * 64 + lane;
    const bool in = r < n_rows;
    unsigned stk = 0u;
    for (int i = 0; i < a.n_ops; ++i) {
      const unsigned op = (a.ops[i >> 2] >> ((i & 3) * 8)) & 0xffu;
      if (op < RF_AND) {
        const LeafDev& lf = a.leaves[op];
        bool bit = false;
        if (in) {
          const unsigned kind = a.kinds[lf.slot][r];
          const u64 pay = a.payload[lf.slot][r];
          if (kind == VRAG_FILTER_KIND_NUMBER) {
            bit = num_answer(lf.num_op, __longlong_as_double((long long)pay), lf.bound);
          } else if (kind == VRAG_FILTER_KIND_STRING) {
            bit = lf.str_mode == VRAG_FILTER_STR_ALWAYS;
            if (lf.str_mode == VRAG_FILTER_STR_TABLE && pay < (u64)lf.table_codes)
              bit = (tables[(size_t)lf.table_off + (size_t)(pay >> 5)] >> (unsigned)(pay & 31ull)) & 1u;
          } else if (kind == VRAG_FILTER_KIND_BOOL) {
            bit = (lf.bits >> (1u + (unsigned)(pay & 1ull))) & 1u;
          } else {
            bit = lf.bits & 1u;
          }
        }
        stk = (stk << 1) | (bit ? 1u : 0u);
      } else if (op == RF_AND) {
        stk = (stk >> 1) & ((stk & 1u) | ~1u);
      } else if (op == RF_OR) {
        stk = (stk >> 1) | (stk & 1u);
      } else {
        stk ^= 1u;
      }
    }
    const u64 m = __ballot(in && (stk & 1u) != 0u);   // every lane of the wave is here (the loops above are wave-uniform); a NOT
                                                      // turns the 0 of a lane behind n_rows into 1, so `in` decides once more
    if (lane < 2) out[2 * g + lane] = lane ? (unsigned)(m >> 32) : (unsigned)(m & 0xffffffffull);
  }
}

}  // namespace
}  // namespace vrag

using namespace vrag;

extern "C" {

int vrag_row_filter_create(int32_t device, vrag_row_filter** out) {
  ARG_CHECK(out, "null argument");
  *out = nullptr;
  ARG_CHECK(device >= 0, "vrag_row_filter_create: negative device");
  DEVICE_CHECK(device);
  HIP_TRY(hipSetDevice(device));
  auto* f = new vrag_row_filter();
  f->device = device;
  const hipError_t e = hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    set_error("row filter stream creation failed: %s", hipGetErrorString(e));
    vrag_row_filter_destroy(f);
    return VRAG_ERR_HIP;
  }
  *out = f;
  return VRAG_OK;
}

void vrag_row_filter_destroy(vrag_row_filter* f) {
  if (!f) return;
  (void)hipSetDevice(f->device);
  if (f->stream) {
    (void)hipStreamSynchronize(f->stream);
    (void)hipStreamDestroy(f->stream);
  }
  delete f;   // the device arrays free themselves
}

int vrag_row_filter_add_column(vrag_row_filter* f, int32_t* col_out) {
  ARG_CHECK(f && col_out, "null argument");
  std::lock_guard<std::mutex> lk(f->mu);
  ARG_CHECK((int)f->cols.size() < RF_MAX_HANDLE_COLUMNS, "a row filter holds at most %d columns", RF_MAX_HANDLE_COLUMNS);
  f->cols.emplace_back();
  *col_out = (int32_t)f->cols.size() - 1;
  return VRAG_OK;
}

int vrag_row_filter_append(vrag_row_filter* f, int32_t col, const uint8_t* kinds, const uint64_t* payload, int64_t n) {
  ARG_CHECK(f, "null argument");
  ARG_CHECK(n >= 0 && (n == 0 || (kinds && payload)), "vrag_row_filter_append: need n >= 0 and both arrays");
  std::lock_guard<std::mutex> lk(f->mu);
  ARG_CHECK(col >= 0 && col < (int)f->cols.size(), "vrag_row_filter_append: no column %d (the filter holds %d)", col, (int)f->cols.size());
  for (int64_t i = 0; i < n; ++i)
    ARG_CHECK(kinds[i] <= VRAG_FILTER_KIND_BOOL, "vrag_row_filter_append: kinds[%lld] = %d is no VRAG_FILTER_KIND_*", (long long)i, (int)kinds[i]);
  if (n == 0) return VRAG_OK;
  FilterColumn& c = f->cols[col];
  HIP_TRY(hipSetDevice(f->device));
  const size_t need = (size_t)c.n + (size_t)n;
  if (need > c.kinds.n) {   // geometric growth; the rows held so far move into the new arrays
    const size_t cap = std::max<size_t>(need, std::max<size_t>(2 * c.kinds.n, 256));
    DevArray<unsigned char> nk;
    DevArray<u64> np;
    HIP_TRY(nk.grow(cap));
    HIP_TRY(np.grow(cap));
    if (c.n) {
      HIP_TRY(hipMemcpyAsync(nk.p, c.kinds.p, (size_t)c.n, hipMemcpyDeviceToDevice, f->stream));
      HIP_TRY(hipMemcpyAsync(np.p, c.payload.p, (size_t)c.n * sizeof(u64), hipMemcpyDeviceToDevice, f->stream));
      HIP_TRY(hipStreamSynchronize(f->stream));   // the old arrays are freed by the assignments below
    }
    c.kinds = std::move(nk);
    c.payload = std::move(np);
  }
  HIP_TRY(hipMemcpyAsync(c.kinds.p + c.n, kinds, (size_t)n, hipMemcpyHostToDevice, f->stream));
  HIP_TRY(hipMemcpyAsync(c.payload.p + c.n, payload, (size_t)n * sizeof(u64), hipMemcpyHostToDevice, f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));   // the caller's arrays are free again
  c.n += n;
  return VRAG_OK;
}

int vrag_row_filter_rows(vrag_row_filter* f, int32_t col, int64_t* n) {
  ARG_CHECK(f && n, "null argument");
  std::lock_guard<std::mutex> lk(f->mu);
  ARG_CHECK(col >= 0 && col < (int)f->cols.size(), "vrag_row_filter_rows: no column %d (the filter holds %d)", col, (int)f->cols.size());
  *n = f->cols[col].n;
  return VRAG_OK;
}

// Drops the rows whose bit is cleared from every column, in place (csrc/compact.h).  Columns are extended lazily, so a column may
// hold fewer rows than the bitmap covers: its rows are compacted under the bitmap's prefix.  The dictionaries hold strings, not rows.
// A call that drops a row DROPS every column's list part (n_list_rows = 0; the allocation stays for the re-append): the store
// re-appends it from its host column before the next list filter.  A CSR compaction on the device would be two more kernels for
// arrays the host holds compacted anyway.
int vrag_row_filter_compact(vrag_row_filter* f, const uint32_t* keep_words, int64_t n_keep) {
  ARG_CHECK(f, "null argument");
  ARG_CHECK(n_keep >= 0 && (keep_words || n_keep == 0), "bad row bitmap (null words or a negative length)");
  std::lock_guard<std::mutex> lk(f->mu);
  for (const FilterColumn& c : f->cols)
    ARG_CHECK(c.n <= n_keep && c.n_list_rows <= n_keep, "the bitmap covers %lld rows, a column holds %lld",
              (long long)n_keep, (long long)std::max(c.n, c.n_list_rows));
  if (n_keep == 0 || f->cols.empty()) return VRAG_OK;
  HIP_TRY(hipSetDevice(f->device));
  int rc;
  if ((rc = compact_plan(f->compact, keep_words, n_keep, f->stream))) return rc;
  if (f->compact.n_keep == n_keep) return VRAG_OK;   // nothing to drop: no launch
  for (FilterColumn& c : f->cols) c.n_list_rows = c.n_elems = 0;
  for (FilterColumn& c : f->cols) {
    if (c.n == 0) continue;
    if ((rc = compact_rows(f->compact, c.kinds.p, 1, c.n, f->stream))) return rc;
    if ((rc = compact_rows(f->compact, c.payload.p, sizeof(u64), c.n, f->stream))) return rc;
  }
  HIP_TRY(hipStreamSynchronize(f->stream));
  for (FilterColumn& c : f->cols) c.n = f->compact.kept_before(c.n);
  return VRAG_OK;
}

}  // extern "C"

// vrag_row_filter_eval, _eval_matched and _eval_lists (`who` names the one called): the matches of the latter two fill their
// leaves' tables in device memory between the upload of `tables` and the eval kernel.  Only _eval_lists (`lists`) takes
// VRAG_FILTER_OP_LIST_ANY; a program that holds one runs on the kernel of csrc/listfilter.hip, every other program on
// row_filter_eval_kernel with the arguments it always had.
static int eval_program(const char* who, bool lists, vrag_row_filter* f, const vrag_filter_leaf* leaves, int32_t n_leaves, const uint32_t* ops,
                        int32_t n_ops, const uint32_t* tables, int64_t n_table_words, const vrag_filter_match* matches, int32_t n_matches,
                        const uint8_t* texts, int64_t n_text_bytes, int64_t n_rows, uint32_t* out_words, void* stream) {
  ARG_CHECK(f && leaves && ops, "null argument");
  ARG_CHECK(n_leaves >= 1 && n_leaves <= VRAG_FILTER_MAX_LEAVES, "%s: 1 <= n_leaves <= %d (got %d)", who,
            VRAG_FILTER_MAX_LEAVES, n_leaves);
  ARG_CHECK(n_ops >= 1 && n_ops <= VRAG_FILTER_MAX_OPS, "%s: 1 <= n_ops <= %d (got %d)", who, VRAG_FILTER_MAX_OPS, n_ops);
  ARG_CHECK(n_table_words >= 0 && n_table_words <= 0x7fffffffll && (n_table_words == 0 || tables),
            "%s: bad table array (%lld words)", who, (long long)n_table_words);
  ARG_CHECK(n_rows >= 0, "%s: negative n_rows", who);
  ARG_CHECK(n_rows == 0 || out_words, "%s: null out_words", who);
  EvalArgs args;
  ListArgs largs;
  std::memset(&args, 0, sizeof(args));
  std::memset(&largs, 0, sizeof(largs));
  // the op list: no underflow, depth <= 32, one value left
  int depth = 0;
  bool as_row[VRAG_FILTER_MAX_LEAVES] = {}, as_list[VRAG_FILTER_MAX_LEAVES] = {};   // how the ops push each leaf
  bool any_list = false;
  for (int i = 0; i < n_ops; ++i) {
    const uint32_t code = ops[i] & 0xffu, leaf = ops[i] >> 8;
    unsigned char byte = 0;
    if (code == VRAG_FILTER_OP_LEAF || (lists && code == VRAG_FILTER_OP_LIST_ANY)) {
      ARG_CHECK(leaf < (uint32_t)n_leaves, "%s: ops[%d] pushes leaf %u of %d", who, i, leaf, n_leaves);
      ARG_CHECK(depth < VRAG_FILTER_MAX_DEPTH, "%s: stack deeper than %d at ops[%d]", who, VRAG_FILTER_MAX_DEPTH, i);
      ++depth;
      if (code == VRAG_FILTER_OP_LEAF) {
        byte = (unsigned char)leaf, as_row[leaf] = true;
      } else {
        byte = (unsigned char)(RF_LIST_ANY + leaf), as_list[leaf] = any_list = true;
      }
    } else if (code == VRAG_FILTER_OP_AND || code == VRAG_FILTER_OP_OR) {
      ARG_CHECK(leaf == 0 && depth >= 2, "%s: stack underflow at ops[%d]", who, i);
      --depth;
      byte = code == VRAG_FILTER_OP_AND ? RF_AND : RF_OR;
    } else {
      ARG_CHECK(code == VRAG_FILTER_OP_NOT && leaf == 0, "%s: ops[%d] = 0x%x is no operation", who, i, ops[i]);
      ARG_CHECK(depth >= 1, "%s: stack underflow at ops[%d]", who, i);
      byte = RF_NOT;
    }
    args.ops[i >> 2] |= (unsigned)byte << ((i & 3) * 8);
  }
  ARG_CHECK(depth == 1, "%s: the program leaves %d values on the stack (one expected)", who, depth);
  args.n_ops = n_ops;

  std::lock_guard<std::mutex> lk(f->mu);
  int slot_col[VRAG_FILTER_MAX_COLUMNS];
  bool slot_rows[VRAG_FILTER_MAX_COLUMNS] = {}, slot_lists[VRAG_FILTER_MAX_COLUMNS] = {};   // which part of the column is checked and bound
  int n_slots = 0;
  for (int l = 0; l < n_leaves; ++l) {
    const vrag_filter_leaf& in = leaves[l];
    ARG_CHECK(in.column >= 0 && in.column < (int)f->cols.size(), "%s: leaf %d names column %d (the filter holds %d)", who, l,
              in.column, (int)f->cols.size());
    ARG_CHECK(in.num_op <= VRAG_FILTER_NUM_GE && in.str_mode <= VRAG_FILTER_STR_TABLE && in.bool_bits <= 3 && in.other_bit <= 1,
              "%s: leaf %d has a field out of range", who, l);
    LeafDev& lf = args.leaves[l];
    if (in.str_mode == VRAG_FILTER_STR_TABLE) {
      ARG_CHECK(in.table_off >= 0 && in.table_codes >= 0 && in.table_codes <= 0xffffffffll &&
                    in.table_off <= n_table_words && (in.table_codes + 31) / 32 <= n_table_words - in.table_off,
                "%s: leaf %d's table (offset %lld, %lld codes) lies outside the %lld table words", who, l,
                (long long)in.table_off, (long long)in.table_codes, (long long)n_table_words);
      lf.table_off = (unsigned)in.table_off, lf.table_codes = (unsigned)in.table_codes;
    }
    int slot = 0;
    while (slot < n_slots && slot_col[slot] != in.column) ++slot;
    if (slot == n_slots) {
      ARG_CHECK(n_slots < VRAG_FILTER_MAX_COLUMNS, "%s: the leaves name more than %d columns", who, VRAG_FILTER_MAX_COLUMNS);
      slot_col[n_slots++] = in.column;
    }
    const FilterColumn& c = f->cols[in.column];
    // a leaf reads the rows of its column, unless list ops alone push it: then it reads the column's list part
    if ((as_row[l] || !as_list[l]) && !slot_rows[slot]) {
      ARG_CHECK(n_rows <= c.n, "%s: n_rows = %lld but column %d holds %lld rows", who, (long long)n_rows, in.column, c.n);
      slot_rows[slot] = true;
      args.kinds[slot] = c.kinds.p, args.payload[slot] = c.payload.p;
    }
    if (as_list[l] && !slot_lists[slot]) {
      ARG_CHECK(n_rows <= c.n_list_rows, "%s: n_rows = %lld but column %d holds the lists of %lld rows", who, (long long)n_rows,
                in.column, c.n_list_rows);
      slot_lists[slot] = true;
      largs.list_off[slot] = c.list_off.p, largs.elem_kinds[slot] = c.elem_kinds.p, largs.elem_payload[slot] = c.elem_payload.p;
    }
    lf.bound = in.bound;
    lf.slot = (unsigned char)slot, lf.num_op = in.num_op, lf.str_mode = in.str_mode;
    lf.bits = (unsigned char)(in.other_bit | (in.bool_bits << 1));
  }
  ARG_CHECK(n_matches >= 0 && n_matches <= n_leaves && (n_matches == 0 || matches), "%s: 0 <= n_matches <= n_leaves (got %d)", who,
            n_matches);
  ARG_CHECK(n_text_bytes >= 0 && (n_text_bytes == 0 || texts), "%s: bad text array (%lld bytes)", who, (long long)n_text_bytes);
  std::vector<MatchProg> progs((size_t)n_matches);
  for (int m = 0; m < n_matches; ++m) {
    const vrag_filter_match& mt = matches[m];
    ARG_CHECK(mt.leaf >= 0 && mt.leaf < n_leaves && leaves[mt.leaf].str_mode == VRAG_FILTER_STR_TABLE,
              "%s: match %d names leaf %d, which is no table leaf", who, m, mt.leaf);
    ARG_CHECK(mt.text_len >= 0 && mt.text_off >= 0 && mt.text_off <= n_text_bytes && mt.text_len <= n_text_bytes - mt.text_off,
              "%s: match %d's text (offset %lld, %d bytes) lies outside the %lld text bytes", who, m, (long long)mt.text_off,
              mt.text_len, (long long)n_text_bytes);
    const FilterColumn& c = f->cols[leaves[mt.leaf].column];
    ARG_CHECK(leaves[mt.leaf].table_codes <= c.n_codes, "%s: match %d asks for %lld codes but column %d's dictionary holds %lld", who, m,
              (long long)leaves[mt.leaf].table_codes, leaves[mt.leaf].column, c.n_codes);
    const int rc = match_compile(who, mt.op, texts ? texts + mt.text_off : nullptr, mt.text_len, &progs[(size_t)m]);
    if (rc != VRAG_OK) return rc;
  }
  if (n_rows == 0) return VRAG_OK;

  HIP_TRY(hipSetDevice(f->device));
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : f->stream;
  const long long n_groups = (n_rows + 63) / 64;
  const size_t n_words = (size_t)((n_rows + 31) / 32);
  HIP_TRY(f->d_out.grow((size_t)n_groups * 2));
  HIP_TRY(f->d_tables.grow((size_t)std::max<long long>(n_table_words, 1)));
  if (n_table_words) HIP_TRY(hipMemcpyAsync(f->d_tables.p, tables, (size_t)n_table_words * sizeof(unsigned), hipMemcpyHostToDevice, st));
  for (int m = 0; m < n_matches; ++m) {   // stream order: behind the upload, in front of the eval kernel
    const vrag_filter_leaf& in = leaves[matches[m].leaf];
    HIP_TRY(match_launch(f->cols[in.column], progs[(size_t)m], in.table_codes, f->d_tables.p + in.table_off, st));
  }
  if (any_list) {
    HIP_TRY(list_eval_launch(args, largs, f->d_tables.p, (long long)n_rows, f->d_out.p, st));
  } else {
    const unsigned blocks = (unsigned)std::min<long long>((n_groups + RF_WAVES - 1) / RF_WAVES, RF_MAX_BLOCKS);
    hipLaunchKernelGGL(row_filter_eval_kernel, dim3(blocks), dim3(64 * RF_WAVES), 0, st, args, f->d_tables.p, (long long)n_rows, n_groups,
                       f->d_out.p);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(out_words, f->d_out.p, n_words * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return VRAG_OK;
}

extern "C" {

int vrag_row_filter_eval(vrag_row_filter* f, const vrag_filter_leaf* leaves, int32_t n_leaves, const uint32_t* ops, int32_t n_ops,
                         const uint32_t* tables, int64_t n_table_words, int64_t n_rows, uint32_t* out_words, void* stream) {
  return eval_program("vrag_row_filter_eval", false, f, leaves, n_leaves, ops, n_ops, tables, n_table_words, nullptr, 0, nullptr, 0, n_rows,
                      out_words, stream);
}

int vrag_row_filter_eval_matched(vrag_row_filter* f, const vrag_filter_leaf* leaves, int32_t n_leaves, const uint32_t* ops, int32_t n_ops,
                                 const uint32_t* tables, int64_t n_table_words, const vrag_filter_match* matches, int32_t n_matches,
                                 const uint8_t* texts, int64_t n_text_bytes, int64_t n_rows, uint32_t* out_words, void* stream) {
  return eval_program("vrag_row_filter_eval_matched", false, f, leaves, n_leaves, ops, n_ops, tables, n_table_words, matches, n_matches,
                      texts, n_text_bytes, n_rows, out_words, stream);
}

int vrag_row_filter_eval_lists(vrag_row_filter* f, const vrag_filter_leaf* leaves, int32_t n_leaves, const uint32_t* ops, int32_t n_ops,
                               const uint32_t* tables, int64_t n_table_words, const vrag_filter_match* matches, int32_t n_matches,
                               const uint8_t* texts, int64_t n_text_bytes, int64_t n_rows, uint32_t* out_words, void* stream) {
  return eval_program("vrag_row_filter_eval_lists", true, f, leaves, n_leaves, ops, n_ops, tables, n_table_words, matches, n_matches,
                      texts, n_text_bytes, n_rows, out_words, stream);
}

}  // extern "C"
