"""One table of searches that, between them, launch every instantiation csrc/topk.hip compiles for its dense scan, prefilter,
sparse and per-query merge kernels (tests/test_topk_instantiations_host.py checks the table, tests/test_topk_instantiations_gpu.py
runs it).  A row is

    Case(kind, dtype, dim, n, nq, k, data, expect, lim_x, lim_q, via)

kind    "dense" | "sparse"
dtype   dense: "bf16" | "f32" | "f32+image" (fp32 rows with the bf16 prefilter image); sparse: "csr"
dim     dense: the row width; sparse: the vocabulary
n       rows / documents
data    "grid"        rows and queries are integers in [-lim_x, lim_x] / 64 and [-lim_q, lim_q] / 64: every partial sum of a dot product
                      is an integer of at most 2^24 in grid units, exact in fp32 in any order (dim * lim_x * lim_q <= 2^24, checked on the
                      host; sparse: positive weights, and the longest document's term count stands for dim)
        "grid_pairs"  the same rows; queries are 9- to 11-bit integers / 256, fp32 numbers that are NOT bf16 numbers
        "tail_last"   grid data where every row equals one base row except in its LAST 8 columns: a lane's final chunk decides the ranking
        "tail_first"  the same with the FIRST 8 columns
        "gauss"       normalised Gaussian rows and queries (sparse: |Gaussian| weights): only where the route's contract is the oracle's
                      sequential fmaf chain -- the exact kernels, the prefilter route and all of sparse
        "bunched"     fp32 + image only: 4 160 of the 4 224 rows are copies of one grid row and query 0 is that row, so more rows reach the
                      one-pass route's entry threshold than its 4 096 candidate slots hold and the 64 best image scores of the batch
                      route are equal: the prefilter flags the query and the full scan behind the flags answers it
        sparse only:  "union1023" / "union1024": sixteen queries whose term union is exactly that many distinct terms
expect  the set of (launch id, p0, p1) the search must log (include/vrag_amd_debug.h: the enum VRAG_DEBUG_TOPK_LAUNCH_* and its
        table of template parameters) -- all of it, nothing else
via     "host" = vrag_*_index_search, "device" = vrag_dense_index_search_device

Out of scope here: the tiled search's kernels (tests/test_topk_unit_gpu.py; they run inside some of these searches and are not
logged), the filtered kernels (tests/test_filtered_topk_gpu.py), IVF, SQ8 and the shard merge.

Shapes are the smallest that still select each kernel: bf16 shards below 4 096 rows (or 4 097 rows at a width that is no multiple
of 64) keep the tiled search out; fp32 + image shards have 4 097 or 4 224 rows because the prefilter route starts at 4 096."""
from collections import namedtuple

Case = namedtuple("Case", "kind dtype dim n nq k data expect lim_x lim_q via")

ML, MS = ("MERGE_LISTS", 0, 0), ("MERGE_SCAN", 0, 0)

# every (id, p0, p1) csrc/topk.hip instantiates for the logged kernels
ALL = frozenset(
    [("DENSE_BF16", qt, dc) for qt, dcs in ((1, (0, 3, 6, 8, 12)), (4, (0, 3, 6, 8))) for dc in dcs]
    + [("DENSE_F32", qt, dc) for qt, dcs in ((1, (0, 3, 6, 8, 12)), (4, (0, 3, 6, 8))) for dc in dcs]
    + [("MFMA", 0, 0), ("MFMA2", 6, 0), ("MFMA2", 12, 0), ("MFMA2", 16, 0)]
    + [("EXACT", 6, 0), ("EXACT", 3, 0), ("EXACT2", 12, 0), ("EXACT2", 24, 0), ("SEED_THRESHOLD", 0, 0)]
    + [("PF_PREFIX", dc, 0) for dc in (0, 3, 6)] + [("PF_COLLECT", dc, 0) for dc in (0, 3, 6)]
    + [("PF_COLLECT_MULTI", d32, qn) for d32 in (1, 2, 3) for qn in (2, 4)]
    + [("PF_RESCORE_LIST", 0, 0), ("PF_RESCORE_LIST", 1, 0), ("PF_RESCORE", 0, 0), ("PF_COMBINE", 0, 0)]
    + [("SPARSE", 0, 0), ("SPARSE", 1, 0), ("SPARSE_SCATTER", 0, 0)]
    + [("SPARSE_MULTI", 16, 4), ("SPARSE_MULTI", 16, 0), ("SPARSE_MULTI", 8, 0)]
    + [ML, MS])

# (id, p0, p1) -> the predicate of csrc/topk.hip that keeps the selection code from ever launching it.  Empty: the one candidate,
# prefilter_prefix_kernel<8> / prefilter_collect_kernel<8> (dim 1024), was dead -- prefilter_route_ok admits the route only where
# dense_use_exact(1, dim, k) holds, i.e. dim <= 768 -- and its instantiation is deleted instead of being listed here.
UNREACHABLE = {}

CASES = []


def _add(kind, dtype, dim, n, nq, k, data, expect, lim_x=64, lim_q=64, via="host"):
    c = Case(kind, dtype, dim, n, nq, k, data, frozenset(expect), lim_x, lim_q, via)
    if c not in CASES:   # the loops below meet some shapes twice
        CASES.append(c)


def _with_tails(dtype, dim, n, nq, k, expect, first="grid"):
    for data in (first, "tail_last", "tail_first"):
        _add("dense", dtype, dim, n, nq, k, data, expect)


NS = (1, 127, 129, 2049, 4095)

# ---------------------------------------------------------------- bf16 rows, scalar kernel, one query: <false, 1, DIMC>
# DIMC = dim / 128 where an instantiation exists (384, 768, 1024, 1536), else the generic loop -- at 24, 72, 136, 264 and 1000 the
# lanes of a 16-lane group make different numbers of steps (dim / 8 % 16 != 0)
for i, (dim, dimc) in enumerate(((8, 0), (24, 0), (72, 0), (136, 0), (264, 0), (1000, 0), (4096, 0), (384, 3), (768, 6), (1024, 8), (1536, 12))):
    _with_tails("bf16", dim, 129, 1, 10, {("DENSE_BF16", 1, dimc), ML})
    _add("dense", "bf16", dim, NS[i % 5], 1, 10, "grid", {("DENSE_BF16", 1, dimc), ML})
    _add("dense", "bf16", dim, NS[(i + 3) % 5], 1, 33 if i % 2 else 32, "grid", {("DENSE_BF16", 1, dimc), MS if i % 2 else ML})

# ---------------------------------------------------------------- bf16 rows, scalar kernel, four queries per pass: <false, 4, DIMC>
# nq = 5 is one pass of four and a single; 384 / 768 at k = 17 and 1024 at k = 9 because the matrix-core kernels stop at k = 16 / 8
# there; 1536 has no <4, 12>: its batches take the generic loop and the single behind them <1, 12>
for i, (dim, k, dc4, dc1) in enumerate(((24, 10, 0, 0), (136, 10, 0, 0), (264, 10, 0, 0), (1000, 10, 0, 0), (384, 17, 3, 3), (768, 17, 6, 6),
                                        (1024, 9, 8, 8), (1536, 10, 0, 12))):
    _with_tails("bf16", dim, 129, 4, k, {("DENSE_BF16", 4, dc4), ML})
    _add("dense", "bf16", dim, NS[(i + 1) % 4 + 1], 2, k, "grid", {("DENSE_BF16", 4, dc4), ML})
    _add("dense", "bf16", dim, NS[(i + 2) % 4 + 1], 5, k, "grid", {("DENSE_BF16", 4, dc4), ("DENSE_BF16", 1, dc1), ML})
for dim in (24, 136, 264, 1000):   # 4 097 rows: only the width keeps the tiled search out
    _add("dense", "bf16", dim, 4097, 5, 10, "grid", {("DENSE_BF16", 4, 0), ("DENSE_BF16", 1, 0), ML})

# ---------------------------------------------------------------- bf16 rows, first-generation matrix-core kernel
# admitted while 32 * dim * 2 + 5 * 16384 + 256 * k * 8 <= 160 KiB: k = 16 up to dim 768, k <= 12 at 896, k <= 4 at 1152; the first
# refused k goes to the scalar kernel (896 / 128 = 7 and 1152 / 128 = 9 have no DIMC: generic loop)
for dim, k, nq in ((128, 16, 3), (512, 16, 32), (640, 16, 33), (896, 12, 33), (1152, 4, 3)):
    _with_tails("bf16", dim, 2049, nq, k, {("MFMA", 0, 0), ML})
    _add("dense", "bf16", dim, 127, 32 if nq != 32 else 3, k, "grid", {("MFMA", 0, 0), ML})
    _add("dense", "bf16", dim, 4095, nq, k, "grid", {("MFMA", 0, 0), ML})
for dim, k in ((896, 13), (1152, 5)):
    _add("dense", "bf16", dim, 2049, 3, k, "grid", {("DENSE_BF16", 4, 0), ML})
    _add("dense", "bf16", dim, 2049, 32, k, "grid", {("DENSE_BF16", 4, 0), ML})
    _add("dense", "bf16", dim, 2049, 33, k, "grid", {("DENSE_BF16", 4, 0), ("DENSE_BF16", 1, 0), ML})
# fp32 queries that are not bf16 numbers ride as (value, remainder) column pairs: 16 queries per pass, 17 = two passes
_add("dense", "bf16", 128, 2049, 17, 16, "grid_pairs", {("MFMA", 0, 0), ML}, lim_x=8, lim_q=2047)

# ---------------------------------------------------------------- bf16 rows, second-generation matrix-core kernel (384, 768, 1024)
for dim, k, kt in ((384, 16, 6), (768, 16, 12), (1024, 8, 16)):
    _with_tails("bf16", dim, 2049, 33, k, {("MFMA2", kt, 0), ML})
    _add("dense", "bf16", dim, 129, 3, k, "grid", {("MFMA2", kt, 0), ML})
    _add("dense", "bf16", dim, 4095, 32, k, "grid", {("MFMA2", kt, 0), ML})

# ---------------------------------------------------------------- fp32 rows without the image, exact kernels (k <= 16)
# exact<NSLOT>: six ring slots while ceil1024(32 * (4 * dim + 16)) + 6 * 16384 <= 160 KiB (dim <= 480), else three (512 .. 736);
# exact2<KT>: 384 and 768 keep their queries in registers
for i, (dim, kern) in enumerate(((32, ("EXACT", 6, 0)), (96, ("EXACT", 6, 0)), (480, ("EXACT", 6, 0)), (512, ("EXACT", 3, 0)),
                                 (736, ("EXACT", 3, 0)), (384, ("EXACT2", 12, 0)), (768, ("EXACT2", 24, 0)))):
    _with_tails("f32", dim, 129, 5, 10, {kern, ML})
    for data in ("grid", "gauss"):
        _add("dense", "f32", dim, 2049, 1, 16, data, {kern, ML})
        _add("dense", "f32", dim, 127 if i % 2 else 4095, 33, 1, data, {kern, ML})
    _add("dense", "f32", dim, 129, 5, 10, "gauss", {kern, ML})
# the two-pass form: a prefix of 32 768 rows seeds the thresholds of the main pass from 131 072 rows on (the one large case)
LARGE = Case("dense", "f32", 512, 131072 + 129, 3, 10, "gauss", frozenset({("EXACT", 3, 0), ("SEED_THRESHOLD", 0, 0), ML}), 64, 64, "host")
CASES.append(LARGE)

# ---------------------------------------------------------------- fp32 rows, scalar kernel (k > 16): <true, QT, DIMC>
# DIMC = dim / 64 where an instantiation exists (192, 384, 512, 768; no <4, 12>), else the generic loop -- lanes differ at 24, 40, 72
# and 1000 (dim / 4 % 16 != 0); k = 65 runs as two pages of 64
for i, (dim, dc1, dc4) in enumerate(((8, 0, 0), (24, 0, 0), (40, 0, 0), (72, 0, 0), (1000, 0, 0), (1024, 0, 0), (192, 3, 3), (384, 6, 6),
                                     (512, 8, 8), (768, 12, 0))):
    _with_tails("f32", dim, 129, 1, 17, {("DENSE_F32", 1, dc1), ML})
    _with_tails("f32", dim, 129, 4, 17, {("DENSE_F32", 4, dc4), ML})
    _add("dense", "f32", dim, NS[i % 4 + 1], 5, 33, "grid", {("DENSE_F32", 4, dc4), ("DENSE_F32", 1, dc1), MS})
    _add("dense", "f32", dim, 2049, 2 if i % 2 else 1, 65, "grid", {("DENSE_F32", 4, dc4) if i % 2 else ("DENSE_F32", 1, dc1), MS})

# ---------------------------------------------------------------- fp32 rows with the bf16 image: the prefilter route (k <= 16)
PF0 = ("PF_RESCORE_LIST", 0, 0)
# one pass for two to four queries where dim % 256 == 0: collect_multi<dim / 256, 2 | 4>; one query: the single-query kernels, whose
# DIMC = dim / 128 exists for 384 and 768 only
for dim, d32, dc in ((256, 1, 0), (512, 2, 0), (768, 3, 6)):
    _with_tails("f32+image", dim, 4097, 1, 16, {("PF_PREFIX", dc, 0), ("PF_COLLECT", dc, 0), PF0})
    for data in ("grid", "gauss"):
        _add("dense", "f32+image", dim, 4224, 1, 1, data, {("PF_PREFIX", dc, 0), ("PF_COLLECT", dc, 0), PF0})
        _add("dense", "f32+image", dim, 4097, 2, 16, data, {("PF_PREFIX", dc, 0), ("PF_COLLECT_MULTI", d32, 2), PF0})
        _add("dense", "f32+image", dim, 4224, 3, 1, data, {("PF_PREFIX", dc, 0), ("PF_COLLECT_MULTI", d32, 4), PF0})
        _add("dense", "f32+image", dim, 4097, 4, 16, data, {("PF_PREFIX", dc, 0), ("PF_COLLECT_MULTI", d32, 4), PF0})
    _with_tails("f32+image", dim, 4224, 4, 16, {("PF_PREFIX", dc, 0), ("PF_COLLECT_MULTI", d32, 4), PF0})
# other widths: one or two queries, each on the single-query kernels
for dim, dc in ((96, 0), (224, 0), (384, 3), (640, 0)):
    _with_tails("f32+image", dim, 4097, 1, 16, {("PF_PREFIX", dc, 0), ("PF_COLLECT", dc, 0), PF0})
    for data in ("grid", "gauss"):
        _add("dense", "f32+image", dim, 4224, 2, 1, data, {("PF_PREFIX", dc, 0), ("PF_COLLECT", dc, 0), PF0})
# batches: the tiled search over the image (dim % 64 == 0) collects the candidates, one launch re-scores every list
for dim in (512, 640):
    for data in ("grid", "gauss"):
        _add("dense", "f32+image", dim, 4097, 5, 16, data, {("PF_RESCORE_LIST", 1, 0)})
        _add("dense", "f32+image", dim, 4224, 70, 1, data, {("PF_RESCORE_LIST", 1, 0)})
# above 256 queries: 64 candidates per query and the sufficiency test
_add("dense", "f32+image", 512, 4224, 257, 1, "gauss", {("PF_RESCORE", 0, 0)})
# no image route at this width for a batch (96 % 64 != 0): the plain fp32 search
_add("dense", "f32+image", 96, 4097, 3, 16, "grid", {("EXACT", 6, 0), ML})
# bunched scores at dim 512: the full scan behind the flags is exact<3>.  The host call of the one-pass route reads the flags and
# runs the plain scan; the batch routes and the device call run it gated, with the per-query pick behind it
_XS = {("EXACT", 3, 0), ML}
_add("dense", "f32+image", 512, 4224, 1, 16, "bunched", {("PF_PREFIX", 0, 0), ("PF_COLLECT", 0, 0), PF0} | _XS)
_add("dense", "f32+image", 512, 4224, 2, 16, "bunched", {("PF_PREFIX", 0, 0), ("PF_COLLECT_MULTI", 2, 2), PF0} | _XS)
_add("dense", "f32+image", 512, 4224, 70, 16, "bunched", {("PF_RESCORE_LIST", 1, 0), ("PF_COMBINE", 0, 0)} | _XS)
_add("dense", "f32+image", 512, 4224, 257, 16, "bunched", {("PF_RESCORE", 0, 0), ("PF_COMBINE", 0, 0)} | _XS)
_add("dense", "f32+image", 512, 4224, 1, 16, "bunched", {("PF_PREFIX", 0, 0), ("PF_COLLECT", 0, 0), PF0, ("PF_COMBINE", 0, 0)} | _XS, via="device")
_add("dense", "f32+image", 512, 4224, 4, 16, "bunched", {("PF_PREFIX", 0, 0), ("PF_COLLECT_MULTI", 2, 4), PF0, ("PF_COMBINE", 0, 0)} | _XS, via="device")
_add("dense", "f32+image", 512, 4224, 70, 16, "bunched", {("PF_RESCORE_LIST", 1, 0), ("PF_COMBINE", 0, 0)} | _XS, via="device")

# ---------------------------------------------------------------- sparse
# The corpus (tests/test_topk_instantiations_gpu.py): slices of 64 equally long documents, 4 * ng terms each, for every edge of the
# batched kernel's load sets -- ng in {0, 1, G, G + 1, 2 G, 2 G + 1}, G = 3 (16 queries per pass) and G = 5 (8) -- 64 empty
# documents among them, and a partial last slice: SPARSE_DOCS documents, no multiple of 64.
SPARSE_NG = (0, 1, 3, 4, 5, 6, 7, 10, 11)
SPARSE_TAIL_DOCS = 37            # 45 .. 60 terms each: the last, partial slice
SPARSE_DOCS = 64 * len(SPARSE_NG) + SPARSE_TAIL_DOCS
SCAT = ("SPARSE_SCATTER", 0, 0)
SPARSE_MAX_TERMS = 60            # the longest document; grid weights are integers in [1, 192] / 64 (documents) and [1, 63] / 64 (queries)


def _sparse(vocab, nq, k, data, expect):
    _add("sparse", "csr", vocab, SPARSE_DOCS, nq, k, data, expect, lim_x=192, lim_q=63)


for data in ("grid", "gauss"):
    # vocab 30 522: term map 61 056 B + table (QB + PAD) * 4 096 B + lists 128 * QB * k B against 160 KiB
    for k, kern in ((10, ("SPARSE_MULTI", 16, 4)), (11, ("SPARSE_MULTI", 16, 0)), (18, ("SPARSE_MULTI", 16, 0)), (19, ("SPARSE_MULTI", 8, 0))):
        _sparse(30522, 17, k, data, {kern, ML})       # 17 = a second, partial pass
    _sparse(30522, 8, 10, data, {("SPARSE_MULTI", 8, 0), ML})   # up to eight queries: the 8-query pass
    _sparse(30522, 17, 33, data, {("SPARSE_MULTI", 8, 0), MS})
    _sparse(30522, 1, 10, data, {("SPARSE", 1, 0), SCAT, ML})   # one query: its dense vector in LDS
    # vocab 50 368: only the 8-query pass fits, up to k = 29; beyond, the single-query kernel with the vector in HBM
    _sparse(50368, 9, 29, data, {("SPARSE_MULTI", 8, 0), ML})
    _sparse(50368, 9, 30, data, {("SPARSE", 0, 0), SCAT, ML})
    # the largest vocabularies: the term map alone leaves no room for a pass
    _sparse(65535, 2, 10, data, {("SPARSE", 0, 0), SCAT, ML})
    _sparse(65536, 2, 10, data, {("SPARSE", 0, 0), SCAT, ML})
    _sparse(65536, 1, 32, data, {("SPARSE", 0, 0), SCAT, ML})
# the union-id table holds ids 1 .. 1 023: 1 023 distinct terms fill it, one more sends the batch to the single-query kernels
_sparse(30522, 16, 10, "union1023", {("SPARSE_MULTI", 16, 4), ML})
_sparse(30522, 16, 10, "union1024", {("SPARSE", 1, 0), SCAT, ML})


def index_key(c):
    """Cases with the same key search one index: (kind, dtype, dim, n, what the rows hold)."""
    rows = c.data if c.kind == "dense" and c.data in ("tail_last", "tail_first", "gauss", "bunched") else "grid"
    if c.kind == "sparse":
        rows = "gauss" if c.data == "gauss" else "grid"
    return (c.kind, c.dtype, c.dim, c.n, rows, c.lim_x)


def case_id(c):
    return f"{c.kind}-{c.dtype}-d{c.dim}-n{c.n}-q{c.nq}-k{c.k}-{c.data}-{c.via}"
