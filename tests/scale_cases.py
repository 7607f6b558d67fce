"""Dense shards past 2^32 elements and 2^24 rows whose top-k is known WITHOUT scanning them on the host: the generator, the case
table and the host-side reference of tests/test_scale_gpu.py (tests/test_scale_host.py checks all three on a few hundred rows with
"virtual" boundaries).

Grid units: every stored value and every query value is a small integer / 64 (the `grid` convention of
tests/topk_instantiation_cases.py), a bf16 number; dim * max|x| * max|q| <= 2^24 in grid units (check_params), so every partial sum
of a dot product is an integer below 2^24, exact in fp32 in any summation order: every route must return the oracle's bits.

Background row r, column c:  x = ((r % 65521) * 40503 + r // 65521 * 30011 + c * 7919 + (r % 8191) * (c % 127 + 1)) % 65537 % 9 - 4,
int64 arithmetic on non-negative numbers, the same in numpy and in torch on any device (background); |x| <= BG = 4.

Classes: NC = 4 classes own the column blocks [j * dim / 4, (j + 1) * dim / 4).  Query i belongs to class i % 4 and is non-zero on its
block only, q[c] = sign(c) * m with QL / 2 <= m <= QL = 64.  A planted row of class j, level P, holds sign(c) * P on block j
(sign(c) * (P + 1) on up to four "varied" columns chosen by its variant) and background elsewhere, FLOOR = 2 BG + 1 <= P, P + 1 <= 64.
For a query of class j therefore (block = dim / 4)
    a background row, or a planted row of another class, scores at most   block * BG * QL        = 256 block
    a planted row of class j scores at least                              block * FLOOR * QL / 2 = 288 block
(check_params asserts it from these constants, not from data): the top-k of a query, for k up to the planted rows of its class, is
oracle/topk_ref over the planted rows ALONE, ids mapped back (expected).

Where rows are planted (make_plan), every row once, in this order of precedence:
  edge    per boundary (an element offset E -> the row E // dim that contains it; or a row number): rows b - 2 and b hold one spec,
          b - 1 and b + 1 another (equal scores on opposite sides of the boundary: (score desc, id asc) has to carry across it), b + 2 a
          third, and one row in each adjacent 256-row tile; then the first row of the last partial tile and row n - 1.  Levels run down
          from 63, five per boundary, so no two edge rows of different boundaries share (class, level).
  floor   kmax rows per class at FLOOR in the first 256-row tile, the classes interleaved: that tile is in every prefix and in the tiled
          search's sample, so every entry threshold lies above the background and no route overflows into its fallback.
  anchor  (shards with a prefilter image) one FLOOR row per class at the start of each of the 256 strides of (n / 256 / 128) * 128 rows:
          the one-pass prefilter ranks 128-row blocks at that stride and keeps two keys of each, so the first tile alone gives it two.
  stride  ~n_stride rows at a prime stride, levels 10 .. 40.
Alias rule: for an edge row r and every wrap w (2^30, 2^31, 2^32 elements where that is a whole number of rows), the rows r - w and
r + w inside the shard are background, a FLOOR row or an edge row of another (class, level) -- never a stride or anchor row: a wrapped
offset reads a row that scores differently for r's class, so it loses the hit or reports it at a wrong score, and array equality breaks.
Rows 3 .. 255 + 2^32 / dim behind the floor rows are background likewise (family A).

SQ8 (family B, both routes): scores are quantised, so the inequality is restated for the codes (check_sq8_params) and the expected
lists are tests/sq8_ref.py over the planted rows alone.

Out of scope: sparse and full-text indexes (their 2^31 lines are in nnz and in postings; building them on the host dominates any
test)."""
from collections import namedtuple

import numpy as np

NC = 4                       # classes
BG = 4                       # |background| <= BG
QL = 64                      # QL / 2 <= |q| <= QL on the query's block
FLOOR = 2 * BG + 1           # lowest planted level
STRIDE_LO, STRIDE_LEVELS = FLOOR + 1, 31   # stride levels 10 .. 40
EDGE_HI = 63                 # highest planted level (+ 1 on a varied column: 64)
VAR_COLS = 4
HOST_TAIL = 4353             # rows that go in through the host add: 17 tiles and one row
FILTER_BLOCK = 32768         # rows per workgroup of the filtered search's bitmap compaction (1 024 words)

Plan = namedtuple("Plan", "dim n tile bounds wraps ids spec kind")


def check_params(dim):
    """The two facts everything rests on, from the constants alone."""
    block = dim // NC
    assert dim % NC == 0 and block >= VAR_COLS
    assert dim * (EDGE_HI + 1) * QL <= 1 << 24, "a partial sum could leave the integers fp32 holds exactly"
    assert EDGE_HI + 1 <= 256 and QL <= 256, "every value must be a bf16 number"
    assert STRIDE_LO + STRIDE_LEVELS - 1 + 1 < EDGE_HI - 5 * 4, "edge rows must outrank every stride row"
    worst_other = block * BG * QL
    least_own = block * FLOOR * (QL // 2)
    assert least_own > worst_other
    return worst_other, least_own


def check_sq8_params(dim):
    """The same two facts for the SQ8 index (include/vrag_amd.h: code = rint(x / s), s = max|x| / 127 per vector, score =
    idot * (s_q * s_r)), in grid units, from the constants alone.  A code times its scale is within s / 2 of the value and at most
    max|x| in size, and s * 64 <= (EDGE_HI + 1) / 127 for every row and QL / 127 for every query.  Per column of the query's block:
      any row's background value, dequantised:  at most BG + (EDGE_HI + 1) / 254  (a background row: at most BG, its own maximum)
      a planted value of the query's class:     at least FLOOR - (EDGE_HI + 1) / 254, of the query's sign
      the query's value:                        between QL / 2 - QL / 254 and QL
    The three fp32 roundings of a score move it by less than 2^-21 of itself: `slack`."""
    block, half = dim // NC, (EDGE_HI + 1) / 254.0
    worst_other = block * (BG + half) * QL
    least_own = block * (FLOOR - half) * (QL / 2 - QL / 254.0)
    slack = 1.0 + 2.0 ** -20
    assert least_own > worst_other * slack * slack
    return worst_other, least_own


def background(rows, dim):
    """int64 [m, dim] background values of the rows (a numpy int64 array or a torch int64 tensor on any device)."""
    if isinstance(rows, np.ndarray):
        r = rows.astype(np.int64)[:, None]
        c = np.arange(dim, dtype=np.int64)[None, :]
    else:
        import torch

        r = rows.to(torch.int64)[:, None]
        c = torch.arange(dim, dtype=torch.int64, device=rows.device)[None, :]
    h = (r % 8191) * (c % 127 + 1)
    h += (r % 65521) * 40503 + (r // 65521) * 30011
    h += c * 7919
    h %= 65537
    h %= 2 * BG + 1
    h -= BG
    return h


def class_sign(dim):
    c = np.arange(dim, dtype=np.int64)
    return np.where(((c * 2654435761) >> 7) & 1, 1, -1).astype(np.int64)


def queries(dim, nq):
    """fp32 [nq, dim]: query i is non-zero on the block of class i % NC only."""
    block, sign = dim // NC, class_sign(dim)
    Q = np.zeros((nq, dim), np.int64)
    for i in range(nq):
        c = np.arange(i % NC * block, (i % NC + 1) * block, dtype=np.int64)
        mag = QL // 2 + (i * 7919 + c * 104729 + (i + 1) * (c % 61)) % 65537 % (QL // 2 + 1)
        Q[i, c] = sign[c] * mag
    assert (np.abs(Q).max(axis=1) <= QL).all() and (np.abs(Q)[Q != 0] >= QL // 2).all()
    return (Q / 64.0).astype(np.float32)


def _next_prime(v):
    v = max(v, 2)
    while any(v % p == 0 for p in range(2, int(v ** 0.5) + 1)):
        v += 1
    return v


def make_plan(dim, n, elem_bounds=(), row_bounds=(), wraps_elems=(1 << 30, 1 << 31, 1 << 32), kmax=64, anchors=False, n_stride=1000,
              tile=256):
    """Which rows are planted, and with what: ids ascending, spec[i] = (class, level, variant), kind[i] in edge / floor / anchor / stride."""
    check_params(dim)
    bounds = sorted({e // dim for e in elem_bounds if e < n * dim} | {r for r in row_bounds if r < n})
    wraps = [w // dim for w in wraps_elems if w % dim == 0]
    spec, kind = {}, {}

    def put(r, s, what):
        assert 0 <= r < n and r not in spec, (r, what)
        spec[r], kind[r] = s, what

    level = EDGE_HI
    for bi, b in enumerate(bounds):
        ca, cb, cc, cd = [(bi + t) % NC for t in range(4)]
        lo_tile, hi_tile = (b // tile - 1) * tile + 7, (b // tile + 1) * tile + 7
        assert b - 2 >= 0 and lo_tile >= 0 and hi_tile < n and b + 2 < n, "a boundary too close to the shard's ends"
        put(b - 2, (ca, level, 5), "edge")
        put(b, (ca, level, 5), "edge")
        put(b - 1, (cb, level - 1, 10), "edge")
        put(b + 1, (cb, level - 1, 10), "edge")
        put(b + 2, (cc, level - 2, 3), "edge")
        put(lo_tile, (cd, level - 3, 6), "edge")
        put(hi_tile, (ca, level - 4, 9), "edge")
        level -= 5
    last_tile = (n - 1) // tile * tile
    put(last_tile, (len(bounds) % NC, level, 12), "edge")
    if n - 1 != last_tile:
        put(n - 1, ((len(bounds) + 1) % NC, level - 1, 7), "edge")
    assert level - 1 > STRIDE_LO + STRIDE_LEVELS, "too many boundaries for the levels above the stride rows"
    edges = sorted(spec)
    reserved = {r + s * w for r in edges for w in wraps for s in (-1, 1) if 0 <= r + s * w < n}
    reserved |= {r + w for r in range(3, tile) for w in wraps[-1:] if r + w < n}   # a few low planted rows: background behind them too
    for i in range(NC * kmax):
        if i not in spec:
            put(i, (i % NC, FLOOR, i // NC % 16), "floor")
    assert NC * kmax <= tile, "the floor rows must fit the first tile"
    if anchors:
        a_stride = n // 256 // 128 * 128
        assert a_stride >= tile
        for b in range(1, 256):
            for t in range(NC):
                r = b * a_stride + t
                if r < n and r not in spec and r not in reserved:
                    put(r, (t, FLOOR, 0), "anchor")
    step = _next_prime(max(2, n // max(n_stride, 1)))
    for i, r in enumerate(range(NC * kmax + 44, n, step)):
        if r not in spec and r not in reserved:
            put(r, (i % NC, STRIDE_LO + i * 7 % STRIDE_LEVELS, i % 16), "stride")
    ids = np.array(sorted(spec), np.int64)
    return Plan(dim, n, tile, bounds, wraps, ids, [spec[int(r)] for r in ids], [kind[int(r)] for r in ids])


def edge_rows(plan):
    return np.array([r for r, what in zip(plan.ids, plan.kind) if what == "edge"], np.int64)


_VALUES = {}


def planted_values(plan, lo=0, hi=None):
    """(ids, int64 [m, dim] grid values) of the planted rows in [lo, hi)."""
    if lo == 0 and hi is None:
        if id(plan.ids) not in _VALUES:
            _VALUES[id(plan.ids)] = (plan.ids, planted_values(plan, 0, plan.n)[1].astype(np.int8))
        return plan.ids, _VALUES[id(plan.ids)][1].astype(np.int64)
    hi = plan.n if hi is None else hi
    a, b = np.searchsorted(plan.ids, [lo, hi])
    ids = plan.ids[a:b]
    V = background(ids, plan.dim)
    block, sign = plan.dim // NC, class_sign(plan.dim)
    for i, (cls, level, var) in enumerate(plan.spec[a:b]):
        c0 = cls * block
        V[i, c0:c0 + block] = sign[c0:c0 + block] * level
        for t in range(VAR_COLS):
            if var >> t & 1:
                V[i, c0 + t] = sign[c0 + t] * (level + 1)
    return ids, V


def rows_numpy(plan, rows):
    """fp32 [m, dim]: what the shard stores in the given rows (any rows, ascending or not)."""
    rows = np.asarray(rows, np.int64)
    V = background(rows, plan.dim)
    pos = np.searchsorted(plan.ids, rows)
    hit = (pos < len(plan.ids)) & (plan.ids[np.minimum(pos, len(plan.ids) - 1)] == rows)
    if hit.any():
        _ids, P = planted_values(plan)
        V[hit] = P[pos[hit]]
    return (V / 64.0).astype(np.float32)


def chunk_torch(plan, r0, r1, device):
    """fp32 [r1 - r0, dim] torch tensor on `device`: the background in torch integer ops, the chunk's planted rows scattered into it."""
    import torch

    X = background(torch.arange(r0, r1, dtype=torch.int64, device=device), plan.dim).to(torch.float32)
    X /= 64.0
    ids, V = planted_values(plan, r0, r1)
    if len(ids):
        X.index_copy_(0, torch.from_numpy(ids - r0).to(device), torch.from_numpy((V / 64.0).astype(np.float32)).to(device))
    return X


def expected(plan, Q, k, allowed=None):
    """(scores, ids) of the top-k by the planted-rows argument: oracle/topk_ref over the planted rows (those with allowed(ids) true
    when a filter is given), ids mapped back.  Asserts the argument's condition: every query finds k planted rows of its own class
    -- or the filter lets nothing but planted rows through (`only_planted`), where -1 / -inf tails are the answer."""
    from oracle import topk_ref as O

    ids, V = planted_values(plan)
    cls = np.array([s[0] for s in plan.spec])
    only_planted = False
    if allowed is not None:
        keep, only_planted = allowed(ids)
        ids, V, cls = ids[keep], V[keep], cls[keep]
    X = (V / 64.0).astype(np.float32)
    assert np.array_equal(O.bf16_round(X), X)
    if not only_planted:
        for j in range(min(NC, len(Q))):
            assert (cls == j).sum() >= k, f"class {j} has {(cls == j).sum()} planted rows for k = {k}: the planted-rows argument needs k"
    if len(ids) == 0:
        return np.full((len(Q), k), -np.inf, np.float32), np.full((len(Q), k), -1, np.int64)
    rs, ri = O.dense_topk(X, Q, k)
    return rs, np.where(ri >= 0, ids[np.maximum(ri, 0)], -1)


def expected_sq8(plan, Q, k, allowed=None):
    """expected() for the SQ8 index: tests/sq8_ref.py (quantise both sides, integer dots, the three roundings) over the planted rows."""
    import sq8_ref as R

    check_sq8_params(plan.dim)
    ids, V = planted_values(plan)
    cls = np.array([s[0] for s in plan.spec])
    if allowed is not None:
        keep = allowed(ids)[0]
        ids, V, cls = ids[keep], V[keep], cls[keep]
    assert min((cls == j).sum() for j in range(NC)) >= k, "the planted-rows argument needs k planted rows of every class"
    rs, ri = R.search((V / 64.0).astype(np.float32), Q, k)
    return rs, np.where(ri >= 0, ids[np.maximum(ri, 0)], -1)


def expected_over(plan, rows, Q, k):
    """The oracle over an explicit, ascending list of rows (a filter small enough to scan on the host)."""
    from oracle import topk_ref as O

    rows = np.asarray(rows, np.int64)
    rs, ri = O.dense_topk(rows_numpy(plan, rows), Q, k)
    return rs, np.where(ri >= 0, rows[np.maximum(ri, 0)], -1)


def check_plan(plan, ks):
    """The edge-set, tie, alias and k conditions of a plan, for every k of `ks` (the host asserts them before any search)."""
    spec = {int(r): s for r, s in zip(plan.ids, plan.spec)}
    kind = {int(r): s for r, s in zip(plan.ids, plan.kind)}
    edges = {int(r) for r in edge_rows(plan)}
    for b in plan.bounds:
        want = {b - 2, b - 1, b, b + 1, b + 2, (b // plan.tile - 1) * plan.tile + 7, (b // plan.tile + 1) * plan.tile + 7}
        assert want <= edges, f"boundary row {b}: edge rows {sorted(want - edges)} are missing"
        assert spec[b - 1] == spec[b + 1] and spec[b - 2] == spec[b], f"boundary row {b}: no equal pair across it"
    assert {(plan.n - 1) // plan.tile * plan.tile, plan.n - 1} <= edges
    for r in edges:
        for w in plan.wraps:
            for a in (r - w, r + w):
                if 0 <= a < plan.n and a in spec:
                    assert kind[a] in ("edge", "floor") and spec[a][:2] != spec[r][:2], f"edge row {r} aliases planted row {a}"
    if plan.wraps and plan.wraps[-1] < plan.n:
        behind = [r + plan.wraps[-1] for r in range(3, plan.tile) if r in spec and r + plan.wraps[-1] < plan.n]
        assert behind and sum(a in spec for a in behind) <= 2, "the rows 2^32 elements behind the floor rows must be background"
    per_class = [sum(1 for r in edges if spec[r][0] == j) for j in range(NC)]
    Q = queries(plan.dim, 2 * NC)
    for k in ks:
        assert max(per_class) <= k, f"k = {k} cannot hold the {max(per_class)} edge rows of a class"
        _rs, ri = expected(plan, Q, k)
        for i in range(len(Q)):
            own = {r for r in edges if spec[r][0] == i % NC}
            assert own <= set(ri[i].tolist()), f"k = {k}, query {i}: edge rows {sorted(own - set(ri[i].tolist()))} are not in its top-k"


# ------------------------------------------------------------------------------------------------ the shapes
def _rows_past(elems, dim):
    """The least multiple of 256 rows that holds `elems` elements."""
    return (-(-elems // dim) + 255) // 256 * 256


Family = namedtuple("Family", "name dim n elem_bounds row_bounds anchors claims")
FAMILIES = {
    # claims: (what, predicate(rows ingested from the device)) -- true at n - HOST_TAIL, false 256 rows earlier (test_scale_host)
    "A": Family("A", 4096, _rows_past(1 << 32, 4096) + HOST_TAIL, (1 << 30, 1 << 31, 1 << 32), (), False,
                [("2^32 elements", lambda m: m * 4096 >= 1 << 32)]),
    "B": Family("B", 768, _rows_past(1 << 32, 768) + HOST_TAIL, (1 << 30, 1 << 31, 1 << 32), (), True,
                [("2^32 elements", lambda m: m * 768 >= 1 << 32)]),
    "C": Family("C", 64, (1 << 24) + HOST_TAIL, (1 << 30,), (1 << 24, 1 << 23), True,
                [("row id 2^24", lambda m: m >= 1 << 24)]),   # and, not minimal, 513 compaction blocks: three rounds of filter_scan_kernel
}
assert FAMILIES["A"].n == 1_052_929 and FAMILIES["B"].n == 5_596_929 and FAMILIES["C"].n == 16_781_569

_PLANS = {}


def family_plan(name):
    if name not in _PLANS:
        f = FAMILIES[name]
        _PLANS[name] = make_plan(f.dim, f.n, f.elem_bounds, f.row_bounds, anchors=f.anchors)
    return _PLANS[name]


def shard_bytes(dim, n, dtype):
    """HBM of the index's row buffers (the library pads by two tiles) plus one 2^28-element ingest chunk and its integer form."""
    rows = (n + 512) * dim
    if dtype == "sq8":
        return rows + 4 * n + (1 << 28) * (4 + 8 + 8)   # int8 codes and one fp32 scale per row
    return rows * {"bf16": 2, "f32": 4, "f32+image": 6}[dtype] + (1 << 28) * (4 + 8 + 8)


# api     "host" = vrag_dense_index_search, "base" / "map" = vrag_dense_index_search_device with id_base = 2^33 / a row_map,
#         "filtered" = vrag_dense_index_search_filtered with the bitmap `arg`, "ivf" = the IVF overlay with nprobe = nlist against the
#         filtered search under an all-ones bitmap
# expect  the launch log's (id, p0, p1) set: all of it, nothing else.  The tiled search logs nothing (its kernels are not logged): an
#         empty set says that no pass kernel answered a flagged query; a prefilter route without EXACT* / PF_COMBINE says that no
#         full scan did.  The filtered searches and the IVF overlay log their merge only.
Case = namedtuple("Case", "family dtype api nq k expect arg")
ML, SEED = ("MERGE_LISTS", 0, 0), ("SEED_THRESHOLD", 0, 0)
PF0, PF1 = ("PF_RESCORE_LIST", 0, 0), ("PF_RESCORE_LIST", 1, 0)
ID_BASE = 1 << 33
CASES, NO_TILED_CASES = [], []


def _add(family, dtype, api, nq, k, expect, arg=None, to=CASES):
    to.append(Case(family, dtype, api, nq, k, None if expect is None else frozenset(expect), arg))


# family A, dim 4096: the generic loops of the scalar kernels, the tiled search in its three tile forms
_add("A", "bf16", "host", 1, 10, {("DENSE_BF16", 1, 0), ML})
for _nq, _k in ((2, 10), (33, 64), (70, 10), (70, 64)):
    _add("A", "bf16", "host", _nq, _k, ())
_add("A", "bf16", "base", 33, 10, ())
_add("A", "bf16", "map", 1, 10, {("DENSE_BF16", 1, 0), ML})
_add("A", "bf16", "filtered", 3, 10, {ML}, "all")
_add("A", "f32", "host", 1, 17, {("DENSE_F32", 1, 0), ML})
_add("A", "f32", "host", 5, 17, {("DENSE_F32", 4, 0), ("DENSE_F32", 1, 0), ML})
_add("A", "f32", "filtered", 3, 10, {ML}, "all")
# family B, dim 768: the width with the most instantiations
_add("B", "bf16", "host", 1, 10, {("DENSE_BF16", 1, 6), ML})
_add("B", "bf16", "host", 2, 10, ())
_add("B", "bf16", "host", 70, 64, ())
_add("B", "bf16", "base", 33, 16, ())
_add("B", "bf16", "filtered", 3, 10, {ML}, "all")
_add("B", "f32", "host", 3, 10, {("EXACT2", 24, 0), SEED, ML})
_add("B", "f32", "host", 33, 16, {("EXACT2", 24, 0), SEED, ML})
_add("B", "f32", "host", 1, 17, {("DENSE_F32", 1, 12), ML})
_add("B", "f32", "host", 4, 17, {("DENSE_F32", 4, 0), ML})
_add("B", "f32", "map", 3, 10, {("EXACT2", 24, 0), SEED, ML})
_add("B", "f32", "filtered", 3, 10, {ML}, "all")
_add("B", "f32+image", "host", 1, 16, {("PF_PREFIX", 6, 0), ("PF_COLLECT", 6, 0), PF0})
_add("B", "f32+image", "host", 4, 10, {("PF_PREFIX", 6, 0), ("PF_COLLECT_MULTI", 3, 4), PF0})
_add("B", "f32+image", "host", 5, 16, {PF1})
_add("B", "f32+image", "host", 70, 10, {PF1})
_add("B", "f32+image", "host", 257, 10, {("PF_RESCORE", 0, 0)})
_add("B", "f32+image", "filtered", 3, 10, {ML}, "all")
_add("B", "f32+image", "ivf", 3, 10, {ML}, 4)
# SQ8 rows of family B (api "sq8" / "sq8_filtered", arg = the route: 0 automatic, 1 scan kernel, 2 tile kernel; no launch log: None)
_add("B", "sq8", "sq8", 1, 10, None, 0)
_add("B", "sq8", "sq8", 3, 10, None, 1)
_add("B", "sq8", "sq8", 3, 10, None, 2)
_add("B", "sq8", "sq8", 70, 64, None, 2)
_add("B", "sq8", "sq8_filtered", 3, 10, None, 1)
_add("B", "sq8", "sq8_filtered", 5, 16, None, 2)
# family C, dim 64: row ids at and above 2^24, 513 compaction blocks
_add("C", "bf16", "host", 1, 10, {("DENSE_BF16", 1, 0), ML})
_add("C", "bf16", "host", 2, 10, ())
_add("C", "bf16", "host", 70, 64, ())
_add("C", "bf16", "base", 33, 10, ())
_add("C", "bf16", "map", 2, 16, ())
for _arg in ("all", "high_blocks", "straddle_255_256", "last_row"):
    _add("C", "bf16", "filtered", 3, 10, {ML}, _arg)
_add("C", "f32", "host", 3, 10, {("EXACT", 6, 0), SEED, ML})
_add("C", "f32", "host", 33, 16, {("EXACT", 6, 0), SEED, ML})
for _arg in ("all", "high_blocks", "straddle_255_256", "last_row"):
    _add("C", "f32", "filtered", 3, 10, {ML}, _arg)
_add("C", "f32", "ivf", 3, 10, {ML}, 8)
_add("C", "f32+image", "host", 1, 16, {("PF_PREFIX", 0, 0), ("PF_COLLECT", 0, 0), PF0})
_add("C", "f32+image", "host", 5, 10, {PF1})
_add("C", "f32+image", "host", 257, 10, {("PF_RESCORE", 0, 0)})
_add("C", "f32+image", "filtered", 3, 10, {ML}, "all")

# The pass kernels behind the tiled search, over the bf16 rows of family B: dense_topk_mfma2_kernel<12> (its two-pass form) and the
# four-queries scalar kernel run there only without the tiled search -- tests/test_scale_gpu.py runs these in a child process.
_add("B", "bf16", "host", 33, 10, {("MFMA2", 12, 0), SEED, ML}, to=NO_TILED_CASES)
_add("B", "bf16", "host", 3, 16, {("MFMA2", 12, 0), SEED, ML}, to=NO_TILED_CASES)
_add("B", "bf16", "host", 5, 17, {("DENSE_BF16", 4, 6), ("DENSE_BF16", 1, 6), ML}, to=NO_TILED_CASES)
_add("B", "bf16", "host", 2, 10, {("DENSE_BF16", 4, 6), ML}, to=NO_TILED_CASES)

KS = sorted({c.k for c in CASES + NO_TILED_CASES})


def shard_order(cases):
    """[(family, dtype)] in the order the shards are built: one at a time."""
    seen = []
    for c in cases:
        if (c.family, c.dtype) not in seen:
            seen.append((c.family, c.dtype))
    return seen


def case_id(c):
    return f"{c.family}-{c.dtype}-{c.api}{'' if c.arg is None else '-' + str(c.arg)}-q{c.nq}-k{c.k}"


def filter_rows(plan, name):
    """A bitmap of the table as (lo, hi): the rows [lo, hi) pass."""
    edge = 256 * FILTER_BLOCK
    return {"all": (0, plan.n), "upper_half": (plan.n // 2, plan.n), "high_blocks": (edge, plan.n), "straddle_255_256": (edge - 40_000, edge + 40_000),
            "last_row": (plan.n - 1, plan.n)}[name]
