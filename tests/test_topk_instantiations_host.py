"""The table of tests/topk_instantiation_cases.py checked without a GPU: its expected sets cover every instantiation csrc/topk.hip
compiles for the logged kernels, its grid data is exact in fp32, and the admission arithmetic of the selection code, recomputed here
from the constants in the source, agrees with the kernels the table expects at every edge it quotes."""
import os
import re

import topk_instantiation_cases as T
from verbatim_rag_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "verbatim-rag_amd", "csrc", "topk.hip")).read()
KERNELS_H = open(os.path.join(ROOT, "verbatim-rag_amd", "csrc", "topk_kernels.h")).read()
LDS = 160 * 1024


def _const(name, text=SRC):
    m = re.search(r"constexpr (?:int|long long) " + name + r" = (\d+);", text)
    assert m, f"constexpr {name} not found"
    return int(m.group(1))


MQ, MSLOTS, MKMAX, XQ, XKL, SUW, MERGE_KMAX, PFQ = (_const(n) for n in ("MQ", "MSLOTS", "MKMAX", "XQ", "XKL", "SUW", "MERGE_KMAX", "PFQ"))
KMAX = _const("KMAX", KERNELS_H)


def _ids(c):
    return {e[0] for e in c.expect}


# ------------------------------------------------------------------ coverage
def test_expected_sets_are_instantiations():
    assert len(T.CASES) == len(set(T.CASES)), "a case is listed twice"
    for c in T.CASES:
        assert c.expect and c.expect <= T.ALL, T.case_id(c)
        assert c.kind in ("dense", "sparse") and c.via in ("host", "device")


def test_every_instantiation_has_a_case():
    """union of the expected sets == ALL - UNREACHABLE, and UNREACHABLE holds only what a predicate quoted from the source excludes."""
    covered = frozenset().union(*(c.expect for c in T.CASES))
    assert set(T.UNREACHABLE) <= T.ALL
    for entry, predicate in T.UNREACHABLE.items():
        assert predicate and predicate in SRC, f"{entry}: the predicate is not a quotation of csrc/topk.hip"
    missing = T.ALL - set(T.UNREACHABLE) - covered
    assert not missing, f"no case launches {sorted(missing)}"
    assert not covered & set(T.UNREACHABLE), "a case expects an instantiation listed as unreachable"


def test_all_is_what_the_source_instantiates():
    """ALL against the launch sites of csrc/topk.hip: the ids are the header's enum, every note in the source names one of them, and
    the template parameters the selection code can pass are the ones ALL lists."""
    ids = set(_lib.DEBUG_TOPK_LAUNCH_IDS)
    assert {e[0] for e in T.ALL} == ids
    noted = set(re.findall(r"VRAG_LAUNCH_NOTE\((\w+),", SRC)) - {"id"}
    assert noted == ids
    dense = {(int(q), int(d)) for q, d in re.findall(r"VRAG_DENSE_CASE\((\d+), (\d+)\);", SRC)}
    for name in ("DENSE_BF16", "DENSE_F32"):
        assert {(e[1], e[2]) for e in T.ALL if e[0] == name} == dense
    body = SRC[SRC.index("void with_pf_dimc("):]
    body = body[:body.index("\n}\n")]
    pf = {int(v) for v in re.findall(r"f\(IntC<(\d+)>\{\}\)", body)}
    for name in ("PF_PREFIX", "PF_COLLECT"):
        assert {e[1] for e in T.ALL if e[0] == name} == pf
    assert {(e[1], e[2]) for e in T.ALL if e[0] == "PF_COLLECT_MULTI"} == {
        (int(d), q) for d in re.findall(r"case (\d): go\(IntC<\1>\{\}\)", SRC) for q in (2, 4)}
    assert {(e[1], e[2]) for e in T.ALL if e[0] == "SPARSE_MULTI"} == {
        (int(q), int(p)) for q, p in re.findall(r"go\(&sparse_topk_multi_kernel<(\d+), 16, (\d+)>\)", SRC)}
    assert {e[1] for e in T.ALL if e[0] == "MFMA2"} == {int(v) for v in re.findall(r"hipLaunchKernelGGL\(dense_topk_mfma2_kernel<(\d+)>", SRC)}
    assert {e[1] for e in T.ALL if e[0] == "EXACT"} == {int(v) for v in re.findall(r"hipLaunchKernelGGL\(dense_topk_exact_kernel<(\d+)>", SRC)}
    assert {e[1] for e in T.ALL if e[0] == "EXACT2"} == {int(v) for v in re.findall(r"hipLaunchKernelGGL\(dense_topk_exact2_kernel<(\d+)>", SRC)}


def test_the_dead_prefilter_instantiation_is_gone():
    """prefilter_route_ok admits the route only where dense_use_exact holds (dim <= 768): with_pf_dimc has no case for 1024."""
    assert "if (!dense_use_exact(1, ix->dim, k)) return false;" in SRC
    assert re.search(r"return !off && dtype == 1 && dim % 32 == 0 && dim <= 768 && k <= XKL;", SRC)
    assert not re.search(r"case 8: f\(IntC<8>", SRC)


# ------------------------------------------------------------------ data
def test_grid_data_is_exact_in_fp32():
    for c in T.CASES:
        if c.data in ("gauss",):
            continue
        terms = T.SPARSE_MAX_TERMS if c.kind == "sparse" else c.dim
        assert terms * c.lim_x * c.lim_q <= 2 ** 24, T.case_id(c)
        if c.data == "grid_pairs":
            assert c.lim_q > 256, "queries of at most 8 bits are bf16 numbers"


def test_gauss_data_only_where_the_contract_is_the_sequential_chain():
    chain = {"EXACT", "EXACT2", "SEED_THRESHOLD", "PF_PREFIX", "PF_COLLECT", "PF_COLLECT_MULTI", "PF_RESCORE_LIST", "PF_RESCORE", "PF_COMBINE",
             "SPARSE", "SPARSE_SCATTER", "SPARSE_MULTI", "MERGE_LISTS", "MERGE_SCAN"}
    for c in T.CASES:
        if c.data == "gauss":
            assert _ids(c) <= chain, T.case_id(c)


def test_every_dense_width_has_both_tail_cases():
    widths = {(c.dtype, c.dim) for c in T.CASES if c.kind == "dense"}
    for data in ("tail_last", "tail_first"):
        assert {(c.dtype, c.dim) for c in T.CASES if c.data == data} == widths, data


def test_shapes_keep_the_routes_out_of_scope_out():
    for c in T.CASES:
        if c.kind == "dense" and c.dtype == "bf16":   # dense_use_tiled
            assert c.nq == 1 or c.n < 4096 or c.dim % 64 != 0, T.case_id(c)
        if c.kind == "dense":
            assert c.dim % 8 == 0 and 0 < c.dim <= 4096 and 1 <= c.k <= 1024
        if c.dtype == "f32+image":
            assert c.n in (4097, 4224) and c.k in (1, 16), T.case_id(c)
    assert sum(c.n > 5000 for c in T.CASES) == 1 and T.LARGE.n == 131072 + 129


# ------------------------------------------------------------------ admission arithmetic
def mfma_admits(dim, nq, k):
    return dim % 128 == 0 and nq >= 3 and k <= MKMAX and MQ * dim * 2 + MSLOTS * 16384 + 256 * k * 8 <= LDS


def test_first_generation_mfma_admission_edges():
    def last_k(dim):
        return max([k for k in range(1, MKMAX + 1) if mfma_admits(dim, 3, k)], default=0)

    assert [last_k(d) for d in (128, 512, 640, 768)] == [16] * 4
    assert (last_k(896), last_k(1024), last_k(1152), last_k(1280)) == (12, 8, 4, 0)
    seen = set()
    for c in T.CASES:
        if c.kind == "dense" and c.dtype == "bf16" and c.k <= KMAX:
            admitted = mfma_admits(c.dim, c.nq, c.k)
            assert admitted == bool(_ids(c) & {"MFMA", "MFMA2"}), T.case_id(c)
            assert ("MFMA2" in _ids(c)) == (admitted and c.dim in (384, 768, 1024)), T.case_id(c)
            if c.nq >= 3:
                seen.add((c.dim, c.k, admitted))
    # the last admitted k and the first refused one
    assert {(896, 12, True), (896, 13, False), (1152, 4, True), (1152, 5, False), (1024, 8, True), (1024, 9, False)} <= seen


def test_exact_kernel_ring_depth():
    def nslot(dim):
        qbytes = (XQ * (dim * 4 + 16) + 1023) // 1024 * 1024
        return 6 if qbytes + 6 * 16384 <= LDS else 3

    assert [d for d in range(32, 769, 32) if nslot(d) == 3] == list(range(512, 769, 32))
    for c in T.CASES:
        if c.kind == "dense" and c.dtype == "f32" and c.k <= XKL:
            want = ("EXACT2", 24 if c.dim == 768 else 12, 0) if c.dim in (384, 768) else ("EXACT", nslot(c.dim), 0)
            assert c.dim % 32 == 0 and c.dim <= 768 and want in c.expect, T.case_id(c)
        if c.kind == "dense" and c.dtype == "f32" and c.k > XKL:
            assert _ids(c) <= {"DENSE_F32", "MERGE_LISTS", "MERGE_SCAN"}, T.case_id(c)
    dims3 = {c.dim for c in T.CASES if ("EXACT", 3, 0) in c.expect}
    assert {512, 736} <= dims3


def sparse_lds(vocab, qb, k, pad):
    return ((vocab + 7) & ~7) * 2 + (qb + pad) * SUW * 4 + 16 * qb * k * 8


def sparse_kernel(vocab, nq, k):
    qb = 8 if nq <= 8 else (16 if sparse_lds(vocab, 16, k, 0) <= LDS else 8)
    if nq >= 2 and vocab <= 65535 and sparse_lds(vocab, qb, k, 0) <= LDS:
        return ("SPARSE_MULTI", qb, 4 if qb == 16 and sparse_lds(vocab, 16, k, 4) <= LDS else 0)
    return ("SPARSE", 1 if vocab * 4 + 16 * k * 8 <= LDS else 0, 0)


def test_sparse_pass_shape_edges():
    assert [sparse_kernel(30522, 17, k)[1:] for k in (10, 11, 18, 19)] == [(16, 4), (16, 0), (16, 0), (8, 0)]
    assert LDS - sparse_lds(30522, 16, 10, 4) == 384          # what the padded 16-query layout has to spare at k = 10
    assert sparse_kernel(50368, 9, 29) == ("SPARSE_MULTI", 8, 0) and sparse_kernel(50368, 9, 30) == ("SPARSE", 0, 0)
    assert SUW == 1024                                         # union ids 1 .. 1 023
    for c in T.CASES:
        if c.kind != "sparse":
            continue
        assert c.n % 64 != 0 and c.k <= KMAX
        want = ("SPARSE", 1, 0) if c.data == "union1024" else sparse_kernel(c.dim, c.nq, c.k)
        assert want in c.expect, T.case_id(c)
        assert (("SPARSE_SCATTER", 0, 0) in c.expect) == (want[0] == "SPARSE"), T.case_id(c)
    ng = set(T.SPARSE_NG)
    for g in (3, 5):                                           # G of the 16- and the 8-query pass
        assert {0, 1, g, g + 1, 2 * g, 2 * g + 1} <= ng


def test_merge_kernel_by_list_length():
    ks = set()
    for c in T.CASES:
        merges = _ids(c) & {"MERGE_LISTS", "MERGE_SCAN"}
        if merges:
            k = min(c.k, KMAX)                                 # k > KMAX: pages of KMAX
            assert merges == ({"MERGE_LISTS"} if k <= MERGE_KMAX else {"MERGE_SCAN"}), T.case_id(c)
            ks.add(c.k)
    assert {32, 33} <= ks
