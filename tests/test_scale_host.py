"""tests/scale_cases.py without a GPU: the generator, the planted-rows argument and the case table, at a few hundred rows with
"virtual" boundaries in place of 2^30 / 2^31 / 2^32 elements and row 2^24 (the generator takes its boundaries as parameters), and
the plans of the real shapes -- those are a few thousand planted rows each, never the rows themselves."""
import numpy as np
import pytest
import torch

import scale_cases as S
from oracle import topk_ref as O

DIM, N, TILE = 64, 700, 16
KS = (8, 12)


@pytest.fixture(scope="module")
def tiny():
    # boundaries: an element offset inside row 200, one at the start of row 400, the row number 520; wraps of 128 and 256 rows
    return S.make_plan(DIM, N, elem_bounds=(200 * DIM + 13, 400 * DIM), row_bounds=(520,), wraps_elems=(128 * DIM, 256 * DIM), kmax=4,
                       n_stride=60, tile=TILE)


def test_numpy_and_torch_forms_agree_element_for_element(tiny):
    for dim, rows in ((DIM, np.arange(N)), (768, np.array([0, 1, 8190, 8191, 65520, 65521, 5_596_928, (1 << 24) + 4352, (1 << 32) - 2]))):
        rows = rows.astype(np.int64)
        a = S.background(rows, dim)
        b = S.background(torch.from_numpy(rows), dim).numpy()
        assert a.dtype == np.int64 and np.array_equal(a, b)
        assert np.abs(a).max() <= S.BG and len(np.unique(a)) == 2 * S.BG + 1
    for r0, r1 in ((0, N), (190, 420), (515, 530)):
        assert np.array_equal(S.chunk_torch(tiny, r0, r1, "cpu").numpy(), S.rows_numpy(tiny, np.arange(r0, r1)))
    X = S.rows_numpy(tiny, np.arange(N))
    assert np.array_equal(O.bf16_round(X), X), "every stored value must be a bf16 number"
    assert np.array_equal(S.rows_numpy(tiny, np.array([521, 3, 200])), X[[521, 3, 200]])


def test_inequality_holds_from_the_parameters_and_in_the_data(tiny):
    for dim in (64, 768, 4096):
        worst_other, least_own = S.check_params(dim)
        assert least_own > worst_other
    with pytest.raises(AssertionError):
        S.check_params(8192)                       # 8192 * 64 * 64 > 2^24
    worst_other, least_own = S.check_params(DIM)
    X = S.rows_numpy(tiny, np.arange(N)).astype(np.float64) * 64
    Q = S.queries(DIM, 9).astype(np.float64) * 64
    score = X @ Q.T
    cls = np.full(N, -1)
    cls[tiny.ids] = [s[0] for s in tiny.spec]
    for i in range(len(Q)):
        own = cls == i % S.NC
        assert score[own, i].min() >= least_own and score[~own, i].max() <= worst_other
    assert np.abs(score).max() <= 1 << 24


@pytest.mark.parametrize("k", KS)
def test_oracle_over_all_rows_equals_oracle_over_planted_rows(tiny, k):
    X = S.rows_numpy(tiny, np.arange(N))
    for nq in (1, 5, 9):
        Q = S.queries(DIM, nq)
        rs, ri = O.dense_topk(X, Q, k)
        es, ei = S.expected(tiny, Q, k)
        assert np.array_equal(ri, ei) and np.array_equal(rs.view(np.uint32), es.view(np.uint32))
    # filters: a range with k planted rows of every class, a range scanned on the host, a single row with its -1 / -inf tail
    Q = S.queries(DIM, 5)
    lo = 100
    es, ei = S.expected(tiny, Q, k, allowed=lambda ids: (ids >= lo, False))
    rs, ri = O.dense_topk(X[lo:], Q, k)
    assert np.array_equal(ei, ri + lo) and np.array_equal(es, rs)
    es, ei = S.expected_over(tiny, np.arange(390, 410), Q, k)
    rs, ri = O.dense_topk(X[390:410], Q, k)
    assert np.array_equal(ei, ri + 390) and np.array_equal(es, rs)
    es, ei = S.expected_over(tiny, [N - 1], Q, k)
    assert (ei[:, 0] == N - 1).all() and (ei[:, 1:] == -1).all() and np.isneginf(es[:, 1:]).all()
    with pytest.raises(AssertionError):
        S.expected(tiny, Q, 64)                    # more than a class has planted: the argument does not hold, and says so


def test_sq8_inequality_and_planted_rows_argument(tiny):
    import sq8_ref as R

    for dim in (64, 768, 4096):
        worst_other, least_own = S.check_sq8_params(dim)
        assert least_own > worst_other
    worst_other, least_own = S.check_sq8_params(DIM)
    X = S.rows_numpy(tiny, np.arange(N))
    Q = S.queries(DIM, 9)
    score = R.scores(*R.quantize(Q), *R.quantize(X)).astype(np.float64) * 4096      # [nq, n] in grid units
    cls = np.full(N, -1)
    cls[tiny.ids] = [s[0] for s in tiny.spec]
    for i in range(len(Q)):
        own = cls == i % S.NC
        assert score[i, own].min() >= least_own * (1 - 2.0 ** -20) and score[i, ~own].max() <= worst_other * (1 + 2.0 ** -20)
    for k in KS:
        rs, ri = R.search(X, Q, k)
        es, ei = S.expected_sq8(tiny, Q, k)
        assert np.array_equal(ri, ei) and np.array_equal(rs.view(np.uint32), es.view(np.uint32))
        lo = 100
        rs, ri = R.search(X, Q, k, passing=np.arange(lo, N))
        es, ei = S.expected_sq8(tiny, Q, k, allowed=lambda ids: (ids >= lo, False))
        assert np.array_equal(ri, ei) and np.array_equal(rs.view(np.uint32), es.view(np.uint32))


def test_edge_alias_and_tie_conditions(tiny):
    assert tiny.bounds == [200, 400, 520] and tiny.wraps == [128, 256]
    S.check_plan(tiny, KS)
    edges = set(S.edge_rows(tiny).tolist())
    assert {198, 199, 200, 201, 202, 183, 215, 688, 699} <= edges
    spec = dict(zip(tiny.ids.tolist(), tiny.spec))
    X = S.rows_numpy(tiny, np.arange(N))
    for b in tiny.bounds:                           # equal rows, hence equal scores, on opposite sides of every boundary
        blk = slice(spec[b - 1][0] * DIM // S.NC, (spec[b - 1][0] + 1) * DIM // S.NC)
        assert spec[b - 1] == spec[b + 1] and np.array_equal(X[b - 1, blk], X[b + 1, blk])
        q = S.queries(DIM, 2 * S.NC)[spec[b - 1][0]::S.NC]
        assert np.array_equal(q @ X[b - 1], q @ X[b + 1])
    for r in edges:                                 # what a wrapped offset would read scores differently for the row's class
        q = S.queries(DIM, S.NC)[spec[r][0]]
        for w in tiny.wraps:
            for a in (r - w, r + w):
                if 0 <= a < N:
                    assert X[a] @ q != X[r] @ q
    assert 200 - 128 not in spec                    # (the alias of row 200 is background; a plan that plants row 200's spec there is refused)
    ids = np.sort(np.append(tiny.ids, 200 - 128))
    at = int(np.searchsorted(ids, 200 - 128))
    broken = tiny._replace(ids=ids, spec=tiny.spec[:at] + [spec[200]] + tiny.spec[at:], kind=tiny.kind[:at] + ["stride"] + tiny.kind[at:])
    with pytest.raises(AssertionError):
        S.check_plan(broken, KS)


@pytest.mark.parametrize("name", list(S.FAMILIES))
def test_family_shapes_are_the_smallest_that_cross(name):
    f = S.FAMILIES[name]
    device_rows = f.n - S.HOST_TAIL
    assert device_rows % 256 == 0 and 0 < f.n < (1 << 32) - 1
    for what, crosses in f.claims:
        assert crosses(device_rows), f"family {name} does not cross {what}"
        assert not crosses(device_rows - 256), f"family {name} is not the smallest shape that crosses {what}"
    for e in f.elem_bounds:
        assert e <= device_rows * f.dim, "the host add's staging offset lies at or beyond the last boundary"
    if name == "C":
        assert device_rows >= 1 << 24 and -(-f.n // S.FILTER_BLOCK) == 513


@pytest.mark.parametrize("name", list(S.FAMILIES))
def test_family_plans_meet_their_conditions(name):
    plan = S.family_plan(name)
    f = S.FAMILIES[name]
    ks = sorted({c.k for c in S.CASES + S.NO_TILED_CASES if c.family == name})
    S.check_plan(plan, ks)
    assert len(plan.ids) < 4000, "a few thousand planted rows"
    per_class = np.bincount([s[0] for s in plan.spec], minlength=S.NC)
    assert per_class.max() < 2048 and per_class.min() >= max(ks), "every class fits a candidate buffer of the tiled search and fills the longest list"
    floor = [r for r, s, what in zip(plan.ids, plan.spec, plan.kind) if what == "floor"]
    assert len(floor) >= S.NC * 64 - 3 and max(floor) < 256
    assert len(plan.bounds) == {"A": 3, "B": 3, "C": 2}[name]
    for e in f.elem_bounds:
        assert e // f.dim in plan.bounds
    if name == "C":                                 # the filters of the table, against what the argument needs
        edge = 256 * S.FILTER_BLOCK
        assert S.filter_rows(plan, "straddle_255_256")[0] // S.FILTER_BLOCK == 254 and (S.filter_rows(plan, "straddle_255_256")[1] - 1) // S.FILTER_BLOCK == 257
        S.expected(plan, S.queries(64, 3), 10, allowed=lambda ids: (ids >= edge, False))


def test_case_table():
    for table in (S.CASES, S.NO_TILED_CASES):
        ids = [S.case_id(c) for c in table]
        assert len(set(ids)) == len(ids)
    assert S.shard_order(S.CASES) == [(f, d) for f in "ABC" for d in ("bf16", "f32", "f32+image", "sq8") if (f, d) not in (("A", "f32+image"), ("A", "sq8"), ("C", "sq8"))]
    for c in S.CASES + S.NO_TILED_CASES:
        assert 1 <= c.k <= 64 and c.nq >= 1 and (c.expect is None) == (c.dtype == "sq8") == c.api.startswith("sq8")
        if c.api in ("base", "map"):
            assert c.k <= 64
        if c.api == "filtered" and c.arg != "all":
            assert c.family == "C"
    for f in "ABC":                                  # one device-resident search with an id base and one with a row map per family
        assert {c.api for c in S.CASES if c.family == f} >= {"host", "base", "map", "filtered"}
    assert S.shard_bytes(768, S.FAMILIES["B"].n, "f32+image") < 32e9
