"""tests/topk_special_cases.py proven against the oracle alone (no GPU): the scalings are exact and leave the oracle's lists
unchanged bit for bit, the tiny scores are exact denormals, the zero sets hold both signs of zero, the sparse denormal corpus has
hits and shared-term non-hits, and the worst-case rows at 2^-75 really lose their squared rounding error in fp32."""
import numpy as np
import pytest

import sq8_ref as R
import topk_special_cases as S
from oracle import topk_ref as O
from verbatim_rag_amd.distributed import merge_topk

_MIN_NORMAL = np.float32(2.0 ** -126)


def _stored(f, X):
    return O.bf16_round(X) if f.dtype == "bf16" else X


def _oracle(f, X, Q):
    return O.dense_topk(_stored(f, X), Q, f.k, blocked=f.nq >= 16)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _normal_or_zero(a):
    return bool(((np.abs(a) >= _MIN_NORMAL) | (a == 0)).all() and np.isfinite(a).all())


_FAMS = [f for f in S.DENSE if f.name != "pf-64"] + [f for f in S.DENSE if f.name == "pf-64"]


@pytest.mark.parametrize("f", _FAMS, ids=lambda f: f.name)
def test_scaled_sets_are_exact_and_rank_like_the_unscaled_set(f):
    X, Q = S.base_data(f)
    rs, ri = _oracle(f, X, Q)
    for e in S.SCALES:
        Xe, Qe = S.scaled(X, Q, e)
        assert _normal_or_zero(Xe) and _normal_or_zero(Qe), e
        back = np.float32(2.0) ** np.float32(-e)
        assert np.array_equal(_bits(Xe * back), _bits(X)) and np.array_equal(_bits(Qe / back), _bits(Q)), e
        assert np.array_equal(_bits(_stored(f, Xe) * back), _bits(_stored(f, X))), e       # the bf16 rounding scales with the rows
        s, i = _oracle(f, Xe, Qe)
        assert np.array_equal(i, ri) and np.array_equal(_bits(s), _bits(rs)), e


@pytest.mark.parametrize("f", S.DENSE, ids=lambda f: f.name)
def test_tiny_scores_are_exact_denormals(f):
    """The bound, re-derived per family: products are multiples of 2^-146, |partial sums| <= dim * 16 * 2^-146 <= 2^tiny_bound(dim)
    < 2^-126 -- at most 24 significant bits above 2^-149 even at dim 1 536, so every sum is exact in any order.  The oracle's
    chain must then equal the float64 dot product."""
    assert f.dim <= S.MAX_DIM and S.tiny_bound(f.dim) <= S.tiny_bound(S.MAX_DIM) == -131
    assert f.dim * S.TINY_G * S.TINY_G * 2.0 ** (S.TINY_X_EXP + S.TINY_Q_EXP) <= 2.0 ** S.tiny_bound(f.dim) < 2.0 ** -126
    assert S.TINY_X_EXP + S.TINY_Q_EXP >= -149 and S.tiny_bound(f.dim) - (S.TINY_X_EXP + S.TINY_Q_EXP) <= 24
    X, Q = S.tiny_data(f)
    assert np.array_equal(_stored(f, X), X) and np.array_equal(O.bf16_round(Q), Q)           # bf16 numbers: no rounding on any route
    units = X.astype(np.float64) * 2.0 ** -S.TINY_X_EXP
    assert np.array_equal(units, np.rint(units)) and np.abs(units).max() <= S.TINY_G
    exact = Q.astype(np.float64) @ X.astype(np.float64).T                                    # [nq, n], exact in float64
    assert np.abs(exact).max() < 2.0 ** -126 and np.array_equal(exact.astype(np.float32).astype(np.float64), exact)
    rs, ri = _oracle(f, X, Q)
    assert (ri >= 0).all() and np.array_equal(rs.astype(np.float64), np.take_along_axis(exact, ri, axis=1))
    assert (rs != 0).any() and (np.abs(rs[rs != 0]) < _MIN_NORMAL).all()
    if f.n > 8:    # the all-zero answer of a flushing route is a different one
        assert not np.array_equal(ri, S.flushed_answer(f.nq, f.k, f.n)[1])


@pytest.mark.parametrize("f", S.DENSE, ids=lambda f: f.name)
def test_zero_sets_hold_both_signs_and_the_negative_zero_has_the_lowest_id(f):
    X, Q = S.zeros_data(f)
    assert np.array_equal(_stored(f, X), X) and _normal_or_zero(X) and _normal_or_zero(Q)
    assert (np.signbit(X) & (X == 0)).any() and (X == 0).all(axis=1).any()
    full = O.dense_topk(X, Q, f.n, blocked=f.nq >= 16)                                       # the whole ranking
    s0, i0 = full[0][0], full[1][0]
    assert np.signbit(s0[i0 == 0])[0] and s0[i0 == 0][0] == 0, "row 0 scores -0.0 on query 0"
    zeros = s0 == 0
    assert (np.signbit(s0[zeros])).any() and (~np.signbit(s0[zeros])).any(), "both signs of zero in the oracle's list"
    assert np.array_equal(i0[zeros], np.sort(i0[zeros])) and i0[zeros][0] == 0, "zeros tie: id ascending, row 0 first"
    if f.n >= 64:
        assert (s0 > 0).sum() == S.ZERO_BIG_ROWS // 2 and (s0 < 0).sum() == S.ZERO_BIG_ROWS // 2
        assert (np.abs(s0[~zeros]) < _MIN_NORMAL).all()
    if f.nq > 1:
        assert (full[0][-1] == 0).all() and np.array_equal(full[1][-1], np.arange(f.n)), "the all-zero query: the whole shard ties"
    Xz, Qz = S.zeros_data(f, zero_queries=True)
    assert np.array_equal(Xz, X) and not Qz.any()
    rs, ri = _oracle(f, Xz, Qz)
    assert (rs == 0).all() and np.array_equal(ri, np.tile(np.arange(f.k), (f.nq, 1)))


@pytest.mark.parametrize("f", [f for f in S.DENSE if f.fallback], ids=lambda f: f.name)
def test_overflow_sets_are_finite_with_row_norms_beyond_fp32(f):
    assert S.dense_kinds(f)[-1] == S.OVERFLOW
    X, Q = S.dense_data(f, S.OVERFLOW)
    assert np.isfinite(X).all() and np.isfinite(Q).all() and Q.any(axis=1).all()
    fmax = float(np.finfo(np.float32).max)
    assert np.linalg.norm(X.astype(np.float64), axis=1).max() > fmax, "a row norm beyond fp32"
    rs, ri = _oracle(f, X, Q)
    assert np.isfinite(rs).all() and (ri >= 0).all() and (np.abs(Q.astype(np.float64) @ X.astype(np.float64).T) < 2.0 ** 40).all()


def test_families_name_each_kernel_family_once():
    names = [f.name for f in S.DENSE] + [f.name for f in S.SPARSE]
    assert len(set(names)) == len(names) and set(S.FLUSHES) <= set(names)
    logged = set().union(*(f.expect for f in S.DENSE), *(f.expect for f in S.SPARSE))
    for want in ("DENSE_BF16", "DENSE_F32", "MFMA", "MFMA2", "EXACT", "EXACT2", "PF_PREFIX", "PF_COLLECT", "PF_COLLECT_MULTI",
                 "PF_RESCORE_LIST", "PF_RESCORE", "SPARSE", "SPARSE_SCATTER", "SPARSE_MULTI", "MERGE_LISTS", "MERGE_SCAN"):
        assert any(k[0] == want for k in logged), want
    assert {k for k in logged if k[0] == "SPARSE"} == {("SPARSE", 0, 0), ("SPARSE", 1, 0)}, "both LDSQ forms"
    assert {k for k in logged if k[0] == "PF_RESCORE_LIST"} == {("PF_RESCORE_LIST", 0, 0), ("PF_RESCORE_LIST", 1, 0)}
    assert all(f.n <= 4224 for f in S.DENSE)
    assert S.filter_mask(129).sum() in (64, 65) and S.filter_mask(129)[0]


# ---------------------------------------------------------------------------------------------------------------- worst case
def test_worst_case_rows_scale_exactly_and_lose_their_squared_error_at_2_to_the_minus_75():
    X, Q, Qb, decoys, truth = S.worst_case(0)
    rs, ri = O.dense_topk(X, Q, S.WORST_K)
    rb, ib = O.dense_topk(X, Qb, S.WORST_K, blocked=True)
    assert np.array_equal(ri[0], truth)
    for e in (-75, 66):
        Xe, Qe, Qbe, _d, _t = S.worst_case(e)
        assert _normal_or_zero(Xe) and _normal_or_zero(Qe) and _normal_or_zero(Qbe)
        back = np.float32(2.0) ** np.float32(-e)
        assert np.array_equal(_bits(Xe * back), _bits(X)) and np.array_equal(_bits(Qe / back), _bits(Q))
        s, i = O.dense_topk(Xe, Qe, S.WORST_K)
        assert np.array_equal(i, ri) and np.array_equal(_bits(s), _bits(rs)), e
        s, i = O.dense_topk(Xe, Qbe, S.WORST_K, blocked=True)
        assert np.array_equal(i, ib) and np.array_equal(_bits(s), _bits(rb)), e
    # fp32 sums of squares, as an ingest that squares the elements themselves would form them
    Xe = S.worst_case(-75)[0]
    d = Xe - O.bf16_round(Xe)
    with np.errstate(under="ignore"):
        d2 = (d * d).sum(axis=1, dtype=np.float32)
    assert (d != 0).any(axis=1).all() and (d2 == 0).all(), "every row has a rounding error and its fp32 square sum is 0"
    d0 = X - O.bf16_round(X)
    assert (d0 * d0).sum(axis=1, dtype=np.float32).max() > 9e-4     # the unscaled set: what the bound needs


# ---------------------------------------------------------------------------------------------------------------- sparse
def _sparse_oracle(f, corpus, queries):
    return O.sparse_topk(*corpus, f.vocab, *queries, f.k)


@pytest.mark.parametrize("f", S.SPARSE, ids=lambda f: f.name)
def test_sparse_scaled_corpora_rank_like_the_unscaled_ones(f):
    for rows in ("grid", "gauss"):
        base = None
        for e in (0,) + S.SCALES:
            corpus, queries = S.sparse_data(f, f"{rows}{e:+d}")
            assert _normal_or_zero(corpus[2]) and (corpus[2] > 0).all() and (queries[2] > 0).all()
            got = _sparse_oracle(f, corpus, queries)
            if base is None:
                base, w0, q0 = got, corpus[2], queries[2]
                assert (got[1][:, 0] >= 0).all()
                continue
            back = np.float32(2.0) ** np.float32(-e)
            assert np.array_equal(_bits(corpus[2] * back), _bits(w0)) and np.array_equal(_bits(queries[2] / back), _bits(q0))
            assert np.array_equal(got[1], base[1]) and np.array_equal(_bits(got[0]), _bits(base[0])), (rows, e)


@pytest.mark.parametrize("f", S.SPARSE, ids=lambda f: f.name)
def test_sparse_denormal_corpus_has_hits_and_shared_term_non_hits(f):
    (indptr, idx, val), (qp, qi, qv) = S.sparse_data(f, "denorm")
    n = len(indptr) - 1
    hits = misses = 0
    for q in range(f.nq):
        qd = np.zeros(f.vocab, np.float64)
        qd[qi[qp[q]:qp[q + 1]]] = qv[qp[q]:qp[q + 1]].astype(np.float64)
        exact = np.array([(val[indptr[d]:indptr[d + 1]].astype(np.float64) * qd[idx[indptr[d]:indptr[d + 1]]]).sum() for d in range(n)])
        shares = np.array([(qd[idx[indptr[d]:indptr[d + 1]]] > 0).any() for d in range(n)])
        big = exact >= 2.0 ** -145            # shares a term of the first kind
        assert (exact[shares & ~big] < 2.0 ** -150 * 9).all() and exact.max() < 2.0 ** -136
        s, i = O.sparse_topk(indptr, idx, val, f.vocab, qp[q:q + 2] - qp[q], qi[qp[q]:qp[q + 1]], qv[qp[q]:qp[q + 1]], n)
        got = i[0][i[0] >= 0]
        assert set(got.tolist()) == set(np.nonzero(big)[0].tolist()), "the hits are exactly the documents with a denormal score"
        assert (s[0][: len(got)] > 0).all() and (s[0][: len(got)] < _MIN_NORMAL).all()
        # a hit's score: the sum of its first-kind products, exact -- the second kind adds nothing
        first = np.where(qd >= 2.0 ** (S.DENORM_HIT_EXP - 1), qd, 0.0)
        want = np.array([(val[indptr[d]:indptr[d + 1]].astype(np.float64) * first[idx[indptr[d]:indptr[d + 1]]]).sum() for d in got])
        assert np.array_equal(s[0][: len(got)].astype(np.float64), want)
        hits += len(got)
        misses += int((shares & ~big).sum())
    assert hits > 0 and misses > 0, "both classes must occur"


# ---------------------------------------------------------------------------------------------------------------- SQ8
def test_sq8_rows_cover_denormal_and_extreme_maxima_and_the_reference_is_defined_on_them():
    X, Q = S.sq8_data()
    m = np.abs(X).max(axis=1)
    assert (m[80:100] < _MIN_NORMAL).all() and (m[80:100] > 0).all() and m[:40].max() < 2.0 ** -95 and m[40:80].min() > 2.0 ** 95
    assert m[5] == 0 and m[6] == 0 and not Q[4].any()
    codes, scales = R.quantize(X)
    assert (scales[100:104] == 0).all() and (m[100:104] > 0).all() and (X[100:104] != 0).all(), "max / 127 underflows"
    assert (np.abs(codes[100:104]) == 127).all() and not codes[5].any() and not codes[6].any() and scales[5] == 0
    assert np.isfinite(scales).all() and (np.abs(codes[:80]).max(axis=1)[m[:80] > 0] == 127).all()     # (a denormal scale is coarse)
    cq, sq = R.quantize(Q)
    sc = R.scores(cq, sq, codes, scales)
    assert np.isfinite(sc).all()
    zero = sc == 0
    assert (np.signbit(sc) & zero).any() and (~np.signbit(sc) & zero).any(), "zeros of both signs among the scores"
    assert ((np.abs(sc) < _MIN_NORMAL) & ~zero).any(), "denormal scores"
    s, i = R.topk(sc, 200)
    assert np.array_equal(i[4, :200], np.arange(200)), "the all-zero query's list is id ascending"
    z = s[5] == 0
    assert z.any() and np.array_equal(i[5][z], np.sort(i[5][z])) and np.signbit(s[5][z]).any() and not np.signbit(s[5][z]).all(), "zeros of either sign tie in the reference"


# ---------------------------------------------------------------------------------------------------------------- shard merge
def test_merge_lists_mix_zero_signs_and_the_host_merge_follows_the_rule():
    scores, ids = S.merge_lists()
    live = ids >= 0
    z = live & (scores == 0)
    assert (np.signbit(scores) & z).any(axis=(1, 2)).all() and (~np.signbit(scores) & z).any(axis=(1, 2)).all(), "both signs in every shard"
    for w in range(scores.shape[0]):      # every list is sorted by the rule, ids unique across the shards
        for q in range(scores.shape[1]):
            s, i = scores[w, q][live[w, q]], ids[w, q][live[w, q]]
            assert all((s[j] > s[j + 1]) or (s[j] == s[j + 1] and i[j] < i[j + 1]) for j in range(len(s) - 1))
    for q in range(scores.shape[1]):
        assert len(set(ids[:, q][live[:, q]].tolist())) == live[:, q].sum()
    for k in (5, 8, 24, 30):
        ws, wi = S.merge_oracle(scores, ids, k)
        s, i = merge_topk(scores, ids, k)
        assert not S.compare(s, i, ws, wi, f"merge_topk k={k}")
        assert np.array_equal(np.isneginf(s), np.isneginf(ws))
    # in key order that ranks -0 below +0 the list of nothing but zeros would differ: the case can tell the two rules apart
    ws, wi = S.merge_oracle(scores, ids, 24)
    flat_s, flat_i = scores[:, 1].ravel(), ids[:, 1].ravel()
    by_sign = flat_i[np.lexsort((flat_i, np.signbit(flat_s)))]
    assert not np.array_equal(by_sign, wi[1])
