"""The numpy reference of the deep lists (tests/deep_ref.py) against the brute-force definition (rank_ref.ranks: the
column at position c has rank c + 1), and the facts the planted corpora of tests/test_search_deep.py are named after."""
import numpy as np

from tests import deep_ref as dr
from tests import rank_ref as rr


def _all_targets(nq, n):
    return rr.targets_csr([list(range(n))] * nq)


def test_topk_rows_against_the_rank_definition():
    rng = np.random.default_rng(5)
    S = rng.integers(0, 6, size=(7, 40)).astype(np.int64)     # few values: ties everywhere, zeros included
    S[3] = 0                                                    # a row without a member
    S[4] = 4                                                    # one tie class over the whole row
    S[5, 7] = 2 ** 32 - 1                                       # the top of the key range
    S[5, 9] = 2 ** 31
    ranks, _ = rr.ranks(S, *_all_targets(7, 40))
    ranks = ranks.reshape(7, 40)
    for k in (1, 5, 39, 40, 41, 100):
        idx, key, n_hit = dr.topk_rows(S, k)
        assert idx.dtype == np.uint32 and key.dtype == np.uint32 and n_hit.dtype == np.int32
        for i in range(7):
            hits = int(np.count_nonzero(S[i]))
            assert n_hit[i] == min(k, hits)
            for c in range(k):
                if c < n_hit[i]:
                    assert ranks[i, idx[i, c]] == c + 1 and key[i, c] == S[i, idx[i, c]]
                else:
                    assert idx[i, c] == dr.NO_COL and key[i, c] == 0
    # the dense route's rule: every column is a member, key 0 included
    idx, key, n_hit = dr.topk_rows(S[3:4], 10, skip_zero=False)
    assert n_hit[0] == 10 and idx[0].tolist() == list(range(10))


def test_tie_class():
    assert dr.tie_class([5, 3, 3, 0, 3, 1], 2) == (3, 3, 1)
    assert dr.tie_class([5, 3, 3, 0, 3, 1], 4) == (3, 3, 3)
    assert dr.tie_class([5, 3, 3, 0, 3, 1], 5) == (0, 0, 0)    # five members: nothing is cut


def test_planted_corpora_hold_what_the_gpu_tests_claim():
    from tests import test_search_deep as t

    n, tile = t.N1, t.T1
    # ties: the cut falls inside the weight-3 class, first in tile 0, then past the first tile edge
    S = rr.scores(*rr.csr([[(0, 2)]]), dr.two_weight_corpus(n), False)[0]
    assert dr.tie_class(S, 4000) == (6, n - (n + 2) // 3, 4000 - (n + 2) // 3)
    assert dr.tie_class(S, 6000) == (6, n - (n + 2) // 3, 6000 - (n + 2) // 3)
    idx, _, _ = dr.topk_rows(S[None, :], 6000)
    assert idx[0, 3999] < tile <= idx[0, 5999]
    # one class over the whole row, cut at both tested k
    S = rr.scores(*rr.csr([[(0, 4)]]), dr.flat_corpus(n), False)[0]
    for k in (1025, n - 1):
        assert dr.tie_class(S, k) == (28, n, k)
    # under the df == N filter the one-term query of those corpora keeps nothing: the tests search with the filter off
    assert not rr.scores(*rr.csr([[(0, 4)]]), dr.flat_corpus(n), True).any()
    # bit 31: every hit in [2^31, 2^32), more hits than k, the term kept under the filter
    S = rr.scores(*rr.csr([[(0, 40000)]]), dr.bit31_corpus(n), True)[0]
    assert np.count_nonzero(S) == n - 1 > 2000 and S[S > 0].min() >= 2 ** 31 and S.max() < 2 ** 32
    assert (S.astype(np.float32).astype(np.int64) != S).any()   # the f32 image rounds
    # case 1: hits on both sides of the tested k; the tile-0 query and the query without a kept term
    D, light, general = t.case1_data()
    for rows in (light, general):
        for drop in (True, False):
            hits = np.count_nonzero(rr.scores(*rr.csr(rows), D, drop), axis=1)
            assert hits.max() > 3000 or rows is light
            assert drop or hits.max() == n
    hits = np.count_nonzero(rr.scores(*rr.csr(light), D, True), axis=1)
    assert 0 < hits[64] < 1024 and hits[65] == 0 and hits[:64].max() > 1025
    # case 2: more hits than MSR_DEEP_KMAX in every query
    D2, rows2 = t.case2_data()
    assert (np.count_nonzero(rr.scores(*rr.csr(rows2), D2, False), axis=1) == t.N2).all() and t.N2 > 16384
