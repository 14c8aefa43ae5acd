"""msr_search_deep on the GPU against numpy (S = Q @ D.T from tests/rank_ref.py, the top-k by np.lexsort from
tests/deep_ref.py): exact equality of every ordinal, u32 score, f32 score and hit count, on the smallest shapes that
reach each way deep_select_rows (csrc/msr_deep_select.hpp) and its sparse producer can go wrong — ragged tiles, every k
at which another instance or shortcut is taken, more hits than MSR_DEEP_KMAX, every tile size with and without a dense
head, tie classes cut inside a row and covering the whole row, scores with bit 31 set, two query passes — and against
the staged search, msr_rank_docs and the searcher."""
import numpy as np
import pytest

from tests import accum_ref as ar
from tests import deep_ref as dr
from tests import rank_ref as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


def check(ix, S, rows, k, drop):
    """One deep call against the reference of the score matrix S; returns the four arrays."""
    want_o, want_s, want_n = dr.topk_rows(S, k)
    o, f, u, n = ix.search_deep(*rr.csr(rows), k, drop_df_eq_n=drop)
    assert o.dtype == np.uint32 and u.dtype == np.uint32 and f.dtype == np.float32 and n.dtype == np.int32
    assert o.shape == u.shape == f.shape == (len(rows), k)
    assert (n == want_n).all(), np.flatnonzero(n != want_n)[:8]
    assert (u == want_s).all(), np.argwhere(u != want_s)[:8]
    assert (o == want_o).all(), np.argwhere(o != want_o)[:8]
    assert (f == want_s.astype(np.float32)).all()
    return o, f, u, n


# ------------------------------------------------------------------------------------- 1. random, three tiles, ragged
N1, T1, V1 = 2 * 4096 + 37, 4096, 300
K1 = [1, 1024, 1025, 3000, N1, 16384]


def case1_data():
    D = rr.random_corpus(N1, V1, 24, seed=1)
    D[T1:, V1 - 1] = 0     # the last term has postings in tile 0 only
    # + a query whose only term lives in tile 0 (hits < k) and one without a kept term (df == N, OOV, zero weight)
    light = rr.random_queries(64, 8, V1, seed=2) + [[(V1 - 1, 3)], [(0, 5), (-1, 2), (7, 0)]]
    general = rr.random_queries(48, 90, V1, seed=3)
    return D, light, general


@pytest.fixture(scope="module")
def case1(m, tmp_path_factory):
    D, light, general = case1_data()
    ix = rr.open_index(m, tmp_path_factory.mktemp("deep1") / "c1.idx", D, T1)
    assert ix.n_tiles == 3
    S = {(p, d): rr.scores(*rr.csr(rows), D, d) for p, rows in (("light", light), ("general", general)) for d in (True, False)}
    yield dict(ix=ix, D=D, light=light, general=general, S=S)
    ix.close()


@pytest.mark.parametrize("k", K1)
@pytest.mark.parametrize("drop", [True, False], ids=["drop_df_eq_n", "keep_df_eq_n"])
@pytest.mark.parametrize("path", ["light", "general"])
def test_random_three_ragged_tiles(case1, path, drop, k):
    c = case1
    o, f, u, n = check(c["ix"], c["S"][(path, drop)], c[path], k, drop)
    if path == "light":
        hits = np.count_nonzero(c["S"][(path, drop)][64])
        assert 0 < hits < 1024 and n[64] == min(k, hits)      # the tile-0 query: fewer hits than a deep k
        assert n[65] == (0 if drop else min(k, N1))           # nothing kept under the filter; term 0 alone without it
        assert drop is False or ((o[65] == dr.NO_COL).all() and (u[65] == 0).all() and (f[65] == 0).all())


def test_ms_and_empty_calls(case1):
    c = case1
    q = rr.csr(c["light"])
    *_, ms = c["ix"].search_deep(*q, 2000, with_ms=True)
    assert ms[0] > 0 and ms[1] > 0
    o, f, u, n = c["ix"].search_deep(np.zeros(1, np.int64), [], [], 2000)   # nq == 0
    assert o.shape == (0, 2000) and len(n) == 0


# --------------------------------------------------------------------------- 2. k = MSR_DEEP_KMAX with more hits than k
N2 = 5 * 4096 + 37


def case2_data():
    D = rr.random_corpus(N2, V1, 24, seed=2)
    rows = [r + [(0, 3)] for r in rr.random_queries(16, 8, V1, seed=12)]    # term 0 (in every doc) in every query
    return D, rows


@pytest.fixture(scope="module")
def case2(m, tmp_path_factory):
    D, rows = case2_data()
    ix = rr.open_index(m, tmp_path_factory.mktemp("deep2") / "c2.idx", D, T1)
    assert ix.n_tiles == 6
    yield dict(ix=ix, D=D, rows=rows)
    ix.close()


def test_more_hits_than_kmax(case2, m):
    c = case2
    kmax = m._cabi.MSR_DEEP_KMAX
    S = rr.scores(*rr.csr(c["rows"]), c["D"], False)
    o, f, u, n = check(c["ix"], S, c["rows"], kmax, False)
    assert (n == kmax).all() and (np.count_nonzero(S, axis=1) > kmax).all()


# ------------------------------------------------------------------------------------------------ 3. every tile size
@pytest.mark.parametrize("dense_max_terms", [16, 0], ids=["dense_head", "no_dense_head"])
@pytest.mark.parametrize("tile_docs", ar.TILE_SIZES)
def test_every_tile_size(m, tmp_path, tile_docs, dense_max_terms):
    n = tile_docs + 37
    D = rr.random_corpus(n, 96, 24, seed=tile_docs)
    rows = rr.random_queries(8, 8, 96, seed=7) + rr.random_queries(4, 90, 96, seed=8)
    with rr.open_index(m, tmp_path / "t.idx", D, tile_docs, dense_max_terms=dense_max_terms) as ix:
        assert ix.n_tiles == 2 and (ix.n_dense > 0) == (dense_max_terms > 0)
        S = rr.scores(*rr.csr(rows), D, True)
        for k in (1500, 16384):
            check(ix, S, rows, k, True)


# ------------------------------------------------------------------------------------------------ 4. ties
def test_tie_class_cut_inside_the_row(m, tmp_path):
    D = dr.two_weight_corpus(N1)
    rows = [[(0, 2)]]
    S = rr.scores(*rr.csr(rows), D, False)
    with rr.open_index(m, tmp_path / "w.idx", D, T1) as ix:
        for k in (4000, 6000):     # the cut falls inside the weight-3 class: in tile 0, and past the first tile edge
            theta, cls, taken = dr.tie_class(S[0], k)
            assert theta == 6 and 0 < taken < cls
            o, *_ = check(ix, S, rows, k, False)
            assert (o[0, k - 1] >= T1) == (k == 6000)


def test_whole_row_is_one_tie_class(m, tmp_path):
    D = dr.flat_corpus(N1)
    rows = [[(0, 4)], [(0, 1)]]
    S = rr.scores(*rr.csr(rows), D, False)
    with rr.open_index(m, tmp_path / "f.idx", D, T1) as ix:
        for k in (1025, N1 - 1):
            o, *_ = check(ix, S, rows, k, False)
            assert (o == np.arange(k, dtype=np.uint32)[None, :]).all()


# ------------------------------------------------------------------------------------------------ 5. bit 31
def test_scores_with_bit_31(m, tmp_path):
    D = dr.bit31_corpus(N1)
    rows = [[(0, 40000)]]
    S = rr.scores(*rr.csr(rows), D, True)
    assert (S[0, :-1] >= 2 ** 31).all() and S.max() < 2 ** 32
    with rr.open_index(m, tmp_path / "b.idx", D, T1) as ix:
        o, f, u, n = check(ix, S, rows, 2000, True)
        assert (u >= 2 ** 31).all() and (f == u.astype(np.float32)).all() and (f != u).any()   # the f32 image rounds


# ------------------------------------------------------------------------------------------------ 6. identities
@pytest.mark.parametrize("path", ["light", "general"])
def test_identities_with_search_and_rank(case1, path):
    c, ix = case1, case1["ix"]
    q = rr.csr(c[path])
    for k in (10, 1024):
        for a, b in zip(ix.search_deep(*q, k), ix.search_csr(*q, k)):
            assert a.dtype == b.dtype and (a == b).all()
    deep = ix.search_deep(*q, 3000)
    for a, b in zip(deep[:3], ix.search_csr(*q, 1024)[:3]):
        assert (a[:, :1024] == b).all()
    # 64 docs from columns >= 1024: msr_rank_docs gives column + 1
    rng = np.random.default_rng(6)
    o, _, u, n = deep
    qs = [i for i in range(len(c[path])) if n[i] > 1024][:8]
    assert len(qs) == 8
    cols = {i: rng.integers(1024, n[i], size=8) for i in qs}
    targets = [o[i, cols[i]].tolist() if i in cols else [] for i in range(len(c[path]))]
    t_ptr, t_ord = rr.targets_csr(targets)
    ranks, scores = ix.rank_docs(*q, t_ptr, t_ord)
    assert len(ranks) == 64
    assert (ranks == np.concatenate([cols[i] + 1 for i in qs])).all()
    assert (scores == np.concatenate([u[i, cols[i]] for i in qs])).all()


# ------------------------------------------------------------------------------------------------ 7. two query passes
def test_two_query_passes(case2):
    c = case2
    per_pass = (256 << 20) // (c["ix"].n_tiles * T1 * 4)
    nq, distinct = per_pass + 1, 61                                # 61 does not divide the pass: rows shift between passes
    base = rr.random_queries(distinct, 8, V1, seed=17)
    S = rr.scores(*rr.csr(base), c["D"], True)
    want_o, want_s, want_n = dr.topk_rows(S, 1025)
    pick = np.arange(nq) % distinct
    o, f, u, n = c["ix"].search_deep(*rr.csr([base[i] for i in pick]), 1025)
    assert (n == want_n[pick]).all() and (o == want_o[pick]).all() and (u == want_s[pick]).all()
    assert (f == want_s[pick].astype(np.float32)).all()


# ------------------------------------------------------------------------------------------------ 8. the searcher
def test_searcher_deep_batch_search(case1, m):
    from mllm_sparse_retrieval_amd.searcher import LuceneImpactSearcher

    c, k = case1, 3000
    texts = [" ".join(" ".join([str(t) if t >= 0 else "oov"] * w) for t, w in r if w > 0) for r in c["light"]]
    qids = ["q%d" % i for i in range(len(texts))]
    want_o, want_s, want_n = dr.topk_rows(c["S"][("light", True)], k)
    s = LuceneImpactSearcher(c["ix"].path, None, deep=True)
    try:
        got = s.batch_search(texts, qids, k)
        s.deep = False                                   # the default: depths beyond MSR_KMAX are still refused
        with pytest.raises(m._cabi.MsrError):
            s.batch_search(texts[:2], qids[:2], k)
    finally:
        s.close()
    ids = rr.doc_ids(N1)
    for i, qid in enumerate(qids):
        cnt = int(want_n[i])
        assert [h.docid for h in got[qid]] == [ids[j] for j in want_o[i, :cnt]]
        assert [h.score for h in got[qid]] == want_s[i, :cnt].astype(np.float32).tolist()
