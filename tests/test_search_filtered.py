"""msr_search_filtered on the GPU against numpy (S = Q @ D.T from tests/rank_ref.py, the masked top-k of
tests/filter_ref.py): exact equality of every ordinal, u32 score, f32 score and hit count on the smallest shapes at which
score_tiles_filtered (csrc/msr_filter.hpp) and its host path can go wrong — three ragged tiles with sets that are empty,
full, one doc, one whole tile (early exit on both sides), off the 4- and 32-doc grid, dense and garbage-tailed, at every k
at which another instance or selection path is taken; every tile size with and without a dense head; the staged route
with a live threshold, a dead one and a second stage that only exits early — and the identities with msr_search_csr and
msr_search_deep, and the searcher."""
import numpy as np
import pytest

from tests import accum_ref as ar
from tests import deep_ref as dr
from tests import filter_ref as fr
from tests import rank_ref as rr

pytestmark = pytest.mark.gpu

KS = [1, 10, 64, 65, 512, 513, 1024]
DROPS = pytest.mark.parametrize("drop", [True, False], ids=["drop_df_eq_n", "keep_df_eq_n"])
PATHS = pytest.mark.parametrize("path", ["light", "general"])


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


def compare(got, want):
    """The four arrays of a filtered call against (cols, keys, n_hit) of the reference, padding included."""
    o, f, u, n = got
    want_o, want_s, want_n = want
    assert o.dtype == np.uint32 and u.dtype == np.uint32 and f.dtype == np.float32 and n.dtype == np.int32
    assert o.shape == u.shape == f.shape == want_o.shape
    assert (n == want_n).all(), np.flatnonzero(n != want_n)[:8]
    assert (u == want_s).all(), np.argwhere(u != want_s)[:8]
    assert (o == want_o).all(), np.argwhere(o != want_o)[:8]
    assert (f == want_s.astype(np.float32)).all()


# --------------------------------------------------------------------------------------- A. three ragged tiles
NA, TA, VA = 2 * 4096 + 37, 4096, 300


@pytest.fixture(scope="module")
def case_a(m, tmp_path_factory):
    D = rr.random_corpus(NA, VA, 24, seed=1)
    rows = dict(light=rr.random_queries(64, 8, VA, seed=2), general=rr.random_queries(48, 90, VA, seed=3))
    ix = rr.open_index(m, tmp_path_factory.mktemp("filt_a") / "a.idx", D, TA)
    assert ix.n_tiles == 3
    S = {(p, d): rr.scores(*rr.csr(r), D, d) for p, r in rows.items() for d in (True, False)}
    member, words = fr.named_sets(NA, TA)
    refs = {}

    def ref(path, drop, q_set, sets=member):
        """The reference at k = 1024, computed once per (batch, flag, assignment) and cut to the k of a test."""
        key = (path, drop, None if q_set is None else tuple(q_set), sets.shape[0])
        if key not in refs:
            refs[key] = fr.masked_topk(S[(path, drop)], sets, q_set, 1024)
        return refs[key]

    yield dict(ix=ix, D=D, rows=rows, S=S, member=member, words=words, ref=ref)
    ix.close()


def mixed_q_set(nq):
    """Every set and -1 across the queries of one call; 9 choices against 64 / 48 queries: every choice occurs >= 5 times."""
    return ((np.arange(nq) * 4) % 9 - 1).astype(np.int32)


@pytest.mark.parametrize("k", KS)
@DROPS
@PATHS
def test_one_call_mixes_all_sets(case_a, path, drop, k):
    c = case_a
    rows = c["rows"][path]
    q_set = mixed_q_set(len(rows))
    assert set(q_set.tolist()) == set(range(-1, 8))
    got = c["ix"].search_filtered(*rr.csr(rows), k, c["words"], q_set, drop_df_eq_n=drop)
    want = fr.cut(c["ref"](path, drop, q_set), k)
    compare(got, want)
    assert (got[3][q_set == 0] == 0).all()                                   # the empty set
    if k == 1024 and path == "light":                                        # rows with hundreds of hits, but fewer than k
        assert ((want[2] > 500) & (want[2] < k)).any()


@pytest.mark.parametrize("s", range(8), ids=fr.SET_NAMES)
@DROPS
@PATHS
def test_every_query_on_one_set(case_a, path, drop, s):
    """Every query of the batch on set s, at the smallest and the largest k and across the 512 / 513 instance change; the
    even and random sets cut tie classes inside rows (the k-th place falls among equal scores: the lower ordinals stay)."""
    c = case_a
    rows = c["rows"][path]
    q_set = np.full(len(rows), s, dtype=np.int32)
    ref = c["ref"](path, drop, q_set)
    for k in (10, 512, 513, 1024):
        compare(c["ix"].search_filtered(*rr.csr(rows), k, c["words"], q_set, drop_df_eq_n=drop), fr.cut(ref, k))
    name = fr.SET_NAMES[s]
    if name in ("even", "random"):
        mask = fr.mask_rows(c["member"], q_set, len(rows))
        cuts = {k: len(fr.cut_rows(c["S"][(path, drop)], mask, k)) for k in (10, 1024)}
        assert cuts[1024] >= 1, cuts                                         # (light: 22-24 rows, general: 1-3)
        if path == "light":
            assert cuts[10] >= 1, cuts                                       # (2-8 rows)
            assert np.count_nonzero(c["S"][(path, drop)] * mask, axis=1).min() < 1024   # rows with fewer hits than k
    if name in ("last", "tile1"):
        assert (ref[2] <= c["member"][s].sum()).all()


@DROPS
@PATHS
def test_q_set_null(case_a, path, drop):
    c = case_a
    q = rr.csr(c["rows"][path])
    nq = len(c["rows"][path])
    for k in (10, 1024):
        # n_sets = 0: nothing is filtered
        compare(c["ix"].search_filtered(*q, k, c["words"][:0], None, drop_df_eq_n=drop),
                fr.cut(c["ref"](path, drop, np.full(nq, -1)), k))
        # n_sets = 1: every query uses set 0 (here: the random set)
        compare(c["ix"].search_filtered(*q, k, c["words"][6:7], None, drop_df_eq_n=drop),
                fr.cut(c["ref"](path, drop, np.full(nq, 6)), k))
        compare(c["ix"].search_filtered(*q, k, c["member"][6:7], None, drop_df_eq_n=drop),   # ... given as a bool matrix
                fr.cut(c["ref"](path, drop, np.full(nq, 6)), k))


# --------------------------------------------------------------------------------------- B. every tile size
@pytest.mark.parametrize("dense_max_terms", [16, 0], ids=["dense_head", "no_dense_head"])
@pytest.mark.parametrize("tile_docs", ar.TILE_SIZES)
def test_every_tile_size(m, tmp_path, tile_docs, dense_max_terms):
    n = tile_docs + 37
    D = rr.random_corpus(n, 96, 24, seed=tile_docs)
    batches = dict(light=rr.random_queries(8, 8, 96, seed=7), general=rr.random_queries(4, 90, 96, seed=8))
    o = np.arange(n)
    member = np.stack([np.random.default_rng(tile_docs).random(n) < 0.5, (o >= 5) & (o < tile_docs + 3)])
    with rr.open_index(m, tmp_path / "t.idx", D, tile_docs, dense_max_terms=dense_max_terms) as ix:
        assert ix.n_tiles == 2 and (ix.n_dense > 0) == (dense_max_terms > 0)
        for rows in batches.values():
            S = rr.scores(*rr.csr(rows), D, True)
            q_set = (np.arange(len(rows)) % 2).astype(np.int32)
            for qs in (q_set, 1 - q_set):
                ref = fr.masked_topk(S, member, qs, 1000)
                for k in (10, 1000):
                    compare(ix.search_filtered(*rr.csr(rows), k, member, qs), fr.cut(ref, k))


# --------------------------------------------------------------------------------------- C. the staged route
NC, TC = 16 * 4096 + 5, 4096          # 17 tiles x 256 queries = 4352 pairs >= kMinStagedPairs (4096): stage 1 = tile 0


@pytest.fixture(scope="module", params=["light", "general"])
def case_c(m, tmp_path_factory, request):
    if request.param == "light":
        D = rr.random_corpus(NC, 64, 12, seed=5)
        rows = rr.random_queries(256, 8, 64, seed=15)
    else:                              # a wider vocabulary: more than 64 sparse terms per query (the general scorer)
        D = rr.random_corpus(NC, 200, 12, seed=6)
        rows = rr.random_queries(256, 90, 200, seed=16)
    ix = rr.open_index(m, tmp_path_factory.mktemp("filt_c") / "c.idx", D, TC)
    assert ix.n_tiles == 17 and ix.n_tiles * len(rows) >= 4096
    Q = rr.query_matrix(*rr.csr(rows), D, True)
    S = (Q.astype(np.float64) @ D.T.astype(np.float64)).astype(np.int64)     # rr.scores through BLAS: every value < 2^53
    if request.param == "general":
        assert (np.count_nonzero(Q[:, 5:], axis=1) > 64).all()               # (terms 0 .. 4 may sit in the dense head)
    o = np.arange(NC)
    member = np.stack([np.random.default_rng(25).random(NC) < 0.5, o >= TC, o < TC])
    yield dict(ix=ix, rows=rows, S=S, member=member, kind=request.param)
    ix.close()


@pytest.mark.parametrize("s", range(3), ids=["random", "no_doc_of_tile0", "tile0_only"])
def test_staged_route(case_c, s):
    """random: every query has >= 10 member hits in tile 0, so at k = 10 stage 1 hands every query a threshold;
    no_doc_of_tile0: stage 1 yields nothing and theta stays 0; tile0_only: every stage-2 workgroup exits early."""
    c = case_c
    q_set = np.full(len(c["rows"]), s, dtype=np.int32)
    if s == 0:
        assert (np.count_nonzero(c["S"][:, :TC] * c["member"][0, :TC], axis=1) >= 10).all()
    ref = fr.masked_topk(c["S"], c["member"], q_set, 1000)
    for k in (10, 1000):
        compare(c["ix"].search_filtered(*rr.csr(c["rows"]), k, c["member"], q_set), fr.cut(ref, k))


def test_staged_route_mixed(case_c):
    c = case_c
    q_set = (np.arange(len(c["rows"])) % 4 - 1).astype(np.int32)
    ref = fr.masked_topk(c["S"], c["member"], q_set, 1000)
    for k in (10, 1000):
        compare(c["ix"].search_filtered(*rr.csr(c["rows"]), k, c["member"], q_set), fr.cut(ref, k))


def test_staged_route_full_set_is_the_unfiltered_search(case_c):
    """One full set at the shape where stage 1, its merge and the theta launch all run: msr_search_filtered and
    msr_search_csr go through the one staged routine (staged_search, csrc/msr_device.hip) with another scorer each, and
    return bit-equal arrays, which are the reference's."""
    c = case_c
    q = rr.csr(c["rows"])
    full = np.ones((1, NC), dtype=bool)
    ref = fr.masked_topk(c["S"], full, None, 1000)
    for k in (10, 1000):
        got = c["ix"].search_filtered(*q, k, full, None)
        compare(got, fr.cut(ref, k))
        for a, b in zip(got, c["ix"].search_csr(*q, k)):                      # bit-equal, padding included
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


# --------------------------------------------------------------------------------------- identities
@PATHS
def test_full_set_is_the_unfiltered_search(case_a, path):
    c, ix = case_a, case_a["ix"]
    q = rr.csr(c["rows"][path])
    nq = len(c["rows"][path])
    for k in (10, 513, 1024):
        plain = ix.search_csr(*q, k)
        for sets, q_set in ((c["words"], np.full(nq, 1)), (c["words"], np.full(nq, 7)), (c["words"], np.full(nq, -1)),
                            (c["words"][1:2], None), (c["words"][:0], None)):
            for a, b in zip(ix.search_filtered(*q, k, sets, q_set), plain):   # bit-equal, padding included
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


@PATHS
def test_struck_out_deep_list_and_partition(case_a, path):
    c, ix = case_a, case_a["ix"]
    q = rr.csr(c["rows"][path])
    nq = len(c["rows"][path])
    deep_o, deep_f, deep_u, deep_n = ix.search_deep(*q, NA)                   # the unfiltered exact ranking: every hit
    k = 1024
    for s in (4, 5, 6):                                                       # even, span, random
        both = np.stack([c["member"][s], ~c["member"][s]])
        lists = [ix.search_filtered(*q, k, both, np.full(nq, side, np.int32)) for side in (0, 1)]
        for side, (o, f, u, n) in enumerate(lists):
            for i in range(nq):
                hits = deep_o[i, :deep_n[i]]
                keep = both[side][hits]
                want = hits[keep][:k]
                assert n[i] == len(want) and (o[i, :n[i]] == want).all()
                assert (u[i, :n[i]] == deep_u[i, :deep_n[i]][keep][:k]).all()
                assert (f[i, :n[i]] == deep_f[i, :deep_n[i]][keep][:k]).all()
        # a set and its complement partition the unfiltered hits (rows with at most k hits on each side: all of them)
        whole = [i for i in range(nq) if lists[0][3][i] < k and lists[1][3][i] < k]
        assert whole or path == "general"
        for i in whole:
            a, b = lists[0][0][i, :lists[0][3][i]], lists[1][0][i, :lists[1][3][i]]
            assert len(a) + len(b) == deep_n[i] and not set(a.tolist()) & set(b.tolist())
            assert set(a.tolist()) | set(b.tolist()) == set(deep_o[i, :deep_n[i]].tolist())


def test_ms_and_empty_calls(case_a):
    c = case_a
    q = rr.csr(c["rows"]["light"])
    q_set = mixed_q_set(64)
    for k in (10, 1000):
        *_, ms = c["ix"].search_filtered(*q, k, c["words"], q_set, with_ms=True)
        assert len(ms) == 2 and ms[0] > 0 and ms[1] > 0
    o, f, u, n = c["ix"].search_filtered(np.zeros(1, np.int64), [], [], 10, c["words"], np.zeros(0, np.int32))   # nq == 0
    assert o.shape == (0, 10) and len(n) == 0


def test_refusals_of_the_normalisation(case_a, m):
    """The CSR arrays are checked with the normalisation, as by msr_search_csr: the same codes."""
    c = case_a
    for rows, code in (([[(VA, 1)]], -8), ([[(1, 1 << 24)]], -8), ([[(5, 0xFFFFFF)] * 300], -7)):
        with pytest.raises(m._cabi.MsrError) as e:
            c["ix"].search_filtered(*rr.csr(rows), 10, c["words"], [4])
        with pytest.raises(m._cabi.MsrError) as e2:
            c["ix"].search_csr(*rr.csr(rows), 10)
        assert e.value.code == e2.value.code == code


# --------------------------------------------------------------------------------------- the searcher
def test_searcher_batch_search_filtered(case_a, m):
    from mllm_sparse_retrieval_amd.searcher import LuceneImpactSearcher

    c, k = case_a, 50
    rows = c["rows"]["light"][:12]
    texts = [" ".join(" ".join([str(t) if t >= 0 else "oov"] * w) for t, w in r if w > 0) for r in rows]
    qids = ["q%d" % i for i in range(len(texts))]
    qids[7] = qids[2]                                                        # a duplicate qid: the later query's list stays
    ids = rr.doc_ids(NA)
    doc_sets = {"even": [ids[j] for j in np.flatnonzero(c["member"][4])],
                "span": [ids[j] for j in np.flatnonzero(c["member"][5])][::-1],   # any order
                "none": []}
    col = {"even": 4, "span": 5, "none": 0, None: -1}
    # a set per qid; q3, q11: no entry = unfiltered
    query_set = {"q%d" % i: name for i, name in enumerate(["even", "span", "none", None] * 3) if name is not None}
    q_set = np.array([col[query_set.get(qid)] for qid in qids])
    assert set(q_set.tolist()) == {4, 5, 0, -1}
    want_o, want_s, want_n = fr.masked_topk(c["S"][("light", True)][:12], c["member"], q_set, k)
    s = LuceneImpactSearcher(c["ix"].path, None)
    try:
        got = s.batch_search_filtered(texts, qids, k, doc_sets, query_set)
        with pytest.raises(ValueError):
            s.batch_search_filtered(texts, qids, k, {"even": ["no such doc"]}, {})
        with pytest.raises(ValueError):
            s.batch_search_filtered(texts, qids, k, doc_sets, {qids[0]: "no such set"})
        plain = s.batch_search(texts, qids, k)
        unfiltered = s.batch_search_filtered(texts, qids, k, doc_sets, {})
    finally:
        s.close()
    assert set(got) == set(qids) and len(got) == 11
    for qid in set(qids):
        i = max(j for j, x in enumerate(qids) if x == qid)                   # duplicate qids collapse onto the last query
        cnt = int(want_n[i])
        assert [h.docid for h in got[qid]] == [ids[j] for j in want_o[i, :cnt]], qid
        assert [h.score for h in got[qid]] == want_s[i, :cnt].astype(np.float32).tolist()
    assert got["q10"] == [] and len(got["q3"]) == k                          # the empty set; no entry = unfiltered
    for qid in qids:
        assert [(h.docid, h.score) for h in unfiltered[qid]] == [(h.docid, h.score) for h in plain[qid]]
